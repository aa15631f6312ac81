"""K34 (csrc/mask_paint.hip) against the host painter, bit for bit, on the full nuScenes and Argoverse 2 shapes, and the detector
on device-painted masks against the same masks loaded from PNG files."""
import os
import sys

import numpy as np
import pytest
import torch

from fullysparsefusion_amd import hip_ops
from fullysparsefusion_amd.mmdet3d_plugin.datasets import mask_paint as mp
from fullysparsefusion_amd.mmdet3d_plugin.datasets.pipelines import LoadMaskFromFiles

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_mask_paint_cpu import AV2_OBJ_MAX, AV2_SHAPES, GOLDEN, golden_dets, golden_planes, full_masks, write_files  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def np_extents(m):
    rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    if len(rows) == 0:
        return [0, 0, 0, 0]
    return [rows[0], cols[0], rows[-1] - rows[0] + 1, cols[-1] - cols[0] + 1]


def test_mask_extents_match_numpy():
    rng = np.random.default_rng(1)
    for h, w in ((900, 1600), (2, 24), (7, 48)):  # 24: 16-byte vectors that straddle rows
        m = np.zeros((9, h, w), bool)
        for k in range(1, 9):
            ys, xs = rng.integers(0, h, 3), rng.integers(0, w, 3)
            m[k, ys, xs] = True
        m[8, h - 1, w - 1] = m[8, 0, 0] = True
        got = hip_ops.mask_extents(torch.from_numpy(m).to(DEV)).cpu().numpy()
        assert np.array_equal(got, np.array([np_extents(x) for x in m])), (h, w)
        idx = torch.tensor([8, 0, 3], dtype=torch.int32, device=DEV)
        sub = hip_ops.mask_extents(torch.from_numpy(m).to(DEV), idx).cpu().numpy()
        assert np.array_equal(sub, np.array([np_extents(m[i]) for i in (8, 0, 3)]))


@pytest.mark.parametrize("form", ["device", "crops", "bbox_only"])
def test_k34_equals_host_painter_nuscenes(form):
    d = golden_dets("nusc")
    plan_host = mp.plan_masks(d, bbox_only=form == "bbox_only")
    want = mp.paint_numpy(plan_host)
    if form == "device":
        dd = {k: v for k, v in d.items() if k not in ("mask_crops", "mask_origins")}
        dd["masks"] = torch.from_numpy(np.stack(full_masks(d, [mp.NUSC_IMG] * 6))).to(DEV)
        dd["scores"] = torch.from_numpy(d["scores"]).to(DEV)  # device scores: one read-back
        plan = mp.plan_masks(dd)
    else:
        plan = plan_host
    got = mp.paint_device(plan, DEV)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (60, 900, 1600)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("form", ["device", "crops"])
def test_k34_equals_host_painter_argoverse2(form):
    d = golden_dets("av2")
    plan_host = mp.plan_masks(d, is_argo=True, img_shapes=AV2_SHAPES)
    want = mp.paint_numpy(plan_host)
    if form == "device":  # per-object 2-D device masks of two image sizes (camera 0 is portrait)
        dd = {k: v for k, v in d.items() if k not in ("mask_crops", "mask_origins")}
        dd["masks"] = [torch.from_numpy(m).to(DEV) for m in full_masks(d, AV2_SHAPES)]
        plan = mp.plan_masks(dd, is_argo=True, img_shapes=AV2_SHAPES)
    else:
        plan = plan_host
    got = mp.paint_device(plan, DEV)
    assert got.dtype == torch.int32 and tuple(got.shape) == (7, 1550, 2048) and int(got.max()) > 255
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("case", ["nusc", "nusc_bbox", "av2"])
def test_k34_pipeline_equals_the_golden_writer_output(case):
    is_argo = case == "av2"
    t = mp.PaintMasksFromDetections(class_names=mp.NAME_NUSC, is_argo=is_argo, obj_max_num=AV2_OBJ_MAX if is_argo else 250,
                                    bbox_only=case == "nusc_bbox", device=DEV)
    res = dict(mask_detections=golden_dets("av2" if is_argo else "nusc"), mask_img_shapes=AV2_SHAPES,
               lidar2img=np.eye(4, dtype=np.float32)[None].repeat(7, 0))
    got = t(res)["mask_data"].cpu()
    if is_argo:
        want = golden_planes(case, AV2_SHAPES)
        for p in range(1, 7):
            assert np.array_equal(got[p, 0].numpy(), want[p]), p
    else:
        want = golden_planes(case, [mp.NUSC_IMG] * 60)
        assert np.array_equal(got.reshape(60, 900, 1600).numpy(), np.stack(want))
    assert res["mask_anno"][:len(GOLDEN[f"{case}_anno"]), 7].tolist() == GOLDEN[f"{case}_anno"][:, 7].tolist()


def test_simple_test_on_device_painted_masks_equals_png_masks(tmp_path):
    import bench

    model = bench.build_model(DEV)
    _, inp = bench.make_inputs(1, 0, DEV)
    d = golden_dets("nusc")
    painted = mp.PaintMasksFromDetections(device=DEV)(dict(mask_detections=d))
    write_files(str(tmp_path / "frame"), "nusc", False)
    loaded = LoadMaskFromFiles(str(tmp_path))(dict(sample_idx="frame"))
    assert torch.equal(painted["mask_data"].cpu(), loaded["mask_data"])
    outs = []
    for r in (painted, loaded):
        with torch.no_grad():
            res = model.simple_test(inp["points"], inp["img_metas"], r["mask_data"].to(DEV)[None], r["mask_anno"].float().to(DEV)[None])
        outs.append(res[0])
    a, b = outs
    assert a["boxes_3d"].tensor.shape[0] > 0
    assert torch.equal(a["boxes_3d"].tensor, b["boxes_3d"].tensor)
    assert torch.equal(a["scores_3d"], b["scores_3d"]) and torch.equal(a["labels_3d"], b["labels_3d"])

