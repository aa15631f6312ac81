"""PaintMasksFromDetections on the host (K34's planner and referee painter) against the reference writers' output
(tests/golden/mask_paint.npz, made by tests/golden/make_mask_paint_golden.py) and against LoadMaskFromFiles reading those files."""
import json
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from fullysparsefusion_amd.mmdet3d_plugin.datasets import mask_paint as mp
from fullysparsefusion_amd.mmdet3d_plugin.datasets.pipelines import LoadMaskFromFiles, _resize_nearest
from fullysparsefusion_amd.mmdet3d_plugin.registry import PIPELINES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "mask_paint.npz"))
AV2_OBJ_MAX = 400


def golden_dets(prefix):
    g = GOLDEN
    shapes, bits = g[f"{prefix}_crop_shapes"], np.unpackbits(g[f"{prefix}_crop_bits"]).astype(bool)
    crops, at = [], 0
    for h, w in shapes:
        crops.append(bits[at:at + h * w].reshape(h, w))
        at += h * w
    return dict(boxes=g[f"{prefix}_boxes"], scores=g[f"{prefix}_scores"], labels=g[f"{prefix}_labels"], cams=g[f"{prefix}_cams"],
                mask_crops=crops, mask_origins=g[f"{prefix}_origins"])


def golden_planes(case, shapes):
    planes = [np.zeros(s, np.int64) for s in shapes]
    for p, y, x, n, i in GOLDEN[f"{case}_runs"]:
        planes[p][y, x:x + n] = i
    return planes


def full_masks(d, shapes):
    out = []
    for k, crop in enumerate(d["mask_crops"]):
        m = np.zeros(shapes[d["cams"][k]], bool)
        y0, x0 = d["mask_origins"][k]
        m[y0:y0 + crop.shape[0], x0:x0 + crop.shape[1]] = crop
        out.append(m)
    return out


def anno_rows(anno):
    rows = []
    for cam in anno:
        objs = [o for name in mp.NAME_NUSC for o in cam[name]] if isinstance(cam, dict) else cam
        rows += [list(o["bbox"]) + [o["score"], o["category"], o["cam_id"], o["obj_id"]] for o in objs]
    return np.asarray(rows, np.float64).reshape(-1, 8)


NUSC_SHAPES = [mp.NUSC_IMG] * 6
AV2_SHAPES = [tuple(s) for s in GOLDEN["av2_img_shapes"]]


@pytest.mark.parametrize("case,form", [("nusc", "crops"), ("nusc", "host"), ("nusc_bbox", "none")])
def test_nuscenes_planner_and_painter_equal_the_reference_writer(case, form):
    d = golden_dets("nusc")
    if form == "host":
        d["masks"] = full_masks(d, NUSC_SHAPES)
        del d["mask_crops"], d["mask_origins"]
    elif form == "none":
        del d["mask_crops"], d["mask_origins"]
    plan = mp.plan_masks(d, class_names=mp.NAME_NUSC, bbox_only=case == "nusc_bbox")  # planes in the writer's file order
    assert np.array_equal(anno_rows(plan.anno), GOLDEN[f"{case}_anno"])
    got = mp.paint_numpy(plan)
    want = golden_planes(case, [mp.NUSC_IMG] * 60)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (60, 900, 1600)
    for p in range(60):
        assert np.array_equal(got[p].numpy(), want[p]), p


def test_argoverse2_planner_and_painter_equal_the_reference_writer():
    plan = mp.plan_masks(golden_dets("av2"), is_argo=True, img_shapes=AV2_SHAPES)
    assert np.array_equal(anno_rows(plan.anno), GOLDEN["av2_anno"])
    got = mp.paint_numpy(plan)
    want = golden_planes("av2", AV2_SHAPES)
    assert got.dtype == torch.int32 and tuple(got.shape) == (7, 1550, 2048)
    assert np.array_equal(got[0].numpy(), _resize_nearest(torch.from_numpy(want[0].astype(np.int32)), (1550, 2048)).numpy())
    for p in range(1, 7):
        assert np.array_equal(got[p].numpy(), want[p]), p
    assert int(got.max()) > 255


def test_mmdet_nested_form_equals_packed_form():
    d = golden_dets("nusc")
    masks = full_masks(d, NUSC_SHAPES)
    nested = []
    for cam in range(6):
        bbox, segm = [], []
        for i in range(10):
            ks = np.flatnonzero((d["cams"] == cam) & (d["labels"] == i))
            bbox.append(np.concatenate([d["boxes"][ks], d["scores"][ks, None]], 1))
            segm.append([masks[k] for k in ks])
        nested.append((bbox, segm))
    a = PaintMasksFromDetections()(dict(mask_detections=nested))
    b = PaintMasksFromDetections()(dict(mask_detections=golden_dets("nusc")))
    assert torch.equal(a["mask_data"], b["mask_data"]) and torch.equal(a["mask_anno"], b["mask_anno"])


PaintMasksFromDetections = mp.PaintMasksFromDetections


def write_files(tmp, case, is_argo):
    """The golden outputs as the writer stores them: PNG planes (8-bit, 16-bit for AV2) + anno.json."""
    os.makedirs(tmp, exist_ok=True)
    rows = GOLDEN[f"{case}_anno"]
    if is_argo:
        for cam, plane in enumerate(golden_planes(case, AV2_SHAPES)):
            Image.fromarray(plane.astype(np.uint16)).save(os.path.join(tmp, f"{cam}.png"))
        anno = [[] for _ in range(7)]
    else:
        for p, plane in enumerate(golden_planes(case, [mp.NUSC_IMG] * 60)):
            Image.fromarray(plane.astype(np.uint8)).save(os.path.join(tmp, f"{p // 10}_{mp.NAME_NUSC[p % 10]}.png"))
        anno = [{n: [] for n in mp.NAME_NUSC} for _ in range(6)]
    for r in rows:
        o = dict(bbox=[float(v) for v in r[:4]], score=float(r[4]), category=int(r[5]), cam_id=int(r[6]), obj_id=int(r[7]))
        (anno[o["cam_id"]] if is_argo else anno[o["cam_id"]][mp.NAME_NUSC[o["category"]]]).append(o)
    with open(os.path.join(tmp, "anno.json"), "w") as f:
        json.dump(anno, f, indent=2)


@pytest.mark.parametrize("case", ["nusc", "nusc_bbox"])
def test_nuscenes_pipeline_equals_load_mask_from_files(tmp_path, case):
    write_files(str(tmp_path / "frame"), case, False)
    want = LoadMaskFromFiles(str(tmp_path))(dict(sample_idx="frame"))
    cfg = dict(type="PaintMasksFromDetections", bbox_only=case == "nusc_bbox")
    got = PIPELINES.build(cfg)(dict(mask_detections=golden_dets("nusc")))
    assert got["mask_data"].dtype == want["mask_data"].dtype == torch.uint8
    assert torch.equal(got["mask_data"], want["mask_data"]) and torch.equal(got["mask_anno"], want["mask_anno"])


def test_argoverse2_pipeline_equals_load_mask_from_files(tmp_path):
    write_files(str(tmp_path / "frame"), "av2", True)
    l2i = np.random.default_rng(0).standard_normal((7, 4, 4)).astype(np.float32)
    want = LoadMaskFromFiles(str(tmp_path), obj_max_num=AV2_OBJ_MAX, is_argo=True)(dict(img_info=dict(uuid="frame"), lidar2img=l2i.copy()))
    got = PaintMasksFromDetections(obj_max_num=AV2_OBJ_MAX, is_argo=True)(
        dict(mask_detections=golden_dets("av2"), mask_img_shapes=AV2_SHAPES, lidar2img=l2i.copy()))
    assert got["mask_data"].dtype == want["mask_data"].dtype == torch.int32
    assert torch.equal(got["mask_data"], want["mask_data"]) and torch.equal(got["mask_anno"], want["mask_anno"])
    assert torch.equal(torch.as_tensor(got["lidar2img"]), torch.as_tensor(want["lidar2img"]))
    assert not np.array_equal(got["lidar2img"][0], l2i[0])


def one_object_dets(scores, cams=None, labels=None, boxes=None, crops=None, origins=None):
    n = len(scores)
    boxes = np.tile(np.array([[10, 10, 20, 20]], np.float32), (n, 1)) if boxes is None else boxes
    crops = [np.ones((10, 10), bool)] * n if crops is None else crops
    origins = np.tile(np.array([[10, 10]]), (n, 1)) if origins is None else origins
    return dict(boxes=boxes, scores=np.asarray(scores, np.float32), labels=np.zeros(n, np.int64) if labels is None else labels,
                cams=np.zeros(n, np.int64) if cams is None else cams, mask_crops=crops, mask_origins=origins)


def test_threshold_is_compared_in_float64():
    """float32(0.1) > 0.1 in float64 (the reference's NumPy 1.x widening); NumPy 2 would say False in float32."""
    f01 = np.float32(0.1)
    below = np.nextafter(f01, np.float32(0))
    plan = mp.plan_masks(one_object_dets([f01, below]))
    assert plan.num_painted == 1 and plan.anno[0]["car"][0]["score"] == float(f01)
    f02 = np.float32(0.2)
    d = one_object_dets([f02, np.nextafter(f02, np.float32(0))])
    plan = mp.plan_masks(d, is_argo=True, img_shapes=[(2048, 1550)] + [(1550, 2048)] * 6)
    assert plan.num_painted == 1 and plan.anno[0][0]["score"] == float(f02)
    assert mp.score_threshold([f01], 250, 0.1) == 0.1


@pytest.mark.parametrize("is_argo", [False, True])
def test_equal_scores_put_the_later_object_first(is_argo):
    crops = [np.ones((10, 10), bool), np.ones((10, 10), bool), np.ones((4, 4), bool)]
    origins = np.array([[10, 10], [15, 15], [100, 100]])
    d = one_object_dets([0.5, 0.5, 0.7], crops=crops, origins=origins)
    shapes = [(2048, 1550)] + [(1550, 2048)] * 6
    plan = mp.plan_masks(d, is_argo=is_argo, img_shapes=shapes, class_names=mp.NAME_NUSC)
    ids = {int(k): int(i) for k, i in zip(plan.obj_index, plan.obj_id)}
    assert ids == {2: 1, 1: 2, 0: 3}  # descending score; the tie goes to the later index
    planes = mp.paint_numpy(plan)
    src = planes[0].numpy() if not is_argo else mp.paint_numpy(mp.plan_masks(d, is_argo=True, img_shapes=[(1550, 2048)] * 7))[0].numpy()
    assert src[17, 17] == 2 and src[12, 12] == 3  # the overlap belongs to the earlier painted (later input) object


def test_bbox_rect_rounds_half_to_even_and_follows_python_slices():
    assert mp.bbox_rect([0.5, 1.5, 2.5, 3.5], (10, 10)) == (2, 0, 2, 2)
    assert mp.bbox_rect([-3.2, 2.0, 5.0, 4.0], (10, 10)) == (2, 7, 2, 0)  # x: slice(-3, 5) of 10 is empty
    assert mp.bbox_rect([1.0, -2.0, 4.0, 9.6], (10, 10)) == (8, 1, 2, 3)  # y: slice(-2, 10) -> rows 8, 9


def test_raises_for_a_loader_class_without_a_plane():
    with pytest.raises(ValueError, match="no plane"):
        PaintMasksFromDetections(class_names=["car", "tram"])(dict(mask_detections=one_object_dets([0.5])))


def test_raises_for_more_rows_than_obj_max_num():
    n = 12
    d = one_object_dets(np.linspace(0.3, 0.9, n), cams=np.arange(n) % 6)
    with pytest.raises(ValueError, match="obj_max_num"):
        PaintMasksFromDetections(obj_max_num=10)(dict(mask_detections=d))


def test_raises_for_mismatched_box_and_mask_counts():
    d = one_object_dets([0.5, 0.6])
    d["mask_crops"] = d["mask_crops"][:1]
    with pytest.raises(ValueError, match="mask crops"):
        mp.plan_masks(d)
    bbox = [np.zeros((0, 5), np.float32)] * 10
    segm = [[] for _ in range(10)]
    bbox[0] = np.array([[1, 1, 5, 5, 0.5], [2, 2, 6, 6, 0.6]], np.float32)
    segm[0] = [np.zeros((900, 1600), bool)]
    with pytest.raises(ValueError, match="2 boxes but 1 masks"):
        mp.plan_masks([(bbox, segm)] * 6)


def test_waymo_raises():
    with pytest.raises(NotImplementedError):
        PaintMasksFromDetections(is_waymo=True)


def test_header_abi_version_is_23():
    hdr = open(os.path.join(ROOT, "include", "fsf_hip.h")).read()
    assert int(re.search(r"#define\s+FSF_ABI_VERSION\s+(\d+)", hdr).group(1)) == 23
    for name in ("fsf_mask_extents", "fsf_paint_instance_masks"):
        assert name in hdr and name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
