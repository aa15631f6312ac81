"""K34c (fsf_paint_roi_masks, csrc/mask_paint.hip) against the host painter `mask_paint.paint_numpy`, bit for bit: small hand-made
plans that reach every path of the kernel (33 x 272 planes cross both tile borders of the 16 x 256 tile), then the whole
`PaintMasksFromDetections` route on `mask_rois` against the `masks=` route fed with the specification's pasted masks."""
import os
import sys

import numpy as np
import pytest
import torch

from fullysparsefusion_amd.mmdet3d_plugin.datasets import mask_paint as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import FILLS, guarded  # noqa: E402
from test_mask_roi_paint_cpu import AV2_SHAPES, NUSC_SHAPES, frame_dets, pasted, random_boxes, random_rois  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PH, PW = 33, 272


def make_plan(boxes, rois, planes, planes_src, dst=None, i32=False, thr=0.5, index=None):
    """A MaskPlan as plan_masks would emit it, on planes of any size: object r of the table is detection index[r] (default r), on
    plane planes[r] (ascending), with id r + 1; every plane is its own 'camera' of image size planes_src[p]."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    planes = np.asarray(planes, np.int64)
    assert (np.diff(planes) >= 0).all()
    index = np.arange(len(planes)) if index is None else np.asarray(index, np.int64)
    cams = np.zeros(len(boxes), np.int64)
    cams[index] = planes
    planes_src = [tuple(s) for s in planes_src]
    return mp.MaskPlan(is_argo=bool(i32), dets=dict(mask_rois=rois), boxes=boxes, cams=cams, img_shapes=planes_src, planes_src=planes_src,
                       dst=tuple(dst if dst is not None else planes_src[0]), bbox_only=False, mask_thr=np.float32(thr), obj_index=index,
                       obj_plane=planes, obj_id=np.arange(1, len(planes) + 1, dtype=np.int64))


def on_device(plan):
    """The same plan with its RoI maps on the device (read in place by element offset)."""
    d = dict(plan.__dict__)
    d["dets"] = dict(mask_rois=torch.from_numpy(np.ascontiguousarray(plan.dets["mask_rois"])).to(DEV))
    return mp.MaskPlan(**d)


def check(plan, both=True):
    want = mp.paint_numpy(plan)
    got = mp.paint_device(plan, DEV)
    assert got.is_cuda and got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(got.cpu(), want), f"host maps: {int((got.cpu() != want).sum())} pixels differ"
    if both:
        got = mp.paint_device(on_device(plan), DEV)
        assert torch.equal(got.cpu(), want), f"device maps: {int((got.cpu() != want).sum())} pixels differ"
    return want


# boxes (x0, y0, x1, y1) on a 33 x 272 plane: leaving it on each side, outside it, covering it, narrower than a pixel, degenerate,
# an edge on a pixel centre, an overlapping pair, one across the tile border at column 256 and row 16
EDGE_BOXES = [
    [-20.3, 5.2, 30.7, 20.9], [250.4, 8.1, 300.0, 25.5], [100.2, -12.6, 140.8, 9.3], [60.5, 20.2, 99.1, 50.0],
    [300.0, 5.0, 340.0, 20.0], [-50.0, -30.0, -5.0, -2.0], [10.0, 40.0, 60.0, 70.0],
    [-300.0, -40.0, 600.0, 80.0],
    [150.2, 3.0, 150.6, 30.0], [160.0, 12.3, 200.0, 12.5], [170.31, 5.07, 170.39, 5.11],
    [180.0, 5.0, 180.0, 25.0], [190.0, 25.0, 185.0, 30.0], [np.nan, 1.0, 20.0, 20.0], [1.0, 1.0, np.inf, 20.0],
    [40.5, 2.5, 68.5, 30.5],
    [200.0, 2.0, 240.0, 28.0], [220.0, 10.0, 262.0, 33.0],
    [240.7, 10.1, 271.9, 21.3],
]
EDGE_ORDER = [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 7]  # the box that covers the plane goes last


@pytest.mark.parametrize("i32", [False, True], ids=["u8", "i32"])
@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("m", [1, 2, 7, 28])
def test_kernel_equals_host_painter_on_every_kind_of_box(m, dtype, i32):
    rng = np.random.default_rng(m)
    boxes = np.asarray(EDGE_BOXES, np.float32)[EDGE_ORDER]
    rois = random_rois(rng, len(boxes), m, dtype)
    rois[EDGE_ORDER.index(15)] = 1.0  # the pixel-centre box, all ones
    rois[EDGE_ORDER.index(16)] = 1.0  # the first of the overlapping pair
    planes = [0] * len(boxes) + [1] * 12
    boxes = np.concatenate([boxes, random_boxes(rng, 12, PH, PW)])
    rois = np.concatenate([rois, random_rois(rng, 12, m, dtype)])
    want = check(make_plan(boxes, rois, planes, [(PH, PW)] * 2, i32=i32))
    assert want[0].unique().numel() >= 4 and bool(want[1].any())
    assert want[0, 16, 40] == EDGE_ORDER.index(15) + 1 and want[0, 16, 39] != EDGE_ORDER.index(15) + 1  # v = 0.5 exactly at column 40


@pytest.mark.parametrize("m", [1, 7, 28])
def test_box_edge_on_a_pixel_centre_is_painted(m):
    """x0 = k + 0.5 and an all-ones map: v = 0.5 exactly at column k, and the kernel decides `>=` as the specification does."""
    k = 40
    box = [k + 0.5, 2.5, k + 0.5 + 2 * m, 2.5 + 2 * m]
    plan = make_plan([box], np.ones((1, m, m), np.float32), [0], [(80, PW)])
    want = check(plan)
    got = mp.paint_device(plan, DEV).cpu()
    assert got[0, 2 + m, k] == 1 and got[0, 2 + m, k - 1] == 0 and got[0, 2, k + m] == 1 and got[0, 1, k + m] == 0
    assert torch.equal(got, want)
    above = make_plan([box], np.ones((1, m, m), np.float32), [0], [(80, PW)], thr=np.nextafter(np.float32(0.5), np.float32(1)))
    assert check(above)[0, 2 + m, k] == 0


def test_first_of_two_overlapping_objects_wins():
    boxes = [[20.0, 4.0, 60.0, 28.0], [40.0, 10.0, 90.0, 30.0]]
    want = check(make_plan(boxes, np.ones((2, 7, 7), np.float32), [0, 0], [(PH, PW)]))
    got = mp.paint_device(make_plan(boxes, np.ones((2, 7, 7), np.float32), [0, 0], [(PH, PW)]), DEV).cpu()
    assert got[0, 15, 50] == 1 and got[0, 15, 80] == 2 and got[0, 6, 30] == 1 and got[0, 6, 80] == 0
    assert torch.equal(got, want)


def test_more_than_256_rows_in_a_plane():
    """Plane 0: 255 small objects, then one that fills every tile, then 44 more in a second chunk that no tile may reach (it is full);
    plane 1: 300 small objects, those of the second chunk painted after a first chunk that leaves pixels open."""
    rng = np.random.default_rng(7)

    def small(n):
        cx, cy = rng.uniform(0, PW, n), rng.uniform(0, PH, n)
        w, h = rng.uniform(3, 14, n), rng.uniform(3, 9, n)
        return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32)

    boxes = np.concatenate([small(255), [[-1000.0, -1000.0, 1272.0, 1033.0]], small(44), small(300)])
    rois = random_rois(rng, 600, 7)
    rois[255] = 1.0
    want = check(make_plan(boxes, rois, [0] * 300 + [1] * 300, [(PH, PW)] * 2, i32=True))
    assert int(want[0].max()) == 256 and bool((want[0] != 0).all())  # the filling object took every pixel left; 257.. came too late
    assert int(want[1].max()) > 300 + 256 and bool((want[1] == 0).any())


def test_empty_plane_between_two_used_ones_and_no_rows_at_all():
    rng = np.random.default_rng(8)
    boxes, rois = random_boxes(rng, 6, PH, PW), random_rois(rng, 6, 14)
    want = check(make_plan(boxes, rois, [0, 0, 0, 2, 2, 2], [(PH, PW)] * 3))
    assert bool(want[0].any()) and not bool(want[1].any()) and bool(want[2].any())
    for fill in FILLS:  # nothing to paint: every element is still written
        with guarded(fill):
            none = mp.paint_device(make_plan(np.zeros((0, 4)), np.zeros((0, 7, 7), np.float32), [], [(PH, PW)] * 2), DEV)
            assert tuple(none.shape) == (2, PH, PW) and not bool(none.any())


def test_resized_plane():
    """Source 64 x 48 painted into 48 x 64 (rows shrink, columns grow), beside a plane that is not resized."""
    rng = np.random.default_rng(9)
    boxes = np.concatenate([random_boxes(rng, 8, 64, 48), random_boxes(rng, 4, 48, 64)])
    rois = random_rois(rng, 12, 7)
    plan = make_plan(boxes, rois, [0] * 8 + [1] * 4, [(64, 48), (48, 64)], dst=(48, 64), i32=True)
    want = check(plan)
    assert tuple(want.shape) == (2, 48, 64) and bool(want[0].any()) and bool(want[1].any())


def test_output_does_not_depend_on_what_the_buffer_held():
    rng = np.random.default_rng(10)
    plan = make_plan(random_boxes(rng, 10, PH, PW), random_rois(rng, 10, 14, np.float16), [0] * 5 + [1] * 5, [(PH, PW)] * 2)
    want = mp.paint_numpy(plan)
    for fill in FILLS:
        with guarded(fill) as g:
            got = mp.paint_device(plan, DEV)
            assert g.violations() == [] and any(r["site"] == "paint_roi_masks" for r in g.records)
        assert torch.equal(got.cpu(), want), hex(fill)


def test_only_painted_rows_of_a_device_tensor_are_read():
    rng = np.random.default_rng(11)
    n, picked = 40, [31, 2, 17, 5, 38, 11]
    boxes = random_boxes(rng, n, PH, PW)
    rois = np.full((n, 7, 7), np.nan, np.float32)
    rois[picked] = random_rois(rng, len(picked), 7)
    plan = make_plan(boxes, rois, [0, 0, 0, 1, 1, 1], [(PH, PW)] * 2, index=picked)
    want = check(plan)
    clean = np.zeros_like(rois)
    clean[picked] = rois[picked]
    assert torch.equal(want, mp.paint_numpy(make_plan(boxes, clean, [0, 0, 0, 1, 1, 1], [(PH, PW)] * 2, index=picked)))
    assert bool(want.any())


# ---------------------------------------------------------------------------------------------------- the whole route
@pytest.mark.parametrize("is_argo", [False, True], ids=["nuscenes", "argoverse2"])
def test_pipeline_on_mask_rois_equals_the_masks_route_and_the_host_route(is_argo):
    shapes = AV2_SHAPES if is_argo else NUSC_SHAPES
    d = frame_dets(21, 30, 28, shapes, np.float16 if is_argo else np.float32)
    l2i = np.eye(4, dtype=np.float32)[None].repeat(7, 0)
    kw = dict(is_argo=is_argo, obj_max_num=250)
    res = lambda dets: dict(mask_detections=dets, mask_img_shapes=shapes, lidar2img=l2i.copy())  # noqa: E731
    host = mp.PaintMasksFromDetections(**kw)(res(d))
    dd = dict(d, mask_rois=torch.from_numpy(d["mask_rois"]).to(DEV), scores=torch.from_numpy(d["scores"]).to(DEV),
              boxes=torch.from_numpy(d["boxes"]).to(DEV))
    got = mp.PaintMasksFromDetections(device=DEV, **kw)(res(dd))
    assert got["mask_data"].is_cuda and got["mask_data"].dtype == (torch.int32 if is_argo else torch.uint8)
    assert torch.equal(got["mask_data"].cpu(), host["mask_data"]) and torch.equal(got["mask_anno"], host["mask_anno"])
    assert got["mask_data"].unique().numel() > 10
    full = pasted(d, shapes)
    full["masks"] = [torch.from_numpy(m).to(DEV) for m in full["masks"]]
    old = mp.PaintMasksFromDetections(device=DEV, **kw)(res(full))
    assert torch.equal(got["mask_data"], old["mask_data"]) and torch.equal(got["mask_anno"], old["mask_anno"])
    from_host = mp.PaintMasksFromDetections(device=DEV, **kw)(res(d))  # host maps: one upload of the painted ones
    assert torch.equal(from_host["mask_data"], got["mask_data"])
