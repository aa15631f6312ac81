"""K34c on the host: the paste specification (`mask_paint.roi_cover`: mmdet's `_do_paste_mask` + `mask_thr_binary` in float32)
against float64 `F.grid_sample` on mmdet's grid, its edge cases, the planner's rules for the `mask_rois` form, and the ABI surface.

Figures of the specification test as measured (M in {1, 2, 7, 14, 28}, 40 boxes each on a 48 x 64 plane, RoIs sigmoid(N(0, 3)), every
fifth all ones): max |spec - ref64| = 2.6e-6 over the candidate pixels, 20 of 614 400 pixels within 1e-4 of the threshold, no differing
decision, no reference-covered pixel outside the candidate rectangle."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fullysparsefusion_amd.mmdet3d_plugin.datasets import mask_paint as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 48, 64
THR = 0.5
MARGIN = 1e-4  # decisions may differ only where the float64 value is this close to the threshold
MARGIN_SHARE = 1e-3  # and such pixels may be at most this share of the pixels compared


def ref64(box, roi, shape):
    """mmdet's paste in float64 over the WHOLE image: grid_sample(bilinear, align_corners=False, zeros) on its normalised grid."""
    x0, y0, x1, y1 = (float(np.float32(v)) for v in box)
    gy = ((torch.arange(shape[0], dtype=torch.float64) + 0.5) - y0) / (y1 - y0) * 2 - 1
    gx = ((torch.arange(shape[1], dtype=torch.float64) + 0.5) - x0) / (x1 - x0) * 2 - 1
    grid = torch.stack([gx[None, :].expand(shape[0], shape[1]), gy[:, None].expand(shape[0], shape[1])], -1)[None]
    return F.grid_sample(torch.from_numpy(np.asarray(roi, np.float64))[None, None], grid, mode="bilinear", padding_mode="zeros",
                         align_corners=False)[0, 0].numpy()


def random_boxes(rng, n, h=H, w=W):
    """Boxes of every kind the paste meets: inside, leaving the image on any side, narrower than a pixel, larger than the image."""
    cx, cy = rng.uniform(-6, w + 6, n), rng.uniform(-6, h + 6, n)
    bw = np.where(rng.random(n) < 0.15, rng.uniform(0.05, 1.0, n), rng.uniform(1.0, 1.2 * w, n))
    bh = np.where(rng.random(n) < 0.15, rng.uniform(0.05, 1.0, n), rng.uniform(1.0, 1.2 * h, n))
    return np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1).astype(np.float32)


def random_rois(rng, n, m, dtype=np.float32):
    """sigmoid(N(0, 3)), every fifth map all ones."""
    r = 1.0 / (1.0 + np.exp(-rng.normal(0.0, 3.0, (n, m, m))))
    r[::5] = 1.0
    return r.astype(dtype)


def test_specification_against_float64_grid_sample():
    rng = np.random.default_rng(0)
    compared = near = differ = outside = 0
    worst = 0.0
    for m in (1, 2, 7, 14, 28):
        boxes, rois = random_boxes(rng, 40), random_rois(rng, 40, m)
        for box, roi in zip(boxes, rois):
            want = ref64(box, roi, (H, W))
            ya, xa, h, w, v, usable = mp.roi_sample(box, roi, (H, W))
            got = mp.paste_roi_mask(box, roi, THR, (H, W))
            assert np.array_equal(got[ya:ya + h, xa:xa + w], (v >= np.float32(THR)) & usable)
            in_rect = np.zeros((H, W), bool)
            in_rect[ya:ya + h, xa:xa + w] = True
            outside += int(((want >= THR) & ~in_rect).sum())
            if h:
                worst = max(worst, float(np.abs(np.where(usable, v, 0.0).astype(np.float64) - want[ya:ya + h, xa:xa + w]).max()))
            close = np.abs(want - THR) <= MARGIN
            bad = got != (want >= THR)
            assert not (bad & ~close).any(), (m, box, np.argwhere(bad & ~close)[:4])
            compared += want.size
            near += int(close.sum())
            differ += int(bad.sum())
    print(f"max |spec - ref64| = {worst:.3g}; {near} of {compared} pixels within {MARGIN} of the threshold; {differ} differing decisions; "
          f"{outside} reference-covered pixels outside the candidate rectangle")
    assert compared == 200 * H * W
    assert near <= MARGIN_SHARE * compared
    assert outside == 0
    # a tap position carries about 5 float32 roundings (6e-8 relative) of values up to M = 28: 8.4e-6 per axis, and v moves by at
    # most one texel difference (<= 1) times that, on both axes
    assert worst < 2e-5


def test_box_edge_on_a_pixel_centre_gives_exactly_one_half_and_is_painted():
    """All-ones map, x0 = k + 0.5: pixel k samples the map's left border half-way, v = 0.5 exactly; the pixel before it gets 0."""
    for m in (1, 7, 28):
        k = 9
        box = np.array([k + 0.5, 3.5, k + 0.5 + 2 * m, 3.5 + 2 * m], np.float32)  # two pixels per texel: every tap position is exact
        roi = np.ones((m, m), np.float32)
        ya, xa, h, w, v, usable = mp.roi_sample(box, roi, (H, W))
        row = 3 + m - ya  # a row well inside the box: wy contributes 1 in total
        assert usable[row, k - xa] and v[row, k - xa] == np.float32(0.5)
        mask = mp.paste_roi_mask(box, roi, 0.5, (H, W))
        assert mask[3 + m, k] and not mask[3 + m, k - 1]
        assert mask[3, k + m] and not mask[2, k + m]  # the same on the top edge (y0 = 3.5)
        assert not mp.paste_roi_mask(box, roi, np.nextafter(np.float32(0.5), np.float32(1)), (H, W))[3 + m, k]


@pytest.mark.parametrize("box", [[10, 10, 10, 20], [10, 10, 5, 20], [10, 20, 20, 20], [10, 10, 20, 5], [np.nan, 1, 5, 5], [1, 1, np.inf, 5],
                                 [-np.inf, 1, 5, 5]])
def test_degenerate_box_paints_nothing_but_keeps_id_and_anno_row(box):
    assert mp.roi_rect(box, (H, W)) == (0, 0, 0, 0)
    assert not mp.paste_roi_mask(box, np.ones((7, 7), np.float32), 0.5, (H, W)).any()
    d = dets(np.array([box, [100, 100, 140, 130]], np.float32), np.ones((2, 7, 7), np.float32), scores=[0.9, 0.8])
    plan = mp.plan_masks(d)
    assert plan.num_painted == 2 and [int(i) for i in plan.obj_id] == [1, 2]
    assert [a["obj_id"] for a in plan.anno[0]["car"]] == [1, 2]
    planes = mp.paint_numpy(plan)
    assert sorted(planes.unique().tolist()) == [0, 2]
    res = mp.PaintMasksFromDetections()(dict(mask_detections=d))
    assert int((res["mask_anno"][:, 8] > 0).sum()) == 2


def test_nan_texels_are_not_covered():
    roi = np.ones((4, 4), np.float32)
    roi[1, 2] = np.nan
    box = np.array([8, 8, 24, 24], np.float32)  # 4 pixels per texel
    mask = mp.paste_roi_mask(box, roi, 0.5, (H, W))
    want = np.nan_to_num(ref64(box, np.nan_to_num(roi, nan=1.0), (H, W))) >= 0.5
    touched = np.isnan(ref64(box, roi, (H, W)))
    assert touched.any() and not mask[touched].any()
    assert np.array_equal(mask[~touched], want[~touched]) and mask.any()
    assert not mp.paste_roi_mask(box, np.full((4, 4), np.nan, np.float32), 0.5, (H, W)).any()


def test_float16_maps_are_widened_exactly():
    rng = np.random.default_rng(3)
    roi16 = random_rois(rng, 1, 7, np.float16)[0]
    box = random_boxes(rng, 1)[0]
    a = mp.roi_sample(box, roi16, (H, W))
    b = mp.roi_sample(box, roi16.astype(np.float32), (H, W))
    assert np.array_equal(a[4], b[4], equal_nan=True) and np.array_equal(a[5], b[5])


# ---------------------------------------------------------------------------------------------------- planner
def dets(boxes, rois, scores=None, cams=None, labels=None):
    n = len(boxes)
    return dict(boxes=np.asarray(boxes, np.float32), scores=np.asarray(scores if scores is not None else np.linspace(0.9, 0.3, n), np.float32),
                labels=np.zeros(n, np.int64) if labels is None else np.asarray(labels), cams=np.zeros(n, np.int64) if cams is None else np.asarray(cams),
                mask_rois=rois)


def frame_dets(seed, n, m, img_shapes, dtype=np.float32, ncls=10):
    """n detections spread over the cameras of `img_shapes` (boxes in each camera's own pixels), distinct scores above both datasets'
    initial thresholds."""
    rng = np.random.default_rng(seed)
    cams = rng.integers(0, len(img_shapes), n)
    boxes = np.zeros((n, 4), np.float32)
    for k, c in enumerate(cams):
        h, w = img_shapes[c]
        bw, bh = rng.uniform(20, 0.3 * w), rng.uniform(20, 0.3 * h)
        x, y = rng.uniform(-0.1 * w, w), rng.uniform(-0.1 * h, h)
        boxes[k] = (x, y, x + bw, y + bh)
    scores = rng.permutation(np.linspace(0.25, 0.99, n)).astype(np.float32)
    return dict(boxes=boxes, scores=scores, labels=rng.integers(0, ncls, n), cams=cams, mask_rois=random_rois(rng, n, m, dtype))


def pasted(d, img_shapes, thr=0.5):
    """The same detections with `masks`: every RoI pasted to full size by the specification."""
    out = {k: v for k, v in d.items() if k != "mask_rois"}
    rois = mp._host(d["mask_rois"])
    boxes, cams = mp._host(d["boxes"]), mp._host(d["cams"])
    out["masks"] = [mp.paste_roi_mask(boxes[k], rois[k], thr, img_shapes[int(cams[k])]) for k in range(len(boxes))]
    return out


def test_mask_rois_excludes_the_other_mask_forms():
    d = dets([[10, 10, 30, 30]], np.ones((1, 7, 7), np.float32))
    with pytest.raises(ValueError, match=r"mask_rois.*masks"):
        mp.plan_masks(dict(d, masks=[np.ones(mp.NUSC_IMG, bool)]))
    with pytest.raises(ValueError, match=r"mask_rois.*mask_crops"):
        mp.plan_masks(dict(d, mask_crops=[np.ones((4, 4), bool)], mask_origins=np.array([[1, 1]])))


@pytest.mark.parametrize("thr", [0.0, -0.5, float("nan")])
def test_mask_thr_must_be_positive(thr):
    d = dets([[10, 10, 30, 30]], np.ones((1, 7, 7), np.float32))
    with pytest.raises(ValueError, match="mask_thr"):
        mp.plan_masks(d, mask_thr=thr)
    with pytest.raises(ValueError, match="mask_thr"):
        mp.PaintMasksFromDetections(mask_thr=thr)


@pytest.mark.parametrize("rois", [np.ones((1, 7), np.float32), np.ones((1, 7, 6), np.float32), np.ones((1, 1, 7, 7), np.float32),
                                  np.ones((1, 65, 65), np.float32), np.ones((1, 0, 0), np.float32), np.ones((2, 7, 7), np.float32),
                                  np.ones((1, 7, 7), np.float64), [np.ones((7, 7), np.float32)]])
def test_wrong_rank_shape_or_type_raises(rois):
    with pytest.raises(ValueError, match="mask_rois"):
        mp.plan_masks(dets([[10, 10, 30, 30]], rois))


def test_mask_form_and_the_error_without_masks():
    d = dets([[10, 10, 30, 30]], np.ones((1, 7, 7), np.float32))
    assert mp._mask_form(mp.plan_masks(d)) == "rois"
    del d["mask_rois"]
    with pytest.raises(ValueError, match="mask detections carry no masks"):
        mp._mask_form(mp.plan_masks(d))


def test_bbox_only_ignores_mask_rois():
    d = dets([[10.4, 10.6, 30.2, 30.5], [50, 50, 80, 90]], np.zeros((2, 7, 7), np.float32))
    bare = {k: v for k, v in d.items() if k != "mask_rois"}
    a = mp.PaintMasksFromDetections(bbox_only=True)(dict(mask_detections=d))
    b = mp.PaintMasksFromDetections(bbox_only=True)(dict(mask_detections=bare))
    assert torch.equal(a["mask_data"], b["mask_data"]) and torch.equal(a["mask_anno"], b["mask_anno"]) and bool(a["mask_data"].any())
    d["mask_rois"] = np.zeros((2, 7), np.float32)  # not even looked at
    assert mp._mask_form(mp.plan_masks(d, bbox_only=True)) == "rect"


NUSC_SHAPES = [mp.NUSC_IMG] * 6
AV2_SHAPES = [(2048, 1550)] + [mp.AV2_PLANE] * 6


@pytest.mark.parametrize("is_argo", [False, True])
def test_order_ids_anno_and_planes_equal_the_pasted_full_size_masks(is_argo):
    shapes = AV2_SHAPES if is_argo else NUSC_SHAPES
    d = frame_dets(5, 24, 14, shapes)
    d["scores"][3] = d["scores"][11]  # an equal pair
    d["cams"][3], d["labels"][3] = d["cams"][11], d["labels"][11]
    d["scores"][0] = 0.05  # below the threshold: no id
    kw = dict(is_argo=is_argo, img_shapes=shapes)
    a, b = mp.plan_masks(d, **kw), mp.plan_masks(pasted(d, shapes), **kw)
    for key in ("obj_index", "obj_plane", "obj_id"):
        assert np.array_equal(getattr(a, key), getattr(b, key)), key
    assert a.anno == b.anno and a.num_painted == b.num_painted == 23
    assert torch.equal(mp.paint_numpy(a), mp.paint_numpy(b)) and bool(mp.paint_numpy(a).any())
    t = mp.PaintMasksFromDetections(is_argo=is_argo, obj_max_num=250)
    ra = t(dict(mask_detections=d, mask_img_shapes=shapes, lidar2img=np.eye(4, dtype=np.float32)[None].repeat(7, 0)))
    rb = t(dict(mask_detections=pasted(d, shapes), mask_img_shapes=shapes, lidar2img=np.eye(4, dtype=np.float32)[None].repeat(7, 0)))
    assert torch.equal(ra["mask_data"], rb["mask_data"]) and torch.equal(ra["mask_anno"], rb["mask_anno"])


def test_mask_thr_reaches_the_painter():
    d = dets([[10, 10, 40, 40]], np.full((1, 7, 7), 0.6, np.float32))
    lo = mp.PaintMasksFromDetections(mask_thr=0.5)(dict(mask_detections=d))["mask_data"]
    hi = mp.PaintMasksFromDetections(mask_thr=0.7)(dict(mask_detections=d))["mask_data"]
    assert bool(lo.any()) and not bool(hi.any())
    assert torch.equal(lo, mp.PaintMasksFromDetections()(dict(mask_detections=d))["mask_data"])  # the default is 0.5


# ---------------------------------------------------------------------------------------------------- ABI surface
def test_entry_point_is_declared_and_documented_and_the_abi_version_is_23():
    from fullysparsefusion_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "fsf_hip.h")).read()
    assert int(re.search(r"#define\s+FSF_ABI_VERSION\s+(\d+)", hdr).group(1)) == 23
    assert "fsf_paint_roi_masks" in hdr and "fsf_paint_roi_masks" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    argtypes, restype = _lib.SIGNATURES["fsf_paint_roi_masks"]
    assert restype is _lib.c_i32 and len(argtypes) == 17 and argtypes[11] is _lib.c_f32 and argtypes[3] is _lib.c_i64
    src = open(os.path.join(ROOT, "fullysparsefusion_amd", "hip_ops_mask.py")).read()
    assert "fsf_paint_roi_masks" in src and "torch.empty" in src and "synchronize" not in src and ".item()" not in src
    assert not re.search(r"torch\.zeros|torch\.full|empty_like|torch\.ones|new_zeros|new_empty|new_full|_lib\.workspace", src)


def test_argument_checks_refuse_on_the_host():
    """K34b's checks (dst_w % 16, a 16-byte aligned output, row and plane limits) and K34c's own (map side, element size, threshold):
    every call below is refused before anything is launched, so it runs without a device."""
    from fullysparsefusion_amd import _lib, build

    build.build()
    h = _lib.lib()
    unsupported, invalid = _lib.DEFINES["FSF_ERR_UNSUPPORTED"], _lib.DEFINES["FSF_ERR_INVALID_ARG"]
    fake, null = _lib.c_p(4096), _lib.c_p(None)  # (never dereferenced)

    def call(n_rows=3, planes=2, rois=fake, side=28, elem=4, thr=0.5, dst=(32, 64), out_elem=1, out=fake, table=fake):
        return h.fsf_paint_roi_masks(table, fake, fake, n_rows, fake, fake, fake, planes, rois, side, elem, thr, dst[0], dst[1], out_elem, out, None)

    assert call(planes=0) == 0  # nothing to write
    for bad in (dict(side=0), dict(side=65), dict(elem=1), dict(elem=8), dict(thr=0.0), dict(thr=-1.0), dict(thr=float("nan")),
                dict(n_rows=-1), dict(planes=-1), dict(dst=(0, 64)), dict(out_elem=2), dict(rois=null), dict(out=null), dict(table=null)):
        assert call(**bad) == invalid, bad
    for bad in (dict(dst=(32, 72)), dict(out=_lib.c_p(4104)), dict(planes=65536), dict(n_rows=1 << 31), dict(rois=_lib.c_p(4098))):
        assert call(**bad) == unsupported, bad
    assert call(rois=_lib.c_p(4098), elem=2, dst=(32, 72)) == unsupported


def test_the_wrapper_of_the_new_module_has_guard_band_cases():
    import ast

    import test_guard_bands_mask_gpu as gb
    from fullysparsefusion_amd import hip_ops_mask

    src = open(os.path.join(ROOT, "fullysparsefusion_amd", "hip_ops_mask.py")).read()
    alloc = {node.name for node in ast.parse(src).body
             if isinstance(node, ast.FunctionDef) and re.search(r"torch\.empty", ast.get_source_segment(src, node))}
    assert alloc == {"paint_roi_masks"} == set(gb.CASES)
    for name, cases in gb.CASES.items():
        assert hasattr(hip_ops_mask, name) and {k for k, _ in cases} >= {"ragged", "minimal", "empty"}
