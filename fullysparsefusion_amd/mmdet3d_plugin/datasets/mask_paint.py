"""The camera branch's inputs `mask_data` / `mask_anno` built in memory from a 2-D instance segmenter's detections, equal to what
`LoadMaskFromFiles` returns for the files the reference's offline writer (tools/mask_tools/save_mask_nusc.py, save_mask_argo2.py)
would have produced for the same detections (docs/kernels/K34_mask_paint.md).

    detections -> plan_masks (host: threshold, paint order, ids, anno rows)   -> paint_numpy  (host referee)
                                                                              -> paint_device (K34: csrc/mask_paint.hip)

The writer's rules, as restated here:
  * threshold = max(k-th highest score over every camera and class (0 with fewer than k), score_thr_init); an object is painted
    iff float64(score) > threshold.  The comparison is float64: the reference ran under NumPy 1.x, where the float32 score is
    widened against the Python float threshold (NumPy 2 would compare in float32).
  * paint order and ids: camera-major; nuScenes then goes class by class in the writer's `name_nusc` order, one plane per
    (camera, class); Argoverse 2 merges the classes of a camera into one plane.  Inside a group objects go by descending score,
    equal scores as the reverse of a STABLE ascending sort (the later object first; the reference's np.argsort is unstable).
    Ids start at 1 and count painted objects only; an object whose pixels are all taken still has its id and anno row.
  * a pixel takes the id of the first object of its plane, in that order, whose mask covers it.
  * bbox_only: the mask is the rectangle mask[round(y1):round(y2), round(x1):round(x2)] (Python round, half to even, and
    Python slice semantics).
Equal-score order and the float64 comparison are the two rules the reference leaves to its environment; tests pin both.

Detections come in two forms:
  * mmdet's per camera `(bbox_result, segm_result)`: 10 nuImages classes, bbox_result[i] f32 [n, 5] (x1, y1, x2, y2, score),
    segm_result[i] n masks of the camera's image size (a class with no masks is skipped, as the writer does);
  * packed (`dict`): boxes [N, 4], scores [N], labels [N] (nuImages index), cams [N] and either `masks` (full image size: one
    [N, H, W] array / tensor, or a list of N 2-D masks, host or device), or `mask_crops` (N 2-D arrays) with `mask_origins` [N, 2]
    (y, x), or `mask_rois` (what a mask head emits: one [N, M, M] float32 / float16 array or tensor of soft masks, host or
    device, pasted over each box by `roi_cover`'s rule: K34c), or none of them (bbox_only).  Boxes and scores are taken as float32.
"""
import math

import numpy as np
import torch

from ..registry import PIPELINES
from .pipelines import LoadMaskFromFiles, _resize_nearest

NUIM_CLASS_NAMES = ["car", "truck", "trailer", "bus", "construction_vehicle", "bicycle", "motorcycle", "pedestrian", "traffic_cone",
                    "barrier"]
NAME_NUSC = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone"]
NAME_TO_NUM_NUSC = {n: i for i, n in enumerate(NAME_NUSC)}
NUSC_CAMS, NUSC_IMG = 6, (900, 1600)
AV2_CAMS, AV2_PLANE = 7, (1550, 2048)
DEFAULTS = dict(nuscenes=dict(score_thr_init=0.1, topk=250), argo=dict(score_thr_init=0.2, topk=65535))


def _host(a):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().numpy()
    return np.asarray(a)


def pack_mmdet(results):
    """mmdet's per-camera (bbox_result, segm_result) -> the packed dict (objects camera-major, then class, then j)."""
    boxes, scores, labels, cams, masks = [], [], [], [], []
    for cam, (bbox_result, segm_result) in enumerate(results):
        if len(bbox_result) != len(NUIM_CLASS_NAMES) or len(segm_result) != len(NUIM_CLASS_NAMES):
            raise ValueError(f"camera {cam}: expected {len(NUIM_CLASS_NAMES)} nuImages classes")
        for i in range(len(NUIM_CLASS_NAMES)):
            if len(segm_result[i]) == 0:  # the writer skips a class without masks
                continue
            b = np.asarray(_host(bbox_result[i]), dtype=np.float32).reshape(-1, 5)
            if len(segm_result[i]) != len(b):
                raise ValueError(f"camera {cam}, class {NUIM_CLASS_NAMES[i]}: {len(b)} boxes but {len(segm_result[i])} masks")
            boxes.append(b[:, :4])
            scores.append(b[:, 4])
            labels.append(np.full(len(b), i, dtype=np.int64))
            cams.append(np.full(len(b), cam, dtype=np.int64))
            masks.extend(segm_result[i][j] for j in range(len(b)))
    cat = lambda xs, shape, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(shape, dt)  # noqa: E731
    return dict(boxes=cat(boxes, (0, 4), np.float32), scores=cat(scores, (0,), np.float32), labels=cat(labels, (0,), np.int64),
                cams=cat(cams, (0,), np.int64), masks=masks, num_cams=len(results))


def _read_small(dets):
    """scores / boxes / labels / cams on the host; the device-resident ones come back in ONE read-back (f32 and small ints are
    exact in f64)."""
    keys = ("scores", "boxes", "labels", "cams")
    on_dev = [k for k in keys if isinstance(dets[k], torch.Tensor) and dets[k].is_cuda]
    out = {k: _host(dets[k]) for k in keys if k not in on_dev}
    if on_dev:
        ts = [dets[k].detach().reshape(-1) for k in on_dev]
        ts = [t.float().double() if t.is_floating_point() else t.double() for t in ts]
        host = torch.cat(ts).cpu().numpy()
        at = 0
        for k, t in zip(on_dev, ts):
            out[k] = host[at:at + t.numel()]
            at += t.numel()
    return out


class MaskPlan:
    """What plan_masks decides: the painted objects in paint order and where they go, and the anno list of anno.json."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _checked_len(dets, n):
    for key in ("boxes", "labels", "cams"):
        if len(dets[key]) != n:
            raise ValueError(f"mask detections: {len(dets[key])} {key} for {n} scores")
    masks = dets.get("masks")
    if masks is not None and len(masks) != n:
        raise ValueError(f"mask detections: {len(masks)} masks for {n} boxes")
    if dets.get("mask_crops") is not None and (len(dets["mask_crops"]) != n or len(dets["mask_origins"]) != n):
        raise ValueError(f"mask detections: {len(dets['mask_crops'])} mask crops for {n} boxes")


ROI_MAX = 64  # the largest RoI map side K34c takes (a mask head's is 14 or 28)


def _checked_rois(dets, n):
    """`mask_rois` excludes the two other mask forms and is one float32 / float16 [n, M, M] array or tensor, 1 <= M <= ROI_MAX."""
    rois = dets.get("mask_rois")
    if rois is None:
        return
    for other in ("masks", "mask_crops"):
        if dets.get(other) is not None:
            raise ValueError(f"mask detections: mask_rois and {other} are both given, pass one form of masks")
    shape = tuple(getattr(rois, "shape", ()))
    if not isinstance(rois, (np.ndarray, torch.Tensor)) or len(shape) != 3 or shape[1] != shape[2] or not 1 <= shape[1] <= ROI_MAX:
        raise ValueError(f"mask detections: mask_rois must be one [N, M, M] array or tensor with 1 <= M <= {ROI_MAX}, "
                         f"got {type(rois).__name__} of shape {shape}")
    if str(rois.dtype).split(".")[-1] not in ("float32", "float16"):
        raise ValueError(f"mask detections: mask_rois must be float32 or float16, got {rois.dtype}")
    if shape[0] != n:
        raise ValueError(f"mask detections: {shape[0]} mask_rois for {n} boxes")


def paint_order(scores, groups):
    """Indices of `scores` grouped by `groups` (ascending), each group by descending score, equal scores later index first."""
    scores = np.asarray(scores, dtype=np.float64)
    by_score = np.argsort(scores, kind="stable")[::-1]  # the reverse of a stable ascending sort
    return by_score[np.argsort(np.asarray(groups)[by_score], kind="stable")]


def score_threshold(scores, topk, score_thr_init):
    """max(k-th highest score (0 with fewer than k), score_thr_init), in float64."""
    s = np.sort(np.asarray(scores, dtype=np.float32).astype(np.float64))[::-1]
    return max(float(s[topk - 1]) if len(s) >= topk else 0.0, float(score_thr_init))


def plan_masks(dets, is_argo=False, class_names=None, img_shapes=None, score_thr_init=None, topk=None, bbox_only=False, mask_thr=0.5):
    """Selection, paint order, ids, output planes and anno rows (the anno.json structure) of one frame.  `dets`: packed dict or
    mmdet's per-camera list.  Scores on the device cost one read-back; nothing else is read from the device here.  `mask_thr`: the
    threshold on pasted `mask_rois` (mmdet's mask_thr_binary), taken as float32."""
    if not isinstance(dets, dict):
        dets = pack_mmdet(dets)
    if not float(mask_thr) > 0.0:
        raise ValueError(f"mask_thr must be above 0, got {mask_thr}: a threshold of 0 or less covers every pixel the paste leaves at 0")
    ds = "argo" if is_argo else "nuscenes"
    score_thr_init = DEFAULTS[ds]["score_thr_init"] if score_thr_init is None else score_thr_init
    topk = DEFAULTS[ds]["topk"] if topk is None else int(topk)
    ncam = AV2_CAMS if is_argo else NUSC_CAMS
    small = _read_small(dets)
    scores = small["scores"].astype(np.float32).reshape(-1)
    n = len(scores)
    _checked_len(dets, n)
    if not bbox_only:
        _checked_rois(dets, n)
    boxes = small["boxes"].astype(np.float32).reshape(n, 4)
    labels = small["labels"].astype(np.int64).reshape(n)
    cams = small["cams"].astype(np.int64).reshape(n)
    if n and (labels.min() < 0 or labels.max() >= len(NUIM_CLASS_NAMES) or cams.min() < 0 or cams.max() >= ncam):
        raise ValueError("mask detections: label or camera index out of range")
    if dets.get("num_cams", ncam) != ncam:
        raise ValueError(f"mask detections: {dets['num_cams']} cameras, the loader expects {ncam}")
    if is_argo:
        if img_shapes is None or len(img_shapes) != ncam:
            raise ValueError("Argoverse 2 needs the image shape (h, w) of each of the 7 cameras")
        img_shapes = [tuple(int(v) for v in s[:2]) for s in img_shapes]
        if any(s != AV2_PLANE for s in img_shapes[1:]):
            raise ValueError(f"Argoverse 2 cameras 1-6 must be {AV2_PLANE} (LoadMaskFromFiles stacks them unresized)")
        planes_src = [img_shapes[0]] + img_shapes[1:]
        dst = AV2_PLANE
        # camera-major, classes merged in the writer's collection order (class, then input index)
        merged = np.lexsort((np.arange(n), labels)) if n else np.zeros(0, np.int64)
        order = merged[paint_order(scores[merged], cams[merged])]
        plane_of = lambda k: int(cams[k])  # noqa: E731
    else:
        class_names = list(class_names if class_names is not None else NUIM_CLASS_NAMES)
        missing = [c for c in class_names if c not in NAME_NUSC]
        if missing:
            raise ValueError(f"the writer has no plane for loader classes {missing}")
        img_shapes = [NUSC_IMG] * ncam
        planes_src = [NUSC_IMG] * (ncam * len(class_names))
        dst = NUSC_IMG
        cls_rank = np.array([NAME_NUSC.index(NUIM_CLASS_NAMES[i]) for i in range(len(NUIM_CLASS_NAMES))])
        order = paint_order(scores, cams * len(NAME_NUSC) + cls_rank[labels]) if n else np.zeros(0, np.int64)
        loader_pos = {NUIM_CLASS_NAMES.index(c): p for p, c in enumerate(class_names)}

        def plane_of(k):
            p = loader_pos.get(int(labels[k]))
            return None if p is None else int(cams[k]) * len(class_names) + p

    thr = score_threshold(scores, topk, score_thr_init)
    painted = [int(k) for k in order if float(scores[k]) > thr]
    max_id = 254 if not is_argo else 65535  # the writer stores u8 (asserting < 255) / u16 PNGs
    if len(painted) > max_id:
        raise ValueError(f"{len(painted)} painted objects: ids above {max_id} do not fit the writer's planes")
    anno = [dict((c, []) for c in NAME_NUSC) for _ in range(ncam)] if not is_argo else [[] for _ in range(ncam)]
    obj_index, obj_plane, obj_id = [], [], []
    for i, k in enumerate(painted):
        a = dict(bbox=[float(v) for v in boxes[k]], score=float(scores[k]), category=NAME_TO_NUM_NUSC[NUIM_CLASS_NAMES[labels[k]]],
                 cam_id=int(cams[k]), obj_id=i + 1)
        (anno[cams[k]] if is_argo else anno[cams[k]][NUIM_CLASS_NAMES[labels[k]]]).append(a)
        p = plane_of(k)
        if p is not None:
            obj_index.append(k)
            obj_plane.append(p)
            obj_id.append(i + 1)
    obj_index, obj_plane, obj_id = (np.asarray(v, dtype=np.int64) for v in (obj_index, obj_plane, obj_id))
    # the planner emits rows plane by plane in paint order: a stable sort by plane keeps the order inside each plane
    by_plane = np.argsort(obj_plane, kind="stable")
    return MaskPlan(is_argo=is_argo, dets=dets, boxes=boxes, cams=cams, img_shapes=img_shapes, planes_src=planes_src, dst=dst,
                    bbox_only=bool(bbox_only), mask_thr=np.float32(mask_thr), threshold=thr, anno=anno, num_painted=len(painted),
                    obj_index=obj_index[by_plane], obj_plane=obj_plane[by_plane], obj_id=obj_id[by_plane],
                    class_names=class_names)


def bbox_rect(box, shape):
    """(y0, x0, h, w) of the writer's `mask[round(y1):round(y2), round(x1):round(x2)] = True` on an image of `shape`."""
    x1, y1, x2, y2 = (round(np.float32(v)) for v in box)
    ya, yb, _ = slice(y1, y2).indices(shape[0])
    xa, xb, _ = slice(x1, x2).indices(shape[1])
    return ya, xa, max(yb - ya, 0), max(xb - xa, 0)


def _nonzero_crop(mask):
    """(y0, x0, crop) of a host 2-D mask cut to its nonzero rectangle ((0, 0, empty) when none)."""
    rows, cols = np.flatnonzero(mask.any(1)), np.flatnonzero(mask.any(0))
    if len(rows) == 0:
        return 0, 0, np.zeros((0, 0), np.uint8)
    y0, y1, x0, x1 = rows[0], rows[-1] + 1, cols[0], cols[-1] + 1
    return int(y0), int(x0), np.ascontiguousarray(mask[y0:y1, x0:x1]).astype(np.uint8)


def roi_rect(box, shape):
    """(y0, x0, h, w) of the pixels `roi_cover` looks at: rows [max(floor(y0) - 1, 0), min(ceil(y1) + 1, H)), columns likewise
    (mmdet's per-object paste window); (0, 0, 0, 0) for a box that is not finite or has x1 <= x0 or y1 <= y0."""
    x0, y0, x1, y1 = (float(np.float32(v)) for v in box)
    if not all(math.isfinite(v) for v in (x0, y0, x1, y1)) or x1 <= x0 or y1 <= y0:
        return 0, 0, 0, 0
    ya, yb = max(math.floor(y0) - 1, 0), min(math.ceil(y1) + 1, int(shape[0]))
    xa, xb = max(math.floor(x0) - 1, 0), min(math.ceil(x1) + 1, int(shape[1]))
    if yb <= ya or xb <= xa:
        return 0, 0, 0, 0
    return ya, xa, yb - ya, xb - xa


def _roi_taps(centres, lo, hi, m):
    """One axis of `roi_cover`: pixel indices -> (texel index + 1 into a zero-padded map, weight of that texel, weight of the next,
    usable).  Float32, one rounding per operation.  A pixel whose first tap is not in [-1, m) touches no texel: not usable."""
    f = np.float32
    with np.errstate(all="ignore"):
        g = ((centres.astype(f) + f(0.5)) - lo) / (hi - lo) * f(2.0) - f(1.0)
        i = ((g + f(1.0)) * f(m) - f(1.0)) * f(0.5)
        i0 = np.floor(i)
        w1 = i - i0
        w0 = f(1.0) - w1
        ok = (i0 >= f(-1.0)) & (i0 < f(m))  # (False for NaN)
    return np.where(ok, i0, f(-1.0)).astype(np.int64) + 1, w0, w1, ok


def roi_cover(box, roi, thr, shape):
    """The host specification of K34c: mmdet's `_do_paste_mask` + `mask_thr_binary` for one object on an image of `shape`, i.e.
    F.grid_sample(bilinear, align_corners=False, zero padding) of the RoI map `roi` [M, M] over the float32 box (x0, y0, x1, y1),
    thresholded.  Returns (y0, x0, h, w, cover): the candidate rectangle (`roi_rect`) and a bool [h, w] of its covered pixels.
    Float32, one rounding per operation, no contraction, fixed order; for pixel (py, px):
        gx = ((px + 0.5) - x0) / (x1 - x0) * 2 - 1;  ix = ((gx + 1) * M - 1) * 0.5;  ix0 = floor(ix);  wx1 = ix - ix0;  wx0 = 1 - wx1
        v  = m[iy0, ix0] * (wx0 * wy0) + m[iy0, ix0 + 1] * (wx1 * wy0) + m[iy0 + 1, ix0] * (wx0 * wy1) + m[iy0 + 1, ix0 + 1] * (wx1 * wy1)
    summed left to right, a texel outside the map counting 0; covered iff v >= thr (never for a NaN).  A float16 map is widened
    exactly."""
    ya, xa, h, w, v, usable = roi_sample(box, roi, shape)
    with np.errstate(invalid="ignore"):
        return ya, xa, h, w, (v >= np.float32(thr)) & usable


def roi_sample(box, roi, shape):
    """`roi_cover` before its threshold: (y0, x0, h, w, v float32 [h, w], usable bool [h, w]); a pixel that is not usable touches no
    texel (its v is meaningless and it is never covered)."""
    f = np.float32
    ya, xa, h, w = roi_rect(box, shape)
    if h == 0:
        return 0, 0, 0, 0, np.zeros((0, 0), f), np.zeros((0, 0), bool)
    roi = np.asarray(roi)
    m = roi.shape[0]
    assert roi.shape == (m, m)
    x0, y0, x1, y1 = (f(v) for v in box)
    pad = np.zeros((m + 2, m + 2), f)
    pad[1:-1, 1:-1] = roi.astype(f)
    iy, wy0, wy1, oky = _roi_taps(np.arange(ya, ya + h), y0, y1, m)
    ix, wx0, wx1, okx = _roi_taps(np.arange(xa, xa + w), x0, x1, m)
    iy, wy0, wy1, ix, wx0, wx1 = iy[:, None], wy0[:, None], wy1[:, None], ix[None, :], wx0[None, :], wx1[None, :]
    with np.errstate(all="ignore"):
        v = pad[iy, ix] * (wx0 * wy0)
        v = v + pad[iy, ix + 1] * (wx1 * wy0)
        v = v + pad[iy + 1, ix] * (wx0 * wy1)
        v = v + pad[iy + 1, ix + 1] * (wx1 * wy1)
    assert v.dtype == f
    return ya, xa, h, w, v, oky[:, None] & okx[None, :]


def paste_roi_mask(box, roi, thr, shape):
    """`roi_cover` as a full-size bool mask [H, W] (what mmdet's paste hands the offline writer)."""
    ya, xa, h, w, cover = roi_cover(box, roi, thr, shape)
    out = np.zeros(tuple(int(v) for v in shape), bool)
    out[ya:ya + h, xa:xa + w] = cover
    return out


def _mask_form(plan):
    """'rect' (bbox_only), 'crops', 'rois' (RoI maps pasted over the boxes), 'device' (full-size device masks) or 'host' (full-size
    host masks)."""
    d = plan.dets
    if plan.bbox_only:
        return "rect"
    if d.get("mask_crops") is not None:
        return "crops"
    if d.get("mask_rois") is not None:
        return "rois"
    masks = d.get("masks")
    if masks is None:
        raise ValueError("mask detections carry no masks: pass masks / mask_crops, or bbox_only=True")
    first = masks if isinstance(masks, torch.Tensor) else (masks[0] if len(masks) else None)
    return "device" if isinstance(first, torch.Tensor) and first.is_cuda else "host"


def _check_full(plan, k, shape):
    want = plan.img_shapes[int(plan.cams[k])]
    if tuple(shape) != tuple(want):
        raise ValueError(f"object {k}: mask of shape {tuple(shape)} on camera {int(plan.cams[k])} of image size {want}")


def host_geometry(plan):
    """Per painted row (y0, x0, crop) with crop a u8 2-D array, or None for a solid rectangle (bbox_only)."""
    form, d, out = _mask_form(plan), plan.dets, []
    rois = _host(d["mask_rois"]) if form == "rois" and len(plan.obj_index) else None
    for k in plan.obj_index:
        shape = plan.img_shapes[int(plan.cams[k])]
        if form == "rect":
            y0, x0, h, w = bbox_rect(plan.boxes[k], shape)
            out.append((y0, x0, h, w, None))
            continue
        if form == "rois":
            y0, x0, h, w, cover = roi_cover(plan.boxes[k], rois[k], plan.mask_thr, shape)
            out.append((y0, x0, h, w, cover.astype(np.uint8)))
            continue
        if form == "crops":
            crop = np.asarray(_host(d["mask_crops"][k])).astype(np.uint8)
            y0, x0 = (int(v) for v in _host(d["mask_origins"][k]))
            if crop.ndim != 2 or y0 < 0 or x0 < 0 or y0 + crop.shape[0] > shape[0] or x0 + crop.shape[1] > shape[1]:
                raise ValueError(f"object {k}: mask crop {crop.shape} at ({y0}, {x0}) outside the {shape} image")
        else:
            m = _host(d["masks"][k])
            _check_full(plan, k, m.shape)
            y0, x0, crop = _nonzero_crop(m)
        out.append((y0, x0, crop.shape[0], crop.shape[1], crop))
    return out


def _finish(plan, planes, results, loader):
    """Planes (one per output plane, destination size) + anno -> results["mask_data"] / ["mask_anno"], as load_nusc / load_argo."""
    anno = plan.anno
    if plan.is_argo:
        oh, ow = plan.img_shapes[0]
        hf, wf = AV2_PLANE[0] / oh, AV2_PLANE[1] / ow
        loader._scale_cam(results, 0, wf, hf)
        loader._scale_boxes(anno[0], wf, hf)
        if sum(len(c) for c in anno) > loader.obj_max_num:
            raise ValueError(f"{sum(len(c) for c in anno)} anno rows for obj_max_num = {loader.obj_max_num}")
        results["mask_anno"] = loader.reorg_anno_single_cls(anno)
        results["mask_data"] = planes.reshape(AV2_CAMS, 1, *AV2_PLANE)
    else:
        if plan.num_painted > loader.obj_max_num:
            raise ValueError(f"{plan.num_painted} anno rows for obj_max_num = {loader.obj_max_num}")
        results["mask_anno"] = loader.reorg_anno_multi_cls(anno)
        results["mask_data"] = planes.reshape(NUSC_CAMS, len(plan.class_names), *NUSC_IMG)
    return results


def paint_numpy(plan):
    """The host painter (the referee of K34): planes [P, dst_h, dst_w], u8 (nuScenes) or i32 (Argoverse 2), as a torch CPU tensor."""
    geom = host_geometry(plan)
    out = []
    rows_of = {}
    for r, p in enumerate(plan.obj_plane):
        rows_of.setdefault(int(p), []).append(r)
    for p, src in enumerate(plan.planes_src):
        ids = np.zeros(src, dtype=np.int64)
        free = np.ones(src, dtype=bool)
        for r in rows_of.get(p, []):
            y0, x0, h, w, crop = geom[r]
            cover = np.ones((h, w), bool) if crop is None else crop != 0
            take = cover & free[y0:y0 + h, x0:x0 + w]
            ids[y0:y0 + h, x0:x0 + w][take] = plan.obj_id[r]
            free[y0:y0 + h, x0:x0 + w][take] = False
        plane = torch.from_numpy(ids.astype(np.int32 if plan.is_argo else np.uint8))
        out.append(_resize_nearest(plane, plan.dst) if tuple(src) != tuple(plan.dst) else plane)
    return torch.stack(out, 0)


def _upload(arrays, dtypes, device):
    """One pinned host -> device copy of several small arrays (no host wait); returns device views, one per array."""
    blob = np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in arrays])
    dev = torch.from_numpy(blob).pin_memory().to(device, non_blocking=True)
    views, at = [], 0
    for a, dt in zip(arrays, dtypes):
        views.append(dev[at:at + a.nbytes].view(dt))
        at += a.nbytes
    return views


def paint_device(plan, device):
    """K34 (csrc/mask_paint.hip): the same planes on `device`, [P, dst_h, dst_w] u8 / i32.  One upload of the object table (plus one
    of the packed crops for host masks); full-size device masks are measured by K34a and never leave the device.  No host wait."""
    from ... import hip_ops

    device = torch.device(device)
    form, m = _mask_form(plan), len(plan.obj_index)
    if form == "rois":
        return _paint_device_rois(plan, device)
    pitch, src_off = np.zeros(m, np.int64), np.zeros(m, np.int64)
    rects, ext_row = np.zeros((m, 4), np.int64), np.full(m, -1, np.int64)
    masks_dev, groups = None, []
    if form == "device":
        masks = plan.dets["masks"]
        row_of = {int(k): r for r, k in enumerate(plan.obj_index)}
        if isinstance(masks, torch.Tensor):
            stacks = [(masks, range(len(masks)))]
        else:  # a list of 2-D device masks: one stacked copy of the painted ones per image size
            by_shape = {}
            for k in plan.obj_index:
                by_shape.setdefault(tuple(masks[k].shape), []).append(int(k))
            stacks = [(torch.stack([masks[k] for k in ks]), ks) for ks in by_shape.values()]
        flat, index, base = [], [], 0
        for t, ks in stacks:
            t = t.to(device).contiguous()
            t = t.view(torch.uint8) if t.dtype == torch.bool else t.to(torch.uint8)
            h, w = t.shape[-2:]
            first = len(index)
            for i, k in enumerate(ks):
                r = row_of.get(int(k))
                if r is None:
                    continue
                _check_full(plan, k, (h, w))
                pitch[r], src_off[r], ext_row[r] = w, base + i * h * w, len(index)
                index.append(i)
            groups.append((t, first, len(index)))
            flat.append(t.reshape(-1))
            base += t.numel()
        masks_dev = flat[0] if len(flat) == 1 else torch.cat(flat)
    else:
        crops, nbytes = [], 0
        for r, (y0, x0, h, w, crop) in enumerate(host_geometry(plan)):
            if crop is None:
                rects[r] = (y0, x0, h, w)
            elif crop.size:
                rects[r] = (y0, x0, h, w)
                pitch[r], src_off[r] = w, nbytes - y0 * w - x0  # the "virtual" offset of the plane's pixel (0, 0)
                crops.append(crop.reshape(-1))
                nbytes += crop.size
        if crops:
            masks_dev = torch.from_numpy(np.concatenate(crops)).pin_memory().to(device, non_blocking=True)
    num_planes = len(plan.planes_src)
    table = np.zeros((m, 8), dtype=np.int32)
    table[:, 0], table[:, 1:5], table[:, 5], table[:, 6], table[:, 7] = plan.obj_plane, rects, pitch, ext_row, plan.obj_id
    plane_ptr = np.searchsorted(plan.obj_plane, np.arange(num_planes + 1)).astype(np.int32)
    src_hw = np.asarray(plan.planes_src, dtype=np.int32).reshape(num_planes, 2)
    scale = (src_hw / np.asarray(plan.dst, dtype=np.float64)).astype(np.float32)  # f32(h / dst_h): _resize_nearest's factor
    index = np.asarray(index if form == "device" else [], dtype=np.int32)
    d_off, d_table, d_ptr, d_hw, d_scale, d_index = _upload(
        [src_off, table, plane_ptr, src_hw, scale, index], [torch.int64, torch.int32, torch.int32, torch.int32, torch.float32, torch.int32],
        device)
    extents = None
    if groups:
        extents = torch.empty((max(len(index), 1), 4), dtype=torch.int32, device=device)
        for t, a, b in groups:
            if b > a:
                hip_ops.mask_extents(t, d_index[a:b], out=extents[a:b])
    return hip_ops.paint_instance_masks(d_table.view(-1, 8), d_off, d_ptr, d_hw, d_scale, plan.dst,
                                        torch.int32 if plan.is_argo else torch.uint8, masks=masks_dev, extents=extents)


def _paint_device_rois(plan, device):
    """K34c (fsf_paint_roi_masks): the `mask_rois` form painted in one launch, no full-size mask in between.  Table rows carry the
    candidate rectangle (`roi_rect`) and point into the RoI buffer by element offset: a device tensor is read where it lies (painted
    rows only, no gather copy), host maps of the painted rows ride in the table's one pinned upload.  K34a does not run; no host wait."""
    from ... import hip_ops_mask

    m, rois = len(plan.obj_index), plan.dets["mask_rois"]
    side = int(rois.shape[1])
    rects = np.zeros((m, 4), np.int64)
    for r, k in enumerate(plan.obj_index):
        rects[r] = roi_rect(plan.boxes[k], plan.img_shapes[int(plan.cams[k])])
    num_planes = len(plan.planes_src)
    table = np.zeros((m, 8), dtype=np.int32)
    table[:, 0], table[:, 1:5], table[:, 6], table[:, 7] = plan.obj_plane, rects, -1, plan.obj_id
    plane_ptr = np.searchsorted(plan.obj_plane, np.arange(num_planes + 1)).astype(np.int32)
    src_hw = np.asarray(plan.planes_src, dtype=np.int32).reshape(num_planes, 2)
    scale = (src_hw / np.asarray(plan.dst, dtype=np.float64)).astype(np.float32)  # f32(h / dst_h): _resize_nearest's factor
    boxes = np.ascontiguousarray(plan.boxes[plan.obj_index], dtype=np.float32).reshape(m, 4)
    arrays = [None, table, plane_ptr, src_hw, scale, boxes]
    dtypes = [torch.int64, torch.int32, torch.int32, torch.int32, torch.float32, torch.float32]
    if isinstance(rois, torch.Tensor) and rois.is_cuda:
        rois_dev = rois.detach().to(device).contiguous()
        arrays[0] = plan.obj_index.astype(np.int64) * (side * side)
    else:
        picked = np.ascontiguousarray(_host(rois)[plan.obj_index]).reshape(m, side, side)
        arrays[0] = np.arange(m, dtype=np.int64) * (side * side)
        arrays.append(picked)
        dtypes.append(torch.float16 if picked.dtype == np.float16 else torch.float32)
    views = _upload(arrays, dtypes, device)
    if len(views) == 7:
        rois_dev = views[6]
    d_off, d_table, d_ptr, d_hw, d_scale, d_boxes = views[:6]
    return hip_ops_mask.paint_roi_masks(d_table.view(-1, 8), d_boxes.view(-1, 4), d_off, d_ptr, d_hw, d_scale, plan.dst,
                                        torch.int32 if plan.is_argo else torch.uint8, rois_dev, side, float(plan.mask_thr))


@PIPELINES.register_module(force=True)
class PaintMasksFromDetections:
    """`mask_data` / `mask_anno` from `results["mask_detections"]` (a 2-D segmenter's output of this frame), equal to what
    LoadMaskFromFiles returns for the reference writer's files.  Argoverse 2 also reads `results["mask_img_shapes"]` (the (h, w) of
    each camera image; or `img_shapes` in the packed detections) and scales lidar2img[0] as load_argo does.  `device`: paint with
    K34 on that device (mask_data stays there); None: the host painter.  `mask_thr`: the threshold on pasted `mask_rois` (mmdet's
    mask_thr_binary)."""

    def __init__(self, class_names=["car", "truck", "trailer", "bus", "construction_vehicle", "bicycle", "motorcycle", "pedestrian",
                                     "traffic_cone", "barrier"], obj_max_num=250, is_argo=False, is_waymo=False, score_thr_init=None,
                 topk=None, bbox_only=False, device=None, mask_thr=0.5):
        if is_waymo:
            raise NotImplementedError("Waymo: the reference has no mask writer to reproduce")
        self.loader = LoadMaskFromFiles(None, class_names=class_names, obj_max_num=obj_max_num, is_argo=is_argo)
        self.class_names, self.is_argo = class_names, is_argo
        self.score_thr_init, self.topk, self.bbox_only, self.device = score_thr_init, topk, bbox_only, device
        if not float(mask_thr) > 0.0:
            raise ValueError(f"mask_thr must be above 0, got {mask_thr}")
        self.mask_thr = mask_thr

    def plan(self, results):
        dets = results["mask_detections"]
        shapes = results.get("mask_img_shapes", dets.get("img_shapes") if isinstance(dets, dict) else None)
        return plan_masks(dets, is_argo=self.is_argo, class_names=self.class_names, img_shapes=shapes,
                          score_thr_init=self.score_thr_init, topk=self.topk, bbox_only=self.bbox_only, mask_thr=self.mask_thr)

    def __call__(self, results):
        plan = self.plan(results)
        planes = paint_numpy(plan) if self.device is None else paint_device(plan, self.device)
        return _finish(plan, planes, results, self.loader)
