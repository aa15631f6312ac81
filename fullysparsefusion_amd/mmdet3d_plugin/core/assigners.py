"""The camera-query head's label assigners: `HybridAssigner` (projects/mmdet3d_plugin/core/bbox/assigners/hybrid_assigner.py),
`PointInBoxAssigner` (point_assigner.py) and mmdet 2.14 `MaxIoUAssigner` with `BboxOverlaps2D`; and the refine heads':
`FrustumAssigner` (frustum_assigner.py) = `HybridAssigner` + `DistAssigner` (dist_assigner.py), on the device through K38
(docs/kernels/K38_frustum_assign.md: `fsf_frustum_assign`, the distance step inside K37b's per-query kernel).

The classes hold the configuration under the upstream constructor arguments and assign ONE sample on the host (`assign`): that is the
unfused path and the restatement the kernels are pinned to.  The training step itself goes through K37
(docs/kernels/K37_hybrid_assign.md: `fsf_gt_boxes_2d` + `fsf_hybrid_assign`, the whole batch in five launches and no host wait).

Pinned arithmetic of the host functions, which K37 reproduces bit for bit:
* corners: half sizes, cos / sin(yaw) in float64 rounded to f32 once, `(x + dx c) - dy s`, `(y + dx s) + dy c` in separately rounded
  f32 operations; the solid is the one `points_in_boxes_first_host` tests (length l along (cos yaw, sin yaw), width w across, z .. z + h);
* projection: the fma chain of K13 (`acc = x m0; acc = fma(y, m1, acc); ...`), depth clipped to [1e-5, 1e5] before the divide;
* the clip of the hull of the eight points against the canvas in float64, every operation rounded separately: the Liang-Barsky clip
  of the 28 point pairs plus the canvas corners that lie inside a triangle of the points; rounded to f32 once;
* IoU in f32: area (x2 - x1)(y2 - y1), intersection sides clamped at 0, union floored at 1e-6.
shapely (upstream's hull and intersection) and mmdet are not needed; tests/test_hybrid_assign_cpu.py compares with scipy's hull."""
import itertools

import torch

from ..registry import BBOX_ASSIGNERS
from .bbox import box_corners_host

CANVAS = (1600.0, 900.0)  # post_process_coords: imsize = (1600, 900)
_PAIRS = list(itertools.combinations(range(8), 2))
_TRIANGLES = list(itertools.combinations(range(8), 3))


class AssignResult:
    """mmdet's AssignResult as far as the heads read it: gt_inds i64 [n] (0 background, k + 1 = GT k), labels i64 [n] (-1 none)."""

    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels


# ----------------------------------------------------------------------------------------------------- geometry on the host
def _fma32(a, b, c):
    """f32 fma through float64 (the product of two f32 values is exact there)."""
    return (a.double() * b.double() + c.double()).float()


def project_corners_host(corners, lidar2img):
    """`prj_lidar_bbox3d_on_img`: corners f32 [M, 8, 3], lidar2img f32 [4, 4] -> (pts f32 [M, 8, 2], valid bool [M])."""
    m = lidar2img.float()
    x, y, z = corners[..., 0], corners[..., 1], corners[..., 2]
    rows = []
    for j in range(3):
        acc = x * m[j, 0]
        acc = _fma32(y, m[j, 1], acc)
        acc = _fma32(z, m[j, 2], acc)
        rows.append(_fma32(torch.ones_like(x), m[j, 3], acc))
    u, v, d = rows
    valid = (d > 1e-5).any(1)
    d = d.clamp(1e-5, 1e5)
    return torch.stack([u / d, v / d], -1), valid


def clip_hull_bbox_host(pts, canvas=CANVAS):
    """Bounding box of (convex hull of the 8 points, clipped to [0, W] x [0, H]) without building the hull: pts f32 [P, 8, 2] ->
    (box f64 [P, 4], found bool [P]).  float64, one rounding per operation."""
    p = pts.double()
    big = float("inf")
    W, H = float(canvas[0]), float(canvas[1])
    i_idx = torch.tensor([i for i, _ in _PAIRS])
    j_idx = torch.tensor([j for _, j in _PAIRS])
    ax, ay, bx, by = p[:, i_idx, 0], p[:, i_idx, 1], p[:, j_idx, 0], p[:, j_idx, 1]
    dx, dy = bx - ax, by - ay
    t0, t1 = torch.zeros_like(ax), torch.ones_like(ax)
    ok = torch.ones_like(ax, dtype=torch.bool)
    for ps, qs in ((-dx, ax), (dx, W - ax), (-dy, ay), (dy, H - ay)):
        zero = ps == 0
        ok = ok & ~(zero & (qs < 0))
        r = qs / torch.where(zero, torch.ones_like(ps), ps)
        neg, pos = ~zero & (ps < 0), ~zero & (ps > 0)
        ok = ok & ~(neg & (r > t1)) & ~(pos & (r < t0))
        t0 = torch.where(neg, torch.maximum(t0, r), t0)
        t1 = torch.where(pos, torch.minimum(t1, r), t1)
    # (a surviving end point is taken as it is; an interpolated point lies inside the canvas up to its rounding: clamped onto it)
    x_in, y_in = torch.where(t0 == 0, ax, (ax + t0 * dx).clamp(0.0, W)), torch.where(t0 == 0, ay, (ay + t0 * dy).clamp(0.0, H))
    x_out, y_out = torch.where(t1 == 1, bx, (ax + t1 * dx).clamp(0.0, W)), torch.where(t1 == 1, by, (ay + t1 * dy).clamp(0.0, H))
    xs, ys, mask = [x_in, x_out], [y_in, y_out], [ok, ok]
    t_i, t_j, t_l = (torch.tensor([t[k] for t in _TRIANGLES]) for k in range(3))

    def cross(a, b, cx, cy):
        return (p[:, b, 0] - p[:, a, 0]) * (cy - p[:, a, 1]) - (p[:, b, 1] - p[:, a, 1]) * (cx - p[:, a, 0])

    for cx, cy in ((0.0, 0.0), (W, 0.0), (W, H), (0.0, H)):
        d1, d2, d3 = cross(t_i, t_j, cx, cy), cross(t_j, t_l, cx, cy), cross(t_l, t_i, cx, cy)
        same = ((d1 >= 0) & (d2 >= 0) & (d3 >= 0)) | ((d1 <= 0) & (d2 <= 0) & (d3 <= 0))
        inside = (same & ~((d1 == 0) & (d2 == 0) & (d3 == 0))).any(1, keepdim=True)
        xs.append(torch.full_like(inside, cx, dtype=torch.float64))
        ys.append(torch.full_like(inside, cy, dtype=torch.float64))
        mask.append(inside)
    xs, ys, mask = torch.cat(xs, 1), torch.cat(ys, 1), torch.cat(mask, 1)
    found = mask.any(1)
    lo = lambda v: torch.where(mask, v, torch.full_like(v, big)).min(1)[0]  # noqa: E731
    hi = lambda v: torch.where(mask, v, torch.full_like(v, -big)).max(1)[0]  # noqa: E731
    box = torch.stack([lo(xs), lo(ys), hi(xs), hi(ys)], 1)
    return torch.where(found[:, None], box, torch.zeros_like(box)), found


def gt_boxes_2d_host(boxes, lidar2img, canvas=CANVAS, labels=None):
    """`get_gt_bboxes_2d` for every camera at once: GT rows f32 [M, >= 7], lidar2img f32 [ncam, 4, 4] -> (boxes_2d f32 [M, ncam, 4],
    keep bool [M, ncam]).  A box is dropped for a camera when no corner has depth > 1e-5, when the hull of its projected corners misses
    the canvas, or when the clipped box has no width or height (upstream raises there); rows with label < 0 are dropped everywhere."""
    rows = getattr(boxes, "tensor", boxes).float().cpu()
    lidar2img = torch.as_tensor(lidar2img).float().cpu()
    m, ncam = rows.shape[0], lidar2img.shape[0]
    out, keep = torch.zeros((m, ncam, 4)), torch.zeros((m, ncam), dtype=torch.bool)
    if m == 0:
        return out, keep
    corners = box_corners_host(rows[:, :7])
    for cam in range(ncam):
        pts, valid = project_corners_host(corners, lidar2img[cam])
        box, found = clip_hull_bbox_host(pts, canvas)
        k = valid & found & (box[:, 2] > box[:, 0]) & (box[:, 3] > box[:, 1])
        if labels is not None:
            k = k & (torch.as_tensor(labels).reshape(-1).cpu() >= 0)
        keep[:, cam] = k
        out[:, cam] = torch.where(k[:, None], box, torch.zeros_like(box)).float()
    return out, keep


def bbox_overlaps_host(gt, dt, eps=1e-6):
    """mmdet 2.14 `bbox_overlaps(gt, dt, mode='iou')` in f32: -> [G, Q]."""
    gt, dt = gt.float(), dt.float()
    area_g = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    area_d = (dt[:, 2] - dt[:, 0]) * (dt[:, 3] - dt[:, 1])
    lt = torch.max(gt[:, None, :2], dt[None, :, :2])
    rb = torch.min(gt[:, None, 2:], dt[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    union = torch.max((area_g[:, None] + area_d[None, :]) - overlap, overlap.new_tensor(eps))
    return overlap / union


def max_iou_assign_host(overlaps, pos_iou_thr, min_pos_iou, match_low_quality=True, gt_max_assign_all=True):
    """`MaxIoUAssigner.assign_wrt_overlaps` on overlaps f32 [G, Q] -> i64 [Q]: the assigned GT row, -1 for background and for mmdet's
    ignore band alike (the callers copy positives only).  Ties for a query's maximum go to the first GT."""
    g, q = overlaps.shape
    assigned = torch.full((q,), -1, dtype=torch.long, device=overlaps.device)
    if g == 0 or q == 0:
        return assigned
    thr = lambda v: torch.tensor(v, dtype=torch.float32, device=overlaps.device)  # noqa: E731
    mx = overlaps.max(0)[0]
    idx = torch.arange(g, device=overlaps.device)[:, None].expand(g, q)
    arg = torch.where(overlaps == mx[None], idx, torch.full_like(idx, g)).min(0)[0]
    pos = mx >= thr(pos_iou_thr)
    assigned[pos] = arg[pos]
    if match_low_quality:
        gmx = overlaps.max(1)[0]
        for j in range(g):  # ascending: a later GT overrides an earlier one, and the >= pos_iou_thr assignment
            if gmx[j] >= thr(min_pos_iou):
                if gt_max_assign_all:
                    assigned[overlaps[j] == gmx[j]] = j
                else:
                    assigned[int(torch.where(overlaps[j] == gmx[j])[0][0])] = j
    return assigned


def enlarge_box_height(boxes7, extra_height):
    """`PointInBoxAssigner.enlarge_box_height`: h + 2e, z_bottom - e."""
    if not extra_height:
        return boxes7
    out = boxes7.clone()
    out[:, 5] += extra_height * 2
    out[:, 2] -= extra_height
    return out


def query_camera(preds_2d):
    """The camera of every query: column 6 of preds_2d (bbox 0..3, score, category, cam id, obj id, valid)."""
    return preds_2d[:, 6]


# ----------------------------------------------------------------------------------------------------- the assigners
@BBOX_ASSIGNERS.register_module()
class PointInBoxAssigner:
    def __init__(self, extra_height=0.0):
        self.extra_height = extra_height

    def assign_rows(self, cluster_xyz, boxes7):
        """Index of the first box containing each centre, -1 when none."""
        from ..models.decode_heads.segmentation_head import points_in_boxes_first_host

        return points_in_boxes_first_host(cluster_xyz[:, :3], enlarge_box_height(boxes7[:, :7].float(), self.extra_height))

    def assign(self, cluster_xyz, old_reg_preds, gt_bboxes_3d, gt_labels):
        n, num_gts = cluster_xyz.size(0), gt_bboxes_3d.size(0)
        gt_inds = cluster_xyz.new_zeros((n,), dtype=torch.long)
        labels = cluster_xyz.new_full((n,), -1, dtype=torch.long)
        if num_gts > 0 and n > 0:
            inbox = self.assign_rows(cluster_xyz, gt_bboxes_3d)
            pos = inbox > -1
            gt_inds[pos] = inbox[pos] + 1
            labels[pos] = gt_labels.long()[inbox[pos]]
        return AssignResult(num_gts, gt_inds, None, labels=labels)


@BBOX_ASSIGNERS.register_module()
class MaxIoUAssigner:
    def __init__(self, pos_iou_thr, neg_iou_thr, min_pos_iou=0.0, gt_max_assign_all=True, ignore_iof_thr=-1, ignore_wrt_candidates=True,
                 match_low_quality=True, gpu_assign_thr=-1, iou_calculator=dict(type="BboxOverlaps2D")):
        self.pos_iou_thr, self.neg_iou_thr, self.min_pos_iou = pos_iou_thr, neg_iou_thr, min_pos_iou
        self.gt_max_assign_all, self.ignore_iof_thr, self.ignore_wrt_candidates = gt_max_assign_all, ignore_iof_thr, ignore_wrt_candidates
        self.match_low_quality, self.gpu_assign_thr = match_low_quality, gpu_assign_thr
        if dict(iou_calculator).get("type") != "BboxOverlaps2D" or len(dict(iou_calculator)) != 1:
            raise NotImplementedError(f"MaxIoUAssigner: iou_calculator {iou_calculator} is not built (BboxOverlaps2D only)")
        self.iou_calculator = dict(iou_calculator)

    def assign_rows(self, bboxes, gt_bboxes):
        """Assigned GT row per box, -1 for negatives and the ignore band."""
        return max_iou_assign_host(bbox_overlaps_host(gt_bboxes[:, :4], bboxes[:, :4]), self.pos_iou_thr, self.min_pos_iou,
                                   self.match_low_quality, self.gt_max_assign_all)

    def assign(self, bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None):
        if gt_bboxes_ignore is not None and self.ignore_iof_thr > 0:
            raise NotImplementedError("MaxIoUAssigner: ignore_iof_thr with gt_bboxes_ignore is not used by the FSF configs and is not built")
        rows = self.assign_rows(bboxes, gt_bboxes)
        overlaps = bbox_overlaps_host(gt_bboxes[:, :4], bboxes[:, :4])
        gt_inds = rows + 1
        if overlaps.numel():  # mmdet marks the ignore band -1 and the negatives 0; the positives are what the heads read
            mx = overlaps.max(0)[0]
            band = (rows < 0) & ~((mx >= 0) & (mx < torch.tensor(self.neg_iou_thr, dtype=torch.float32)))
            gt_inds[band] = -1
        labels = None
        if gt_labels is not None:
            labels = gt_inds.new_full((bboxes.size(0),), -1)
            labels[rows >= 0] = gt_labels.long()[rows[rows >= 0]]
        return AssignResult(gt_bboxes.size(0), gt_inds, overlaps.max(0)[0] if overlaps.numel() else None, labels=labels)


@BBOX_ASSIGNERS.register_module()
class HybridAssigner:
    """3-D containment first; the queries it leaves unassigned take a GT whose image projection their 2-D box overlaps."""

    def __init__(self, assigner_2d=None, assigner_3d=None, assigner_dist=None, num_cams=6,
                 class_names=["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
                              "traffic_cone"], tasks=None, is_frustum=False):
        self.assigner_2d = BBOX_ASSIGNERS.build(assigner_2d) if assigner_2d is not None else None
        self.assigner_3d = BBOX_ASSIGNERS.build(assigner_3d) if assigner_3d is not None else None
        self.assigner_dist = BBOX_ASSIGNERS.build(assigner_dist) if assigner_dist is not None else None
        self.num_cams, self.class_names, self.tasks, self.is_frustum = num_cams, class_names, tasks, is_frustum

    def check(self, who="HybridAssigner"):
        """What no FSF config sets for the camera-query head is refused by name, not approximated."""
        if self.is_frustum:
            raise NotImplementedError(f"{who}: is_frustum=True is not used by the FSF configs and is not built")
        self._check_dist(who)
        if type(self.assigner_3d) is not PointInBoxAssigner or type(self.assigner_2d) is not MaxIoUAssigner:
            raise NotImplementedError(f"{who}: assigner_3d must be a PointInBoxAssigner and assigner_2d a MaxIoUAssigner (both set)")
        a = self.assigner_2d
        if not a.match_low_quality or not a.gt_max_assign_all:
            raise NotImplementedError(f"{who}: match_low_quality=False / gt_max_assign_all=False are not used by the FSF configs and are not built")
        if a.ignore_iof_thr > 0:
            raise NotImplementedError(f"{who}: ignore_iof_thr > 0 is not used by the FSF configs and is not built")

    def _check_dist(self, who):
        if self.assigner_dist is not None:
            raise NotImplementedError(f"{who}: assigner_dist is the refine heads' (FrustumAssigner + DistAssigner) and is not built "
                                      "into a HybridAssigner")

    def assign_2d_rows(self, preds_2d, no_aug_rows, lidar2img, canvas=CANVAS):
        """`assign_2d` for one sample: -> (row of the un-augmented GT per query or -1, boxes_2d, keep)."""
        n = preds_2d.shape[0]
        out = torch.full((n,), -1, dtype=torch.long)
        lidar2img = torch.as_tensor(lidar2img).float()[:self.num_cams]
        boxes_2d, keep = gt_boxes_2d_host(no_aug_rows, lidar2img, canvas)
        if no_aug_rows.shape[0] == 0 or n == 0:
            return out, boxes_2d, keep
        cams = query_camera(preds_2d).cpu()
        for cam in range(lidar2img.shape[0]):
            kept = torch.nonzero(keep[:, cam]).reshape(-1)
            mine = torch.nonzero(cams == cam).reshape(-1)
            if kept.numel() == 0 or mine.numel() == 0:
                continue
            rows = self.assigner_2d.assign_rows(preds_2d[mine, :4].cpu(), boxes_2d[kept, cam])
            out[mine[rows >= 0]] = kept[rows[rows >= 0]]
        return out, boxes_2d, keep

    def assign_rows(self, preds_2d, no_aug_rows, cluster_xyz, gt_rows, lidar2img, canvas=CANVAS):
        """One sample, GT already in the task's order: -> dict(final, rows_3d, rows_2d i64 [n]: a row of the AUGMENTED list or -1;
        boxes_2d, keep).  A 2-D match names a row of the un-augmented list; the same row of the augmented list is taken, and a row
        beyond its end leaves the query background (upstream would index out of range)."""
        self.check()
        rows_3d = self.assigner_3d.assign_rows(cluster_xyz.cpu().float(), gt_rows.cpu().float()) if gt_rows.shape[0] \
            else torch.full((cluster_xyz.shape[0],), -1, dtype=torch.long)
        rows_2d, boxes_2d, keep = self.assign_2d_rows(preds_2d, no_aug_rows.cpu().float(), lidar2img, canvas)
        rows_2d = torch.where(rows_2d < gt_rows.shape[0], rows_2d, torch.full_like(rows_2d, -1))
        final = torch.where(rows_3d >= 0, rows_3d, rows_2d)
        return dict(final=final, rows_3d=rows_3d, rows_2d=rows_2d, boxes_2d=boxes_2d, keep=keep)

    def assign(self, preds_2d, no_aug_gt_bboxes_3d, no_aug_gt_labels_3d, cluster_xyz, old_cluster_logits, old_reg_preds, gt_bboxes_3d,
               gt_labels_3d, img_metas, task_id):
        """Upstream's signature for one sample: -> (final, 3-D, 2-D) `AssignResult`s; labels are the augmented list's."""
        gt_rows = getattr(gt_bboxes_3d, "tensor", gt_bboxes_3d)
        na_rows = getattr(no_aug_gt_bboxes_3d, "tensor", no_aug_gt_bboxes_3d)
        r = self.assign_rows(preds_2d, na_rows, cluster_xyz, gt_rows, img_metas["lidar2img"])
        labels = torch.as_tensor(gt_labels_3d).long().cpu()

        def result(rows):
            lab = torch.full_like(rows, -1)
            lab[rows >= 0] = labels[rows[rows >= 0]]
            return AssignResult(gt_rows.shape[0], rows + 1, None, labels=lab)

        return result(r["final"]), result(r["rows_3d"]), result(r["rows_2d"])


# ----------------------------------------------------------------------------------------------------- the refine heads' (K38)
def bev_distance_host(query_xy, gt_xy):
    """BEV distances f32 [n, M] with the arithmetic pinned as K38 computes it: dx = qx - gx, dy = qy - gy, fl(fl(dx dx) + fl(dy dy))
    (no fma), a correctly rounded square root: the float64 root of an f32 value rounds to the correctly rounded f32 root, which
    ATen's f32 sqrt need not be.  Upstream's `torch.cdist` is this up to its matmul form (docs/kernels/K38)."""
    q, g = query_xy.float(), gt_xy.float()
    dx, dy = q[:, None, 0] - g[None, :, 0], q[:, None, 1] - g[None, :, 1]
    return (dx * dx + dy * dy).double().sqrt().float()


def first_argmax_host(logits, num_classes):
    """Arg-max of columns 0 .. num_classes - 1 by a strict `>` scan from column 0: the lowest index wins a tie, a row of NaN gives 0."""
    logits = logits.float()
    n = logits.shape[0]
    arg = torch.zeros((n,), dtype=torch.long, device=logits.device)
    if n == 0:
        return arg
    top = logits[:, 0].clone()
    for j in range(1, num_classes):
        better = logits[:, j] > top
        top = torch.where(better, logits[:, j], top)
        arg = torch.where(better, torch.full_like(arg, j), arg)
    return arg


class _ScopeFromCheck:
    """`OUT_OF_SCOPE` for the assigners whose scope depends on their configuration (the stand-ins' is a class constant)."""

    @property
    def OUT_OF_SCOPE(self):
        """True when this instance's configuration is one `check()` refuses."""
        try:
            self.check()
        except NotImplementedError:
            return True
        return False


@BBOX_ASSIGNERS.register_module()
class DistAssigner(_ScopeFromCheck):
    """`DistAssigner` (core/bbox/assigners/dist_assigner.py): a query takes the nearest GT, in BEV, of the class its logits predict,
    when that GT is closer than the class's radius.  Upstream's constructor arguments; all default to None so that a config naming the
    class alone still builds (and is refused by `check`)."""

    def __init__(self, assign_tasks=None, class_names=None, max_dist=None):
        self.tasks, self.class_names, self.max_dist = assign_tasks, class_names, max_dist
        self.num_tasks = len(assign_tasks) if assign_tasks is not None else 0

    def check(self, who="DistAssigner"):
        """One class per assign task, every class at most once: upstream's mapping back from the per-task index to the GT list is
        inconsistent for anything else, which is refused by name."""
        if self.tasks is None or self.class_names is None or self.max_dist is None:
            raise NotImplementedError(f"{who}: assign_tasks, class_names and max_dist must all be set")
        if len(self.max_dist) != len(self.tasks):
            raise NotImplementedError(f"{who}: max_dist needs one entry per assign_tasks entry")
        seen = set()
        for task, dist in zip(self.tasks, self.max_dist):
            names = list(task["class_names"])
            if len(names) != 1:
                raise NotImplementedError(f"{who}: assign_tasks entries with more than one class ({names}) are not built: upstream maps "
                                          "their per-task indices back to the GT list inconsistently")
            if names[0] in seen:
                raise NotImplementedError(f"{who}: class '{names[0]}' is named in two assign_tasks entries, which is not built")
            if names[0] not in self.class_names:
                raise NotImplementedError(f"{who}: class '{names[0]}' of assign_tasks is not in class_names")
            if len(dist) != 1:
                raise NotImplementedError(f"{who}: max_dist needs one radius per class of its assign_tasks entry")
            seen.add(names[0])

    def class_table(self, num_task_classes=None):
        """f32 [C]: the radius of every class of `class_names` (the first `num_task_classes`), 0 for a class in no assign task."""
        self.check()
        c = len(self.class_names) if num_task_classes is None else int(num_task_classes)
        radius = {task["class_names"][0]: float(dist[0]) for task, dist in zip(self.tasks, self.max_dist)}
        return torch.tensor([radius.get(name, 0.0) for name in list(self.class_names)[:c]] + [0.0] * max(0, c - len(self.class_names)),
                            dtype=torch.float32)

    def assign_rows(self, cluster_xyz, cluster_logits, gt_rows, gt_labels):
        """One sample: query centres [n, >= 2], their logits [n, >= C], GT rows [M, >= 2] with labels i64 [M] (indices into
        `class_names`; rows < 0 are skipped) -> i64 [n]: the assigned GT row or -1."""
        n, m = cluster_xyz.shape[0], gt_rows.shape[0]
        out = torch.full((n,), -1, dtype=torch.long)
        if n == 0 or m == 0:
            return out
        table = self.class_table()
        c = table.numel()
        labels = torch.as_tensor(gt_labels).long().reshape(-1).cpu()
        pred = first_argmax_host(cluster_logits.detach().cpu()[:, :c], c)
        d = bev_distance_host(cluster_xyz.detach().cpu()[:, :2], gt_rows.detach().cpu()[:, :2])
        d = torch.where(torch.isfinite(d) & (labels[None, :] == pred[:, None]), d, torch.full_like(d, float("inf")))
        near = d.min(1)[0]
        idx = torch.arange(m)[None, :].expand(n, m)
        arg = torch.where(d == near[:, None], idx, torch.full_like(idx, m)).min(1)[0]  # the first row of minimum distance
        ok = near < table[pred]  # (inf, the marker of "no candidate", compares false)
        out[ok] = arg[ok]
        return out

    def assign(self, cluster_xyz, cluster_logits, gt_bboxes_3d, gt_labels):
        """Upstream's signature for one sample (labels are indices into `class_names`)."""
        rows = getattr(gt_bboxes_3d, "tensor", gt_bboxes_3d)
        labels = torch.as_tensor(gt_labels).long().reshape(-1).cpu()
        hit = self.assign_rows(cluster_xyz, cluster_logits, rows, labels)
        lab = torch.zeros_like(hit)  # (upstream's combine_assign_result starts from zeros)
        lab[hit >= 0] = labels[hit[hit >= 0]]
        return AssignResult(rows.shape[0], hit + 1, None, labels=lab)


@BBOX_ASSIGNERS.register_module()
class FrustumAssigner(HybridAssigner, _ScopeFromCheck):
    """`FrustumAssigner` (core/bbox/assigners/frustum_assigner.py): `HybridAssigner`'s two steps, then `assigner_dist` for the queries
    they left unassigned.  Without an `assigner_dist` it is the hybrid assignment."""

    def __init__(self, assigner_2d=None, assigner_3d=None, assigner_dist=None, num_cams=6,
                 class_names=["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
                              "traffic_cone"], tasks=None, is_frustum=False, vis_dir=None, ignore_bev_dist=None):
        super().__init__(assigner_2d, assigner_3d, assigner_dist, num_cams, class_names, tasks, is_frustum)
        self.vis_dir, self.ignore_bev_dist = vis_dir, ignore_bev_dist

    def check(self, who="FrustumAssigner", head_tasks=None, head_class_names=None):
        """`head_tasks` / `head_class_names`: the tasks and class names of the head that owns the assigner, held to the same rule as
        the assigner's own (`_check_labels`)."""
        if self.vis_dir is not None:
            raise NotImplementedError(f"{who}: vis_dir (upstream's debugging pictures) is not built")
        if self.ignore_bev_dist is not None:
            raise NotImplementedError(f"{who}: ignore_bev_dist is not used by the FSF configs and is not built")
        super().check(who)
        if head_tasks is not None or head_class_names is not None:
            self._check_labels(who, head_tasks, head_class_names)

    def _check_dist(self, who):
        dist = self.assigner_dist
        if dist is None:
            return
        if type(dist) is not DistAssigner:
            raise NotImplementedError(f"{who}: assigner_dist must be a DistAssigner, not a {type(dist).__name__}")
        dist.check(f"{who}: DistAssigner")
        self._check_labels(who, self.tasks, self.class_names)

    def _check_labels(self, who, tasks, class_names):
        """DistAssigner compares task-local labels with indices into its own class_names: one task of exactly those names."""
        dist = self.assigner_dist
        if dist is None:
            return
        if tasks is None or len(tasks) != 1 or class_names is None or list(tasks[0]["class_names"]) != list(class_names) \
                or list(dist.class_names) != list(class_names):
            raise NotImplementedError(f"{who}: assigner_dist needs task-local labels that are the global class indices (a single task "
                                      "whose class_names equal the head's, the assigner's and the DistAssigner's); anything else is "
                                      "not built")

    def assign_rows(self, preds_2d, no_aug_rows, cluster_xyz, gt_rows, lidar2img, canvas=CANVAS, old_cls_logits=None, gt_labels=None):
        """`HybridAssigner.assign_rows` plus rows_dist (the distance step's row for EVERY query, -1 none) and source i64 [n]
        (0 none, 1 3-D, 2 2-D, 3 distance); `final` takes the distance row where both other steps gave none."""
        self.check()
        r = HybridAssigner.assign_rows(self, preds_2d, no_aug_rows, cluster_xyz, gt_rows, lidar2img, canvas)
        n = cluster_xyz.shape[0]
        rows_dist = torch.full((n,), -1, dtype=torch.long)
        if self.assigner_dist is not None:
            if old_cls_logits is None or gt_labels is None:
                raise ValueError("FrustumAssigner.assign_rows: the distance step needs old_cls_logits and gt_labels")
            rows_dist = self.assigner_dist.assign_rows(cluster_xyz, old_cls_logits, gt_rows, gt_labels)
        final = torch.where(r["final"] >= 0, r["final"], rows_dist)
        source = torch.where(r["rows_3d"] >= 0, 1, torch.where(r["rows_2d"] >= 0, 2, torch.where(rows_dist >= 0, 3, 0)))
        r.update(final=final, rows_dist=rows_dist, source=source.long())
        return r

    def assign(self, preds_2d, no_aug_gt_bboxes_3d, no_aug_gt_labels_3d, cluster_xyz, old_cluster_logits, old_reg_preds, gt_bboxes_3d,
               gt_labels_3d, img_metas, task_id):
        """Upstream's signature for one sample: -> (final, 3-D, 2-D) `AssignResult`s; labels are the augmented list's."""
        gt_rows = getattr(gt_bboxes_3d, "tensor", gt_bboxes_3d)
        na_rows = getattr(no_aug_gt_bboxes_3d, "tensor", no_aug_gt_bboxes_3d)
        labels = torch.as_tensor(gt_labels_3d).long().cpu()
        r = self.assign_rows(preds_2d, na_rows, cluster_xyz, gt_rows, img_metas["lidar2img"], old_cls_logits=old_cluster_logits,
                             gt_labels=labels)

        def result(rows):
            lab = torch.full_like(rows, -1)
            lab[rows >= 0] = labels[rows[rows >= 0]]
            return AssignResult(gt_rows.shape[0], rows + 1, None, labels=lab)

        return result(r["final"]), result(r["rows_3d"]), result(r["rows_2d"])
