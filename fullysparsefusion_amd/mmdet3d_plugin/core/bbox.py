"""Box-side pieces the heads need at inference:

* `BasePointBBoxCoder` — projects/mmdet3d_plugin/core/bbox/coders/base_point_bbox_coder.py:8-82.
* `LiDARInstance3DBoxes`, `xywhr2xyxyr`, `box3d_multiclass_nms`, `nms_gpu`, `nms_normal_gpu`, `bbox3d2result` — the
  handful of mmdet3d 0.x [UNVENDORED] symbols imported at
  projects/mmdet3d_plugin/models/dense_heads/frustum_cluster_head.py:9 and detectors/FSF.py (bbox3d2result), restated
  from their published behaviour.  The NMS itself is the HIP kernel pair behind `fsf_nms_bev` (K20): the greedy scan
  stays on the device instead of mmdet3d's bitmask-to-host round trip.
"""
import numpy as np
import torch

from ... import hip_ops
from ..registry import BBOX_CODERS


@BBOX_CODERS.register_module(force=True)
class BasePointBBoxCoder:
    """reg = (center - base_point, log(dims), sin(yaw), cos(yaw)[, vx, vy])."""

    def __init__(self, post_center_range=None, score_thresh=0.1, num_classes=10, max_num=500, code_size=10):
        self.post_center_range = post_center_range
        self.code_size = code_size
        self.EPS = 1e-6
        self.score_thresh = score_thresh
        self.num_classes = num_classes
        self.max_num = max_num

    def encode(self, bboxes, base_points):
        assert bboxes.size(1) in (7, 9, 10), f"bboxes shape: {bboxes.shape}"
        assert bboxes.size(0) == base_points.size(0)
        yaw = bboxes[:, 6:7]
        target = torch.cat([bboxes[:, :3] - base_points, (bboxes[:, 3:6] + self.EPS).log(), yaw.sin(), yaw.cos()], dim=1)
        if bboxes.size(1) in (9, 10):  # velocity (or copy-paste flag) rides along
            assert self.code_size == 10
            target = torch.cat([target, bboxes[:, [7, 8]]], dim=1)
        return target

    def decode(self, reg_preds, base_points, detach_yaw=False):
        assert reg_preds.size(1) in (8, 10) and reg_preds.size(1) == self.code_size
        velo = reg_preds[:, -2:] if self.code_size == 10 else None
        reg = reg_preds[:, :8]
        dims = reg[:, 3:6].exp() - self.EPS
        xyz = reg[:, :3] + base_points
        yaw = torch.atan2(reg[:, 6:7], reg[:, 7:8])
        if detach_yaw:
            yaw = yaw.clone().detach()
        parts = [xyz, dims, yaw] + ([velo] if velo is not None else [])
        return torch.cat(parts, dim=1)


def box_corners_host(boxes7):
    """f32 [M, >= 7] rows (x, y, z_bottom, w, l, h, yaw) -> f32 [M, 8, 3]: the vertices of the solid the containment test
    (`points_in_boxes_first_host`, csrc/box_contain.h) tests.  Vertex v: bit 2 -> +l/2 along (cos yaw, sin yaw), bit 1 -> +w/2 across,
    bit 0 -> the top face."""
    b = boxes7.float()
    yaw = b[:, 6].detach().cpu().double()
    c, s = torch.cos(yaw).float().to(b.device), torch.sin(yaw).float().to(b.device)
    hw, hl, top = b[:, 3] * 0.5, b[:, 4] * 0.5, b[:, 2] + b[:, 5]
    out = []
    for v in range(8):
        dx = hl if v & 4 else -hl
        dy = hw if v & 2 else -hw
        out.append(torch.stack([(b[:, 0] + dx * c) - dy * s, (b[:, 1] + dx * s) + dy * c, top if v & 1 else b[:, 2]], 1))
    return torch.stack(out, 1)


class LiDARInstance3DBoxes:
    """mmdet3d 0.x LiDAR boxes, as far as the FSF heads touch them: rows (x, y, z_bottom, w, l, h, yaw[, extras])."""

    def __init__(self, tensor, box_dim=7, with_yaw=True, origin=(0.5, 0.5, 0)):
        if not isinstance(tensor, torch.Tensor):
            tensor = torch.as_tensor(tensor, dtype=torch.float32)
        if tensor.numel() == 0:
            tensor = tensor.reshape((0, box_dim)).to(dtype=torch.float32)
        assert tensor.dim() == 2 and tensor.size(-1) == box_dim, tensor.size()
        if tensor.shape[-1] == 6:
            assert box_dim == 6
            tensor = torch.cat((tensor, tensor.new_zeros(tensor.shape[0], 1)), dim=-1)
            box_dim, with_yaw = 7, False
        self.box_dim, self.with_yaw = box_dim, with_yaw
        self.tensor = tensor.clone()
        if tuple(origin) != (0.5, 0.5, 0):
            self.tensor[:, :3] += self.tensor[:, 3:6] * (self.tensor.new_tensor((0.5, 0.5, 0)) - self.tensor.new_tensor(origin))

    @classmethod
    def _wrap(cls, tensor, box_dim, with_yaw=True):
        """The boxes AS `tensor` (no copy, no origin shift): for rows that were just produced for this object alone."""
        self = cls.__new__(cls)
        self.box_dim, self.with_yaw, self.tensor = box_dim, with_yaw, tensor
        return self

    @property
    def bev(self):
        return self.tensor[:, [0, 1, 3, 4, 6]]

    @property
    def gravity_center(self):
        c = self.tensor[:, :3].clone()
        c[:, 2] = c[:, 2] + self.tensor[:, 5] * 0.5
        return c

    @property
    def corners(self):
        """f32 [M, 8, 3]: the vertices of the solid the containment test tests (`box_corners_host`)."""
        return box_corners_host(self.tensor[:, :7])

    @property
    def dims(self):
        return self.tensor[:, 3:6]

    @property
    def yaw(self):
        return self.tensor[:, 6]

    @property
    def device(self):
        return self.tensor.device

    def __len__(self):
        return self.tensor.shape[0]

    def __getitem__(self, item):
        if isinstance(item, int):
            return type(self)(self.tensor[item].view(1, -1), box_dim=self.box_dim, with_yaw=self.with_yaw)
        return type(self)(self.tensor[item], box_dim=self.box_dim, with_yaw=self.with_yaw)

    def to(self, device):
        return type(self)(self.tensor.to(device), box_dim=self.box_dim, with_yaw=self.with_yaw)

    def clone(self):
        return type(self)(self.tensor.clone(), box_dim=self.box_dim, with_yaw=self.with_yaw)

    @classmethod
    def cat(cls, boxes_list):
        assert isinstance(boxes_list, (list, tuple))
        if len(boxes_list) == 0:
            return cls(torch.empty(0))
        assert all(isinstance(b, cls) for b in boxes_list)
        return cls(torch.cat([b.tensor for b in boxes_list], dim=0), box_dim=boxes_list[0].tensor.shape[1],
                   with_yaw=boxes_list[0].with_yaw)

    def __repr__(self):
        return self.__class__.__name__ + "(\n    " + str(self.tensor) + ")"


def xywhr2xyxyr(boxes_xywhr):
    """(x, y, w, h, r) -> (x - w/2, y - h/2, x + w/2, y + h/2, r)."""
    boxes = torch.zeros_like(boxes_xywhr)
    half_w, half_h = boxes_xywhr[:, 2] / 2, boxes_xywhr[:, 3] / 2
    boxes[:, 0] = boxes_xywhr[:, 0] - half_w
    boxes[:, 1] = boxes_xywhr[:, 1] - half_h
    boxes[:, 2] = boxes_xywhr[:, 0] + half_w
    boxes[:, 3] = boxes_xywhr[:, 1] + half_h
    boxes[:, 4] = boxes_xywhr[:, 4]
    return boxes


def _nms(boxes, scores, thresh, rotated, pre_maxsize=None, post_max_size=None):
    order = scores.sort(0, descending=True)[1]
    if pre_maxsize is not None:
        order = order[:pre_maxsize]
    keep = hip_ops.nms_bev(boxes[order].float().contiguous(), thresh, rotated=rotated)
    keep = order[keep].contiguous()
    if post_max_size is not None:
        keep = keep[:post_max_size]
    return keep


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, post_max_size=None):
    """mmdet3d.ops.iou3d.nms_gpu: rotated BEV NMS; boxes (x1, y1, x2, y2, ry); returns kept indices into `boxes`."""
    return _nms(boxes, scores, thresh, True, pre_maxsize, post_max_size)


def nms_normal_gpu(boxes, scores, thresh):
    """mmdet3d.ops.iou3d.nms_normal_gpu: the same with the yaw ignored."""
    return _nms(boxes, scores, thresh, False)


def box3d_multiclass_nms(mlvl_bboxes, mlvl_bboxes_for_nms, mlvl_scores, score_thr, max_num, cfg):
    """mmdet3d.core.post_processing.box3d_multiclass_nms (the arguments the FSF heads pass): per class, threshold ->
    BEV NMS -> concatenate class by class; over max_num keep the best scores.  The last score column is the padded
    background.  Upstream runs one nms_gpu per class (each with its own host round trip); here every class goes through
    ONE `fsf_nms_bev_multiclass` call and there is a single device->host read (how many boxes survived)."""
    num_classes = mlvl_scores.shape[1] - 1
    n = mlvl_scores.shape[0]
    if n == 0 or num_classes == 0:
        return (mlvl_scores.new_zeros((0, mlvl_bboxes.size(-1))), mlvl_scores.new_zeros((0,)),
                mlvl_scores.new_zeros((0,), dtype=torch.long))
    st = mlvl_scores[:, :num_classes].t().contiguous()                      # [C, n]
    valid = st > score_thr
    order = torch.where(valid, st, st.new_full((), float("-inf"))).sort(dim=1, descending=True, stable=True)[1]
    count = valid.sum(1, dtype=torch.int32)
    pos = torch.arange(n, device=st.device, dtype=torch.int32).expand(num_classes, n)
    rank = torch.empty_like(pos).scatter_(1, order, pos)
    rank = torch.where(valid, rank, rank.new_full((), -1))
    cap = int(max_num) if max_num is not None and max_num > 0 else 0  # (only the best max_num survive below)
    boxes_nms = mlvl_bboxes_for_nms.float()
    rotated = bool(cfg.get("use_rotate_nms", False))
    if cap > 0:
        # per-class masks over each class's best-scoring window only; a class that runs out of window before `cap` keeps
        # (checked after the host sync the compaction below needs anyway) repeats the call on full masks
        keep, num, incomplete = hip_ops.nms_bev_multiclass(boxes_nms, rank, count, cfg["nms_thr"], rotated=rotated, max_keep=cap,
                                                           windowed=True)
    else:
        keep, num = hip_ops.nms_bev_multiclass(boxes_nms, rank, count, cfg["nms_thr"], rotated=rotated)
        incomplete = None
    kept = (torch.arange(n, device=st.device)[None, :] < num[:, None]).nonzero(as_tuple=False)  # class-major, score order
    if incomplete is not None and bool(incomplete.item()):
        keep, num = hip_ops.nms_bev_multiclass(boxes_nms, rank, count, cfg["nms_thr"], rotated=rotated, max_keep=cap)
        kept = (torch.arange(n, device=st.device)[None, :] < num[:, None]).nonzero(as_tuple=False)
    labels = kept[:, 0]
    box_idx = order[labels, keep[labels, kept[:, 1]]]
    bboxes, scores = mlvl_bboxes[box_idx], st[labels, box_idx]
    if bboxes.shape[0] > max_num:
        inds = scores.sort(descending=True)[1][:max_num]
        bboxes, labels, scores = bboxes[inds, :], labels[inds], scores[inds]
    return bboxes, scores, labels


def bbox3d2result(bboxes, scores, labels, attrs=None):
    """mmdet3d.core.bbox3d2result: results on the host, the form the dataset evaluators take."""
    t = getattr(bboxes, "tensor", None)
    hr = getattr(bboxes, "_host_rows", None)  # (boxes | score | label) rows already on the host (the fused box tail's one read-back)
    if (hr is not None and t is not None and attrs is None and hr[1] is t and t._version == hr[2] and hr[3] is scores
            and scores._version == hr[4] and hr[5] is labels and labels._version == hr[6]):
        # ... and still what the device tensors hold: the very tensors the box tail returned, un-edited since
        host = hr[0]
        c = t.size(1)
        return dict(boxes_3d=type(bboxes)._wrap(host[:, :c].contiguous(), c, getattr(bboxes, "with_yaw", True)),
                    scores_3d=host[:, c].contiguous(), labels_3d=host[:, c + 1].to(labels.dtype))
    if t is not None and t.is_cuda and t.dtype == torch.float32 and scores.dtype == torch.float32 and labels.numel() == len(t):
        # one device -> host transfer instead of three (class indices are exact in fp32)
        packed = torch.cat([t, scores[:, None], labels[:, None].to(torch.float32)], dim=1).cpu()
        c = t.size(1)
        host_boxes = bboxes.to("cpu") if len(t) == 0 else type(bboxes)(packed[:, :c].contiguous(), box_dim=c, with_yaw=getattr(bboxes, "with_yaw", True))
        result = dict(boxes_3d=host_boxes, scores_3d=packed[:, c].contiguous(), labels_3d=packed[:, c + 1].to(labels.dtype))
    else:
        result = dict(boxes_3d=bboxes.to("cpu"), scores_3d=scores.cpu(), labels_3d=labels.cpu())
    if attrs is not None:
        result["attrs_3d"] = attrs.cpu()
    return result


# ------------------------------------------------------------------------------ test-time augmentation (K33)
def _bev_corners(b):
    """xyxyr [n, 5] (float64) -> [n, 4, 2]: the corners iou3d rotates (`rotate_around_center`: by -yaw about the centre)."""
    cx, cy = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
    c, s = torch.cos(b[:, 4]), torch.sin(b[:, 4])
    out = []
    for ix, iy in ((0, 1), (2, 1), (2, 3), (0, 3)):
        dx, dy = b[:, ix] - cx, b[:, iy] - cy
        out.append(torch.stack([dx * c + dy * s + cx, -dx * s + dy * c + cy], -1))
    return torch.stack(out, 1)


def _clip_area(p, q):
    """Area of the intersection of two convex quadrilaterals (lists of (x, y); Sutherland-Hodgman)."""
    def area(poly):
        return 0.5 * abs(sum(poly[i][0] * poly[i - 1][1] - poly[i - 1][0] * poly[i][1] for i in range(len(poly))))

    orient = 1.0 if sum(q[i - 1][0] * q[i][1] - q[i][0] * q[i - 1][1] for i in range(4)) > 0 else -1.0
    out = list(p)
    for i in range(4):
        a, b = q[i - 1], q[i]
        side = lambda v: orient * ((b[0] - a[0]) * (v[1] - a[1]) - (b[1] - a[1]) * (v[0] - a[0]))  # noqa: E731
        inp, out = out, []
        for j in range(len(inp)):
            cur, prev = inp[j], inp[j - 1]
            sc, sp = side(cur), side(prev)
            if sc >= 0:
                if sp < 0:
                    t = sp / (sp - sc)
                    out.append((prev[0] + t * (cur[0] - prev[0]), prev[1] + t * (cur[1] - prev[1])))
                out.append(cur)
            elif sp >= 0:
                t = sp / (sp - sc)
                out.append((prev[0] + t * (cur[0] - prev[0]), prev[1] + t * (cur[1] - prev[1])))
        if not out:
            return 0.0
    return area(out)


def bev_iou_host(a, b, rotated=True):
    """BEV IoU of xyxyr rows a [n, 5] and b [m, 5] in float64 on the host (the overlap iou3d's nms_gpu / nms_normal_gpu test)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    if not rotated:
        w = (torch.minimum(a[:, None, 2], b[None, :, 2]) - torch.maximum(a[:, None, 0], b[None, :, 0])).clamp(min=0)
        h = (torch.minimum(a[:, None, 3], b[None, :, 3]) - torch.maximum(a[:, None, 1], b[None, :, 1])).clamp(min=0)
        inter = w * h
    else:
        ca, cb = _bev_corners(a).tolist(), _bev_corners(b).tolist()
        inter = torch.tensor([[_clip_area(p, q) for q in cb] for p in ca], dtype=torch.float64).reshape(len(ca), len(cb))
    return inter / (area_a[:, None] + area_b[None, :] - inter).clamp(min=1e-8)


def _nms_host(boxes_xyxyr, scores, thresh, rotated):
    """Greedy NMS on the host: stable descending score order (ties: ascending index), suppress IoU > thresh."""
    order = scores.sort(descending=True, stable=True)[1]
    b = boxes_xyxyr[order]
    iou = bev_iou_host(b, b, rotated)
    removed = torch.zeros(len(order), dtype=torch.bool)
    keep = []
    for i in range(len(order)):
        if removed[i]:
            continue
        keep.append(i)
        removed[i + 1:] |= iou[i, i + 1:] > thresh
    return order[torch.tensor(keep, dtype=torch.long)]


def bbox3d_mapping_back(bboxes, scale_factor, flip_horizontal, flip_vertical, rot_factor=0.0):
    """mmdet3d's bbox3d_mapping_back [UNVENDORED mmdet3d.core.bbox.transforms] plus the rotation the reference's TTA adds: undo
    the vertical flip, the horizontal flip, the scale (x fp32(1 / s)), then the rotation (centre and velocity by -angle, yaw + angle:
    this box convention turns yaw clockwise).  fp32, the arithmetic of K33b (csrc/augment.hip)."""
    from ..datasets.pipelines import augmentation_descriptor

    t = getattr(bboxes, "tensor", bboxes).clone()
    c, s, inv, angle, rot, _, _ = augmentation_descriptor(rot_factor, scale_factor, flip_horizontal, flip_vertical, inverse=True)
    vel = t.size(1) >= 9
    if flip_vertical:
        t[:, 0] = -t[:, 0]
        if vel:
            t[:, 7] = -t[:, 7]
        t[:, 6] = -t[:, 6]
    if flip_horizontal:
        t[:, 1] = -t[:, 1]
        if vel:
            t[:, 8] = -t[:, 8]
        t[:, 6] = -t[:, 6] + float(np.float32(np.pi))
    t[:, :6] *= inv
    t[:, 7:] *= inv
    if rot:
        for i, j in ((0, 1), (7, 8)) if vel else ((0, 1),):
            x, y = t[:, i].clone(), t[:, j].clone()
            t[:, i] = (x * c) + (y * s)
            t[:, j] = (y * c) - (x * s)
        t[:, 6] = t[:, 6] + angle
    if isinstance(bboxes, LiDARInstance3DBoxes):
        return type(bboxes)(t, box_dim=t.size(1), with_yaw=bboxes.with_yaw)
    return t


def _meta0(meta):
    return meta[0] if isinstance(meta, (list, tuple)) else meta


def merge_aug_bboxes_3d(aug_results, img_metas, test_cfg):
    """mmdet3d's merge_aug_bboxes_3d [UNVENDORED mmdet3d.core.post_processing.merge_augs] on the host — the readable spec of
    `merge_aug_bboxes_3d_device` and the route for CPU tensors / configurations the device path does not take.
      aug_results  one bbox3d2result dict per pass (boxes_3d, scores_3d, labels_3d) in the pass's augmented frame;
      img_metas    one meta dict (or mmdet3d's one-element list of it) per pass: pcd_scale_factor, pcd_horizontal_flip,
                   pcd_vertical_flip, pcd_rot_factor (absent: 0);
      test_cfg     nms_thr, use_rotate_nms, max_num.
    Every pass's boxes are mapped back (`bbox3d_mapping_back`), concatenated, class-wise BEV NMS'ed (class by class, ascending
    class id), then sorted by descending score and cut to max_num.  Ties: both sorts are stable, so equal scores keep
    class-major order and, inside a class, concatenation (pass, then row) order — mmdet3d's unstable sort leaves them open."""
    assert len(aug_results) == len(img_metas)
    get = test_cfg.get if isinstance(test_cfg, dict) else lambda k, d=None: getattr(test_cfg, k, d)
    boxes, scores, labels, box_dim = [], [], [], None
    for res, meta in zip(aug_results, img_metas):
        m = _meta0(meta)
        t = getattr(res["boxes_3d"], "tensor", res["boxes_3d"])
        if len(t) == 0:
            continue
        box_dim = t.size(1)
        boxes.append(bbox3d_mapping_back(t.float().cpu(), m.get("pcd_scale_factor", 1.0), m.get("pcd_horizontal_flip", False),
                                         m.get("pcd_vertical_flip", False), m.get("pcd_rot_factor", 0.0)))
        scores.append(res["scores_3d"].float().cpu())
        labels.append(res["labels_3d"].long().cpu())
    if not boxes:
        t0 = getattr(aug_results[0]["boxes_3d"], "tensor", aug_results[0]["boxes_3d"])
        d = t0.size(1) if t0.dim() == 2 else 7
        return dict(boxes_3d=LiDARInstance3DBoxes(torch.zeros((0, d)), box_dim=d), scores_3d=torch.zeros(0),
                    labels_3d=torch.zeros(0, dtype=torch.long))
    aug_boxes, aug_scores, aug_labels = torch.cat(boxes), torch.cat(scores), torch.cat(labels)
    for_nms = xywhr2xyxyr(aug_boxes[:, [0, 1, 3, 4, 6]])
    rotated = bool(get("use_rotate_nms", False))
    mb, ms, ml = [], [], []
    for class_id in range(int(aug_labels.max()) + 1):
        idx = (aug_labels == class_id).nonzero(as_tuple=True)[0]
        if len(idx) == 0:
            continue
        sel = idx[_nms_host(for_nms[idx], aug_scores[idx], float(get("nms_thr")), rotated)]
        mb.append(aug_boxes[sel])
        ms.append(aug_scores[sel])
        ml.append(aug_labels[sel])
    mb, ms, ml = torch.cat(mb), torch.cat(ms), torch.cat(ml)
    order = ms.sort(descending=True, stable=True)[1][: min(int(get("max_num")), len(aug_boxes))]
    return dict(boxes_3d=LiDARInstance3DBoxes(mb[order].contiguous(), box_dim=box_dim), scores_3d=ms[order].contiguous(),
                labels_3d=ml[order].contiguous())


def merge_aug_bboxes_3d_device(boxes, scores, labels, pass_idx, img_metas, test_cfg, num_classes):
    """`merge_aug_bboxes_3d` on the device, for the concatenated per-pass results (boxes f32 [m, 7 | 9], scores f32 [m], labels
    i64 [m], pass index i32 [m]): K33b (map back + NMS form + class-major scores), K24's class ranks, K20's capped class-wise NMS,
    K24's selection, a stable score sort of the <= max_num rows — and ONE read-back.  Returns the bbox3d2result dict (host)."""
    from ..datasets.pipelines import meta_descriptor

    get = test_cfg.get if isinstance(test_cfg, dict) else lambda k, d=None: getattr(test_cfg, k, d)
    max_num = int(get("max_num"))
    d = boxes.size(1)
    descs = [meta_descriptor(_meta0(m), inverse=True) for m in img_metas]
    out, for_nms, scores_t = hip_ops.aug_boxes_map_back(boxes, scores, labels, pass_idx, descs, num_classes)
    order, rank, count = hip_ops.class_rank_desc(scores_t, float("-inf"))
    keep, num, incomplete = hip_ops.nms_bev_multiclass(for_nms, rank, count, float(get("nms_thr")),
                                                       rotated=bool(get("use_rotate_nms", False)), max_keep=max_num, windowed=True)
    buf = hip_ops.nms_select(out, scores_t, order, keep, num, max_num, max_num, None, incomplete)
    w = d + 2
    rows = buf[: max_num * w].view(max_num, w)
    meta = buf[max_num * w:].view(torch.int32)
    valid = torch.arange(max_num, device=buf.device) < meta[0]
    key = torch.where(valid, rows[:, d], rows.new_full((), float("-inf")))
    rows = rows[key.sort(descending=True, stable=True)[1]]  # (nms_select: class-major when <= max_num kept; merge: by score)
    host = torch.cat([rows.reshape(-1), buf[max_num * w:]]).cpu()  # the merge's one read-back
    hm = host[max_num * w:].view(torch.int32)
    if int(hm[2]) != 0:  # a class ran out of its mask window before max_num keeps: full masks (never expected at TTA sizes)
        keep, num = hip_ops.nms_bev_multiclass(for_nms, rank, count, float(get("nms_thr")), rotated=bool(get("use_rotate_nms", False)),
                                               max_keep=max_num)
        buf = hip_ops.nms_select(out, scores_t, order, keep, num, max_num, max_num, None, None)
        rows = buf[: max_num * w].view(max_num, w)
        valid = torch.arange(max_num, device=buf.device) < buf[max_num * w:].view(torch.int32)[0]
        key = torch.where(valid, rows[:, d], rows.new_full((), float("-inf")))
        rows = rows[key.sort(descending=True, stable=True)[1]]
        host = torch.cat([rows.reshape(-1), buf[max_num * w:]]).cpu()
        hm = host[max_num * w:].view(torch.int32)
    k = int(hm[0])
    r = host[: max_num * w].view(max_num, w)[:k]
    return dict(boxes_3d=LiDARInstance3DBoxes._wrap(r[:, :d].contiguous(), d), scores_3d=r[:, d].contiguous(),
                labels_3d=r[:, d + 1].long())
