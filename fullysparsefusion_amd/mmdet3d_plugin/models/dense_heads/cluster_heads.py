"""Query heads, inference side: `SparseClusterHead` (projects/mmdet3d_plugin/models/dense_heads/sparse_cluster_head.py
:18-115, split_by_batch :269-278), `FSDSeparateHead` / `SparseClusterHeadV2` (sparse_cluster_head_v2.py:18-167,
get_bboxes :447-608) and `FrustumClusterHead` (frustum_cluster_head.py:19-95, get_bboxes :500-697).

Same constructor arguments, sub-module names (state-dict keys `shared_mlp.*`, `task_heads.N.<attr>.*`) and return
conventions.  The MLPs are the fused Linear -> LayerNorm+GELU blocks of ops/sst_ops.py; box decoding is the coder of
core/bbox.py; NMS is the HIP kernel pair K20.

Training side: `SparseClusterHeadV2.loss` (sparse_cluster_head_v2.py:170-439 with sparse_cluster_head.py:364-397,459-463) — the
LiDAR-query head's targets and losses, on the device through K36 (docs/kernels/K36_cluster_losses.md): `fsf_cluster_targets` assigns
every cluster centre the first GT box of its sample that contains it (K35a's pinned containment test) and encodes the box,
`fsf_cluster_loss_forward` / `_backward` are the sigmoid focal loss + the L1 groups.  `cluster_targets_host` and
`loss(..., fused=False)` are the torch restatement the kernels are checked against.  `SparseClusterHead.loss` (v1) is not built.

`FrustumClusterHead.loss` (frustum_cluster_head.py:96-462) — the camera-query head's: the same losses on the targets of the hybrid
3-D / 2-D assignment (`HybridAssigner`, core/assigners.py), on the device through K37 (docs/kernels/K37_hybrid_assign.md):
`fsf_gt_boxes_2d` projects and clips the un-augmented GT into every camera, `fsf_hybrid_assign` assigns and encodes.
`hybrid_targets_host` is its restatement.

The refine stages' heads are the same class with a `FrustumAssigner`: the hybrid assignment plus `DistAssigner`'s third step (a query
both steps left unassigned takes the nearest GT, in BEV, of the class the previous stage predicted for it, inside the class's radius),
on the device through K38 (docs/kernels/K38_frustum_assign.md: `fsf_frustum_assign`, the step folded into K37b's per-query kernel).
`frustum_targets_host` is its restatement.  A head with neither assigner raises.
"""
from .... import switches
import copy
import os

import torch
import torch.nn as nn

from .... import hip_ops
from ...core.assigners import CANVAS, FrustumAssigner, HybridAssigner
from ...core.bbox import BasePointBBoxCoder, LiDARInstance3DBoxes, box3d_multiclass_nms, xywhr2xyxyr
from ...ops.sst_ops import build_mlp
from ...registry import BBOX_ASSIGNERS, BBOX_CODERS, HEADS, build_head, build_loss
from ..decode_heads.segmentation_head import gt_box_rows, pack_gt_for_device, points_in_boxes_first_host
from ..losses import FocalLoss, L1Loss


def _cfg_get(cfg, key, default=None):
    if cfg is None:
        return default
    return cfg.get(key, default)


# ----------------------------------------------------------------------------------------------------- K36: targets on the host
def regroup_gt_for_task(boxes, labels, class_lut, num_task_classes):
    """`modify_gt_for_single_task_single_sample` with static shapes: the sample's rows regrouped class by class in the order of the
    task's class names (original order inside a class; a stable sort on the index inside the task), labels replaced by that index.
    Rows of classes outside the task and rows with label < 0 are keyed last and labelled -1 (every consumer skips them), so nothing
    here depends on the values: no host wait for device-resident GT.  -> (boxes [M, D], task labels i64 [M])."""
    labels = labels.reshape(-1).long()
    lut = class_lut if torch.is_tensor(class_lut) else torch.tensor(class_lut, dtype=torch.long)  # (i64 [num classes], where labels is)
    known = (labels >= 0) & (labels < lut.numel())
    key = torch.where(known, lut[labels.clamp(0, lut.numel() - 1)], torch.full_like(labels, -1))
    key = torch.where(key < 0, torch.full_like(key, num_task_classes), key)
    key, order = torch.sort(key, stable=True)
    return boxes[order], torch.where(key < num_task_classes, key, torch.full_like(key, -1))


def enlarge_box_rows(boxes7, width):
    """mmdet3d 0.x `LiDARInstance3DBoxes.enlarged_box`: dims + 2 * width, z_bottom - width."""
    if not width:
        return boxes7
    out = boxes7.clone()
    out[:, 3:6] += width * 2
    out[:, 2] -= width
    return out


def encode_box_targets_host(boxes, base_points, code_size):
    """`BasePointBBoxCoder.encode` with the arithmetic pinned as K36a computes it: the centre delta one f32 subtraction (box columns
    0..2 as stored), log(f32(dim + 1e-6)) and sin / cos(yaw) in float64 rounded to f32 once (on the CPU whatever the boxes' device),
    plus box columns 7, 8 when code_size is 10."""
    boxes = boxes.float()
    assert boxes.shape[1] in (7, 9, 10) and (boxes.shape[1] == 7) == (code_size == 8), f"bboxes shape: {tuple(boxes.shape)}"
    dims = (boxes[:, 3:6] + 1e-6).detach().cpu().double().log().float().to(boxes.device)
    yaw = boxes[:, 6:7].detach().cpu().double()
    parts = [boxes[:, :3] - base_points.float(), dims, yaw.sin().float().to(boxes.device), yaw.cos().float().to(boxes.device)]
    if code_size == 10:
        parts.append(boxes[:, 7:9])
    return torch.cat(parts, dim=1)


def cluster_targets_host(cluster_xyz, batch_idx, gt_rows_list, gt_task_labels_list, num_task_classes, code_size, enlarge_width=None):
    """`get_targets` / `get_targets_single` / `assign_single` (PseudoSampler, point-in-box assignment) for one task on GT that is
    already in the task's order: -> (labels i64 [n], label_weights f32 [n], bbox_targets f32 [n, code], bbox_weights f32 [n, code],
    assigned i64 [n] = index of the box inside its sample's valid rows or -1, stats f32 [6] = (num_preds, num_pos_preds, num_gts,
    assigned_gts, cls_avg_factor, reg_avg_factor) as totals over the batch).  Rows with label < 0 are dropped first."""
    return _targets_from_assignment_host(
        cluster_xyz, batch_idx, gt_rows_list, gt_task_labels_list, num_task_classes, code_size,
        lambda b, centres, rows: points_in_boxes_first_host(centres, enlarge_box_rows(rows[:, :7], enlarge_width)))


def _targets_from_assignment_host(cluster_xyz, batch_idx, gt_rows_list, gt_task_labels_list, num_task_classes, code_size, assign_fn):
    """The part of `get_targets_single` every query head shares (PseudoSampler, the coder, the copy-paste flag, the log scalars):
    `assign_fn(b, centres f32 [m, 3], rows f32 [M, D]) -> i64 [m]` names each centre's row of sample b's valid GT, or -1."""
    xyz = cluster_xyz[:, :3].float()
    n, dev = xyz.shape[0], xyz.device
    labels = torch.full((n,), num_task_classes, dtype=torch.long, device=dev)
    label_weights = xyz.new_ones(n)
    bbox_targets = xyz.new_zeros((n, code_size))
    bbox_weights = xyz.new_zeros((n, code_size))
    assigned = torch.full((n,), -1, dtype=torch.long, device=dev)
    num_gts = assigned_gts = 0
    for b, (rows, task_labels) in enumerate(zip(gt_rows_list, gt_task_labels_list)):
        rows = gt_box_rows(rows).to(dev).float()
        task_labels = torch.as_tensor(task_labels).to(dev).long().reshape(-1)
        assert rows.shape[0] == task_labels.shape[0]
        valid = task_labels >= 0
        rows, task_labels = rows[valid], task_labels[valid]
        num_gts += int(rows.shape[0])
        mine = torch.nonzero(batch_idx == b, as_tuple=False).reshape(-1)
        if rows.shape[0] == 0 or mine.numel() == 0:
            continue
        centres = xyz[mine]
        inbox = assign_fn(b, centres, rows).to(dev)
        pos = inbox > -1
        pos_inds, pos_gt = mine[pos], inbox[pos]
        assigned[pos_inds] = pos_gt
        assigned_gts += int(pos_gt.unique().numel())
        labels[pos_inds] = task_labels[pos_gt]
        bbox_weights[pos_inds] = 1.0
        if pos_inds.numel() > 0:
            pos_rows = rows[pos_gt]
            bbox_targets[pos_inds] = encode_box_targets_host(pos_rows, centres[pos], code_size)
            if pos_rows.size(1) == 10:  # zero velocity loss weight for pasted objects
                assert pos_rows[:, 9].max().item() in (0, 1) and pos_rows[:, 9].min().item() in (0, 1)
                assert bbox_weights.size(1) == 10, "It is not safe to use -2: as follows if size(1) != 10"
                bbox_weights[pos_inds, -2:] = pos_rows[:, [9]]
    assert (labels >= 0).all()
    num_pos = int((labels < num_task_classes).sum())
    stats = torch.tensor([n, num_pos, num_gts, assigned_gts, n, num_pos], dtype=torch.float32, device=dev)
    return labels, label_weights, bbox_targets, bbox_weights, assigned, stats


def hybrid_targets_host(assigner, cluster_xyz, batch_idx, preds_2d, no_aug_rows_list, no_aug_labels_list, gt_rows_list,
                        gt_task_labels_list, lidar2img, num_task_classes, code_size, canvas=None, return_parts=False):
    """`FrustumClusterHead.get_targets` / `get_targets_single` with `HybridAssigner.assign` for one task on GT that is already in the
    task's order (both lists): the tuple of `cluster_targets_host`, from the merged 3-D / 2-D assignment on the AUGMENTED GT.
    `lidar2img` f32 [B, ncam, 4, 4].  The restatement K37 agrees with bit for bit.  With `return_parts` also a list of the per-sample
    dicts of `HybridAssigner.assign_rows` (2-D boxes, keep flags, the 3-D and 2-D rows)."""
    return _hybrid_targets_host(assigner, cluster_xyz, batch_idx, preds_2d, no_aug_rows_list, no_aug_labels_list, gt_rows_list,
                                gt_task_labels_list, lidar2img, num_task_classes, code_size, None, canvas, return_parts)


def frustum_targets_host(assigner, cluster_xyz, batch_idx, preds_2d, no_aug_rows_list, no_aug_labels_list, gt_rows_list,
                         gt_task_labels_list, lidar2img, num_task_classes, code_size, old_cls_logits=None, canvas=None,
                         return_parts=False):
    """`hybrid_targets_host` for a `FrustumAssigner`: the same tuple from the merged 3-D / 2-D / distance assignment.
    `old_cls_logits` [n, >= num_task_classes] are the previous stage's logits of this task (needed when the assigner has an
    `assigner_dist`; without one the result is `hybrid_targets_host`'s).  The restatement K38 agrees with bit for bit.  The per-sample
    dicts of `return_parts` also hold `rows_dist` and `source` (0 none, 1 3-D, 2 2-D, 3 distance) for the sample's queries."""
    if assigner.assigner_dist is not None and old_cls_logits is None:
        raise ValueError("frustum_targets_host: an assigner with an assigner_dist needs old_cls_logits")
    return _hybrid_targets_host(assigner, cluster_xyz, batch_idx, preds_2d, no_aug_rows_list, no_aug_labels_list, gt_rows_list,
                                gt_task_labels_list, lidar2img, num_task_classes, code_size, old_cls_logits, canvas, return_parts)


def _hybrid_targets_host(assigner, cluster_xyz, batch_idx, preds_2d, no_aug_rows_list, no_aug_labels_list, gt_rows_list,
                         gt_task_labels_list, lidar2img, num_task_classes, code_size, old_cls_logits, canvas, return_parts):
    assigner.check()
    canvas = CANVAS if canvas is None else canvas
    lidar2img = torch.as_tensor(lidar2img).float().cpu()
    parts = {}
    with_dist = getattr(assigner, "assigner_dist", None) is not None
    old = old_cls_logits.detach().float().cpu()[:, :num_task_classes] if with_dist else None
    n_samples = len(gt_rows_list)
    assert len(no_aug_rows_list) == len(no_aug_labels_list) == n_samples == len(gt_task_labels_list)
    p2d = preds_2d.detach().float().cpu()
    bidx = batch_idx.detach().cpu()

    def na_valid(b):
        rows = gt_box_rows(no_aug_rows_list[b]).float().cpu()
        lab = torch.as_tensor(no_aug_labels_list[b]).long().reshape(-1).cpu()
        return rows[lab >= 0]

    def assign_fn(b, centres, rows):
        mine = torch.nonzero(bidx == b, as_tuple=False).reshape(-1)
        if isinstance(assigner, FrustumAssigner):
            lab = torch.as_tensor(gt_task_labels_list[b]).long().reshape(-1).cpu()
            parts[b] = assigner.assign_rows(p2d[mine], na_valid(b), centres.cpu(), rows.cpu(), lidar2img[b], canvas,
                                            old_cls_logits=old[mine] if with_dist else None, gt_labels=lab[lab >= 0])
        else:
            parts[b] = assigner.assign_rows(p2d[mine], na_valid(b), centres.cpu(), rows.cpu(), lidar2img[b], canvas)
        return parts[b]["final"]

    out = _targets_from_assignment_host(cluster_xyz, batch_idx, gt_rows_list, gt_task_labels_list, num_task_classes, code_size, assign_fn)
    return out + ([parts.get(b) for b in range(n_samples)],) if return_parts else out


class _ClusterLossFn(torch.autograd.Function):
    """K36b forward / K36c backward: (loss_cls, loss_center, loss_size, loss_rot, loss_vel) of (cls_logits, reg_preds) with the
    targets and the averaging factors held fixed.  Head-agnostic: any assigner's labels / targets / weights can feed it."""

    @staticmethod
    def forward(ctx, cls_logits, reg_preds, labels, label_weights, bbox_targets, bbox_weights, avg_factors, gamma, alpha, loss_weights,
                with_vel):
        losses, counts = hip_ops.cluster_loss_forward(cls_logits, reg_preds, labels, label_weights, bbox_targets, bbox_weights, avg_factors,
                                                      gamma, alpha, loss_weights, with_vel)
        ctx.save_for_backward(cls_logits, reg_preds, labels, label_weights, bbox_targets, bbox_weights, avg_factors, counts)
        ctx.cfg = (gamma, alpha, loss_weights, with_vel)
        ctx.set_materialize_grads(False)
        return tuple(losses.unbind(0))

    @staticmethod
    def backward(ctx, *grads):
        cls_logits, reg_preds, labels, label_weights, bbox_targets, bbox_weights, avg_factors, counts = ctx.saved_tensors
        grads = [None if g is None else g.float().reshape(1) for g in grads]
        g_cls, g_reg = hip_ops.cluster_loss_backward(cls_logits, reg_preds, labels, label_weights, bbox_targets, bbox_weights, avg_factors,
                                                     *ctx.cfg, counts, grads)
        return (g_cls if ctx.needs_input_grad[0] else None, g_reg if ctx.needs_input_grad[1] else None) + (None,) * 9


def _reduce_mean(t):
    """mmdet `reduce_mean`: the mean over the process group, the tensor itself in a single process."""
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()):
        return t
    t = t.clone()
    dist.all_reduce(t.div_(dist.get_world_size()), op=dist.ReduceOp.SUM)
    return t


@HEADS.register_module()
class FSDSeparateHead(nn.Module):
    def __init__(self, in_channels, attrs, norm_cfg=dict(type="LN"), act="relu", init_cfg=None):
        super().__init__()
        self.attrs = attrs
        for attr_name in self.attrs:
            out_dim, num_layer, hidden_dim = self.attrs[attr_name]
            self.add_module(attr_name, build_mlp(in_channels, [hidden_dim] * num_layer + [out_dim], norm_cfg, is_head=True, act=act))

    def forward(self, x):
        fused = self._forward_sliced(x)
        if fused is not None:
            return fused
        return {attr_name: getattr(self, attr_name)(x) for attr_name in self.attrs}

    def accepts_planes(self, n_rows):
        """Will `forward` take the query features in plane form (RowPlanes) for `n_rows` rows?  (Its first layer then runs on K22h.)"""
        if not switches.K22H or self.training or n_rows < switches.K22H_MIN_ROWS or len(self.attrs) <= 1:
            return False
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return False
        plan = self._sliced_plan()
        return plan is not None and "first_f16" in plan

    # ---- inference on the GPU: the attribute branches are independent MLPs of one shape on the same input, so layer i of
    # all of them is ONE K22 launch (fsf_linear_norm_act_sliced) instead of one per attribute — per query head 15 launches
    # (10 fused blocks + 5 library GEMMs for the 2..10-wide outputs) become 3, and a 10 k-row x 1024 -> 128 layer, which
    # fills a third of the chip on its own, runs five abreast.  Per branch the arithmetic is unchanged.
    _OUT_PAD = 16  # output channels per branch in the last (plain Linear) layer's launch: padded with zero weight rows

    def _sliced_plan(self):
        from ...ops.sst_ops import MLPBlock

        names = list(self.attrs)
        mlps = [getattr(self, a) for a in names]
        depth = len(mlps[0])
        if any(len(m) != depth for m in mlps) or depth < 2:
            return None
        params = self.__dict__.get("_fsf_param_list")  # (the Parameter objects: walking the module tree per frame and head costs ~50 us)
        if params is None:
            params = self.__dict__["_fsf_param_list"] = [p for m in mlps for p in m.parameters()]
        key = tuple((p.data_ptr(), p._version) for p in params)
        cache = self.__dict__.get("_fsf_sliced")
        if cache is not None and cache[0] == key:
            return cache[1]
        plan = None
        blocks_ok = True
        for li in range(depth - 1):
            layer = [m[li] for m in mlps]
            if not all(isinstance(b, MLPBlock) and len(b) == 3 and isinstance(b[0], nn.Linear) and isinstance(b[1], nn.LayerNorm)
                       and b[1].elementwise_affine and len(b[1].normalized_shape) == 1 for b in layer):
                blocks_ok = False
                break
            ref = layer[0]
            act_code = "relu" if isinstance(ref[2], nn.ReLU) else (
                "gelu" if isinstance(ref[2], nn.GELU) and getattr(ref[2], "approximate", "none") == "none" else None)
            if act_code is None or any(type(b[2]) is not type(ref[2]) or b[0].weight.shape != ref[0].weight.shape
                                       or b[1].eps != ref[1].eps or (b[0].bias is None) != (ref[0].bias is None) for b in layer):
                blocks_ok = False
                break
            if ref[0].out_features % 4 or ref[0].out_features > 128:
                blocks_ok = False
                break
        last = [m[depth - 1] for m in mlps]
        if blocks_ok and all(isinstance(l, nn.Linear) and l.out_features <= self._OUT_PAD for l in last) \
                and len({l.in_features for l in last}) == 1:
            with torch.no_grad():
                layers = []
                for li in range(depth - 1):
                    layer = [m[li] for m in mlps]
                    h = layer[0][0].out_features
                    w = torch.cat([b[0].weight for b in layer], 0)
                    layers.append(dict(
                        k=layer[0][0].in_features, h=h, planes=hip_ops.linear_prepare_weight_sliced(w, len(names), h),
                        bias=torch.cat([b[0].bias for b in layer]) if layer[0][0].bias is not None else None,
                        gamma=torch.cat([b[1].weight for b in layer]), beta=torch.cat([b[1].bias for b in layer]),
                        eps=layer[0][1].eps,
                        act="relu" if isinstance(layer[0][2], nn.ReLU) else "gelu"))
                pad = self._OUT_PAD
                kin = last[0].in_features
                w = torch.zeros((len(names) * pad, kin), dtype=torch.float32, device=last[0].weight.device)
                b = torch.zeros((len(names) * pad,), dtype=torch.float32, device=w.device)
                for i, l in enumerate(last):
                    w[i * pad:i * pad + l.out_features] = l.weight
                    if l.bias is not None:
                        b[i * pad:i * pad + l.out_features] = l.bias
                plan = dict(names=names, layers=layers, out_k=kin, out_planes=hip_ops.linear_prepare_weight_sliced(w, len(names), pad),
                            out_bias=b, out_dims=[l.out_features for l in last])
                # the branches' FIRST layer on K22h (f16 x 3 planes; all branches read the same >= 256-wide query features)
                first = [m[0][0] for m in mlps]
                k0, h0 = first[0].in_features, first[0].out_features
                if switches.K22H and k0 % 32 == 0 and k0 >= 256 and 64 < h0 <= 128 and h0 % 4 == 0:
                    plan["first_f16"] = hip_ops.linear_prepare_weight_f16(torch.cat([l.weight for l in first], 0), h0)
        self.__dict__["_fsf_sliced"] = (key, plan)
        return plan

    def _forward_sliced(self, x):
        from ...ops.sst_ops import as_row_planes

        is_planes = isinstance(x, hip_ops.RowPlanes)
        if self.training or (torch.is_grad_enabled() and ((not is_planes and x.requires_grad) or any(p.requires_grad for p in self.parameters()))):
            return None
        if not is_planes and not (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and x.size(0) >= 1 and x.stride(1) == 1
                                  and (x.size(0) == 1 or x.stride(0) % 4 == 0) and x.data_ptr() % 16 == 0 and len(self.attrs) > 1):
            return None
        plan = self._sliced_plan()
        k_in, n_rows = (x.c, x.n) if is_planes else (x.size(1), x.size(0))
        if plan is None or plan["layers"][0]["k"] != k_in:
            return None
        ns = len(plan["names"])
        h_prev = 0
        for li, lay in enumerate(plan["layers"]):
            if li == 0 and "first_f16" in plan and (is_planes or (n_rows >= switches.K22H_MIN_ROWS and hip_ops.rows_to_planes_supported(x))):
                x = hip_ops.linear_planes_norm_act(as_row_planes(x), plan["first_f16"], ns * lay["h"], lay["h"], bias=lay["bias"], norm="ln",
                                                   gamma=lay["gamma"], beta=lay["beta"], eps=lay["eps"], act=lay["act"])
                h_prev = lay["h"]
                continue
            if isinstance(x, hip_ops.RowPlanes):
                return None
            x = hip_ops.linear_norm_act_sliced(x, lay["k"], h_prev, lay["planes"], ns, lay["h"], bias=lay["bias"], norm="ln",
                                               gamma=lay["gamma"], beta=lay["beta"], eps=lay["eps"], act=lay["act"])
            h_prev = lay["h"]
        y = hip_ops.linear_norm_act_sliced(x, plan["out_k"], h_prev, plan["out_planes"], ns, self._OUT_PAD, bias=plan["out_bias"])
        pad = self._OUT_PAD
        return {a: y[:, i * pad:i * pad + d] for i, (a, d) in enumerate(zip(plan["names"], plan["out_dims"]))}


@HEADS.register_module()
class SparseClusterHead(nn.Module):
    def __init__(self, num_classes, bbox_coder, loss_cls, loss_center, loss_size, loss_rot, in_channel, shared_mlp_dims,
                 shared_dropout=0, cls_mlp=None, reg_mlp=None, iou_mlp=None, train_cfg=None, test_cfg=None,
                 norm_cfg=dict(type="LN"), loss_iou=None, act="relu", corner_loss_cfg=None, enlarge_width=None,
                 as_rpn=False, init_cfg=None):
        super().__init__()
        self.print_info = {}
        self.loss_center, self.loss_size = build_loss(loss_center), build_loss(loss_size)
        self.loss_rot, self.loss_cls = build_loss(loss_rot), build_loss(loss_cls)
        self.bbox_coder = BBOX_CODERS.build(bbox_coder)
        self.box_code_size = self.bbox_coder.code_size
        self.corner_loss_cfg = corner_loss_cfg
        self.num_classes = num_classes
        self.enlarge_width = enlarge_width
        self.sync_reg_avg_factor = False if train_cfg is None else train_cfg.get("sync_reg_avg_factor", True)
        self.sync_cls_avg_factor = False if train_cfg is None else train_cfg.get("sync_cls_avg_factor", True)
        self.as_rpn = as_rpn
        self.train_cfg = self.test_cfg = None
        if train_cfg is not None:
            self.cfg = self.train_cfg = train_cfg
        if test_cfg is not None:
            self.cfg = self.test_cfg = test_cfg
        self.num_anchors = num_anchors = 1
        self.loss_iou = build_loss(loss_iou) if loss_iou is not None else None
        self.fp16_enabled = False
        self.shared_mlp = None
        if len(shared_mlp_dims) > 0:
            self.shared_mlp = build_mlp(in_channel, shared_mlp_dims, norm_cfg, act=act, dropout=shared_dropout)
        end_channel = shared_mlp_dims[-1] if len(shared_mlp_dims) > 0 else in_channel
        if cls_mlp is not None:
            self.conv_cls = build_mlp(end_channel, cls_mlp + [num_classes * num_anchors], norm_cfg, True, act=act)
        else:
            self.conv_cls = nn.Linear(end_channel, num_classes * num_anchors)
        if reg_mlp is not None:
            self.conv_reg = build_mlp(end_channel, reg_mlp + [self.box_code_size * num_anchors], norm_cfg, True, act=act)
        else:
            self.conv_reg = nn.Linear(end_channel, self.box_code_size * num_anchors)
        self.save_list = []

    def forward(self, feats, pts_xyz=None, pts_inds=None):
        if self.shared_mlp is not None:
            feats = self.shared_mlp(feats)
        return dict(cls_logits=self.conv_cls(feats), reg_preds=self.conv_reg(feats))

    def split_by_batch(self, data, batch_idx, batch_size):
        if batch_size == 1:
            return [data]
        return [data[batch_idx == i] for i in range(batch_size)]

    def combine_by_batch(self, data_list, batch_idx, batch_size):
        assert len(data_list) == batch_size
        if data_list[0] is None:
            return None
        full = data_list[0].new_zeros((len(batch_idx),) + data_list[0].shape[1:])
        for i, data in enumerate(data_list):
            full[batch_idx == i] = data
        return full

    def loss(self, *args, **kwargs):
        raise NotImplementedError("SparseClusterHead.loss (v1) is not built: the FSF configs use SparseClusterHeadV2, whose loss is")


@HEADS.register_module()
class SparseClusterHeadV2(SparseClusterHead):
    BATCH_COL = 1  # cluster_inds rows are (class, batch, cluster id)  (sparse_cluster_head_v2.py:509-512)
    EMPTY_BOX_DIM = 7

    def __init__(self, num_classes, bbox_coder, loss_cls, loss_center, loss_size, loss_rot, in_channel, shared_mlp_dims,
                 tasks, class_names, common_attrs, num_cls_layer, cls_hidden_dim, separate_head, cls_mlp=None,
                 reg_mlp=None, iou_mlp=None, train_cfg=None, test_cfg=None, norm_cfg=dict(type="LN"), loss_iou=None,
                 act="relu", corner_loss_cfg=None, enlarge_width=None, as_rpn=False, init_cfg=None, shared_dropout=0,
                 loss_vel=None):
        super().__init__(num_classes, bbox_coder, loss_cls, loss_center, loss_size, loss_rot, in_channel, shared_mlp_dims,
                         shared_dropout, cls_mlp, reg_mlp, iou_mlp, train_cfg, test_cfg, norm_cfg, loss_iou, act,
                         corner_loss_cfg, enlarge_width, as_rpn, init_cfg)
        self.conv_cls = None  # overridden by the per-task separate heads
        self.conv_reg = None
        sep_head_in_channels = shared_mlp_dims[-1] if self.shared_mlp is not None else in_channel
        self.tasks = tasks
        self.task_heads = nn.ModuleList()
        for t in tasks:
            attrs = copy.deepcopy(dict(common_attrs))
            attrs.update(dict(score=(len(t["class_names"]), num_cls_layer, cls_hidden_dim)))
            head_cfg = dict(separate_head)
            head_cfg.update(in_channels=sep_head_in_channels, attrs=attrs)
            self.task_heads.append(build_head(head_cfg))
        self.class_names = class_names
        self.loss_vel = build_loss(loss_vel) if loss_vel is not None else None
        self.task_info = {}

    def forward(self, feats, pts_xyz=None, pts_inds=None):
        if self.shared_mlp is not None:
            # (the shared MLP's output only feeds the task heads' branches: in plane form when every one of them takes it)
            as_planes = (torch.is_tensor(feats) and feats.dim() == 2 and feats.is_cuda
                         and all(getattr(h, "accepts_planes", lambda n: False)(feats.size(0)) for h in self.task_heads)
                         and self.task_heads[0]._sliced_plan()["layers"][0]["k"] == self.shared_mlp[-1][0].out_features)
            feats = self.shared_mlp(feats, planes_out=True) if as_planes else self.shared_mlp(feats)
        cls_logit_list, reg_pred_list, iou_logits_list = [], [], []
        for h in self.task_heads:
            ret = h(feats)
            parts = [ret["center"], ret["dim"], ret["rot"]] + ([ret["vel"]] if "vel" in ret else [])
            reg_pred_list.append(torch.cat(parts, dim=-1))  # same column order as v1's single regression branch
            cls_logit_list.append(ret["score"])
            if "iou" in ret:
                iou_logits_list.append(ret["iou"])
        outs = dict(cls_logits=cls_logit_list, reg_preds=reg_pred_list)
        if len(iou_logits_list) > 0:
            outs.update(iou_logits=iou_logits_list)
        return outs

    # ------------------------------------------------------------------------------------------- losses (K36)
    _REFUSED_TRAIN_CFG = ("max_assign_dist", "assign_by_dist", "code_weight")

    def _check_loss_cfg(self):
        """Options neither FSF config sets for this head are refused, not approximated."""
        cfg = self.train_cfg or {}
        for key in self._REFUSED_TRAIN_CFG:
            if cfg.get(key, None):
                raise NotImplementedError(f"SparseClusterHeadV2.loss: train_cfg['{key}'] is not used by the FSF configs and is not built")
        if self.loss_iou is not None:
            raise NotImplementedError("SparseClusterHeadV2.loss: loss_iou is not used by the FSF configs and is not built")
        if self.corner_loss_cfg is not None:
            raise NotImplementedError("SparseClusterHeadV2.loss: corner_loss_cfg is not used by the FSF configs and is not built")
        for name in ("loss_cls", "loss_center", "loss_size", "loss_rot", "loss_vel"):
            mod = getattr(self, name)
            if getattr(mod, "OUT_OF_SCOPE", False):  # (the Argoverse 2 config's SmoothL1Loss: models/placeholders.py)
                raise NotImplementedError(f"SparseClusterHeadV2.loss: {name} is a {type(mod).__name__}, which is not built")

    def _fused_loss_ok(self, cls_logits, reg_preds, cluster_xyz):
        l1 = [self.loss_center, self.loss_size, self.loss_rot] + ([self.loss_vel] if self.loss_vel is not None else [])
        return (cls_logits.is_cuda and reg_preds.is_cuda and cluster_xyz.is_cuda and cls_logits.dtype == reg_preds.dtype
                == cluster_xyz.dtype == torch.float32 and cls_logits.dim() == reg_preds.dim() == 2
                and type(self.loss_cls) is FocalLoss and self.loss_cls.reduction == "mean"
                and all(type(m) is L1Loss and m.reduction == "mean" for m in l1)
                and type(self.bbox_coder) is BasePointBBoxCoder and self.box_code_size in (8, 10)
                and not (self.loss_vel is not None and self.box_code_size != 10))

    def _task_class_lut(self, task_id, device=None):
        """global class index -> index inside the task, -1 outside it: a list, or with `device` an i64 tensor there, uploaded once
        (pinned, non-blocking)."""
        names = self.tasks[task_id]["class_names"]
        lut = [names.index(n) if n in names else -1 for n in self.class_names]
        if device is None:
            return lut
        cache = self.__dict__.setdefault("_task_luts", {})
        key = (task_id, str(device), tuple(lut))
        if key not in cache:
            host = torch.tensor(lut, dtype=torch.long)
            cache[key] = host.pin_memory().to(device, non_blocking=True) if torch.device(device).type == "cuda" else host
        return cache[key]

    def loss(self, cls_logits, reg_preds, cluster_xyz, cluster_inds, gt_bboxes_3d, gt_labels_3d, img_metas=None, iou_logits=None,
             gt_bboxes_ignore=None, fused=True):
        """:170-200 — every task's losses and log scalars, keys suffixed with the task's class-name list.  CUDA fp32 inputs with the
        FocalLoss + L1Loss configuration run K36 (no host wait); `fused=False`, CPU tensors or anything else run the torch restatement
        with upstream's asserts.  GT: per sample LiDARInstance3DBoxes or [M, 7 | 9 | 10] rows, and labels (rows < 0 are dropped)."""
        assert isinstance(cls_logits, list) and isinstance(reg_preds, list)
        assert len(cls_logits) == len(reg_preds) == len(self.tasks)
        self._check_loss_cfg()
        all_task_losses = {}
        self.task_info = {}
        for i in range(len(self.tasks)):
            all_task_losses.update(self.loss_single_task(i, cls_logits[i], reg_preds[i], cluster_xyz, cluster_inds, gt_bboxes_3d,
                                                         gt_labels_3d, iou_logits, fused=fused))
        return all_task_losses

    def modify_gt_for_single_task(self, gt_bboxes_3d, gt_labels_3d, task_id):
        """:316-343 — per sample (rows [M', D], task labels i64 [M']) in the task's order.  Host GT loses the rows outside the task, as
        upstream; device GT keeps them, last and labelled -1, so that no shape depends on device data."""
        num = len(self.tasks[task_id]["class_names"])
        out_b, out_l = [], []
        for gts_b, gts_l in zip(gt_bboxes_3d, gt_labels_3d):
            rows, labels = gt_box_rows(gts_b), torch.as_tensor(gts_l).reshape(-1)
            assert rows.size(0) == labels.size(0)
            if labels.size(0) > 0:
                rows, labels = regroup_gt_for_task(rows, labels.to(rows.device), self._task_class_lut(task_id, rows.device), num)
                if not rows.is_cuda:
                    keep = int((labels >= 0).sum())
                    rows, labels = rows[:keep], labels[:keep]
                    if keep > 0:
                        assert labels.max().item() < num
            out_b.append(rows)
            out_l.append(labels.long())
        return out_b, out_l

    def get_targets(self, num_task_classes, cluster_xyz, batch_idx, gt_bboxes_3d, gt_labels_3d, reg_preds=None, task_id=None, fused=True):
        """:345-439 — (labels, label_weights, bbox_targets, bbox_weights, iou_labels = None) for GT already in the task's order
        (`modify_gt_for_single_task`), and `task_info[str(task_id)]` = the four log scalars as f32 device scalars.  They are TOTALS over
        the batch (upstream overwrites them sample by sample and so reports the last sample's; with one sample the two agree)."""
        self._check_loss_cfg()
        width = self.enlarge_width
        if fused and cluster_xyz.is_cuda and cluster_xyz.dtype == torch.float32:
            box_ptr, boxes, box_labels = pack_gt_for_device(gt_bboxes_3d, gt_labels_3d, cluster_xyz.device, cols=None)
            labels, bbox_targets, bbox_weights, assigned, stats = hip_ops.cluster_targets(
                cluster_xyz, batch_idx, box_ptr, boxes, box_labels, num_task_classes, self.box_code_size, width or 0.0)
            label_weights = cluster_xyz.new_ones(cluster_xyz.size(0))
        else:
            labels, label_weights, bbox_targets, bbox_weights, assigned, stats = cluster_targets_host(
                cluster_xyz, batch_idx, gt_bboxes_3d, gt_labels_3d, num_task_classes, self.box_code_size, width)
        self.task_info[str(task_id)] = dict(num_preds=stats[0], num_pos_preds=stats[1], num_gts=stats[2], assigned_gts=stats[3])
        self._last_assignment = dict(assigned=assigned, avg_factors=stats[4:6])
        return labels, label_weights, bbox_targets, bbox_weights, None

    def _zero_losses(self, task_id, cls_logits, reg_preds, gt_labels_3d):
        """No cluster at all: upstream divides 0 by 0; here every loss is 0 with (empty) zero gradients."""
        zero = cls_logits.sum() * 0 + reg_preds.sum() * 0
        losses = dict(loss_cls=zero, loss_center=zero, loss_size=zero, loss_rot=zero)
        dev = reg_preds.device
        f = lambda v: torch.tensor(float(v), dtype=torch.float32, device=dev)  # noqa: E731
        num_gts = f(0)
        for l in gt_labels_3d:  # (device labels are counted where they are)
            num_gts = num_gts + (l >= 0).sum().to(device=dev, dtype=torch.float32)
        losses.update(num_preds=f(0), num_pos_preds=f(0), num_gts=num_gts, assigned_gts=f(0))
        self.task_info[str(task_id)] = {k: losses[k] for k in ("num_preds", "num_pos_preds", "num_gts", "assigned_gts")}
        if self.loss_vel is not None:
            losses["loss_vel"] = zero
        return losses

    def loss_single_task(self, task_id, cls_logits, reg_preds, cluster_xyz, cluster_inds, gt_bboxes_3d, gt_labels_3d, iou_logits=None,
                         fused=True):
        """:203-312.  loss_cls = focal over all rows / n; loss_center / loss_size / loss_rot = L1 over the positive rows / num_pos;
        loss_vel (when the head has it) is called upstream without avg_factor: the plain mean over the positive rows' two columns.
        Without positives the regression losses are 0 with zero gradients."""
        return self._loss_single_task_with(self.get_targets, task_id, cls_logits, reg_preds, cluster_xyz, cluster_inds, gt_bboxes_3d,
                                           gt_labels_3d, fused)

    def _loss_single_task_with(self, get_targets, task_id, cls_logits, reg_preds, cluster_xyz, cluster_inds, gt_bboxes_3d, gt_labels_3d,
                               fused):
        """The losses of one task on the targets of `get_targets(num_task_classes, cluster_xyz, batch_idx, gt boxes, gt labels,
        reg_preds, task_id, fused=)`: this head's point-in-box assignment, or the camera-query head's hybrid one."""
        self._check_loss_cfg()
        class_names = self.tasks[task_id]["class_names"]
        num_task_classes = len(class_names)
        gt_bboxes_3d, gt_labels_3d = self.modify_gt_for_single_task(gt_bboxes_3d, gt_labels_3d, task_id)
        batch_idx = cluster_inds if cluster_inds.ndim == 1 else cluster_inds[:, self.BATCH_COL]
        num_total_samples = len(reg_preds)
        assert cls_logits.size(0) == num_total_samples == cluster_xyz.size(0) and cls_logits.size(1) == num_task_classes
        assert reg_preds.size(1) == self.box_code_size
        if num_total_samples == 0:
            losses = self._zero_losses(task_id, cls_logits, reg_preds, gt_labels_3d)
            return {k + f"{class_names}": v for k, v in losses.items()}
        use_kernels = fused and self._fused_loss_ok(cls_logits, reg_preds, cluster_xyz)
        if not use_kernels:
            cls_logits, reg_preds, cluster_xyz = cls_logits.float(), reg_preds.float(), cluster_xyz.float()
        labels, label_weights, bbox_targets, bbox_weights, _ = get_targets(
            num_task_classes, cluster_xyz, batch_idx, gt_bboxes_3d, gt_labels_3d, reg_preds, task_id, fused=use_kernels)
        avg_factors = self._last_assignment["avg_factors"]  # (cls, reg) = (n, num_pos) as f32 scalars where the targets live
        sync = (self.sync_cls_avg_factor, self.sync_reg_avg_factor)
        if any(sync):
            synced = _reduce_mean(avg_factors)
            if synced is not avg_factors:  # (a process group exists: the all-reduce sits between targets and losses on the stream)
                avg_factors = torch.stack([synced[k] if sync[k] else avg_factors[k] for k in range(2)])
        if use_kernels:
            with_vel = self.loss_vel is not None
            weights = (self.loss_cls.loss_weight, self.loss_center.loss_weight, self.loss_size.loss_weight, self.loss_rot.loss_weight,
                       self.loss_vel.loss_weight if with_vel else 0.0)
            out = _ClusterLossFn.apply(cls_logits, reg_preds, labels, None, bbox_targets, bbox_weights, avg_factors,
                                       float(self.loss_cls.gamma), float(self.loss_cls.alpha), tuple(float(w) for w in weights), with_vel)
            losses = dict(loss_cls=out[0], loss_center=out[1], loss_size=out[2], loss_rot=out[3])
            losses.update(self.task_info[str(task_id)])
            if with_vel:
                losses["loss_vel"] = out[4]
            return {k + f"{class_names}": v for k, v in losses.items()}
        assert (label_weights == 1).all(), "for now"
        cls_avg_factor, reg_avg_factor = avg_factors[0], avg_factors[1]
        loss_cls = self.loss_cls(cls_logits, labels, label_weights, avg_factor=cls_avg_factor)
        pos_inds = ((labels >= 0) & (labels < num_task_classes)).nonzero(as_tuple=False).reshape(-1)
        num_pos = len(pos_inds)
        pos_reg_preds, pos_bbox_targets, pos_bbox_weights = reg_preds[pos_inds], bbox_targets[pos_inds], bbox_weights[pos_inds]
        if num_pos > 0:
            loss_center = self.loss_center(pos_reg_preds[:, :3], pos_bbox_targets[:, :3], pos_bbox_weights[:, :3], avg_factor=reg_avg_factor)
            loss_size = self.loss_size(pos_reg_preds[:, 3:6], pos_bbox_targets[:, 3:6], pos_bbox_weights[:, 3:6], avg_factor=reg_avg_factor)
            loss_rot = self.loss_rot(pos_reg_preds[:, 6:8], pos_bbox_targets[:, 6:8], pos_bbox_weights[:, 6:8], avg_factor=reg_avg_factor)
            if self.loss_vel is not None:
                loss_vel = self.loss_vel(pos_reg_preds[:, 8:10], pos_bbox_targets[:, 8:10], pos_bbox_weights[:, 8:10])
        else:
            loss_center = pos_reg_preds.sum() * 0
            loss_size = pos_reg_preds.sum() * 0
            loss_rot = pos_reg_preds.sum() * 0
            if self.loss_vel is not None:
                loss_vel = pos_reg_preds.sum() * 0
        losses = dict(loss_cls=loss_cls, loss_center=loss_center, loss_size=loss_size, loss_rot=loss_rot)
        losses.update(self.task_info[str(task_id)])
        if self.loss_vel is not None:
            losses["loss_vel"] = loss_vel
        return {k + f"{class_names}": v for k, v in losses.items()}

    # ------------------------------------------------------------------------------------------- boxes
    @torch.no_grad()
    def get_bboxes(self, cls_logits, reg_preds, cluster_xyz, cluster_inds, input_metas, iou_logits=None, rescale=False):
        return self._get_bboxes_all_tasks(cls_logits, reg_preds, None, cluster_xyz, cluster_inds, input_metas, iou_logits)

    def _get_bboxes_all_tasks(self, cls_logits, reg_preds, preds_2d, cluster_xyz, cluster_inds, input_metas, iou_logits):
        assert isinstance(cls_logits, list) and isinstance(reg_preds, list)
        assert len(cls_logits) == len(reg_preds) == len(self.tasks)
        per_task = [self.get_bboxes_single_task(i, cls_logits[i], reg_preds[i], preds_2d, cluster_xyz, cluster_inds,
                                                input_metas, iou_logits[i] if iou_logits is not None else None)
                    for i in range(len(self.tasks))]
        batch_size = len(input_metas)
        assert len(per_task[0]) <= batch_size
        if len(per_task) == 1:  # one task (the nuScenes / AV2 configs): nothing to concatenate
            return [tuple(per_task[0][b_idx]) for b_idx in range(batch_size)]
        out = []
        for b_idx in range(batch_size):
            out.append((LiDARInstance3DBoxes.cat([t[b_idx][0] for t in per_task]),
                        torch.cat([t[b_idx][1] for t in per_task], dim=0),
                        torch.cat([t[b_idx][2] for t in per_task], dim=0)))
        return out

    @torch.no_grad()
    def get_bboxes_single_task(self, task_id, cls_logits, reg_preds, preds_2d, cluster_xyz, cluster_inds, input_metas,
                               iou_logits=None, rescale=False):
        batch_inds = cluster_inds if cluster_inds.ndim == 1 else cluster_inds[:, self.BATCH_COL]
        batch_size = len(input_metas)
        split = lambda t: self.split_by_batch(t, batch_inds, batch_size)  # noqa: E731
        cls_l, reg_l, xyz_l = split(cls_logits), split(reg_preds), split(cluster_xyz)
        p2d_l = split(preds_2d) if preds_2d is not None else [None] * len(cls_l)
        iou_l = split(iou_logits) if iou_logits is not None else [None] * len(cls_l)
        return [self._get_bboxes_single(task_id, cls_l[b], iou_l[b], reg_l[b], p2d_l[b], xyz_l[b], input_metas[b])
                for b in range(len(cls_l))]

    def _box_type(self, input_meta):
        return input_meta.get("box_type_3d", LiDARInstance3DBoxes) if isinstance(input_meta, dict) else LiDARInstance3DBoxes

    def _get_bboxes_single(self, task_id, cls_logits, iou_logits, reg_preds, preds_2d, cluster_xyz, input_meta):
        """One sample, one task: sigmoid scores -> (optional top-k) -> decode -> per-class rotated BEV NMS."""
        if self.as_rpn:
            cfg = self.train_cfg["rpn"] if self.training else self.test_cfg["rpn"]
        else:
            cfg = self.test_cfg
        box_type = self._box_type(input_meta)
        assert cls_logits.size(0) == reg_preds.size(0) == cluster_xyz.size(0)
        assert cls_logits.size(1) == len(self.tasks[task_id]["class_names"])
        assert reg_preds.size(1) == self.box_code_size
        if len(cls_logits) == 0:
            empty = reg_preds.new_zeros((0, self.EMPTY_BOX_DIM))
            return box_type(empty, box_dim=self.EMPTY_BOX_DIM), reg_preds.new_zeros(0), reg_preds.new_zeros(0)
        fused = self._box_tail_fused(task_id, cfg, box_type, cls_logits, iou_logits, reg_preds, cluster_xyz)
        if fused is not None:
            return fused
        scores = cls_logits.sigmoid()
        if iou_logits is not None:
            a = cfg.get("iou_score_weight", 0.5)
            scores = (scores ** (1 - a)) * (iou_logits.sigmoid() ** a)
        nms_pre = cfg.get("nms_pre", -1)
        if nms_pre > 0 and scores.shape[0] > nms_pre:
            topk_inds = scores.max(dim=1)[0].topk(nms_pre)[1]
            reg_preds, scores, cluster_xyz = reg_preds[topk_inds, :], scores[topk_inds, :], cluster_xyz[topk_inds, :]
        bboxes = self.bbox_coder.decode(reg_preds, cluster_xyz)
        bboxes = self._append_debug_columns(bboxes, preds_2d)
        bboxes_for_nms = xywhr2xyxyr(box_type(bboxes, box_dim=bboxes.size(1)).bev)
        scores = torch.cat([scores, scores.new_zeros(scores.shape[0], 1)], dim=1)  # dummy background column
        out_bboxes, out_scores, out_labels = box3d_multiclass_nms(bboxes, bboxes_for_nms, scores, cfg.get("score_thr", 0),
                                                                  cfg["max_num"], cfg)
        out_bboxes, out_scores = self._strip_debug_columns(out_bboxes, out_scores)
        out_bboxes = box_type(out_bboxes, out_bboxes.size(1))
        # task-local label -> global class index: one table gather (the reference loops over the class names with a
        # masked assignment each — a hidden device sync per class — and asserts on the host that every label was mapped;
        # with a table every label is mapped by construction)
        lut = self._label_lut(task_id, out_labels.device)
        new_labels = lut[out_labels] if len(out_labels) > 0 else torch.zeros_like(out_labels) - 1
        return out_bboxes, out_scores, new_labels

    def _label_lut(self, task_id, device):
        luts = self.__dict__.setdefault("_label_luts", {})
        lut = luts.get((task_id, device))
        if lut is None:
            lut = torch.tensor([self.class_names.index(name) for name in self.tasks[task_id]["class_names"]], dtype=torch.long,
                               device=device)
            luts[(task_id, device)] = lut
        return lut

    def _box_tail_fused(self, task_id, cfg, box_type, cls_logits, iou_logits, reg_preds, cluster_xyz):
        """Inference on the GPU: everything between the head's outputs and the host-side result as four C-ABI calls (K24 decode,
        K24 class ranks, K20 capped multi-class NMS, K24 selection) and ONE read-back, instead of ~95 ATen launches and three host
        round trips.  Returns None when the configuration is outside what that path takes (the generic path below runs)."""
        max_num = cfg.get("max_num", 0)
        nms_pre = cfg.get("nms_pre", -1)
        n, c = cls_logits.shape
        if not (switches.BOX_TAIL_FUSED and cls_logits.is_cuda and cls_logits.dtype == torch.float32 and reg_preds.dtype == torch.float32
                and cluster_xyz.dtype == torch.float32 and iou_logits is None and not torch.is_grad_enabled()
                and box_type is LiDARInstance3DBoxes and getattr(self, "vis_dir", None) is None
                and isinstance(max_num, int) and max_num > 0 and c * max_num <= hip_ops.nms_select_capacity()
                and c <= hip_ops.box_tail_max_classes()
                and not (nms_pre > 0 and n > nms_pre) and type(self.bbox_coder) is BasePointBBoxCoder):
            return None
        boxes, boxes_nms, scores_t = hip_ops.decode_cluster_boxes(cls_logits, reg_preds, cluster_xyz, self.bbox_coder.EPS)
        order, rank, count = hip_ops.class_rank_desc(scores_t, cfg.get("score_thr", 0))
        keep, num, incomplete = hip_ops.nms_bev_multiclass(boxes_nms, rank, count, cfg["nms_thr"],
                                                           rotated=bool(cfg.get("use_rotate_nms", False)), max_keep=max_num, windowed=True)
        buf = hip_ops.nms_select(boxes, scores_t, order, keep, num, max_num, max_num, self._label_lut(task_id, cls_logits.device),
                                 incomplete)
        d = boxes.size(1)
        hook = self.__dict__.pop("_before_readback", None)
        if hook is not None:
            hook()  # (FSF: the next frame's front, issued while the device works through this frame's tail)
        host = buf.cpu()  # the frame's one read-back for the box tail: rows + (rows written, boxes kept, incomplete)
        meta = host[max_num * (d + 2):].view(torch.int32)
        if int(meta[2]) != 0:  # a class ran out of its mask window before max_num keeps (never seen): the generic path repeats it in full
            return None
        k = int(meta[0])
        rows = buf[:max_num * (d + 2)].view(max_num, d + 2)[:k]
        # (views of `buf`: row stride d + 2 — consumers index / reshape them; `.view()` needs `.contiguous()` first)
        out_bboxes, out_scores, out_labels = LiDARInstance3DBoxes._wrap(rows[:, :d], d), rows[:, d], rows[:, d + 1].long()
        # the same rows already on the host, for bbox3d2result — valid only while nobody has edited the device tensors since
        # (rescale / flip / score re-weighting between get_bboxes and bbox3d2result): identity + version counters travel along
        out_bboxes._host_rows = (host[:max_num * (d + 2)].view(max_num, d + 2)[:k], out_bboxes.tensor, out_bboxes.tensor._version,
                                 out_scores, out_scores._version, out_labels, out_labels._version)
        return out_bboxes, out_scores, out_labels

    def _append_debug_columns(self, bboxes, preds_2d):
        return bboxes

    def _strip_debug_columns(self, out_bboxes, out_scores):
        return out_bboxes, out_scores


@HEADS.register_module()
class FrustumClusterHead(SparseClusterHeadV2):
    BATCH_COL = 0  # frustum query coors are (batch, 0, obj id)  (frustum_cluster_head.py:562-565)
    EMPTY_BOX_DIM = 9

    def __init__(self, num_classes, bbox_coder, loss_cls, loss_center, loss_size, loss_rot, in_channel, shared_mlp_dims,
                 tasks, class_names, common_attrs, num_cls_layer, cls_hidden_dim, separate_head, cls_mlp=None,
                 reg_mlp=None, iou_mlp=None, train_cfg=dict(), test_cfg=dict(), norm_cfg=dict(type="LN"), loss_iou=None,
                 act="relu", corner_loss_cfg=None, enlarge_width=None, as_rpn=False, init_cfg=None, shared_dropout=0,
                 loss_vel=None, assigner=None, num_objs=250, vis_dir=None, use_one_to_one=False):
        super().__init__(num_classes, bbox_coder, loss_cls, loss_center, loss_size, loss_rot, in_channel, shared_mlp_dims,
                         tasks, class_names, common_attrs, num_cls_layer, cls_hidden_dim, separate_head, cls_mlp, reg_mlp,
                         iou_mlp, train_cfg, test_cfg, norm_cfg, loss_iou, act, corner_loss_cfg, enlarge_width, as_rpn,
                         init_cfg, shared_dropout, loss_vel)
        self.assigner = BBOX_ASSIGNERS.build(assigner) if assigner is not None else None
        self.num_objs = num_objs
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.task_info = {}
        self.vis_dir = vis_dir
        self.use_one_to_one = use_one_to_one

    # ------------------------------------------------------------------------------------------- losses (K37 + K36b / K36c)
    def _refuse_unbuilt(self):
        if type(self.assigner) not in (HybridAssigner, FrustumAssigner):
            raise NotImplementedError(
                "FrustumClusterHead.loss (frustum_cluster_head.py:96-462) is built for a HybridAssigner (K37) or a FrustumAssigner (K38); "
                f"this head has {'no assigner' if self.assigner is None else 'a ' + type(self.assigner).__name__}")

    def _check_loss_cfg(self):
        self._refuse_unbuilt()
        super()._check_loss_cfg()
        if self.use_one_to_one:
            raise NotImplementedError("FrustumClusterHead.loss: use_one_to_one=True is not used by the FSF configs and is not built")
        if self.enlarge_width:
            raise NotImplementedError("FrustumClusterHead.loss: enlarge_width is not read by the camera-query head's assigners")
        who = f"FrustumClusterHead.loss: {type(self.assigner).__name__}"
        if type(self.assigner) is FrustumAssigner:  # (the rule on task-local labels is the assigner's, applied to this head's tasks too)
            self.assigner.check(who, head_tasks=self.tasks, head_class_names=self.class_names)
        else:
            self.assigner.check(who)

    def _with_dist(self):
        return type(self.assigner) is FrustumAssigner and self.assigner.assigner_dist is not None

    def _dist_table(self, num_task_classes, device):
        """The DistAssigner's per-class radii f32 [C], uploaded once per head and device (pinned, non-blocking)."""
        cache = self.__dict__.setdefault("_dist_tables", {})
        key = (int(num_task_classes), str(device))
        if key not in cache:
            host = self.assigner.assigner_dist.class_table(num_task_classes)
            cache[key] = host.pin_memory().to(device, non_blocking=True) if torch.device(device).type == "cuda" else host
        return cache[key]

    def _source_ids(self, device):
        cache = self.__dict__.setdefault("_source_id_rows", {})
        if str(device) not in cache:
            host = torch.arange(4, dtype=torch.int32)
            cache[str(device)] = host.pin_memory().to(device, non_blocking=True) if torch.device(device).type == "cuda" else host
        return cache[str(device)]

    def gt_boxes_2d_pack(self, task_id, no_aug_gt_bboxes_3d, no_aug_gt_labels_3d, lidar2img, device):
        """K37a for one task: the un-augmented GT regrouped in the task's order, projected and clipped into every camera ->
        (ptr_2d, boxes_2d, keep), what `loss(..., boxes_2d_packs={task_id: pack})` takes instead of running K37a itself."""
        from .... import hip_ops_assign

        rows, labels = self.modify_gt_for_single_task(no_aug_gt_bboxes_3d, no_aug_gt_labels_3d, task_id)
        ptr_2d, rows_2d, labels_2d = pack_gt_for_device(rows, labels, device, cols=7)
        boxes_2d, keep = hip_ops_assign.gt_boxes_2d(rows_2d, labels_2d, ptr_2d, lidar2img.to(device))
        return ptr_2d, boxes_2d, keep

    def _lidar2img_batch(self, img_metas, device):
        """img_metas[b]['lidar2img'] (host lists) -> f32 [B, ncam, 4, 4]: rounded to f32 on the host, one pinned non-blocking copy."""
        import numpy as np

        mats = [meta["lidar2img"] for meta in img_metas]
        ncam = self.assigner.num_cams
        if all(torch.is_tensor(m) for m in mats):  # (already tensors: stacked where they are)
            stacked = torch.stack([m[:ncam].float() for m in mats])
            assert stacked.dim() == 4 and stacked.shape[2:] == (4, 4), f"lidar2img: {tuple(stacked.shape)}"
            if stacked.is_cuda or torch.device(device).type != "cuda":
                return stacked.to(device)
            return stacked.pin_memory().to(device, non_blocking=True)
        host = torch.from_numpy(np.stack([np.stack([np.asarray(m.cpu() if torch.is_tensor(m) else m, dtype=np.float64) for m in meta][:ncam])
                                          for meta in mats]).astype(np.float32))
        assert host.dim() == 4 and host.shape[2:] == (4, 4), f"lidar2img: {tuple(host.shape)}"
        if torch.device(device).type != "cuda":
            return host
        return host.pin_memory().to(device, non_blocking=True)

    def loss(self, cls_logits, reg_preds, cluster_xyz, cluster_inds, no_aug_gt_bboxes_3d, no_aug_gt_labels_3d, gt_bboxes_3d, gt_labels_3d,
             preds_2d=None, img_metas=None, iou_logits=None, old_cls_logits=None, old_reg_preds=None, gt_bboxes_ignore=None, fused=True,
             boxes_2d_packs=None):
        """:96-136 — every task's losses and log scalars under the hybrid assignment (a query takes the augmented GT box that contains
        its centre, else the one whose un-augmented image projection its 2-D box overlaps: docs/kernels/K37_hybrid_assign.md), keys
        suffixed with the task's class-name list.  CUDA fp32 inputs run K37 + K36b / K36c with no host wait; `fused=False` or CPU
        tensors run the torch restatement.  A head without a built assigner raises before it looks at its arguments.

        The refine stages' heads (a `FrustumAssigner` with an `assigner_dist`) also take `old_cls_logits`, the previous stage's
        per-task class logits: a query both steps left unassigned takes the nearest GT of the class they predict, inside that class's
        radius (K38).  `old_reg_preds` is accepted and unused, as upstream's PointInBoxAssigner ignores it.  `boxes_2d_packs`:
        optionally {task id: `gt_boxes_2d_pack(...)`}, K37a's output computed by the caller (two heads sharing one projection)."""
        self._check_loss_cfg()  # (refuses a head without a built assigner first, before any argument is looked at)
        if self._with_dist():
            if old_cls_logits is None:
                raise ValueError("FrustumClusterHead.loss: a FrustumAssigner with an assigner_dist needs old_cls_logits (the previous "
                                 "stage's class logits, one tensor per task)")
            assert isinstance(old_cls_logits, (list, tuple)) and len(old_cls_logits) == len(self.tasks)
        assert isinstance(cls_logits, list) and isinstance(reg_preds, list)
        assert len(cls_logits) == len(reg_preds) == len(self.tasks)
        assert preds_2d is not None and img_metas is not None, "the hybrid assignment needs preds_2d and img_metas[b]['lidar2img']"
        assert len(img_metas) == len(gt_bboxes_3d) == len(no_aug_gt_bboxes_3d)
        lidar2img = self._lidar2img_batch(img_metas, cluster_xyz.device if fused else "cpu")
        all_task_losses = {}
        self.task_info = {}
        for i in range(len(self.tasks)):
            all_task_losses.update(self.loss_single_task(i, cls_logits[i], reg_preds[i], cluster_xyz, cluster_inds, no_aug_gt_bboxes_3d,
                                                         no_aug_gt_labels_3d, gt_bboxes_3d, gt_labels_3d, preds_2d, img_metas,
                                                         old_cls_logits=old_cls_logits[i] if self._with_dist() else None,
                                                         fused=fused, lidar2img=lidar2img,
                                                         boxes_2d_pack=(boxes_2d_packs or {}).get(i)))
        return all_task_losses

    def get_targets(self, num_task_classes, no_aug_gt_bboxes_3d, no_aug_gt_labels_3d, gt_bboxes_3d, gt_labels_3d, preds_2d, cluster_xyz,
                    cluster_inds, task_id=None, img_metas_list=None, reg_preds=None, new_cls_logits=None, old_cls_logits=None,
                    old_reg_preds=None, fused=True, lidar2img=None, boxes_2d_pack=None):
        """:267-462 — (labels, label_weights, bbox_targets, bbox_weights, iou_labels = None) for GT already in the task's order
        (`modify_gt_for_single_task`, both lists), and `task_info[str(task_id)]` = the four log scalars (totals over the batch).
        With a `FrustumAssigner` the assignment is K38's (`old_cls_logits`: the previous stage's logits of this task) and
        `_last_assignment` also holds `source` (per query) and `source_counts` i64 [4] (none, 3-D, 2-D, distance)."""
        self._check_loss_cfg()
        frustum = type(self.assigner) is FrustumAssigner
        with_dist = self._with_dist()
        if with_dist and old_cls_logits is None:
            raise ValueError("FrustumClusterHead.get_targets: a FrustumAssigner with an assigner_dist needs old_cls_logits")
        source = None
        batch_idx = cluster_inds if cluster_inds.ndim == 1 else cluster_inds[:, self.BATCH_COL]
        a = self.assigner
        on_device = fused and cluster_xyz.is_cuda and cluster_xyz.dtype == torch.float32
        if lidar2img is None:
            lidar2img = self._lidar2img_batch(img_metas_list, cluster_xyz.device if on_device else "cpu")
        if on_device:
            from .... import hip_ops_assign

            dev = cluster_xyz.device
            if boxes_2d_pack is not None:
                ptr_2d, boxes_2d, keep = boxes_2d_pack
            else:
                ptr_2d, rows_2d, labels_2d = pack_gt_for_device(no_aug_gt_bboxes_3d, no_aug_gt_labels_3d, dev, cols=7)
                boxes_2d, keep = hip_ops_assign.gt_boxes_2d(rows_2d, labels_2d, ptr_2d, lidar2img.to(dev))
            box_ptr, boxes, box_labels = pack_gt_for_device(gt_bboxes_3d, gt_labels_3d, dev, cols=None)
            if frustum:
                from .... import hip_ops_frustum

                labels, bbox_targets, bbox_weights, assigned, source, stats = hip_ops_frustum.frustum_assign(
                    cluster_xyz, batch_idx, preds_2d.float(), ptr_2d, boxes_2d, keep, box_ptr, boxes, box_labels, num_task_classes,
                    self.box_code_size, a.assigner_3d.extra_height or 0.0, a.assigner_2d.pos_iou_thr, a.assigner_2d.min_pos_iou,
                    old_cls_logits.detach().float() if with_dist else None,
                    self._dist_table(num_task_classes, dev) if with_dist else None)
            else:
                labels, bbox_targets, bbox_weights, assigned, stats = hip_ops_assign.hybrid_assign(
                    cluster_xyz, batch_idx, preds_2d.float(), ptr_2d, boxes_2d, keep, box_ptr, boxes, box_labels, num_task_classes,
                    self.box_code_size, a.assigner_3d.extra_height or 0.0, a.assigner_2d.pos_iou_thr, a.assigner_2d.min_pos_iou)
            label_weights = cluster_xyz.new_ones(cluster_xyz.size(0))
        elif frustum:
            *out, parts = frustum_targets_host(
                a, cluster_xyz, batch_idx, preds_2d, no_aug_gt_bboxes_3d, no_aug_gt_labels_3d, gt_bboxes_3d, gt_labels_3d, lidar2img,
                num_task_classes, self.box_code_size, old_cls_logits if with_dist else None, return_parts=True)
            labels, label_weights, bbox_targets, bbox_weights, assigned, stats = out
            source = torch.zeros((cluster_xyz.size(0),), dtype=torch.int32)
            for b, part in enumerate(parts):
                if part is not None:
                    source[torch.nonzero(batch_idx.cpu() == b, as_tuple=False).reshape(-1)] = part["source"].int()
            source = source.to(cluster_xyz.device)
        else:
            labels, label_weights, bbox_targets, bbox_weights, assigned, stats = hybrid_targets_host(
                a, cluster_xyz, batch_idx, preds_2d, no_aug_gt_bboxes_3d, no_aug_gt_labels_3d, gt_bboxes_3d, gt_labels_3d, lidar2img,
                num_task_classes, self.box_code_size)
        self.task_info[str(task_id)] = dict(num_preds=stats[0], num_pos_preds=stats[1], num_gts=stats[2], assigned_gts=stats[3])
        self._last_assignment = dict(assigned=assigned, avg_factors=stats[4:6])
        if source is not None:
            self._last_assignment.update(source=source, source_counts=(source[:, None] == self._source_ids(source.device)[None, :]).sum(0))
        return labels, label_weights, bbox_targets, bbox_weights, None

    def loss_single_task(self, task_id, cls_logits, reg_preds, cluster_xyz, cluster_inds, no_aug_gt_bboxes_3d, no_aug_gt_labels_3d,
                         gt_bboxes_3d, gt_labels_3d, preds_2d, img_metas, iou_logits=None, old_cls_logits=None, old_reg_preds=None,
                         fused=True, lidar2img=None, boxes_2d_pack=None):
        """:138-265.  The LiDAR-query head's losses (`SparseClusterHeadV2.loss_single_task`) on the hybrid assignment's targets."""
        this_task = task_id

        def targets(num_task_classes, xyz, batch_idx, gt_b, gt_l, reg_preds=None, task_id=None, fused=True):
            # the un-augmented GT is read only to project it (K37a): a pack handed in already holds that, regrouped once by its maker
            pack_used = boxes_2d_pack is not None and fused and xyz.is_cuda and xyz.dtype == torch.float32
            no_aug = (None, None) if pack_used else self.modify_gt_for_single_task(no_aug_gt_bboxes_3d, no_aug_gt_labels_3d, this_task)
            return self.get_targets(num_task_classes, no_aug[0], no_aug[1], gt_b, gt_l, preds_2d, xyz, batch_idx, task_id=task_id,
                                    img_metas_list=img_metas, reg_preds=reg_preds, old_cls_logits=old_cls_logits, fused=fused,
                                    lidar2img=lidar2img, boxes_2d_pack=boxes_2d_pack)

        return self._loss_single_task_with(targets, task_id, cls_logits, reg_preds, cluster_xyz, cluster_inds, gt_bboxes_3d, gt_labels_3d,
                                           fused)

    @torch.no_grad()
    def get_bboxes(self, cls_logits, reg_preds, preds_2d, cluster_xyz, cluster_inds, input_metas, iou_logits=None,
                   rescale=False):
        return self._get_bboxes_all_tasks(cls_logits, reg_preds, preds_2d, cluster_xyz, cluster_inds, input_metas, iou_logits)

    def _append_debug_columns(self, bboxes, preds_2d):
        if self.vis_dir is not None:  # visualisation runs carry the 2-D object id through NMS (:629-631)
            bboxes = torch.cat([bboxes, preds_2d[:, 7:8]], dim=-1)
        return bboxes

    def _strip_debug_columns(self, out_bboxes, out_scores):
        if self.vis_dir is not None:
            out_bboxes, out_obj_id = out_bboxes[:, :-1], out_bboxes[:, -1]
            out_scores = out_scores + out_obj_id
        return out_bboxes, out_scores
