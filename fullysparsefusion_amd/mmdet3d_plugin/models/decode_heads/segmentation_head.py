"""`VoteSegHead` (HEADS): projects/mmdet3d_plugin/models/decode_heads/segmentation_head.py — per-point MLP, seg logits and vote
offsets (:15-104, dense GEMMs on rocBLAS via torch), and the training targets and losses (:106-265).

Targets and losses run on the device through K35 (docs/kernels/K35_seg_losses.md): `fsf_seg_targets` labels every point by the
first GT box of its sample that contains it (mmdet3d 0.x points_in_boxes_gpu with pinned arithmetic), `fsf_seg_loss_forward` /
`_backward` are the weighted cross entropy + the L1 on the point's own class's vote columns.  No `.item()`, no `nonzero`, no boolean
indexing on that path.  `seg_targets_host` / `losses(..., fused=False)` are the torch restatement the kernels are checked against."""
from .... import switches
import os

import torch
from torch import nn

from ...ops.sst_ops import PointLinear, build_mlp
from ...registry import HEADS, build_loss
from ..losses import CrossEntropyLoss, L1Loss


def gt_box_rows(boxes):
    """GT boxes of one sample -> f32 [M, >=7] rows (x, y, z_bottom, w, l, h, yaw, ...): `LiDARInstance3DBoxes` (7 or 9 columns) or
    a plain tensor / array."""
    t = getattr(boxes, "tensor", boxes)
    t = torch.as_tensor(t)
    return t.reshape(-1, t.shape[-1]) if t.numel() else t.reshape(0, max(7, t.shape[-1] if t.dim() else 7))


def box_constants_host(boxes7):
    """Per-box constants of the containment test, pinned as the kernel computes them: cz = f32(z_bottom + h / 2), half sizes, and
    cos / sin(-yaw) in float64 rounded to f32 once (on the CPU whatever the boxes' device)."""
    b = boxes7.float()
    h = b[:, 5]
    cz = b[:, 2] + h * 0.5
    yaw = -(b[:, 6].detach().cpu().double())
    cosa, sina = torch.cos(yaw).float().to(b.device), torch.sin(yaw).float().to(b.device)
    return b[:, 0], b[:, 1], cz, b[:, 3] * 0.5, b[:, 4] * 0.5, h * 0.5, cosa, sina


def points_in_boxes_first_host(xyz, boxes7):
    """mmdet3d 0.x points_in_boxes_gpu (check_pt_in_box3d) restated in torch: index of the FIRST box containing each point, -1 when
    none.  Every product and sum is a separately rounded f32 operation: lx = f32(f32(sx * cosa) + f32(sy * -sina)),
    ly = f32(f32(sx * sina) + f32(sy * cosa)); the z test is |z - cz| > h / 2 and the footprint test strict on all four sides."""
    xyz = xyz.float()
    inbox = torch.full((xyz.shape[0],), -1, dtype=torch.long, device=xyz.device)
    if boxes7.shape[0] == 0 or xyz.shape[0] == 0:
        return inbox
    cx, cy, cz, hw, hl, hh, cosa, sina = box_constants_host(boxes7)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    for k in range(boxes7.shape[0] - 1, -1, -1):  # later boxes first: the first containing box is written last
        sx, sy = x - cx[k], y - cy[k]
        lx = sx * cosa[k] + sy * (-sina[k])
        ly = sx * sina[k] + sy * cosa[k]
        inside = ((z - cz[k]).abs() <= hh[k]) & (lx > -hl[k]) & (lx < hl[k]) & (ly > -hw[k]) & (ly < hw[k])
        inbox = torch.where(inside, torch.full_like(inbox, k), inbox)
    return inbox


def encode_vote_targets(delta):
    """sign(d) * sqrt(|d|) with a correctly rounded f32 sqrt (the reference's `** 0.5`).  ATen's f32 pow / sqrt need not round
    correctly; the float64 root of an f32 value rounds to the correctly rounded f32 root."""
    return torch.sign(delta) * delta.abs().double().sqrt().to(delta.dtype)


def seg_targets_host(points, gt_boxes, gt_labels, bg_label):
    """One sample's (labels i64 [n], vote targets f32 [n, 3], vote mask bool [n]) — `get_targets`' per-sample body (:218-244) without
    `extra_width` / `centroid_offset` (the FSF configs set neither), with the containment test of `points_in_boxes_first_host`."""
    xyz = points[:, :3].float()
    boxes = gt_box_rows(gt_boxes).to(xyz.device).float()
    labels = torch.as_tensor(gt_labels).to(xyz.device).long().reshape(-1)
    valid = labels >= 0
    boxes, labels = boxes[valid], labels[valid]
    if labels.numel() == 0:
        return (torch.full((xyz.shape[0],), bg_label, dtype=torch.long, device=xyz.device), torch.zeros_like(xyz),
                torch.zeros((xyz.shape[0],), dtype=torch.bool, device=xyz.device))
    inbox = points_in_boxes_first_host(xyz, boxes[:, :7])
    bg = inbox < 0
    this_label = labels[inbox]
    this_label[bg] = bg_label
    gravity = boxes[:, :3].clone()
    gravity[:, 2] = boxes[:, 2] + boxes[:, 5] * 0.5
    delta = gravity[inbox] - xyz
    delta[bg] = 0
    return this_label, encode_vote_targets(delta), ~bg


def pack_gt_for_device(gt_bboxes_list, gt_labels_list, device, cols=7):
    """Per-sample GT -> (box_ptr i32 [B + 1], boxes f32 [M, cols], labels i32 [M]) on `device` with no host wait: CPU boxes and labels
    travel in ONE pinned buffer and one non-blocking copy; device boxes are concatenated where they are (only the CSR offsets, known
    from the shapes, are uploaded).  `cols=None` keeps every column of the rows (all non-empty samples must have the same number)."""
    rows = [gt_box_rows(b) for b in gt_bboxes_list]
    labs = [torch.as_tensor(l).reshape(-1) for l in gt_labels_list]
    counts = [int(r.shape[0]) for r in rows]
    assert all(int(l.numel()) == c for l, c in zip(labs, counts)), "one label per GT box"
    if cols is None:
        widths = {int(r.shape[1]) for r in rows if r.shape[0]}
        assert len(widths) <= 1, f"GT rows of one batch differ in their number of columns: {sorted(widths)}"
        cols = widths.pop() if widths else 7
    b, m = len(rows), sum(counts)
    ptr = [0]
    for c in counts:
        ptr.append(ptr[-1] + c)
    on_host = all(not r.is_cuda for r in rows) and all(not l.is_cuda for l in labs)
    if on_host:
        buf = torch.empty((b + 1 + m + cols * m,), dtype=torch.int32, pin_memory=True)
        buf[:b + 1] = torch.tensor(ptr, dtype=torch.int32)
        if m:
            buf[b + 1:b + 1 + m] = torch.cat([l.to(torch.int32) for l in labs])
            buf[b + 1 + m:].view(torch.float32).view(m, cols).copy_(torch.cat([r[:, :cols].float() for r in rows if r.shape[0]]))
        dev = buf.to(device, non_blocking=True)
        return dev[:b + 1], dev[b + 1 + m:].view(torch.float32).view(m, cols), dev[b + 1:b + 1 + m]
    def up(t, dtype):  # (a host tensor in a mixed list goes through pinned memory: a pageable copy would wait)
        return t.to(device=device, dtype=dtype) if t.is_cuda else t.to(dtype).pin_memory().to(device, non_blocking=True)

    box_ptr = up(torch.tensor(ptr, dtype=torch.int32), torch.int32)
    boxes = torch.cat([up(r[:, :cols], torch.float32) for r in rows if r.shape[0]]) if m else torch.empty((0, cols), device=device)
    labels = torch.cat([up(l, torch.int32) for l in labs]) if m else torch.empty((0,), dtype=torch.int32, device=device)
    return box_ptr, boxes.contiguous(), labels


class _SegLossFn(torch.autograd.Function):
    """K35b forward / K35c backward: (loss_sem_seg, loss_vote) of (logits, votes) with the targets held fixed."""

    @staticmethod
    def forward(ctx, logits, votes, labels, targets, mask, class_weight, ce_weight, vote_weight):
        from .... import hip_ops

        loss_ce, loss_vote, counts = hip_ops.seg_loss_forward(logits, votes, labels, targets, mask, class_weight, ce_weight, vote_weight)
        ctx.save_for_backward(logits, votes, labels, targets, mask, class_weight, counts)
        ctx.weights = (ce_weight, vote_weight)
        return loss_ce, loss_vote

    @staticmethod
    def backward(ctx, g_ce, g_vote):
        from .... import hip_ops

        logits, votes, labels, targets, mask, class_weight, counts = ctx.saved_tensors
        gl, gv = hip_ops.seg_loss_backward(logits, votes, labels, targets, mask, class_weight, *ctx.weights, counts,
                                           g_ce.float().reshape(1), g_vote.float().reshape(1))
        return (gl if ctx.needs_input_grad[0] else None, gv if ctx.needs_input_grad[1] else None, None, None, None, None, None, None)


@HEADS.register_module()
class VoteSegHead(nn.Module):
    def __init__(self, in_channel, num_classes, hidden_dims=[], dropout_ratio=0.5, conv_cfg=dict(type="Conv1d"),
                 norm_cfg=dict(type="naiveSyncBN1d"), act_cfg=dict(type="ReLU"),
                 loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, class_weight=None, loss_weight=1.0),
                 loss_vote=dict(type="L1Loss"), loss_aux=None, ignore_index=255, logit_scale=1, checkpointing=False,
                 init_bias=None, init_cfg=None):
        super().__init__()
        end_channel = hidden_dims[-1] if len(hidden_dims) > 0 else in_channel
        self.channels = end_channel
        self.num_classes = num_classes
        self.dropout_ratio = dropout_ratio
        self.norm_cfg, self.act_cfg, self.ignore_index = norm_cfg, act_cfg, ignore_index
        self.loss_decode_cfg, self.loss_vote_cfg, self.loss_aux_cfg = loss_decode, loss_vote, loss_aux
        self.loss_decode = build_loss(loss_decode)
        self.loss_vote = build_loss(loss_vote)
        self.loss_aux = build_loss(loss_aux) if loss_aux is not None else None
        self.dropout = nn.Dropout(dropout_ratio) if dropout_ratio > 0 else None
        self.pre_seg_conv = None
        if len(hidden_dims) > 0:
            self.pre_seg_conv = build_mlp(in_channel, hidden_dims, norm_cfg, act=act_cfg["type"])
        self.use_sigmoid = loss_decode.get("use_sigmoid", False)
        self.bg_label = self.num_classes
        if not self.use_sigmoid:
            self.num_classes += 1
        self.logit_scale = logit_scale
        self.conv_seg = PointLinear(end_channel, self.num_classes)
        self.voting = PointLinear(end_channel, self.num_classes * 3)
        self.checkpointing = checkpointing
        self.init_bias = init_bias
        self.train_cfg = self.test_cfg = None
        self.init_weights()

    def init_weights(self):
        if self.init_bias is not None:
            self.conv_seg.bias.data.fill_(self.init_bias)
        else:
            nn.init.normal_(self.conv_seg.weight, mean=0, std=0.01)
            nn.init.constant_(self.conv_seg.bias, 0)

    def cls_seg(self, feat):
        if self.dropout is not None:
            feat = self.dropout(feat)
        return self.conv_seg(feat)

    def forward(self, voxel_feat):
        output = voxel_feat
        if self.pre_seg_conv is not None:
            output = self.pre_seg_conv(voxel_feat)
        both = self._seg_and_vote(output)
        if both is not None:
            return both
        return self.cls_seg(output), self.voting(output)

    def _seg_and_vote(self, feat):
        """Inference on the GPU: `conv_seg` (-> classes + 1) and `voting` (-> 3 per class) read the same features, so the two
        Linears are ONE K22 launch on the stacked weight ([11 + 33, 128] for nuScenes: the library ran each of the two thin
        GEMMs over 3e5 rows in ~160 us); the results are the column blocks of one buffer."""
        from .... import hip_ops
        from ...ops.sst_ops import _SMALL_N_MIN

        if (self.training or (torch.is_grad_enabled() and (feat.requires_grad or self.conv_seg.weight.requires_grad))
                or not feat.is_cuda or feat.dim() != 2 or feat.size(0) < _SMALL_N_MIN or (self.dropout is not None and self.training)):
            return None
        c1, c2 = self.conv_seg.out_features, self.voting.out_features
        ctot = (c1 + c2 + 3) // 4 * 4
        if not hip_ops.linear_norm_act_supported(feat, ctot) or self.conv_seg.bias is None or self.voting.bias is None:
            return None
        params = (self.conv_seg.weight, self.conv_seg.bias, self.voting.weight, self.voting.bias)
        key = tuple((p.data_ptr(), p._version) for p in params)
        cache = self.__dict__.get("_fsf_stacked")
        if cache is None or cache[0] != key:
            with torch.no_grad():
                w = torch.zeros((ctot, feat.size(1)), dtype=torch.float32, device=feat.device)
                b = torch.zeros((ctot,), dtype=torch.float32, device=feat.device)
                w[:c1], w[c1:c1 + c2] = self.conv_seg.weight, self.voting.weight
                b[:c1], b[c1:c1 + c2] = self.conv_seg.bias, self.voting.bias
                cache = (key, hip_ops.linear_prepare_weight(w), b)
            self.__dict__["_fsf_stacked"] = cache
        y = hip_ops.linear_norm_act(feat, cache[1], ctot, bias=cache[2])
        return y[:, :c1], y[:, c1:c1 + c2]

    def forward_test(self, inputs, img_metas, test_cfg):
        return self.forward(inputs)

    def forward_train(self, inputs, img_metas, pts_semantic_mask, vote_targets, vote_mask, return_preds=False, fused=True):
        seg_logits, vote_preds = self.forward(inputs)
        losses = self.losses(seg_logits, vote_preds, pts_semantic_mask, vote_targets, vote_mask, fused=fused)
        if return_preds:
            return losses, dict(seg_logits=seg_logits, vote_preds=vote_preds)
        return losses

    # ------------------------------------------------------------------------------------------------ targets
    def _check_train_cfg(self):
        cfg = self.train_cfg or {}
        if cfg.get("extra_width", None) is not None or cfg.get("centroid_offset", False):
            raise NotImplementedError("VoteSegHead targets with extra_width / centroid_offset are not used by the FSF configs")

    def get_targets(self, points_list, gt_bboxes_list, gt_labels_list, fused=True):
        """:206-246 — per-sample points and GT -> (labels i64 [N], vote_targets f32 [N, 3], vote_mask bool [N]), samples concatenated
        in order.  GT rows with label < 0 are dropped.  CUDA points take the device path (K35a) unless fused=False."""
        points = torch.cat([p[:, :3] for p in points_list]) if len(points_list) != 1 else points_list[0]
        if fused and points.is_cuda:
            batch_idx = torch.cat([torch.full((int(p.shape[0]),), b, dtype=torch.int32, device=points.device)
                                   for b, p in enumerate(points_list)])
            return self.get_targets_flat(points, batch_idx, gt_bboxes_list, gt_labels_list)
        self._check_train_cfg()
        out = [seg_targets_host(p, b, l, self.bg_label) for p, b, l in zip(points_list, gt_bboxes_list, gt_labels_list)]
        return tuple(torch.cat([o[k] for o in out], dim=0) for k in range(3))

    def get_targets_flat(self, points, batch_idx, gt_bboxes_list, gt_labels_list, fused=True):
        """`get_targets` on points of every sample in one tensor, row r belonging to sample batch_idx[r] (any row order).  The
        targets of a point depend only on its xyz and its sample's boxes, so these are `get_targets`' rows in this order."""
        self._check_train_cfg()
        if fused and points.is_cuda and points.dtype == torch.float32:
            from .... import hip_ops

            box_ptr, boxes, labels = pack_gt_for_device(gt_bboxes_list, gt_labels_list, points.device)
            pts = points if points.stride(-1) == 1 else points.contiguous()
            labels, targets, mask, _ = hip_ops.seg_targets(pts, batch_idx, box_ptr, boxes, labels, self.bg_label)
            return labels, targets, mask
        labels = torch.empty((points.shape[0],), dtype=torch.long, device=points.device)
        targets = torch.empty((points.shape[0], 3), dtype=torch.float32, device=points.device)
        mask = torch.empty((points.shape[0],), dtype=torch.bool, device=points.device)
        for b, (gb, gl) in enumerate(zip(gt_bboxes_list, gt_labels_list)):
            rows = batch_idx == b
            lb, tg, mk = seg_targets_host(points[rows], gb, gl, self.bg_label)
            labels[rows], targets[rows], mask[rows] = lb, tg, mk
        return labels, targets, mask

    def get_point_labels(self, inbox_inds, bbox_labels):
        bg_mask = inbox_inds < 0
        class_labels = bbox_labels[inbox_inds]
        class_labels[bg_mask] = self.bg_label
        return class_labels

    def get_vote_target(self, inbox_inds, points, bboxes):
        self._check_train_cfg()
        bg_mask = inbox_inds < 0
        rows = gt_box_rows(bboxes).to(points.device).float()
        center = rows[:, :3].clone()
        center[:, 2] = rows[:, 2] + rows[:, 5] * 0.5
        delta = center[inbox_inds] - points[:, :3]
        delta[bg_mask] = 0
        return self.encode_vote_targets(delta), ~bg_mask

    # ------------------------------------------------------------------------------------------------ losses
    def _fused_loss_ok(self, seg_logit, vote_preds):
        return (seg_logit.is_cuda and vote_preds.is_cuda and seg_logit.dtype == torch.float32 and vote_preds.dtype == torch.float32
                and seg_logit.dim() == 2 and vote_preds.dim() == 2 and not self.use_sigmoid and self.loss_aux is None
                and type(self.loss_decode) is CrossEntropyLoss and self.loss_decode.reduction == "mean"
                and type(self.loss_vote) is L1Loss and self.loss_vote.reduction == "mean")

    def _class_weight_on(self, device):
        """`loss_decode.class_weight` as f32 [C] on `device`, uploaded once (pinned, non-blocking)."""
        cw = self.loss_decode.class_weight
        key = (str(device), None if cw is None else tuple(float(w) for w in cw))
        cache = self.__dict__.get("_fsf_class_weight")
        if cache is None or cache[0] != key:
            host = torch.ones(self.num_classes) if cw is None else torch.tensor([float(w) for w in cw])
            assert host.numel() == self.num_classes, "class_weight needs one weight per logit"
            cache = (key, host.float().pin_memory().to(device, non_blocking=True))
            self.__dict__["_fsf_class_weight"] = cache
        return cache[1]

    def losses(self, seg_logit, vote_preds, seg_label, vote_targets, vote_mask, fused=True):
        """:106-167 — dict(loss_sem_seg, loss_vote).  seg_logit [N, C], vote_preds [N, 3C] (column views allowed), seg_label i64 [N],
        vote_targets [N, 3], vote_mask bool [N].  loss_sem_seg = loss_weight * mean_i(w[y_i] * CE_i) (divides by N);
        loss_vote = loss_weight * mean |vote_preds[i, 3y_i:3y_i+3] - t_i| over the masked rows (0, with a zero gradient, when none).
        CUDA fp32 inputs with a CE + L1 config run K35b / K35c (no host sync, no asserts); fused=False or anything else runs the
        reference expression with its asserts."""
        if fused and self._fused_loss_ok(seg_logit, vote_preds):
            if self.logit_scale != 1:
                seg_logit = seg_logit * self.logit_scale
            loss_ce, loss_vote = _SegLossFn.apply(seg_logit, vote_preds, seg_label, vote_targets, vote_mask,
                                                  self._class_weight_on(seg_logit.device), float(self.loss_decode.loss_weight),
                                                  float(self.loss_vote.loss_weight))
            return dict(loss_sem_seg=loss_ce, loss_vote=loss_vote)
        seg_logit, vote_preds = seg_logit.float(), vote_preds.float()
        seg_logit = seg_logit * self.logit_scale
        loss = dict()
        loss["loss_sem_seg"] = self.loss_decode(seg_logit, seg_label)
        if self.loss_aux is not None:
            loss["loss_aux"] = self.loss_aux(seg_logit, seg_label)
        vote_preds = vote_preds.reshape(-1, self.num_classes, 3)
        if not self.use_sigmoid:
            assert seg_label.max().item() == self.num_classes - 1
        else:
            assert seg_label.max().item() == self.num_classes
        valid_vote_preds = vote_preds[vote_mask].reshape(-1, 3)
        num_valid = vote_mask.sum()
        valid_label = seg_label[vote_mask]
        if num_valid > 0:
            assert valid_label.max().item() < self.num_classes
            assert valid_label.min().item() >= 0
            indices = torch.arange(num_valid, device=valid_label.device) * self.num_classes + valid_label
            loss["loss_vote"] = self.loss_vote(valid_vote_preds[indices, :], vote_targets[vote_mask])
        else:
            loss["loss_vote"] = vote_preds.sum() * 0
        return loss

    @staticmethod
    def encode_vote_targets(delta):
        return encode_vote_targets(delta)

    @staticmethod
    def decode_vote_targets(preds):
        if preds.is_cuda and preds.dim() == 2 and preds.dtype == torch.float32 and not (torch.is_grad_enabled() and preds.requires_grad):
            # the result in rows padded to a multiple of four floats: pre_voxelize's mean then reads it with float4 lanes
            c = preds.size(1)
            buf = torch.empty((preds.size(0), (c + 3) // 4 * 4), dtype=torch.float32, device=preds.device)
            return torch.mul(preds, preds.abs(), out=buf[:, :c])
        return preds * preds.abs()
