"""Thin torch-tensor wrapper of the refine-stage heads' target assignment in libfsf_hip.so (K38, `FrustumAssigner` + `DistAssigner`:
include/fsf_hip.h, docs/kernels/K38_frustum_assign.md).

Same rules as hip_ops.py / hip_ops_assign.py: the function only marshals pointers / sizes and allocates caller-owned outputs
(`torch.empty`) and scratch (`_lib.workspace`); all arithmetic happens in the HIP kernels; nothing here waits for the device.  Every
allocating function has ragged / minimal / empty guard-band cases in tests/test_guard_bands_frustum_gpu.py
(tests/test_frustum_assign_cpu.py holds it to that).
"""
import torch

from . import _lib
from ._lib import c_p, check, ptr, require_cuda, stream_ptr
from .hip_ops import _L


def frustum_assign(cluster_xyz: torch.Tensor, batch_idx: torch.Tensor, preds_2d: torch.Tensor, box_ptr_2d: torch.Tensor,
                   boxes_2d: torch.Tensor, keep_2d: torch.Tensor, box_ptr: torch.Tensor, boxes: torch.Tensor, box_labels: torch.Tensor,
                   num_classes: int, code_size: int, extra_height: float = 0.0, pos_iou_thr: float = 0.7, min_pos_iou: float = 0.3,
                   old_cls_logits: torch.Tensor = None, class_max_dist: torch.Tensor = None):
    """fsf_frustum_assign (K38): the arguments of `hip_ops_assign.hybrid_assign`, plus the previous stage's class logits
    f32 [n, >= num_classes] (any row stride) and the per-class radii f32 [num_classes] (<= 0: never) -> (labels i64 [n],
    bbox_targets f32 [n, code], bbox_weights f32 [n, code], assigned i32 [n] = row inside the sample's augmented GT or -1,
    source i32 [n] = 0 none / 1 3-D / 2 2-D / 3 distance, stats f32 [6]), all on the device.  3-D containment first, MaxIoUAssigner on
    the 2-D boxes for the rest, then the nearest GT of the previously predicted class inside its radius.  `class_max_dist=None`: no
    distance step, the outputs are `hybrid_assign`'s bit for bit.  No sync."""
    require_cuda(cluster_xyz, batch_idx, preds_2d, box_ptr_2d, boxes_2d, keep_2d, box_ptr, boxes, box_labels)
    assert cluster_xyz.dtype == torch.float32 and cluster_xyz.dim() == 2 and cluster_xyz.size(1) >= 3
    if cluster_xyz.stride(1) != 1:
        cluster_xyz = cluster_xyz.contiguous()
    n, m, dev = cluster_xyz.size(0), boxes.size(0), cluster_xyz.device
    assert batch_idx.dtype in (torch.int32, torch.int64) and batch_idx.dim() == 1 and batch_idx.numel() == n
    assert preds_2d.dtype == torch.float32 and preds_2d.dim() == 2 and preds_2d.size(0) == n and preds_2d.size(1) >= 7
    if preds_2d.stride(1) != 1:
        preds_2d = preds_2d.contiguous()
    assert box_ptr.dtype == torch.int32 and box_ptr.dim() == 1 and box_ptr.numel() >= 1
    assert box_ptr_2d.dtype == torch.int32 and box_ptr_2d.shape == box_ptr.shape, "both GT lists describe the same samples"
    assert boxes_2d.dtype == torch.float32 and boxes_2d.dim() == 3 and boxes_2d.size(2) == 4 and boxes_2d.size(1) >= 1
    m2, ncam = boxes_2d.size(0), boxes_2d.size(1)
    assert keep_2d.dtype == torch.int32 and keep_2d.shape == (m2, ncam)
    assert boxes.dtype == torch.float32 and boxes.dim() == 2 and (boxes.size(0) == 0 or boxes.stride(1) == 1)
    assert box_labels.dtype == torch.int32 and box_labels.dim() == 1 and box_labels.numel() == m
    code, num_classes = int(code_size), int(num_classes)
    assert code in (8, 10) and (m == 0 or (boxes.size(1) in (7, 9, 10) and (boxes.size(1) == 7) == (code == 8))), \
        "the coder appends box columns 7, 8 exactly when the boxes have them (7 columns <-> code size 8)"
    if n > 1 and batch_idx.stride(0) < 1:
        batch_idx = batch_idx.contiguous()
    logits_stride = num_classes
    if class_max_dist is not None:
        assert old_cls_logits is not None, "the distance step needs old_cls_logits (the previous stage's class logits)"
        require_cuda(old_cls_logits, class_max_dist)
        assert class_max_dist.dtype == torch.float32 and class_max_dist.dim() == 1 and class_max_dist.numel() == num_classes
        assert old_cls_logits.dtype == torch.float32 and old_cls_logits.dim() == 2 and old_cls_logits.size(0) == n
        assert old_cls_logits.size(1) >= num_classes
        if old_cls_logits.stride(1) != 1 or (n > 1 and old_cls_logits.stride(0) < num_classes):
            old_cls_logits = old_cls_logits.contiguous()
        class_max_dist = class_max_dist.contiguous()
        logits_stride = old_cls_logits.stride(0) if n > 1 else max(old_cls_logits.size(1), num_classes)
    box_ptr, box_labels, box_ptr_2d = box_ptr.contiguous(), box_labels.contiguous(), box_ptr_2d.contiguous()
    boxes_2d, keep_2d = boxes_2d.contiguous(), keep_2d.contiguous()
    labels = torch.empty((n,), dtype=torch.int64, device=dev)
    targets = torch.empty((n, code), dtype=torch.float32, device=dev)
    weights = torch.empty((n, code), dtype=torch.float32, device=dev)
    assigned = torch.empty((n,), dtype=torch.int32, device=dev)
    source = torch.empty((n,), dtype=torch.int32, device=dev)
    stats = torch.empty((6,), dtype=torch.float32, device=dev)
    h = _L()
    ws = _lib.workspace(h.fsf_frustum_assign_workspace_bytes(m, m2, ncam, n), dev)
    with_dist = class_max_dist is not None
    check(h.fsf_frustum_assign(c_p(cluster_xyz.data_ptr()) if n else c_p(None), n, cluster_xyz.stride(0) if n > 1 else 3,
                               c_p(batch_idx.data_ptr()) if n else c_p(None), batch_idx.element_size(),
                               batch_idx.stride(0) if n > 1 else 1, c_p(preds_2d.data_ptr()) if n else c_p(None),
                               preds_2d.stride(0) if n > 1 else max(preds_2d.size(1), 7), ptr(box_ptr_2d),
                               ptr(boxes_2d) if m2 else c_p(None), ptr(keep_2d) if m2 else c_p(None), m2, ncam, ptr(box_ptr),
                               box_ptr.numel() - 1, c_p(boxes.data_ptr()) if m else c_p(None), m,
                               boxes.stride(0) if m > 1 else max(boxes.size(1), 7), boxes.size(1) if m else 7, ptr(box_labels),
                               num_classes, code, float(extra_height), float(pos_iou_thr), float(min_pos_iou),
                               c_p(old_cls_logits.data_ptr()) if with_dist and n else c_p(None), logits_stride,
                               ptr(class_max_dist) if with_dist else c_p(None), ptr(ws), ws.numel(), ptr(labels), ptr(targets),
                               ptr(weights), ptr(assigned), ptr(source) if n else c_p(None), ptr(stats), stream_ptr()),
          "fsf_frustum_assign")
    return labels, targets, weights, assigned, source, stats
