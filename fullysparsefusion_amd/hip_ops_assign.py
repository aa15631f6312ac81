"""Thin torch-tensor wrappers of the target-assignment entry points of libfsf_hip.so that came after hip_ops.py's set (K37, the
camera-query head's hybrid 3-D / 2-D assigner: include/fsf_hip.h, docs/kernels/K37_hybrid_assign.md).

Same rules as hip_ops.py: the functions only marshal pointers / sizes and allocate caller-owned outputs (`torch.empty`) and scratch
(`_lib.workspace`); all arithmetic happens in the HIP kernels; nothing here waits for the device.  Every allocating function has
ragged / minimal / empty guard-band cases in tests/test_guard_bands_assign_gpu.py (tests/test_hybrid_assign_cpu.py holds it to that).
"""
import torch

from . import _lib
from ._lib import c_p, check, ptr, require_cuda, stream_ptr
from .hip_ops import _L

CANVAS = (1600.0, 900.0)  # upstream's image canvas (post_process_coords: imsize = (1600, 900))


def gt_boxes_2d(boxes: torch.Tensor, box_labels: torch.Tensor, box_ptr: torch.Tensor, lidar2img: torch.Tensor, canvas=CANVAS):
    """fsf_gt_boxes_2d (K37a): un-augmented GT boxes f32 [M, >= 7] in the task's order, box_labels i32 [M] (rows < 0 are dropped),
    per-sample CSR box_ptr i32 [B + 1], lidar2img f32 [B, ncam, 4, 4] -> (boxes_2d f32 [M, ncam, 4], keep i32 [M, ncam]): the clipped
    image-plane bounding box of every box in every camera of its sample, and whether there is one.  No sync."""
    require_cuda(boxes, box_labels, box_ptr, lidar2img)
    assert boxes.dtype == torch.float32 and boxes.dim() == 2 and (boxes.size(0) == 0 or boxes.stride(1) == 1)
    assert box_labels.dtype == torch.int32 and box_labels.dim() == 1 and box_labels.numel() == boxes.size(0)
    assert box_ptr.dtype == torch.int32 and box_ptr.dim() == 1 and box_ptr.numel() >= 1
    assert lidar2img.dtype == torch.float32 and lidar2img.dim() == 4 and lidar2img.shape[2:] == (4, 4)
    assert lidar2img.size(0) == box_ptr.numel() - 1, "one set of camera matrices per sample"
    m, ncam, dev = boxes.size(0), lidar2img.size(1), boxes.device
    assert m == 0 or boxes.size(1) >= 7
    box_ptr, box_labels, lidar2img = box_ptr.contiguous(), box_labels.contiguous(), lidar2img.contiguous()
    boxes_2d = torch.empty((m, ncam, 4), dtype=torch.float32, device=dev)
    keep = torch.empty((m, ncam), dtype=torch.int32, device=dev)
    check(_L().fsf_gt_boxes_2d(c_p(boxes.data_ptr()) if m else c_p(None), m, boxes.stride(0) if m > 1 else max(boxes.size(1), 7),
                               ptr(box_labels), ptr(box_ptr), box_ptr.numel() - 1, ptr(lidar2img), ncam, float(canvas[0]),
                               float(canvas[1]), ptr(boxes_2d), ptr(keep), stream_ptr()), "fsf_gt_boxes_2d")
    return boxes_2d, keep


def hybrid_assign(cluster_xyz: torch.Tensor, batch_idx: torch.Tensor, preds_2d: torch.Tensor, box_ptr_2d: torch.Tensor,
                  boxes_2d: torch.Tensor, keep_2d: torch.Tensor, box_ptr: torch.Tensor, boxes: torch.Tensor, box_labels: torch.Tensor,
                  num_classes: int, code_size: int, extra_height: float = 0.0, pos_iou_thr: float = 0.7, min_pos_iou: float = 0.3):
    """fsf_hybrid_assign (K37b): query centres f32 [n, >= 3], batch_idx i32 / i64 [n] (any element stride), preds_2d f32 [n, >= 7]
    (2-D box in columns 0..3, camera id in column 6), the un-augmented GT's CSR box_ptr_2d i32 [B + 1] with K37a's boxes_2d
    f32 [M0, ncam, 4] / keep_2d i32 [M0, ncam], and the augmented GT as `hip_ops.cluster_targets` takes it -> (labels i64 [n],
    bbox_targets f32 [n, code], bbox_weights f32 [n, code], assigned i32 [n] = row inside the sample's augmented GT or -1,
    stats f32 [6]), all on the device.  3-D containment first, MaxIoUAssigner on the 2-D boxes for the rest.  No sync."""
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
    code = int(code_size)
    assert code in (8, 10) and (m == 0 or (boxes.size(1) in (7, 9, 10) and (boxes.size(1) == 7) == (code == 8))), \
        "the coder appends box columns 7, 8 exactly when the boxes have them (7 columns <-> code size 8)"
    if n > 1 and batch_idx.stride(0) < 1:
        batch_idx = batch_idx.contiguous()
    box_ptr, box_labels, box_ptr_2d = box_ptr.contiguous(), box_labels.contiguous(), box_ptr_2d.contiguous()
    boxes_2d, keep_2d = boxes_2d.contiguous(), keep_2d.contiguous()
    labels = torch.empty((n,), dtype=torch.int64, device=dev)
    targets = torch.empty((n, code), dtype=torch.float32, device=dev)
    weights = torch.empty((n, code), dtype=torch.float32, device=dev)
    assigned = torch.empty((n,), dtype=torch.int32, device=dev)
    stats = torch.empty((6,), dtype=torch.float32, device=dev)
    h = _L()
    ws = _lib.workspace(h.fsf_hybrid_assign_workspace_bytes(m, m2, ncam, n), dev)
    check(h.fsf_hybrid_assign(c_p(cluster_xyz.data_ptr()) if n else c_p(None), n, cluster_xyz.stride(0) if n > 1 else 3,
                              c_p(batch_idx.data_ptr()) if n else c_p(None), batch_idx.element_size(),
                              batch_idx.stride(0) if n > 1 else 1, c_p(preds_2d.data_ptr()) if n else c_p(None),
                              preds_2d.stride(0) if n > 1 else max(preds_2d.size(1), 7), ptr(box_ptr_2d),
                              ptr(boxes_2d) if m2 else c_p(None), ptr(keep_2d) if m2 else c_p(None), m2, ncam, ptr(box_ptr),
                              box_ptr.numel() - 1, c_p(boxes.data_ptr()) if m else c_p(None), m,
                              boxes.stride(0) if m > 1 else max(boxes.size(1), 7), boxes.size(1) if m else 7, ptr(box_labels),
                              int(num_classes), code, float(extra_height), float(pos_iou_thr), float(min_pos_iou), ptr(ws), ws.numel(),
                              ptr(labels), ptr(targets), ptr(weights), ptr(assigned), ptr(stats), stream_ptr()), "fsf_hybrid_assign")
    return labels, targets, weights, assigned, stats
