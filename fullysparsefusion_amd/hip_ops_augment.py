"""Thin torch-tensor wrappers of the train-time augmentation kernels in libfsf_hip.so (K40: include/fsf_hip.h,
docs/kernels/K40_train_augment.md).  `mmdet3d_plugin.datasets.train_augment.DeviceTrainAugment` is the public interface.

Same rules as hip_ops.py / hip_ops_optim.py: the functions only marshal pointers / sizes and allocate caller-owned outputs
(`torch.empty`) and scratch (`_lib.workspace`); all arithmetic happens in the HIP kernels; nothing here waits for the device.  Every
allocating function has ragged / minimal / empty guard-band cases in tests/test_guard_bands_augment_gpu.py
(tests/test_train_augment_cpu.py holds it to that).
"""
import torch

from . import _lib
from ._lib import c_p, check, f32_array, i64_array, ptr, require_cuda, stream_ptr
from .hip_ops import _L, _rows_view

DESC_WORDS = _lib.DEFINES["FSF_TRAIN_AUGMENT_DESC_WORDS"]
MAX_BATCH = _lib.DEFINES["FSF_TRAIN_AUGMENT_MAX_BATCH"]


def train_augment_points(points: torch.Tensor, desc, pc_range=None, shuffle_seed: int = -1, count: torch.Tensor = None):
    """fsf_train_augment_points (K40a, the radix sort, K40b): ONE frame's cloud f32 [n, C] (xyz | features | no-aug xyz) + its host
    descriptor (cos, sin, scale, angle, rotate, flip_h, flip_v, tx, ty, tz) -> (out f32 [n, C] capacity, count i64 [1] on the device):
    rows [0, count) of `out` are the flipped, rotated, scaled, translated rows that pass the strict range test on the augmented xyz, in
    the order of the seed's key mix (`shuffle_seed >= 0`) or in source order (`< 0`).  `count`: a caller-owned i64 [1] device view
    (one element of a per-batch tensor, read back once for all frames) instead of a new tensor.  No sync: the caller reads `count`."""
    require_cuda(points, count)
    assert points.dtype == torch.float32 and points.dim() == 2 and points.size(1) >= 3 and len(desc) == DESC_WORDS
    points = points.contiguous()
    n, cols = points.shape
    out = torch.empty((n, cols), dtype=torch.float32, device=points.device)
    if count is None:
        count = torch.empty((1,), dtype=torch.int64, device=points.device)
    assert count.dtype == torch.int64 and count.numel() == 1
    h = _L()
    ws = _lib.workspace(h.fsf_train_augment_points_workspace_bytes(n), points.device)
    check(h.fsf_train_augment_points(ptr(points) if n else c_p(None), n, cols, f32_array(desc),
                                     f32_array(pc_range) if pc_range is not None else c_p(None), int(shuffle_seed),
                                     ptr(out) if n else c_p(None), ptr(count), c_p(None), ptr(ws), ws.numel(), stream_ptr()),
          "fsf_train_augment_points")
    return out, count


def train_augment_boxes(boxes: torch.Tensor, labels: torch.Tensor, no_aug_boxes: torch.Tensor, no_aug_labels: torch.Tensor,
                        sample_offsets, descs, pc_range):
    """fsf_train_augment_boxes (K40c): a batch's concatenated GT boxes f32 [g, 7..16] (row-strided views are taken as they are) and
    labels i64 [g], the un-augmented ones, `sample_offsets` (num_samples + 1 host ints) and one host descriptor per sample ->
    (boxes f32 [g, D] augmented with yaw wrapped, labels i64 [g] with -1 on the rows MyObjectRangeFilter drops, no-aug boxes with yaw
    wrapped, no-aug labels with the same -1).  One launch, no scratch, no sync."""
    require_cuda(boxes, labels, no_aug_boxes, no_aug_labels)
    assert boxes.dtype == torch.float32 and no_aug_boxes.dtype == torch.float32 and boxes.dim() == 2 and no_aug_boxes.shape == boxes.shape
    assert labels.dtype == torch.int64 and no_aug_labels.dtype == torch.int64
    assert len(descs) == len(sample_offsets) - 1 and all(len(d) == DESC_WORDS for d in descs)
    boxes, stride = _rows_view(boxes)
    no_aug_boxes, na_stride = _rows_view(no_aug_boxes)
    labels, no_aug_labels = labels.contiguous(), no_aug_labels.contiguous()
    g, dim = boxes.shape
    assert labels.numel() == g and no_aug_labels.numel() == g and int(sample_offsets[-1]) == g
    dev = boxes.device
    boxes_out = torch.empty((g, dim), dtype=torch.float32, device=dev)
    labels_out = torch.empty((g,), dtype=torch.int64, device=dev)
    na_boxes_out = torch.empty((g, dim), dtype=torch.float32, device=dev)
    na_labels_out = torch.empty((g,), dtype=torch.int64, device=dev)
    p = (lambda t: c_p(t.data_ptr())) if g else (lambda t: c_p(None))
    check(_L().fsf_train_augment_boxes(p(boxes), stride, dim, p(labels), p(no_aug_boxes), na_stride, p(no_aug_labels),
                                       i64_array(sample_offsets), len(descs), f32_array([v for d in descs for v in d]),
                                       f32_array(pc_range), p(boxes_out), p(labels_out), p(na_boxes_out), p(na_labels_out), stream_ptr()),
          "fsf_train_augment_boxes")
    return boxes_out, labels_out, na_boxes_out, na_labels_out
