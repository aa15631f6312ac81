"""Thin torch-tensor wrapper of the detection-metric kernels in libfsf_hip.so (K41: include/fsf_hip.h, docs/kernels/K41_det_eval.md).
`mmdet3d_plugin.core.det_eval.DeviceDetectionEval` is the public interface.

Same rules as hip_ops.py / hip_ops_augment.py: the function only marshals pointers / sizes and allocates caller-owned outputs
(`torch.empty`) and scratch (`_lib.workspace`); all arithmetic happens in the HIP kernels; nothing here waits for the device.  It has
ragged / minimal / empty guard-band cases in tests/test_guard_bands_eval_gpu.py (tests/test_det_eval_cpu.py holds it to that).
"""
import ctypes

import torch

from . import _lib
from ._lib import c_p, check, i32_array, ptr, require_cuda, stream_ptr
from .hip_ops import _L

MAX_CLASSES = _lib.DEFINES["FSF_DET_EVAL_MAX_CLASSES"]
MAX_THRESHOLDS = _lib.DEFINES["FSF_DET_EVAL_MAX_THRESHOLDS"]
HEAD = _lib.DEFINES["FSF_DET_EVAL_HEAD"]
POINTS = 101


def _f64_array(vals):
    return (ctypes.c_double * len(vals))(*[float(v) for v in vals])


def det_eval(pred: torch.Tensor, score: torch.Tensor, pred_label: torch.Tensor, pred_attr: torch.Tensor, pred_sample: torch.Tensor,
             gt: torch.Tensor, gt_label: torch.Tensor, gt_attr: torch.Tensor, gt_sample: torch.Tensor, num_samples: int, class_flags,
             dist_ths, tp_threshold: int, first_recall: int, min_precision: float, mean_ap_weight: float, class_range=None):
    """fsf_det_eval_compute (K41a match, K41b curves, K41c summary behind two radix sorts): the accumulated predictions f32 [P, 9] (x y z
    w l h yaw vx vy) with score f32 / label i32 / attribute i32 / sample i32 [P] and ground truth f32 [G, 9] with label / attribute /
    sample i32 [G], both sample-major with non-decreasing sample ids in [0, num_samples) -> (match i32 [T, P]: the matched GT row of every
    prediction per threshold or -1; curves f64 [C, 2 T + 5, 101]: precision per threshold, confidence per threshold, the five error curves
    of threshold `tp_threshold`; result f64 [HEAD + C (3 T + 7)]: mAP, mATE, mASE, mAOE, mAVE, mAAE, NDS, 0, then AP [C, T], TP errors
    [C, 5], npos [C], predictions [C], true positives [C, T], no_predictions [C, T]).  `class_flags`: per class bit 0 = orientation period
    pi, bit 1 + e = error e undefined.  No sync: the caller reads `result` back."""
    require_cuda(pred, score, pred_label, pred_attr, pred_sample, gt, gt_label, gt_attr, gt_sample)
    P, G, C, T = pred.shape[0], gt.shape[0], len(class_flags), len(dist_ths)
    assert pred.dtype == torch.float32 and gt.dtype == torch.float32 and score.dtype == torch.float32
    assert pred.shape == (P, 9) and gt.shape == (G, 9) and score.shape == (P,)
    for t, n in ((pred_label, P), (pred_attr, P), (pred_sample, P), (gt_label, G), (gt_attr, G), (gt_sample, G)):
        assert t.dtype == torch.int32 and t.shape == (n,)
    assert 1 <= C <= MAX_CLASSES and 1 <= T <= MAX_THRESHOLDS and 0 <= tp_threshold < T and (class_range is None or len(class_range) == C)
    dev = pred.device
    match = torch.empty((T, P), dtype=torch.int32, device=dev)
    curves = torch.empty((C, 2 * T + 5, POINTS), dtype=torch.float64, device=dev)
    result = torch.empty((HEAD + C * (3 * T + 7),), dtype=torch.float64, device=dev)
    h = _L()
    assert result.numel() == h.fsf_det_eval_result_words(C, T)
    ws = _lib.workspace(h.fsf_det_eval_scratch_bytes(P, G, int(num_samples), C, T), dev)
    p = ptr if P else (lambda t: c_p(None))
    g = ptr if G else (lambda t: c_p(None))
    check(h.fsf_det_eval_compute(p(pred), p(score), p(pred_label), p(pred_attr), p(pred_sample), P, g(gt), g(gt_label), g(gt_attr),
                                 g(gt_sample), G, int(num_samples), C, i32_array(class_flags),
                                 _f64_array(class_range) if class_range is not None else c_p(None), _f64_array(dist_ths), T,
                                 int(tp_threshold), int(first_recall), _f64_array([min_precision, mean_ap_weight]), p(match), ptr(curves),
                                 ptr(result), ptr(ws), ws.numel(), stream_ptr()),
          "fsf_det_eval_compute")
    return match, curves, result
