"""Inputs shared by tests/test_det_eval_cpu.py and tests/test_det_eval_gpu.py (a plain helper module, not a conftest): a small
validation set that reaches every path of K41 (docs/kernels/K41_det_eval.md), and the host specification's answer for it, computed once.

7 samples, 3 classes (one named `barrier`, one `traffic_cone`).  Predictions per sample from {0, 1, 5, 70, 501}; ground truth per
(sample, class) from {0, 1, 2, 65, 130}: more than one pass of the 64 lanes over a sample's GT and more than one 64-bit word of
taken marks.  The `lattice` case makes ties frequent and exact in binary: scores from 16 values, centres on a 0.25 m lattice (distances
of exactly 0.5 / 1 / 2 / 4 m occur), one class with GT and no predictions, one sample with predictions and no GT, part of the GT
velocities NaN and part of the GT attributes -1, some labels -1 (ignored rows).  The `continuous` case draws everything at random."""
import functools

import numpy as np

CLASSES = ("car", "barrier", "traffic_cone")
DIST_THS = (0.5, 1.0, 2.0, 4.0)
PRED_PER_SAMPLE = (501, 0, 1, 5, 70, 501, 70)
GT_PER_SAMPLE_CLASS = ((130, 65, 2), (1, 0, 1), (2, 1, 0), (0, 0, 0), (65, 2, 1), (2, 130, 0), (1, 1, 65))


def make_case(kind, seed=0):
    """-> dict(frames=[per sample dict(pred, score, label, attr, gt, gt_label, gt_attr)]) of numpy arrays (f32 rows / scores, i64 ids)."""
    rng = np.random.default_rng(seed)
    lattice = kind == "lattice"
    frames = []
    for n, per_class in zip(PRED_PER_SAMPLE, GT_PER_SAMPLE_CLASS):
        gt_label = rng.permutation(np.repeat(np.arange(len(CLASSES)), per_class))  # the classes mixed in stored order
        g = gt_label.size

        def rows(m):
            r = np.zeros((m, 9), dtype=np.float32)
            r[:, :2] = rng.integers(0, 40, (m, 2)) * 0.25 if lattice else rng.random((m, 2)) * 10
            r[:, 2] = rng.normal(size=m)
            r[:, 3:6] = rng.random((m, 3)) * 3.5 + 0.5
            r[:, 6] = rng.uniform(-4, 4, m)
            r[:, 7:] = rng.normal(size=(m, 2))
            return r

        gt, pred = rows(g), rows(n)
        gt[rng.random(g) < 0.2, 7:] = np.nan
        gt_attr = rng.integers(-1, 4, g)
        gt_label = np.where(rng.random(g) < 0.05, -1, gt_label)
        label = rng.integers(0, 2 if lattice else 3, n)  # lattice: no prediction of class 2, which has GT
        label = np.where(rng.random(n) < 0.05, -1, label)
        score = (rng.integers(1, 17, n) / 16).astype(np.float32) if lattice else rng.random(n).astype(np.float32)
        frames.append(dict(pred=pred, score=score, label=label.astype(np.int64), attr=rng.integers(0, 4, n).astype(np.int64), gt=gt,
                           gt_label=gt_label.astype(np.int64), gt_attr=gt_attr.astype(np.int64)))
    return dict(frames=frames)


def concatenated(case):
    """The frames as the nine arrays of `evaluate_host` (sample-major, sample ids from the frame index)."""
    f = case["frames"]
    cat = lambda key: np.concatenate([x[key] for x in f])  # noqa: E731
    psample = np.concatenate([np.full(x["score"].size, k) for k, x in enumerate(f)])
    gsample = np.concatenate([np.full(x["gt_label"].size, k) for k, x in enumerate(f)])
    return (cat("pred"), cat("score"), cat("label"), cat("attr"), psample, cat("gt"), cat("gt_label"), cat("gt_attr"), gsample)


@functools.lru_cache(maxsize=None)
def case_and_reference(kind, class_range=None):
    """(case, (match, curves, result) of the host specification); computed once per process and never modified."""
    from fullysparsefusion_amd.mmdet3d_plugin.core.det_eval import evaluate_host

    case = make_case(kind, seed=7 if kind == "lattice" else 8)
    ref = evaluate_host(*concatenated(case), CLASSES, DIST_THS, class_range=list(class_range) if class_range else None)
    for a in ref:
        a.setflags(write=False)
    return case, ref
