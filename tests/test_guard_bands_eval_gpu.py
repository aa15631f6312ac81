"""Guard bands and poison around the allocating C-ABI wrapper of hip_ops_eval.py (K41), in the manner of
tests/test_guard_bands_augment_gpu.py: each case calls the wrapper plain, under `guarded(0xFF)` and under `guarded(0x00)`; no guard byte
of an output or scratch buffer may change, the scratch request is exactly `fsf_det_eval_scratch_bytes`, and every result (matches,
curves, the result block) is bit-identical across the three runs: every documented output is written, nothing is read before it is.
tests/test_det_eval_cpu.py fails when a wrapper of the module has no ragged / minimal / empty case here."""
import numpy as np
import pytest
import torch

from det_eval_cases import CLASSES, DIST_THS, concatenated, make_case
from test_guard_bands_gpu import three_runs

pytestmark = pytest.mark.gpu

CASES = {}  # wrapper name -> [(kind, build)], build(ops, dev) -> (run, expected scratch bytes)


def cases(name, **kinds):
    def deco(factory):
        for kind, kw in kinds.items():
            CASES.setdefault(name, []).append((kind, lambda ops, dev, _kw=kw: factory(ops, dev, **_kw)))
        return factory
    return deco


@pytest.fixture(scope="module")
def ops(device):
    from fullysparsefusion_amd import hip_ops_eval

    return hip_ops_eval


@cases("det_eval", ragged=dict(kind="lattice"), ragged_range=dict(kind="continuous", class_range=(6.0, 9.0, 12.0)), minimal=dict(kind="minimal"),
       empty=dict(kind="empty"), no_predictions=dict(kind="lattice", drop="pred"), no_gt=dict(kind="lattice", drop="gt"))
def _det_eval(ops, dev, kind, drop=None, class_range=None):
    from fullysparsefusion_amd import _lib
    from fullysparsefusion_amd.mmdet3d_plugin.core.det_eval import class_flags, first_recall_index

    if kind == "minimal":  # one prediction, one GT
        frames = [dict(pred=np.array([[1, 1, 0, 2, 4, 1.5, 0.1, 0, 0]], dtype=np.float32), score=np.array([0.5], dtype=np.float32),
                       label=np.array([1]), attr=np.array([0]), gt=np.array([[1, 1.5, 0, 2, 4, 1.5, 0, 0, 0]], dtype=np.float32),
                       gt_label=np.array([1]), gt_attr=np.array([0]))]
    elif kind == "empty":  # no samples at all
        frames = []
    else:
        frames = make_case(kind, seed=3)["frames"]
    if frames:
        arrays = list(concatenated(dict(frames=frames)))
    else:
        arrays = [np.zeros((0, 9), np.float32), np.zeros(0, np.float32)] + [np.zeros(0, np.int64)] * 3 + [np.zeros((0, 9), np.float32)] + [np.zeros(0, np.int64)] * 3
    if drop == "pred":
        arrays[:5] = [a[:0] for a in arrays[:5]]
    if drop == "gt":
        arrays[5:] = [a[:0] for a in arrays[5:]]
    tensors = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]
    tensors = [t if t.dtype == torch.float32 else t.to(torch.int32) for t in tensors]
    P, G, S = tensors[0].shape[0], tensors[5].shape[0], len(frames)
    exact = int(_lib.lib().fsf_det_eval_scratch_bytes(P, G, S, len(CLASSES), len(DIST_THS)))

    def run():
        return list(ops.det_eval(*tensors, S, class_flags(CLASSES), DIST_THS, 2, first_recall_index(0.1), 0.1, 5.0, class_range))
    return run, exact


@pytest.mark.parametrize("name,kind", [(n, k) for n in sorted(CASES) for k, _ in CASES[n]])
def test_wrapper_under_guard_bands_and_poison(ops, device, name, kind):
    run, exact = dict(CASES[name])[kind](ops, device)

    def scratch_expected(g):
        assert g.workspace_sizes == [exact] and exact > 0, (g.workspace_sizes, exact)
        assert any(r["kind"] == "workspace" and r["site"] == name for r in g.records)

    match, curves, result = three_runs(run, scratch_expected)
    T, C = len(DIST_THS), len(CLASSES)
    assert curves.shape == (C, 2 * T + 5, 101) and result.shape == (8 + C * (3 * T + 7),) and match.shape[0] == T
    assert bool(torch.isfinite(curves).all())
    if kind in ("ragged", "ragged_range"):
        assert 0 < int((match >= 0).sum()) < match.numel() and float(result[0]) > 0
    elif kind == "minimal":
        assert match.tolist() == [[-1], [0], [0], [0]] and abs(float(result[8 + 4 + 2]) - 1.0) < 1e-12  # 0.5 m apart: a miss at 0.5; barrier AP at 2 m
    else:
        assert float(result[0]) == 0.0 and float(result[6]) == 0.0 and bool((curves[:, :2 * T] == 0).all()) and bool((curves[:, 2 * T:] == 1).all())
        assert bool((result[-C * T:] == 1).all())  # every (class, threshold) took the no_predictions path
