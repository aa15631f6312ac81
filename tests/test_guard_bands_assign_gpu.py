"""Guard bands and poison around the allocating C-ABI wrappers of hip_ops_assign.py (K37), in the manner of
tests/test_guard_bands_gpu.py: each case calls its wrapper plain, under `guarded(0xFF)` and under `guarded(0x00)`; no guard byte of an
output or scratch buffer may change, the scratch request is exactly `fsf_hybrid_assign_workspace_bytes`, and every returned tensor is
bit-identical across the three runs.  tests/test_hybrid_assign_cpu.py fails when a wrapper of the module has no ragged / minimal /
empty case here."""
import numpy as np
import pytest
import torch

from test_guard_bands_gpu import G, gt_boxes, points5, three_runs, wide
from fullysparsefusion_amd import synthetic

pytestmark = pytest.mark.gpu

CASES = {}  # wrapper name -> [(kind, build)], build(ops, dev) -> (run, expected scratch bytes or None)


def cases(name, **kinds):
    def deco(factory):
        for kind, kw in kinds.items():
            CASES.setdefault(name, []).append((kind, lambda ops, dev, _kw=kw: factory(ops, dev, **_kw)))
        return factory
    return deco


@pytest.fixture(scope="module")
def ops(device):
    from fullysparsefusion_amd import hip_ops_assign

    return hip_ops_assign


def _gt(dev, per_sample, dim, seed):
    pts = points5(dev, 4001, seed)
    m = sum(per_sample)
    boxes = gt_boxes(dev, pts, m, dim, seed + 1)
    labels = torch.randint(-1, 10, (m,), generator=G(seed + 2)).to(torch.int32).to(dev)
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(per_sample)]), dtype=torch.int32, device=dev)
    l2i = torch.from_numpy(np.stack([synthetic.make_lidar2img()] * len(per_sample)).astype(np.float32)).to(dev)
    return pts, boxes, labels, ptr, l2i


@cases("gt_boxes_2d", ragged=dict(per_sample=(7, 0, 13)), minimal=dict(per_sample=(1,)), empty=dict(per_sample=(0, 0)))
def _gt_boxes_2d(ops, dev, per_sample):
    _, boxes, labels, ptr, l2i = _gt(dev, per_sample, 9, 31)
    rows = wide(boxes) if boxes.size(0) else boxes
    return (lambda: ops.gt_boxes_2d(rows, labels, ptr, l2i)), None


@cases("hybrid_assign", ragged=dict(n=1009, per_sample=(7, 0, 13), code=10), minimal=dict(n=1, per_sample=(1,), code=8),
       empty=dict(n=0, per_sample=(3, 2), code=10))
def _hybrid_assign(ops, dev, n, per_sample, code):
    pts, boxes, labels, ptr, l2i = _gt(dev, per_sample, 9 if code == 10 else 7, 37)
    boxes_2d, keep = ops.gt_boxes_2d(boxes, labels, ptr, l2i)
    g = G(41)
    xyz = pts[torch.randint(0, pts.size(0), (n,), generator=g).to(dev), :3].contiguous()
    table = torch.stack([torch.randint(0, len(per_sample), (n,), generator=g), torch.zeros(n, dtype=torch.long),
                         torch.arange(n)], 1).to(dev)
    preds = torch.cat([torch.rand((n, 2), generator=g) * 1200, torch.rand((n, 2), generator=g) * 300 + 1300,
                       torch.rand((n, 2), generator=g), torch.randint(0, 6, (n, 1), generator=g).float(), torch.zeros((n, 2))], 1).to(dev)
    if n and boxes_2d.size(0):  # some detections sit on projected boxes, so that the 2-D branch assigns
        k = torch.nonzero(keep.reshape(-1)).reshape(-1)[:n // 2]
        preds[:k.numel(), :4] = boxes_2d.reshape(-1, 4)[k]
        preds[:k.numel(), 6] = (k % 6).float()
    preds = wide(preds) if n else preds
    from fullysparsefusion_amd import _lib
    exact = int(_lib.lib().fsf_hybrid_assign_workspace_bytes(boxes.size(0), boxes_2d.size(0), 6, n))
    return (lambda: ops.hybrid_assign(xyz, table[:, 0], preds, ptr, boxes_2d, keep, ptr, boxes, labels, 10, code, 0.1)), exact


@pytest.mark.parametrize("name,kind", [(n, k) for n in sorted(CASES) for k, _ in CASES[n]])
def test_wrapper_under_guard_bands_and_poison(ops, device, name, kind):
    run, exact = dict(CASES[name])[kind](ops, device)

    def scratch_expected(g):
        if exact is None:
            assert g.counts["workspace"] == 0
        else:
            assert g.workspace_sizes == [exact] and exact > 0, (g.workspace_sizes, exact)
            assert any(r["kind"] == "workspace" and r["site"] == name for r in g.records)

    plain = three_runs(run, scratch_expected)
    assert len(plain) == (2 if name == "gt_boxes_2d" else 5)
