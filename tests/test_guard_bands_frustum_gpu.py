"""Guard bands and poison around the allocating C-ABI wrapper of hip_ops_frustum.py (K38), in the manner of
tests/test_guard_bands_assign_gpu.py: each case calls the wrapper plain, under `guarded(0xFF)` and under `guarded(0x00)`; no guard byte
of an output or scratch buffer may change, the scratch request is exactly `fsf_frustum_assign_workspace_bytes`, and every returned
tensor is bit-identical across the three runs.  tests/test_frustum_assign_cpu.py fails when a wrapper of the module has no ragged /
minimal / empty case here."""
import pytest
import torch

from test_guard_bands_assign_gpu import _gt  # noqa: F401  (the GT builder of K37's file)
from test_guard_bands_gpu import G, three_runs, wide

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
    from fullysparsefusion_amd import hip_ops_frustum

    return hip_ops_frustum


@cases("frustum_assign", ragged=dict(n=1009, per_sample=(7, 0, 13), code=10), minimal=dict(n=1, per_sample=(1,), code=8),
       empty=dict(n=0, per_sample=(3, 2), code=10))
def _frustum_assign(ops, dev, n, per_sample, code):
    from fullysparsefusion_amd import _lib, hip_ops_assign

    pts, boxes, labels, ptr, l2i = _gt(dev, per_sample, 9 if code == 10 else 7, 37)
    boxes_2d, keep = hip_ops_assign.gt_boxes_2d(boxes, labels, ptr, l2i)
    g = G(43)
    table = torch.stack([torch.randint(0, len(per_sample), (n,), generator=g), torch.zeros(n, dtype=torch.long),
                         torch.arange(n)], 1).to(dev)
    xyz = pts[torch.randint(0, pts.size(0), (n,), generator=g).to(dev), :3].contiguous()
    preds = torch.cat([torch.rand((n, 2), generator=g) * 1200, torch.rand((n, 2), generator=g) * 300 + 1300,
                       torch.rand((n, 2), generator=g), torch.randint(0, 6, (n, 1), generator=g).float(), torch.zeros((n, 2))], 1).to(dev)
    old = torch.randn((n, 10), generator=g).to(dev)
    if n and boxes.size(0):  # a third of the queries sit above a box of their own sample, so that the distance step assigns
        lo, hi = ptr[table[:, 0]].long(), ptr[table[:, 0] + 1].long()
        k = (lo + torch.arange(n, device=dev) % (hi - lo).clamp(min=1)).clamp(max=boxes.size(0) - 1)
        near = (torch.arange(n, device=dev) % 3 == 0) & (hi > lo)
        xyz[near, :2] = boxes[k[near], :2] + 0.05
        xyz[near, 2] = 40.0
        old[near, :] = -4.0
        old[near, labels[k[near]].clamp(min=0).long()] = 4.0
    if n and boxes_2d.size(0):  # some detections sit on projected boxes, so that the 2-D branch assigns
        j = torch.nonzero(keep.reshape(-1)).reshape(-1)[:n // 2]
        preds[:j.numel(), :4] = boxes_2d.reshape(-1, 4)[j]
        preds[:j.numel(), 6] = (j % 6).float()
    preds = wide(preds) if n else preds
    old = wide(old) if n else old
    radii = torch.tensor([1.0, 1.0, 0.5, 4.0, 2.0, 0.0, 0.5, 0.5, 0.5, 0.5], device=dev)
    exact = int(_lib.lib().fsf_frustum_assign_workspace_bytes(boxes.size(0), boxes_2d.size(0), 6, n))
    return (lambda: ops.frustum_assign(xyz, table[:, 0], preds, ptr, boxes_2d, keep, ptr, boxes, labels, 10, code, 0.1, 0.7, 0.3, old,
                                       radii)), exact


@pytest.mark.parametrize("name,kind", [(n, k) for n in sorted(CASES) for k, _ in CASES[n]])
def test_wrapper_under_guard_bands_and_poison(ops, device, name, kind):
    run, exact = dict(CASES[name])[kind](ops, device)

    def scratch_expected(g):
        assert g.workspace_sizes == [exact] and exact > 0, (g.workspace_sizes, exact)
        assert any(r["kind"] == "workspace" and r["site"] == name for r in g.records)

    plain = three_runs(run, scratch_expected)
    assert len(plain) == 6
    if kind == "ragged":
        counts = torch.bincount(plain[4].cpu().long(), minlength=4).tolist()
        print(f"K38 guard-band ragged case: none / 3-D / 2-D / distance {counts}")
        assert counts[3] >= 1
