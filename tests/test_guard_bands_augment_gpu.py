"""Guard bands and poison around the allocating C-ABI wrappers of hip_ops_augment.py (K40), in the manner of
tests/test_guard_bands_optim_gpu.py: each case calls the wrapper plain, under `guarded(0xFF)` and under `guarded(0x00)`; no guard byte of
an output or scratch buffer may change, the scratch request is exactly `fsf_train_augment_points_workspace_bytes`, and every result is
bit-identical across the three runs.  The point output is a capacity buffer: only its rows below `count` are defined and compared.
tests/test_train_augment_cpu.py fails when a wrapper of the module has no ragged / minimal / empty case here."""
import numpy as np
import pytest
import torch

from test_guard_bands_gpu import G, three_runs

pytestmark = pytest.mark.gpu

CASES = {}  # wrapper name -> [(kind, build)], build(ops, dev) -> (run, expected scratch bytes or None)
RANGE = [-50.0, -50.0, -5.0, 50.0, 50.0, 3.0]


def cases(name, **kinds):
    def deco(factory):
        for kind, kw in kinds.items():
            CASES.setdefault(name, []).append((kind, lambda ops, dev, _kw=kw: factory(ops, dev, **_kw)))
        return factory
    return deco


@pytest.fixture(scope="module")
def ops(device):
    from fullysparsefusion_amd import hip_ops_augment

    return hip_ops_augment


def descriptor(rot, scale, flip_h, flip_v, trans):
    from fullysparsefusion_amd.mmdet3d_plugin.datasets.train_augment import train_descriptor

    return train_descriptor(dict(pcd_rot_factor=rot, pcd_scale_factor=scale, pcd_horizontal_flip=flip_h, pcd_vertical_flip=flip_v,
                                 pcd_trans=np.asarray(trans)))


@cases("train_augment_points", ragged=dict(n=4099, cols=7, seed=77), ragged_in_order=dict(n=2049, cols=8, seed=-1), minimal=dict(n=1, cols=3, seed=5),
       empty=dict(n=0, cols=8, seed=5))
def _train_augment_points(ops, dev, n, cols, seed):
    from fullysparsefusion_amd import _lib

    gen = G(61)
    pts = torch.cat([(torch.rand(n, 3, generator=gen) * 2 - 1) * torch.tensor([60.0, 60.0, 6.0]), torch.rand(n, cols - 3, generator=gen)], 1).to(dev)
    if n == 1:
        pts[0, :3] = 1.0  # (the one row survives)
    desc = descriptor(0.3, 0.95, True, False, (0.5, -0.3, 0.2))
    exact = int(_lib.lib().fsf_train_augment_points_workspace_bytes(n))

    def run():
        out, count = ops.train_augment_points(pts, desc, RANGE, seed)
        k = int(count)
        assert out.shape == (n, cols) and 0 <= k <= n and (n < 100 or 0 < k < n) and (n != 1 or k == 1)
        return [out[:k].clone(), count]
    return run, exact


@cases("train_augment_boxes", ragged=dict(sizes=(0, 1, 300), dim=9), minimal=dict(sizes=(1,), dim=7), empty=dict(sizes=(0, 0), dim=9))
def _train_augment_boxes(ops, dev, sizes, dim):
    gen = G(62)
    g = sum(sizes)
    wide = torch.zeros(g, dim + 3)
    wide[:, :2] = (torch.rand(g, 2, generator=gen) * 2 - 1) * 58
    wide[:, 2:dim] = torch.randn(g, dim - 2, generator=gen) * 3
    wide = wide.to(dev)
    boxes = wide[:, :dim]  # a row-strided view
    no_aug = (torch.randn(g, dim, generator=gen) * 4).to(dev)
    labels = torch.randint(-1, 10, (g,), generator=gen).to(dev)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    descs = [descriptor(0.1 * k, 1.0 + 0.05 * k, k % 2 == 0, k % 3 == 0, (0.5 * k, -0.3, 0.2)) for k in range(len(sizes))]

    def run():
        return list(ops.train_augment_boxes(boxes, labels, no_aug, labels, offsets, descs, RANGE))
    return run, None


@pytest.mark.parametrize("name,kind", [(n, k) for n in sorted(CASES) for k, _ in CASES[n]])
def test_wrapper_under_guard_bands_and_poison(ops, device, name, kind):
    run, exact = dict(CASES[name])[kind](ops, device)

    def scratch_expected(g):
        if exact is None:
            assert g.workspace_sizes == [] and any(r["kind"] == "empty" and r["site"] == name for r in g.records)
        else:
            assert g.workspace_sizes == [exact] and exact > 0, (g.workspace_sizes, exact)
            assert any(r["kind"] == "workspace" and r["site"] == name for r in g.records)

    plain = three_runs(run, scratch_expected)
    if name == "train_augment_boxes":
        boxes, labels, na_boxes, na_labels = plain
        assert boxes.shape == na_boxes.shape and labels.shape == na_labels.shape == boxes.shape[:1]
        if kind == "ragged":
            dropped = int((labels < 0).sum())
            assert 0 < dropped < labels.numel() and torch.equal(labels < 0, na_labels < 0)
            assert bool(((boxes[:, 6] >= -np.pi - 1e-6) & (boxes[:, 6] < np.pi + 1e-6)).all())
    elif kind == "empty":
        assert int(plain[1]) == 0 and plain[0].shape == (0, 8)
