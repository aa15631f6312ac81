"""Guard bands and poison around the allocating C-ABI wrapper of hip_ops_project.py (K13c), in the manner of
tests/test_guard_bands_augment_gpu.py: each case calls the wrapper plain, under `guarded(0xFF)` and under `guarded(0x00)`; no guard byte of
the output or the scratch buffer may change, the scratch request is exactly `fsf_project_gather_bilinear_backward_workspace_bytes`, and
every result is bit-identical across the three runs.  tests/test_bilinear_backward_cpu.py fails when a wrapper of the module has no
ragged / minimal / empty case here."""
import pytest
import torch

from test_guard_bands_gpu import G, camera_inputs, randn, three_runs

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
    from fullysparsefusion_amd import hip_ops_project

    return hip_ops_project


@cases("project_gather_bilinear_backward", ragged=dict(n=1009, ncam=3, c=131, hf=29, wf=53), minimal=dict(n=1, ncam=1, c=1, hf=1, wf=1),
       empty=dict(n=0, ncam=2, c=3, hf=2, wf=2))
def _project_gather_bilinear_backward(ops, dev, n, ncam, c, hf, wf):
    from fullysparsefusion_amd import _lib

    pts, L, _, _ = camera_inputs(dev, n, ncam, 1, 450, 800, 31)
    g = G(33)
    u, u_red = randn(dev, g, n, ncam, c), randn(dev, g, n, c)
    exact = int(_lib.lib().fsf_project_gather_bilinear_backward_workspace_bytes(n, ncam, hf, wf, c))

    def run():
        return [ops.project_gather_bilinear_backward(pts, L, u, (hf, wf), (450, 800)),
                ops.project_gather_bilinear_backward(pts, L, u_red, (hf, wf), (450, 800), channels_last=True, reduce_cams=True)]
    return run, exact


@pytest.mark.parametrize("name,kind", [(n, k) for n in sorted(CASES) for k, _ in CASES[n]])
def test_wrapper_under_guard_bands_and_poison(ops, device, name, kind):
    run, exact = dict(CASES[name])[kind](ops, device)

    def scratch_expected(g):
        assert g.workspace_sizes == [exact, exact] and exact > 0, (g.workspace_sizes, exact)
        assert sum(r["kind"] == "workspace" and r["site"] == name for r in g.records) == 2
        assert sum(r["kind"] == "empty" and r["site"] == name for r in g.records) == 2

    nchw, cl = three_runs(run, scratch_expected)
    assert nchw.dim() == 4 and cl.shape == (nchw.size(0), nchw.size(2), nchw.size(3), nchw.size(1))
    if kind == "ragged":
        assert bool(nchw.any()) and bool(cl.any()) and bool((nchw == 0).all(1).any())  # taps landed, and not on every texel
    if kind == "empty":
        assert not nchw.any() and not cl.any()
