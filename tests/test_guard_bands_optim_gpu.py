"""Guard bands and poison around the allocating C-ABI wrappers of hip_ops_optim.py (K39), in the manner of
tests/test_guard_bands_frustum_gpu.py: each case calls the wrapper plain, under `guarded(0xFF)` and under `guarded(0x00)`; no guard byte
of an output or scratch buffer may change, the scratch request is exactly `fsf_optim_workspace_bytes`, and every result is
bit-identical across the three runs.  The step works in place: every run starts from equal copies of the parameters, gradients and
moments, and what it left in them is the result.  tests/test_optim_cpu.py fails when a wrapper of the module has no ragged / minimal /
empty case here."""
import pytest
import torch

from test_guard_bands_gpu import G, three_runs

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
    from fullysparsefusion_amd import hip_ops_optim

    return hip_ops_optim


def _entries(sizes, lead, g, m, v, params):
    """(addresses, count, group) per parameter: gradient and moments `lead` floats into their flat buffers, then back to back."""
    out, off = [], lead
    for i, (n, p) in enumerate(zip(sizes, params)):
        out.append((p.data_ptr(), g.data_ptr() + 4 * off, m.data_ptr() + 4 * off, v.data_ptr() + 4 * off, n, i % 3))
        off += n
    return out


@cases("chunk_table", ragged=dict(sizes=(1, 3, 4097, 8197, 128)), minimal=dict(sizes=(1,)), empty=dict(sizes=()))
def _chunk_table(ops, dev, sizes):
    from fullysparsefusion_amd.optim import chunk_rows

    rows = chunk_rows([(1 << 20, 2 << 20, 3 << 20, 4 << 20, n, i % 3) for i, n in enumerate(sizes)], ops.CHUNK)  # (never dereferenced)
    assert rows.size(0) == sum(-(-n // ops.CHUNK) for n in sizes)
    return (lambda: ops.chunk_table(rows, dev)), None


@cases("adamw_step", ragged=dict(sizes=(1, 3, 4097, 8197, 128, 4095), lead=1), minimal=dict(sizes=(1,), lead=0), empty=dict(sizes=(), lead=0))
def _adamw_step(ops, dev, sizes, lead):
    from fullysparsefusion_amd import _lib
    from fullysparsefusion_amd.optim import chunk_rows

    gen = G(47)
    total = lead + sum(sizes)
    start = dict(g=torch.randn(total + 3, generator=gen).to(dev) * 3, m=torch.randn(total + 3, generator=gen).to(dev) * 0.1,
                 v=torch.rand(total + 3, generator=gen).to(dev) * 0.01, p=[torch.randn(n, generator=gen).to(dev) for n in sizes])
    g, m, v = (torch.zeros(total + 3, device=dev) for _ in range(3))
    params = [torch.zeros(n, device=dev) for n in sizes]
    table = ops.chunk_table(chunk_rows(_entries(sizes, lead, g, m, v, params), ops.CHUNK), dev)
    exact = int(_lib.lib().fsf_optim_workspace_bytes(table.size(0)))

    def run():
        g.copy_(start["g"]), m.copy_(start["m"]), v.copy_(start["v"])
        for p, s in zip(params, start["p"]):
            p.copy_(s)
        norm = torch.full((1,), -1.0, device=dev)
        ops.adamw_step(table, [0.999, 1.0, 0.9995], [1e-2, 2e-3, 1e-2], 0.1, 0.999, 0.001, 0.0316, 1e-8, 35.0, True, norm)
        return [p.clone() for p in params] + [g.clone(), m.clone(), v.clone(), norm]
    return run, exact


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
    if name == "adamw_step":
        *params, g, m, v, norm = plain
        if kind == "empty":
            assert float(norm) == -1.0  # nothing launched
        else:
            total = sum(p.numel() for p in params)
            lead = 1 if kind == "ragged" else 0
            assert float(norm) > (35.0 if kind == "ragged" else 0.0)  # (ragged: clipping was active)
            assert float(g[lead:lead + total].abs().max()) == 0.0 and float(g[lead + total:].abs().min()) > 0.0  # cleared, and only there
            assert lead == 0 or float(g[0]) != 0.0
            assert float(v[lead:lead + total].min()) >= 0.0 and bool(torch.isfinite(torch.cat(params)).all())
