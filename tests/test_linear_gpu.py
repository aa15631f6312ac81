"""GPU: the K22 Linear family (K22, K22f, K22s, K22h and the sliced entry; fullysparsefusion_amd/csrc/linear_norm_act.hip) on the crafted
layouts of tests/linear_cases.py — tests/test_linear_cases_cpu.py shows which decisions of the launch each case reaches and that a model
of it with any of twelve defects fails one of them.  No tensor-wide tolerance anywhere:

* the `ints` and `one_hot` families are compared bit for bit with the int64 / float64 referee;
* the LayerNorm cases row by row with float64, each row within max(2 x the fp32 host reference's own error on that row, 2e-6 of the
  row's largest value); the largest err / tolerance of a case is printed;
* K22s's maxima bit for bit with the maxima of the rows the same call returned; a `want_rows=False` call gives the same maxima; the
  columns of the wider buffer beside the slice and the rows of the ids no row carries still hold -inf.
Every case runs twice (bitwise determinism), and before every case that takes more than one row block per workgroup and every K22s
case the same shape runs once with other values, so that nothing stale in LDS, in the slots or in an output can stand in for a result.
Shapes the entry points refuse are checked as FsfHipError."""
import numpy as np
import pytest
import torch

import linear_cases as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(device):
    from fullysparsefusion_amd import hip_ops

    return hip_ops


def _dev(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _bits(t):
    return t.contiguous().view(torch.int32)


def call(ops, device, c, d):
    """The case's entry point on operands `d`, prepared: a function that launches it and returns the rows f32 [n, c] — for K22s
    (rows | None, the [m, 2 c + 4] buffer of -inf whose columns c .. 2 c took the maxima)."""
    xbuf = _dev(d["xbuf"], device)
    x = xbuf[:, :c.in_cols]
    w, bias, gamma, beta = (_dev(d[f], device) for f in ("w", "bias", "gamma", "beta"))
    kw = dict(bias=bias, norm=c.norm, gamma=gamma, beta=beta, eps=L.EPS, act=c.act)
    if c.entry == "sliced":
        planes = ops.linear_prepare_weight_sliced(w, c.nslice, c.slice_c)
        run = lambda: ops.linear_norm_act_sliced(x, c.k, c.x_slice_off, planes, c.nslice, c.slice_c, **kw)  # noqa: E731
    elif c.entry == "planes":
        assert ops.linear_planes_supported(c.k, c.c, c.slice_c)
        planes = ops.linear_prepare_weight_f16(w, c.slice_c)
        xp = ops.rows_to_planes(x)
        run = lambda: ops.linear_planes_norm_act(xp, planes, c.c, c.slice_c, **kw)  # noqa: E731
    else:
        planes = ops.linear_prepare_weight(w, fmt=c.fmt)
        assert ops.linear_weight_is_f16(planes) == (c.fmt == "f16x3") and ops.linear_norm_act_supported(x, c.c)
        if c.addend:
            kw.update(row_add=_dev(d["table"], device), row_add_index=_dev(d["index"], device))
        if c.entry != "segmax":
            run = lambda: ops.linear_norm_act(x, planes, c.c, **kw)  # noqa: E731
        else:
            ids, m = _dev(d["ids"], device), d["m"]

            def run(want_rows=True):
                wide = torch.full((m, 2 * c.c + 4), float("-inf"), device=device)
                rows = ops.linear_norm_act_segmax(x, planes, c.c, ids, wide[:, c.c:2 * c.c], want_rows=want_rows, **kw)
                return rows, wide
    return run


@pytest.mark.parametrize("name", L.NAMES)
def test_linear_family_equals_the_referee(ops, device, name):
    c = L.SPECS[name]
    if L.needs_stale_run(c):
        stale = call(ops, device, c, L.operands(c, key=7))()
        stale = stale[0] if c.entry == "segmax" else stale
        assert bool(torch.isfinite(stale).all())
    d = L.case(name)
    run = call(ops, device, c, d)
    got = run()
    wide = None
    if c.entry == "segmax":
        got, wide = got
    assert got.shape == (c.n, c.c)
    if c.family in L.EXACT_FAMILIES:
        if not torch.equal(_bits(got), _bits(_dev(d["want"], device))):
            L.check_exact(name, got.cpu().numpy(), d["want"])
    else:
        ratio = L.check_rows(name, got.cpu().numpy(), d["want"], d["tol"])
        print("err/tol %-60s %.3f" % (name, ratio))
    if c.entry != "segmax":
        assert torch.equal(_bits(got), _bits(run()))
        return
    ids, m = _dev(d["ids"], device), d["m"]
    seg = wide[:, c.c:2 * c.c]
    want = torch.full((m, c.c), float("-inf"), device=device).scatter_reduce(0, ids[:, None].expand(c.n, c.c), got, "amax", include_self=True)
    if not torch.equal(seg, want):
        bad = torch.nonzero((seg != want).any(1)).flatten()[:8].tolist()
        first = {s: int(torch.nonzero(ids == s)[0]) if bool((ids == s).any()) else None for s in bad}
        raise AssertionError("%s: maxima differ in segments %s (first rows %s)" % (name, bad, first))
    assert bool(torch.isinf(wide[:, :c.c]).all()) and bool(torch.isinf(wide[:, 2 * c.c:]).all())  # nothing written beside the slice
    unused = torch.ones(m, dtype=torch.bool, device=device)
    unused[ids] = False
    assert int(unused.sum()) == m - len(np.unique(d["ids"])) >= 2 and bool((seg[unused] == float("-inf")).all())  # the empty segments
    rows2, wide2 = run()
    assert torch.equal(_bits(got), _bits(rows2)) and torch.equal(_bits(wide), _bits(wide2))
    none, wide3 = run(want_rows=False)
    assert none is None and torch.equal(_bits(wide), _bits(wide3))


@pytest.mark.parametrize("what", L.REFUSALS)
def test_refused_shapes_raise(ops, device, what):
    n = 17
    x = torch.ones(n, 64, device=device)
    ids = torch.arange(n, device=device)

    def layer(c, k=64, fmt="bf16x6"):
        w = torch.ones(c, k, device=device)
        return ops.linear_prepare_weight(w, fmt=fmt), torch.ones(c, device=device), torch.zeros(c, device=device)

    def segmax(c, norm, act):
        planes, g, b = layer(c)
        seg_out = torch.full((n, c), float("-inf"), device=device)
        return lambda: ops.linear_norm_act_segmax(x, planes, c, ids, seg_out, norm=norm, gamma=g, beta=b, eps=L.EPS, act=act)  # noqa: E731

    if what == "k22f_c32":
        planes, g, b = layer(32, fmt="f16x3")
        fn = lambda: ops.linear_norm_act(x, planes, 32, norm="ln", gamma=g, beta=b, eps=L.EPS, act="gelu")  # noqa: E731
    elif what == "k22s_c32":
        fn = segmax(32, "ln", "gelu")
    elif what == "k22s_c132":
        fn = segmax(132, "ln", "gelu")
    elif what == "k22s_affine":
        fn = segmax(64, "affine", "gelu")
    elif what == "k22s_no_act":
        fn = segmax(64, "ln", "none")
    else:
        k, slice_c = (64, 64) if what == "k22h_slice64" else (40, 128)
        w = torch.ones(128, k, device=device)
        planes = ops.linear_prepare_weight_f16(w, slice_c)
        xp = ops.rows_to_planes(x[:, :k])
        assert not ops.linear_planes_supported(k, 128, slice_c)
        fn = lambda: ops.linear_planes_norm_act(xp, planes, 128, slice_c)  # noqa: E731
    with pytest.raises(ops.FsfHipError):
        fn()
