"""GPU: the norm kernels (K12 fsf_norm_act / fsf_norm_act_backward, K23 fsf_column_stats / fsf_batch_norm_*) on the cases of
tests/norm_cases.py: every kernel choice at its narrowest, widest and a ragged width, every reason for the scalar fallback, output
slices of poisoned wider buffers, the second trip of every grid-stride loop, every step of the fold loops, every tail of the K23
unroll.  Every comparison is bit for bit (the `ints`, `balanced` and `exact` families) or per element against float64 with the budgets
derived in norm_cases.py; no tolerance is a tensor-wide constant.  Each call is repeated once and must give the same bits.  What the
cases reach, and that they would tell a subtly wrong kernel from a right one, is asserted on the CPU in tests/test_norm_cases_cpu.py."""
import numpy as np
import pytest
import torch

import norm_cases as C

pytestmark = pytest.mark.gpu

F32 = np.float32
FSF_ERR_UNSUPPORTED = -6


@pytest.fixture(scope="module")
def ops(device):
    from fullysparsefusion_amd import hip_ops

    return hip_ops


def _np(t):
    return t.cpu().numpy()


def place(arr, off, device):
    """`arr` on the device as a contiguous tensor that starts `off` floats after a 16-byte boundary."""
    if arr is None:
        return None
    flat = torch.empty(arr.size + 4, dtype=torch.float32, device=device)
    t = flat[off:off + arr.size].view(arr.shape)
    t.copy_(torch.from_numpy(arr))
    assert t.is_contiguous() and flat.data_ptr() % 16 == 0 and (arr.size == 0 or t.data_ptr() % 16 == (4 * off) % 16)
    return t


def _act(c):
    return None if c["act"] == "none" else c["act"]


# ---- K12 forward ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.FWD_NAMES)
def test_norm_act_forward(ops, device, name):
    c = C.case(name)
    n, ch = c["n"], c["c"]
    lay = C.LAYOUTS[c["layout"]]
    x = place(c["x"], lay.x_off, device)
    gamma, beta = place(c["gamma"], lay.gb_off, device), place(c["beta"], lay.gb_off, device)
    outs = []
    for _ in range(2):
        buf = torch.full((n, ch + lay.pad), float(C.POISON), dtype=torch.float32, device=device)
        out = buf[:, lay.out_off:lay.out_off + ch] if lay.pad else buf
        assert out.stride(0) == ch + lay.pad and out.data_ptr() % 16 == (4 * lay.out_off) % 16
        # the 16-byte form exactly where the case says so
        assert c["v4"] == (ch % 4 == 0 and out.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and
                           (gamma is None or (gamma.data_ptr() % 16 == 0 and beta.data_ptr() % 16 == 0)))
        got = ops.norm_act(x, gamma, beta, c["eps"], "affine" if c["form"] == "aff" else "ln", _act(c), inplace=False, out=out)
        assert got.data_ptr() == out.data_ptr()
        outs.append(buf)
    assert torch.equal(outs[0], outs[1]), f"{name}: two calls differ"
    assert torch.equal(x, torch.from_numpy(c["x"]).to(device))  # the input is not written
    got = _np(outs[0])
    outside = np.ones(ch + lay.pad, bool)
    outside[lay.out_off:lay.out_off + ch] = False
    assert (got[:, outside] == C.POISON).all(), f"{name}: columns outside the slice were written"
    C.check_fwd(c, np.ascontiguousarray(got[:, lay.out_off:lay.out_off + ch]))


def test_norm_act_in_place_equals_out_of_place(ops, device):
    for width in (68, 3):
        name = next(k for k in C.FWD_NAMES if C.FWD_SPECS[k][0] == width and C.FWD_SPECS[k][2] == "lna" and C.FWD_SPECS[k][1] > 1)
        c = C.case(name)
        x = place(c["x"], 0, device)
        g, b = place(c["gamma"], 0, device), place(c["beta"], 0, device)
        want = ops.norm_act(x, g, b, c["eps"], "ln", _act(c), inplace=False)
        assert ops.norm_act(x, g, b, c["eps"], "ln", _act(c)).data_ptr() == x.data_ptr() and torch.equal(x, want)


@pytest.mark.parametrize("c", C.FWD_UNSUPPORTED)
def test_norm_act_forward_unsupported_width(ops, device, c):
    from fullysparsefusion_amd._lib import FsfHipError

    x = torch.ones(3, c, device=device)
    out = torch.full((3, c), 7.0, device=device)
    with pytest.raises(FsfHipError) as e:
        ops.norm_act(x, None, None, 1e-3, "ln", None, inplace=False, out=out)
    assert e.value.status == FSF_ERR_UNSUPPORTED and bool((out == 7.0).all())


# ---- K12 backward --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.BWD_NAMES)
def test_norm_act_backward(ops, device, name):
    c = C.case(name)
    lay = C.LAYOUTS[c["layout"]]
    x, go = place(c["x"], lay.x_off, device), place(c["go"], lay.go_off, device)
    gamma, beta = place(c["gamma"], lay.gb_off, device), place(c["beta"], lay.gb_off, device)
    first = ops.norm_act_backward(x, go, gamma, beta, c["eps"], _act(c))
    again = ops.norm_act_backward(x, go, gamma, beta, c["eps"], _act(c))
    for a, b in zip(first, again):
        assert (a is None and b is None) or torch.equal(a, b), f"{name}: two calls differ"
    gx, dg, db = (None if t is None else _np(t) for t in first)
    C.check_bwd(c, gx, dg, db)


@pytest.mark.parametrize("c,layout", C.BWD_UNSUPPORTED)
def test_norm_act_backward_unsupported(ops, device, c, layout):
    """More than 1024 channels, and 513..1024 channels without the 16-byte form."""
    from fullysparsefusion_amd._lib import FsfHipError

    assert C.bwd_kernel(c, C.is_v4(c, layout, True)) is None
    lay = C.LAYOUTS[layout]
    x = place(np.ones((3, c), F32), lay.x_off, device)
    go = place(np.ones((3, c), F32), lay.go_off, device)
    g, b = place(np.ones(c, F32), lay.gb_off, device), place(np.zeros(c, F32), lay.gb_off, device)
    with pytest.raises(FsfHipError) as e:
        ops.norm_act_backward(x, go, g, b, 1e-3, "gelu")
    assert e.value.status == FSF_ERR_UNSUPPORTED


# ---- K23 -----------------------------------------------------------------------------------------------------------------------------

def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _eq(got, want, what):
    np.testing.assert_array_equal(_np(got), want, err_msg=what)


@pytest.mark.parametrize("name", C.BN_NAMES)
def test_column_sums_and_statistics(ops, device, name):
    c = C.bn_case(name)
    n, ch = c["n"], c["c"]
    x = _dev(c["x"], device)
    s = ops.column_sum(x)
    _eq(s, c["want_sum"], f"{name} column_sum")
    assert torch.equal(s, ops.column_sum(x))
    mean, var = ops.column_mean_var(x)
    _eq(mean, c["want_mean"], f"{name} mean of ints")
    m2, v2 = ops.column_mean_var(x)
    assert torch.equal(mean, m2) and torch.equal(var, v2)
    stats = ops.batch_norm_train_stats(x, None, None, C.BN_EPS, C.BN_MOMENTUM)
    _eq(stats[0], c["want_mean"], f"{name} train_stats mean of ints")
    if n == 1:  # one row: the deviation is exactly 0
        _eq(var, np.zeros(ch, F32), f"{name} var of one row")
        _eq(stats[1], np.full(ch, 1.0 / np.sqrt(np.float64(F32(C.BN_EPS))), np.float64).astype(F32), f"{name} invstd of one row")
        return
    xb, st = _dev(c["xb"], device), c["stats"]
    mean, var = ops.column_mean_var(xb)
    _eq(mean, np.zeros(ch, F32), f"{name} mean of balanced")
    _eq(var, c["want_var"], f"{name} var of balanced")
    assert all(torch.equal(a, b2) for a, b2 in zip((mean, var), ops.column_mean_var(xb))), f"{name}: two calls differ"
    w, b = _dev(st["weight"], device), _dev(st["bias"], device)
    for _ in range(2):
        rm, rv = _dev(st["running_mean"], device), _dev(st["running_var"], device)
        mean, invstd, scale, shift = ops.batch_norm_train_stats(xb, w, b, C.BN_EPS, C.BN_MOMENTUM, rm, rv)
        _eq(mean, np.zeros(ch, F32), f"{name} train_stats mean")
        _eq(invstd, st["invstd"], f"{name} invstd")
        _eq(scale, st["scale"], f"{name} scale")
        _eq(shift, st["shift"], f"{name} shift")
        _eq(rm, st["new_running_mean"], f"{name} running_mean")
        _eq(rv, st["new_running_var"], f"{name} running_var")
    mean, invstd, scale, shift = ops.batch_norm_train_stats(xb, None, None, C.BN_EPS, C.BN_MOMENTUM)
    _eq(invstd, st["invstd"], f"{name} invstd, no affine")
    _eq(scale, st["scale_plain"], f"{name} scale, no affine")
    _eq(shift, st["shift_plain"], f"{name} shift, no affine")


@pytest.mark.parametrize("name", C.BN_NAMES)
def test_batch_norm_act_forward_and_backward(ops, device, name):
    c = C.bn_case(name)
    b = c["bwd"]
    x, go, mean, invstd = (_dev(b[k], device) for k in ("x", "go", "mean", "invstd"))
    scale, shift = _dev(b["scale"], device), _dev(b["shift"], device)
    for relu in (False, True):
        y = b[("affine", relu)]["y"]
        want = np.maximum(y, F32(0)) if relu else y
        out = ops.batch_norm_act_forward(x, scale, shift, relu)
        _eq(out, want, f"{name} forward relu={relu}")
        assert torch.equal(out, ops.batch_norm_act_forward(x, scale, shift, relu))
        for key, sc, sh in (("affine", scale, shift), ("plain", None, None)):
            w = b[(key, relu)]
            gx, dg, db = ops.batch_norm_act_backward(x, go, mean, invstd, sc, sh, relu)
            _eq(db, w["db"], f"{name} grad_beta {key} relu={relu}")
            _eq(dg, w["dg"], f"{name} grad_gamma {key} relu={relu}")
            C.check_bn_grad_x(c, key, relu, _np(gx))
            for a, a2 in zip((gx, dg, db), ops.batch_norm_act_backward(x, go, mean, invstd, sc, sh, relu)):
                assert torch.equal(a, a2), f"{name}: two calls differ"


@pytest.mark.parametrize("ch,n,off", C.BN_NORMAL)
def test_column_statistics_of_normal_values(ops, device, ch, n, off):
    """Two passes: a common offset of 1000 does not cost the variance its digits."""
    r = C.bn_normal(ch, n, off)
    x = _dev(r["x"], device)
    C.check_columns(_np(ops.column_sum(x)), r["sum"], r["sum_bound"], "column_sum")
    mean, var = ops.column_mean_var(x)
    C.check_columns(_np(mean), r["mean"], r["mean_bound"], "mean")
    C.check_columns(_np(var), r["var"], r["var_bound"], "var")
    assert all(torch.equal(a, b) for a, b in zip((mean, var), ops.column_mean_var(x)))
    if off:  # the bound is ten times below one rounding of E[x^2] = 1e6: a one-pass form cannot meet it
        assert r["var_bound"].max() < 0.1 * C.U * 1000.0 ** 2
