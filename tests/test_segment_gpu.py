"""GPU: the segmented reductions (fsf_segment_reduce, fsf_segment_reduce_short, fsf_segment_reduce_backward) and the segment plan
(fsf_segment_plan_from_inverse, fsf_unique_rows) on the cases of tests/segment_cases.py: segments placed at every chunk and span
edge, long folds of every shape, widths and views of both vector forms, values that tie, that are exactly summable and that are
infinite.  Every comparison is bit for bit or the per-element summation bound derived in segment_cases.py; no tolerance is a
tensor-wide constant.  What the cases reach, and that they would tell a subtly wrong kernel from a right one, is asserted on the CPU
in tests/test_segment_cases_cpu.py.  Segment ids outside [0, m) are the caller's contract and are never fed."""
import numpy as np
import pytest
import torch

import segment_cases as C

pytestmark = pytest.mark.gpu

MODES = ("sum", "mean", "max")
F32 = np.float32


@pytest.fixture(scope="module")
def ops(device):
    from fullysparsefusion_amd import hip_ops

    return hip_ops


class Built:
    """A case with its inputs on the device, built once and shared by the tests of that case."""

    def __init__(self, ops, device, name):
        self.c = c = C.case(name)
        self.inv = torch.from_numpy(c["inv"].copy()).to(device)
        self.plan = ops.segment_plan_from_inverse(self.inv, c["m"], return_counts=True)
        w = c["width"]
        self.buf = torch.from_numpy(C.feature_buffer(c)).to(device)
        self.feat = self.buf[:, w.off:w.off + w.c]  # the view of the width class
        rng = np.random.default_rng([6, c["n"], c["m"], w.c])
        self.go = C.INT_CHOICES[rng.integers(0, C.INT_CHOICES.size, (c["m"], w.c))]  # integer-valued, never 0


@pytest.fixture(scope="module", params=C.NAMES)
def built(request, ops, device):
    return Built(ops, device, request.param)


def _np(t):
    return t.cpu().numpy()


def _check_plan(plan, inv, m):
    order, offs, cnt = C.plan_of(inv, m)
    assert plan.order.dtype == torch.int32 and plan.seg_offsets.dtype == torch.int32 and plan.m == m
    np.testing.assert_array_equal(_np(plan.order), order)  # the stable argsort: ascending row index inside a segment
    np.testing.assert_array_equal(_np(plan.seg_offsets), offs)
    np.testing.assert_array_equal(_np(plan.cnt), cnt)


def test_plans(ops, built):
    c = built.c
    _check_plan(built.plan, c["inv"], c["m"])
    if c["n"] and (c["lengths"] > 0).all():  # no empty id: the unique of the ids is the same plan
        ids, uplan = ops.unique_rows(built.inv[:, None])
        np.testing.assert_array_equal(_np(ids)[:, 0], np.arange(c["m"]))
        np.testing.assert_array_equal(_np(uplan.inv), c["inv"])
        _check_plan(uplan, c["inv"], c["m"])
        for a, b in ((uplan.order, built.plan.order), (uplan.seg_offsets, built.plan.seg_offsets), (uplan.cnt, built.plan.cnt)):
            assert torch.equal(a, b)


@pytest.mark.parametrize("name", C.PLAN_NAMES)
def test_plan_from_inverse_at_sort_pass_and_tile_edges(ops, device, name):
    inv, m = C.plan_case(name)
    assert inv.min() >= max(0, m - 40) and inv.max() < m
    _check_plan(ops.segment_plan_from_inverse(torch.from_numpy(inv).to(device), m, return_counts=True), inv, m)


def _check_max(c, out, arg, cols=None, what=""):
    sel = slice(None) if cols is None else cols
    np.testing.assert_array_equal(out, c["want_max"][:, sel], err_msg=f"{c['name']} max {what}")
    if arg is not None:
        np.testing.assert_array_equal(arg, c["want_arg"][:, sel], err_msg=f"{c['name']} argmax {what}")


def test_segment_reduce(ops, built):
    c = built.c
    if c["n"] > 1:
        assert built.feat.data_ptr() % 16 == (4 * c["width"].off) % 16 and built.feat.stride(0) == c["width"].buf
    out, arg = ops.segment_reduce(built.feat, built.plan, "max", return_argmax=True)
    assert arg.dtype == torch.int64
    _check_max(c, _np(out), _np(arg))
    out2, arg2 = ops.segment_reduce(built.feat, built.plan, "max", return_argmax=True)
    assert torch.equal(out, out2) and torch.equal(arg, arg2)
    assert torch.equal(ops.segment_reduce(built.feat, built.plan, "max"), out)  # (the form that keeps no argmax)
    if c["family"] == "inf":
        return
    for mode in ("sum", "mean"):
        got = ops.segment_reduce(built.feat, built.plan, mode)
        C.check_sum(c, mode, _np(got))
        assert torch.equal(got, ops.segment_reduce(built.feat, built.plan, mode)), f"{c['name']} {mode}: two calls differ"


def _short_tensors(built, widths):
    """The list's tensors on the device (column selections of the case's features, in the view each width asks for) and the case
    columns each is made of."""
    c = built.c
    feats, cols = [], []
    for t, w in enumerate(widths):
        k = C.short_columns(c["width"].c, t, w.c)
        sel = built.feat[:, torch.from_numpy(k).to(built.feat.device)]
        if w.buf != w.c:
            buf = torch.full((c["n"], w.buf), float(C.POISON), dtype=torch.float32, device=sel.device)
            buf[:, w.off:w.off + w.c] = sel
            sel = buf[:, w.off:w.off + w.c]
        feats.append(sel)
        cols.append(k)
    return feats, cols


def test_segment_reduce_short(ops, built):
    """The four tensor lists of C.SHORT_LISTS, each in one launch per mode."""
    c = built.c
    chunked = {mode: ops.segment_reduce(built.feat, built.plan, mode) for mode in (MODES if c["family"] in C.EXACT_SUM_FAMILIES else ("max",))}
    for which, widths in C.SHORT_LISTS.items():
        assert C.short_list_is_float4(widths) == (which in ("float4", "eight"))
        feats, cols = _short_tensors(built, widths)
        for mode in MODES if c["family"] != "inf" else ("max",):
            outs = ops.segment_reduce_short(feats, built.plan, mode)
            assert len(outs) == len(widths)
            for t, (o, k) in enumerate(zip(outs, cols)):
                what = f"short list {which}[{t}]"
                assert o.shape == (c["m"], widths[t].c)
                if mode == "max":
                    _check_max(c, _np(o), None, k, what)
                else:
                    C.check_sum(c, mode, _np(o), k, what)
                if mode in chunked:  # short and chunked agree bit for bit on max and on the exactly summable families
                    assert torch.equal(o, chunked[mode][:, torch.from_numpy(k).to(o.device)]), f"{c['name']} {mode} {what}"


def test_segment_reduce_short_argmax(ops, built):
    """A single tensor, in the case's own width and view, with its argmax."""
    c = built.c
    (out,), arg = ops.segment_reduce_short([built.feat], built.plan, "max", return_argmax=True)
    _check_max(c, _np(out), _np(arg), None, "short, single tensor")
    if c["family"] != "inf":
        for mode in ("sum", "mean"):
            C.check_sum(c, mode, _np(ops.segment_reduce_short([built.feat], built.plan, mode)[0]), None, "short, single tensor")


def _want_backward(c, go, mode):
    n, ch = c["n"], c["width"].c
    if mode == "sum":
        return go[c["inv"]]
    if mode == "mean":
        return go[c["inv"]] / np.maximum(c["cnt"], 1).astype(F32)[c["inv"], None]
    want = np.zeros((n, ch), F32)
    seg, col = np.nonzero(np.broadcast_to(c["lengths"][:, None] > 0, (c["m"], ch)))
    want[c["want_arg"][seg, col], col] = go[seg, col]  # the gradient goes to the REFEREE's argmax, and nowhere else
    return want


def test_segment_reduce_backward(ops, built):
    c = built.c
    go = torch.from_numpy(built.go).to(built.inv.device)
    for mode in ("sum", "mean"):
        g = ops.segment_reduce_backward(go, built.plan, mode)
        np.testing.assert_array_equal(_np(g), _want_backward(c, built.go, mode), err_msg=f"{c['name']} backward {mode}")
    _, arg = ops.segment_reduce(built.feat, built.plan, "max", return_argmax=True)  # the device's own argmax, ties and all
    g = _np(ops.segment_reduce_backward(go, built.plan, "max", argmax=arg))
    np.testing.assert_array_equal(g, _want_backward(c, built.go, "max"), err_msg=f"{c['name']} backward max")
    # every (segment, channel) gradient appears exactly once in its column (grad_out holds no zero)
    np.testing.assert_array_equal((g != 0).sum(0), np.full(c["width"].c, int((c["lengths"] > 0).sum())))


@pytest.mark.parametrize("short", [False, True])
def test_autograd_functions_on_a_frame(ops, device, short):
    """_SegmentReduce and _GatherRows of ops/sst_ops.py on the mixed frame with post-ReLU values: the forward is the hip_ops call, the
    backward the composition above; the adjoint of the row gather is the exact integer segment sum."""
    from fullysparsefusion_amd.mmdet3d_plugin.ops.sst_ops import _GatherRows, _SegmentReduce

    b = Built(ops, device, C.AUTOGRAD_CASE)
    c = b.c
    go = torch.from_numpy(b.go).to(device)
    for mode in MODES:
        f = b.feat.detach().clone().requires_grad_(True)
        out = _SegmentReduce.apply(f, b.plan, mode, short)
        direct = ops.segment_reduce_short([f.detach()], b.plan, mode)[0] if short else ops.segment_reduce(f.detach(), b.plan, mode)
        assert torch.equal(out, direct)
        if mode == "max":
            _check_max(c, _np(out.detach()), None)
        else:
            C.check_sum(c, mode, _np(out.detach()))
        out.backward(go)
        np.testing.assert_array_equal(_np(f.grad), _want_backward(c, b.go, mode), err_msg=f"autograd {mode}")
    src = go.clone().requires_grad_(True)
    rows = _GatherRows.apply(src, b.plan)
    np.testing.assert_array_equal(_np(rows.detach()), b.go[c["inv"]])
    rows.backward(b.feat.detach().clone())  # integer-valued: the adjoint is the case's exact segment sum
    np.testing.assert_array_equal(_np(src.grad), c["want_sum"])
