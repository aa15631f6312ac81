"""GPU: every kernel that reproduces an fp32 product on the matrix cores, held to the per-ELEMENT budget of tests/product_budget.py on
inputs whose rows, input columns and output channels differ by 2^12 .. 2^30 in magnitude (tests/test_product_budget_cpu.py shows that
the documented formats meet the budget and that a scale shared by 16 rows, a dropped lo plane or a 2-way bf16 split do not — while
the batch-maximum criterion of tests/test_hip_ops.py passes the first).  Each case: the bare product, the product with the fused
epilogue, bitwise determinism.  The LayerNorm epilogues stay with their own tests (LayerNorm judges each row at its own scale)."""
import numpy as np
import pytest
import torch

import product_budget as P

pytestmark = pytest.mark.gpu

LINEAR = [(name, n) for name in P.LINEAR_CASES for n in P.LINEAR_N]
CONV = [(name, t) for name in P.CONV_CASES for t in P.CONV_TABLES[name]]


@pytest.fixture(scope="module")
def ops(device):
    from fullysparsefusion_amd import hip_ops

    return hip_ops


def _hold(label, b, got, classes, want=None, B=None):
    """Assert |got - want| <= B on every element; the message names the worst element, its ratio and the magnitude classes behind it."""
    got = got.detach().cpu().numpy().astype(np.float64).reshape(b.want.shape)
    assert np.isfinite(got).all(), label
    ratio, at = b.worst(got, want, B)
    print("BUDGET %-28s rho32 %.3g  max err/B %.3f at %s (%s)" % (label, b.rho32, ratio, at, classes(at)))
    assert ratio <= 1.0, "%s: err / B = %.3g at (row, channel) = %s, magnitude class %s" % (label, ratio, at, classes(at))


def _channel_vectors(rng, c, dev):
    """(scale, shift) f32 [c]: scale of either sign, shift at the channel's own level of the small rows."""
    scale = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32)
    shift = rng.standard_normal(c) * 2.0 ** -12
    P._channel_treatment(shift)
    shift = shift.astype(np.float32)
    return scale, shift, torch.from_numpy(scale).to(dev), torch.from_numpy(shift).to(dev)


def _decode_planes(pl):
    m, c = pl.m, pl.c
    raw = pl.data.cpu().numpy()[: (m + 1) * c * 4].view(np.float16).reshape(m + 1, c // 8, 2, 8).astype(np.float64)
    inv = pl.scales.cpu().numpy().astype(np.float64)
    return (raw[:, :, 0, :] + raw[:, :, 1, :]).reshape(m + 1, c) * inv[:, np.minimum(np.arange(c) // 128, inv.shape[1] - 1)]


def _device_table(ops, device, table):
    """The neighbour table from the device rulebook — equal to the host one the budget was made from."""
    idx = torch.from_numpy(P.sparse_sites()[0]).to(device)
    if table == "subm":
        nbr = ops.rulebook_subm(idx, 1, P.GRID)
    else:
        _, fwd, inv, _ = ops.rulebook_strided(idx, 1, P.GRID, (3, 3, 3), (2, 2, 2), (1, 1, 1))
        nbr = fwd if table == "strided" else inv
    assert np.array_equal(nbr.cpu().numpy(), P.conv_tables()[table][0])
    return nbr.contiguous()


@pytest.mark.parametrize("name,table", CONV)
def test_sparse_conv_forward_within_budget(ops, device, name, table):
    c = P.conv_case(name, table)
    b, kernel, cins, cout = c["budget"], c["kernel"], c["cins"], c["cout"]
    nbr = _device_table(ops, device, table)
    f, w = torch.from_numpy(c["feat"]).to(device), torch.from_numpy(c["w"]).to(device)
    if kernel == "K9":
        wt = ops.spconv_transpose_weight(w)
        run = lambda **e: ops.spconv_forward(f, wt, nbr, **e)
    elif kernel == "K9b":
        pl = ops.spconv_prepare_weight_split(w)
        run = lambda **e: ops.spconv_forward_split(f, pl, 27, cout, nbr, **e)
    elif kernel == "K9c":
        assert ops.spconv_planes_supported(cins, cout, 27)
        pl = ops.spconv_prepare_weight_planes(w)
        srcs = [ops.to_planes(f[:, o:o + ci]) for o, ci in zip(np.cumsum((0,) + cins[:-1]), cins)]
        run = lambda **e: ops.spconv_forward_planes(srcs, pl, 27, cout, nbr, **e)[0]
    else:
        assert ops.spconv_split_planes_supported(sum(cins), cout)
        pl = ops.spconv_prepare_weight_split_f16(w)
        xp = ops.rows_to_planes(f)
        run = lambda **e: ops.spconv_forward_split_planes(xp, pl, 27, cout, nbr, **e)
    host_nbr, cls = c["nbr"], c["cls"]
    classes = lambda at: "neighbour rows at " + "/".join(sorted({P.class_name(cls[i]) for i in host_nbr[at[0]] if i >= 0}))
    out = run()
    _hold("%s-%s" % (name, table), b, out, classes)
    assert torch.equal(out, run())
    if kernel == "K9c":  # the plane-form output: the 22-bit split of the fp32 output, per element
        out_p, opl = ops.spconv_forward_planes(srcs, pl, 27, cout, nbr, want_planes=True)
        assert torch.equal(out_p, out)
        o64, dec = out.cpu().numpy().astype(np.float64), _decode_planes(opl)
        assert opl.scales.shape == (o64.shape[0] + 1, (cout + 127) // 128)
        for s0 in range(0, cout, 128):  # one scale per (row, 128-channel chunk): the absolute part is relative to the CHUNK's maximum
            o = o64[:, s0:s0 + 128]
            bound = np.maximum(np.abs(o) * 2.0 ** -21.9, np.abs(o).max(1, keepdims=True) * 2.0 ** -37.9)
            assert (np.abs(dec[:-1, s0:s0 + 128] - o) <= bound).all()
        assert not dec[-1].any()
    rng = np.random.default_rng(len(name) + len(table))
    scale, shift, scale_d, shift_d = _channel_vectors(rng, cout, device)
    res = (rng.standard_normal(b.want.shape) * np.abs(b.want)).astype(np.float32)
    want2, B2 = b.with_epilogue(scale.astype(np.float64), shift.astype(np.float64), res.astype(np.float64))
    e = dict(scale=scale_d, shift=shift_d, residual=torch.from_numpy(res).to(device))
    out2 = run(**e)
    _hold("%s-%s+epilogue" % (name, table), b, out2, classes, want2, B2)
    assert torch.equal(out2, run(**e))


@pytest.mark.parametrize("name,n", LINEAR)
def test_linear_within_budget(ops, device, name, n):
    c = P.linear_case(name, n)
    b, kernel, width, slice_c = c["budget"], c["kernel"], c["c"], c["slice_c"]
    x, w = torch.from_numpy(c["x"]).to(device), torch.from_numpy(c["w"]).to(device)
    add = {}
    if c["table"] is not None:
        add = dict(row_add=torch.from_numpy(c["table"]).to(device), row_add_index=torch.from_numpy(c["index"]).to(device))
    if kernel == "K22h":
        assert ops.linear_planes_supported(P.K, width, slice_c) and ops.rows_to_planes_supported(x)
        wp, xp = ops.linear_prepare_weight_f16(w, slice_c), ops.rows_to_planes(x)
        run = lambda **e: ops.linear_planes_norm_act(xp, wp, width, slice_c, **e)
    else:
        fmt = "f16x3" if kernel.startswith("K22f") else "bf16x6"
        assert ops.linear_norm_act_supported(x, width)
        pl = ops.linear_prepare_weight(w, fmt=fmt)
        assert ops.linear_weight_is_f16(pl) == (fmt == "f16x3")
        run = lambda **e: ops.linear_norm_act(x, pl, width, **add, **e)
    cls = c["cls"]
    classes = lambda at: "row at " + ("0" if at[0] == P.ZERO_ROW else P.class_name(cls[at[0]]))
    out = run()
    _hold("%s-n%d" % (name, n), b, out, classes)
    assert torch.equal(out, run())
    # bias + the affine epilogue: (y + bias) * gamma + beta
    rng = np.random.default_rng(n + width)
    gamma, beta, gamma_d, beta_d = _channel_vectors(rng, width, device)
    _, bias, _, bias_d = _channel_vectors(rng, width, device)
    g64, be64, bi64 = gamma.astype(np.float64), beta.astype(np.float64), bias.astype(np.float64)
    want2 = (b.want + bi64) * g64 + be64
    B2 = np.abs(g64) * (b.B + P.U32 * (np.abs(b.want) + np.abs(bi64))) + P.U32 * (np.abs(g64 * (b.want + bi64)) + np.abs(be64))
    e = dict(bias=bias_d, norm="affine", gamma=gamma_d, beta=beta_d)
    out2 = run(**e)
    _hold("%s-n%d+affine" % (name, n), b, out2, classes, want2, B2)
    assert torch.equal(out2, run(**e))


def _weight_gradient(ops, device, c, table):
    """The case's weight gradient, twice (the second for the determinism check): through spconv_backward_weight on the device rulebook's
    pair lists, or through linear_backward_weight ('dense-<n>')."""
    feat, gout = torch.from_numpy(c["feat"]).to(device), torch.from_numpy(c["gout"]).to(device)
    if table.startswith("dense-"):
        run = lambda: ops.linear_backward_weight(feat, gout)
    else:
        pairs, num = ops.rulebook_to_pairs(_device_table(ops, device, table))
        assert num.cpu().tolist() == [int((c["nbr"][:, k] >= 0).sum()) for k in range(27)]
        assert pairs.shape == (27, 2, P.wgrad_pair_capacity(table))
        run = lambda: ops.spconv_backward_weight(feat, gout, pairs, num)
    cin = c["cin"]
    classes = lambda at: "offset %d, input column %s, grad-out column %s" % (
        at[0] // cin, "2^-12" if at[0] % cin % 4 == 0 else "1", "2^-12" if at[1] % 5 == 0 else "1")
    return run(), run(), classes


@pytest.mark.parametrize("table", P.WGRAD_TABLES)
def test_weight_gradient_within_budget(ops, device, table):
    """K10 (32 x 68 channels: the 64 x 128 tile of the fp32 matrix pipe) through spconv_backward_weight (the three tables) and through
    linear_backward_weight (192 and 257 rows).  The pair range of an offset is split in two (partial sums folded by a second kernel) on
    the strided table, whose pair lists have room for 276 pairs, and on the 257 rows; tests/test_product_budget_cpu.py derives that from
    the launch plan, the capacity is asserted here."""
    c = P.wgrad_case(table)
    assert c["kernel"] == "K10"
    got, again, classes = _weight_gradient(ops, device, c, table)
    _hold("K10-%s" % table, c["budget"], got, classes)
    assert torch.equal(got, again)


@pytest.mark.parametrize("table,cin,cout,absolute", P.K10P_CASES)
def test_k10p_weight_gradient_within_budget(ops, device, table, cin, cout, absolute):
    """K10p (both channel counts above 64: the six-term bf16 kernel) on 68 x 68 and 132 x 68 channels, the same five pair layouts, signed
    and with both operands non-negative (every piece of the truncating split is then non-negative: a dropped term cannot cancel).
    tests/test_product_budget_cpu.py: the six terms stay below 0.5 of this budget, any five are 9 or more times over it."""
    c = P.wgrad_case(table, cin, cout, absolute)
    assert c["kernel"] == "K10p"
    got, again, classes = _weight_gradient(ops, device, c, table)
    _hold("K10p-%s-%dx%d%s" % (table, cin, cout, "-abs" if absolute else ""), c["budget"], got, classes)
    assert torch.equal(got, again)
