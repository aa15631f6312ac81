"""CPU: what the per-element budget tests of the matrix-core product kernels (tests/test_product_budget_gpu.py) stand on.

* Every documented operand format, emulated in numpy with float64 accumulation, and torch's fp32 product stay inside the budget B of
  tests/product_budget.py on every family; every planted defect (one scale per 16-row group, the lo plane dropped on the small rows, a
  2-way bf16 split) leaves it — and the shared scale passes the batch-maximum criterion tests/test_hip_ops.py applies, which is the gap
  the budget closes.
* Where the format's floor sets the budget: per format, exactly the scaled-down output channels of the f16 forms — more than the
  quarter of the output that was aimed for, which the test states.
* Layout witnesses of the sparse family, and the scale rules and caps the budgets assume against the kernel sources, so that a retuned
  kernel gets its budget re-derived."""
import os
import re

import numpy as np
import pytest

import product_budget as P
from conftest import ROOT

LINEAR = [(name, n) for name in P.LINEAR_CASES for n in P.LINEAR_N]
CONV = [(name, t) for name in P.CONV_CASES for t in P.CONV_TABLES[name]]
F16_KERNELS = ("K9c", "K9b-XP", "K22f", "K22f-grouped", "K22h")


def _case(family, name, arg):
    return P.linear_case(name, arg) if family == "linear" else P.conv_case(name, arg)


def _x_rule(family, name):
    return P.conv_x_rule(name) if family == "conv" else P.SCALE_RULES[P.LINEAR_CASES[name][0]][0]


ALL = [("linear", a, b) for a, b in LINEAR] + [("conv", a, b) for a, b in CONV]
ALL_F16 = [c for c in ALL if _case(*c)["kernel"] in F16_KERNELS]
ALL_BF16 = [c for c in ALL if _case(*c)["kernel"] not in F16_KERNELS]


@pytest.mark.parametrize("family,name,arg", ALL)
def test_documented_format_and_fp32_stay_inside_the_budget(family, name, arg):
    c = _case(family, name, arg)
    b = c["budget"]
    fmt = P.emulate_f16(c["prod"], _x_rule(family, name)) if c["kernel"] in F16_KERNELS else P.emulate_bf16(c["prod"], 3)
    for what, y in (("format", fmt), ("fp32", c["prod"].ref32())):
        ratio, at = b.worst(y)
        assert ratio <= 1.0, (what, ratio, at)
    # B = 0 only where the value is an exact zero: the all-zero row of a Linear without an addend
    zero = b.B == 0
    assert not b.want[zero].any()
    if family == "linear" and c["table"] is None:
        assert zero[P.ZERO_ROW].all() and int(zero.sum()) == zero.shape[1]
    else:
        assert not zero.any()


@pytest.mark.parametrize("family,name,arg", ALL_F16)
def test_shared_scale_and_dropped_lo_plane_leave_the_budget(family, name, arg):
    """One scale per 16-row group is more than 10 x over the budget — on elements the FORMAT's floor does not dominate — and passes the
    batch-maximum criterion of tests/test_hip_ops.py on the same data: the suite could not tell it from the correct kernel.  The lo plane
    dropped on the small rows is more than 10 x over as well (the batch criterion notices it only through the 2^12 rows' own error)."""
    c = _case(family, name, arg)
    b = c["budget"]
    tight = ~b.floor_dominated()
    for defect in ("group_scale", "drop_lo"):
        y = P.emulate_f16(c["prod"], _x_rule(family, name), defect)
        ratio, at = b.worst(y)
        assert ratio > 10.0, (defect, ratio, at)
        err = np.abs(y - b.want)
        assert (err[tight & (b.B > 0)] / b.B[tight & (b.B > 0)]).max() > 10.0, defect
    passes_today, rel = b.today(P.emulate_f16(c["prod"], _x_rule(family, name), "group_scale"))
    assert passes_today and rel < 2e-7, rel  # the record of the gap
    # the small rows alone: with the lo plane kept on the 1 and 2^12 rows the batch criterion is blind to the 2^-12 rows as well
    rows = c["prod"].x
    small = np.abs(rows).max(1) < 2.0 ** -6
    s = P.x_scales(rows, _x_rule(family, name))
    xh, xl = P.split_f16(rows, s)
    xl[small] = 0.0
    wh, wl = P.split_f16(c["prod"].w, P.pick_scale(np.abs(c["prod"].w).max()))
    y = c["prod"].rows(xh) @ wh + c["prod"].rows(xh) @ wl + c["prod"].rows(xl) @ wh
    if c["prod"].addend is not None:
        y = y + c["prod"].addend.astype(np.float64)
    assert b.worst(y)[0] > 10.0 and b.today(y)[0]


@pytest.mark.parametrize("family,name,arg", ALL_BF16)
def test_two_way_bf16_split_leaves_the_budget(family, name, arg):
    c = _case(family, name, arg)
    ratio, at = c["budget"].worst(P.emulate_bf16(c["prod"], 2))
    assert ratio > 1.0, (ratio, at)


@pytest.mark.parametrize("table", P.WGRAD_TABLES)
def test_weight_gradient_budget(table):
    """K10 (32 x 68 channels: the fp32 matrix pipe), fp32 operands: torch's fp32 product is inside the budget (m = 2 over its own worst ratio), a 2-way bf16 split of the operands is
    outside; offsets without a pair ask for exact zeros."""
    c = P.wgrad_case(table)
    b = c["budget"]
    assert c["kernel"] == b.kernel == "K10" and P.SCALE_RULES["K10"][:2] == ("fp32", "fp32")
    assert float((b.err32[b.A > 0] / b.B[b.A > 0]).max()) <= 1.0
    assert not b.err32[b.A == 0].any() and not b.want[b.A == 0].any()
    assert b.floor_share() == 0.0
    empty = [k for k in range(c["nbr"].shape[1]) if not (c["nbr"][:, k] >= 0).any()]
    assert bool(empty) == (table in ("subm", "strided", "inverse"))  # the two z layers are four cells apart: no pair straight up or down
    worst = 0.0
    for k, part in enumerate(c["parts"]):
        out_rows = np.nonzero(c["nbr"][:, k] >= 0)[0]
        in_rows = c["nbr"][out_rows, k].astype(np.int64)
        f2 = sum(P.split_bf16(c["feat"], 2))
        g2 = sum(P.split_bf16(c["gout"], 2))
        y = f2[in_rows].T @ g2[out_rows]
        bk = b.rel * part.A
        if (bk > 0).any():
            worst = max(worst, float((np.abs(y - part.want)[bk > 0] / bk[bk > 0]).max()))
    assert worst > 1.0
    if table == "dense-%d" % P.WGRAD_SPLIT_N:
        assert c["feat"].shape[0] == 8 * P.BW_RT + 1


@pytest.mark.parametrize("table,cin,cout,absolute", P.K10P_CASES)
def test_k10p_budget_holds_the_six_terms_and_no_five(table, cin, cout, absolute):
    """K10p (cin > 64 and cout > 64: the bf16 matrix cores) on 68 x 68 (one partial tile) and 132 x 68 (two `a` tiles), signed and with
    both operands made non-negative: the six-term arithmetic and torch's fp32 product stay inside the budget; with any ONE cross term
    other than hi * hi left out the result leaves it, on every case.  Measured here, max err / B over the 20 cases: six terms 0.06 ..
    0.50; without hi * lo, lo * hi or mid * mid 9.0 .. 74; without hi * mid or mid * hi 2 900 .. 11 700 — so a factor m up to 8 instead
    of 2 would still tell every five-term kernel from the six-term one."""
    c = P.wgrad_case(table, cin, cout, absolute)
    b = c["budget"]
    assert c["kernel"] == b.kernel == "K10p" and P.wgrad_plan(P.wgrad_pair_capacity(table), cin, cout, c["nbr"].shape[1])[:2] == (128, 128)
    assert (b.g, b.m) == (0.0, 2.0) and b.floor_share() == 0.0 and not b.floor.any()
    assert absolute == bool((c["feat"] >= 0).all() and (c["gout"] >= 0).all())
    ratio, at = b.worst(P.wgrad_emulate_bf16(c))
    assert ratio <= 1.0, (ratio, at)
    assert float((b.err32[b.A > 0] / b.B[b.A > 0]).max()) <= 1.0
    assert not b.err32[b.A == 0].any() and not b.want[b.A == 0].any()
    for drop in P.BF16_TERMS[1:]:
        ratio, at = b.worst(P.wgrad_emulate_bf16(c, drop))
        assert ratio > 1.0, (drop, ratio, at)


def test_floor_dominated_share_per_format_exceeds_a_quarter_for_the_f16_forms():
    """Where the format's floor, not the arithmetic, sets the budget: the share of elements with floor > (g + m 2^-23) A, per (family,
    format), never averaged over formats.

    The condition these families were meant to satisfy — at most 25 % — is NOT met by the f16 forms, and this test says so instead of
    asserting it: every f16 case (K9c, K9b-XP, K22f with and without the addend, K22h) has exactly its output channels ::5 and 1::7
    floor-dominated (the next test), 1/5 + 1/7 - 1/35 of any width: 31.2 % of 64 and of 256 channels, 32.4 % of 68, 33.3 % of 36.  The
    cause is in the inputs: the weight columns ::4 at 2^12 set the layer-wide weight scale s_w, which leaves the plain-column weights of
    the 2^-10 channels 15 bits above the weight floor 2^-25 / s_w; without those columns only the 2^-20 channels are floor-dominated
    (10 of 68 = 14.7 %).  The inputs are kept as specified — the 2^12 columns are what makes the small x columns carry as much of the
    result as the large ones.  What keeps the floor from swallowing the check: the share is a fixed set of channels, not of rows — every
    plain channel of every row, 2^-12 rows included, is held to the arithmetic bound, and the planted defects are > 10 x over there
    (test_shared_scale_and_dropped_lo_plane_leave_the_budget); and on the floor-dominated channels the budget is still per element and
    still 15 (2^-10 channels) or 5 (2^-20 channels) bits below the element's own size.
    The exact formats (bf16 x 3: K9b, K22, K10p; fp32 operands: K9, K10) have no floor: share 0."""
    for c in ALL:
        b = _case(*c)["budget"]
        width = b.A.shape[1]
        ch = np.arange(width)
        treated = int(((ch % 5 == 0) | (ch % 7 == 1)).sum())
        if b.g == 0.0:
            assert b.floor_share() == 0.0, c
        else:
            rows_with_budget = int((b.floor > 0).any(1).sum())
            assert int(b.floor_dominated().sum()) == treated * rows_with_budget, c
            assert rows_with_budget >= b.A.shape[0] - 1 and 0.31 < treated / width < 0.34 and b.floor_share() > 0.25, c
    assert all(P.wgrad_case(t)["budget"].floor_share() == 0.0 for t in P.WGRAD_TABLES)


@pytest.mark.parametrize("family,name,arg", ALL_F16)
def test_floor_dominated_elements_are_exactly_the_scaled_down_channels(family, name, arg):
    """Where the format's floor sets the budget: the output channels ::5 and 1::7 (weights 2^-10 / 2^-20 of a layer whose scale the 2^12
    columns set) of the rows that have a budget at all — and nowhere else: no plain channel, whatever the row's magnitude."""
    b = _case(family, name, arg)["budget"]
    dom = b.floor_dominated()
    ch = np.arange(dom.shape[1])
    treated = (ch % 5 == 0) | (ch % 7 == 1)
    assert not dom[:, ~treated].any()
    assert dom[:, treated][(b.floor > 0).any(1)].all()


# ---- layout witnesses ------------------------------------------------------------------------------------------------------------

def test_sparse_family_layout():
    idx, isl, cls = P.sparse_sites()
    m = idx.shape[0]
    assert m == 192 and (idx[:, 1:] < np.asarray(P.GRID)).all() and (idx >= 0).all()
    lin = (idx[:, 1].astype(np.int64) * P.GRID[1] + idx[:, 2]) * P.GRID[2] + idx[:, 3]
    assert (np.diff(lin) > 0).all()  # sorted by (z, y, x), no site twice
    nbr = P.conv_tables()["subm"][0]
    assert nbr.shape == (m, 27) and (nbr[:, 13] == np.arange(m)).all()
    # every island's outputs depend on that island's rows only (the patch on its own rows only)
    src = np.where(nbr >= 0, isl[np.clip(nbr, 0, None)], isl[:, None])
    assert (src == isl[:, None]).all()
    for i in range(int(isl.max()) + 1):
        assert (isl == i).sum() == 6 and len(set(cls[isl == i])) == 1
    assert (np.array([cls[isl == i][0] for i in range(int(isl.max()) + 1)]) == np.arange(int(isl.max()) + 1) % 3).all()
    # every 16-row group of the sorted order holds at least two magnitudes; about five islands
    groups = [slice(s, min(s + 16, m)) for s in range(0, m, 16)]
    assert all(len(set(cls[g])) >= 2 for g in groups)
    assert np.median([len(set(isl[g])) for g in groups if (isl[g] >= 0).all()]) >= 4
    # the dense patch: neighbours of all three magnitudes meet in one output row
    patch = np.nonzero(isl < 0)[0]
    assert len(patch) == 36
    met = [len(set(cls[n[n >= 0]])) for n in nbr[patch]]
    assert max(met) == 3 and np.mean(np.array(met) == 3) > 0.8
    # the strided tables: m_in != m_out, in both directions
    strided, inverse = P.conv_tables()["strided"], P.conv_tables()["inverse"]
    assert strided[0].shape[0] != m and strided[1] == m and inverse[0].shape[0] == m and inverse[1] == strided[0].shape[0]


def test_linear_family_layout_and_caps():
    for name, n in LINEAR:
        c = P.linear_case(name, n)
        x, w, cls = c["x"], c["w"], c["cls"]
        assert not x[P.ZERO_ROW].any() and all(len(set(cls[s:s + 16])) == 3 for s in range(0, n - 15, 16))
        amax = np.abs(x).max(1)
        for k in range(3):
            rows = (cls == k) & (amax > 0)
            assert (amax[rows] > P.MAGS[k]).all() and (amax[rows] < 8 * P.MAGS[k]).all()
        # the magnitudes stay below the documented caps: K22f with an addend keeps s_x * s_w <= 2^40
        s_w = float(P.pick_scale(np.abs(w).max()))
        s_x = P.x_scales(x, "row_running")[amax > 0]
        assert float(s_x.max()) * s_w <= 2.0 ** P.K22F_ADDEND_CAP_EXP
    for name, t in CONV:
        c = P.conv_case(name, t)
        amax = np.abs(c["feat"]).max(1)
        assert float(P.x_scales(c["feat"], "row")[amax > 0].max()) <= 2.0 ** P.K9BXP_UNIT_CAP_EXP


# ---- the kernels' constants ------------------------------------------------------------------------------------------------------

def _src(name):
    return open(os.path.join(ROOT, "fullysparsefusion_amd", "csrc", name)).read()


def test_scale_rules_and_caps_equal_the_kernel_sources():
    planes, split, lna_h, lna, bwd, fmt_h, fmt = (_src(n) for n in ("spconv_planes.hip", "spconv_split.hip", "linear_norm_act.h",
                                                                     "linear_norm_act.hip", "spconv_bwd.hip", "operand_formats.h",
                                                                     "operand_formats.hip"))
    csrc_dir = os.path.join(ROOT, "fullysparsefusion_amd", "csrc")
    others = {n: _src(n) for n in sorted(os.listdir(csrc_dir)) if n.endswith((".h", ".hip")) and n != "operand_formats.h"}
    # the one scale rule: s * amax in [2^13, 2^14), s = 1 for amax = 0, the exponent clamped at -113 (s <= 2^126) — defined once
    body = fmt_h[fmt_h.index("void fmt_pick_scale(float amax"):][:500]
    assert "e = amax > 0.0f ? (e < -113 ? -113 : e) : %d;" % P.TOP_EXP in body
    assert "s = __uint_as_float((unsigned)(%d - e + 127) << 23);" % P.TOP_EXP in body
    assert len(re.findall(r"void \w*pick_scale\(", fmt_h)) == 1
    # the split and its floor: hi = rn_f16(x s), lo = rn_f16(x s - hi) — defined once
    assert "|x s - hi - lo| <= max(2^-22 |x s|, 2^-25)" in planes and "|x s - hi - lo| <= max(2^-22 |x s|, 2^-25)" in fmt_h
    f16_body = fmt_h[fmt_h.index("void fmt_split_f16("):][:600]
    for line in ("const float xs = __fmul_rn(v[e], s);", "h[e] = (_Float16)xs;", "l[e] = (_Float16)__fsub_rn(xs, (float)h[e]);"):
        assert f16_body.count(line) == 1, line
    assert fmt_h.count("__fsub_rn(xs, (float)h[e])") == 1
    # no other file under csrc/ has a scale pick, a bf16 truncation split or an f16 split of its own
    for name, src in others.items():
        assert not re.search(r"void \w*pick_scale\(", src), name
        assert "& 0xffff0000u" not in src and "__fsub_rn(xs, (float)h[e])" not in src, name
        assert "%d - e + 127" % P.TOP_EXP not in src, name
    assert "(+ terms <= 3 * 2^-22 |x w|)" in planes and P.G_F16 == 3 * 2.0 ** -22
    # where the scales apply
    assert "const int nchunk = (c + %d) / %d;" % (P.PLANE_CHUNK - 1, P.PLANE_CHUNK) in planes        # fsf_to_planes: per (row, 128-channel chunk)
    # ... over its team of 16 threads, in to_planes and in the pair sum
    assert planes.count("for (int o = 8; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 16));\n    float s, inv;\n"
                        "    fmt_pick_scale(amax, s, inv);") == 2
    assert "The weights get\n//     one power-of-two scale per layer" in planes                                   # K9c weights
    assert "one power-of-two scale per layer (s * max |w| in [2^13, 2^14))" in split                              # K9b-XP weights
    assert "amax = fsf_wave_max(amax);\n    float s_row, inv_row;\n    fmt_pick_scale(amax, s_row, inv_row);" in lna  # rows_to_planes: per row
    # the f16 weights of every entry: ONE max |w| word for the layer (every workgroup's atomicMax lands in header word 2, one kernel,
    # one host helper that all three prepare entries call), one fmt_pick_scale of it in the entry's prepare kernel
    assert re.search(r"constexpr int FMT_HDR_AMAX_BITS = 2;", fmt_h) and re.search(r"constexpr int FMT_HDR_BYTES = 256;", fmt_h)
    assert "atomicMax(hdr + FMT_HDR_AMAX_BITS, __float_as_uint(fmaxf(fmaxf(wave_max[0], wave_max[1]), fmaxf(wave_max[2], wave_max[3]))));" in fmt
    assert sum(src.count("atomicMax(hdr + ") for src in others.values()) == 1
    for src, kernel in ((lna, "lna_prepare_f16_kernel("), (split, "scs_prepare_f16_kernel("), (planes, "sp_weight_planes_kernel(")):
        assert src.count("fsf_weight_layer_absmax(weight, ") == 1
        prep = src[src.index(kernel):][:2000]
        assert prep[:prep.index("\n}\n")].count("fmt_pick_scale(") == 1
        assert "fmt_pick_scale(__uint_as_float(reinterpret_cast<const unsigned*>(hdr)[FMT_HDR_AMAX_BITS]), s" in prep
    prep = lna[lna.index("lna_prepare_f16_kernel("):][:2000]
    assert prep.count("fmt_split_f16(v, s_w, hi, lo);") == 1
    assert int(re.search(r"constexpr int LNA_KC = (\d+);", lna_h).group(1)) == P.LNA_KC
    assert "if (mb == 0u || s_new > xs_cur[rg]) { s_new = xs_cur[rg]; inv_new = xinv[rg]; }" in lna_h              # K22f: the scale only falls
    # the caps
    assert "- 127 + %d;" % P.K22F_ADDEND_CAP_EXP in lna and "s * s_w stays <= 2^%d" % P.K22F_ADDEND_CAP_EXP in lna
    assert "sc_x[rg] = fmaxf(raw, 0x1p-%df);" % P.K9BXP_UNIT_CAP_EXP in split
    # K10: fp32 operands on the fp32 matrix pipe.  K10p: the exact 3-way bf16 split (truncation, the remainder formed in fp32) and the
    # six cross terms of P.BF16_TERMS on the bf16 matrix cores.  Neither has an f16 form.  Which shapes run which: both tiles 128 wide.
    k10, k10p = bwd[:bwd.index("// K10p (round 4)")], bwd[bwd.index("// K10p (round 4)"):]
    assert "v_mfma_f32_16x16x4_f32" in k10 and "__builtin_amdgcn_mfma_f32_16x16x4f32(" in k10 and "bf16" not in k10
    assert "v_mfma_f32_16x16x32_bf16" in k10p and k10p.count("__builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ta][TERM_A[term]], bf[TERM_B[term]]") == 1
    assert "f16" not in bwd.lower().replace("bf16", "")
    term_a, term_b = (tuple(int(v) for v in re.search(r"constexpr int TERM_%s\[6\] = \{([0-9, ]+)\};" % ab, k10p).group(1).split(","))
                      for ab in "AB")
    assert sorted(zip(term_a, term_b)) == sorted(P.BF16_TERMS)
    # (the split is the shared one: two truncations per value, the remainders formed in fp32)
    assert k10p.count("fmt_split_bf16(v, hi, mid, lo);") == 1
    bf16_body = fmt_h[fmt_h.index("void fmt_split_bf16("):][:1400]
    bf16_body = bf16_body[:bf16_body.index("\n}\n")]
    assert bf16_body.count("& 0xffff0000u") == 4 and fmt_h.count("& 0xffff0000u") == 4
    assert "const float ar = __fsub_rn(a, ah), br = __fsub_rn(b, bh);" in bf16_body and "const float al = __fsub_rn(ar, am), bl = __fsub_rn(br, bm);" in bf16_body
    assert bf16_body.count("__builtin_amdgcn_perm(") == 3 and bf16_body.count("0x07060302u") == 3
    assert "  if (cap > 0 && ta == 128 && tb == 128) {\n" in bwd and bwd.count("spconv_bwd_weight_split_kernel, grid, dim3(256), BWS_SMEM") == 1
    assert (P.wgrad_kernel(64, 68), P.wgrad_kernel(68, 64), P.wgrad_kernel(68, 68), P.wgrad_kernel(P.WGRAD_CIN, P.WGRAD_COUT)) == ("K10", "K10", "K10p", "K10")
    # the pair range splits from 8 stages + 1 pair
    assert int(re.search(r"constexpr int BW_RT = (\d+);", bwd).group(1)) == P.BW_RT
    for line in ("*ta = cin <= 64 ? 64 : 128;", "*tb = cout <= 64 ? 64 : 128;", "int64_t s = fsf_cdiv(kvol >= 8 ? 6144 : 512, kvol * tiles);",
                 "const int64_t max_s = fsf_cdiv(cap, 8 * BW_RT);", "int64_t r = fsf_align_up(fsf_cdiv(cap, s), BW_RT);",
                 "*nsplit = fsf_cdiv(cap > 0 ? cap : 1, r);"):
        assert line in bwd, line  # P.wgrad_plan mirrors these
    for line in ("*range = (int)r;", "if (r < BW_RT) r = BW_RT;", "if (s > max_s) s = max_s;", "if (s < 1) s = 1;",
                 "const int64_t tiles = (int64_t)fsf_cdiv(cin, *ta) * fsf_cdiv(cout, *tb);"):
        assert line in bwd, line
    assert "cap = max(m_out, 1)" in open(os.path.join(ROOT, "fullysparsefusion_amd", "hip_ops.py")).read()  # rulebook_to_pairs


def test_pick_scale_has_the_kernel_clamp():
    """s * amax in [2^13, 2^14) down to amax = 2^-113; below it s stays 2^126 (fmt_pick_scale clamps the exponent so that s and 1 / s are
    normal fp32 numbers), subnormal maxima included; s = 1 for amax = 0."""
    amax = np.array([0.0, 2.0 ** -149, 2.0 ** -126, 2.0 ** -120, 1.5 * 2.0 ** -114, 2.0 ** -113, 1.99 * 2.0 ** -113, 2.0 ** -112, 1.0, 2.0 ** 13,
                     1.5 * 2.0 ** 100, float(np.finfo(np.float32).max)])
    s = P.pick_scale(amax)
    assert s.tolist() == [1.0] + [2.0 ** 126] * 6 + [2.0 ** 125, 2.0 ** 13, 1.0, 2.0 ** -87, 2.0 ** -114]
    assert P.MIN_AMAX_EXP == -113 and "(e < %d ? %d : e)" % (P.MIN_AMAX_EXP, P.MIN_AMAX_EXP) in _src("operand_formats.h")
    s32 = s.astype(np.float32)
    tiny = float(np.finfo(np.float32).tiny)
    assert (s32 == s).all() and (s32 >= tiny).all() and ((1.0 / s).astype(np.float32) >= tiny).all()  # exact and normal, both ways
    above = amax >= 2.0 ** -113
    assert ((s * amax)[above] >= 2.0 ** 13).all() and ((s * amax)[above] < 2.0 ** 14).all()


def test_weight_gradient_cases_on_both_sides_of_the_range_split():
    """Which weight-gradient cases split an offset's pair range (nsplit > 1, partial sums folded by the second kernel): the same for
    the K10 shape and the two K10p shapes."""
    for cin, cout in ((P.WGRAD_CIN, P.WGRAD_COUT),) + P.K10P_SHAPES:
        assert {t: P.wgrad_nsplit(P.wgrad_pair_capacity(t), cin, cout, 1 if t.startswith("dense-") else 27) for t in P.WGRAD_TABLES} == {
            "subm": 1, "strided": 2, "inverse": 1, "dense-192": 1, "dense-257": 2}
    nsplit = {t: P.wgrad_nsplit(P.wgrad_pair_capacity(t), P.WGRAD_CIN, P.WGRAD_COUT, 1 if t.startswith("dense-") else 27) for t in P.WGRAD_TABLES}
    assert {t: P.wgrad_pair_capacity(t) for t in P.WGRAD_TABLES} == {"subm": 192, "strided": 276, "inverse": 192, "dense-192": 192, "dense-257": 257}
    assert nsplit == {"subm": 1, "strided": 2, "inverse": 1, "dense-192": 1, "dense-257": 2}
    assert P.wgrad_nsplit(P.WGRAD_SPLIT_N - 1, P.WGRAD_CIN, P.WGRAD_COUT, 1) == 1


def test_factors_over_fp32_equal_the_existing_tests():
    """m: what each kernel's test in tests/test_hip_ops.py grants over err32 (2 where it grants none)."""
    src = open(os.path.join(ROOT, "tests", "test_hip_ops.py")).read()

    def body(name):
        s = src[src.index("def %s(" % name):]
        return s[:s.index("\n\n\n")] if "\n\n\n" in s else s

    for test, factor, kernels in (("test_spconv_forward_split_vs_oracle_and_fp32_kernel", "2.0", ("K9b",)),
                                  ("test_linear_norm_act_split_bf16_is_fp32_accurate", "2.0", ("K22",)),
                                  ("test_linear_f16x3_in_kernel_split_vs_float64", "2.0", ("K22f",)),
                                  ("test_linear_norm_act_grouped_equals_linear_of_concat", "3.0", ("K22-grouped", "K22f-grouped")),
                                  ("test_spconv_forward_planes_vs_float64", "4.0", ("K9c",)),
                                  ("test_linear_planes_f16x3_vs_float64", "8.0", ("K22h",))):
        assert "max(%s * err32" % factor in body(test), test
        for k in kernels:
            assert P.SCALE_RULES[k][3] == float(factor)
    for test, k in (("test_spconv_forward_split_planes_f16x3_vs_float64", "K9b-XP"), ("test_spconv_forward_subm_vs_oracle", "K9"),
                    ("test_spconv_backward_weight_on_strided_and_inverse_tables_equals_float64", "K10p")):
        assert "err32" not in body(test) and P.SCALE_RULES[k][3] == 2.0
    assert P.SCALE_RULES["K10"][3] == 2.0  # (no test in tests/test_hip_ops.py grants the fp32-pipe weight gradient a factor either)
