"""CPU: what the norm-kernel tests on the device (tests/test_norm_gpu.py) stand on.

* The constants and dispatch rules restated in tests/norm_cases.py against the text of csrc/norm_act.hip and csrc/batch_norm.hip, so
  that a retuned cap or team size fails here and does not silently un-reach a case.
* Reachability: every kernel template instantiation of the two files and every branch the cases are there for has a named case.
* The referees against a plain Python loop on the small cases, and the exact-integer arguments of the `ints` / `balanced` / `exact`
  families.
* The budget constants of the `normal` family from torch's own fp32 composition on the host.
* Decisiveness without a GPU: a numpy model of the K12 row pass + column-sum fold and one of the K23 rows -> partial -> fold scheme,
  each walking rows in the kernels' visiting order, equal the referee on every case, and with each of ten plausible defects switched
  on differ on a case named here."""
import math
import os
import re

import numpy as np
import pytest
import torch

import norm_cases as C
from conftest import ROOT

F32, F64 = np.float32, np.float64
CSRC = os.path.join(ROOT, "fullysparsefusion_amd", "csrc")


# ---- source pin ------------------------------------------------------------------------------------------------------------------------

def _flat(fname):
    """The file without its line comments, white space collapsed."""
    return re.sub(r"\s+", " ", re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, fname)).read()))


def test_constants_and_rules_equal_the_kernel_source():
    na = _flat("norm_act.hip")
    assert f"constexpr int NA_MAX_PER_LANE = {C.NA_MAX_PER_LANE};" in na and f"constexpr int NA_BWD_BLOCKS = {C.NA_BWD_BLOCKS};" in na
    assert f"if (g > {C.FWD_CAP_SCALAR}) g = {C.FWD_CAP_SCALAR};" in na and f"if (g > {C.FWD_CAP_V4}) g = {C.FWD_CAP_V4};" in na
    assert na.count("if (g > NA_BWD_BLOCKS) g = NA_BWD_BLOCKS;") == 2
    assert "if (c > 64 * 16) return FSF_ERR_UNSUPPORTED;" in na and C.NA_MAX_C == 64 * 16
    assert "if (c > 64 * 16 || (c > 64 * NA_MAX_PER_LANE && !v4_ok)) return FSF_ERR_UNSUPPORTED;" in na
    # the 16-byte conditions of both entry points
    assert ("(c % 4) == 0 && (out_stride % 4) == 0 && (((uintptr_t)x | (uintptr_t)out) % 16) == 0 && "
            "(!gamma || (((uintptr_t)gamma | (uintptr_t)beta) % 16) == 0)") in na
    assert ("(c % 4) == 0 && (((uintptr_t)x | (uintptr_t)grad_out | (uintptr_t)grad_x) % 16) == 0 && "
            "(!gamma || (((uintptr_t)gamma | (uintptr_t)beta) % 16) == 0)") in na
    # which kernel: read the launch ladders and compare with the restated rules at every width
    fwd_src, bwd_src = na.split('extern "C" int fsf_norm_act_backward(')[0], na.split('extern "C" int fsf_norm_act_backward(')[1]
    for src, rule, launch in ((fwd_src, C.fwd_kernel, "launch_norm_act"), (bwd_src, C.bwd_kernel, "launch_norm_act_bwd")):
        ladder = [(int(a), C.Kern("v4", int(t), int(p), int(r)))
                  for a, t, p, r in re.findall(rf"if \(c4 <= (\d+)\) return {launch}_v4<(\d+), (\d+), (\d+)>\(", src)]
        every = re.findall(rf"return {launch}_v4<(\d+), (\d+), (\d+)>\(", src)
        last = every[-1]  # the one launch without a width test in front
        assert [a for a, _ in ladder] == [16, 32, 64, 128] and len(every) == 5
        for c in range(4, 1025, 4):
            want = next((k for a, k in ladder if c // 4 <= a), C.Kern("v4", *map(int, last)))
            assert rule(c, True) == want, c
    assert "if (c > 64 * NA_MAX_PER_LANE) return launch_norm_act<64, 16>(" in fwd_src
    for src, launch in ((fwd_src, "launch_norm_act"), (bwd_src, "launch_norm_act_bwd")):
        assert f"if (c <= 16 * NA_MAX_PER_LANE / 2) return {launch}<16>(" in src and f"if (c <= 32 * NA_MAX_PER_LANE / 2) return {launch}<32>(" in src
        assert f"return {launch}<64>(" in src
    assert [C.fwd_kernel(c, False).name for c in (64, 65, 128, 129, 512, 513, 1024)] == \
        ["s_t16_p8_r1", "s_t32_p8_r1", "s_t32_p8_r1", "s_t64_p8_r1", "s_t64_p8_r1", "s_t64_p16_r1", "s_t64_p16_r1"]
    assert [C.bwd_kernel(c, False) and C.bwd_kernel(c, False).name for c in (64, 65, 128, 129, 512, 513)] == \
        ["s_t16_p8_r1", "s_t32_p8_r1", "s_t32_p8_r1", "s_t64_p8_r1", "s_t64_p8_r1", None]
    assert C.fwd_kernel(1025, True) is None and C.bwd_kernel(1025, True) is None
    # rows per workgroup and the grid-stride steps
    assert na.count("const int rows_per_block = 256 / TEAM * RU;") == 2 and na.count("const int teams_per_block = 256 / TEAM;") == 3
    assert na.count("row0 < n; row0 += (int64_t)gridDim.x * TEAMS * RU)") == 2
    assert "row += (int64_t)gridDim.x * teams_per_block)" in na and "row < n; row += (int64_t)gridDim.x * TEAMS)" in na
    assert "template <int TEAM, int ACT, int NORM, int PL = NA_MAX_PER_LANE>" in na
    bn = _flat("batch_norm.hip")
    assert f"constexpr int CS_BLOCKS = {C.CS_BLOCKS};" in bn
    assert "static int cs_cw_log2(int c) { int l = 0; while ((1 << l) < c && l < 8) ++l; return l; }" in bn
    assert "const int ry = 256 >> cw_log2; int64_t rpb = fsf_cdiv(n, (int64_t)CS_BLOCKS); const int64_t min_rows = (int64_t)ry * 8;" in bn
    assert "if (rpb < min_rows) rpb = min_rows; *rows_per_block = rpb; return (int)fsf_cdiv(n, rpb);" in bn
    assert "a.rows_per_block = (int64_t)ry * 4;" in bn and "b.rows_per_block = (int64_t)ry * 4;" in bn
    assert "for (; r + 3 * ry < r1; r += 4 * ry)" in bn and "const int64_t r1 = r0 + a.rows_per_block < a.n ? r0 + a.rows_per_block : a.n;" in bn
    # the fold kernels: 16 slices, 64 partials a trip, a tail of three
    assert C.FOLD_STEP == 64 and C.FOLD_SLICES == 16
    assert na.count("for (; b + 48 < blocks; b += 64)") == 1 and bn.count("for (; b + 48 < blocks; b += 64)") == 2
    assert na.count("for (int u = 0; u < 3; ++u) { if (b + 16 * u < blocks)") == 1
    assert bn.count("for (int u = 0; u < 3; ++u) { if (b + 16 * u < blocks)") + bn.count("for (int u = 0; u < 3; ++u) if (b + 16 * u < blocks)") == 2
    assert na.count("const int cl = threadIdx.x & 15, sl = threadIdx.x >> 4;") == 1 and bn.count("const int cl = threadIdx.x & 15, sl = threadIdx.x >> 4;") == 2


def test_restated_rules_give_the_sizes_the_cases_are_built_on():
    assert [C.cs_cw_log2(c) for c in (1, 2, 3, 4, 5, 8, 9, 128, 129, 256, 257, 513)] == [0, 1, 2, 2, 3, 3, 4, 7, 8, 8, 8, 8]
    assert C.cs_blocks(8192, 131) == (1024, 8) and C.cs_blocks(8193, 131) == (911, 9)
    assert C.cs_blocks(32768, 64) == (1024, 32) and C.cs_blocks(32769, 64) == (993, 33) and 33 % C.cs_ry(64)
    assert [C.fwd_kernel(c, True).rows_per_wg for c in (4, 68, 132, 260, 516)] == [32, 16, 8, 4, 4]
    assert [C.bwd_kernel(c, True).rows_per_wg for c in (4, 68, 132, 260, 516)] == [32, 16, 4, 4, 4]
    biggest = max(C.FWD_SPECS.values(), key=lambda s: s[0] * s[1])
    assert biggest[0] * biggest[1] * 4 <= 135e6 and biggest[:2] == (513, 65537)


# ---- reachability ----------------------------------------------------------------------------------------------------------------------

FWD_KERNELS = ("v4_t16_p1_r2", "v4_t32_p1_r2", "v4_t64_p1_r2", "v4_t64_p2_r1", "v4_t64_p4_r1", "s_t16_p8_r1", "s_t32_p8_r1", "s_t64_p8_r1",
               "s_t64_p16_r1")
BWD_KERNELS = ("v4_t16_p1_r2", "v4_t32_p1_r2", "v4_t64_p1_r1", "v4_t64_p2_r1", "v4_t64_p4_r1", "s_t16_p8_r1", "s_t32_p8_r1", "s_t64_p8_r1")


def full_tags():
    t = set()
    for k in FWD_KERNELS:
        t |= {f"fwd:{k}:{norm}:{act}" for norm in ("ln", "affine") for act in C.ACTS} | {f"fwd:{k}:second_trip"}
        t.add(f"fwd:{k}:ragged")
    t |= {f"fwd:fallback_{lay}:{k}" for lay in C.FWD_FALLBACKS for k in FWD_KERNELS[5:]}
    t |= {"fwd:slice_keeps_v4", "fwd:dead_ru_row", "fwd:n1", "fwd:form_ln", "fwd:form_lna", "fwd:form_aff"}
    for k in BWD_KERNELS:
        t |= {f"bwd:{k}:{act}" for act in C.ACTS} | {f"bwd:{k}:second_trip"}
    t |= {f"bwd:{k}:{why}" for k in BWD_KERNELS[5:] for why in ("by_width", "by_misalignment")}
    t |= {f"bwd:layout_{lay}" for lay in C.BWD_FALLBACKS} | {"bwd:no_affine", "bwd:affine", "bwd:n0", "bwd:dead_ru_row"}
    t |= {f"bwd:fold_blocks_{b}" for b in C.FOLD_BLOCKS}
    t |= {f"bn:cw_log2_{l}" for l in range(9)} | {"bn:c_at_pow2", "bn:c_below_pow2", "bn:column_passes", "bn:column_passes_ragged", "bn:n1",
                                                  "bn:last_block_one_row", "bn:rpb_above_floor", "bn:rpb_above_floor_not_multiple_of_ry",
                                                  "bn:rpb_floor_at_1024_blocks", "bn:rows_kernel_partial_block"}
    t |= {f"bn:tail_first_{k}" for k in range(4)} | {f"bn:tail_last_{k}" for k in range(4)} | {f"bn:fold_blocks_{b}" for b in C.FOLD_BLOCKS}
    return t


def reach_table():
    table = {t: [] for t in full_tags()}
    for name in C.FWD_NAMES + C.BWD_NAMES + C.BN_NAMES:
        for t in C.tags_of(name):
            if t in table:
                table[t].append(name)
    return table


def test_reachability_table_has_no_empty_row():
    table = reach_table()
    empty = sorted(t for t, names in table.items() if not names)
    assert not empty, empty
    # the issue's widths, each in the class it names
    assert {C.FWD_SPECS[n][0] for n in C.FWD_NAMES if C.FWD_SPECS[n][4] == "plain"} >= \
        set(C.V4_WIDTHS) | set(C.SCALAR_WIDTHS)
    assert set(C.V4_WIDTHS) == {4, 64, 68, 128, 132, 256, 260, 512, 516, 1024} and set(C.SCALAR_WIDTHS) == {1, 3, 65, 127, 129, 511, 513, 1023}
    assert C.FWD_UNSUPPORTED == (1025,)
    # the second trip of each forward kernel starts one row beyond the capped grid
    for name in table["fwd:v4_t16_p1_r2:second_trip"] + table["fwd:s_t64_p16_r1:second_trip"]:
        c, n = C.FWD_SPECS[name][:2]
        k = C.fwd_kernel(c, c % 4 == 0)
        assert n == C.fwd_cap(k) * k.rows_per_wg + 1
    assert len(C.FWD_NAMES) + len(C.BWD_NAMES) + len(C.BN_NAMES) <= 800


DOC = os.path.join(ROOT, "docs", "kernels", "K12_K23_norms.md")


def reach_markdown():
    """The reachability table as docs/kernels/K12_K23_norms.md holds it: per decision the first two cases and how many more."""
    lines = ["| decision | cases |", "|---|---|"]
    for t, names in sorted(reach_table().items()):
        more = f" (+{len(names) - 2})" if len(names) > 2 else ""
        lines.append(f"| `{t}` | " + ", ".join(f"`{n}`" for n in names[:2]) + more + " |")
    return "\n".join(lines)


def test_doc_lists_the_reachability_table():
    doc = open(DOC).read()
    block = doc.split("<!-- reach:begin -->\n")[1].split("\n<!-- reach:end -->")[0]
    assert block == reach_markdown()  # regenerate the block from reach_markdown() when the cases change
    for k, v in (("K_FWD", C.K_FWD), ("K_GX", C.K_GX), ("K_COL", C.K_COL)):
        assert re.search(rf"`{k}`\)? \|[^|]*\| {v}", doc), k


def test_bn_cases_hold_the_widths_and_edges_asked_for():
    assert {C.BN_SPECS[n][0] for n in C.BN_NAMES} == set(C.BN_WIDTHS)
    for c in C.BN_WIDTHS:  # every tail length for the first and the last ty, at every width
        firsts = {C.bn_tail_tags(n, cc)[0] for cc, n in C.BN_SPECS.values() if cc == c}
        lasts = {C.bn_tail_tags(n, cc)[1] for cc, n in C.BN_SPECS.values() if cc == c}
        assert firsts == lasts == {0, 1, 2, 3}, c
    pow2 = [n for n in C.BN_NAMES if C._is_pow2(C.BN_SPECS[n][1]) and C.BN_SPECS[n][1] >= 64]
    exact = [n for n in pow2 if all(C.bn_case(n)["bwd"][k]["gx_exact"] is not None for k in (("affine", True), ("plain", False)))]
    assert len(exact) >= 8, (len(pow2), len(exact))  # grad_x bit for bit on these
    zero = sum(int((C.bn_case(n)["bwd"][("affine", True)]["y"] == 0).sum() > 0) for n in C.BN_NAMES[:40])
    assert zero >= 20  # pre-activations that are exactly 0: `>` and `>=` differ


# ---- referees against plain loops -----------------------------------------------------------------------------------------------------

def _loop_layer_norm(x, g, b, eps, form, act):
    n, c = x.shape
    out = np.zeros((n, c))
    for i in range(n):
        row = [float(v) for v in x[i]]
        mean = math.fsum(row) / c if form != "aff" else 0.0
        rstd = 1.0 / math.sqrt(math.fsum((v - mean) ** 2 for v in row) / c + eps) if form != "aff" else 1.0
        for j in range(c):
            y = (row[j] - mean) * rstd * (float(g[j]) if g is not None else 1.0) + (float(b[j]) if b is not None else 0.0)
            out[i, j] = max(y, 0.0) if act == "relu" else 0.5 * y * (1.0 + math.erf(y / math.sqrt(2.0))) if act == "gelu" else y
    return out


SMALL_FWD = [n for n in C.FWD_NAMES if C.FWD_SPECS[n][0] * C.FWD_SPECS[n][1] <= 600]
SMALL_BWD = [n for n in C.BWD_NAMES if 0 < C.BWD_SPECS[n][0] * C.BWD_SPECS[n][1] <= 600]
SMALL_BN = [n for n in C.BN_NAMES if C.BN_SPECS[n][0] * C.BN_SPECS[n][1] <= 600]


@pytest.mark.parametrize("name", SMALL_FWD)
def test_forward_referee_equals_a_plain_loop(name):
    c = C.case(name)
    want = _loop_layer_norm(c["x"], c["gamma"], c["beta"], c["eps"], c["form"], c["act"])
    got, B = C.fwd_reference(c)
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-11 * max(1.0, float(np.abs(c["x"]).max())))
    assert (B > 0).all() or c["c"] == 0


@pytest.mark.parametrize("name", SMALL_BWD)
def test_backward_referee_equals_float64_autograd(name):
    """(autograd of the plain float64 composition: an independent derivation of the three gradients)"""
    c = C.case(name)
    x = torch.from_numpy(c["x"]).double().requires_grad_()
    g = torch.from_numpy(c["gamma"]).double().requires_grad_() if c["gamma"] is not None else None
    b = torch.from_numpy(c["beta"]).double().requires_grad_() if c["beta"] is not None else None
    mean = x.mean(1, keepdim=True)
    y = (x - mean) / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + c["eps"])
    if g is not None:
        y = y * g + b
    y = torch.relu(y) if c["act"] == "relu" else 0.5 * y * (1 + torch.erf(y / math.sqrt(2.0))) if c["act"] == "gelu" else y
    y.backward(torch.from_numpy(c["go"]).double())
    r = C.bwd_reference(c)
    np.testing.assert_allclose(r["gx"], x.grad.numpy(), rtol=1e-9, atol=1e-9 * max(1.0, float(np.abs(r["gx"]).max())))
    if g is not None:
        np.testing.assert_allclose(r["dg"], g.grad.numpy(), rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(r["db"], b.grad.numpy(), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("name", SMALL_BN)
def test_bn_referee_equals_a_plain_loop(name):
    c = C.case(name)
    n, ch = c["n"], c["c"]
    for j in range(ch):
        assert int(c["want_sum"][j]) == sum(int(v) for v in c["x"][:, j])
        assert c["want_mean"][j] == F32(F32(sum(int(v) for v in c["x"][:, j])) * (F32(1.0) / F32(n)))
        if n >= 2:
            assert sum(int(v) for v in c["xb"][:, j]) == 0
            assert c["want_var"][j] == F32(F32(sum(int(v) ** 2 for v in c["xb"][:, j])) * (F32(1.0) / F32(n)))
    b = c["bwd"]
    for key, relu in (("affine", True), ("plain", False), ("plain", True)):
        sc, sh = (b["scale"], b["shift"]) if key == "affine" else (b["invstd"], -b["mean"] * b["invstd"])
        w = b[(key, relu)]
        for j in range(ch):
            sg = sgx = 0.0
            for i in range(n):
                y = float(b["x"][i, j]) * float(sc[j]) + float(sh[j])
                g = float(b["go"][i, j]) if (y > 0 or not relu) else 0.0
                sg += g
                sgx += g * (float(b["x"][i, j]) - float(b["mean"][j])) * float(b["invstd"][j])
            assert w["db"][j] == sg and w["dg"][j] == sgx
            i = n // 2
            y = float(b["x"][i, j]) * float(sc[j]) + float(sh[j])
            g = float(b["go"][i, j]) if (y > 0 or not relu) else 0.0
            t = (float(b["x"][i, j]) - float(b["mean"][j])) * float(b["invstd"][j])
            assert abs(w["gx64"][i, j] - float(sc[j]) * (g - (sg + t * sgx) / n)) <= 1e-12 * (1 + abs(w["gx64"][i, j]))


def test_exact_families_keep_every_partial_sum_exact():
    for name in C.BWD_NAMES:
        c, n, _, _, _, fam = C.BWD_SPECS[name]
        if fam == "ints":
            assert 8 * n < 2 ** 24
    big = max(n for _, n in C.BN_SPECS.values())
    assert 64 * big < 2 ** 24 and 2 * 40 * big < 2 ** 24 and big == 32769
    c = C.bn_case("bn-c5-n97")
    assert set(np.unique(np.abs(c["x"]))) == set(range(1, 9)) and (c["want_mean"] != 0).any()


def test_relu_backward_cases_keep_the_mask_unambiguous():
    seen = zeros = 0
    for name in C.BWD_NAMES:
        spec = C.BWD_SPECS[name]
        if spec[3] != "relu" or spec[0] * spec[1] > 1 << 18 or spec[1] == 0:
            continue
        c = C.case(name)
        y, B = c["mask_margin"]
        exact0 = np.zeros(c["c"], bool) if c["gamma"] is None else (c["gamma"] == 0) & (c["beta"] == 0)
        live = (c["go"] != 0) & ~exact0
        assert (np.abs(y[live]) > C.MASK_MARGIN * B[live]).all(), name
        if exact0.any():
            assert (c["go"][:, exact0] != 0).all() and (y[:, exact0] == 0).all()
            zeros += 1
        assert (c["go"] != 0).mean() > 0.9  # (the margin silences few elements)
        seen += 1
    assert seen >= 20 and zeros >= 20


def test_grad_gamma_is_judged_only_where_one_row_exceeds_the_bound():
    judged = 0
    for name in C.BWD_NAMES:
        spec = C.BWD_SPECS[name]
        if spec[1] == 0 or spec[1] > C.GAMMA_MAX_ROWS or not spec[2]:
            continue
        c = C.case(name)
        r = C.bwd_reference(c)
        one_row = np.abs(r["gy"] * r["xh"]).mean(0)
        live = one_row > 0  # (c = 1: xhat is 0; the two channels of a ReLU case with gamma = beta = 0)
        bound = C.K_COL * r["P_dg"] + r["A_dg"]
        assert (one_row[live] > bound[live]).all(), (name, float((bound[live] / one_row[live]).max()))
        one_b = np.abs(r["gy"]).mean(0)
        assert (one_b[one_b > 0] > (C.K_COL * r["P_db"] + r["A_db"])[one_b > 0]).all(), name
        judged += 1
    assert judged >= 100


# ---- the constants of the normal family, from the host's fp32 ------------------------------------------------------------------------

def measure_host_ratios():
    """Largest |torch fp32 - float64| / (budget at K = 1) over the `normal` cases: (forward, grad_x, column sums)."""
    import torch.nn.functional as Fn

    r_fwd = r_gx = r_col = 0.0
    for name in C.FWD_NAMES:
        c, n, form, act, layout, fam = C.FWD_SPECS[name]
        if c * n > 1 << 18:
            continue
        cs = C.case(name)
        x = torch.from_numpy(cs["x"])
        g = torch.from_numpy(cs["gamma"]) if cs["gamma"] is not None else None
        b = torch.from_numpy(cs["beta"]) if cs["beta"] is not None else None
        y = Fn.layer_norm(x, (c,), g, b, cs["eps"]) if form != "aff" else x * g + b
        y = torch.relu(y) if act == "relu" else Fn.gelu(y) if act == "gelu" else y
        want, B = C.fwd_reference(cs)
        unit = (B - (C.GELU_FWD_ABS if act == "gelu" else 0.0)) / C.K_FWD
        r_fwd = max(r_fwd, float((np.abs(y.numpy().astype(F64) - want) / unit).max()))
    for name in C.BWD_NAMES:
        c, n, affine, act, layout, fam = C.BWD_SPECS[name]
        if c * n > 1 << 18 or n == 0 or fam == "ints":
            continue
        cs = C.case(name)
        x = torch.from_numpy(cs["x"]).requires_grad_()
        g = torch.from_numpy(cs["gamma"]).requires_grad_() if affine else None
        b = torch.from_numpy(cs["beta"]).requires_grad_() if affine else None
        y = Fn.layer_norm(x, (c,), g, b, cs["eps"])
        y = torch.relu(y) if act == "relu" else Fn.gelu(y) if act == "gelu" else y
        y.backward(torch.from_numpy(cs["go"]))
        r = C.bwd_reference(cs)
        r_gx = max(r_gx, float((np.abs(x.grad.numpy().astype(F64) - r["gx"]) / np.maximum(r["P_gx"], 1e-300)).max()))
        if affine:
            for got, want, P, A in ((g.grad, r["dg"], r["P_dg"], r["A_dg"]), (b.grad, r["db"], r["P_db"], r["A_db"])):
                err = np.abs(got.numpy().astype(F64) - want) - A  # beyond the summation bound
                live = P > 0
                if live.any():
                    r_col = max(r_col, float((np.maximum(err, 0)[live] / P[live]).max()))
    return r_fwd, r_gx, r_col


def test_budget_constants_are_twice_the_hosts_fp32_ratio_with_a_floor_of_4():
    ratios = measure_host_ratios()
    print("host fp32 ratios (forward, grad_x, column sums):", ratios)
    for r, k in zip(ratios, (C.K_FWD, C.K_GX, C.K_COL)):
        assert k >= 4.0 and 2.0 * r <= k, (ratios, k)


# ---- numpy models of the two reduction schemes, with switchable defects ---------------------------------------------------------------

DEFECTS = ("grid_stride_by_threads_not_teams", "dead_ru_row_counted", "tail_lanes_enter_the_mean", "division_by_padded_width",
           "fold_tail_drops_b_plus_32", "fold_main_loop_off_by_one_at_48", "unroll_tail_drops_a_row", "last_block_r1_not_clamped",
           "gamma_beta_partials_swapped", "relu_mask_from_ge")


def fold(part, blocks, mul=None, defect=None):
    """[blocks, c] f32 -> [c] as norm_act_bwd_fold_kernel / column_fold_kernel / bn_finalize_kernel add them; what lies beyond
    `blocks` in the workspace is NaN here."""
    c = part.shape[1]
    buf = np.full((C.CS_BLOCKS + 2 * C.FOLD_STEP, c), np.nan, F32)
    buf[:blocks] = part
    total = np.zeros(c, F32)
    for sl in range(C.FOLD_SLICES):
        a = [np.zeros(c, F32) for _ in range(4)]
        b = sl
        while (b + 48 <= blocks) if defect == "fold_main_loop_off_by_one_at_48" else (b + 48 < blocks):
            for u in range(4):
                a[u] = a[u] + buf[b + 16 * u]
            b += C.FOLD_STEP
        for u in range(2 if defect == "fold_tail_drops_b_plus_32" else 3):
            if b + 16 * u < blocks:
                a[u] = a[u] + buf[b + 16 * u]
        total = total + ((a[0] + a[1]) + (a[2] + a[3]))
    return total if mul is None else total * F32(mul)


def k12_visits(n, k, G, defect=None):
    """(rows, workgroup of each) in the grid-stride loop of a K12 kernel, with multiplicity."""
    teams = 256 // k.team
    step = G * (256 if defect == "grid_stride_by_threads_not_teams" else teams) * k.ru
    start = np.arange(G * teams, dtype=np.int64) * k.ru
    row0 = start[:, None] + np.arange(C.cdiv(n, step) + 1, dtype=np.int64)[None, :] * step
    rows = row0[..., None] + np.arange(k.ru)
    live = (row0 < n)[..., None] & (rows < n)
    if defect == "dead_ru_row_counted":
        dead = (row0 < n)[..., None] & (rows >= n)
        rows, live = np.where(dead, n - 1, rows), live | dead
    blk = np.broadcast_to((np.arange(G * teams) // teams)[:, None, None], rows.shape)
    return rows[live], blk[live]


def _k12_stats(c, k, defect):
    x = c["x"]
    if c["form"] == "aff":
        return np.zeros((c["n"], 1), F32), np.ones((c["n"], 1), F32)
    inv_c = F32(1.0) / F32(k.slots if defect == "division_by_padded_width" else c["c"])
    mean = x.sum(1, dtype=F32, keepdims=True) * inv_c
    d = x - mean
    q = (d * d).sum(1, dtype=F32, keepdims=True)
    if defect == "tail_lanes_enter_the_mean":
        q = q + F32(k.slots - c["c"]) * (mean * mean)
    return mean, F32(1.0) / np.sqrt(q * inv_c + F32(c["eps"]))


def k12_forward_model(c, defect=None):
    k, n = c["kern"], c["n"]
    mean, rstd = _k12_stats(c, k, defect)
    y = (c["x"] - mean) * rstd
    if c["gamma"] is not None:
        y = y * c["gamma"] + c["beta"]
    if c["act"] == "relu":
        y = np.maximum(y, F32(0))
    elif c["act"] == "gelu":
        y = (0.5 * y.astype(F64) * (1.0 + C._erf(y.astype(F64) / np.sqrt(2.0)))).astype(F32)
    rows, _ = k12_visits(n, k, C.grid(n, k, C.fwd_cap(k)), defect)
    out = np.full((n, c["c"]), np.nan, F32)
    out[rows] = y[rows]
    return out


def k12_backward_model(c, defect=None):
    k, n, ch = c["kern"], c["n"], c["c"]
    if n == 0:
        z = np.zeros(ch, F32) if c["gamma"] is not None else None
        return np.zeros((0, ch), F32), z, z
    mean, rstd = _k12_stats(c, k, defect)
    inv_c = F32(1.0) / F32(k.slots if defect == "division_by_padded_width" else ch)
    g = c["gamma"] if c["gamma"] is not None else np.ones(ch, F32)
    b = c["beta"] if c["beta"] is not None else np.zeros(ch, F32)
    xh = (c["x"] - mean) * rstd
    y = xh * g + b
    gy = c["go"]
    if c["act"] == "relu":
        gy = np.where((y >= 0) if defect == "relu_mask_from_ge" else (y > 0), gy, F32(0))
    elif c["act"] == "gelu":
        y64 = y.astype(F64)
        gy = (gy * (0.5 * (1.0 + C._erf(y64 / np.sqrt(2.0))) + y64 * np.exp(-0.5 * y64 * y64) / np.sqrt(2.0 * np.pi))).astype(F32)
    gh = gy * g
    m1 = gh.sum(1, dtype=F32, keepdims=True) * inv_c
    m2 = (gh * xh).sum(1, dtype=F32, keepdims=True) * inv_c
    G = C.grid(n, k, C.NA_BWD_BLOCKS)
    rows, blk = k12_visits(n, k, G, defect)
    gx = np.full((n, ch), np.nan, F32)
    gx[rows] = (rstd * (gh - m1 - xh * m2))[rows]
    part = np.zeros((2, G, ch), F64)
    np.add.at(part[0], blk, (gy * xh).astype(F64)[rows])
    np.add.at(part[1], blk, gy.astype(F64)[rows])
    part = part.astype(F32)
    if defect == "gamma_beta_partials_swapped":
        part = part[::-1]
    if c["gamma"] is None:
        return gx, None, None
    return gx, fold(part[0], G, None, defect), fold(part[1], G, None, defect)


def k23_included(n, c, defect=None):
    """(row, workgroup) pairs column_stats_kernel accumulates: ty walks r0 + ty, + ry, ... four at a time, then a tail of up to three."""
    blocks, rpb = C.cs_blocks(n, c)
    ry = C.cs_ry(c)
    n_eff = blocks * rpb if defect == "last_block_r1_not_clamped" else n
    r = np.arange(n_eff, dtype=np.int64)
    b = r // rpb
    local = r - b * rpb
    R = np.minimum(rpb, n_eff - b * rpb)
    ty, j = local % ry, local // ry
    cnt = -(-(R - ty) // ry)
    inc = j < 4 * (cnt // 4) + np.minimum(2 if defect == "unroll_tail_drops_a_row" else 3, cnt % 4)
    return r[inc], b[inc], blocks, n_eff


def k23_sums(vals, n, c, defect=None):
    """Column sums of one or two [n, c] arrays through rows -> partial -> fold (no final factor)."""
    r, b, blocks, n_eff = k23_included(n, c, defect)
    out = []
    for v in vals:
        v = np.concatenate([v.astype(F64), np.full((n_eff - n, c), np.nan)])  # rows beyond n: not the caller's memory
        part = np.zeros((blocks, c), F64)
        np.add.at(part, b, v[r])
        out.append(part.astype(F32))
    if defect == "gamma_beta_partials_swapped":
        out = out[::-1]
    return [fold(p, blocks, None, defect) for p in out]


def k23_model(c, defect=None):
    n, ch = c["n"], c["c"]
    inv_n = F32(1.0) / F32(n)
    got = {}
    (got["sum"],) = k23_sums([c["x"]], n, ch, defect)
    got["mean"] = got["sum"] * inv_n
    if n >= 2:
        (mb,) = k23_sums([c["xb"]], n, ch, defect)
        mb = mb * inv_n
        d = c["xb"] - mb
        (sq,) = k23_sums([d * d], n, ch, defect)
        got["mean_b"], got["var"] = mb, sq * inv_n
    bw = c["bwd"]
    for key, relu in (("affine", True), ("plain", False), ("plain", True), ("affine", False)):
        sc, sh = (bw["scale"], bw["shift"]) if key == "affine" else (bw["invstd"], -bw["mean"] * bw["invstd"])
        y = bw["x"] * sc + sh
        g = np.where((y >= 0) if defect == "relu_mask_from_ge" else (y > 0), bw["go"], F32(0)) if relu else bw["go"]
        got[(key, relu)] = tuple(k23_sums([g, g * ((bw["x"] - bw["mean"]) * bw["invstd"])], n, ch, defect))  # (grad_beta, grad_gamma)
    return got


def _differs(fn, *a):
    try:
        fn(*a)
    except AssertionError:
        return True
    return False


def k12_disagreements(c, defect=None):
    bad = []
    if c["name"].startswith("fwd"):
        return ["out"] if _differs(C.check_fwd, c, k12_forward_model(c, defect)) else []
    gx, dg, db = k12_backward_model(c, defect)
    if c["n"] == 0:
        return ["grads"] if _differs(C.check_bwd, c, gx, dg, db) else []
    r = C.bwd_reference(c)
    if _differs(C._per_element, gx, r["gx"], C.K_GX * r["P_gx"] + r["A_gx"], "gx"):
        bad.append("gx")
    if c["gamma"] is not None:
        if "want_db" in c:
            if not np.array_equal(db, c["want_db"]):
                bad.append("db")
        elif _differs(C._per_element, db, r["db"], C.K_COL * r["P_db"] + r["A_db"], "db"):
            bad.append("db")
        if C.gamma_judged(c) and _differs(C._per_element, dg, r["dg"], C.K_COL * r["P_dg"] + r["A_dg"], "dg"):
            bad.append("dg")
    return bad


def k23_disagreements(c, defect=None):
    got, bad = k23_model(c, defect), []
    for key, want in (("sum", "want_sum"), ("mean", "want_mean"), ("var", "want_var")):
        if key in got and not np.array_equal(got[key], c[want]):
            bad.append(key)
    if "mean_b" in got and (got["mean_b"] != 0).any():
        bad.append("mean_b")
    for k in (("affine", True), ("plain", False), ("plain", True), ("affine", False)):
        db, dg = got[k]
        if not np.array_equal(db, c["bwd"][k]["db"]):
            bad.append(("db",) + k)
        if not np.array_equal(dg, c["bwd"][k]["dg"]):
            bad.append(("dg",) + k)
    return bad


def _modelled(name):
    spec = (C.FWD_SPECS if name.startswith("fwd") else C.BWD_SPECS)[name]
    return spec[0] * spec[1] <= 1 << 21


K12_MODELLED = [n for n in C.FWD_NAMES + C.BWD_NAMES if _modelled(n)]


@pytest.mark.parametrize("name", K12_MODELLED)
def test_k12_model_without_defect_equals_the_referee(name):
    assert k12_disagreements(C.case(name)) == []


@pytest.mark.parametrize("name", C.BN_NAMES)
def test_k23_model_without_defect_equals_the_referee(name):
    assert k23_disagreements(C.bn_case(name)) == []


def test_every_second_trip_case_visits_each_row_once_and_the_wrong_step_does_not():
    """The large forward cases are not modelled in values: here their visiting order alone."""
    for name in C.FWD_NAMES:
        c, n, form, act, layout, _ = C.FWD_SPECS[name]
        k = C.fwd_kernel(c, C.is_v4(c, layout, form != "ln"))
        cap = C.fwd_cap(k)
        if n <= cap * k.rows_per_wg:
            continue
        rows, _ = k12_visits(n, k, C.grid(n, k, cap))
        assert np.array_equal(np.sort(rows), np.arange(n)), name
        rows, _ = k12_visits(n, k, C.grid(n, k, cap), "grid_stride_by_threads_not_teams")
        assert not np.isin(n - 1, rows), name  # a step of whole workgroups of threads: the row of the second trip is never written


# one case per defect that tells the defective kernel from the right one, and the output it shows in
WITNESS = {
    "grid_stride_by_threads_not_teams": ("fwd-c4-n262145-ln-gelu-plain-normal", "out"),
    "dead_ru_row_counted": ("bwd-c4-n31-lna-none-plain-ints", "db"),
    "tail_lanes_enter_the_mean": ("fwd-c68-n17-ln-none-plain-normal_off", "out"),
    "division_by_padded_width": ("fwd-c132-n9-lna-none-plain-normal", "out"),
    "fold_tail_drops_b_plus_32": ("bn-c131-n376", "sum"),
    "fold_main_loop_off_by_one_at_48": ("bwd-c4-n1536-lna-none-plain-ints", "db"),
    "unroll_tail_drops_a_row": ("bn-c5-n96", "sum"),
    "last_block_r1_not_clamped": ("bn-c64-n33", "sum"),
    "gamma_beta_partials_swapped": ("bwd-c3-n15-lna-none-plain-ints", "db"),
    "relu_mask_from_ge": ("bwd-c68-n17-lna-relu-plain-normal_off", "db"),
}


def _disagreements(name, defect=None):
    return k23_disagreements(C.bn_case(name), defect) if name.startswith("bn") else k12_disagreements(C.case(name), defect)


@pytest.mark.parametrize("defect", DEFECTS)
def test_each_defect_is_caught_by_its_named_case(defect):
    name, where = WITNESS[defect]
    assert name in C.FWD_SPECS or name in C.BWD_SPECS or name in C.BN_SPECS, name
    assert _disagreements(name) == []
    assert where in _disagreements(name, defect), (defect, name, _disagreements(name, defect))


def test_defects_are_caught_widely():
    """Not one lucky case: every defect shows in several cases."""
    names = [n for n in K12_MODELLED if (C.FWD_SPECS.get(n) or C.BWD_SPECS[n])[0] * (C.FWD_SPECS.get(n) or C.BWD_SPECS[n])[1] <= 1 << 17]
    names = names[::3] + [n for n in C.BN_NAMES if C.BN_SPECS[n][0] * C.BN_SPECS[n][1] <= 1 << 17][::2] + [w for w, _ in WITNESS.values()]
    names += [n for n in C.BWD_NAMES if C.BWD_SPECS[n][1] > 4096 and C.BWD_SPECS[n][0] <= 4]  # (second trips of the grid-stride loop)
    caught = {d: 0 for d in DEFECTS}
    for n in dict.fromkeys(names):
        for d in DEFECTS:
            caught[d] += bool(_disagreements(n, d))
    print(caught)
    assert all(v >= 3 for v in caught.values()), caught
