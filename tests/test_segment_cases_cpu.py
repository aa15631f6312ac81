"""CPU: what the segmented-reduction tests on the device (tests/test_segment_gpu.py) stand on.

* The constants and the three selection rules restated in tests/segment_cases.py against the text of csrc/segment.hip and
  csrc/radix_sort.h, so that a retuned kernel gets its witnesses re-derived.
* Path witnesses: each layout family reaches the kernel decisions it is there for, and the union over all cases is the full tag set.
* The referee against a plain Python loop on the small cases, and the exact-integer argument of the `ints` families.
* Decisiveness without a GPU: a numpy model of the chunked algorithm (chunk pass with slots 0 / 1, short fix-up, long fold by teams
  in the kernel's visiting order) equals the referee on every case, and with each of eight plausible defects switched on it differs
  on a case named here: the cases can tell such a kernel from a right one."""
import os
import re

import numpy as np
import pytest

import segment_cases as C
from conftest import ROOT

F32 = np.float32
CSRC = os.path.join(ROOT, "fullysparsefusion_amd", "csrc")


# ---- source pin ------------------------------------------------------------------------------------------------------------------

def _const(src, name):
    return int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))


def test_constants_and_rules_equal_the_kernel_source():
    src = open(os.path.join(CSRC, "segment.hip")).read()
    assert int(re.search(r"#define SEG_CHUNK_ROWS (\d+)", src).group(1)) == C.SEG_CHUNK and "constexpr int SEG_CHUNK = SEG_CHUNK_ROWS;" in src
    for name in ("SEG_BLOCK", "SEG_MIN_TEAM", "SEG_LONG_SPAN", "UNR", "SEG_SHORT_MAX"):
        assert _const(src, name) == getattr(C, name), name
    rs = open(os.path.join(CSRC, "radix_sort.h")).read()
    assert _const(rs, "RS_THREADS") * _const(rs, "RS_ITEMS") == C.RS_TILE and "constexpr int RS_TILE = RS_THREADS * RS_ITEMS;" in rs
    flat = re.sub(r"\s+", " ", src)
    # pick_team
    assert ("static int pick_team(int c, int vec) { int groups = (c + vec - 1) / vec; int t = SEG_MIN_TEAM; "
            "while (t < groups && t < 64) t <<= 1; return t; }") in flat
    # gridDim.y of the long fold, its x cap, and when it is launched at all
    assert "const int groups = (a.c + VEC - 1) / VEC;" in flat
    assert "(unsigned)(VEC == 4 ? (groups >= 32 ? 4 : (groups >= 16 ? 2 : 1)) : 1)" in flat
    assert f"int64_t g3x = a.m < {C.LONG_GRID_X} ? a.m : {C.LONG_GRID_X};" in flat
    assert "const bool has_long = a.n > (int64_t)SEG_LONG_SPAN * SEG_CHUNK;" in flat
    # channel slice and team of the long fold
    assert "const int csl = (int)((a.c + (int)gridDim.y * VEC - 1) / ((int)gridDim.y * VEC)) * VEC;" in flat
    assert "int team = SEG_MIN_TEAM; while (team * VEC < csl && team < 64) team <<= 1; const int nteams = SEG_BLOCK / team;" in flat
    assert "for (int p0 = team_id; act && p0 <= ce - cs; p0 += nteams * UNR)" in flat and "const int p = p0 + u * nteams;" in flat
    # which pass folds which span, and the slot of a piece
    assert "if (cs == ce || ce - cs > SEG_LONG_SPAN) continue;" in flat and "if (ce - cs <= SEG_LONG_SPAN) continue;" in flat
    assert "const int which = (S < piece_lo) ? 0 : 1;" in flat
    # the float4 condition of both entry points
    assert "(c % 4 == 0) && (a.feat_stride % 4 == 0) && (((uintptr_t)feat | (uintptr_t)out) % 16 == 0)" in flat
    assert "(channels[t] % 4) == 0 && (st % 4) == 0 && (((uintptr_t)feats[t] | (uintptr_t)outs[t]) % 16) == 0" in flat


def test_restated_rules_give_the_sweeps_the_layouts_are_built_on():
    shape = {w: C.long_fold_shape(C.WIDTHS[w].c, C.WIDTHS[w].vec) for w in C.WIDTHS}
    assert {w: shape[w][3] * C.UNR for w in C.SWEEP_WIDTHS} == {"c4": 256, "c64": 128, "c128": 128, "c256": 64, "c131": 16}
    assert [shape[w][0] for w in ("c4", "c32", "c64", "c68", "c128", "c260", "c131", "v72_4", "v68_1")] == [1, 1, 2, 2, 4, 4, 1, 2, 1]
    assert shape["c68"][:2] == (2, 36) and shape["c260"][:2] == (4, 68)  # last slices of 32 and 56 channels
    assert [C.WIDTHS[w].vec for w in ("v72_4", "v68_1", "v66_0")] == [4, 1, 1]
    assert {w.c for w in C.WIDTHS.values() if w.vec == 4} == set(C.VEC4_CHANNELS) and \
        {w.c for w in C.WIDTHS.values() if w.vec == 1} == set(C.VEC1_CHANNELS) | {64}
    assert C.pick_team(260, 4) * 4 < 260 and C.pick_team(256, 4) * 4 == 256 and C.pick_team(131, 1) == 64 and C.pick_team(5, 1) == 8


# ---- path witnesses --------------------------------------------------------------------------------------------------------------

def _tags(layout, width="c4"):
    lengths = C.LAYOUTS[layout]()
    w = C.WIDTHS[width]
    return C.paths(lengths, sum(lengths), w.c, w.vec)


def _spans(lengths):
    off = C.offsets(lengths)
    return [((off[s + 1] - 1) // C.SEG_CHUNK - off[s] // C.SEG_CHUNK) if lengths[s] else None for s in range(len(lengths))]


def test_inside_keeps_every_segment_within_one_chunk():
    lengths = C.inside()
    t = _tags("inside")
    assert set(_spans(lengths)) == {0} and sum(lengths) % C.SEG_CHUNK == 0
    assert {"whole_in_chunk", "whole_aligned_chunk", "long_launch_no_long_segment"} <= t and "partial_last_chunk" not in t
    runs = "".join("1" if v == 1 else "x" for v in lengths)
    assert "1" * 32 in runs  # a whole chunk of 1-row segments


def test_straddle_holds_every_kind_of_span_1():
    lengths = C.straddle()
    off = C.offsets(lengths)
    t = _tags("straddle")
    assert {"short_span_1", "head_whole_chunk", "tail_on_boundary", "tail_whole_head_chunk", "partial_last_chunk", "whole_in_chunk",
            "no_long_launch"} <= t
    assert set(_spans(lengths)) == {0, 1}
    kinds = {(int(off[s] % 32 == 0), int(off[s + 1] % 32 == 0), int(lengths[s])) for s in range(len(lengths)) if _spans(lengths)[s] == 1}
    assert any(a == 0 and b == 0 for a, b, _ in kinds)                  # both pieces partial
    assert any(a == 1 and b == 0 and 33 <= v <= 63 for a, b, v in kinds)  # from a chunk boundary
    assert any(a == 0 and b == 1 for a, b, _ in kinds)                  # to a chunk boundary
    assert (1, 1, 64) in kinds                                          # two whole chunks
    s = lengths.index(10, 8)
    assert off[s] // 32 == (off[s + 1] - 1) // 32 == 8 and off[s - 1] < 256 < off[s] and off[s + 1] < 288 < off[s + 2]  # tail + whole + head


def test_span_edges_put_equal_lengths_on_both_sides_of_the_rule():
    lengths = C.span_edges()
    off, spans = C.offsets(lengths), _spans(lengths)
    got = {(int(lengths[s]), int(off[s] % 32)): spans[s] for s in range(len(lengths)) if spans[s]}
    assert got[(514, 0)] == 16 and got[(514, 31)] == 17 and got[(544, 0)] == 16 and got[(545, 0)] == 17
    assert sorted(set(got.values())) == [2, 15, 16, 17, 18]
    assert {"short_span_2", "short_span_15", "short_span_16", "long_span_17", "long_span_18"} <= _tags("span_edges")


def test_single_segments_select_each_launch():
    assert C.SINGLE_SIZES == (1, 31, 32, 33, 16 * 32, 16 * 32 + 1, 17 * 32 + 1, 8193)
    for n in C.SINGLE_SIZES:
        t = _tags(f"single_{n}")
        assert ("no_long_launch" in t) == (n <= 512), n
        assert ("long_launch_no_long_segment" in t) == (n == 513) and ("long_span_17" in t) == (n == 545), n
    assert "whole_aligned_chunk" in _tags("single_32") and "short_span_1" in _tags("single_33") and "short_span_16" in _tags("single_513")
    assert "long_span_more" in _tags("single_8193")


def test_long_sweeps_pin_the_partial_count_against_the_sweep():
    want = {"idle": {"long_idle_teams", "long_dead_slot"}, "teams+1": {"long_dead_slot"}, "sweep-1": {"long_dead_slot"}, "sweep": set(),
            "sweep+1": {"long_second_sweep", "long_dead_slot"}, "2sweep+3": {"long_second_sweep", "long_dead_slot"}}
    three = {"long_idle_teams", "long_dead_slot", "long_second_sweep"}
    rows = 0
    for width in C.SWEEP_WIDTHS:
        w = C.WIDTHS[width]
        nteams = C.long_fold_shape(w.c, w.vec)[3]
        sweep = nteams * C.UNR
        for kind, fn in C.SWEEP_KINDS:
            layout = f"long_sweeps_{width}_{kind}"
            if layout not in C.LAYOUTS:
                assert fn(nteams, sweep) < C.MIN_LONG_PARTIALS or sweep < C.MIN_LONG_PARTIALS, layout  # no long segment has so few partials
                continue
            lengths = C.LAYOUTS[layout]()
            (span,) = [s for s in _spans(lengths) if s]
            P = span + 1
            rows = max(rows, sum(lengths))
            t = _tags(layout, width)
            if sweep >= C.MIN_LONG_PARTIALS:
                assert P == fn(nteams, sweep) and t & three == want[kind], (layout, P, t)
            else:  # c = 131: the same edge whole sweeps later
                assert (P - fn(nteams, sweep)) % sweep == 0 and "long_second_sweep" in t, (layout, P)
            assert C.find(layout=layout, width=width), layout
    assert {sp[0].split("_")[2] for sp in C.SPECS.values() if sp[0].startswith("long_sweeps")} == set(C.SWEEP_WIDTHS)
    assert {C.sweep_partials("c131", k) for k, _ in C.SWEEP_KINDS} >= {31, 32, 33, 35}
    assert rows == (2 * 256 + 3 - 1) * 32 + 9 + 3  # the largest: 515 partials of 4 channels, ~16.5 k rows


def test_mixed_frame_is_a_frame():
    lengths = np.asarray(C.mixed_frame())
    assert 19000 <= lengths.sum() <= 23000 and lengths.size == C.MIXED_M > 2048
    assert ((lengths >= 1) & (lengths <= 5)).sum() >= 1800 and ((lengths >= 40) & (lengths <= 500)).sum() >= 24 and (lengths == 0).sum() >= 150
    assert sorted(lengths[lengths > 500].tolist()) == [600, 3000, 6000]
    k = sorted(C.MIXED_LONG)[0]
    assert lengths[k] > 17 * 32 + 31 and lengths[k + C.LONG_GRID_X] > 17 * 32 + 31 and min(lengths.size, C.LONG_GRID_X) == C.LONG_GRID_X
    assert {"two_long_one_workgroup", "tail_whole_head_chunk", "whole_in_chunk", "short_span_1"} <= _tags("mixed_frame")


def test_empty_ids_first_last_and_in_runs():
    assert {"empty_first", "empty_last", "empty_run", "no_long_launch"} <= _tags("empty_ends")
    assert {"no_rows", "empty_first", "empty_last", "empty_run"} <= _tags("empty_n0") and C.LAYOUTS["empty_n0"]() == [0, 0, 0]


def test_channel_rules_are_reached_on_long_segments():
    for width, tags in (("c4", {"grid_y_1"}), ("c64", {"grid_y_2"}), ("c68", {"grid_y_2", "uneven_slice"}), ("c128", {"grid_y_4"}),
                        ("c260", {"grid_y_4", "uneven_slice", "chan_loop_vec4"}), ("c131", {"grid_y_1", "chan_loop_vec1"}),
                        ("v72_4", {"grid_y_2"}), ("v68_1", {"grid_y_1"}), ("v66_0", {"grid_y_1"})):
        for layout in C.ALL_WIDTH_LAYOUTS:
            assert tags <= _tags(layout, width), (layout, width)
            assert C.find(layout=layout, width=width), (layout, width)


def test_the_cross_holds_what_it_must_and_the_union_is_every_tag():
    union = set()
    for name in C.NAMES:
        union |= C.case_paths(name)
    assert union >= C.FULL_TAGS, sorted(C.FULL_TAGS - union)
    for layout in C.CROSS_LAYOUTS:
        n = sum(C.LAYOUTS[layout]())
        for width in C.CORE_WIDTHS:
            orders = {C.SPECS[x][2] for x in C.find(layout=layout, width=width)}
            assert orders == (set(C.ORDERS) if n > 1 else {"identity"}), (layout, width)
        fams = {(C.SPECS[x][3], C.WIDTHS[C.SPECS[x][1]].vec) for x in C.find(layout=layout)}
        if n > 1:
            assert fams >= {(f, v) for f in C.FAMILIES for v in (1, 4)}, layout  # every family in a float4 and in a scalar width
    for layout in C.ALL_WIDTH_LAYOUTS:
        assert {C.SPECS[x][1] for x in C.find(layout=layout)} == set(C.WIDTHS)
    assert C.SPECS[C.AUTOGRAD_CASE] == ("mixed_frame", "c68", "shuffled", "relu_like")
    assert len(C.NAMES) <= 170


def test_shuffled_cases_are_real_permutations_and_sizes_hold():
    for name in C.NAMES:
        c = C.case(name)
        assert c["feat"].shape == (c["n"], c["width"].c) and c["feat"].dtype == F32 and c["inv"].dtype == np.int64
        np.testing.assert_array_equal(np.bincount(c["inv"], minlength=c["m"]), c["lengths"])
        if (c["lengths"] > 0).sum() > 1:  # (the rows of a single segment have one order)
            assert bool((np.diff(c["inv"]) >= 0).all()) == (c["order"] == "identity"), name
        assert c["n"] <= 23000 and c["width"].c <= 260 and not np.isnan(c["feat"]).any()
        if c["family"] != "inf":
            assert np.isfinite(c["feat"]).all()
        if c["family"] == "relu_like" and c["width"].c >= 16 and c["n"] > 1:
            longest = int(np.argmax(c["lengths"]))
            assert (c["feat"][c["inv"] == longest] == 0).all(0).any(), name  # a whole column of the longest segment is 0


def test_inf_cases_hold_each_kind_of_infinity():
    seen = 0
    for name in C.find(family="inf"):
        c = C.case(name)
        mk, x = c["marks"], c["feat"]
        if c["n"] == 0:
            continue
        assert mk["neg_cols"], name
        for s, ch in mk["neg_cols"]:
            rows = np.nonzero(c["inv"] == s)[0]
            assert (x[rows, ch] == -np.inf).all() and c["want_max"][s, ch] == -np.inf and c["want_arg"][s, ch] == rows.min(), name
        if c["layout"] in C.ALL_WIDTH_LAYOUTS and c["width"].c > 1:
            assert mk["neg_first"] and mk["pos"], name
        if mk["neg_first"]:
            s, ch, row = mk["neg_first"]
            rows = np.nonzero(c["inv"] == s)[0]
            assert row == rows.min() and x[row, ch] == -np.inf and np.isfinite(x[rows[1:], ch]).all()
            assert np.isfinite(c["want_max"][s, ch]) and c["want_arg"][s, ch] != row
            seen += 1
        if mk["pos"]:
            r, ch = mk["pos"]
            assert x[r, ch] == np.inf and c["want_max"][c["inv"][r], ch] == np.inf and c["want_arg"][c["inv"][r], ch] == r
    assert seen >= 10


# ---- referee ---------------------------------------------------------------------------------------------------------------------

SMALL = [n for n in C.NAMES if 0 < sum(C.LAYOUTS[C.SPECS[n][0]]()) * C.WIDTHS[C.SPECS[n][1]].c <= 3400]


def _loop_referee(c):
    m, ch, n = c["m"], c["width"].c, c["n"]
    vmax, arg = np.zeros((m, ch), F32), np.full((m, ch), n, np.int64)
    tot, seen = np.zeros((m, ch), np.float64), np.zeros(m, np.int64)
    for i in range(n):
        s = int(c["inv"][i])
        for k in range(ch):
            v = c["feat"][i, k]
            if seen[s] == 0 or v > vmax[s, k]:
                vmax[s, k], arg[s, k] = v, i
            tot[s, k] += float(v)
        seen[s] += 1
    return vmax, arg, tot, seen


@pytest.mark.parametrize("name", SMALL)
def test_referee_equals_a_plain_loop(name):
    c = C.case(name)
    vmax, arg, tot, seen = _loop_referee(c)
    np.testing.assert_array_equal(c["want_max"], vmax)
    np.testing.assert_array_equal(c["want_arg"], arg)
    np.testing.assert_array_equal(c["cnt"], seen)
    if c["family"] in C.EXACT_SUM_FAMILIES:
        np.testing.assert_array_equal(c["want_sum"].astype(np.float64), tot)
        np.testing.assert_array_equal(c["want_mean"], tot.astype(F32) / np.maximum(seen, 1).astype(F32)[:, None])
    elif c["family"] == "normal":
        np.testing.assert_allclose(c["sum64"], tot, rtol=1e-12, atol=1e-300)  # (two float64 summation orders)


def test_small_cases_cover_the_families_and_ties_are_everywhere():
    assert {C.SPECS[n][3] for n in SMALL} == set(C.FAMILIES) and {C.SPECS[n][0] for n in SMALL} >= {"straddle", "empty_ends", "single_33"}
    c = C.case(C.find(layout="span_edges", family="ints")[0])
    long_rows = c["lengths"][:, None] >= 481
    ties = (c["feat"] == c["want_max"][c["inv"]]).astype(np.int64)
    per = C.oscatter.segment_sum(C.torch.from_numpy(ties), C.torch.from_numpy(c["inv"].copy()), c["m"]).numpy()
    assert (per[long_rows[:, 0]] >= 10).all()  # every column of a long segment attains its maximum ten times or more


def test_exact_families_keep_every_partial_sum_below_two_to_the_24():
    worst = 0.0
    for name in C.NAMES:
        if C.SPECS[name][3] in C.EXACT_SUM_FAMILIES:
            c = C.case(name)
            assert np.abs(c["feat"]).max(initial=0) <= 8 and (c["feat"] == np.round(c["feat"])).all()
            worst = max(worst, 8.0 * c["lengths"].max(initial=0))  # |any partial sum, in any order| <= 8 * rows of the segment
    assert 8.0 * 8193 <= worst < 2.0 ** 24


def test_derived_bounds_are_what_the_doc_says():
    assert C.gamma(0) == 0 and abs(C.gamma(5999) / (5999 * C.U) - 1) < 1e-3
    c = C.case(C.find(layout="mixed_frame", family="normal")[0])
    one = c["lengths"] == 1
    assert (c["sum_bound"][one] == 0).all() and (c["sum_bound"][c["lengths"] > 1] > 0).all()  # a one-row sum is exact
    s = 100 + C.LONG_GRID_X
    assert (c["sum_bound"][s] < 6000 * C.U * 1.001 * np.abs(c["feat"].astype(np.float64)[c["inv"] == s]).sum(0)).all()


# ---- a numpy model of the chunked algorithm, with switchable defects --------------------------------------------------------------

DEFECTS = ("ge_in_short_fixup", "long_fold_without_index", "which_inverted_for_whole_chunk_head", "rule_off_by_one",
           "mean_by_piece_length", "dead_slot_folded", "last_chunk_hi", "empty_unwritten")
INT32_MAX = 2 ** 31 - 1


def model(c, defect=None):
    """dict(sum, mean, max f32 [m, ch], arg i64 [m, ch]) as csrc/segment.hip computes them: the chunk pass writes whole segments and
    parks the head piece of a straddler in slot 1 and every later piece in slot 0 of its chunk; the short fix-up folds spans of 1..16 in
    chunk order; the long fold gives partial p to team p % nteams, UNR at a time, and folds the teams in order.  What no pass writes
    stays NaN / -7."""
    assert defect is None or defect in DEFECTS
    n, m, inv, w = c["n"], c["m"], c["inv"], c["width"]
    ch, K = w.c, C.SEG_CHUNK
    off = C.offsets(c["lengths"])
    out = {k: np.full((m, ch), np.nan, F32) for k in ("sum", "mean", "max")}
    arg = np.full((m, ch), -7, np.int64)
    nch = -(-n // K)
    ps, pm, pa = np.full((nch, 2, ch), np.nan, F32), np.full((nch, 2, ch), np.nan, F32), np.full((nch, 2, ch), -9, np.int64)
    if n:  # chunk pass: a piece is a run of one segment's rows within one chunk
        order = np.argsort(inv, kind="stable")
        x, seg, pos = c["feat"][order], inv[order], np.arange(n)
        brk = (pos % K == 0) | np.r_[True, seg[1:] != seg[:-1]]
        starts = np.nonzero(brk)[0]
        ends = np.r_[starts[1:], n]
        pid = np.cumsum(brk) - 1
        psum = np.add.reduceat(x, starts, axis=0)
        pmax = np.maximum.reduceat(x, starts, axis=0)
        first = np.minimum.reduceat(np.where(x == pmax[pid], pos[:, None], n), starts, axis=0)  # strict >: the first of the maxima
        parg = order[first]
        pseg, pchunk = seg[starts], starts // K
        S, E = off[pseg], off[pseg + 1]
        chunk_end = np.minimum((pchunk + 1) * K, n)
        hi = (pchunk + 1) * K if defect == "last_chunk_hi" else chunk_end
        flush_hi = np.where(ends == chunk_end, hi, ends)  # the last piece of a chunk is flushed with the chunk's `hi`
        whole = (starts == S) & (flush_hi == E)
        which = np.where(S < starts, 0, 1)
        if defect == "which_inverted_for_whole_chunk_head":
            which = np.where((S == starts) & (starts % K == 0) & (ends - starts == K) & ~whole, 0, which)
        out["sum"][pseg[whole]] = psum[whole]
        out["mean"][pseg[whole]] = psum[whole] / (E - S)[whole].astype(F32)[:, None]
        out["max"][pseg[whole]], arg[pseg[whole]] = pmax[whole], parg[whole]
        ps[pchunk[~whole], which[~whole]] = psum[~whole]
        pm[pchunk[~whole], which[~whole]], pa[pchunk[~whole], which[~whole]] = pmax[~whole], parg[~whole]
    empty = c["lengths"] == 0
    if defect != "empty_unwritten":
        for k in out:
            out[k][empty] = 0
        arg[empty] = n
    nteams = C.long_fold_shape(ch, w.vec)[3]
    sweep = nteams * C.UNR
    long_from = C.SEG_LONG_SPAN + (2 if defect == "rule_off_by_one" else 1)

    def fold_max(acc, a, v, va, tie):
        take = (v > acc) | ((v == acc) & (va < a)) if tie else (v > acc)
        return np.where(take, v, acc), np.where(take, va, a)

    for s in np.nonzero(~empty)[0]:
        cs, ce = int(off[s] // K), int((off[s + 1] - 1) // K)
        span = ce - cs
        if span == 0:
            continue
        cnt = F32(off[s + 1] - ce * K) if defect == "mean_by_piece_length" else F32(off[s + 1] - off[s])
        if span <= C.SEG_LONG_SPAN:
            a_s, a_m, a_a = ps[cs, 1], pm[cs, 1], pa[cs, 1]
            for cc in range(cs + 1, ce + 1):
                a_s = a_s + ps[cc, 0]
                v = pm[cc, 0]
                take = (v >= a_m) if defect == "ge_in_short_fixup" else (v > a_m)
                a_m, a_a = np.where(take, v, a_m), np.where(take, pa[cc, 0], a_a)
        elif span >= long_from:
            P = span + 1
            vs = np.concatenate([ps[cs:cs + 1, 1], ps[cs + 1:ce + 1, 0]])  # virtual partial p: slot 1 of cs, then slot 0 of cs + p
            vm = np.concatenate([pm[cs:cs + 1, 1], pm[cs + 1:ce + 1, 0]])
            va = np.concatenate([pa[cs:cs + 1, 1], pa[cs + 1:ce + 1, 0]])
            tie = defect != "long_fold_without_index"
            teams = []
            for t in range(nteams):
                t_s, t_m, t_a = np.zeros(ch, F32), np.full(ch, -np.inf, F32), np.full(ch, INT32_MAX, np.int64)
                for p0 in range(t, P, sweep):
                    for u in range(C.UNR):
                        p = p0 + u * nteams
                        if p >= P:
                            if defect != "dead_slot_folded":
                                continue
                            p = p0  # (the kernel loads partial p0 again into a dead slot, to stay in bounds)
                        t_s = t_s + vs[p]
                        t_m, t_a = fold_max(t_m, t_a, vm[p], va[p], tie)
                teams.append((t_s, t_m, t_a))
            a_s, a_m, a_a = teams[0]
            for t_s, t_m, t_a in teams[1:]:
                a_s = a_s + t_s
                a_m, a_a = fold_max(a_m, a_a, t_m, t_a, tie)
        else:
            continue  # folded by neither pass
        out["sum"][s], out["mean"][s], out["max"][s], arg[s] = a_s, a_s / cnt, a_m, a_a
    out["arg"] = arg
    return out


def disagreements(c, got):
    """The outputs of `got` that are not the referee's by the case's own rule."""
    bad = []
    if not (np.array_equal(got["max"], c["want_max"]) and np.array_equal(got["arg"], c["want_arg"])):
        bad.append("max")
    if c["family"] != "inf":
        for mode in ("sum", "mean"):
            try:
                C.check_sum(c, mode, got[mode])
            except AssertionError:
                bad.append(mode)
    return bad


@pytest.mark.parametrize("name", C.NAMES)
def test_model_without_defect_equals_the_referee(name):
    c = C.case(name)
    got = model(c)
    np.testing.assert_array_equal(got["max"], c["want_max"])
    np.testing.assert_array_equal(got["arg"], c["want_arg"])
    if c["family"] != "inf":
        C.check_sum(c, "sum", got["sum"])
        C.check_sum(c, "mean", got["mean"])


# one case per defect that tells the defective kernel from the right one, and the output it shows in
WITNESS = {
    "ge_in_short_fixup": ("straddle-c4-identity-relu_like", "max"),               # a later chunk's equal maximum wins: a larger index
    "long_fold_without_index": ("single_545-c131-identity-ints", "max"),          # team 1's partial 1 loses to team 0's partial 4
    "which_inverted_for_whole_chunk_head": ("straddle-c128-identity-ints", "sum"),  # the fix-up reads a slot nobody wrote
    "rule_off_by_one": ("single_545-c4-identity-ints", "sum"),                    # the span of 17 is never written
    "mean_by_piece_length": ("straddle-c5-shuffled-ints", "mean"),
    "dead_slot_folded": ("single_545-c5-identity-relu_like", "sum"),              # 18 partials, 32 teams: partial p0 counted four times
    "last_chunk_hi": ("single_31-c5-identity-ints", "max"),                       # a whole segment that ends at n is parked, not written
    "empty_unwritten": ("empty_ends-c4-identity-ints", "max"),
}


@pytest.mark.parametrize("defect", DEFECTS)
def test_each_defect_is_caught_by_its_named_case(defect):
    name, where = WITNESS[defect]
    c = C.case(name)
    assert disagreements(c, model(c)) == []
    assert where in disagreements(c, model(c, defect)), (defect, name)


def test_defects_are_caught_widely():
    """Not one lucky case: every defect shows in several cases, the tie defects in every exact family that has straddlers."""
    names = [n for n in C.NAMES if C.SPECS[n][0] in ("straddle", "span_edges", "empty_ends", "single_31", "single_545") and
             C.SPECS[n][1] in C.CORE_WIDTHS]
    caught = {d: 0 for d in DEFECTS}
    for n in names:
        c = C.case(n)
        for d in DEFECTS:
            caught[d] += bool(disagreements(c, model(c, d)))
    print(caught)
    assert all(v >= 3 for v in caught.values()), caught
