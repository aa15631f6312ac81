"""CPU: what the crafted K22-family cases of tests/linear_cases.py (run on the device by tests/test_linear_gpu.py) stand on.

* The constants and rules `linear_cases.plan` restates are the source's: pinned to its text.
* Every catalogue tag is reached by a named case.
* The exact families are exact under the host models of the operand formats (tests/product_budget.py), and every segment edge of the
  LayerNorm cases carries a witness in the float64 reference.
* A numpy model of the launch — which workgroup takes which row block of which slice, from which block the software pipeline took the
  rows and the addend index, the two clamped 16-byte loads per lane and the zeroed k tail — and of K22s's runs, slots, merge order and
  plain / atomic flushes equals the referee on every case; with each of twelve planted defects it fails a case this module names.
  "Fails" is a wrong value, an output element or a (segment, block) pair written twice or never, a flush of the wrong kind (a segment
  inside one 128-row block must be stored once, one that crosses blocks must go through atomics), or a read out of range (IndexError):
  two of the defects change no value at all, they read past a buffer or write twice.
  One exception is written into the expectation: the segment that holds row n - 1 may take either kind, because the rows past n repeat
  row n - 1 and so keep its run open at the tail when they follow it inside its wave (harmless: seg_out holds -inf on entry)."""
import pathlib
import re

import numpy as np
import pytest

import linear_cases as L
import product_budget as P

SRC = pathlib.Path(__file__).resolve().parents[1] / "fullysparsefusion_amd" / "csrc"
DEFECTS = ("next_block_plus_1", "addend_index_of_current", "k_tail_not_zeroed", "no_clamp", "k22h_decode_swapped", "k22h_idle_reprocess",
           "sid_before_at_row0", "sid_after_unguarded", "head_open_stored", "merge_drops_after_closed", "slots_at_block_start_buf",
           "group_past_n_runs")


class ModelFailure(AssertionError):
    pass


# ---- the launch model ------------------------------------------------------------------------------------------------------------
def workgroups(c, defect=None):
    """[(slice_id, [blocks])] decoded as the kernel does, from blockIdx alone."""
    p = L.plan(c)
    nblk, nslice, gx = p["nblk"], p["nslice"], p["gx"]
    out = []
    if c.entry == "planes":
        for wg in range(gx * nslice):
            q = wg >> 3
            if defect == "k22h_decode_swapped":
                slice_id, first = q // nslice, (q % nslice) * 8 + (wg & 7)
            else:
                slice_id, first = q % nslice, (q // nslice) * 8 + (wg & 7)
            blocks = list(range(first, nblk, gx))
            if not blocks and defect == "k22h_idle_reprocess":
                blocks = [nblk - 1]
            out.append((slice_id, blocks))
    else:
        out = [(s, list(range(bx, nblk, gx))) for s in range(nslice) for bx in range(gx)]
    return out


def launch_model(c, d, defect=None):
    """f32 [n, c] of an exact-family case, NaN where nothing was written."""
    p = L.plan(c)
    n, k, nkc, nslice, sw = c.n, c.k, p["nkc"], p["nslice"], p["slice_w"]
    kp = nkc * L.LNA_KC
    stride = c.x_stride
    flat = d["xbuf"].reshape(-1)
    out = np.full((n, c.c), np.nan, np.float64)
    writes = np.zeros((p["nblk"], nslice), np.int64)
    per_slice = {}
    for s, blocks in workgroups(c, defect):
        if blocks and not 0 <= s < nslice:
            raise ModelFailure("slice %d of %d" % (s, nslice))
        for j, blk in enumerate(blocks):
            xblk = blocks[j - 1] + 1 if (j and defect == "next_block_plus_1") else blk
            ablk = blocks[j - 1] if (j and defect == "addend_index_of_current") else blk
            per_slice.setdefault(s, []).append((blk, xblk, ablk))
    lane = np.arange(L.LNA_ROWS)
    col = np.arange(kp)
    for s, trip in per_slice.items():
        blk, xblk, ablk = (np.array(v, np.int64) for v in zip(*trip))
        np.add.at(writes[:, s], blk, 1)
        rows = (blk[:, None] * L.LNA_ROWS + lane).reshape(-1)
        xrows = np.minimum((xblk[:, None] * L.LNA_ROWS + lane).reshape(-1), n - 1)
        arows = np.minimum((ablk[:, None] * L.LNA_ROWS + lane).reshape(-1), n - 1)
        if c.entry == "planes":  # whole 32-column chunks of the row's planes, no clamp
            x = d["xbuf"][xrows][:, :k]
        else:
            off = s * c.x_slice_off if c.entry == "sliced" else 0
            last_quad = stride - 4 - off
            quad = col // 4 * 4
            q = quad if defect == "no_clamp" else np.minimum(quad, last_quad)
            idx = xrows[:, None] * stride + off + (q + col % 4)[None, :]
            if idx.max() >= flat.size:
                raise IndexError("x read at float %d of %d" % (idx.max(), flat.size))
            x = flat[idx]
            if defect != "k_tail_not_zeroed":
                x[:, k:] = 0.0
        ch = np.arange(s * sw, min((s + 1) * sw, c.c))
        wpad = np.zeros((len(ch), x.shape[1]), L.F32)
        wpad[:, :k] = d["w"][ch]
        if c.family == "ln":
            x, wpad = x.astype(np.float64), wpad.astype(np.float64)
        y = (x @ wpad.T).astype(np.float64)  # (the exact families: exact in fp32 in any order, shown by the exactness tests below)
        if d["bias"] is not None:
            y += d["bias"][ch]
        if d["table"] is not None:
            y += d["table"][d["index"][arows]][:, ch]
        if c.norm == "affine":
            y = y * d["gamma"][ch] + d["beta"][ch]
        elif c.norm == "ln":  # (the LayerNorm cases have one slice; the model's rows are float64 and held to the row tolerance)
            mean = y.mean(1, keepdims=True)
            y = (y - mean) / np.sqrt(((y - mean) ** 2).mean(1, keepdims=True) + L.EPS) * d["gamma"][ch] + d["beta"][ch]
        if c.act == "relu":
            y = np.maximum(y, 0) + 0.0
        elif c.act == "gelu":
            y = 0.5 * y * (1.0 + L.torch.special.erf(L.torch.from_numpy(y / np.sqrt(2.0))).numpy())
        live = rows < n
        out[np.ix_(rows[live], ch)] = y[live]
    if not (writes == 1).all():
        raise ModelFailure("(block, slice) pairs written %s times" % sorted(set(writes.reshape(-1).tolist())))
    return out if c.family == "ln" else out.astype(L.F32)


# ---- the K22s model ----------------------------------------------------------------------------------------------------------------
def seg_model(c, d, rows, defect=None):
    """(seg_out f32 [m, c], flush log [(sid, blk, kind)]) from the rows [n, c] the call returns."""
    ids, m, n = d["ids"], d["m"], c.n
    p = L.plan(c)
    order = {}  # block -> (its position in its workgroup's sequence, whether a block follows)
    for _, blocks in p["wgs"]:
        for j, b in enumerate(blocks):
            order[b] = (j, j + 1 < len(blocks))
    seg_out = np.full((m, c.c), -np.inf, L.F32)
    log = []
    for blk, runs in L.seg_blocks(ids, n, defect):
        j, has_next = order[blk]
        buf_last = p["buf0"](j) ^ ((p["nkc"] - 1) & 1)          # the buffer the last chunk was read from: free after the loop
        slot_buf = p["buf0"](j) if defect == "slots_at_block_start_buf" else buf_last
        clobbered = has_next and slot_buf != buf_last             # the other buffer is receiving the next block's first weights
        mx = [rows[a:b + 1].max(0) for a, b, _, _, _ in runs]
        for sid, kind, idxs in L.seg_merge(runs, defect):
            v = np.maximum.reduce([mx[i] for i in idxs])
            if clobbered and runs[idxs[0]][4] >= 0:
                v = np.full_like(v, np.nan)
            seg_out[sid] = v if kind == "store" else np.fmax(seg_out[sid], v) if not np.isnan(v).any() else v
            log.append((sid, blk, kind))
    return seg_out, log


def check_seg(c, d, rows, defect=None):
    ids, n = d["ids"], c.n
    got, log = seg_model(c, d, rows, defect)
    want = L.segment_max(rows, ids, d["m"])
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        raise ModelFailure("segment maxima differ in segments %s" % np.flatnonzero((got != want).any(1))[:8].tolist())
    starts = np.flatnonzero(np.r_[True, ids[1:] != ids[:-1]])
    ends = np.r_[starts[1:] - 1, n - 1]
    expect = {}
    for a, b in zip(starts.tolist(), ends.tolist()):
        for blk in range(a // L.LNA_ROWS, b // L.LNA_ROWS + 1):
            kind = "atomic" if a // L.LNA_ROWS != b // L.LNA_ROWS else ("any" if b == n - 1 else "store")
            expect[(int(ids[a]), blk)] = kind
    seen = {}
    for sid, blk, kind in log:
        if (sid, blk) in seen:
            raise ModelFailure("segment %d flushed twice by block %d" % (sid, blk))
        seen[(sid, blk)] = kind
    if set(seen) != set(expect):
        raise ModelFailure("flushes missing or unexpected: %s" % sorted(set(seen) ^ set(expect))[:6])
    bad = [(key, seen[key]) for key in expect if expect[key] not in ("any", seen[key])]
    if bad:
        raise ModelFailure("wrong kind of flush: %s" % bad[:6])


def run_model(name, defect=None):
    d = L.case(name)
    c = d["case"]
    if c.entry == "segmax":
        check_seg(c, d, d["want"].astype(L.F32), defect)
    else:
        got = launch_model(c, d, defect)
        if c.family == "ln":
            assert L.check_rows(name, got, d["want"], d["tol"]) < 1e-3
        elif not np.array_equal(got.view(np.uint32), d["want"].view(np.uint32)):
            bad = np.argwhere(got.view(np.uint32) != d["want"].view(np.uint32))
            raise ModelFailure("%d elements differ, first %s" % (len(bad), bad[0].tolist()))


BIG = "n%d" % L.N1
# defect -> the cases it must fail on (and why)
CAUGHT_ON = {
    "next_block_plus_1": ("plain-bf16x6-%s-k32-c36-affine-relu-ints" % BIG,          # workgroup 0's second block is 768, not 1
                          "planes-f16x3-n%d-k32-c816-affine-relu-ints" % L.N_K22H12),
    "addend_index_of_current": ("grouped-f16x3-%s-k32-c36-affine-relu-ints" % BIG,
                                "grouped-f16x3-n%d-k32-c68-affine-relu-ints" % L.N2),
    "k_tail_not_zeroed": ("plain-bf16x6-n129-k33-c36-affine-relu-ints", "sliced-bf16x6-n129-k33-c48-affine-relu-ints-s16o0"),
    "no_clamp": ("plain-bf16x6-n385-k33-c68-affine-none-ints-pad0", "plain-bf16x6-n385-k1-c68-affine-none-ints-pad0"),
    "k22h_decode_swapped": ("planes-f16x3-n1025-k64-c204-affine-relu-ints",),       # 2 lanes of 8, 3 slices: slice 2 is never written
    "k22h_idle_reprocess": ("planes-f16x3-n256-k64-c204-affine-relu-ints", "planes-f16x3-n1025-k64-c204-affine-relu-ints"),
    "sid_before_at_row0": ("segmax-bf16x6-n385-k64-c36-ln-gelu-ln-edges",),          # the segment that starts at row 256 goes atomic
    "sid_after_unguarded": ("segmax-bf16x6-n384-k64-c36-ln-gelu-ln-edges", "segmax-bf16x6-n352-k64-c36-ln-gelu-ln-mixed"),    # the last wave ends at n
    "head_open_stored": ("segmax-bf16x6-n385-k64-c36-ln-gelu-ln-edges", "segmax-f16x3-n385-k96-c68-ln-relu-ln-two_open"),
    "merge_drops_after_closed": ("segmax-bf16x6-n385-k64-c36-ln-relu-ln-edges", "segmax-bf16x6-n320-k33-c36-ln-gelu-ln-mixed"),
    "slots_at_block_start_buf": ("segmax-bf16x6-%s-k64-c36-ln-gelu-ln-runs" % BIG,),  # nkc = 2: the block's first buffer takes the DMA
    "group_past_n_runs": ("segmax-bf16x6-n352-k64-c36-ln-gelu-ln-mixed", "segmax-bf16x6-n320-k33-c36-ln-gelu-ln-mixed"),
}
NOT_CAUGHT_ON = {"slots_at_block_start_buf": "segmax-bf16x6-%s-k96-c36-ln-gelu-ln-long" % BIG}  # odd nkc: the same buffer


@pytest.mark.parametrize("name", L.NAMES)
def test_model_equals_the_referee(name):
    run_model(name)
    d = L.case(name)
    c = d["case"]
    assert workgroups(c) == L.plan(c)["wgs"]
    assert np.isnan(d["xbuf"][:, c.in_cols:]).all() and np.isfinite(d["xbuf"][:, :c.in_cols]).all()
    if c.pad == 0:
        assert c.x_stride == L.cdiv(c.in_cols, 4) * 4
    if c.entry == "segmax":
        ids = d["ids"]
        assert (np.diff(ids) >= 0).all() and ids.min() >= 1 and ids.max() == d["m"] - 2 and len(ids) == c.n


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_planted_defect_fails_its_named_cases(defect):
    assert set(CAUGHT_ON) == set(DEFECTS)
    for name in CAUGHT_ON[defect]:
        run_model(name)
        with pytest.raises((ModelFailure, IndexError)):
            run_model(name, defect)
    if defect in NOT_CAUGHT_ON:
        run_model(NOT_CAUGHT_ON[defect], defect)


def test_every_tag_is_reached():
    reached = {}
    for name in L.NAMES:
        for t in L.paths(L.SPECS[name]):
            reached.setdefault(t, name)
    assert L.FULL_TAGS <= set(reached), sorted(L.FULL_TAGS - set(reached))
    # the multi-block sizes are the smallest the grid cap allows: one row more than the cap's blocks
    assert (L.N1, L.N2, L.N_C260, L.N_SLICED6, L.N_K22H12) == (98305, 196737, 32769, 16385, 8193)
    for name in L.NAMES:
        c = L.SPECS[name]
        p = L.plan(c)
        counts = [len(b) for _, b in p["wgs"]]
        if c.n == L.N1:
            assert sorted(set(counts)) == [1, 2] and counts.count(2) == 1 and L.is_multi_block(c)
        if c.n == L.N2:
            assert sorted(set(counts)) == [2, 3] and counts.count(3) == 2 and p["wgs"][1][1][-1] * L.LNA_ROWS == c.n - 1
        if c.n in (L.N_C260, L.N_SLICED6, L.N_K22H12):
            assert max(counts) == 2 and counts.count(2) == p["nslice"] and p["nslice"] in (3, 6, 12)
        if L.is_multi_block(c):
            assert [p["buf0"](j) for j in range(3)] == ([0, 1, 0] if p["nkc"] % 2 else [0, 0, 0])
        assert c.n <= 385 or L.is_multi_block(c) or c.entry == "planes", name
        assert c.k <= 96
    # every variant takes more than one block per workgroup, with both buffer parities; K22h leaves workgroups idle
    for v in L.VARIANT_TAGS:
        tags = set().union(*(L.paths(c) for c in L.SPECS.values() if L.variant_tag(c) == v and L.is_multi_block(c)))
        assert "blocks_per_wg_2" in tags, v
        if not v.startswith("k22s_f16") and v != "sliced":
            assert {"odd_nkc_multi_block", "even_nkc_multi_block"} <= tags, v
        if v in ("k22_t2", "k22_t4", "k22_t8", "k22f_t4", "k22f_t8") or (v.startswith("k22s_t")):
            assert {"blocks_per_wg_3plus", "uneven_blocks"} <= tags, v
    p = L.plan(L.SPECS["planes-f16x3-n256-k64-c204-affine-relu-ints"])
    assert (p["gx"], p["nblk"], p["nwg"]) == (8, 2, 24) and sum(1 for _, b in p["wgs"] if not b) == 18
    p = L.plan(L.SPECS["planes-f16x3-n1025-k64-c204-affine-relu-ints"])
    assert (p["gx"], p["nblk"]) == (16, 9) and sum(1 for _, b in p["wgs"] if not b) == 21
    # tags that name one decision each
    edges = L.paths(L.SPECS["segmax-bf16x6-n385-k64-c36-ln-gelu-ln-edges"])
    assert {"run_closed", "run_head_open", "run_tail_open", "run_both_open", "segment_of_one_row", "crosses_group", "crosses_wave",
            "crosses_block", "ends_at_block_edge", "starts_at_block_edge", "empty_segment_first", "empty_segment_middle",
            "empty_segment_last", "negative_max_across_blocks", "group_past_n", "multi_seg_group", "one_seg_group"} <= edges
    assert "block_inside_one_segment" in L.paths(L.SPECS["segmax-bf16x6-n385-k64-c36-ln-gelu-ln-inside"])
    assert "two_open_segments_in_a_block" in L.paths(L.SPECS["segmax-bf16x6-n385-k64-c36-ln-gelu-ln-two_open"])
    assert "crosses_a_workgroups_consecutive_blocks" in L.paths(L.SPECS["segmax-bf16x6-%s-k32-c36-ln-gelu-ln-long" % BIG])
    assert "last_run_ends_at_n" in L.paths(L.SPECS["segmax-bf16x6-n384-k64-c36-ln-gelu-ln-edges"])


def test_every_k22s_variant_meets_every_run_tag():
    for v in [t for t in L.VARIANT_TAGS if t.startswith("k22s")]:
        tags = set().union(*(L.paths(c) for c in L.SPECS.values() if L.variant_tag(c) == v))
        want = set(L.RUN_TAGS) - {"last_run_ends_at_n", "segment_of_one_row"}
        if v.endswith("relu"):
            want -= {"negative_max_across_blocks", "mixed_sign_across_blocks"}
        assert want <= tags, (v, sorted(want - tags))


def test_the_restated_launch_is_the_source():
    h = (SRC / "linear_norm_act.h").read_text()
    s = (SRC / "linear_norm_act.hip").read_text()
    for text, value in (("constexpr int LNA_KC = ", L.LNA_KC), ("constexpr int LNA_NW = ", L.LNA_NW), ("constexpr int LNA_RG = ", L.LNA_RG),
                        ("#define LNA_WPS ", L.LNA_WPS), ("#define LNA_SEG_WPS ", L.LNA_SEG_WPS)):
        assert re.search(re.escape(text) + r"(\d+)\b", h).group(1) == str(value), text
    assert "constexpr int LNA_ROWS = LNA_NW * LNA_RG * 16;" in h and L.LNA_ROWS == 128
    for line in ("const int t = (c + 15) / 16;", "return t <= 2 ? 2 : (t <= 4 ? 4 : 8);", "static int lna_slices(int c) { return (c + 127) / 128; }",
                 "const int T = lna_tiles(a.slice_w < a.c ? a.slice_w : a.c);", "const int64_t nblk = (a.n + LNA_ROWS - 1) / LNA_ROWS;",
                 "int64_t gx = (256 * (a.seg_out ? LNA_SEG_WPS : LNA_WPS) + nslice - 1) / nslice;", "if (gx > nblk) gx = nblk;",
                 "gx = (gx + 7) / 8 * 8;", "dim3((unsigned)(gx * nslice))", "const dim3 grid((unsigned)gx, (unsigned)nslice);",
                 "const int wg = (int)blockIdx.x, q = wg >> 3;", "slice_id = q % nslice;", "blk_first = (int64_t)(q / nslice) * 8 + (wg & 7);",
                 "blk_step = gridDim.x / nslice;", "int64_t blk_first = blockIdx.x, blk_step = gridDim.x;",
                 "for (int64_t blk = blk_first; blk < nblk; blk += blk_step) {", "for (int kc = 0; kc < nkc; ++kc, buf ^= 1) {",
                 "else if (blk + blk_step < nblk) {", "float* slots = reinterpret_cast<float*>(wbuf + (buf ^ 1) * CHUNK_U4);",
                 "const int last_quad = XP ? 0 : (int)a.x_stride - 4 - (int)((int64_t)slice_id * a.x_slice_off);",
                 "const float4 p = *reinterpret_cast<const float4*>(xrow[rg] + min(kq, last_quad));",
                 "if (kc * LNA_KC + 8 * grp + e >= a.k) xc[rg][e] = 0.0f;",
                 "sb.sid_before = row0 > 0 ? (int)a.seg_ids[row0 - 1 < a.n ? row0 - 1 : a.n - 1] : -1;",
                 "sb.sid_after = row0 + 16 * LNA_RG < a.n ? (int)a.seg_ids[row0 + 16 * LNA_RG] : -1;",
                 "if (xf && (c <= 32 || ((uintptr_t)planes % 16) != 0)) return FSF_ERR_UNSUPPORTED;",
                 "if (norm != 1 || act == 0 || c > 128 || c <= 32 ||",
                 "if ((k % 32) != 0 || slice_c > 128 || slice_c <= 64 ||"):
        assert line in s, line
    for line in ("if (grow0 < a.n && (rowl == 15 || dn1 != sid)) {", "const int slot = 2 * g + (head_open ? 0 : 1);",
                 "const bool head_open = sid == first && above == first, tail_open = sid == last && below == last;",
                 "if (complete && !(tag & LNA_SLOT_HEAD_OPEN)) *p = v;", "if (!(ss & LNA_SLOT_TAIL_OPEN)) {",
                 "if (cs >= 0) flush(cs, cv, false);  // continues below this block"):
        assert line in h, line
    assert L.lna_tiles(32) == 2 and L.lna_tiles(36) == 4 and L.lna_tiles(64) == 4 and L.lna_tiles(68) == 8 and L.lna_tiles(4) == 2


SMALL_EXACT = [n for n in L.NAMES if L.SPECS[n].family in L.EXACT_FAMILIES and L.SPECS[n].n <= 1152] + \
    ["grouped-f16x3-%s-k96-c68-affine-relu-ints" % BIG]


@pytest.mark.parametrize("name", SMALL_EXACT)
def test_exact_families_are_exact_under_the_format_models(name):
    d = L.case(name)
    c = d["case"]
    x, w = np.ascontiguousarray(d["xbuf"][:, :c.in_cols]), d["w"]
    if c.family == "ints":
        for a in (x, w, d["bias"], d["table"], d["beta"]):
            assert a is None or (a == np.round(a)).all()
        if d["gamma"] is not None:
            assert (np.frexp(d["gamma"])[0] == 0.5).all() and d["gamma"].min() >= 0.25 and d["gamma"].max() <= 4
        # every partial sum in any order is an integer below 2^24 (a quarter of it under the smallest gamma)
        xs = [L.slice_inputs(c, d, s) for s in range(c.nslice)] if c.entry == "sliced" else [x]
        bound = max(float((np.abs(v.astype(np.float64)) @ np.abs(w.astype(np.float64)).T).max()) for v in xs) + 8 + 8 + 3
        assert 4 * bound < 2 ** 24
        hi, mid, lo = P.split_bf16(x)
        assert (hi == x).all() and not mid.any() and not lo.any()
        hi, mid, lo = P.split_bf16(w)
        assert (hi == w).all() and not mid.any() and not lo.any()
        for rule in ("row_running", "row"):  # K22f's running scale; K22h's row scale
            xh, xl = P.split_f16(x, P.x_scales(x, rule))
            assert (xh == x).all() and not xl.any(), rule
        wh, wl = P.split_f16(w, P.pick_scale(np.abs(w).max()))
        assert (wh == w).all() and not wl.any()
        if c.xkind == "scales" and c.k > L.LNA_KC:
            s = P.x_scales(x, "row_running")
            assert (s[1::4, 0] > s[1::4, -1]).all() and not x[2::4, :L.LNA_KC].any() and x[2::4, L.LNA_KC:].any() and not x[3::8].any()
            assert (s[0::4, 0] == s[0::4, -1]).mean() > 0.5
    else:
        assert c.fmt == "bf16x6" and (np.count_nonzero(w, axis=1) <= 1).all()
        nz = w[w != 0]
        assert (np.frexp(np.abs(nz))[0] == 0.5).all() and np.abs(np.log2(np.abs(nz))).max() <= 12
        assert (x.view(np.uint32) & 0xFF).astype(bool).mean() > 0.9  # the lo piece is live
        if c.entry == "plain":  # the six-term arithmetic re-assembles every product; without a cross term it does not
            prod = P.linear_product(x, w)
            want = np.maximum(prod.want(), 0) + 0.0 if c.act == "relu" else prod.want()
            emu = lambda drop: np.maximum(P.emulate_bf16(prod, 3, drop), 0) + 0.0 if c.act == "relu" else P.emulate_bf16(prod, 3, drop)  # noqa: E731
            assert np.array_equal(emu(None).astype(L.F32), d["want"]) and np.array_equal(want.astype(L.F32), d["want"])
            for drop in ((1, 0), (2, 0)):
                assert not np.array_equal(emu(drop).astype(L.F32), d["want"]), drop


LN_SMALL = [n for n in L.NAMES if L.SPECS[n].entry == "segmax" and L.SPECS[n].n <= 385]
LN_BIG = ["segmax-bf16x6-%s-k32-c36-ln-gelu-ln-long" % BIG, "segmax-bf16x6-n%d-k32-c68-ln-relu-ln-long" % L.N2]


@pytest.mark.parametrize("name", LN_SMALL + LN_BIG)
def test_every_segment_edge_carries_a_witness(name):
    d = L.case(name)
    c = d["case"]
    assert L.witness_margin(c, d, d["want"], d["tol"]) > 100.0
    if c.act == "gelu":  # the channels that make a maximum negative, and of both signs, across a block edge
        want, ids = d["want"], d["ids"]
        assert (want[:, L.NEG_CHANNELS] < 0).all()
        blk = np.arange(c.n) // L.LNA_ROWS
        cross = [s for s in np.unique(ids) if len(set(blk[ids == s].tolist())) > 1][:4]
        assert bool(cross) == ("crosses_block" in L.paths(c))
        mixed = False  # (a part that holds the segment's first row is positive in channel 20, every other part negative)
        for s in cross:
            parts = np.stack([want[(ids == s) & (blk == b)][:, L.MIXED_CHANNELS].max(0) for b in sorted(set(blk[ids == s].tolist()))[:3]])
            mixed |= bool(((parts.max(0) > 0) & (parts.min(0) < 0)).any())
        assert mixed == bool(cross)
    e32 = (d["tol"] / 2.0).max()
    assert 0 < e32 < 1e-4


def test_stale_runs_use_other_values():
    names = [n for n in L.NAMES if L.needs_stale_run(L.SPECS[n])]
    assert set(L.find(entry="segmax")) <= set(names) and len(names) >= 60
    c = L.SPECS["segmax-bf16x6-n385-k64-c36-ln-gelu-ln-edges"]
    a, b = L.operands(c), L.operands(c, key=7)
    assert (a["xbuf"][:, :c.k] != b["xbuf"][:, :c.k]).mean() > 0.9 and (a["w"] != b["w"]).mean() > 0.9
    assert np.array_equal(a["ids"], b["ids"])
