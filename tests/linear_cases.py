"""Layouts for the K22 Linear family (K22, K22f, K22s, K22h and the sliced entry: fullysparsefusion_amd/csrc/linear_norm_act.hip and
linear_norm_act.h) that reach the kernels' decisions one by one, and the referees they are judged by: shared by
tests/test_linear_cases_cpu.py (the path witnesses, a numpy model of the launch and of the K22s run / slot / merge logic with switchable
defects) and tests/test_linear_gpu.py.  No GPU and no product import here; torch is used on the host only, for erf and for the fp32
reference whose own error sets the LayerNorm tolerance.

  out = act(norm(x @ W^T + bias [+ table[index]]))            seg_out[s] = max over the rows of segment s of out   (K22s)

A case is (entry, fmt, n, k, c, slice_c, nslice, x_slice_off, norm, act, bias, addend, ids_layout, family) and two layout fields: `pad`
(floats of NaN behind the last 4-column quad of a row: 0 = the last row's last quad is the buffer's last 16 bytes) and `xkind`.

Entries   plain | grouped (a per-row addend) -> K22 (fmt bf16x6) or K22f (fmt f16x3); segmax -> K22s; sliced; planes -> K22h.

Value families and how they are judged — no tensor-wide tolerance anywhere
* ints      x, W, bias and the addend table are integers in [-8, 8]; with xkind `scales` row 4 i + 1 holds +-2^(4 j) in k chunk j (K22f's
            scale falls from chunk to chunk and the accumulators are rescaled), row 4 i + 2 starts with a chunk of zeros, row 8 i + 3 is
            zero.  norm none, or affine with gamma a power of two and beta an integer; act none or ReLU.  Every partial sum in any order
            is an integer below 2^24 times one power of two: exact in fp32, through the bf16 split (hi is the whole value), through the
            f16 hi | lo split under a power-of-two scale and through K22f's rescale.  Bit for bit against the int64 referee.
* one_hot   bf16x6 only.  W rows are +-2^t e_j (t in -12 .. 12, j = channel % k), x holds full 24-bit significands: every output is ONE
            product, exact through hi + mid + lo.  In the grouped form every fourth weight row is zero and the addend table is non-zero
            in those channels only: the output there is the gathered addend's bit pattern.
* ln        LayerNorm + ReLU / GELU (every segmax case, one per K22 / K22f variant).  Each ROW is held to
            |got - want| <= max(2 err32_row, 2e-6 max |want_row|) against float64, err32_row = the distance of torch's fp32 host
            computation from float64 on that row.  The K22s maxima are compared bit for bit with the maxima of the rows the same call
            returned.  The weight's first min(k, c) columns are a scaled identity: a row with one large input has one dominant channel,
            and the first and last row of every segment carry one (channels 4 (s % 3) and 4 (s % 3) + 1 of segment s), so that a
            row lost from or added to a segment at an edge changes the float64 maximum (`witness_margin`).

Which decisions a case reaches is computed by `paths(case)` from `plan(case)`, which restates the launch, and for K22s from
`seg_blocks`, which restates lna_seg_prepare and lna_seg_merge.  Arrays handed out by `case()` must not be written to."""
import functools
import zlib
from typing import NamedTuple

import numpy as np
import torch

F32 = np.float32
# linear_norm_act.h
LNA_KC, LNA_NW, LNA_RG, LNA_WPS, LNA_SEG_WPS = 32, 4, 2, 3, 3
LNA_ROWS = LNA_NW * LNA_RG * 16
CUS = 256
EPS = 1e-3
HEAD_OPEN, TAIL_OPEN = 1, 2


def cdiv(a, b):
    return -(-a // b)


def lna_tiles(c):
    t = cdiv(c, 16)
    return 2 if t <= 2 else (4 if t <= 4 else 8)


def lna_slices(c):
    return cdiv(c, 128)


class Case(NamedTuple):
    name: str
    entry: str
    fmt: str
    n: int
    k: int
    c: int
    slice_c: int
    nslice: int
    x_slice_off: int
    norm: str
    act: str
    bias: bool
    addend: str          # "" | "one_row" | "repeat" | "perm"
    ids_layout: str      # "" for every entry but segmax
    family: str
    pad: int = 4
    xkind: str = "plain"

    @property
    def in_cols(self):
        return (self.nslice - 1) * self.x_slice_off + self.k if self.entry == "sliced" else self.k

    @property
    def x_stride(self):
        return cdiv(self.in_cols, 4) * 4 + self.pad


# ---- the launch ------------------------------------------------------------------------------------------------------------------
def plan(c):
    """dict: T, nslice, slice_w, nkc, nblk, gx, nwg, and per workgroup `wgs` = [(slice_id, [blocks])]; `buf0(j)` = the LDS buffer the
    j-th block of a workgroup starts on."""
    if c.entry == "sliced":
        slice_w, nslice = c.slice_c, c.nslice
    elif c.entry == "planes":
        slice_w, nslice = c.slice_c, cdiv(c.c, c.slice_c)
    else:
        slice_w, nslice = 128, (1 if c.entry == "segmax" else lna_slices(c.c))
    T = lna_tiles(min(slice_w, c.c))
    nblk = cdiv(c.n, LNA_ROWS)
    wps = LNA_SEG_WPS if c.entry == "segmax" else LNA_WPS
    gx = min(cdiv(CUS * wps, nslice), nblk)
    wgs = []
    if c.entry == "planes":
        gx = cdiv(gx, 8) * 8
        for wg in range(gx * nslice):
            q = wg >> 3
            wgs.append((q % nslice, list(range((q // nslice) * 8 + (wg & 7), nblk, gx))))
    else:
        for s in range(nslice):
            for bx in range(gx):
                wgs.append((s, list(range(bx, nblk, gx))))
    nkc = cdiv(c.k, LNA_KC)
    return dict(T=T, nslice=nslice, slice_w=slice_w, nkc=nkc, nblk=nblk, gx=gx, nwg=len(wgs), wgs=wgs, buf0=lambda j: (j * nkc) & 1)


# ---- K22s: runs, slots, merge ------------------------------------------------------------------------------------------------------
def seg_blocks(ids, n, defect=None):
    """lna_seg_prepare per 128-row block: [(blk, [run])], run = (first row, last row, sid, flags, slot | -1) with rows clipped to n - 1,
    flags = HEAD_OPEN | TAIL_OPEN, slot = 2 g + (0 if head-open else 1) for an open run of group g.  Raises IndexError where a planted
    defect reads seg_ids out of range."""
    ids = np.asarray(ids)

    def at(r):
        if not 0 <= r < n:
            raise IndexError("seg_ids[%d] of %d" % (r, n))
        return int(ids[r])

    out = []
    for blk in range(cdiv(n, LNA_ROWS)):
        runs = []
        for g in range(LNA_NW * LNA_RG):
            grow0 = blk * LNA_ROWS + 16 * g
            if grow0 >= n and defect != "group_past_n_runs":
                continue
            wave, rg = divmod(g, LNA_RG)
            row0 = blk * LNA_ROWS + 16 * LNA_RG * wave
            sid = ids[np.minimum(grow0 + np.arange(16), n - 1)]
            if rg == 0:
                rb = row0 if defect == "sid_before_at_row0" else row0 - 1
                above = at(min(rb, n - 1)) if row0 > 0 else -1
            else:
                above = at(min(grow0 - 1, n - 1))
            if rg == LNA_RG - 1:
                ra = row0 + 16 * LNA_RG
                below = at(ra) if (ra < n or defect == "sid_after_unguarded") else -1
            else:
                below = at(min(grow0 + 16, n - 1))
            first, last = int(sid[0]), int(sid[15])
            ends = [l for l in range(16) if l == 15 or sid[l + 1] != sid[l]]
            start = 0
            for l in ends:
                s = int(sid[l])
                fl = (HEAD_OPEN if s == first and above == first else 0) | (TAIL_OPEN if s == last and below == last else 0)
                slot = -1 if fl == 0 else 2 * g + (0 if fl & HEAD_OPEN else 1)
                runs.append((min(grow0 + start, n - 1), min(grow0 + l, n - 1), s, fl, slot))
                start = l + 1
        out.append((blk, runs))
    return out


def seg_merge(runs, defect=None):
    """lna_seg_merge over one block's runs: the flushes [(sid, kind, [run indices])] in order, kind "store" | "atomic"; closed runs come
    first, as the stores the epilogue issues itself."""
    flushes = [(r[2], "store", [i]) for i, r in enumerate(runs) if r[4] < 0]
    slots = {r[4]: i for i, r in enumerate(runs) if r[4] >= 0}
    cs, chain, skip = None, [], False
    for s in range(16):
        if s not in slots:
            continue
        if skip:
            skip = False
            continue
        i = slots[s]
        _, _, sid, fl, _ = runs[i]
        if cs is not None and cs[0] == sid:
            chain.append(i)
        else:
            if cs is not None:
                flushes.append((cs[0], "atomic", chain))
            cs, chain = (sid, bool(fl & HEAD_OPEN)), [i]
        if not fl & TAIL_OPEN:
            flushes.append((cs[0], "atomic" if cs[1] and defect != "head_open_stored" else "store", chain))
            cs, chain = None, []
            skip = defect == "merge_drops_after_closed"
    if cs is not None:
        flushes.append((cs[0], "atomic", chain))
    return flushes


# ---- ids layouts ---------------------------------------------------------------------------------------------------------------
def _ids_from_starts(n, starts, skip_ids=()):
    """Segment j begins at starts[j]; the ids ascend and leave out `skip_ids` (empty segments), and id 0, and one id past the last."""
    starts = sorted(set(s for s in starts if 0 <= s < n) | {0})
    pos = np.zeros(n, np.int64)
    pos[starts] = 1
    j = np.cumsum(pos) - 1
    avail = np.array([v for v in range(1, len(starts) + len(skip_ids) + 2) if v not in skip_ids][:len(starts)], np.int64)
    return avail[j], int(avail[-1]) + 2


def ids_layout(layout, n):
    """(ids i64 [n] nondecreasing, m): m - 1 and m - 2 are unused ids (so is 0 and, in `edges`, a middle one)."""
    if layout == "edges":      # n = 385: runs at every 16 / 32 / 128 edge
        return _ids_from_starts(n, [0, 1, 5, 16, 24, 40, 100, 140, 256, 300, 330, 331, 384], skip_ids=(4,))
    if layout == "inside":     # block 1 lies inside one segment; the segment before it ends at 99
        return _ids_from_starts(n, [0, 3, 100, 300, 380])
    if layout == "two_open":   # block 1 holds the end of one open segment and the beginning of the next
        return _ids_from_starts(n, [0, 120, 200, 300])
    if layout == "singles":
        return _ids_from_starts(n, range(n))
    if layout == "one":
        return _ids_from_starts(n, [0])
    if layout == "mixed":      # short runs of 1 .. 40 rows, seeded
        rng = np.random.default_rng(n)
        return _ids_from_starts(n, np.cumsum(rng.integers(1, 41, n // 8 + 2)).tolist(), skip_ids=(7,))
    if layout == "runs":       # multi-block sizes: runs of 1 .. 300 rows over everything, seeded
        rng = np.random.default_rng(n)
        return _ids_from_starts(n, np.cumsum(rng.integers(1, 301, n // 100)).tolist(), skip_ids=(3,))
    if layout == "long":       # multi-block sizes: one segment that spans more row blocks than the grid has workgroups
        if n <= N1:            # (one block more than the grid: the segment must hold rows of block 0 and the last row)
            return _ids_from_starts(n, [0, 3, 40, 100], skip_ids=(3,))
        rng = np.random.default_rng(n)
        head = np.cumsum(rng.integers(1, 301, 600))
        tail = n - 1 - np.cumsum(rng.integers(1, 150, 8))
        return _ids_from_starts(n, [0] + head[head < 60000].tolist() + [60100] + tail.tolist() + [n - 1], skip_ids=(3,))
    raise ValueError(layout)


@functools.lru_cache(maxsize=None)
def _ids_cached(layout, n):
    ids, m = ids_layout(layout, n)
    ids.setflags(write=False)
    return ids, m


@functools.lru_cache(maxsize=None)
def _seg_cached(layout, n):
    return seg_blocks(_ids_cached(layout, n)[0], n)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
N1, N2 = CUS * LNA_WPS * LNA_ROWS + 1, 2 * CUS * LNA_WPS * LNA_ROWS + LNA_ROWS + 1   # 98 305, 196 737
N_C260 = cdiv(CUS * LNA_WPS, 3) * LNA_ROWS + 1                                        # 32 769
N_SLICED6 = cdiv(CUS * LNA_WPS, 6) * LNA_ROWS + 1                                      # 16 385
N_K22H12 = cdiv(CUS * LNA_WPS, 12) * LNA_ROWS + 1                                      # 8 193


def _specs():
    out = {}

    def add(entry, fmt, n, k, c, family, norm="none", act="none", bias=False, addend="", ids="", slice_c=128, nslice=1, off=0, pad=4,
            xkind="plain", tag=""):
        if entry == "planes":
            nslice = cdiv(c, slice_c)
        elif entry != "sliced":
            nslice = 1 if entry == "segmax" else lna_slices(c)
        name = "-".join(str(v) for v in (entry, fmt, "n%d" % n, "k%d" % k, "c%d" % c, norm, act, family, tag) if v != "")
        assert name not in out, name
        out[name] = Case(name, entry, fmt, n, k, c, slice_c, nslice, off, norm, act, bias, addend, ids, family, pad, xkind)

    # rows: 1 .. 129 rows on the 4-tile K22 (k = 33: two chunks, a k tail, NaN in the row's padding)
    for n in (1, 15, 16, 17, 127, 128, 129):
        add("plain", "bf16x6", n, 33, 36, "ints", "affine", "relu", True)
    # widths (k = 63); 44 = 12 channels in the last tile
    for c in (4, 32, 36, 44, 64, 68, 128, 132, 260):
        add("plain", "bf16x6", 129, 63, c, "ints", "affine" if c % 8 else "none", "relu" if c % 3 else "none", c != 64, pad=0 if c in (4, 68) else 4)
    # k: 1 and 3 with and without floats behind the row; one, two, three chunks
    for k, pad in ((1, 0), (1, 4), (3, 0), (3, 4), (32, 4), (64, 0), (96, 4), (33, 0)):
        add("plain", "bf16x6", 385, k, 68, "ints", "affine", "none", True, pad=pad, tag="pad%d" % pad)
    # addend: one-row table, a repeating index, a permutation, on a partial tile
    for kind in ("one_row", "repeat", "perm"):
        add("grouped", "bf16x6", 129, 33, 36, "ints", "affine", "relu", True, addend=kind, tag=kind)
        add("grouped", "f16x3", 129, 96, 36, "ints", "none", "relu", False, addend=kind, xkind="scales", tag=kind)
    # K22f: both tile counts, the row scales (xkind scales: falling, zero first chunk, zero row, constant), with and without an addend
    for c in (36, 68, 132):
        add("plain", "f16x3", 385, 96, c, "ints", "affine", "relu", True, xkind="scales")
        add("plain", "f16x3", 129, 33, c, "ints", "none", "none", True, pad=0)
    add("grouped", "f16x3", 385, 64, 68, "ints", "affine", "none", True, addend="repeat", xkind="scales")
    add("plain", "bf16x6", 385, 96, 68, "ints", "none", "none", False, xkind="scales")
    # sliced: slice widths 16, 20, 64, 128; shared and shifted inputs
    for sc, ns, k, off, pad in ((16, 3, 33, 0, 4), (20, 3, 33, 36, 0), (64, 2, 63, 64, 4), (128, 2, 32, 32, 0), (16, 6, 3, 4, 0)):
        add("sliced", "bf16x6", 129, k, ns * sc, "ints", "affine", "relu", True, slice_c=sc, nslice=ns, off=off, pad=pad, tag="s%do%d" % (sc, off))
    # K22h: slice widths 68 and 128; two and nine row blocks (idle workgroups), one block and a row
    for n in (129, 256, 1025):
        add("planes", "f16x3", n, 64, 204, "ints", "affine", "relu", True, slice_c=68)
    add("planes", "f16x3", 129, 96, 256, "ints", "none", "none", True, slice_c=128, xkind="scales")
    add("planes", "f16x3", 1152, 32, 128, "ints", "none", "relu", False, slice_c=128)
    # one product per output
    for c in (36, 68, 260):
        add("plain", "bf16x6", 129, 63, c, "one_hot", "none", "relu" if c == 68 else "none", pad=0 if c == 36 else 4)
    add("grouped", "bf16x6", 129, 33, 36, "one_hot", addend="perm")
    add("sliced", "bf16x6", 129, 33, 60, "one_hot", slice_c=20, nslice=3, off=36, tag="s20o36")
    # LayerNorm + GELU on every K22 / K22f variant
    for fmt, c in (("bf16x6", 32), ("bf16x6", 36), ("bf16x6", 68), ("f16x3", 36), ("f16x3", 68)):
        add("plain" if c != 36 else "grouped", fmt, 385, 96, c, "ln", "ln", "gelu", True, addend="repeat" if c == 36 else "")
    # K22s, small: every layout on every variant
    for fmt in ("bf16x6", "f16x3"):
        for c, k in ((36, 64), (68, 96)):
            for act in ("relu", "gelu"):
                for lay, n in (("edges", 385), ("inside", 385), ("two_open", 385)):
                    add("segmax", fmt, n, k, c, "ln", "ln", act, True, ids=lay, tag=lay)
    for lay, n, k, addend in (("singles", 129, 64, ""), ("one", 385, 96, "repeat"), ("mixed", 320, 33, "perm"), ("mixed", 352, 64, ""),
                              ("mixed", 97, 64, ""), ("edges", 384, 64, "")):
        add("segmax", "bf16x6", n, k, 36 if k != 96 else 128, "ln", "ln", "gelu", True, addend=addend, ids=lay, tag=lay, pad=0 if k == 33 else 4)
    # more than one row block per workgroup: the smallest sizes the grid cap allows
    for n, k in ((N1, 32), (N1, 64), (N1, 96), (N2, 32)):
        for c in (32, 36, 68):
            add("plain", "bf16x6", n, k, c, "ints", "affine", "relu", True)
        for c in (36, 68):
            add("grouped", "f16x3", n, k, c, "ints", "affine", "relu", True, addend="repeat", xkind="scales" if k > 32 else "plain")
        for c in (36, 68):
            for act in ("relu", "gelu"):
                lay = "runs" if k == 64 else "long"
                add("segmax", "bf16x6", n, k, c, "ln", "ln", act, True, ids=lay, tag=lay, addend="repeat" if (c, act) == (68, "gelu") else "")
    for c, act in ((36, "gelu"), (68, "relu"), (36, "relu"), (68, "gelu")):
        add("segmax", "f16x3", N1, 64 if act == "gelu" else 96, c, "ln", "ln", act, True, ids="long", tag="long")
    add("plain", "bf16x6", N_C260, 32, 260, "ints", "none", "none", True)
    add("sliced", "bf16x6", N_SLICED6, 33, 96, "ints", "affine", "relu", True, slice_c=16, nslice=6, off=4, tag="s16o4")
    add("planes", "f16x3", N_K22H12, 32, 816, "ints", "affine", "relu", True, slice_c=68)
    add("planes", "f16x3", N_K22H12, 64, 816, "ints", "none", "relu", False, slice_c=68)
    add("planes", "f16x3", N_K22H12, 96, 816, "ints", "none", "none", True, slice_c=68)
    return out


SPECS = _specs()
NAMES = tuple(SPECS)
EXACT_FAMILIES = ("ints", "one_hot")


def find(**kw):
    return [n for n, c in SPECS.items() if all(getattr(c, f) == v for f, v in kw.items())]


def is_multi_block(c):
    return c.n > LNA_ROWS * plan(c)["gx"]


def needs_stale_run(c):
    """The cases before which the same shape is run once with other values."""
    return is_multi_block(c) or c.entry == "segmax"


# refused shapes: (what, why) — each is one FsfHipError with no launch of the family behind it
REFUSALS = ("k22f_c32", "k22s_c32", "k22s_c132", "k22s_affine", "k22s_no_act", "k22h_slice64", "k22h_k40")


# ---- tags ------------------------------------------------------------------------------------------------------------------------
VARIANT_TAGS = ("k22_t2", "k22_t4", "k22_t8", "k22f_t4", "k22f_t8", "k22h", "sliced") + tuple(
    "k22s%s_t%d_%s" % (f, t, a) for f in ("", "_f16") for t in (4, 8) for a in ("relu", "gelu"))
WIDTH_TAGS = tuple("c_%d" % v for v in (4, 32, 36, 64, 68, 128, 132, 260)) + ("partial_quad_tile_4", "partial_quad_tile_12") + tuple(
    "slice_c_%d" % v for v in (16, 20, 64, 128)) + ("k22h_slice_c_68", "k22h_slice_c_128")
K_TAGS = ("k_1", "k_3", "k_lt_4", "k_mod4", "k_tail", "k_33", "k_63", "nkc_1", "nkc_2", "nkc_3", "stride_eq_kpad", "stride_gt_k")
ROW_TAGS = tuple("n_%d" % v for v in (1, 15, 16, 17, 127, 128, 129)) + (
    "tail_block_one_row", "blocks_per_wg_1", "blocks_per_wg_2", "blocks_per_wg_3plus", "uneven_blocks", "odd_nkc_multi_block",
    "even_nkc_multi_block")
GRID_TAGS = ("nslice_gt1_multi_block_plain", "nslice_gt1_multi_block_sliced", "nslice_gt1_multi_block_k22h", "k22h_idle_workgroups_nblk2",
             "k22h_idle_workgroups_nblk9", "k22h_multi_block")
ADDEND_TAGS = ("addend_partial_tile", "addend_one_row", "addend_repeat", "addend_perm", "k22f_addend_cap")
SCALE_TAGS = ("scale_falls", "zero_first_chunk", "zero_row", "scale_constant")
RUN_TAGS = ("run_closed", "run_head_open", "run_tail_open", "run_both_open", "one_seg_group", "multi_seg_group", "segment_of_one_row",
            "crosses_group", "crosses_wave", "crosses_block", "block_inside_one_segment", "two_open_segments_in_a_block",
            "ends_at_block_edge", "starts_at_block_edge", "crosses_a_workgroups_consecutive_blocks", "group_past_n", "last_run_ends_at_n",
            "empty_segment_first", "empty_segment_middle", "empty_segment_last", "negative_max_across_blocks", "mixed_sign_across_blocks",
            "want_rows_false", "seg_out_column_slice")
FULL_TAGS = frozenset(VARIANT_TAGS + WIDTH_TAGS + K_TAGS + ROW_TAGS + GRID_TAGS + ADDEND_TAGS + SCALE_TAGS + RUN_TAGS)
NEG_CHANNELS = slice(16, 20)      # beta = -3, gamma = 1 / 8 under GELU: negative for every row
MIXED_CHANNELS = slice(20, 24)    # beta = -0.4, gamma = 1 / 8: negative but for a segment's first row, which has a large input in column 20


def variant_tag(c):
    T = plan(c)["T"]
    if c.entry == "sliced":
        return "sliced"
    if c.entry == "planes":
        return "k22h"
    if c.entry == "segmax":
        return "k22s%s_t%d_%s" % ("_f16" if c.fmt == "f16x3" else "", T, c.act)
    return "%s_t%d" % ("k22f" if c.fmt == "f16x3" else "k22", T)


def paths(c):
    """The set of tags the launch reaches on this case."""
    p = plan(c)
    tags = {variant_tag(c)}
    if c.entry in ("plain", "grouped", "segmax"):
        tags.add("c_%d" % c.c)
        if c.c % 16 in (4, 12):
            tags.add("partial_quad_tile_%d" % (c.c % 16))
    elif c.entry == "sliced":
        tags.add("slice_c_%d" % c.slice_c)
    else:
        tags.add("k22h_slice_c_%d" % c.slice_c)
    if c.entry != "planes":
        tags.add("k_%d" % c.k)
        if c.k < 4:
            tags.add("k_lt_4")
        if c.k % 4:
            tags.add("k_mod4")
        if c.k % LNA_KC:
            tags.add("k_tail")
        tags.add("stride_eq_kpad" if c.pad == 0 else "stride_gt_k")
    tags.add("nkc_%d" % p["nkc"] if p["nkc"] <= 3 else "nkc_more")
    tags.add("n_%d" % c.n)
    if c.n % LNA_ROWS == 1 and c.n > 1:
        tags.add("tail_block_one_row")
    counts = sorted({len(b) for _, b in p["wgs"]})
    for v in counts:
        if v:
            tags.add("blocks_per_wg_%s" % (v if v < 3 else "3plus"))
    if len([v for v in counts if v]) > 1:
        tags.add("uneven_blocks")
    multi = counts[-1] > 1
    if multi:
        tags.add("odd_nkc_multi_block" if p["nkc"] % 2 else "even_nkc_multi_block")
        if p["nslice"] > 1:
            tags.add("nslice_gt1_multi_block_%s" % {"plain": "plain", "sliced": "sliced", "planes": "k22h"}[c.entry])
    if c.entry == "planes":
        if 0 in counts and p["nblk"] in (2, 9):
            tags.add("k22h_idle_workgroups_nblk%d" % p["nblk"])
        if multi:
            tags.add("k22h_multi_block")
    if c.addend:
        tags.add("addend_%s" % c.addend)
        if c.c % 16:
            tags.add("addend_partial_tile")
        if c.fmt == "f16x3" and c.xkind == "scales":
            tags.add("k22f_addend_cap")  # a row whose first chunk is zero takes the cap as its first scale
    if c.fmt == "f16x3" and c.entry != "planes" and c.xkind == "scales" and c.k > LNA_KC:
        tags.update(SCALE_TAGS)
    if c.entry == "segmax":
        tags |= seg_paths(c)
    return tags


def seg_paths(c):
    ids, m = _ids_cached(c.ids_layout, c.n)
    blocks = _seg_cached(c.ids_layout, c.n)
    n, p = c.n, plan(c)
    tags = {"want_rows_false", "seg_out_column_slice"}
    used = set(np.unique(ids).tolist())
    if 0 not in used:
        tags.add("empty_segment_first")
    if m - 1 not in used:
        tags.add("empty_segment_last")
    if any(v not in used for v in range(int(ids[0]), int(ids[-1]))):
        tags.add("empty_segment_middle")
    if cdiv(n, LNA_ROWS) * LNA_ROWS - n >= 16:
        tags.add("group_past_n")
    if n % 16 == 0:
        tags.add("last_run_ends_at_n")
    starts = np.flatnonzero(np.r_[True, ids[1:] != ids[:-1]])
    ends = np.r_[starts[1:] - 1, n - 1]
    crossing = False
    for a, b in zip(starts.tolist(), ends.tolist()):
        if a == b:
            tags.add("segment_of_one_row")
        if a // 16 != b // 16:
            tags.add("crosses_group")
        if a // 32 != b // 32:
            tags.add("crosses_wave")
        if a // LNA_ROWS != b // LNA_ROWS:
            tags.add("crosses_block")
            crossing = True
            if b // LNA_ROWS - a // LNA_ROWS >= 2:
                tags.add("block_inside_one_segment")
            if b // LNA_ROWS - a // LNA_ROWS >= p["gx"] and p["gx"] < p["nblk"]:
                tags.add("crosses_a_workgroups_consecutive_blocks")
        else:
            if b % LNA_ROWS == LNA_ROWS - 1 and b + 1 < n:
                tags.add("ends_at_block_edge")
            if a % LNA_ROWS == 0 and a > 0:
                tags.add("starts_at_block_edge")
    if crossing and c.act == "gelu":
        tags.update(("negative_max_across_blocks", "mixed_sign_across_blocks"))  # (shown on the reference in the CPU test)
    for blk, runs in blocks:
        open_sids = set()
        per_group = {}
        for a, b, sid, fl, slot in runs:
            tags.add(("run_closed", "run_head_open", "run_tail_open", "run_both_open")[fl])
            per_group[a // 16] = per_group.get(a // 16, 0) + 1
            lo, hi = blk * LNA_ROWS, min((blk + 1) * LNA_ROWS, n) - 1
            if (fl & HEAD_OPEN and a == lo and lo > 0 and ids[lo - 1] == sid) or (fl & TAIL_OPEN and b == hi and hi + 1 < n and ids[hi + 1] == sid):
                open_sids.add(sid)
        for v in per_group.values():
            tags.add("one_seg_group" if v == 1 else "multi_seg_group")
        if len(open_sids) >= 2:
            tags.add("two_open_segments_in_a_block")
    return tags


# ---- values ----------------------------------------------------------------------------------------------------------------------
def _rng(name, *key):
    return np.random.default_rng([22, zlib.crc32(name.encode()), *key])


def _ints(rng, *shape):
    return rng.integers(-8, 9, shape).astype(F32)


def _full(rng, *shape):
    return (rng.standard_normal(shape) * np.exp(rng.standard_normal(shape))).astype(F32)


def operands(c, key=1):
    """dict: xbuf f32 [n, x_stride] (NaN wherever no slice reads), w f32 [c, k], bias, gamma, beta (or None), table f32 [g, c] and index
    i64 [n] (or None), ids i64 [n] and m (segmax).  `key` 1 is the case's own data, any other the values of the stale run."""
    rng = _rng(c.name, key)
    n, k, cc = c.n, c.k, c.c
    d = dict(bias=None, gamma=None, beta=None, table=None, index=None, ids=None, m=0)
    xbuf = np.full((n, c.x_stride), np.nan, F32)
    ch = np.arange(cc)
    if c.family == "ints":
        x = _ints(rng, n, c.in_cols)
        if c.xkind == "scales":
            r = np.arange(n)
            falls = np.sign(x[1::4]) + (x[1::4] == 0)
            x[1::4] = falls * np.exp2(4 * (np.arange(c.in_cols) // LNA_KC))[None, :].astype(F32)
            x[2::4, :LNA_KC] = 0.0
            x[r % 8 == 3] = 0.0
        w = _ints(rng, cc, k)
        if c.bias:
            d["bias"] = _ints(rng, cc)
        if c.norm == "affine":
            d["gamma"], d["beta"] = np.exp2((ch % 5) - 2).astype(F32), ((ch % 7) - 3).astype(F32)
    elif c.family == "one_hot":
        x = _full(rng, n, c.in_cols)
        w = np.zeros((cc, k), F32)
        w[ch, ch % k] = rng.choice([-1.0, 1.0], cc) * np.exp2(rng.integers(-12, 13, cc))
        if c.addend:
            w[3::4] = 0.0
    else:  # ln: a scaled identity in the first min(k, c) columns + small noise; segment-edge rows carry large inputs
        # (bounded noise: no row's normalised value reaches that of a row with a large input, however many rows a segment has)
        x = (rng.uniform(-1.0, 1.0, (n, c.in_cols)) * 0.5 * np.exp(rng.standard_normal((n, 1)) * 0.5)).astype(F32)
        w = (rng.standard_normal((cc, k)) * 0.05).astype(F32)
        dd = min(k, cc)
        w[np.arange(dd), np.arange(dd)] += 2.0
        d["bias"] = (rng.standard_normal(cc) * 0.1).astype(F32) if c.bias else None
        d["gamma"], d["beta"] = (rng.random(cc) * 0.5 + 0.75).astype(F32), (rng.standard_normal(cc) * 0.1).astype(F32)
        if c.act == "gelu":
            d["gamma"][NEG_CHANNELS], d["beta"][NEG_CHANNELS] = 0.125, -3.0
            d["gamma"][MIXED_CHANNELS], d["beta"][MIXED_CHANNELS] = 0.125, -0.4
    if c.entry == "segmax":
        ids, m = _ids_cached(c.ids_layout, n)
        d["ids"], d["m"] = ids, m
        first = np.flatnonzero(np.r_[True, ids[1:] != ids[:-1]])
        last = np.r_[first[1:] - 1, n - 1]
        s = np.arange(len(first))
        amp = (6.0 + (s % 5)).astype(F32) * (1 if key == 1 else -1)
        x[first, 4 * (s % 3)] = amp
        x[last, 4 * (s % 3) + 1] = amp
        x[first, MIXED_CHANNELS.start] = amp
    xbuf[:, :c.in_cols] = x
    if c.addend:
        g = {"one_row": 1, "repeat": 7, "perm": n}[c.addend]
        if c.family == "ints":
            table = _ints(rng, g, cc)
        elif c.family == "one_hot":
            table = np.zeros((g, cc), F32)
            table[:, 3::4] = _full(rng, g, len(ch[3::4]))
        else:
            table = (rng.standard_normal((g, cc)) * 0.2).astype(F32)
        d["table"] = table
        d["index"] = (rng.permutation(n) if c.addend == "perm" else rng.integers(0, g, n)).astype(np.int64)
    d.update(xbuf=xbuf, w=w)
    return d


def slice_inputs(c, d, s):
    """x of slice s, f32 [n, k] (every entry but `sliced` has one input for all slices)."""
    o = s * c.x_slice_off if c.entry == "sliced" else 0
    return d["xbuf"][:, o:o + c.k]


def _epilogue_np(c, d, y, dt):
    """bias / addend / norm / act on y [n, c] in dtype dt (float64 for the referees)."""
    if d["bias"] is not None:
        y = y + d["bias"].astype(dt)
    if d["table"] is not None:
        y = y + d["table"].astype(dt)[d["index"]]
    if c.norm == "affine":
        y = y * d["gamma"].astype(dt) + d["beta"].astype(dt)
    elif c.norm == "ln":
        w = c.slice_c if c.entry == "sliced" else c.c
        yy = y.reshape(y.shape[0], -1, w)
        mean = yy.mean(-1, keepdims=True)
        var = ((yy - mean) ** 2).mean(-1, keepdims=True)
        y = ((yy - mean) / np.sqrt(var + dt(EPS))).reshape(y.shape) * d["gamma"].astype(dt) + d["beta"].astype(dt)
    if c.act == "relu":
        y = np.maximum(y, 0) + 0.0
    elif c.act == "gelu":
        y = 0.5 * y * (1.0 + torch.special.erf(torch.from_numpy(y / np.sqrt(dt(2.0)))).numpy())
    return y


def product64(c, d):
    """x @ W^T in float64, [n, c]; slice s of a sliced case from its own input columns."""
    w = d["w"].astype(np.float64)
    if c.entry != "sliced":
        return d["xbuf"][:, :c.k].astype(np.float64) @ w.T
    return np.concatenate([slice_inputs(c, d, s).astype(np.float64) @ w[s * c.slice_c:(s + 1) * c.slice_c].T for s in range(c.nslice)], 1)


def referee(c, d):
    """f32 [n, c] for the exact families: float64 (int64-exact: every sum is an integer or one product), rounded once, which rounds
    nothing; zeros are +0."""
    want = _epilogue_np(c, d, product64(c, d), np.float64) + 0.0
    out = want.astype(F32)
    assert (out.astype(np.float64) == want).all()
    return out


def reference_ln(c, d):
    """(want f64 [n, c], tol f64 [n]): the float64 rows and the per-row tolerance max(2 err32_row, 2e-6 max |want_row|), err32_row from
    torch's fp32 host computation of the same expression."""
    Fn = torch.nn.functional
    want = _epilogue_np(c, d, product64(c, d), np.float64)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    y = Fn.linear(t(d["xbuf"][:, :c.k]), t(d["w"]), t(d["bias"]))
    if d["table"] is not None:
        y = y + t(d["table"])[t(d["index"])]
    y = Fn.layer_norm(y, (c.c,), t(d["gamma"]), t(d["beta"]), EPS)
    y = Fn.gelu(y) if c.act == "gelu" else Fn.relu(y)
    err32 = np.abs(y.numpy().astype(np.float64) - want).max(1)
    return want, np.maximum(2.0 * err32, 2e-6 * np.abs(want).max(1))


def segment_max(rows, ids, m):
    """f32 [m, c]: the maximum of `rows` over every segment, -inf for an id without rows."""
    out = np.full((m, rows.shape[1]), -np.inf, rows.dtype)
    starts = np.flatnonzero(np.r_[True, ids[1:] != ids[:-1]])
    out[ids[starts]] = np.maximum.reduceat(rows, starts, axis=0)
    return out


def witness_margin(c, d, want, tol):
    """For every segment edge (first row, last row, the row outside either): by how many of that row's tolerances the float64 segment
    maximum changes, in its best channel, when the edge row is dropped from the segment or the outside row is absorbed.  The smallest
    such factor over the case's edges (segments of one row are dropped whole: their maximum becomes -inf)."""
    ids = d["ids"]
    n = c.n
    starts = np.flatnonzero(np.r_[True, ids[1:] != ids[:-1]])
    ends = np.r_[starts[1:] - 1, n - 1]
    worst = np.inf
    for a, b in zip(starts.tolist(), ends.tolist()):
        if b - a > 4096:  # the long segments: the maxima over the interior once, the edges against it
            inner = want[a + 1:b].max(0)
            full = np.maximum(inner, np.maximum(want[a], want[b]))
            drops = ((a, np.maximum(inner, want[b])), (b, np.maximum(inner, want[a])))
        else:
            full = want[a:b + 1].max(0)
            drops = ((a, want[a + 1:b + 1].max(0) if b > a else np.full_like(full, -np.inf)),
                     (b, want[a:b].max(0) if b > a else np.full_like(full, -np.inf)))
        for r, mx in drops:
            worst = min(worst, float(np.abs(full - mx).max() / tol[r]))
        for r in (a - 1, b + 1):
            if 0 <= r < n:
                worst = min(worst, float((np.maximum(full, want[r]) - full).max() / tol[r]))
    return worst


@functools.lru_cache(maxsize=2)
def case(name):
    """dict(case, the operands, want f32 [n, c] (exact families) or want f64 + tol f64 [n] (ln))."""
    c = SPECS[name]
    d = operands(c)
    d["case"] = c
    if c.family in EXACT_FAMILIES:
        d["want"] = referee(c, d)
    else:
        d["want"], d["tol"] = reference_ln(c, d)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def check_exact(name, got, want):
    got = np.ascontiguousarray(got, F32).reshape(want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, ("%s: %d of %d elements differ, first (row, channel) %s: got %r, want %r; row blocks touched %s" % (
        name, len(bad), want.size, bad[0].tolist(), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]),
        sorted(set((bad[:, 0] // LNA_ROWS).tolist()))[:12]))


def check_rows(name, got, want, tol):
    """Every row within its own tolerance; returns the largest err / tolerance."""
    err = np.abs(np.asarray(got, np.float64) - want).max(1)
    ratio = err / tol
    r = int(np.argmax(ratio))
    assert ratio[r] <= 1.0, "%s: row %d (block %d) off by %.3g, %.2f of its tolerance %.3g" % (name, r, r // LNA_ROWS, err[r], ratio[r], tol[r])
    return float(ratio[r])
