"""Segment layouts for the segmented reductions (K4-K6, fullysparsefusion_amd/csrc/segment.hip) and the segment plan
(fsf_segment_plan_from_inverse, csrc/unique.hip) that reach the kernels' decisions one by one, and the referee they are judged by:
shared by tests/test_segment_cases_cpu.py (the source pin, the path witnesses, the referee against a plain loop, a numpy model of the
chunked algorithm with switchable defects) and tests/test_segment_gpu.py.  No GPU and no product import here.

A case is a list of segment lengths in segment-id order (0 = an id no row carries), a row order (identity: the rows already lie in
segment order; shuffled: a seeded permutation of them, so that `order` is a real permutation), a width class (channels, and the view
of a wider buffer the rows are handed over in) and a value family.  Its name is `layout-width-order-family`.

Referee: `oracle.scatter.segment_max` as it is (first index among the maxima, empty -> (0, n)); float64 `oracle.scatter.segment_sum`;
the mean is the exact sum divided in fp32, np.float32(sum) / np.float32(cnt), the IEEE division `__fdiv_rn` performs.

Value families and how they are judged
* ints       integers uniform in [-8, 8] without 0.  Every fp32 sum of at most 2^24 / 8 such rows is exact in ANY order, so sum and mean
             are compared bit for bit: one dropped, doubled or misplaced row changes the result.  Maxima tie massively.
* relu_like  `ints` clamped at 0, a quarter of the (segment, channel) columns entirely 0 whatever the segment's length: the post-ReLU
             features the SIR blocks reduce, where the maximum of a column is attained by every row.
* inf        `ints` with some (segment, channel) columns entirely -inf (out = -inf, arg = the segment's smallest row), one +inf and
             one -inf first row followed by finite rows.  Max only.
* normal     standard_normal * exp(standard_normal) per row.  Max is exact; a sum of L fp32 terms in any order obeys
             |err| <= gamma(L - 1) * sum |x_i|, gamma(k) = k u / (1 - k u), u = 2^-24 (Higham, Accuracy and Stability of Numerical
             Algorithms, §4.2), judged per element; the mean the same bound divided by L plus u |mean| for the division.
NaN features are out of scope (the passes treat them differently; see docs/kernels/K03_K08_unique_segment_rulebook.md).

Cases are generated from their names, built one at a time (`case(name)`, a small cache) and must not be written to."""
import functools
import zlib
from typing import NamedTuple

import numpy as np
import torch

from oracle import scatter as oscatter

# restated from csrc/segment.hip and csrc/radix_sort.h (pinned by test_segment_cases_cpu.py::test_constants_and_rules_equal_the_kernel_source)
SEG_CHUNK = 32       # rows of the sorted list one lane team walks
SEG_LONG_SPAN = 16   # a segment with ce - cs above this is folded by a whole workgroup
SEG_BLOCK = 256
SEG_MIN_TEAM = 4
UNR = 4              # partials a team of the long fold requests before it folds the first
SEG_SHORT_MAX = 8    # tensors of one fsf_segment_reduce_short launch
RS_TILE = 2048       # keys per workgroup of the one-sweep radix sort
LONG_GRID_X = 1024   # workgroups (x) of the long fold: segment s is folded by workgroup s % min(m, 1024)

F32 = np.float32
U = 2.0 ** -24


def pick_team(c, vec):
    """Lanes per team of the chunk pass and the short fix-up."""
    groups = (c + vec - 1) // vec
    t = SEG_MIN_TEAM
    while t < groups and t < 64:
        t <<= 1
    return t


def grid_y(c, vec):
    """Channel slices (gridDim.y) of the long fold."""
    groups = (c + vec - 1) // vec
    return (4 if groups >= 32 else (2 if groups >= 16 else 1)) if vec == 4 else 1


def long_fold_shape(c, vec):
    """(slices, channels per slice, lanes per team, teams) of the long fold."""
    gy = grid_y(c, vec)
    csl = (c + gy * vec - 1) // (gy * vec) * vec
    team = SEG_MIN_TEAM
    while team * vec < csl and team < 64:
        team <<= 1
    return gy, csl, team, SEG_BLOCK // team


def has_long_launch(n):
    return n > SEG_LONG_SPAN * SEG_CHUNK


# ---- width classes ---------------------------------------------------------------------------------------------------------------

class Width(NamedTuple):
    name: str
    c: int      # channels
    buf: int    # columns of the row-major buffer the feature is a column slice of (= the row stride in floats)
    off: int    # first column of the slice

    @property
    def vec(self):
        """4 where fsf_segment_reduce takes the float4 form (the buffer itself is allocator-aligned), else 1."""
        return 4 if self.c % 4 == 0 and self.buf % 4 == 0 and self.off % 4 == 0 else 1


VEC4_CHANNELS = (4, 16, 20, 32, 64, 68, 128, 256, 260)
VEC1_CHANNELS = (1, 3, 5, 131)
WIDTHS = {f"c{c}": Width(f"c{c}", c, c, 0) for c in VEC4_CHANNELS + VEC1_CHANNELS}
WIDTHS["v72_4"] = Width("v72_4", 64, 72, 4)   # [n, 72][:, 4:68]: aligned, strided, float4
WIDTHS["v68_1"] = Width("v68_1", 64, 68, 1)   # [n, 68][:, 1:65]: pointer 4 bytes off, scalar
WIDTHS["v66_0"] = Width("v66_0", 64, 66, 0)   # [n, 66][:, :64]: row stride no multiple of 4, scalar
CORE_WIDTHS = ("c4", "c5", "c128", "c131")
POISON = F32(1e30)  # what the columns of the buffer outside the slice hold


def feature_buffer(c):
    """float32 [n, buf] whose columns off .. off + c hold the case's features and every other column POISON."""
    w = c["width"]
    buf = np.full((c["n"], w.buf), POISON, F32)
    buf[:, w.off:w.off + w.c] = c["feat"]
    return buf


# ---- path model ------------------------------------------------------------------------------------------------------------------

FULL_TAGS = frozenset({
    "whole_in_chunk", "whole_aligned_chunk", "head_whole_chunk", "tail_on_boundary", "tail_whole_head_chunk",
    "short_span_1", "short_span_2", "short_span_15", "short_span_16", "long_span_17", "long_span_18",
    "long_idle_teams", "long_dead_slot", "long_second_sweep", "grid_y_1", "grid_y_2", "grid_y_4", "uneven_slice",
    "chan_loop_vec1", "chan_loop_vec4", "no_long_launch", "long_launch_no_long_segment", "two_long_one_workgroup",
    "empty_first", "empty_last", "empty_run", "partial_last_chunk", "no_rows"})


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]).astype(np.int64)


def paths(lengths, n, c, vec):
    """The set of path tags fsf_segment_reduce reaches on segments of these lengths over n rows of c channels in the `vec` form: a
    function of S, E, cs = S // 32, ce = (E - 1) // 32 of every segment and of the launch rules restated above."""
    lengths = np.asarray(lengths, np.int64)
    off = offsets(lengths)
    assert off[-1] == n
    m = lengths.size
    tags = set()
    if n == 0:
        tags.add("no_rows")
    if n % SEG_CHUNK:
        tags.add("partial_last_chunk")
    empty = lengths == 0
    if m and empty[0]:
        tags.add("empty_first")
    if m and empty[-1]:
        tags.add("empty_last")
    if (empty[1:] & empty[:-1]).any():
        tags.add("empty_run")
    if pick_team(c, vec) * vec < c:
        tags.add(f"chan_loop_vec{vec}")  # the chunk pass and the short fix-up take more than one trip over the channels
    gy, csl, _, nteams = long_fold_shape(c, vec)
    sweep = nteams * UNR
    heads, tails, wholes, long_ids = set(), set(), set(), []
    for s in np.nonzero(~empty)[0]:
        S, E = int(off[s]), int(off[s + 1])
        cs, ce = S // SEG_CHUNK, (E - 1) // SEG_CHUNK
        span = ce - cs
        if span == 0:
            tags.add("whole_in_chunk")
            wholes.add(cs)
            if S % SEG_CHUNK == 0 and E - S == SEG_CHUNK:
                tags.add("whole_aligned_chunk")
            continue
        heads.add(cs)
        tails.add(ce)
        if S % SEG_CHUNK == 0:
            tags.add("head_whole_chunk")  # the head piece is a whole chunk: it still goes to slot 1
        if E % SEG_CHUNK == 0:
            tags.add("tail_on_boundary")
        if span <= SEG_LONG_SPAN:
            tags.add(f"short_span_{span}" if span in (1, 2, SEG_LONG_SPAN - 1, SEG_LONG_SPAN) else "short_span_mid")
            continue
        tags.add(f"long_span_{span}" if span <= SEG_LONG_SPAN + 2 else "long_span_more")
        long_ids.append(int(s))
        P = span + 1  # partials: the head piece and slot 0 of every later chunk
        if P < nteams:
            tags.add("long_idle_teams")  # teams without a partial fold the identity (-inf, INT32_MAX)
        if P > sweep:
            tags.add("long_second_sweep")
        if any(p0 % sweep < nteams and p0 + (UNR - 1) * nteams >= P for p0 in range(P)):
            tags.add("long_dead_slot")  # a trip whose later unroll slots lie past the last partial
        tags.add(f"grid_y_{gy}")
        if gy > 1 and c - (gy - 1) * csl != csl:
            tags.add("uneven_slice")
    if heads & tails & wholes:
        tags.add("tail_whole_head_chunk")
    if not has_long_launch(n):
        assert not long_ids
        tags.add("no_long_launch")  # seg_fixup_kernel
    elif not long_ids:
        tags.add("long_launch_no_long_segment")
    gx = max(1, min(m, LONG_GRID_X))
    if len({s % gx for s in long_ids}) < len(long_ids):
        tags.add("two_long_one_workgroup")
    return tags


# ---- layout families -------------------------------------------------------------------------------------------------------------

def inside():
    """Every segment within one chunk; n = 640 (a multiple of 32, and above 512: the long launch without a long segment)."""
    chunks = [[32], [1] * 32, [5, 7, 20], [32], [16, 16], [31, 1], [1, 30, 1], [10, 10, 10, 2], [32], [3] * 10 + [2]]
    assert all(sum(ch) == SEG_CHUNK for ch in chunks)
    return [v for ch in chunks * 2 for v in ch]


def straddle():
    """Span-1 segments of each kind (S .. E): 20..44 both pieces partial; 64..104 from a boundary; 110..160 to a boundary; 160..224
    two whole chunks; chunk 8 = rows 256..288 holds the tail of 240..266, the whole 266..276 and the head of 276..300; the last
    segment 310..333 ends in a partial last chunk."""
    return [20, 24, 20, 40, 6, 50, 64, 16, 26, 10, 24, 10, 23]


def span_edges():
    """ce - cs of 16 (514 rows from S % 32 == 0), 17 (514 rows from S % 32 == 31), 16 (544 aligned), 17 (545 aligned), 2, 15, 18; the
    short ones in between set the starts."""
    return [514, 29, 514, 31, 544, 545, 70, 25, 481, 5, 582, 3]


SINGLE_SIZES = (1, 31, 32, 33, 512, 513, 545, 8193)

# (tag, partial count P of the one long segment as a function of (nteams, sweep)); a count a long segment cannot have is left out
SWEEP_KINDS = (("idle", lambda t, w: t - 3), ("teams+1", lambda t, w: t + 1), ("sweep-1", lambda t, w: w - 1), ("sweep", lambda t, w: w),
               ("sweep+1", lambda t, w: w + 1), ("2sweep+3", lambda t, w: 2 * w + 3))
SWEEP_WIDTHS = ("c4", "c64", "c128", "c256", "c131")
MIN_LONG_PARTIALS = SEG_LONG_SPAN + 2


def sweep_partials(width, kind):
    """P of the kind at this width.  Where a whole sweep is shorter than the shortest long segment (c = 131: 16 partials), the same
    edge is taken whole sweeps later, where a long segment can have it."""
    w = WIDTHS[width]
    _, _, _, nteams = long_fold_shape(w.c, w.vec)
    sweep = nteams * UNR
    P = dict(SWEEP_KINDS)[kind](nteams, sweep)
    while sweep < MIN_LONG_PARTIALS and P < MIN_LONG_PARTIALS:
        P += sweep
    return P


def long_sweeps(width, kind):
    """[5, L, 3]: one long segment from row 5 whose last row lies in chunk P - 1, so that it has exactly P partials."""
    P = sweep_partials(width, kind)
    assert P >= MIN_LONG_PARTIALS
    return [5, (P - 1) * SEG_CHUNK + 9 - 5, 3]


MIXED_LONG = {100: 3000, 100 + LONG_GRID_X: 6000, 2000: 600}
MIXED_M = 2300


def mixed_frame():
    """What a frame looks like: ~2 000 voxels of 1..5 rows, 24 segments of 40..500 rows, long segments of 600, 3 000 and 6 000 rows (two
    of them at ids k and k + 1024, which one workgroup of the long fold takes), every 11th remaining id empty; m = 2 300."""
    rng = np.random.default_rng([4, 7])
    lengths = rng.integers(1, 6, MIXED_M)
    lengths[5::11] = 0
    lengths[[0, MIXED_M - 1]] = 2
    free = [s for s in range(1, MIXED_M - 1) if s % 11 != 5 and s not in MIXED_LONG]
    lengths[rng.permutation(free)[:24]] = rng.integers(40, 501, 24)
    for s, v in MIXED_LONG.items():
        lengths[s] = v
    return lengths.tolist()


def empty_ends():
    return [0, 0, 0, 5, 0, 40, 0, 0, 7, 33, 0, 0]


LAYOUTS = {"inside": inside, "straddle": straddle, "span_edges": span_edges, "mixed_frame": mixed_frame, "empty_ends": empty_ends,
           "empty_n0": lambda: [0, 0, 0]}
for _n in SINGLE_SIZES:
    LAYOUTS[f"single_{_n}"] = functools.partial(lambda n: [n], _n)
CROSS_LAYOUTS = tuple(LAYOUTS)        # every one of these at every core width, in both row orders
ALL_WIDTH_LAYOUTS = ("span_edges", "mixed_frame")  # and these at every other width too
for _w in SWEEP_WIDTHS:
    _seen = set()
    for _k, _ in SWEEP_KINDS:
        _p = sweep_partials(_w, _k)
        if _p >= MIN_LONG_PARTIALS and _p not in _seen:  # (a count a long segment cannot have, or has under another kind, is left out)
            _seen.add(_p)
            LAYOUTS[f"long_sweeps_{_w}_{_k}"] = functools.partial(long_sweeps, _w, _k)

FAMILIES = ("ints", "relu_like", "inf", "normal")
EXACT_SUM_FAMILIES = ("ints", "relu_like")
ORDERS = ("identity", "shuffled")


def _specs():
    """name -> (layout, width, order, family).  The family rotates with the layout, the width and the order, so that every layout sees
    all four families, each in a float4 and in a scalar width."""
    out = {}

    def add(layout, width, order, k):
        if order == "shuffled" and sum(LAYOUTS[layout]()) <= 1:
            return  # (no rows, or one: nothing to permute)
        fam = FAMILIES[k % 4]
        out[f"{layout}-{width}-{order}-{fam}"] = (layout, width, order, fam)

    for li, layout in enumerate(CROSS_LAYOUTS):
        for wi, width in enumerate(CORE_WIDTHS):
            for oi, order in enumerate(ORDERS):
                add(layout, width, order, li + wi + 2 * oi + (wi // 2))
    others = [w for w in WIDTHS if w not in CORE_WIDTHS]
    for li, layout in enumerate(ALL_WIDTH_LAYOUTS):
        for wi, width in enumerate(others):
            add(layout, width, ORDERS[(wi + li) % 2], wi + li)
    for wi, width in enumerate(SWEEP_WIDTHS):
        ki = 0
        for kind, _ in SWEEP_KINDS:
            if f"long_sweeps_{width}_{kind}" in LAYOUTS:
                add(f"long_sweeps_{width}_{kind}", width, ORDERS[(ki // 2 + wi) % 2], ki + wi)
                ki += 1
    return out


SPECS = _specs()
NAMES = tuple(SPECS)
AUTOGRAD_CASE = "mixed_frame-c68-shuffled-relu_like"  # what _SegmentReduce / _GatherRows of ops/sst_ops.py are run on
assert AUTOGRAD_CASE in SPECS


def find(layout=None, width=None, order=None, family=None):
    """The case names whose fields equal the given ones."""
    want = (layout, width, order, family)
    return [n for n, spec in SPECS.items() if all(w is None or w == v for w, v in zip(want, spec))]


def case_paths(name):
    layout, width, _, _ = SPECS[name]
    lengths = LAYOUTS[layout]()
    w = WIDTHS[width]
    return paths(lengths, int(sum(lengths)), w.c, w.vec)


# ---- values ----------------------------------------------------------------------------------------------------------------------

INT_CHOICES = np.array([v for v in range(-8, 9) if v != 0], F32)


def _rng(name, *key):
    return np.random.default_rng([5, zlib.crc32(name.encode()), *key])


def _values(name, family, n, c, inv, lengths):
    """(feat f32 [n, c], marks): marks of the `inf` family = dict(neg_cols [(segment, channel)], neg_first (segment, channel, row) | None,
    pos (row, channel) | None)."""
    rng = _rng(name, 1)
    if family == "normal":
        return (rng.standard_normal((n, c)) * np.exp(rng.standard_normal((n, 1)))).astype(F32), None
    x = INT_CHOICES[rng.integers(0, INT_CHOICES.size, (n, c))]
    if family == "relu_like":
        dead = rng.random((len(lengths), c)) < 0.25  # (segment, channel) columns a ReLU left entirely 0
        return np.where(dead[inv], F32(0), np.maximum(x, F32(0))), None
    if family == "ints":
        return x, None
    marks = dict(neg_cols=[], neg_first=None, pos=None)
    by_length = [int(s) for s in np.argsort(-np.asarray(lengths), kind="stable") if lengths[s] > 0]
    if not by_length:
        return x, marks
    picked = by_length[:1] + [int(s) for s in rng.permutation(by_length[1:])[:3]]  # the longest segment and three others
    for s in picked:
        ch = int(rng.integers(c))
        x[inv == s, ch] = -np.inf
        marks["neg_cols"].append((s, ch))
    used = set(marks["neg_cols"])
    for s in by_length:  # the longest segment with two rows and a free channel: -inf in its FIRST row, finite after
        free = [ch for ch in range(c) if (s, ch) not in used]
        if lengths[s] >= 2 and free:
            row = int(np.nonzero(inv == s)[0][0])
            x[row, free[0]] = -np.inf
            marks["neg_first"] = (s, free[0], row)
            used.add((s, free[0]))
            break
    free = [(r, ch) for r in rng.permutation(n)[:8] for ch in range(c) if (int(inv[r]), ch) not in used]
    if free:
        r, ch = free[0]
        x[r, ch] = np.inf
        marks["pos"] = (int(r), int(ch))
    return x, marks


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


@functools.lru_cache(maxsize=3)
def case(name):
    """dict(name, layout, width, order, family, lengths i64 [m], n, m, inv i64 [n], cnt i64 [m], feat f32 [n, c], marks,
    want_max f32 [m, c], want_arg i64 [m, c], and, but for `inf`: want_sum / want_mean (f32, exact: EXACT_SUM_FAMILIES) or
    sum64 / mean64 with sum_bound / mean_bound (f64 [m, c]: normal))."""
    layout, width, order, family = SPECS[name]
    w = WIDTHS[width]
    lengths = np.asarray(LAYOUTS[layout](), np.int64)
    m, n = int(lengths.size), int(lengths.sum())
    inv = np.repeat(np.arange(m, dtype=np.int64), lengths)
    if order == "shuffled":
        inv = inv[_rng(name, 0).permutation(n)]
    feat, marks = _values(name, family, n, w.c, inv, lengths)
    out = dict(name=name, layout=layout, width=w, order=order, family=family, lengths=lengths, n=n, m=m, inv=inv, cnt=lengths.copy(),
               feat=feat, marks=marks)
    t, ti = torch.from_numpy(feat), torch.from_numpy(inv)
    wmax, warg = oscatter.segment_max(t, ti, m)
    out["want_max"], out["want_arg"] = wmax.numpy(), warg.numpy()
    if family != "inf":
        sum64 = oscatter.segment_sum(t.double(), ti, m).numpy()
        abs64 = oscatter.segment_sum(t.double().abs(), ti, m).numpy()
        div = np.maximum(lengths, 1)[:, None]
        if family in EXACT_SUM_FAMILIES:
            assert abs64.max(initial=0.0) < 2.0 ** 24  # every partial sum in any order is an integer below 2^24: exact in fp32
            out["want_sum"] = sum64.astype(F32)
            out["want_mean"] = out["want_sum"] / div.astype(F32)
        else:
            out["sum64"], out["sum_bound"] = sum64, gamma(np.maximum(lengths - 1, 0))[:, None] * abs64
            out["mean64"] = sum64 / div
            out["mean_bound"] = out["sum_bound"] / div + U * np.abs(out["mean64"])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def check_sum(c, mode, got, cols=None, what=""):
    """`got` f32 [m, len(cols)] against the case's sum / mean of the columns `cols` (all): bit for bit in the exact families, within the
    derived per-element bound in `normal`."""
    sel = slice(None) if cols is None else cols
    if c["family"] in EXACT_SUM_FAMILIES:
        np.testing.assert_array_equal(got, c[f"want_{mode}"][:, sel], err_msg=f"{c['name']} {mode} {what}")
        return
    err = np.abs(got.astype(np.float64) - c[f"{mode}64"][:, sel])
    bound = c[f"{mode}_bound"][:, sel]
    bad = np.argwhere(~(err <= bound))  # (a NaN is past every bound)
    assert bad.size == 0, (f"{c['name']} {mode} {what}: {len(bad)} elements past the summation bound, first (segment, column) "
                           f"{bad[0].tolist()}: |err| {err[tuple(bad[0])]:.3e} > {bound[tuple(bad[0])]:.3e}")


# ---- the tensor lists of fsf_segment_reduce_short ---------------------------------------------------------------------------------
# every tensor is a selection of the case's own columns (column j of tensor t = case column (3 j + t) % c), so that the case's referee,
# taken at the same columns, judges it: the reduction is per column

SHORT_LISTS = {
    "scalar": [Width("s131", 131, 131, 0), Width("s33", 33, 33, 0), Width("s5", 5, 5, 0)],
    "float4": [Width("f64", 64, 64, 0), Width("f128", 128, 128, 0)],
    "eight": [Width(f"e{c}", c, c, 0) for c in (4, 64, 20, 128, 8, 32, 68, 16)],
    "misaligned": [Width("m128", 128, 128, 0), Width("m64", 64, 68, 1), Width("m4", 4, 4, 0)],  # one slice 4 bytes off: all scalar
}
assert all(len(v) <= SEG_SHORT_MAX for v in SHORT_LISTS.values())


def short_list_is_float4(widths):
    return all(w.vec == 4 for w in widths)


def short_columns(c, t, w):
    """The case columns tensor `t` of a list, `w` channels wide, is made of."""
    return (3 * np.arange(w) + t) % c


# ---- plan-only cases -------------------------------------------------------------------------------------------------------------

PLAN_M = (1, 256, 257, 65537)                                   # 0, 1, 2 and 3 passes of the 8-bit radix sort
PLAN_N = (RS_TILE - 1, RS_TILE, RS_TILE + 1, 3 * RS_TILE + 1)   # tile edges of the one-sweep look-back
PLAN_NAMES = tuple(f"plan_bits-m{m}-n{n}" for m in PLAN_M for n in PLAN_N)


def plan_case(name):
    """(inv i64 [n], m): ids drawn only from the top 40 of the range, in random row order."""
    _, m, n = name.split("-")
    m, n = int(m[1:]), int(n[1:])
    return _rng(name).integers(max(0, m - 40), m, n).astype(np.int64), m


def plan_of(inv, m):
    """(order i32 [n], seg_offsets i32 [m + 1], cnt i64 [m]) a segment plan must hold."""
    cnt = np.bincount(inv, minlength=m).astype(np.int64)
    return np.argsort(inv, kind="stable").astype(np.int32), offsets(cnt).astype(np.int32), cnt
