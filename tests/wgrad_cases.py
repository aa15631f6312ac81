"""Pair lists for the sparse-convolution weight gradient (K10 / K10p, fullysparsefusion_amd/csrc/spconv_bwd.hip) that reach the
kernels' decisions one by one, and the referee they are judged by: shared by tests/test_wgrad_cases_cpu.py (the path witnesses, a numpy
model of the two-launch algorithm with switchable defects) and tests/test_wgrad_gpu.py.  No GPU and no product import here.

  grad_W[k] = feat[in_k]^T gout[out_k]            over the num[k] pairs (in_k[p], out_k[p]) of offset k

A case is (cin, cout, kvol, cap, num[kvol], m_in, m_out, pattern, family); its name is `list-cinxcout-pattern-family`.

Patterns (how the pair lists are laid out)
* identity   no lists at all: ops.linear_backward_weight, pair p = (row p, row p), kvol = 1, cap = n rows.
* ascending  both lists ascend: num[k] of the cap live rows, drawn without replacement and sorted, each side on its own.
* shuffled   the same draws in random order.
* one_row    every pair of an offset names the SAME input row (one per offset); the output rows are a shuffled draw.
* mixed      rows drawn with replacement from few rows, m_in != m_out.
Every slot at or past num[k] names the POISON row: the last row of feat and of gout, a valid row that holds 2^20 in every channel and
that no live pair names.  A kernel that reads a slot past num[k] changes the result by at least 2^20, and no index is out of range.

Value families and how they are judged — no tensor-wide tolerance anywhere
* ints      both operands uniform in [-8, 8] without 0: a product is at most 64, an offset holds at most 33 280 pairs, so every partial sum
            in ANY order is an integer below 2^22 < 2^24 — exact in fp32, and on the bf16 path too, where the hi piece is the whole value.
            Compared bit for bit with the int64 referee.
* one_hot   the exact case with all three pieces live: one operand holds full 24-bit significands (standard_normal * exp(standard_normal)),
            the rows of the other are +-2^t e_j, t in -12 .. 12, one non-zero channel j = row % channels, and the pairs of an offset name
            every hot channel at most once (num[k] <= min(cin, cout)).  Every element of grad_W[k] is then ONE product x * 2^t plus zeros:
            exact in fp32, and through the split, where lo g + mid g + hi g re-assembles x without a rounding.  Bit for bit, with gout
            (`one_hot`) or feat (`one_hot_t`) as the one-hot operand.  A misplaced piece, k slot or swizzled row is a wrong bit pattern.
A zero of the result is +0 in the referee; the kernels start every sum from +0, so they must produce +0 as well.

Which decisions a case reaches is computed by `paths(case)` from the launch plan (product_budget.wgrad_plan, whose lines
tests/test_product_budget_cpu.py pins to the source text).  Cases are built one at a time (`case(name)`, a small cache) and must not be
written to."""
import functools
import zlib
from typing import NamedTuple, Optional, Tuple

import numpy as np

import product_budget as P

F32 = np.float32
BW_RT = P.BW_RT
POISON = F32(2.0 ** 20)
FOLD_ELEMS = 2048 * 16 * 4   # floats one sweep of the fold covers: fsf_stream_grid caps it at 2048 workgroups of 16 float4
PATTERNS = ("ascending", "shuffled", "one_row", "mixed")
MIXED_ROWS = (301, 517)      # live rows of feat / gout in the `mixed` pattern

SHAPES = ((4, 4), (64, 64), (20, 132), (132, 20), (68, 68), (128, 128), (132, 260))
KERNEL_SHAPE = {"fp32_64x64": (64, 64), "fp32_64x128": (20, 132), "fp32_128x64": (132, 20), "split_128x128": (68, 68)}
LIST_A = (256, (0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 95, 97, 255, 256))
LIST_B = (33280, (0, 1, 256, 257, 4096, 4097, 12288, 12289, 16384, 16385, 28672, 28673, 33280))
# 132 x 260 (six channel tiles, a fold that grid-strides): nsplit = 9, range = 256.  live = 0 .. 9 each at least once, both edges of a
# range (256 | 257, 2048 | 2049), and last stages of 1, 3, 4, 5, 31 and 32 pairs in a LATER split than the first
LIST_C = (2049, (0, 1, 31, 33, 255, 256, 257, 259, 260, 261, 287, 288, 289, 512, 513, 768, 1023, 1025, 1280, 1283, 1536, 1541, 1792,
                 2047, 2048, 2049, 0))
IDENTITY_N = (1, 31, 33, 256, 257, 2049)
ONE_HOT_NUM = (1, 5, 33, 65)
ONE_HOT_CAP = 256


class Case(NamedTuple):
    name: str
    cin: int
    cout: int
    kvol: int
    cap: int
    num: Optional[Tuple[int, ...]]   # None: identity
    m_in: int                        # rows of feat, the poison row included
    m_out: int
    pattern: str
    family: str

    @property
    def counts(self):
        return (self.cap,) if self.num is None else self.num


def _rows(pattern, cap):
    return tuple(r + 1 for r in MIXED_ROWS) if pattern == "mixed" else (cap + 1, cap + 1)


def _specs():
    out = {}

    def add(lst, cin, cout, kvol, cap, num, pattern, family):
        name = "%s-%dx%d-%s-%s" % (lst, cin, cout, pattern, family)
        m_in, m_out = (cap, cap) if pattern == "identity" else _rows(pattern, cap)
        out[name] = Case(name, cin, cout, kvol, cap, None if pattern == "identity" else tuple(num), m_in, m_out, pattern, family)

    for cin, cout in SHAPES:  # list A (nsplit = 1): every pattern on every shape
        for pattern in PATTERNS:
            add("A", cin, cout, len(LIST_A[1]), LIST_A[0], LIST_A[1], pattern, "ints")
    for i, (cin, cout) in enumerate(KERNEL_SHAPE.values()):  # list B (nsplit = 130): one shape per kernel, two patterns each
        for pattern in (PATTERNS[i % 2], PATTERNS[2 + (i // 2 + i) % 2]):
            add("B", cin, cout, len(LIST_B[1]), LIST_B[0], LIST_B[1], pattern, "ints")
    for pattern in ("shuffled", "mixed"):
        add("C", 132, 260, len(LIST_C[1]), LIST_C[0], LIST_C[1], pattern, "ints")
    for cin, cout in SHAPES:
        for n in IDENTITY_N:
            add("I%d" % n, cin, cout, 1, n, None, "identity", "ints")
    for i, (cin, cout) in enumerate(SHAPES):  # num capped by the number of hot channels
        num = tuple(min(v, cin, cout) for v in ONE_HOT_NUM)
        add("H", cin, cout, len(num), ONE_HOT_CAP, num, PATTERNS[i % 4], "one_hot")
        add("H", cin, cout, len(num), ONE_HOT_CAP, num, PATTERNS[(i + 2) % 4], "one_hot_t")
    return out


SPECS = _specs()
NAMES = tuple(SPECS)
EXACT_FAMILIES = ("ints", "one_hot", "one_hot_t")


def find(lst=None, shape=None, pattern=None, family=None):
    """The case names whose fields equal the given ones."""
    return [n for n, c in SPECS.items() if (lst is None or n.split("-")[0] == lst) and (shape is None or (c.cin, c.cout) == tuple(shape))
            and (pattern is None or c.pattern == pattern) and (family is None or c.family == family)]


def needs_stale_workspace(c):
    """The cases before which the same plan is run once with every list full: the dead splits' workspace slices then hold that call's
    non-zero sums (the library's workspace is one grow-only buffer)."""
    return plan(c)[4] > 1 and c.num is not None


# ---- path model ------------------------------------------------------------------------------------------------------------------

KERNEL_TAGS = ("fp32_64x64", "fp32_64x128", "fp32_128x64", "split_128x128")
FULL_TAGS = frozenset(KERNEL_TAGS + (
    "full_tile", "partial_tile_a", "partial_tile_b", "clamped_quad", "multi_tile_a", "multi_tile_b", "tiles_a_ne_tiles_b", "min_width",
    "nsplit_1", "nsplit_gt1", "dead_split", "last_split_one_pair", "empty_offset_nsplit1", "empty_offset_nsplit_gt1", "num_eq_cap",
    "stages_1", "stages_2", "stages_3plus", "full_last_stage", "rem_1", "rem_3", "rem_4", "rem_5", "rem_31",
    "live_1", "live_16", "live_17", "live_48", "live_49", "live_64", "live_65", "live_112", "live_113", "fold_grid_stride"))
LIVE_EDGES = (1, 16, 17, 48, 49, 64, 65, 112, 113)
REM_EDGES = (1, 3, 4, 5, 31)


def cdiv(a, b):
    return -(-a // b)


def plan(c):
    """(ta, tb, tiles_a, tiles_b, nsplit, range) of the case."""
    return P.wgrad_plan(c.cap, c.cin, c.cout, c.kvol)


def kernel_tag(c):
    ta, tb = plan(c)[:2]
    return "split_128x128" if (ta, tb) == (128, 128) else "fp32_%dx%d" % (ta, tb)


def live_splits(c):
    """Per offset, how many of the launched splits hold a pair: cdiv(num, range)."""
    rng = plan(c)[5]
    return [cdiv(n, rng) for n in c.counts]


def paths(c):
    """The set of path tags the two launches reach on this case."""
    ta, tb, tiles_a, tiles_b, nsplit, rng = plan(c)
    tags = {kernel_tag(c)}
    part_a, part_b = c.cin % ta != 0, c.cout % tb != 0
    if not part_a and not part_b:
        tags.add("full_tile")
    if part_a:
        tags.add("partial_tile_a")
    if part_b:
        tags.add("partial_tile_b")
    if part_a or part_b:
        tags.add("clamped_quad")  # channels are multiples of 4: a partial tile leaves whole loader quads past cin / cout
    if tiles_a > 1:
        tags.add("multi_tile_a")
    if tiles_b > 1:
        tags.add("multi_tile_b")
    if tiles_a != tiles_b:
        tags.add("tiles_a_ne_tiles_b")
    if c.cin == c.cout == 4:
        tags.add("min_width")
    tags.add("nsplit_1" if nsplit == 1 else "nsplit_gt1")
    if c.kvol * c.cin * c.cout > FOLD_ELEMS:
        tags.add("fold_grid_stride")
    for n, live in zip(c.counts, live_splits(c)):
        if n == 0:
            tags.add("empty_offset_nsplit1" if nsplit == 1 else "empty_offset_nsplit_gt1")
        if n == c.cap:
            tags.add("num_eq_cap")
        if live < nsplit:
            tags.add("dead_split")
        if nsplit > 1 and live in LIVE_EDGES:
            tags.add("live_%d" % live)
        for s in range(live):
            cnt = min(n, (s + 1) * rng) - s * rng
            if s == live - 1 and cnt == 1 and live > 1:
                tags.add("last_split_one_pair")
            nst = cdiv(cnt, BW_RT)
            tags.add("stages_%s" % (nst if nst < 3 else "3plus"))
            rem = cnt - (nst - 1) * BW_RT
            tags.add("full_last_stage" if rem == BW_RT else ("rem_%d" % rem if rem in REM_EDGES else "rem_other"))
    return tags


# ---- pair lists and values ---------------------------------------------------------------------------------------------------------

INT_CHOICES = np.array([v for v in range(-8, 9) if v != 0], F32)


def _rng(name, *key):
    return np.random.default_rng([10, zlib.crc32(name.encode()), *key])


def _draw(rng, live_rows, n, replace):
    return rng.choice(live_rows, n, replace=replace).astype(np.int32)


def _one_hot_rows(rng, m_live, channels, n):
    """n rows of a one-hot operand with n DIFFERENT hot channels (row r is hot at r % channels)."""
    ch = rng.permutation(min(channels, m_live))[:n]
    reps = np.array([rng.integers(0, cdiv(m_live - c0, channels)) for c0 in ch], np.int64)
    return (ch + reps * channels).astype(np.int32)


def _pairs(c):
    """pairs i32 [kvol, 2, cap]: the live slots by the pattern, every other slot the poison row."""
    pairs = np.empty((c.kvol, 2, c.cap), np.int32)
    pairs[:, 0], pairs[:, 1] = c.m_in - 1, c.m_out - 1
    live_in, live_out = c.m_in - 1, c.m_out - 1
    for k, n in enumerate(c.num):
        rng = _rng(c.name, 2, k)
        if c.pattern == "mixed":
            i, o = _draw(rng, live_in, n, True), _draw(rng, live_out, n, True)
        else:
            i, o = _draw(rng, live_in, n, False), _draw(rng, live_out, n, False)
            if c.pattern == "ascending":
                i.sort()
                o.sort()
            elif c.pattern == "one_row":
                i[:] = rng.integers(live_in)
        if c.family == "one_hot":      # the hot channels of gout's rows differ inside an offset
            o = _one_hot_rows(rng, live_out, c.cout, n)
            if c.pattern == "ascending":
                o.sort()
        elif c.family == "one_hot_t":
            i = _one_hot_rows(rng, live_in, c.cin, n)
            if c.pattern == "ascending":
                i.sort()
            if c.pattern == "one_row":  # the one-hot side cannot repeat a row: the other side does
                o[:] = rng.integers(live_out)
        pairs[k, 0, :n], pairs[k, 1, :n] = i, o
    return pairs


def _ints(rng, m, ch):
    return INT_CHOICES[rng.integers(0, INT_CHOICES.size, (m, ch))]


def _full(rng, m, ch):
    return (rng.standard_normal((m, ch)) * np.exp(rng.standard_normal((m, ch)))).astype(F32)


def _hot(rng, m, ch):
    x = np.zeros((m, ch), F32)
    x[np.arange(m), np.arange(m) % ch] = rng.choice([-1.0, 1.0], m) * np.exp2(rng.integers(-12, 13, m))
    return x


def operands(c, key=1):
    """feat f32 [m_in, cin], gout f32 [m_out, cout]; with pair lists the last row of each is the poison row.  `key` 1 is the case's own
    data; any other key gives the different values of the call that fills the workspace first."""
    rng = _rng(c.name, key)
    hot = {"one_hot": "gout", "one_hot_t": "feat"}.get(c.family)
    feat = (_hot if hot == "feat" else _full if hot else _ints)(rng, c.m_in, c.cin)
    gout = (_hot if hot == "gout" else _full if hot else _ints)(rng, c.m_out, c.cout)
    if c.num is not None:
        feat[-1], gout[-1] = POISON, POISON
    return feat, gout


def referee(feat, gout, pairs, counts):
    """f32 [kvol, cin, cout]: feat[in]^T gout[out] per offset in float64 (int64-exact for `ints`: every sum is an integer below 2^53),
    rounded once — which in the exact families rounds nothing.  Zeros are +0."""
    want = np.zeros((len(counts), feat.shape[1], gout.shape[1]), np.float64)
    f64, g64 = feat.astype(np.float64), gout.astype(np.float64)
    for k, n in enumerate(counts):
        i, o = (np.arange(n), np.arange(n)) if pairs is None else (pairs[k, 0, :n], pairs[k, 1, :n])
        want[k] = f64[i].T @ g64[o] + 0.0
    out = want.astype(F32)
    assert (out.astype(np.float64) == want).all()  # the referee itself is exact: no rounding in the conversion
    return out


@functools.lru_cache(maxsize=2)
def case(name):
    """dict(case, feat, gout, pairs | None, num i32 [kvol] | None, want f32 [kvol, cin, cout])."""
    c = SPECS[name]
    feat, gout = operands(c)
    pairs = None if c.num is None else _pairs(c)
    out = dict(case=c, feat=feat, gout=gout, pairs=pairs, num=None if c.num is None else np.asarray(c.num, np.int32),
               want=referee(feat, gout, pairs, c.counts))
    if c.family == "ints":
        assert max(c.counts) * 64 < 2 ** 24  # every partial sum in any order is an integer below 2^24
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def check_exact(name, got, want):
    """`got` f32 [kvol, cin, cout] equals the referee bit for bit; the message names the first offset and element that differ."""
    got = np.ascontiguousarray(got, F32).reshape(want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, ("%s: %d of %d elements differ, first (offset, ci, co) %s: got %r, want %r; offsets touched %s" % (
        name, len(bad), want.size, bad[0].tolist(), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]), sorted(set(bad[:, 0].tolist()))))
