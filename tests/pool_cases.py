"""Inputs for the dynamic point pooling (K17, fullysparsefusion_amd/csrc/point_pool.hip) that reach the kernel's paths one by one, and
the referee they are judged by: shared by tests/test_pool_cases_cpu.py (margins, path witnesses, the source pin), tests/test_point_pool_gpu.py
and the pooling tests of tests/test_hip_ops.py / tests/test_plugin_gpu.py.  No GPU and no product import here.

Referee: `oracle.refine.dynamic_point_pool` as it is, per sample where a case carries batch indices (the rows of all samples merged in
ascending (roi, point) order, then the global cap: what one batched launch returns).

Margin-clean: a (point, RoI) pair that lies within rounding of a box face may be decided either way by the device's sinf / cosf, and a
test that has to tolerate that cannot compare exactly.  So every case is cleaned: the oracle lists the pairs closer than NEAR_TOL to
a face (`return_margin=True, near_tol=NEAR_TOL`), every point in such a pair is PARKED (x, y kept, z = PARK_Z: above every enlarged box,
so it stays in its BEV cell and keeps its index, but is a hit of no RoI), and this repeats until the list is empty.  NEAR_TOL is 10 x
the 1e-4 the suite used to treat as "may flip on the device".

A case is a dict(rois f32 [R, C], pts f32 [P, Cp], box_col, batch_col (-1: none), xyz_col, pts_batch i64 [P] | None, extra, max_inbox,
max_all, tol 'fixed' | 'measured', parked i64 [k], passes, expect dict).  Every case is generated from a seed, built once (`case(name)`)
and must not be written to (the arrays are read-only)."""
import functools

import numpy as np

from oracle import refine as orefine

# restated from csrc/point_pool.hip, csrc/scan.h and csrc/radix_sort.h (pinned by test_pool_cases_cpu.py::test_constants_equal_the_kernel_source)
PB_CAP = 1024            # hits of one RoI the binned fill sorts in LDS; max_inbox above it takes the brute-force passes
PB_BINS = 1024           # index ranges of one narrowing round
PB_BITS = 10             # 1 m BEV cells, 2^10 per axis around the origin, border cells take everything beyond
PB_WALK_CELLS = 1024     # a circle rectangle of more cells walks the whole sorted array
PB_ROIS_PER_WG = 4       # binned kernels: one wave per RoI, four per workgroup
PP_TILE = 2048           # points per tile of the brute-force passes
PP_ROIS_PER_GROUP = 256  # brute-force passes: thread = RoI, 256 per group, groups counted in chunks of 1, 2, 4, ...
SC_TILE = 2048           # items per tile of the exclusive scan
SC_VALUE_MASK = (1 << 30) - 1  # the look-back scan's status words carry 30-bit running totals
RS_TILE = 2048           # keys per workgroup of the radix sort

F32 = np.float32
NEAR_TOL = 1e-3
PARK_Z = 1000.0
MAX_PARKED_SHARE = 0.02
BIG = 10 ** 9


# ---- referee ---------------------------------------------------------------------------------------------------------------------

def boxes(c):
    return c["rois"][:, c["box_col"]:c["box_col"] + 7]


def xyz(c):
    return c["pts"][:, c["xyz_col"]:c["xyz_col"] + 3]


def _samples(c):
    """[(roi rows, point rows)] of every sample; one entry of None, None without batch indices."""
    if c["pts_batch"] is None:
        return [(None, None)]
    rb = c["rois"][:, c["batch_col"]].astype(np.int64)
    return [(np.nonzero(rb == b)[0], np.nonzero(c["pts_batch"] == b)[0]) for b in np.unique(np.concatenate([rb, c["pts_batch"]]))]


def reference(c, max_inbox=None, max_all=None, stop_at_cap=False):
    """(pts_idx, roi_idx, feats) of the oracle at the case's caps (or the ones given)."""
    mi = c["max_inbox"] if max_inbox is None else max_inbox
    ma = c["max_all"] if max_all is None else max_all
    with np.errstate(all="ignore"):  # (inf - inf, inf * 0 of the non-finite rows: NaN compares false, the row is a hit of nothing)
        if c["pts_batch"] is None:
            return orefine.dynamic_point_pool(boxes(c), xyz(c), c["extra"], mi, ma, stop_at_cap=stop_at_cap)
        ps, rs, fs = [], [], []
        for rm, pm in _samples(c):  # the reference loops over the samples and offsets the indices
            if rm.size == 0 or pm.size == 0:
                continue
            p, r, f = orefine.dynamic_point_pool(boxes(c)[rm], xyz(c)[pm], c["extra"], mi, BIG)
            ps.append(pm[p])
            rs.append(rm[r])
            fs.append(f)
    if not ps:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 13), F32)
    p, r, f = np.concatenate(ps), np.concatenate(rs), np.concatenate(fs)
    o = np.lexsort((p, r))[:ma]
    return p[o], r[o], f[o]


def near_pairs(rois7, pts3, extra, pts_batch=None, roi_batch=None, tol=NEAR_TOL):
    """Rows (roi, point, margin) of the pairs the oracle decides within `tol` of a face (same-sample pairs only)."""
    with np.errstate(all="ignore"):
        if pts_batch is None:
            return orefine.dynamic_point_pool(rois7, pts3, extra, BIG, BIG, return_margin=True, near_tol=tol)[3]
        out = []
        for b in np.unique(roi_batch):
            rm, pm = np.nonzero(roi_batch == b)[0], np.nonzero(pts_batch == b)[0]
            if pm.size == 0:
                continue
            near = orefine.dynamic_point_pool(rois7[rm], pts3[pm], extra, BIG, BIG, return_margin=True, near_tol=tol)[3]
            out.append(np.stack([rm[near[:, 0].astype(np.int64)], pm[near[:, 1].astype(np.int64)], near[:, 2]], 1))
        return np.concatenate(out) if out else np.zeros((0, 3))


def margin_clean(rois7, pts3, extra, pts_batch=None, roi_batch=None, tol=NEAR_TOL, max_passes=6):
    """-> (points with every near-face point parked, parked indices, passes that parked something)."""
    pts3 = np.array(pts3, F32)
    parked, passes = [], 0
    for _ in range(max_passes + 1):
        near = near_pairs(rois7, pts3, extra, pts_batch, roi_batch, tol)
        if near.shape[0] == 0:
            return pts3, np.unique(np.concatenate(parked)).astype(np.int64) if parked else np.zeros(0, np.int64), passes
        idx = np.unique(near[:, 1].astype(np.int64))
        pts3[idx, 2] = PARK_Z
        parked.append(idx)
        passes += 1
    raise AssertionError("points keep landing near a face")


def features_f64(c, p, r):
    """Columns 3..11 (local coordinates, face distances) of the rows (p, r) in float64: the oracle's expressions
    (oracle/refine.py:35-56) on the fp32 inputs."""
    b, x = boxes(c)[r].astype(np.float64), xyz(c)[p].astype(np.float64)
    rot = b[:, 6] + np.pi / 2
    cosa, sina = np.cos(rot), np.sin(rot)
    dx, dy = x[:, 0] - b[:, 0], x[:, 1] - b[:, 1]
    lz = x[:, 2] - (b[:, 2] + b[:, 5] * 0.5)
    lx, ly = dx * cosa - dy * sina, dx * sina + dy * cosa
    hl, hw, hh = b[:, 4] * 0.5, b[:, 3] * 0.5, b[:, 5] * 0.5
    return np.stack([lx, ly, lz, lx + hl, ly + hw, lz + hh, hl - lx, hw - ly, hh - lz], 1)


def feature_tolerance(c, p, r, f):
    """Allowance for columns 3..11 against the fp32 oracle's rows (p, r, f): 2e-5 for the 'fixed' cases (boxes of a few metres within
    +-45 m, as the suite always had it); for the others 4 x the largest error the fp32 oracle itself makes against float64 on those
    rows, never below 2e-5.  -> (tolerance, the oracle's own error)."""
    if c["tol"] == "fixed" or p.size == 0:
        return 2e-5, 0.0
    own = float(np.abs(f[:, 3:12].astype(np.float64) - features_f64(c, p, r)).max())
    return max(2e-5, 4.0 * own), own


# ---- host models of the kernel's path choices ------------------------------------------------------------------------------------

def narrowing_trace(hit_indices, n_pts, keep):
    """pb_fill_kernel's index-range narrowing (point_pool.hip, the `hits_full > PB_CAP` block) for one RoI whose hits are the point
    indices `hit_indices`: per round (width, crossing bin, hits before it, hits in it), and the final limit."""
    h = np.sort(np.asarray(hit_indices, np.int64))
    assert h.size > PB_CAP >= keep >= 1
    lo, hi, below, rounds = 0, int(n_pts), 0, []
    while True:
        width = (hi - lo + PB_BINS - 1) // PB_BINS
        inside = h[(h >= lo) & (h < hi)]
        hist = np.bincount((inside - lo) // width, minlength=PB_BINS)
        cum = below + np.cumsum(hist)
        b = int(np.nonzero(cum >= keep)[0][0])
        c = int(hist[b])
        run = int(cum[b]) - c
        bin_lo = lo + b * width
        bin_hi = min(hi, bin_lo + width)
        rounds.append((width, b, run, c))
        if run + c <= PB_CAP or width == 1:
            return rounds, bin_hi
        lo, hi, below = bin_lo, bin_hi, run


def narrowing_rounds(hit_indices, n_pts, keep):
    """-> (rounds, limit, hits below the limit): the fill gathers the hits of index < limit, at least `keep` and at most PB_CAP."""
    rounds, limit = narrowing_trace(hit_indices, n_pts, keep)
    return len(rounds), limit, int((np.asarray(hit_indices) < limit).sum())


def pool_path(max_inbox):
    return "binned" if max_inbox <= PB_CAP else "brute"


def scan_form(n, max_item):
    """exclusive_scan_u32's choice (scan.h): one look-back launch while n * max_item cannot reach 2^30."""
    return "lookback" if n < SC_VALUE_MASK // max(int(max_item), 1) else "three_launch"


def _coord(v):
    with np.errstate(all="ignore"):
        f = np.floor(F32(v)) + F32(1 << (PB_BITS - 1))
    return 0 if not f == f else int(min(max(f, F32(0)), F32((1 << PB_BITS) - 1)))


def cell_rect(box7, extra):
    """(cells in x, cells in y, distance of the circle's four extremes from the nearest cell boundary) of the rectangle of cells
    pb_for_candidates walks for a box: load_box's fp32 radius, pb_coord's cells."""
    b = np.asarray(box7, F32)
    lhw, lhl = (b[3] + F32(extra[0])) * F32(0.5), (b[4] + F32(extra[1])) * F32(0.5)
    rad = np.sqrt((lhw * lhw + lhl * lhl) * F32(1.0001) + F32(1e-6))
    ends = [b[0] - rad, b[0] + rad, b[1] - rad, b[1] + rad]
    slack = min(float(min(e - np.floor(e), np.ceil(e) - e)) for e in ends)
    return _coord(ends[1]) - _coord(ends[0]) + 1, _coord(ends[3]) - _coord(ends[2]) + 1, slack


# ---- building blocks -------------------------------------------------------------------------------------------------------------

def _rng(*key):
    return np.random.default_rng([17, *key])


def random_rois(rng, r, spread=40.0):
    ctr = rng.uniform(-spread, spread, (r, 2))
    z = rng.uniform(-2.5, -0.5, (r, 1))
    wlh = np.stack([rng.uniform(0.5, 2.5, r), rng.uniform(0.8, 6.0, r), rng.uniform(1.0, 3.0, r)], 1)
    rz = rng.uniform(-np.pi, np.pi, (r, 1))
    return np.concatenate([ctr, z, wlh, rz], 1).astype(F32)


def _scene(rng, r, p, spread, near=0.5):
    """r random RoIs and p points, a share `near` of them clustered around RoI centres so that the boxes are populated."""
    rois = random_rois(rng, r, spread)
    k = int(np.ceil(p * near))
    which = rng.integers(0, r, k)
    a = rois[which, :3] + rng.normal(0, 1.5, (k, 3)) + np.array([0, 0, 1.0])
    b = np.concatenate([rng.uniform(-spread - 5, spread + 5, (p - k, 2)), rng.uniform(-3, 2, (p - k, 1))], 1)
    return rois, np.concatenate([a, b]).astype(F32)


def _inside(rng, n, roi, extra, clear=0.02):
    """n points inside the enlarged box of `roi`, each local coordinate at least `clear` away from both the box's and the enlarged
    box's face (so about (extra / 2) / (half extent) of them are margin points)."""
    cx, cy, czb, w, l, h, rz = [float(v) for v in roi]
    half = np.array([l, w, h]) * 0.5
    large = half + np.array([extra[1], extra[0], extra[2]]) * 0.5
    out = np.zeros((0, 3))
    while out.shape[0] < n:
        v = rng.uniform(-large + clear, large - clear, (2 * n + 64, 3))
        ok = (np.abs(np.abs(v) - half) >= clear).all(1)
        out = np.concatenate([out, v[ok]])
    lx, ly, lz = out[:n].T
    c, s = np.cos(rz + np.pi / 2), np.sin(rz + np.pi / 2)
    return np.stack([cx + lx * c + ly * s, cy - lx * s + ly * c, czb + h * 0.5 + lz], 1)


def _misses(rng, n, rois7):
    """n points that are a hit of no RoI: half of them above the boxes (same cells, inside the circles), half far away in the plane."""
    k = n // 2
    ctr = rois7[rng.integers(0, rois7.shape[0], k), :2] + rng.normal(0, 2.0, (k, 2))
    above = np.concatenate([ctr, rng.uniform(30.0, 40.0, (k, 1))], 1)
    far = np.concatenate([rng.uniform(150.0, 250.0, (n - k, 2)), rng.uniform(-3, 2, (n - k, 1))], 1)
    return np.concatenate([above, far])


def _layout(rng, n_pts, rois7, extra, hits):
    """Points [n_pts, 3]: the indices hits[r] lie inside RoI r's enlarged box (the boxes must not overlap), all others are misses."""
    pts = _misses(rng, n_pts, rois7)
    for r, idx in hits.items():
        pts[idx] = _inside(rng, len(idx), rois7[r], extra)
    return pts.astype(F32)


def _box(cx, cy, w=4.0, l=8.0, h=2.0, rz=0.3):
    return [cx, cy, -1.0, w, l, h, rz]


def _finish(rois, pts, max_inbox, max_all, extra=(1.0, 1.0, 1.0), box_col=0, batch_col=-1, xyz_col=0, pts_batch=None, tol="measured",
            expect=None, cleaned=None):
    rois, pts = np.array(rois, F32), np.array(pts, F32)
    if cleaned is None:
        rb = rois[:, batch_col].astype(np.int64) if pts_batch is not None else None
        clean, parked, passes = margin_clean(rois[:, box_col:box_col + 7], pts[:, xyz_col:xyz_col + 3], extra, pts_batch, rb)
        pts[:, xyz_col:xyz_col + 3] = clean
    else:
        parked, passes = cleaned
    c = dict(rois=rois, pts=pts, box_col=box_col, batch_col=batch_col, xyz_col=xyz_col,
             pts_batch=None if pts_batch is None else np.array(pts_batch, np.int64), extra=tuple(float(v) for v in extra),
             max_inbox=int(max_inbox), max_all=int(max_all), tol=tol, parked=parked, passes=passes, expect=expect or {})
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ---- a. the eight parametrisations the suite always had (tests/test_hip_ops.py), margin-clean -----------------------------------------

FAMILY_A = ((37, 20000, 512, 50000), (300, 60000, 16, 50000), (300, 60000, 512, 700), (1, 5000, 512, 50000), (700, 3000, 512, 50000),
            (2000, 20000, 32, 3000), (2000, 20000, 512, 10 ** 6), (1100, 8000, 4, 900))


@functools.lru_cache(maxsize=None)
def _family_a_inputs(r, p):
    rng = np.random.default_rng(r * 31 + p)
    rois = random_rois(rng, r)
    which = rng.integers(0, r, p // 2)  # points: half uniform, half clustered around RoI centres so boxes are well populated
    near = rois[which, :3] + rng.normal(0, 1.5, (p // 2, 3)) + np.array([0, 0, 1.0])
    pts = np.concatenate([near, np.concatenate([rng.uniform(-45, 45, (p - p // 2, 2)), rng.uniform(-3, 2, (p - p // 2, 1))], 1)])
    pts = np.concatenate([pts, rng.random((p, 2))], 1).astype(F32)  # stride-5 rows like the real points
    clean, parked, passes = margin_clean(rois, pts[:, :3], (1.0, 1.0, 1.0))
    pts[:, :3] = clean
    return rois, pts, parked, passes


def _family_a(r, p, max_inbox, max_all):
    rois, pts, parked, passes = _family_a_inputs(r, p)
    return _finish(rois, pts, max_inbox, max_all, tol="fixed", cleaned=(parked, passes))  # (one cleaning per input set)


def family_a_name(r, p, max_inbox, max_all):
    return f"a-{r}-{p}-{max_inbox}-{max_all}"


# ---- b, c, g. one RoI's hits against PB_CAP, the narrowing rounds, the brute-force passes above PB_CAP ------------------------------

def _cap_edges(max_inbox):
    """Three RoIs with exactly PB_CAP, PB_CAP + 1 and 3000 hits among 5400 points in random order."""
    rng = _rng(2)
    rois = np.array([_box(0, 0), _box(20, 0, rz=-1.2), _box(40, 3, rz=2.5)], F32)
    counts = [PB_CAP, PB_CAP + 1, 3000]
    order = rng.permutation(5400)
    cuts = np.cumsum([0] + counts)
    hits = {r: np.sort(order[cuts[r]:cuts[r + 1]]) for r in range(3)}
    pts = _layout(rng, 5400, rois, (1.0, 1.0, 1.0), hits)
    return _finish(rois, pts, max_inbox, 50000, expect=dict(hits=dict(enumerate(counts))))


def _every_second(max_inbox, max_all=50000):
    """One RoI whose hits are the even indices of 6000 points (3000 hits over three point tiles), one light RoI after it."""
    rng = _rng(3)
    rois = np.array([_box(0, 0), _box(20, 0, rz=-0.7)], F32)
    hits = {0: np.arange(0, 6000, 2), 1: np.arange(1, 600, 6)}
    pts = _layout(rng, 6000, rois, (1.0, 1.0, 1.0), hits)
    return _finish(rois, pts, max_inbox, max_all, expect=dict(hits={0: 3000, 1: 100}, hit_index={0: hits[0]}))


BIG_N = (1 << 20) + 4096


def _million():
    """2^20 + 4096 points inside ONE box footprint, three RoIs stacked on it: RoI 0 is hit by every index except 0 (three narrowing
    rounds at max_inbox 1024), RoI 1 by every index except 0 and those = 7 mod 2048 (two rounds), RoI 2 by the 514 of index = 7 mod 2048
    only; max_all cuts RoI 2's list in the middle."""
    rng = _rng(4)
    n = BIG_N
    upper = (np.arange(n) % 2048) == 7
    rois = np.array([[0, 0, -2.0, 4, 8, 8.0, 0.3], [0, 0, -1.5, 4, 8, 3.0, 0.3], [0, 0, 2.5, 4, 8, 2.0, 0.3]], F32)
    flat = np.array([0, 0, -0.5, 4, 8, 1.0, 0.3])  # local z in (-0.48, 0.48) around 0
    pts = _inside(rng, n, flat, (1.0, 1.0, 0.0))
    pts[upper, 2] += 3.5
    pts[0, 2] = PARK_Z
    idx = np.arange(n)
    hits = {0: idx[1:], 1: idx[~upper][1:], 2: idx[upper]}
    return _finish(rois, pts, PB_CAP, 2 * PB_CAP + 452,
                   expect=dict(hits={r: int(h.size) for r, h in hits.items()}, hit_index={0: hits[0], 1: hits[1]}, rounds={0: 3, 1: 2}))


def _last_bin():
    """7003 points: the bins are 7 indices wide and bin 1000 holds only [7000, 7003).  RoI 0 has 1022 hits below 7000 and the three last
    indices: at max_inbox 1024 the count crosses in the partial bin, which alone is then split again."""
    rng = _rng(5)
    rois = np.array([_box(0, 0), _box(20, 0, rz=1.1)], F32)
    low = np.sort(rng.choice(7000, 1022 + 300, replace=False))
    hits = {0: np.concatenate([low[:1022], [7000, 7001, 7002]]), 1: low[1022:]}
    hits = {r: np.sort(h) for r, h in hits.items()}
    pts = _layout(rng, 7003, rois, (1.0, 1.0, 1.0), hits)
    return _finish(rois, pts, PB_CAP, 50000, expect=dict(hits={0: 1025, 1: 300}, hit_index={0: hits[0]}, rounds={0: 2}))


def _lane_edges():
    """12288 points (bins of 12 indices).  RoI 0's 512th hit lies in bin 160, the FIRST of the 16 bins lane 10 sums; RoI 1's in bin 175,
    the LAST of them: the wave-level prefix finds the lane, the walk over its bins has to stop at once / at its end."""
    rng = _rng(6)
    rois = np.array([_box(0, 0), _box(20, 0, rz=-2.0)], F32)
    even, odd = np.arange(0, 12288, 2), np.arange(1, 12288, 2)
    h0 = np.concatenate([rng.choice(even[even < 160 * 12], 511, replace=False), even[(even >= 160 * 12) & (even < 161 * 12)],
                         rng.choice(even[even >= 161 * 12], 600, replace=False)])
    h1 = np.concatenate([rng.choice(odd[odd < 175 * 12], 511, replace=False), odd[(odd >= 175 * 12) & (odd < 176 * 12)],
                         rng.choice(odd[odd >= 176 * 12], 600, replace=False)])
    hits = {0: np.sort(h0), 1: np.sort(h1)}
    pts = _layout(rng, 12288, rois, (1.0, 1.0, 1.0), hits)
    return _finish(rois, pts, 512, 50000, expect=dict(hits={0: 1117, 1: 1117}, hit_index=hits, rounds={0: 1, 1: 1}, bins={0: 160, 1: 175}))


# ---- d. the global cap inside the binned fill ----------------------------------------------------------------------------------------

LIGHT = (40, 55, 70, 35, 50)


def _cap_in_fill(where):
    """Five light RoIs, then a heavy one (3000 hits, cut to 512) LAST: nothing after it masks a wrong cut.  max_all falls in the middle
    of the heavy RoI's list ('middle'), exactly on its first row, so that it contributes nothing ('first_row'), or one row further."""
    rng = _rng(7)
    rois = np.array([_box(12.0 * i, -20.0, rz=0.4 * i) for i in range(5)] + [_box(0, 20)], F32)
    order = rng.permutation(4000)
    cuts = np.cumsum((0,) + LIGHT + (3000,))
    hits = {r: np.sort(order[cuts[r]:cuts[r + 1]]) for r in range(6)}
    pts = _layout(rng, 4000, rois, (1.0, 1.0, 1.0), hits)
    max_all = sum(LIGHT) + {"middle": 200, "first_row": 0, "second_row": 1}[where]
    return _finish(rois, pts, 512, max_all, expect=dict(hits=dict(enumerate(LIGHT + (3000,))), rows_of_last={"middle": 200, "first_row": 0,
                                                                                                           "second_row": 1}[where]))


# ---- e. cell geometry ------------------------------------------------------------------------------------------------------------------

def _cell_rect_case():
    """Two long boxes of the same size: the rectangle of cells under RoI 0's circle is 32 x 32 = 1024 (the table walk's last size), under
    RoI 1's 32 x 33 = 1056 (the whole-array walk).  The sides of such a rectangle differ by at most one, so 1025 = 25 x 41 cells does not
    exist: 1056 is the first size above 1024."""
    rng = _rng(8)
    rois = np.array([[0.0, 0.0, -1.0, 7.6, 29.0, 2.0, 0.5], [40.0, 0.5, -1.0, 7.6, 29.0, 2.0, -0.9]], F32)
    pts = np.concatenate([np.concatenate([rng.uniform(-20, 60, (5000, 1)), rng.uniform(-20, 20, (5000, 1)), rng.uniform(-2, 2, (5000, 1))], 1),
                          _inside(rng, 500, rois[0], (1.0, 1.0, 1.0)), _inside(rng, 500, rois[1], (1.0, 1.0, 1.0))])
    pts = pts[rng.permutation(pts.shape[0])]
    return _finish(rois, pts, 512, 50000, expect=dict(rect={0: (32, 32), 1: (32, 33)}))


def _cell_edges_case():
    """RoIs straddling cell rows at negative coordinates, on the +-512 m border cells and beyond them (the border cells collect
    everything outside); points on exact integer coordinates, at -0.0, NaN and +-inf."""
    rng = _rng(9)
    centres = [(-3.0, -7.0), (-0.5, 0.5), (0.0, 0.0), (-16.0, 3.0), (511.5, 0.2), (-512.2, -511.8), (600.0, 600.0), (-700.0, 511.0), (3.5, -2.0)]
    rois = random_rois(rng, len(centres), 1.0)
    rois[:, :2] = centres
    rois[:, 3:5] += 1.0
    parts = [np.array(c + (0.0,)) + np.concatenate([rng.normal(0, 2.5, (400, 2)), rng.uniform(-3, 2, (400, 1))], 1) for c in centres]
    g = np.arange(-8, 9, dtype=np.float64)
    grid = np.stack(np.meshgrid(g, g, [-1.0, 0.0]), -1).reshape(-1, 3)  # exact integers around the origin
    zeros = np.array([[-0.0, -0.0, -0.0], [-0.0, 0.0, -1.0], [0.0, -0.0, -1.0], [-0.0, 1.0, -0.0], [-1.0, -0.0, 0.0]])
    pts = np.concatenate(parts + [grid, zeros])
    pts = pts[rng.permutation(pts.shape[0])]
    bad = np.array([[np.nan, 0, 0], [0, np.nan, -1], [0, 0, np.nan], [np.inf, 0, 0], [0, -np.inf, 0], [0.5, 0.5, np.inf], [-np.inf, np.inf, 0],
                    [np.nan, np.nan, np.nan]])
    at = np.sort(rng.choice(pts.shape[0], bad.shape[0], replace=False))
    pts[at] = bad
    return _finish(rois, pts, 512, 50000, expect=dict(nonfinite=at))


def _batched_case():
    """Two samples whose points share cells and whose RoIs overlap in space (a point inside a RoI of the other sample must not count), points
    of the two samples interleaved, RoIs not in sample order, a heavy RoI (> PB_CAP hits) cut by max_inbox, max_all cutting a later RoI's list."""
    rng = _rng(10)
    r, p = 24, 9000
    rois = random_rois(rng, r, 8.0)
    rois[5] = [1.0, -1.0, -2.0, 7.0, 9.0, 4.0, 0.8]  # heavy
    rb = rng.integers(0, 2, r).astype(np.float64)
    rb[5] = 1.0
    pb = rng.integers(0, 2, p).astype(np.int64)
    pts = np.concatenate([rng.normal(0, 5.0, (p, 2)), rng.uniform(-3, 2, (p, 1))], 1)
    rois8 = np.concatenate([rb[:, None], rois], 1)
    return _finish(rois8, pts, 256, 2000, box_col=1, batch_col=0, pts_batch=pb, expect=dict(heavy=5))


# ---- f. sizes at the tile edges, column offsets ----------------------------------------------------------------------------------------

PTS_SIZES = (1, 63, 64, 65, 256, 257, 2047, 2048, 2049, 4097)
ROI_SIZES = (1, 3, 4, 5, 256, 257)


def _pts_size(n):
    rois, pts = _scene(_rng(11, n), 5, n, 6.0, near=0.8)
    if n == 1:  # the only point: 0.25 m off the centre of RoI 2
        pts[0] = rois[2, :3] + np.array([0.25, 0.25, 0.5 * rois[2, 5]], F32)
    return _finish(rois, pts, 512, 50000)


def _roi_size(n):
    rois, pts = _scene(_rng(12, n), n, 3000, 3.0 * np.sqrt(n), near=0.7)
    return _finish(rois, pts, 16, 700)


def _strided_case():
    """RoI rows [junk, batch, junk, box (7), junk], point rows [junk, junk, x, y, z, junk]: the op gets column offsets and row strides."""
    rng = _rng(13)
    rois, pts = _scene(rng, 40, 4000, 10.0, near=0.6)
    rb, pb = np.sort(rng.integers(0, 2, 40)), np.sort(rng.integers(0, 2, 4000)).astype(np.int64)
    junk = lambda n, k: rng.uniform(-50, 50, (n, k))  # noqa: E731
    rois11 = np.concatenate([junk(40, 1), rb[:, None], junk(40, 1), rois, junk(40, 1)], 1)
    pts6 = np.concatenate([junk(4000, 2), pts, junk(4000, 1)], 1)
    return _finish(rois11, pts6, 32, 600, box_col=3, batch_col=1, xyz_col=2, pts_batch=pb)


# ---- g. the scan's two forms behind the brute-force passes -----------------------------------------------------------------------------

SCAN_MAX_INBOX = 1 << 19


def _scan_case(n_rois):
    """max_inbox_point = 2^19 bounds every scanned value: 2000 RoIs stay below 2^30 in all (look-back form), 2100 do not (three launches).
    max_all is above the number of rows, so that the offsets of the last scan tile's RoIs (2048 ..) decide where rows land."""
    rois, pts = _scene(_rng(14, n_rois), n_rois, 4000, 40.0, near=0.6)
    return _finish(rois, pts, SCAN_MAX_INBOX, 50000, expect=dict(scan={2000: "lookback", 2100: "three_launch"}[n_rois]))


# ---- registry --------------------------------------------------------------------------------------------------------------------

_BUILDERS = {family_a_name(*t): functools.partial(_family_a, *t) for t in FAMILY_A}
_BUILDERS.update({f"b-cap_edges-{m}": functools.partial(_cap_edges, m) for m in (PB_CAP - 1, PB_CAP, PB_CAP + 1)})
_BUILDERS.update({f"c-every_second-{m}": functools.partial(_every_second, m) for m in (512, PB_CAP - 1, PB_CAP)})
_BUILDERS.update({"c-million": _million, "c-last_bin": _last_bin, "c-lane_edges": _lane_edges})
_BUILDERS.update({f"d-cap_{w}": functools.partial(_cap_in_fill, w) for w in ("middle", "first_row", "second_row")})
_BUILDERS.update({"e-cell_rect": _cell_rect_case, "e-cell_edges": _cell_edges_case, "e-batched": _batched_case})
_BUILDERS.update({f"f-pts-{n}": functools.partial(_pts_size, n) for n in PTS_SIZES})
_BUILDERS.update({f"f-rois-{n}": functools.partial(_roi_size, n) for n in ROI_SIZES})
_BUILDERS.update({"f-strided": _strided_case, "g-every_second-2048": functools.partial(_every_second, 2 * PB_CAP),
                  "g-every_second-capped": functools.partial(_every_second, 2 * PB_CAP, 1500),
                  "g-scan-2000": functools.partial(_scan_case, 2000), "g-scan-2100": functools.partial(_scan_case, 2100)})
NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def want(name):
    """The referee's rows of a case, computed once: (pts_idx i64 [k], roi_idx i64 [k], feats f32 [k, 13]), read-only."""
    out = reference(case(name))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def full_rows(name):
    """(pts_idx, roi_idx) of the referee without any cap."""
    p, r, _ = reference(case(name), BIG, BIG)
    return p, r


def full_hits(name):
    """Hits per RoI without any cap."""
    return np.bincount(full_rows(name)[1], minlength=case(name)["rois"].shape[0])


def hit_index(name, r):
    """The point indices that hit RoI r, ascending."""
    p, ri = full_rows(name)
    return p[ri == r]
