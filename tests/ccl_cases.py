"""Point layouts for the device connected components (K19, fullysparsefusion_amd/csrc/ccl.hip) that reach the kernel's paths one by
one, and the referee they are judged by: shared by tests/test_ccl_cases_cpu.py (the referee against a brute-force union-find, the
path witnesses, the source pin) and tests/test_ccl_gpu.py.  No GPU and no product import here.

Referee: `oracle.modules.connected_components_xy` as it is (the reference's fp32 expression decides each pair, scipy labels), run
per sample (`batched`) or per group with the group's own distance (`grouped`), the labels then numbered by first member over all
rows: what `hip_ops.connected_components(..., batch_idx=)` and `hip_ops.connected_components_grouped` return.

A case is a dict(kind 'plain' | 'batched' | 'grouped', points f32 [n, cols], dist float | None, idx int32 [n] | None,
table f32 [G] | None, want int32 [n]).  Every case is generated from a seed, built once (`case(name)`) and must not be written to."""
import functools

import numpy as np
import torch

from oracle import modules as omod

# restated from csrc/ccl.hip (pinned by test_ccl_cases_cpu.py::test_constants_equal_the_kernel_source): rows per tile of the pair
# matrix, tiles of a tile row one block walks, capacity of the LDS link queue of one tile pair
TILE = 256
CCL_TJ = 4
QCAP = 2048

F32 = np.float32
DIST = 0.6


# ---- referee ---------------------------------------------------------------------------------------------------------------------

def number_by_first_member(raw):
    """Arbitrary component ids [n] -> 0..K-1 in order of each component's first row."""
    raw = np.asarray(raw)
    if raw.size == 0:
        return np.zeros(0, np.int32)
    _, first, inv = np.unique(raw, return_index=True, return_inverse=True)
    rank = np.empty(first.size, np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.size)
    return rank[inv.reshape(-1)].astype(np.int32)


def plain(points, dist):
    return omod.connected_components_xy(torch.from_numpy(np.array(points, F32, order="C")), float(dist)).numpy().astype(np.int32)


def _per_part(points, part, dist_of):
    raw = np.full(points.shape[0], -1, np.int64)
    base = 0
    for p in np.unique(part):
        rows = np.nonzero(part == p)[0]
        d = dist_of(int(p))
        lab = plain(points[rows], d).astype(np.int64) if d > 0 else np.arange(rows.size)  # (not > 0: singletons)
        raw[rows] = base + lab
        base += int(lab.max()) + 1
    return raw


def batched_reference_order(points, batch_idx, dist):
    """The reference's find_connected_componets: per-sample components, sample 0's numbered first, then sample 1's, ..."""
    return _per_part(points, np.asarray(batch_idx), lambda b: float(dist)).astype(np.int32)


def batched(points, batch_idx, dist):
    return number_by_first_member(batched_reference_order(points, batch_idx, dist))


def grouped(points, group_idx, table):
    """Per group with table[g]; a group whose distance is not > 0 gives singletons; numbered by first member over all rows."""
    table = np.asarray(table, F32)
    return number_by_first_member(_per_part(points, np.asarray(group_idx), lambda g: float(table[g])))


# ---- layout families -------------------------------------------------------------------------------------------------------------

def _rng(*key):
    return np.random.default_rng([19, *key])


def _cloud(rng, n, dist, degree=1.5, cols=3):
    """n points uniform in the square in which a point has `degree` neighbours within `dist` on average."""
    side = np.sqrt(n * np.pi * dist * dist / degree)
    p = rng.uniform(-1.0, 1.0, (n, cols))
    p[:, :2] = rng.uniform(0.0, side, (n, 2))
    return p.astype(F32)


TILE_EDGE_SIZES = (2, 255, 256, 257, 1023, 1024, 1025, 2049)


def tile_edges(n):
    return _cloud(_rng(1, n), n, DIST), DIST, None


def strips(order):
    rng = _rng(2)
    p = np.concatenate([rng.uniform(0.0, 100.0, (4096, 2)), rng.uniform(-1.0, 1.0, (4096, 1))], 1).astype(F32)
    if order == "x":
        o = np.argsort(p[:, 0], kind="stable")
    elif order == "y":
        o = np.argsort(p[:, 1], kind="stable")
    else:  # the product's order: 0.5 m cells, y cell then x cell
        c = np.floor(p[:, :2] / 0.5).astype(np.int64)
        o = np.lexsort((c[:, 0], c[:, 1]))
    return p[o], DIST, None


def chains(order, gaps):
    k = np.arange(6000)
    x = 0.5 * k + (0.2 * (k // 1000) if gaps else 0.0)  # a 0.7 step after every 1000th point
    p = np.stack([x, np.full(6000, 3.0), np.zeros(6000)], 1).astype(F32)
    o = {"ascending": k, "descending": k[::-1], "permuted": _rng(3).permutation(6000)}[order]
    return p[o], DIST, None


BRIDGE_ROWS = 9


def late_bridge():
    x = 0.5 * np.arange(2000)
    a = np.stack([x, np.zeros(2000)], 1)
    b = np.stack([x, np.full(2000, 5.0)], 1)
    c = np.stack([np.full(BRIDGE_ROWS, 500.0), 0.5 * np.arange(1, BRIDGE_ROWS + 1)], 1)  # y = 0.5 .. 4.5: the last rows of the array
    p = np.concatenate([a, b, c])
    return np.concatenate([p, np.zeros((p.shape[0], 1))], 1).astype(F32), DIST, None


def blobs(permuted):
    rng = _rng(5)
    a = rng.uniform(0.0, 0.1, (300, 2))
    b = rng.uniform(0.0, 0.1, (300, 2)) + [0.4, 0.0]  # 0.3 m between the squares; the farthest pair is 0.51 m apart
    g = np.arange(424)
    far = np.stack([100.0 + 2.0 * (g % 21), 100.0 + 2.0 * (g // 21)], 1)
    p = np.concatenate([a, b, far])
    p = np.concatenate([p, rng.uniform(-1.0, 1.0, (1024, 1))], 1).astype(F32)
    return (p[rng.permutation(1024)] if permuted else p), DIST, None


SATELLITES = 8


def blob_satellites():
    """Links that only the queue-full fallback can make.  Tile 0 is one 256-point blob A in a 0.1 m square; tile 1 begins with 128
    rows R of such a blob 0.45 m to the right of A (every A-R pair links: 32 768 links at the low columns of tile pair (0, 1), and a
    single 64-thread wave queues 8 192 of them, four times QCAP, before it gets to column 128) and continues with SATELLITES rows S
    0.45 m to the LEFT of A: within dist of every row of A, 0.9 m from R.  S meets A in tile pair (0, 1) alone, at columns >= 128,
    when the queue is full whatever the order the waves run in.  The rest are far-away singletons.  One component of 392 rows."""
    rng = _rng(5, 1)
    a = rng.uniform(0.0, 0.1, (TILE, 2))
    r = rng.uniform(0.0, 0.1, (128, 2)) + [0.45, 0.0]
    s = rng.uniform(0.0, 0.1, (SATELLITES, 2)) + [-0.45, 0.0]
    g = np.arange(1024 - TILE - 128 - SATELLITES)
    far = np.stack([100.0 + 2.0 * (g % 21), 100.0 + 2.0 * (g // 21)], 1)
    p = np.concatenate([a, r, s, far])
    return np.concatenate([p, rng.uniform(-1.0, 1.0, (1024, 1))], 1).astype(F32), DIST, None


def _lattice(spacing):
    k = np.arange(40, dtype=F32)
    gx, gy = np.meshgrid(F32(spacing) * k, F32(spacing) * k)
    return np.stack([gx.ravel(), gy.ravel(), np.zeros(1600, F32)], 1).astype(F32)


def lattice_half(successor):
    d = F32(0.5)
    return _lattice(0.5), float(np.nextafter(d, F32(np.inf)) if successor else d), None


def pythagorean(k, successor):
    p = np.array([[0.0, 0.0, 0.0], [0.75 * k, 1.0 * k, 0.0]], F32)
    d = F32(1.25 * k)
    return p, float(np.nextafter(d, F32(np.inf)) if successor else d), None


def reference_distances(p, i, j):
    """The referee's own fp32 distance expression on the pairs (i, j)."""
    t = torch.from_numpy(np.ascontiguousarray(p[:, :2]))
    return (((t[torch.as_tensor(i)] - t[torch.as_tensor(j)]) ** 2).sum(1) ** 0.5).numpy()


def lattice_tenth(successor):
    """Spacing float32(0.1): neighbouring pairs differ by an ulp or two from one another; dist is the referee's distance of the
    neighbouring pair (row 20 of the lattice, columns 20 and 21)."""
    p = _lattice(0.1)
    d = reference_distances(p, [20 * 40 + 20], [20 * 40 + 21])[0]
    return p, float(np.nextafter(d, F32(np.inf)) if successor else d), None


def _triples():
    rng = _rng(7)
    p = np.concatenate([rng.uniform(0.0, 20.0, (500, 2)), rng.uniform(-1.0, 1.0, (500, 1))], 1).astype(F32)
    return np.tile(p, (3, 1))[rng.permutation(1500)]


def triples(dist):
    return _triples(), dist, None


NONFINITE_ROWS = {3: (np.nan, 1.0), 200: (1.0, np.nan), 255: (np.inf, 1.0), 256: (-np.inf, 1.0), 257: (1.0, np.inf), 600: (np.inf, -np.inf),
                  601: (np.inf, np.inf), 602: (np.inf, np.inf), 1000: (np.nan, np.nan), 1024: (1.0, -np.inf)}


def nonfinite_clean():
    return _cloud(_rng(7, 1), 1025, DIST)


def nonfinite_rows():
    p = nonfinite_clean().copy()
    for r, xy in NONFINITE_ROWS.items():
        p[r, :2] = xy
    return p, DIST, None


def nonfinite_tile():
    """A whole tile (rows 256..511) of NaN rows, and one of +inf rows (512..767), among ordinary ones."""
    p = nonfinite_clean().copy()
    p[256:512, :2] = np.nan
    p[512:768, :2] = np.inf
    return p, DIST, None


def columns(cols):
    p = _cloud(_rng(7, 2), 777, DIST, cols=2)
    if cols > 2:
        rng = _rng(7, 3)
        extra = rng.uniform(-1.0, 1.0, (777, cols - 2)) * 10.0 ** rng.integers(-30, 30, (777, cols - 2))
        extra[::5, -1] = np.nan
        extra[1::5, -1] = np.inf
        p = np.concatenate([p, extra.astype(F32)], 1)
    return p, DIST, None


def batch_shared(samples):
    """The same cloud given to samples 0 and 1 (every cross-sample pair of the two at distance 0), a third sample with a cloud of its
    own in the same square, rows interleaved."""
    rng = _rng(8, samples)
    p = _cloud(rng, 700, DIST)
    parts, idx = [p, p.copy()], [np.zeros(700, np.int32), np.ones(700, np.int32)]
    if samples == 3:
        parts.append(_cloud(rng, 700, DIST))
        idx.append(np.full(700, 2, np.int32))
    o = rng.permutation(700 * samples)
    return np.concatenate(parts)[o], DIST, np.concatenate(idx)[o]


GROUP_TABLE = np.array([0.6, 0.4, 0.0, 1.0, 0.2, 0.6], F32)


def _group_clouds(sizes, table):
    """One cloud per group, all in squares with the same corner, each at ~1.5 neighbours within its own distance (0.6 where it is 0)."""
    pts, ids = [], []
    for g, m in enumerate(sizes):
        pts.append(_cloud(_rng(9, g, m), m, float(table[g]) if table[g] > 0 else DIST))
        ids.append(np.full(m, g, np.int32))
    return np.concatenate(pts), np.concatenate(ids)


def group_sorted():
    p, ids = _group_clouds([500] * 6, GROUP_TABLE)
    return p, GROUP_TABLE, ids


GROUP_HALVES = (0, 5, 2, 4, 1, 3, 5, 0, 3, 1, 4, 2)


def group_unsorted():
    """The groups' rows in half-groups of 250 in the order GROUP_HALVES: a tile holds two or three groups, and its (min, max) range
    spans groups it does not hold (rows 0..255: groups 0 and 5, range 0..5)."""
    p, ids = _group_clouds([500] * 6, GROUP_TABLE)
    seen, o = [0] * 6, []
    for g in GROUP_HALVES:
        o.append(500 * g + 250 * seen[g] + np.arange(250))
        seen[g] += 1
    o = np.concatenate(o)
    return p[o], GROUP_TABLE, ids[o]


def group_permuted():
    p, ids = _group_clouds([500] * 6, GROUP_TABLE)
    o = _rng(9, 100).permutation(3000)
    return p[o], GROUP_TABLE, ids[o]


GROUP_STRIP_SIZES = (520, 512, 512, 512, 512, 432)


def group_strips():
    """Group-sorted rows, each group uniform in the same 20 m square and sorted by x inside its group, ascending in even groups and
    descending in odd ones, so that a tile is a thin strip as in the product.  A group ends 8 rows into a tile: the tile that holds the
    last 8 rows of group 2 (distance 0) holds the first 248 of group 3 (distance 1.0), and its links to the next strip of group 3 need
    the LARGEST distance of the tile's group range in the box test."""
    pts, ids = [], []
    for g, m in enumerate(GROUP_STRIP_SIZES):
        rng = _rng(9, 400, g)
        p = np.concatenate([rng.uniform(0.0, 20.0, (m, 2)), rng.uniform(-1.0, 1.0, (m, 1))], 1).astype(F32)
        o = np.argsort(p[:, 0], kind="stable")
        pts.append(p[o if g % 2 == 0 else o[::-1]])
        ids.append(np.full(m, g, np.int32))
    return np.concatenate(pts), GROUP_TABLE, np.concatenate(ids)


def group_same_coordinates(interleaved):
    """One 250-point cloud in every one of the six groups: cross-group pairs at distance 0."""
    p = _cloud(_rng(9, 200), 250, 0.4)
    if interleaved:
        return np.repeat(p, 6, 0), GROUP_TABLE, np.tile(np.arange(6, dtype=np.int32), 250)
    return np.tile(p, (6, 1)), GROUP_TABLE, np.repeat(np.arange(6, dtype=np.int32), 250)


def group_single_member():
    """Groups of 400, 1, 0, 300, 1 and 322 rows (n = 1024): one-member groups, one with a distance of 0, and an empty group."""
    table = np.array([0.6, 0.4, 1.0, 1.0, 0.0, 0.6], F32)
    p, ids = _group_clouds([400, 1, 0, 300, 1, 322], table)
    return p, table, ids


def group_one_entry_table():
    return _cloud(_rng(9, 300), 777, DIST), np.array([DIST], F32), np.zeros(777, np.int32)


BUILDERS = {}
for _n in TILE_EDGE_SIZES:
    BUILDERS[f"tile_edges-{_n}"] = ("plain", functools.partial(tile_edges, _n))
for _o in ("x", "y", "cell"):
    BUILDERS[f"strips-{_o}"] = ("plain", functools.partial(strips, _o))
for _g in (False, True):
    for _o in ("ascending", "descending", "permuted"):
        BUILDERS[f"chain{'_gaps' if _g else ''}-{_o}"] = ("plain", functools.partial(chains, _o, _g))
BUILDERS["late_bridge"] = ("plain", late_bridge)
BUILDERS["blobs"] = ("plain", functools.partial(blobs, False))
BUILDERS["blobs-permuted"] = ("plain", functools.partial(blobs, True))
BUILDERS["blob_satellites"] = ("plain", blob_satellites)
for _s in (False, True):
    _t = "next" if _s else "at"
    BUILDERS[f"lattice_half-{_t}"] = ("plain", functools.partial(lattice_half, _s))
    BUILDERS[f"lattice_tenth-{_t}"] = ("plain", functools.partial(lattice_tenth, _s))
    for _k in (1.0, 2.0, 0.5):
        BUILDERS[f"pythagorean-{_k}-{_t}"] = ("plain", functools.partial(pythagorean, _k, _s))
for _d in (1e-30, 1e-20, 0.0, -1.0):
    BUILDERS[f"triples-{_d}"] = ("plain", functools.partial(triples, _d))
BUILDERS["nonfinite_rows"] = ("plain", nonfinite_rows)
BUILDERS["nonfinite_tile"] = ("plain", nonfinite_tile)
for _c in (2, 5):
    BUILDERS[f"columns-{_c}"] = ("plain", functools.partial(columns, _c))
for _s in (2, 3):
    BUILDERS[f"batch_shared-{_s}"] = ("batched", functools.partial(batch_shared, _s))
BUILDERS["group_sorted"] = ("grouped", group_sorted)
BUILDERS["group_unsorted"] = ("grouped", group_unsorted)
BUILDERS["group_permuted"] = ("grouped", group_permuted)
BUILDERS["group_strips"] = ("grouped", group_strips)
BUILDERS["group_same_coordinates"] = ("grouped", functools.partial(group_same_coordinates, False))
BUILDERS["group_same_coordinates-interleaved"] = ("grouped", functools.partial(group_same_coordinates, True))
BUILDERS["group_single_member"] = ("grouped", group_single_member)
BUILDERS["group_one_entry_table"] = ("grouped", group_one_entry_table)

NAMES = tuple(BUILDERS)
MAX_POINTS = 6000


@functools.lru_cache(maxsize=None)
def case(name):
    kind, fn = BUILDERS[name]
    points, d, idx = fn()
    points = np.ascontiguousarray(points, F32)
    n = points.shape[0]
    assert n <= MAX_POINTS and (np.isfinite(points[:, :2]).all() or n <= 4096), name  # (the k-d tree path takes no NaN)
    out = dict(name=name, kind=kind, points=points, dist=None, idx=None, table=None)
    if kind == "plain":
        out["dist"], out["want"] = float(d), plain(points, d)
    elif kind == "batched":
        out["dist"], out["idx"], out["want"] = float(d), idx.astype(np.int32), batched(points, idx, d)
    else:
        table = np.asarray(d, F32)
        assert idx.min() >= 0 and idx.max() < table.size, name  # (ids outside the table are the caller's contract: never tried)
        out["table"], out["idx"], out["want"] = table, idx.astype(np.int32), grouped(points, idx, table)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- path witnesses (dense, n <= 4096) -------------------------------------------------------------------------------------------

def row_distance(c):
    """float32 [n]: the distance each row links at (the case's dist, or its group's)."""
    n = c["points"].shape[0]
    return np.full(n, c["dist"], F32) if c["kind"] != "grouped" else c["table"][c["idx"]]


def links(c):
    """bool [n, n], upper triangle: the pairs the referee's fp32 expression links (same sample / group, distance > 0)."""
    p = torch.from_numpy(c["points"][:, :2].copy())
    d = p[:, None, :] - p[None, :, :]
    d = ((d ** 2).sum(2) ** 0.5).numpy()
    rd = row_distance(c)
    adj = (d < rd[:, None]) & (rd[:, None] > 0)
    if c["idx"] is not None:
        adj &= c["idx"][:, None] == c["idx"][None, :]
    return np.triu(adj, 1)


def tile_count(n):
    return (n + TILE - 1) // TILE


def links_per_tile_pair(c):
    """int [tiles, tiles]: links (i in tile ti) x (j in tile tj), i < j."""
    a = links(c)
    t = tile_count(a.shape[0])
    pad = t * TILE - a.shape[0]
    a = np.pad(a, ((0, pad), (0, pad)))
    return a.reshape(t, TILE, t, TILE).sum((1, 3))


def tile_boxes(points):
    """f32 [tiles, 4] (xmin, xmax, ymin, ymax) over each tile's rows, NaN ignored as fminf / fmaxf do."""
    t = tile_count(points.shape[0])
    out = np.empty((t, 4), F32)
    for k in range(t):
        q = points[k * TILE:(k + 1) * TILE, :2]
        with np.errstate(all="ignore"):
            out[k] = [np.fmin.reduce(q[:, 0]), np.fmax.reduce(q[:, 0]), np.fmin.reduce(q[:, 1]), np.fmax.reduce(q[:, 1])]
    return out


def tile_gaps(points):
    """f32 [tiles, tiles]: the separation of two tiles' boxes along the axis that separates them most (<= 0: they overlap)."""
    b = tile_boxes(points)
    gx = np.maximum(b[None, :, 0] - b[:, None, 1], b[:, None, 0] - b[None, :, 1])
    gy = np.maximum(b[None, :, 2] - b[:, None, 3], b[:, None, 2] - b[None, :, 3])
    return np.maximum(gx, gy)


def tile_group_ranges(idx):
    t = tile_count(idx.shape[0])
    return np.array([[idx[k * TILE:(k + 1) * TILE].min(), idx[k * TILE:(k + 1) * TILE].max()] for k in range(t)])
