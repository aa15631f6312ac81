"""Site sets and convolution geometries for the rulebook kernels (K7/K8, fullysparsefusion_amd/csrc/rulebook.hip: fsf_rulebook_subm,
fsf_rulebook_strided, fsf_rulebook_to_pairs, fsf_order_by_neighbor_mask + fsf_remap_indices) that reach the kernels' decisions one by
one, and the referee they are judged by: shared by tests/test_rulebook_cases_cpu.py (the source pin, the path witnesses, the referee
against the oracle, a numpy model of the device algorithm with switchable defects) and tests/test_rulebook_gpu.py.  No GPU and no
product import here.

Referee.  `dense_referee` scatters the row ids into a dense [B, Z, Y, X] array of -1 and READS, for every output cell and offset k,
the input cell o * stride - pad + k * dil: the convolution's definition.  The kernels and `oracle.spconv.build_rulebook` work the
other way round (an input proposes an output through (in + pad - k * dil) % stride == 0), so a mistake in that rule is not shared.
An output site is a cell with at least one hit, output rows run in ascending linear (b, z, y, x) order (the order the cells are
walked in), the inverse table is the transpose of the forward one, the submanifold table is the same read at the input sites.
The grids of `wide_keys` hold more than 2^32 cells: there the referee is the oracle (int64 throughout) on the huge grid, and the
CPU test shows that it gives the tables of the same two site clusters laid into the interior of a small grid (translation by a
multiple of the stride, away from every border), where the dense referee applies.

A case is a dict: name, group, batch B, grid `shape`, the strided geometry (ksize, stride, padding, dilation), the submanifold
geometry (subm_ksize, subm_dilation), the sites `idx` int32 [m, 4] (b, z, y, x) without duplicates, the path tags it must reach
(`tags`) and `dense` (whether the grid fits the dense referee).  Every case goes through every entry point; a case made for one of them carries the default geometry of the others (3 x 3 x 3, stride 2, padding 1).
Cases are built from their names, one at a time (`case(name)`, cached), and must not be written to."""
import functools
import math

import numpy as np

from oracle import spconv as osp

# restated from csrc/rulebook.hip, csrc/common.h and csrc/radix_sort.h (pinned by
# test_rulebook_cases_cpu.py::test_constants_and_rules_equal_the_kernel_source)
RBP_SEG = 256              # rows per counting segment of fsf_rulebook_to_pairs
BLOCK = 256                # threads per workgroup, every kernel of the file
STREAM_GRID_MAX = 2048     # fsf_stream_grid: workgroups of a grid-stride launch
LDS_NO_ATTRIBUTE = 64 * 1024   # dynamic + static LDS a launch gets without a function attribute
HASH_CAP_FLOOR = 1024      # pow2_at_least
RADIX_BITS = 8             # key bits per pass of the radix sort
POISON = 0x5A5A5A5A

DEFAULT = dict(ksize=(3, 3, 3), stride=(2, 2, 2), padding=(1, 1, 1), dilation=(1, 1, 1), subm_ksize=(3, 3, 3), subm_dilation=(1, 1, 1))


# ---- launch rules ----------------------------------------------------------------------------------------------------------------

def hash_mix(k):
    """hash_mix of rulebook.hip on numpy uint64 (wrapping multiplication)."""
    k = np.asarray(k).astype(np.uint64)
    with np.errstate(over="ignore"):
        k = k ^ (k >> np.uint64(33))
        k = k * np.uint64(0xff51afd7ed558ccd)
        k = k ^ (k >> np.uint64(33))
        k = k * np.uint64(0xc4ceb9fe1a85ec53)
        k = k ^ (k >> np.uint64(33))
    return k


def pow2_at_least(v):
    p = HASH_CAP_FLOOR
    while p < v:
        p <<= 1
    return p


def per_in(ksize, stride, dilation):
    """Distinct output sites one input can propose: per axis, the offsets k with (in + pad - k * dil) % stride == 0."""
    n = 1
    for k, s, d in zip(ksize, stride, dilation):
        period = s // math.gcd(s, d)
        n *= (k + period - 1) // period
    return n


def rows_kernel_lds(p):
    return BLOCK * p * 8


def proposes_by_pair(p):
    return rows_kernel_lds(p) + 8 > LDS_NO_ATTRIBUTE


def stream_grid(items):
    return max(1, min((items + BLOCK - 1) // BLOCK, STREAM_GRID_MAX))


def sort_passes(cells):
    return -(-max(int(cells) - 1, 0).bit_length() // RADIX_BITS)


def out_shape(shape, ksize, stride, padding, dilation):
    return [(shape[j] + 2 * padding[j] - dilation[j] * (ksize[j] - 1) - 1) // stride[j] + 1 for j in range(3)]


def lin(idx, shape):
    idx = np.asarray(idx).astype(np.int64)
    return ((idx[:, 0] * shape[0] + idx[:, 1]) * shape[1] + idx[:, 2]) * shape[2] + idx[:, 3]


def unlin(v, shape):
    v = np.asarray(v).astype(np.int64).copy()
    x = v % shape[2]
    v //= shape[2]
    y = v % shape[1]
    v //= shape[1]
    return np.stack([v // shape[0], v % shape[0], y, x], 1)


# ---- the referee -----------------------------------------------------------------------------------------------------------------

def _offsets(ksize):
    return [(a, b, c) for a in range(ksize[0]) for b in range(ksize[1]) for c in range(ksize[2])]


def _dense_read(grid, cells, ksize, stride, padding, dilation):
    """table[o, k] = grid[b, o * stride - pad + k * dil] (-1 outside the grid) for the cells [n, 4] (b, oz, oy, ox)."""
    shape = grid.shape[1:]
    table = np.full((cells.shape[0], len(_offsets(ksize))), -1, np.int64)
    for k, off in enumerate(_offsets(ksize)):
        pos = [cells[:, 1 + j] * stride[j] - padding[j] + off[j] * dilation[j] for j in range(3)]
        ok = np.ones(cells.shape[0], bool)
        for j in range(3):
            ok &= (pos[j] >= 0) & (pos[j] < shape[j])
        table[ok, k] = grid[cells[ok, 0], pos[0][ok], pos[1][ok], pos[2][ok]]
    return table


def _dense_grid(idx, batch, shape):
    grid = np.full((batch,) + tuple(shape), -1, np.int64)
    idx = np.asarray(idx).astype(np.int64)
    grid[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = np.arange(idx.shape[0])
    return grid


def transpose_table(nbr, m_in):
    inv = np.full((m_in, nbr.shape[1]), -1, np.int32)
    o, k = np.nonzero(nbr >= 0)
    inv[nbr[o, k], k] = o
    return inv


def dense_subm(idx, batch, shape, ksize, dilation):
    pad = [dilation[j] * (ksize[j] - 1) // 2 for j in range(3)]
    return _dense_read(_dense_grid(idx, batch, shape), np.asarray(idx).astype(np.int64), ksize, (1, 1, 1), pad, dilation).astype(np.int32)


def dense_strided(idx, batch, shape, ksize, stride, padding, dilation):
    """(out_indices int32 [m_out, 4], nbr int32 [m_out, kvol], nbr_inv int32 [m, kvol], out_shape)."""
    oshape = out_shape(shape, ksize, stride, padding, dilation)
    cells = np.stack(np.meshgrid(*[np.arange(n) for n in [batch] + oshape], indexing="ij"), -1).reshape(-1, 4).astype(np.int64)
    table = _dense_read(_dense_grid(idx, batch, shape), cells, ksize, stride, padding, dilation)
    keep = (table >= 0).any(1)
    nbr = table[keep].astype(np.int32)
    return cells[keep].astype(np.int32), nbr, transpose_table(nbr, np.asarray(idx).shape[0]), oshape


def oracle_subm(idx, batch, shape, ksize, dilation):
    pad = [dilation[j] * (ksize[j] - 1) // 2 for j in range(3)]
    _, pairs, _ = osp.build_rulebook(idx, batch, list(shape), ksize, (1, 1, 1), pad, dilation, True)
    return osp.pairs_to_nbr(pairs, np.asarray(idx).shape[0])


def oracle_strided(idx, batch, shape, ksize, stride, padding, dilation):
    out_idx, pairs, oshape = osp.build_rulebook(idx, batch, list(shape), ksize, stride, padding, dilation, False)
    return out_idx, osp.pairs_to_nbr(pairs, out_idx.shape[0]), osp.pairs_inverse_nbr(pairs, np.asarray(idx).shape[0]), list(oshape)


def table_pairs(nbr):
    """spconv v1 pair lists of a table: per offset (in rows, out rows) in ascending out row, and their number."""
    out = []
    for k in range(nbr.shape[1]):
        o = np.nonzero(nbr[:, k] >= 0)[0]
        out.append((nbr[o, k].astype(np.int32), o.astype(np.int32)))
    return out


def popcount(v):
    v = np.asarray(v).astype(np.uint64)
    n = np.zeros(v.shape, np.int64)
    for b in range(27):
        n += ((v >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    return n


def mask_order_key(nbr27):
    """(key, mid, lo, hi) of fsf_order_by_neighbor_mask from a 3 x 3 x 3 submanifold table."""
    mask = ((nbr27 >= 0).astype(np.int64) << np.arange(27)).sum(1)
    mid, lo, hi = (mask >> 9) & 511, np.minimum(popcount(mask & 511), 7), np.minimum(popcount(mask >> 18), 15)
    return (mid << 7) | (lo << 4) | hi, mid, lo, hi


def mask_order(idx, nbr27):
    """The expected permutation: descending key, then coordinate parity, then row (the expression of
    tests/test_fullsize_gpu.py::test_order_by_neighbor_mask_is_a_stable_sort_by_its_key)."""
    idx = np.asarray(idx)
    n = idx.shape[0]
    key = mask_order_key(nbr27)[0]
    parity = (idx[:, 1] & 1) * 4 + (idx[:, 2] & 1) * 2 + (idx[:, 3] & 1)
    return np.lexsort((np.arange(n), parity, -key))


@functools.lru_cache(maxsize=None)
def expected(name):
    """Everything the GPU test compares with, computed once per case: the dense referee where the grid fits, else the oracle."""
    c = case(name)
    idx, b, shape = c["idx"], c["batch"], c["shape"]
    if c["dense"]:
        subm = dense_subm(idx, b, shape, c["subm_ksize"], c["subm_dilation"])
        strided = dense_strided(idx, b, shape, c["ksize"], c["stride"], c["padding"], c["dilation"])
        nbr27 = subm if tuple(c["subm_ksize"]) == (3, 3, 3) and tuple(c["subm_dilation"]) == (1, 1, 1) else dense_subm(idx, b, shape, (3, 3, 3), (1, 1, 1))
    else:
        subm = oracle_subm(idx, b, shape, c["subm_ksize"], c["subm_dilation"])
        strided = oracle_strided(idx, b, shape, c["ksize"], c["stride"], c["padding"], c["dilation"])
        nbr27 = subm
    out = dict(subm=subm, out_indices=strided[0], nbr=strided[1], nbr_inv=strided[2], out_shape=strided[3], nbr27=nbr27,
               perm=mask_order(idx, nbr27))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- path model ------------------------------------------------------------------------------------------------------------------

FULL_TAGS = frozenset({
    # which kernel proposes the output sites, and how full its LDS list may get
    "propose_rows", "propose_rows_lds_over_48k", "propose_rows_lds_61440", "propose_by_pair", "per_in_8", "per_in_27",
    # geometry
    "strided_dilation", "subm_dilation", "stride_dilation_share_a_factor", "anisotropic", "stride_3", "stride_1_strided",
    "even_kernel", "kvol_1", "no_padding", "corner_sites", "same_site_in_two_batches",
    # degenerate results
    "m_out_zero", "inverse_dead_rows",
    # fsf_rulebook_to_pairs
    "pairs_single_partial_segment", "pairs_whole_segments", "pairs_partial_last_segment", "pairs_before_second_trip",
    "pairs_kvol_second_trip", "pairs_empty_offset", "pairs_dead_row",
    # hash tables
    "cap_1024_load_half", "cap_2048_smallest", "hash_wrap_inputs", "hash_wrap_outputs",
    # grid-stride loops and key widths
    "stream_grid_capped", "lin_in_over_32_bits", "lin_out_over_32_bits", "sort_passes_5", "sort_passes_up_to_4",
    # fsf_order_by_neighbor_mask
    "mo_single_row", "mo_odd_m", "mo_even_m", "mo_second_round", "mo_full_row", "mo_lone_row", "mo_lo_saturates", "mo_hi_9",
    "mo_all_parities"})


def wrap_forced(keys, cap):
    """More keys have their home in the last three slots of a `cap`-slot table than there are slots there."""
    return int((hash_mix(keys) & np.uint64(cap - 1) >= np.uint64(cap - 3)).sum()) > 3


def paths(c):
    """The decisions of rulebook.hip the case reaches, from its numbers and its referee tables."""
    e = expected(c["name"])
    idx, b, shape = c["idx"], c["batch"], c["shape"]
    m, m_out = idx.shape[0], e["nbr"].shape[0]
    kvol = int(np.prod(c["ksize"]))
    tags = set()
    p = per_in(c["ksize"], c["stride"], c["dilation"])
    if proposes_by_pair(p):
        tags.add("propose_by_pair")
    else:
        tags.add("propose_rows")
        if rows_kernel_lds(p) > 48 * 1024:
            tags.add("propose_rows_lds_over_48k")
        if rows_kernel_lds(p) == 61440:
            tags.add("propose_rows_lds_61440")
    if p in (8, 27):
        tags.add("per_in_%d" % p)
    if max(c["dilation"]) > 1:
        tags.add("strided_dilation")
    if max(c["subm_dilation"]) > 1:
        tags.add("subm_dilation")
    if any(math.gcd(s, d) > 1 for s, d in zip(c["stride"], c["dilation"])):
        tags.add("stride_dilation_share_a_factor")
    if len(set(c["ksize"])) > 1 or len(set(c["stride"])) > 1 or len(set(c["subm_ksize"])) > 1:
        tags.add("anisotropic")
    if 3 in c["stride"]:
        tags.add("stride_3")
    if tuple(c["stride"]) == (1, 1, 1):
        tags.add("stride_1_strided")
    if any(k % 2 == 0 for k in c["ksize"]):
        tags.add("even_kernel")
    if int(np.prod(c["subm_ksize"])) == 1:
        tags.add("kvol_1")
    if tuple(c["padding"]) == (0, 0, 0) and max(c["ksize"]) > 1:
        tags.add("no_padding")
    corners = {(bb, z, y, x) for bb in (0, b - 1) for z in (0, shape[0] - 1) for y in (0, shape[1] - 1) for x in (0, shape[2] - 1)}
    sites = set(map(tuple, idx.tolist()))
    if corners <= sites:
        tags.add("corner_sites")
    if b > 1 and any((1,) + s[1:] in sites for s in sites if s[0] == 0):
        tags.add("same_site_in_two_batches")
    if m_out == 0:
        tags.add("m_out_zero")
    elif (e["nbr_inv"] < 0).all(1).any():
        tags.add("inverse_dead_rows")
    # fsf_rulebook_to_pairs runs on every table of the case
    for t in (e["subm"], e["nbr"], e["nbr_inv"]):
        rows, kv = t.shape
        if rows == 0:
            continue
        nseg = (rows + RBP_SEG - 1) // RBP_SEG
        if nseg == 1 and rows < RBP_SEG:
            tags.add("pairs_single_partial_segment")
        if rows % RBP_SEG == 0:
            tags.add("pairs_whole_segments")
        elif nseg > 1:
            tags.add("pairs_partial_last_segment")
        if nseg - 1 > BLOCK:   # the last segment sums the counts of more than 256 segments before it
            tags.add("pairs_before_second_trip")
        if kv > BLOCK:
            tags.add("pairs_kvol_second_trip")
        if kv > 1 and (t < 0).all(0).any():
            tags.add("pairs_empty_offset")
        if (t < 0).all(1).any():
            tags.add("pairs_dead_row")
    in_cap = pow2_at_least(2 * m)
    if m == 512 and in_cap == 1024:
        tags.add("cap_1024_load_half")
    if m == 513 and in_cap == 2048:
        tags.add("cap_2048_smallest")
    if wrap_forced(lin(idx, shape), in_cap):
        tags.add("hash_wrap_inputs")
    if m_out and wrap_forced(lin(e["out_indices"], e["out_shape"]), pow2_at_least(2 * m * p)):
        tags.add("hash_wrap_outputs")
    if max(m * kvol, m * int(np.prod(c["subm_ksize"])), m_out * kvol) > STREAM_GRID_MAX * BLOCK:
        tags.add("stream_grid_capped")
    if int(lin(idx, shape).max()) >= 2 ** 32:
        tags.add("lin_in_over_32_bits")
    if m_out:
        if int(lin(e["out_indices"], e["out_shape"]).max()) >= 2 ** 32:
            tags.add("lin_out_over_32_bits")
        n = sort_passes(b * int(np.prod(e["out_shape"])))
        tags.add("sort_passes_5" if n == 5 else "sort_passes_up_to_4")
        assert n <= 5
    # fsf_order_by_neighbor_mask: half a wave per row, 2048 workgroups * 256 / 32 halves per round
    if m == 1:
        tags.add("mo_single_row")
    tags.add("mo_odd_m" if m % 2 else "mo_even_m")
    if m > stream_grid(m * 32) * BLOCK // 32:
        tags.add("mo_second_round")
    _, mid, lo, hi = mask_order_key(e["nbr27"])
    full = (e["nbr27"] >= 0).all(1)
    if full.any():
        tags.add("mo_full_row")
        assert (mid[full] == 511).all()
    if ((e["nbr27"] >= 0).sum(1) == 1).any():
        tags.add("mo_lone_row")
    if (popcount(((e["nbr27"][:, :9] >= 0).astype(np.int64) << np.arange(9)).sum(1)) > 7).any():
        tags.add("mo_lo_saturates")
    if ((hi == 9) & (lo == 7)).any():
        tags.add("mo_hi_9")
    if len({tuple(r) for r in (idx[:, 1:] & 1).tolist()}) == 8:
        tags.add("mo_all_parities")
    return tags


# ---- site sets -------------------------------------------------------------------------------------------------------------------

def _sorted_sites(sites, shape):
    arr = np.array(sorted(set(map(tuple, sites))), dtype=np.int64).reshape(-1, 4)
    assert ((arr[:, 1:] >= 0) & (arr[:, 1:] < np.asarray(shape))).all() and (arr[:, 0] >= 0).all()
    return arr.astype(np.int32)


def geometry_sites(shape=(9, 14, 11), batch=2, seed=0):
    """The eight grid corners of both batches, a dense 4 x 4 x 4 cube at the top of batch 0 and the same cube at the bottom of batch 1
    (the same (y, x): with OZ in place of Z in the input linearisation the two collide), a site that both batches hold, random fill."""
    z, y, x = shape
    sites = [(b, cz, cy, cx) for b in range(batch) for cz in (0, z - 1) for cy in (0, y - 1) for cx in (0, x - 1)]
    for dz in range(min(4, z)):
        for dy in range(4):
            for dx in range(4):
                sites.append((0, z - 1 - dz, 5 + dy, 3 + dx))
                sites.append((batch - 1, dz, 5 + dy, 3 + dx))
    rng = np.random.default_rng(seed)
    cells = rng.choice(z * y * x, size=z * y * x // 8, replace=False)
    for cidx in cells.tolist():
        s = (cidx // (y * x), (cidx // x) % y, cidx % x)
        sites.append((int(rng.integers(batch)),) + s)
    for s in [(2, 2, 2), (z // 2, y - 1, x - 1), (z - 1, 0, x // 2)]:
        sites += [(b,) + s for b in range(batch)]
    # the first and the last cell of every row of the bottom layer: a read at x = X that is not refused lands on the next row's site
    sites += [(0, 0, yy, xx) for yy in range(y) for xx in (0, x - 1)]
    return _sorted_sites(sites, shape)


def random_sites(m, shape, batch, seed):
    rng = np.random.default_rng(seed)
    cells = batch * int(np.prod(shape))
    return unlin(np.sort(rng.choice(cells, size=m, replace=False)), shape).astype(np.int32)


def sheet_sites(m, side):
    """A thin sheet: the first m cells of a one-cell-high side x side layer, one batch."""
    v = np.arange(m)
    return np.stack([np.zeros(m, np.int64), np.zeros(m, np.int64), v // side, v % side], 1).astype(np.int32)


def spread_sites(m, shape, batch):
    """No two sites adjacent: every third cell of every third row of every third layer."""
    sites = [(b, z, y, x) for b in range(batch) for z in range(0, shape[0], 3) for y in range(0, shape[1], 3) for x in range(0, shape[2], 3)]
    return _sorted_sites(sites[:m], shape)


def wrap_sites(shape, batch, cap, n_last=12, fill_slots=9, per_slot=2):
    """Cells of the grid whose home slot in a `cap`-slot table is one of the last three (n_last of them) or one of the first
    `fill_slots` (`per_slot` each): the probe chain of the former wraps past slot cap - 1 and displaces the latter in turn."""
    cells = np.arange(batch * int(np.prod(shape)), dtype=np.int64)
    home = (hash_mix(cells) & np.uint64(cap - 1)).astype(np.int64)
    pick = list(cells[home >= cap - 3][:n_last])
    assert len(pick) == n_last
    for s in range(fill_slots):
        pick += list(cells[home == s][:per_slot])
    return np.sort(np.array(pick, np.int64))


def delta_of(value, shape):
    """(db, dz, dy, dx) with lin(site + delta) - lin(site) == value."""
    return tuple(int(v) for v in unlin(np.array([value]), shape)[0])


WIDE_GRIDS = {"wide_keys_av2": ((41, 40000, 40000), 2), "wide_keys_batch": ((41, 2000, 2000), 2000)}
WIDE_SMALL = ((41, 48, 48), 2)   # the small grid the same clusters are laid into (translation invariance)


def wide_clusters(seed=5):
    """The two clusters of a wide-key case, relative to their anchors: `main`, about 400 sites of a 12 x 12 x 12 block; `ghost`, for
    every main site s and in-plane offset n with s + n empty, the site s + n (to be shifted back by 2^32 cells)."""
    rng = np.random.default_rng(seed)
    block = rng.random((12, 12, 12)) < 0.16
    block[4:8, 4:8, 4:8] = True
    main = np.argwhere(block)
    occupied = set(map(tuple, main.tolist()))
    ghost = set()
    for s in main[::9].tolist():
        for n in ((0, 0, 1), (0, 1, 0), (0, -1, 1)):
            t = (s[0] + n[0], s[1] + n[1], s[2] + n[2])
            if t not in occupied and min(t) >= 0 and max(t) < 12:
                ghost.add(t)
    return main, np.array(sorted(ghost))


def wide_sites(shape, batch, small=False):
    """`main` in the far corner of the last batch, 16 cells (a multiple of every stride used) away from the borders; `ghost` exactly
    2^32 linear cells before the empty cells next to `main` it mirrors: a 32-bit input key makes each ghost the neighbour of a main
    site.  small=True: the same two clusters in the interior of WIDE_SMALL (ghost first, as in the huge grid)."""
    main, ghost = wide_clusters()
    z, y, x = shape
    a_main = (batch - 1, z - 12 - 5, y - 12 - 16, x - 12 - 16)
    a_main = (a_main[0], a_main[1] - a_main[1] % 2, a_main[2] - a_main[2] % 2, a_main[3] - a_main[3] % 2)
    d = delta_of(2 ** 32, shape)
    a_ghost = tuple(a - dd for a, dd in zip(a_main, d))
    assert d[2] > 40 and a_main[1] == 24   # the ghost lies in rows (y) far below the main cluster's: the row order is (b, z, then y)
    if small:
        # same batch relation, same z offset, same parities, the ghost in lower rows (y): the same row order and the same tables
        (z, y, x), b = WIDE_SMALL
        a_ghost = (b - 1 if d[0] == 0 else 0, 24 - d[1], 8 + (a_ghost[2] - 8) % 2, 8 + (a_ghost[3] - 8) % 2)
        a_main = (b - 1, 24, 24, 24)
    sites = [(a_main[0], a_main[1] + s[0], a_main[2] + s[1], a_main[3] + s[2]) for s in main.tolist()]
    sites += [(a_ghost[0], a_ghost[1] + s[0], a_ghost[2] + s[1], a_ghost[3] + s[2]) for s in ghost.tolist()]
    return _sorted_sites(sites, (z, y, x))


# ---- the cases -------------------------------------------------------------------------------------------------------------------

# name -> (ksize, stride, padding, dilation, tags)
STRIDED_GEOMETRIES = {
    "k3_s2_p1": ((3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 1, 1), {"propose_rows", "per_in_8", "corner_sites", "same_site_in_two_batches"}),
    "k3_s2_p011": ((3, 3, 3), (2, 2, 2), (0, 1, 1), (1, 1, 1), {"per_in_8"}),
    "k3_s2_p0": ((3, 3, 3), (2, 2, 2), (0, 0, 0), (1, 1, 1), {"no_padding"}),
    "k3_s1_p1": ((3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), {"per_in_27", "stride_1_strided", "propose_rows_lds_over_48k"}),
    "k3_s2_p2_d2": ((3, 3, 3), (2, 2, 2), (2, 2, 2), (2, 2, 2), {"per_in_27", "stride_dilation_share_a_factor", "strided_dilation"}),
    "k3_s2_p3_d3": ((3, 3, 3), (2, 2, 2), (3, 3, 3), (3, 3, 3), {"strided_dilation", "per_in_8"}),
    "k5_s3_p2_d2": ((5, 5, 5), (3, 3, 3), (2, 2, 2), (2, 2, 2), {"stride_3", "strided_dilation", "per_in_8"}),
    "k311_s211_p0": ((3, 1, 1), (2, 1, 1), (0, 0, 0), (1, 1, 1), {"anisotropic"}),
    "k133_s122_p011": ((1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 1, 1), {"anisotropic"}),
    "k2_s2_p0": ((2, 2, 2), (2, 2, 2), (0, 0, 0), (1, 1, 1), {"even_kernel"}),
    "k532_s1_p0": ((5, 3, 2), (1, 1, 1), (0, 0, 0), (1, 1, 1), {"propose_rows_lds_61440", "even_kernel", "anisotropic"}),
    "k442_s1_p0": ((4, 4, 2), (1, 1, 1), (0, 0, 0), (1, 1, 1), {"propose_by_pair", "even_kernel"}),
    "k5_s1_p2": ((5, 5, 5), (1, 1, 1), (2, 2, 2), (1, 1, 1), {"propose_by_pair", "stride_1_strided"}),
}
# name -> (ksize, dilation, tags)
SUBM_GEOMETRIES = {
    "k3": ((3, 3, 3), (1, 1, 1), {"corner_sites"}),
    "k3_d2": ((3, 3, 3), (2, 2, 2), {"subm_dilation"}),
    "k5": ((5, 5, 5), (1, 1, 1), set()),
    "k311": ((3, 1, 1), (1, 1, 1), {"anisotropic"}),
    "k133": ((1, 3, 3), (1, 1, 1), {"anisotropic"}),
    "k1": ((1, 1, 1), (1, 1, 1), {"kvol_1"}),
}
SEG_EDGE_M = (255, 256, 257, 512, 513)
SHEET_PAIRS_M = 65537 + 256   # 258 segments of 256 rows
SHEET_MASK_M = 16385          # 2048 workgroups * 256 / 32 halves + 1, odd
MASK_ORDER_M = (1, 2, 63, 64, 65)
NO_OUTPUT = dict(shape=(4, 6, 6), batch=2, ksize=(3, 3, 3), stride=(2, 2, 2), padding=(0, 0, 0), dilation=(1, 1, 1))


def _names():
    names = ["geometry-strided-" + g for g in STRIDED_GEOMETRIES] + ["geometry-subm-" + g for g in SUBM_GEOMETRIES]
    names += ["no_output-all", "no_output-half"]
    names += ["seg_edges-m%d" % m for m in SEG_EDGE_M] + ["seg_edges-sheet", "seg_edges-spread", "seg_edges-k7"]
    names += ["hash_wrap-inputs", "hash_wrap-outputs"]
    names += list(WIDE_GRIDS)
    names += ["mask_order-m%d" % m for m in MASK_ORDER_M] + ["mask_order-cube5", "mask_order-lone", "mask_order-sheet"]
    return names


ALL = tuple(_names())
DENSE = tuple(n for n in ALL if n not in WIDE_GRIDS)


def _make(name):
    group, _, rest = name.partition("-")
    c = dict(DEFAULT, name=name, group=group, batch=2, tags=set(), dense=True)
    if group == "geometry":
        kind, _, g = rest.partition("-")
        c.update(shape=(9, 14, 11), idx=geometry_sites())
        if kind == "strided":
            ks, st, pd, dl, tags = STRIDED_GEOMETRIES[g]
            c.update(ksize=ks, stride=st, padding=pd, dilation=dl, tags=set(tags))
        else:
            ks, dl, tags = SUBM_GEOMETRIES[g]
            c.update(subm_ksize=ks, subm_dilation=dl, tags=set(tags))
    elif group == "no_output":
        c.update(NO_OUTPUT)
        sites = [(b, 3, y, x) for b in range(2) for y in range(6) for x in range(0, 6, 2)]
        if rest == "half":
            sites += [(b, z, y, x) for b in range(2) for z in (0, 2) for y in range(1, 6, 2) for x in range(1, 6, 2)]
        c.update(idx=_sorted_sites(sites, c["shape"]),
                 tags={"m_out_zero", "no_padding"} if rest == "all" else {"inverse_dead_rows", "pairs_dead_row", "no_padding"})
    elif group == "seg_edges":
        if rest == "sheet":
            c.update(shape=(2, 260, 260), batch=1, idx=sheet_sites(SHEET_PAIRS_M, 260),
                     tags={"pairs_before_second_trip", "stream_grid_capped", "mo_second_round", "pairs_partial_last_segment"})
        elif rest == "spread":
            c.update(shape=(7, 13, 13), idx=spread_sites(100, (7, 13, 13), 2), tags={"pairs_empty_offset", "mo_lone_row"})
        elif rest == "k7":
            c.update(shape=(8, 12, 10), idx=random_sites(300, (8, 12, 10), 2, 7), subm_ksize=(7, 7, 7), tags={"pairs_kvol_second_trip"})
        else:
            m = int(rest[1:])
            tags = {255: {"pairs_single_partial_segment"}, 256: {"pairs_whole_segments"}, 257: {"pairs_partial_last_segment"},
                    512: {"pairs_whole_segments", "cap_1024_load_half"}, 513: {"pairs_partial_last_segment", "cap_2048_smallest"}}[m]
            c.update(shape=(8, 12, 10), idx=random_sites(m, (8, 12, 10), 2, m), tags=tags)
    elif group == "hash_wrap":
        if rest == "inputs":
            shape = (16, 64, 64)
            c.update(shape=shape, idx=unlin(wrap_sites(shape, 2, 1024), shape).astype(np.int32), tags={"hash_wrap_inputs"})
        else:
            # inputs at all-even coordinates propose exactly one output site each (stride 2, padding 1: only the centre offset passes
            # the stride test), the cell at half their coordinates: the OUTPUT cells are the crafted set, set_cap = pow2(2 * m * 8)
            shape, oshape = (16, 64, 64), (8, 32, 32)
            out_cells = unlin(wrap_sites(oshape, 2, 1024, n_last=12, fill_slots=9, per_slot=2), oshape)
            idx = out_cells.copy()
            idx[:, 1:] *= 2
            c.update(shape=shape, idx=_sorted_sites(idx.tolist(), shape), tags={"hash_wrap_outputs"})
    elif group in ("wide_keys_av2", "wide_keys_batch"):
        shape, batch = WIDE_GRIDS[name]
        c.update(shape=shape, batch=batch, idx=wide_sites(shape, batch), dense=False,
                 tags={"lin_in_over_32_bits", "lin_out_over_32_bits"} | ({"sort_passes_5"} if name == "wide_keys_av2" else set()))
    elif group == "mask_order":
        if rest == "cube5":
            sites = [(0, 2 + z, 3 + y, 4 + x) for z in range(5) for y in range(5) for x in range(5)]
            c.update(shape=(9, 12, 12), batch=1, idx=_sorted_sites(sites, (9, 12, 12)),
                     tags={"mo_full_row", "mo_lo_saturates", "mo_hi_9", "mo_all_parities", "mo_odd_m"})
        elif rest == "lone":
            c.update(shape=(7, 13, 13), idx=spread_sites(45, (7, 13, 13), 2), tags={"mo_lone_row", "mo_all_parities"})
        elif rest == "sheet":
            c.update(shape=(2, 130, 130), batch=1, idx=sheet_sites(SHEET_MASK_M, 130), tags={"mo_second_round", "mo_odd_m"})
        else:
            m = int(rest[1:])
            c.update(shape=(4, 6, 6), idx=random_sites(m, (4, 6, 6), 2, 100 + m),
                     tags={"mo_single_row"} if m == 1 else {"mo_odd_m" if m % 2 else "mo_even_m"})
    else:
        raise KeyError(name)
    c["idx"].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    return _make(name)


# ---- a numpy model of the device algorithm, with switchable defects ----------------------------------------------------------------

DEFECTS = ("bounds_x", "lin_in_u32", "oz_for_z", "inverse_ignores_dilation", "stride_test_one_axis", "before_first_256",
           "probe_no_wrap", "m_out_zero_unwritten")


class HashTable:
    """Open addressing with linear probing as rulebook.hip does it (any winner of a contended slot: the lookups do not depend on it).
    wrap=False: a chain that reaches the table's end falls off it; its key is never found (on the device: an access out of bounds)."""

    def __init__(self, cap, wrap=True):
        self.cap, self.wrap = cap, wrap
        self.keys = np.full(cap, np.uint64(2 ** 64 - 1), np.uint64)
        self.vals = np.full(cap, -1, np.int64)

    def insert(self, keys, vals):
        keys = np.asarray(keys).astype(np.uint64)
        vals = np.asarray(vals).astype(np.int64)
        slot = (hash_mix(keys) & np.uint64(self.cap - 1)).astype(np.int64)
        live = np.arange(keys.shape[0])
        while live.size:
            s = slot[live]
            inside = s < self.cap
            live, s = live[inside], s[inside]
            empty = self.keys[s] == np.uint64(2 ** 64 - 1)
            _, first = np.unique(s[empty], return_index=True)      # one claimant per empty slot
            win = live[empty][first]
            self.keys[slot[win]] = keys[win]
            hit = self.keys[s] == keys[live]                          # the slot now holds this key (its own or an equal one: last writer)
            self.vals[s[hit]] = vals[live[hit]]
            live = live[~hit]
            slot[live] = slot[live] + 1 if not self.wrap else (slot[live] + 1) & (self.cap - 1)

    def lookup(self, keys):
        keys = np.asarray(keys).astype(np.uint64)
        out = np.full(keys.shape[0], -1, np.int64)
        slot = (hash_mix(keys) & np.uint64(self.cap - 1)).astype(np.int64)
        live = np.arange(keys.shape[0])
        while live.size:
            s = slot[live]
            inside = s < self.cap
            live, s = live[inside], s[inside]
            k = self.keys[s]
            hit = k == keys[live]
            out[live[hit]] = self.vals[s[hit]]
            live = live[~(hit | (k == np.uint64(2 ** 64 - 1)))]
            slot[live] = slot[live] + 1 if not self.wrap else (slot[live] + 1) & (self.cap - 1)
        return out


def _model_lin_in(b, z, y, x, shape, oshape, defect):
    zz = oshape[0] if defect == "oz_for_z" else shape[0]
    v = ((b.astype(np.uint64) * np.uint64(zz) + z.astype(np.uint64)) * np.uint64(shape[1]) + y.astype(np.uint64)) * np.uint64(shape[2]) + x.astype(np.uint64)
    return v & np.uint64(0xFFFFFFFF) if defect == "lin_in_u32" else v


def _model_read(idx_rows, table, shape, oshape, ksize, stride, padding, dilation, defect):
    """rb_subm_kernel / rb_strided_nbr_kernel: per (row, offset) a bounds test and a lookup of the input table."""
    out = np.full((idx_rows.shape[0], len(_offsets(ksize))), -1, np.int32)
    for k, off in enumerate(_offsets(ksize)):
        pos = [idx_rows[:, 1 + j] * stride[j] - padding[j] + off[j] * dilation[j] for j in range(3)]
        ok = np.ones(idx_rows.shape[0], bool)
        for j in range(3):
            ok &= pos[j] >= 0
            if not (defect == "bounds_x" and j == 2):
                ok &= pos[j] < shape[j]
        r = np.nonzero(ok)[0]
        out[r, k] = table.lookup(_model_lin_in(idx_rows[r, 0], pos[0][r], pos[1][r], pos[2][r], shape, oshape, defect))
    return out


def model_subm(c, defect=None):
    idx = c["idx"].astype(np.int64)
    m = idx.shape[0]
    pad = [c["subm_dilation"][j] * (c["subm_ksize"][j] - 1) // 2 for j in range(3)]
    table = HashTable(pow2_at_least(2 * m), wrap=defect != "probe_no_wrap")
    table.insert(_model_lin_in(idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3], c["shape"], c["shape"], defect), np.arange(m))
    return _model_read(idx, table, c["shape"], c["shape"], c["subm_ksize"], (1, 1, 1), pad, c["subm_dilation"], defect)


def model_strided(c, defect=None):
    """propose -> unique (the candidate set) -> radix sort by the key's low 8 * passes bits -> out-site map -> the two tables."""
    idx = c["idx"].astype(np.int64)
    m = idx.shape[0]
    shape, ks, st, pd, dl = c["shape"], c["ksize"], c["stride"], c["padding"], c["dilation"]
    kvol = len(_offsets(ks))
    oshape = out_shape(shape, ks, st, pd, dl)
    wrap = defect != "probe_no_wrap"
    in_table = HashTable(pow2_at_least(2 * m), wrap)
    in_table.insert(_model_lin_in(idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3], shape, oshape, defect), np.arange(m))

    def proposals(dil, one_axis):
        rows, ks_, keys = [], [], []
        for k, off in enumerate(_offsets(ks)):
            n = [idx[:, 1 + j] + pd[j] - off[j] * dil[j] for j in range(3)]
            ok = (n[0] >= 0) & (n[1] >= 0) & (n[2] >= 0)
            for j in range(3):
                if not one_axis or j == 0:
                    ok &= n[j] % st[j] == 0
            o = [n[j] // st[j] for j in range(3)]
            for j in range(3):
                ok &= o[j] < oshape[j]
            r = np.nonzero(ok)[0]
            rows.append(r)
            ks_.append(np.full(r.shape[0], k))
            keys.append(((idx[r, 0] * oshape[0] + o[0][r]) * oshape[1] + o[1][r]) * oshape[2] + o[2][r])
        return np.concatenate(rows), np.concatenate(ks_), np.concatenate(keys)

    one_axis = defect == "stride_test_one_axis"
    _, _, keys = proposals(dl, one_axis)
    set_cap = pow2_at_least(2 * m * per_in(ks, st, dl))
    out_table = HashTable(set_cap, wrap)
    out_table.insert(keys, np.zeros(keys.shape[0]))
    sites = np.unique(out_table.keys[out_table.keys != np.uint64(2 ** 64 - 1)]).astype(np.int64)
    m_out = sites.shape[0]
    nbr_inv = np.full((m, kvol), POISON, np.int32)
    if m_out == 0:
        if defect != "m_out_zero_unwritten":
            nbr_inv[:] = -1
        return np.zeros((0, 4), np.int32), np.zeros((0, kvol), np.int32), nbr_inv, oshape
    bits = RADIX_BITS * sort_passes(c["batch"] * int(np.prod(oshape)))
    sites = sites[np.argsort(sites & ((1 << bits) - 1), kind="stable")]
    out_table.insert(sites, np.arange(m_out))
    out_idx = unlin(sites, oshape)
    nbr = _model_read(out_idx, in_table, shape, oshape, ks, st, pd, dl, defect)
    rows, kk, keys = proposals((1, 1, 1) if defect == "inverse_ignores_dilation" else dl, one_axis)
    nbr_inv[:] = -1
    nbr_inv[rows, kk] = out_table.lookup(keys)
    return out_idx.astype(np.int32), nbr, nbr_inv, oshape


def model_pairs(nbr, defect=None):
    """rb_pairs_count_kernel + rb_pairs_fill_kernel: counts per 256-row segment, then every (segment, offset) compacts its rows
    behind the counts of the segments before it.  Returns (pairs int32 [kvol, 2, cap] pre-filled with -1, num [kvol])."""
    m_out, kvol = nbr.shape
    cap = max(m_out, 1)
    pairs = np.full((kvol, 2, cap), -1, np.int32)
    num = np.zeros(kvol, np.int32)
    if m_out == 0:
        return pairs, num
    nseg = (m_out + RBP_SEG - 1) // RBP_SEG
    live = np.zeros((nseg * RBP_SEG, kvol), bool)
    live[:m_out] = nbr >= 0
    cnt = live.reshape(nseg, RBP_SEG, kvol).sum(1)
    for seg in range(nseg):
        before = cnt[:min(seg, BLOCK) if defect == "before_first_256" else seg].sum(0)
        if seg == nseg - 1:
            num[:] = before + cnt[seg]
        rows = np.arange(seg * RBP_SEG, min((seg + 1) * RBP_SEG, m_out))
        for k in np.nonzero(cnt[seg])[0]:
            r = rows[nbr[rows, k] >= 0]
            pos = before[k] + np.arange(r.shape[0])
            pairs[k, 0, pos], pairs[k, 1, pos] = nbr[r, k], r
    return pairs, num
