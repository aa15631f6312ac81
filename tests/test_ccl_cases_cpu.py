"""CPU: what the device connected-components tests (tests/test_ccl_gpu.py) stand on.

* The referee helpers of tests/ccl_cases.py against a plain Python union-find over the referee's own fp32 pair decisions.
* Path witnesses: each layout family does reach the kernel path it is there for (tile pairs the box test prunes, a tile pair that
  overflows the link queue, pairs exactly at the threshold, a bridge that arrives last, group ranges that do not meet).  They are
  conditions on the inputs, derived with the kernel's constants.
* The constants themselves against csrc/ccl.hip, so that a retuned kernel gets its witnesses re-derived."""
import os
import re

import numpy as np
import pytest

import ccl_cases as C
from conftest import ROOT


def _union_find_labels(adj):
    """Labels by first member from the links of a boolean upper-triangular matrix."""
    n = adj.shape[0]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in zip(*np.nonzero(adj)):
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return C.number_by_first_member(np.array([find(i) for i in range(n)]))


SMALL = [n for n in C.NAMES if C.case(n)["points"].shape[0] <= 1500]


@pytest.mark.parametrize("name", SMALL)
def test_referee_equals_brute_force_union_find(name):
    c = C.case(name)
    np.testing.assert_array_equal(c["want"], _union_find_labels(C.links(c)))


def test_every_family_has_a_brute_force_checked_case_and_the_sizes_hold():
    assert {n.split("-")[0] for n in SMALL} >= {"tile_edges", "blobs", "pythagorean", "triples", "nonfinite_rows", "nonfinite_tile", "columns",
                                                "batch_shared", "group_same_coordinates", "group_single_member", "group_one_entry_table"}
    assert [C.case(f"tile_edges-{n}")["points"].shape[0] for n in C.TILE_EDGE_SIZES] == list(C.TILE_EDGE_SIZES)
    assert C.TILE_EDGE_SIZES == (2, C.TILE - 1, C.TILE, C.TILE + 1, C.CCL_TJ * C.TILE - 1, C.CCL_TJ * C.TILE, C.CCL_TJ * C.TILE + 1, 2049)
    for n in C.NAMES:
        assert C.case(n)["points"].shape[0] <= C.MAX_POINTS and C.case(n)["want"].dtype == np.int32


def test_constants_equal_the_kernel_source():
    src = open(os.path.join(ROOT, "fullysparsefusion_amd", "csrc", "ccl.hip")).read()
    assert int(re.search(r"constexpr int CCL_TJ = (\d+);", src).group(1)) == C.CCL_TJ
    assert int(re.search(r"constexpr int QCAP = (\d+);", src).group(1)) == C.QCAP
    tiles = re.findall(r"const int64_t tiles = \((?:n|nn) \+ (\d+)\) / (\d+);", src)  # (the tile is a literal in the source)
    assert len(tiles) == 2 and all((int(a), int(b)) == (C.TILE - 1, C.TILE) for a, b in tiles)
    assert f"__shared__ __attribute__((aligned(16))) float sx[{C.TILE}], sy[{C.TILE}];" in src
    assert "gap > fminf(di, tile_dmax[tj]) * 1.0001f" in src


# ---- path witnesses --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", C.TILE_EDGE_SIZES[1:])
def test_tile_edge_clouds_mix_singletons_and_larger_components(n):
    sizes = np.bincount(C.case(f"tile_edges-{n}")["want"])
    assert (sizes == 1).sum() >= n // 10 and (sizes >= 3).sum() >= n // 50


@pytest.mark.parametrize("order", ["x", "y", "cell"])
def test_strips_have_most_tile_pairs_pruned_by_the_box_test(order):
    c = C.case(f"strips-{order}")
    t = C.tile_count(c["points"].shape[0])
    iu = np.triu_indices(t)
    pruned = C.tile_gaps(c["points"])[iu] > np.float32(c["dist"]) * np.float32(1.0001)
    print(order, int(pruned.sum()), "of", pruned.size)
    assert t == 16 and 2 * pruned.sum() >= pruned.size
    per_pair = C.links_per_tile_pair(c)[iu]
    assert per_pair[pruned].sum() == 0  # (the prune is sound on this layout: what it skips holds no link)
    assert (per_pair[~pruned] > 0).sum() > t  # and links do cross tiles
    np.testing.assert_array_equal(np.sort(c["points"], 0), np.sort(C.case("strips-x")["points"], 0))  # one cloud, three orders


@pytest.mark.parametrize("gaps", [False, True])
def test_chains_form_the_expected_components(gaps):
    name = "chain_gaps" if gaps else "chain"
    asc = C.case(f"{name}-ascending")
    assert asc["points"].shape[0] == 6000 and (np.diff(asc["points"][:, 0]) > 0).all()
    np.testing.assert_array_equal(asc["want"], np.arange(6000) // 1000 if gaps else np.zeros(6000))
    np.testing.assert_array_equal(C.case(f"{name}-descending")["points"], asc["points"][::-1])
    for order in ("descending", "permuted"):
        assert C.case(f"{name}-{order}")["want"].max() + 1 == (6 if gaps else 1)


def test_late_bridge_is_joined_by_its_last_rows_only():
    c = C.case("late_bridge")
    assert not c["want"].any()
    without = C.plain(c["points"][:-C.BRIDGE_ROWS], c["dist"])
    np.testing.assert_array_equal(without, np.repeat([0, 1], 2000))


@pytest.mark.parametrize("name", ["blobs", "blobs-permuted"])
def test_blobs_overflow_the_link_queue(name):
    c = C.case(name)
    per_pair = C.links_per_tile_pair(c)
    print(name, per_pair.max())
    assert per_pair.max() > C.QCAP
    if name == "blobs":
        assert per_pair[0, 0] == C.TILE * (C.TILE - 1) // 2 == 32640
    sizes = np.bincount(c["want"])
    assert sizes.max() == 600 and (sizes == 1).sum() == 424


def test_blob_satellites_hang_on_links_found_after_the_queue_is_full():
    c = C.case("blob_satellites")
    a = C.links(c)
    sat = np.arange(C.TILE + 128, C.TILE + 128 + C.SATELLITES)
    sizes = np.bincount(c["want"])
    assert sizes[0] == C.TILE + 128 + C.SATELLITES and (sizes[1:] == 1).all() and not c["want"][sat].any()
    assert a[:C.TILE, C.TILE:C.TILE + 128].all() and a[:C.TILE, sat].all()  # every row of A links every row of R and of S
    # a wave of 64 rows of A has queued 64 x 128 links, more than QCAP, before its first column >= 128; S sits at such columns
    assert 64 * 128 > C.QCAP and sat.min() - C.TILE >= 128
    # and S has no other way in: without its links to A (tile pair (0, 1)) it is a component of its own
    a = a.copy()
    a[:C.TILE, sat] = False
    outside = np.setdiff1d(np.arange(a.shape[0]), sat)
    assert not a[np.ix_(outside, sat)].any() and not a[np.ix_(sat, outside)].any()


def _distances_of_close_pairs(c):
    """(reference fp32 distances of all pairs i < j within 1.5 dist, n)"""
    p = c["points"]
    i, j = np.triu_indices(p.shape[0], 1)
    near = np.abs(p[i, :2].astype(np.float64) - p[j, :2]).max(1) <= 1.5 * c["dist"]
    return C.reference_distances(p, i[near], j[near])


@pytest.mark.parametrize("name,components", [("lattice_half", (1600, 1)), ("lattice_tenth", (None, 1))])
def test_lattices_hold_pairs_exactly_at_the_threshold(name, components):
    at, nxt = C.case(f"{name}-at"), C.case(f"{name}-next")
    assert np.float32(nxt["dist"]) == np.nextafter(np.float32(at["dist"]), np.float32(np.inf))
    d = _distances_of_close_pairs(at)
    equal = int((d == np.float32(at["dist"])).sum())
    print(name, "pairs at dist:", equal, "below:", int((d < np.float32(at["dist"])).sum()))
    assert equal >= 100
    if components[0] is not None:
        assert at["want"].max() + 1 == components[0]
    assert at["want"].max() + 1 > nxt["want"].max() + 1 == components[1]  # the pairs at the threshold decide the partition


@pytest.mark.parametrize("k", [1.0, 2.0, 0.5])
def test_pythagorean_pair_sits_exactly_at_the_threshold(k):
    at, nxt = C.case(f"pythagorean-{k}-at"), C.case(f"pythagorean-{k}-next")
    d = C.reference_distances(at["points"], [0], [1])[0]
    assert d == np.float32(at["dist"]) == np.float32(1.25 * k) and np.float32(nxt["dist"]) == np.nextafter(d, np.float32(np.inf))
    assert at["want"].tolist() == [0, 1] and nxt["want"].tolist() == [0, 0]


def test_degenerate_distances():
    for d in (1e-30, 1e-20):
        c = C.case(f"triples-{d}")
        assert np.float32(d) > 0 and np.float32(d) * np.float32(d) < np.finfo(np.float32).tiny  # dist^2 underflows (to 0 or a denormal)
        assert (np.bincount(c["want"]) == 3).all() and c["want"].max() + 1 == 500
        for lab in (0, 250, 499):  # a component is one point three times
            assert len(np.unique(c["points"][c["want"] == lab], axis=0)) == 1
    for d in (0.0, -1.0):
        np.testing.assert_array_equal(C.case(f"triples-{d}")["want"], np.arange(1500))


def test_non_finite_rows_are_singletons_and_leave_the_rest_alone():
    c = C.case("nonfinite_rows")
    bad = ~np.isfinite(c["points"][:, :2]).all(1)
    assert sorted(np.nonzero(bad)[0]) == sorted(C.NONFINITE_ROWS) and {0, C.TILE - 1, C.TILE, 1024} & set(C.NONFINITE_ROWS)
    sizes = np.bincount(c["want"])
    assert (sizes[c["want"][bad]] == 1).all()
    clean = C.plain(C.nonfinite_clean()[~bad], c["dist"])
    np.testing.assert_array_equal(C.number_by_first_member(c["want"][~bad]), clean)
    t = C.case("nonfinite_tile")
    bad = ~np.isfinite(t["points"][:, :2]).all(1)
    assert bad[C.TILE:3 * C.TILE].all() and bad.sum() == 2 * C.TILE and (np.bincount(t["want"])[t["want"][bad]] == 1).all()
    np.testing.assert_array_equal(C.number_by_first_member(t["want"][~bad]), C.plain(C.nonfinite_clean()[~bad], t["dist"]))


def test_columns_past_y_are_ignored():
    two, five = C.case("columns-2"), C.case("columns-5")
    assert two["points"].shape == (777, 2) and five["points"].shape == (777, 5)
    np.testing.assert_array_equal(two["points"], five["points"][:, :2])
    extra = five["points"][:, 2:]
    fin = np.abs(extra[np.isfinite(extra)])
    assert fin.max() > 1e20 and fin.min() < 1e-20 and np.isnan(extra).any() and np.isinf(extra).any()
    np.testing.assert_array_equal(two["want"], five["want"])


@pytest.mark.parametrize("samples", [2, 3])
def test_batched_samples_share_coordinates_and_are_interleaved(samples):
    c = C.case(f"batch_shared-{samples}")
    idx, p = c["idx"], c["points"]
    assert sorted(np.unique(idx)) == list(range(samples)) and (np.diff(idx) != 0).sum() > len(idx) // 4
    a, b = p[idx == 0], p[idx == 1]
    np.testing.assert_array_equal(a[np.lexsort(a.T)], b[np.lexsort(b.T)])  # the same cloud in samples 0 and 1
    ignoring = C.plain(p, c["dist"])  # without the sample index every point joins its copy
    assert ignoring.max() + 1 < c["want"].max() + 1
    for lab in np.unique(c["want"])[:50]:
        assert len(np.unique(idx[c["want"] == lab])) == 1
    # the reference's order (sample-major) is another numbering of the same partition
    ref = C.batched_reference_order(p, idx, c["dist"])
    np.testing.assert_array_equal(C.number_by_first_member(ref), c["want"])
    assert (np.diff(ref[np.argsort(idx, kind="stable")]) >= -ref.max()).all() and ref[idx == 0].max() < ref[idx == 1].min()


def _cross_group_pairs_closer_than_both(c):
    p = c["points"][:, :2].astype(np.float64)
    d = np.hypot(p[:, None, 0] - p[None, :, 0], p[:, None, 1] - p[None, :, 1])
    rd = C.row_distance(c).astype(np.float64)
    other = c["idx"][:, None] != c["idx"][None, :]
    return int((other & (d < np.minimum(rd[:, None], rd[None, :]))).sum()) // 2


def test_grouped_cases_reach_range_pruning_and_cross_group_neighbours():
    s = C.case("group_sorted")
    assert (np.diff(s["idx"]) >= 0).all() and s["table"].tolist() == C.GROUP_TABLE.tolist() and s["points"].shape[0] == 3000
    r = C.tile_group_ranges(s["idx"])
    disjoint = (r[:, None, 1] < r[None, :, 0]) | (r[None, :, 1] < r[:, None, 0])
    print("tile pairs with disjoint group ranges:", int(np.triu(disjoint).sum()), "of", len(r) * (len(r) + 1) // 2)
    assert np.triu(disjoint).sum() >= 1
    assert (r[:, 0] < r[:, 1]).any()  # and a tile that spans two groups
    assert _cross_group_pairs_closer_than_both(s) >= 1
    u = C.case("group_unsorted")
    ru = C.tile_group_ranges(u["idx"])
    held = [set(u["idx"][k * C.TILE:(k + 1) * C.TILE].tolist()) for k in range(len(ru))]
    unheld = [set(range(lo, hi + 1)) - h for (lo, hi), h in zip(ru, held)]
    assert sum(bool(x) for x in unheld) >= len(ru) // 2 and unheld[0] == {1, 2, 3, 4}  # ranges that span groups the tile does not hold
    assert any(float(u["table"][sorted(x)].max()) > float(u["table"][sorted(h)].max()) for x, h in zip(unheld, held) if x)  # (and a larger distance)
    np.testing.assert_array_equal(np.sort(u["points"], 0), np.sort(s["points"], 0))
    pm = C.case("group_permuted")
    assert all(len(set(pm["idx"][k * C.TILE:(k + 1) * C.TILE].tolist())) == 6 for k in range(11))  # every tile holds every group
    for name in ("group_sorted", "group_unsorted", "group_permuted", "group_single_member", "group_strips"):
        c = C.case(name)
        zero = c["table"][c["idx"]] == 0
        assert zero.any() and (np.bincount(c["want"])[c["want"][zero]] == 1).all()  # a distance of 0: singletons
    for name in ("group_same_coordinates", "group_same_coordinates-interleaved"):
        c = C.case(name)
        assert len(np.unique(c["points"], axis=0)) == 250 and _cross_group_pairs_closer_than_both(c) >= 250
        for lab in np.unique(c["want"])[:50]:
            assert len(np.unique(c["idx"][c["want"] == lab])) == 1
    m = C.case("group_single_member")
    assert np.bincount(m["idx"], minlength=6).tolist() == [400, 1, 0, 300, 1, 322]
    o = C.case("group_one_entry_table")
    assert o["table"].shape == (1,) and not o["idx"].any()
    np.testing.assert_array_equal(o["want"], C.plain(o["points"], float(o["table"][0])))


def test_group_strips_need_the_largest_distance_of_a_tiles_range():
    c = C.case("group_strips")
    idx, table = c["idx"], c["table"]
    assert (np.diff(idx) >= 0).all() and np.bincount(idx).tolist() == list(C.GROUP_STRIP_SIZES)
    assert all(int(e) % C.TILE == 8 for e in np.cumsum(C.GROUP_STRIP_SIZES)[:-1])
    r = C.tile_group_ranges(idx)
    t = len(r)
    iu = np.triu_indices(t)
    gaps, per_pair = C.tile_gaps(c["points"])[iu], C.links_per_tile_pair(c)[iu]
    dmax = np.array([table[lo:hi + 1].max() for lo, hi in r])
    dmin = np.array([table[lo:hi + 1].min() for lo, hi in r])
    meet = ~((r[:, None, 1] < r[None, :, 0]) | (r[None, :, 1] < r[:, None, 0]))[iu]
    slack = np.float32(1.0001)
    pruned = meet & (gaps > np.minimum(dmax[:, None], dmax[None, :])[iu] * slack)
    print("group_strips: box-pruned", int(pruned.sum()), "range-pruned", int((~meet).sum()), "of", pruned.size)
    assert pruned.sum() >= 1 and per_pair[pruned].sum() == 0 and per_pair[~meet].sum() == 0
    # linked tile pairs that a smaller distance of either tile's range would have pruned
    would = (per_pair > 0) & (gaps > np.minimum(dmin[:, None], dmin[None, :])[iu] * slack)
    print("linked tile pairs that need the range's largest distance:", int(would.sum()))
    assert would.sum() >= 1
