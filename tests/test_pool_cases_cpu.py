"""CPU: what the point-pooling tests on the device (tests/test_point_pool_gpu.py and the pooling tests of tests/test_hip_ops.py) stand on.

* Every case of tests/pool_cases.py is margin-clean: the oracle reports no (point, RoI) pair within NEAR_TOL of a box face, at most 2 %
  of a case's points were parked to get there, and a parked point is a hit of no RoI.
* Path witnesses: each case does reach the kernel path it is there for (hits of a RoI against PB_CAP, the modelled rounds of the
  index-range narrowing, the size of the rectangle of cells, the scan's form, which RoI meets which cap).  They are conditions on the
  inputs, derived with the kernel's constants, and they are checked AFTER the parking.
* The constants themselves against the kernel sources, so that a retuned kernel gets its witnesses re-derived.
* The oracle with `stop_at_cap=True` against the plain oracle on these cases."""
import os
import re

import numpy as np
import pytest

import pool_cases as P
from conftest import ROOT

CSRC = os.path.join(ROOT, "fullysparsefusion_amd", "csrc")


def _rows_per_roi(name):
    return np.bincount(P.want(name)[1], minlength=P.case(name)["rois"].shape[0])


# ---- margins ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", P.NAMES)
def test_case_is_margin_clean_and_parks_little(name):
    c = P.case(name)
    rb = None if c["pts_batch"] is None else c["rois"][:, c["batch_col"]].astype(np.int64)
    near = P.near_pairs(P.boxes(c), P.xyz(c), c["extra"], c["pts_batch"], rb)
    assert near.shape[0] == 0, near[:5]  # i.e. the smallest margin is >= NEAR_TOL
    n = c["pts"].shape[0]
    print(name, "parked", c["parked"].size, "of", n, "in", c["passes"], "passes")
    assert c["parked"].size <= P.MAX_PARKED_SHARE * n and c["passes"] <= 1
    assert (P.xyz(c)[c["parked"], 2] == P.PARK_Z).all() and not np.isin(c["parked"], P.full_rows(name)[0]).any()
    assert not any(v.flags.writeable for v in c.values() if isinstance(v, np.ndarray))
    assert P.NEAR_TOL == 10 * 1e-4


def test_margin_clean_parks_exactly_the_near_points():
    """Three points 1e-4 inside, 5e-4 outside and 5e-3 inside the enlarged face of one box: the first two are parked, nothing else is."""
    roi = np.array([[0, 0, -1, 2, 4, 2, -np.pi / 2]], P.F32)  # local frame = world frame up to rounding of pi / 2
    pts = np.array([[2.5 - 1e-4, 0, 0], [2.5 + 5e-4, 0, 0], [2.5 - 5e-3, 0, 0], [0, 0, 0], [9, 9, 0]], P.F32)
    clean, parked, passes = P.margin_clean(roi, pts, (1.0, 1.0, 1.0))
    assert parked.tolist() == [0, 1] and passes == 1
    np.testing.assert_array_equal(clean[2:], pts[2:])
    np.testing.assert_array_equal(clean[:2, :2], pts[:2, :2])
    assert (clean[:2, 2] == P.PARK_Z).all()


# ---- the constants -----------------------------------------------------------------------------------------------------------------

def test_constants_equal_the_kernel_source():
    pool = open(os.path.join(CSRC, "point_pool.hip")).read()
    scan = open(os.path.join(CSRC, "scan.h")).read()
    sort = open(os.path.join(CSRC, "radix_sort.h")).read()

    def const(src, name):
        return int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))

    assert const(pool, "PB_CAP") == P.PB_CAP and const(pool, "PB_BINS") == P.PB_BINS and const(pool, "PB_BITS") == P.PB_BITS
    assert const(pool, "PP_TILE") == P.PP_TILE
    assert "constexpr float PB_INV_CELL = 1.0f;" in pool
    assert f"(cx1 - cx0 + 1) * (cy1 - cy0 + 1) <= {P.PB_WALK_CELLS})" in pool
    assert "if (!brute && max_inbox_point <= PB_CAP) {" in pool
    assert "if (b.hits_full[r] > (uint32_t)PB_CAP) {" in pool
    assert "if (run + c <= (uint32_t)PB_CAP || width == 1) {" in pool
    assert "const uint32_t width = (hi - lo + PB_BINS - 1) / PB_BINS;" in pool
    # four RoIs per workgroup of the binned kernels, 256 per group of the brute-force passes
    assert pool.count(f"(int64_t)blockIdx.x * {P.PB_ROIS_PER_WG} + ") == 2 and f"(n_rois + {P.PB_ROIS_PER_WG - 1}) / {P.PB_ROIS_PER_WG}" in pool
    assert f"((int64_t)blockIdx.x + a.group0) * {P.PP_ROIS_PER_GROUP} + threadIdx.x" in pool and f"fsf_cdiv(n_rois, {P.PP_ROIS_PER_GROUP})" in pool
    assert const(scan, "SC_THREADS") * const(scan, "SC_ITEMS") == P.SC_TILE and "SC_TILE = SC_THREADS * SC_ITEMS;" in scan
    assert "SC_VALUE_MASK = (1u << 30) - 1u" in scan and P.SC_VALUE_MASK == (1 << 30) - 1
    assert "if (n < (int64_t)SC_VALUE_MASK / max_item) {" in scan
    assert const(sort, "RS_THREADS") * const(sort, "RS_ITEMS") == P.RS_TILE and "RS_TILE = RS_THREADS * RS_ITEMS;" in sort


# ---- the host model of the narrowing ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_pts,hits,keep,rounds", [(6000, "even", 512, 1), (6000, "even", 1023, 1), (6000, "even", 1024, 2),
                                                    ((1 << 20) + 4096, "all_but_0", 1024, 3)])
def test_narrowing_model_round_counts(n_pts, hits, keep, rounds):
    h = np.arange(0, n_pts, 2) if hits == "even" else np.arange(1, n_pts)
    got, limit, below = P.narrowing_rounds(h, n_pts, keep)
    assert got == rounds and keep <= below <= P.PB_CAP
    assert below == (h < limit).sum()


def test_narrowing_model_against_a_direct_search():
    """Whatever the rounds do, the limit must leave at least `keep` and at most PB_CAP hits below it."""
    rng = np.random.default_rng(3)
    for n_pts, k in ((5000, 1100), (40000, 30000), (3_000_000, 2_000_000), (1025, 1025)):
        h = np.sort(rng.choice(n_pts, k, replace=False))
        for keep in (1, 500, 1023, 1024):
            rounds, limit, below = P.narrowing_rounds(h, n_pts, keep)
            assert keep <= below <= P.PB_CAP and 1 <= rounds <= 3
            np.testing.assert_array_equal(h[h < limit][:keep], h[:keep])


# ---- path witnesses --------------------------------------------------------------------------------------------------------------

CAPS_A = {  # (RoIs with more hits than max_inbox, is max_all reached), from the parametrisations' own comments in test_hip_ops.py
    (37, 20000, 512, 50000): (False, False), (300, 60000, 16, 50000): (True, False), (300, 60000, 512, 700): (False, True),
    (1, 5000, 512, 50000): (True, False), (700, 3000, 512, 50000): (False, False), (2000, 20000, 32, 3000): (True, True),
    (2000, 20000, 512, 10 ** 6): (False, False), (1100, 8000, 4, 900): (True, True)}


@pytest.mark.parametrize("t", P.FAMILY_A, ids=lambda t: "-".join(map(str, t)))
def test_family_a_meets_the_caps_it_always_met(t):
    name = P.family_a_name(*t)
    c, h = P.case(name), P.full_hits(name)
    assert c["rois"].shape == (t[0], 7) and c["pts"].shape == (t[1], 5) and (c["max_inbox"], c["max_all"]) == t[2:]
    over, reached = CAPS_A[t]
    assert bool((h > t[2]).any()) == over and (np.minimum(h, t[2]).sum() > t[3]) == reached
    assert P.pool_path(t[2]) == "binned" and h.max() <= P.PB_CAP and P.want(name)[0].size > 0
    if t[0] >= 1100:  # several chunks (1, 2, 4, ... groups) of RoI groups on the brute-force side
        assert -(-t[0] // P.PP_ROIS_PER_GROUP) >= 4


@pytest.mark.parametrize("max_inbox", [P.PB_CAP - 1, P.PB_CAP, P.PB_CAP + 1])
def test_cap_edges_hits_and_paths(max_inbox):
    name = f"b-cap_edges-{max_inbox}"
    c = P.case(name)
    assert P.full_hits(name).tolist() == [P.PB_CAP, P.PB_CAP + 1, 3000] == list(c["expect"]["hits"].values())
    assert P.pool_path(max_inbox) == ("brute" if max_inbox > P.PB_CAP else "binned")
    # RoI 0 fills its list to the last slot without narrowing, RoI 1 is the lightest RoI that narrows
    assert _rows_per_roi(name).tolist() == [min(P.PB_CAP, max_inbox), max_inbox, max_inbox]
    if max_inbox <= P.PB_CAP:
        for r, rounds in ((1, 1), (2, 2)):
            got, limit, below = P.narrowing_rounds(P.hit_index(name, r), c["pts"].shape[0], max_inbox)
            assert got == rounds and max_inbox <= below <= P.PB_CAP


@pytest.mark.parametrize("max_inbox,rounds", [(512, 1), (P.PB_CAP - 1, 1), (P.PB_CAP, 2)])
def test_every_second_index_rounds(max_inbox, rounds):
    name = f"c-every_second-{max_inbox}"
    c = P.case(name)
    np.testing.assert_array_equal(P.hit_index(name, 0), np.arange(0, 6000, 2))
    assert P.full_hits(name).tolist() == [3000, 100] and c["pts"].shape[0] == 6000
    assert P.narrowing_rounds(P.hit_index(name, 0), 6000, max_inbox)[0] == rounds
    np.testing.assert_array_equal(P.want(name)[0][:max_inbox], np.arange(0, 2 * max_inbox, 2))


def test_million_points_rounds_and_the_exclusive_limit():
    name = "c-million"
    c = P.case(name)
    n = c["pts"].shape[0]
    assert n == (1 << 20) + 4096 and c["max_inbox"] == P.PB_CAP
    np.testing.assert_array_equal(P.hit_index(name, 0), np.arange(1, n))
    assert P.full_hits(name).tolist() == [n - 1, n - 1 - 514, 514]
    trace0, limit0 = P.narrowing_trace(P.hit_index(name, 0), n, P.PB_CAP)
    assert [w for w, *_ in trace0] == [1028, 2, 1] and limit0 == 1025  # three rounds, left through a bin of one index
    assert P.narrowing_rounds(P.hit_index(name, 1), n, P.PB_CAP)[0] == 2
    # exactly PB_CAP hits lie below the limit and index `limit` is a hit too: a fill that took `pi <= limit` would gather PB_CAP + 1
    assert P.narrowing_rounds(P.hit_index(name, 0), n, P.PB_CAP)[2] == P.PB_CAP and limit0 in P.hit_index(name, 0)
    assert _rows_per_roi(name).tolist() == [P.PB_CAP, P.PB_CAP, 452]  # max_all cuts the light RoI's list in the middle


def test_last_bin_is_partial_and_split_again():
    name = "c-last_bin"
    n = P.case(name)["pts"].shape[0]
    trace, limit = P.narrowing_trace(P.hit_index(name, 0), n, P.PB_CAP)
    (w0, b0, run0, c0), (w1, b1, _, _) = trace
    assert (w0, b0, run0, c0) == (7, 1000, 1022, 3) and b0 * w0 + w0 > n  # bin_hi = min(hi, ...) is the `hi` branch
    assert (w1, b1) == (1, 1) and limit == n - 1 and P.full_hits(name).tolist() == [1025, 300]


def test_lane_edges_cross_in_the_first_and_the_last_bin_of_a_lane():
    name = "c-lane_edges"
    c = P.case(name)
    per_lane = P.PB_BINS // 64
    for r, (bin_, pos) in enumerate(((160, 0), (175, per_lane - 1))):
        trace, _ = P.narrowing_trace(P.hit_index(name, r), c["pts"].shape[0], c["max_inbox"])
        assert len(trace) == 1 and trace[0][1] == bin_ and bin_ % per_lane == pos and trace[0][2] == c["max_inbox"] - 1
    assert P.full_hits(name).tolist() == [1117, 1117]


@pytest.mark.parametrize("where,rows", [("middle", 200), ("first_row", 0), ("second_row", 1)])
def test_global_cap_inside_the_heavy_last_roi(where, rows):
    name = f"d-cap_{where}"
    c = P.case(name)
    assert P.full_hits(name).tolist() == list(P.LIGHT) + [3000] and P.pool_path(c["max_inbox"]) == "binned"
    assert c["max_all"] == sum(P.LIGHT) + rows and _rows_per_roi(name).tolist() == list(P.LIGHT) + [rows]
    assert c["rois"].shape[0] - 1 == 5 and 5 // P.PB_ROIS_PER_WG == 1  # the heavy RoI is the last one, in the second workgroup


def test_cell_rectangles_on_both_sides_of_the_walk_threshold():
    c = P.case("e-cell_rect")
    (nx0, ny0, s0), (nx1, ny1, s1) = (P.cell_rect(b, c["extra"]) for b in P.boxes(c))
    assert (nx0, ny0) == (32, 32) and nx0 * ny0 == P.PB_WALK_CELLS and (nx1, ny1) == (32, 33)
    assert min(s0, s1) > 0.05  # the circles' extremes are nowhere near a cell boundary: fp32 rounding cannot change the counts
    assert abs(nx1 - ny1) <= 1 and 1025 == 25 * 41  # no rectangle under a circle has 1025 cells
    assert (P.full_hits("e-cell_rect") > 400).all()


def test_cell_edges_case_holds_what_it_says():
    name = "e-cell_edges"
    c = P.case(name)
    b, x = P.boxes(c), P.xyz(c)
    assert (P.full_hits(name) > 0).all()
    rects = [P.cell_rect(k, c["extra"])[:2] for k in b]
    assert all(nx >= 5 and ny >= 5 for nx, ny in rects[:4]) and (b[:4, :2].min(1) <= 0).all()  # rows of cells below 0 and on both sides of it
    assert rects[6] == (1, 1) and rects[4][0] < rects[4][1] and rects[5][0] < rects[2][0]  # cut off by / collapsed into the border cells
    assert (np.abs(b[4:8, :2]).max(1) > 511).all()
    p, _ = P.full_rows(name)
    hit = x[np.unique(p)]
    assert ((hit[:, :2] == np.round(hit[:, :2])).all(1)).sum() >= 100   # points on exact integer coordinates among the hits
    assert ((hit == 0) & np.signbit(hit)).any(1).sum() >= 5            # and points with a -0.0 coordinate
    bad = c["expect"]["nonfinite"]
    assert not np.isfinite(x[bad]).all(1).any() and np.isnan(x[bad]).any() and np.isinf(x[bad]).any() and not np.isin(bad, p).any()
    assert np.isfinite(np.delete(x, bad, 0)).all()


def test_batched_case_holds_what_it_says():
    name = "e-batched"
    c = P.case(name)
    rb, pb = c["rois"][:, c["batch_col"]].astype(np.int64), c["pts_batch"]
    assert set(rb) == set(pb) == {0, 1} and (np.diff(pb) < 0).any() and (np.diff(rb) < 0).any()  # neither is in sample order
    h = P.full_hits(name)
    heavy = c["expect"]["heavy"]
    assert h[heavy] > P.PB_CAP and P.pool_path(c["max_inbox"]) == "binned"
    rows = _rows_per_roi(name)
    assert rows[heavy] == c["max_inbox"] and rows.sum() == c["max_all"] < np.minimum(h, c["max_inbox"]).sum()  # both caps cut
    last = P.want(name)[1][-1]
    assert 0 < rows[last] < min(h[last], c["max_inbox"]) and last > heavy  # max_all falls inside a RoI's list, after the heavy one
    # a point of the other sample inside a RoI must not count: without the batch indices every RoI would get about twice the hits
    blind = dict(c, pts_batch=None)
    hb = np.bincount(P.reference(blind, P.BIG, P.BIG)[1], minlength=h.size)
    assert (hb >= h).all() and hb.sum() > 1.8 * h.sum()
    cells = lambda s: set(map(tuple, np.floor(P.xyz(c)[pb == s][:, :2]).astype(int)))  # noqa: E731
    assert len(cells(0) & cells(1)) > 100


def test_sizes_at_the_tile_edges():
    assert P.PTS_SIZES == (1, 63, 64, 65, 256, 257, P.PP_TILE - 1, P.PP_TILE, P.PP_TILE + 1, 2 * P.PP_TILE + 1)
    assert P.ROI_SIZES == (1, P.PB_ROIS_PER_WG - 1, P.PB_ROIS_PER_WG, P.PB_ROIS_PER_WG + 1, P.PP_ROIS_PER_GROUP, P.PP_ROIS_PER_GROUP + 1)
    assert P.PP_TILE == P.RS_TILE == P.SC_TILE
    for n in P.PTS_SIZES:
        c = P.case(f"f-pts-{n}")
        assert c["pts"].shape[0] == n and P.want(f"f-pts-{n}")[0].size > 0
    for n in P.ROI_SIZES:
        c = P.case(f"f-rois-{n}")
        rows = _rows_per_roi(f"f-rois-{n}")
        assert c["rois"].shape[0] == n and rows.sum() > 0 and rows.sum() == min(c["max_all"], np.minimum(P.full_hits(f"f-rois-{n}"), 16).sum())
    assert _rows_per_roi("f-rois-257").sum() == P.case("f-rois-257")["max_all"]


def test_strided_case_uses_every_offset():
    c = P.case("f-strided")
    assert c["rois"].shape[1] == 11 and (c["box_col"], c["batch_col"]) == (3, 1) and c["pts"].shape[1] == 6 and c["xyz_col"] == 2
    rows = _rows_per_roi("f-strided")
    assert rows.sum() == c["max_all"] and rows.max() == c["max_inbox"]
    # reading the box or the points one column off gives other rows: the offsets matter
    for shifted in (dict(c, box_col=2), dict(c, xyz_col=1)):
        p, r, _ = P.reference(shifted)
        assert p.size != c["max_all"] or not np.array_equal(p, P.want("f-strided")[0])


def test_brute_force_cases_above_pb_cap():
    for name, rows in (("g-every_second-2048", [2048, 100]), ("g-every_second-capped", [1500, 0])):
        c = P.case(name)
        assert P.pool_path(c["max_inbox"]) == "brute" and c["max_inbox"] == 2048 and _rows_per_roi(name).tolist() == rows
        tiles = np.unique(P.hit_index(name, 0) // P.PP_TILE)
        assert tiles.tolist() == [0, 1, 2] and P.full_hits(name)[0] > c["max_inbox"]


@pytest.mark.parametrize("n_rois,form", [(2000, "lookback"), (2100, "three_launch")])
def test_scan_pair_selects_both_forms(n_rois, form):
    name = f"g-scan-{n_rois}"
    c = P.case(name)
    assert c["rois"].shape[0] == n_rois and c["max_inbox"] == 1 << 19 and P.pool_path(c["max_inbox"]) == "brute"
    assert P.scan_form(n_rois, c["max_inbox"]) == form == c["expect"]["scan"]
    assert P.scan_form(n_rois, P.PB_CAP) == "lookback"  # (what every other case takes)
    rows = _rows_per_roi(name)
    assert 0 < rows.sum() < c["max_all"] and c["max_all"] * 13 * 4 < 4 << 20  # no cap: every offset decides where rows land
    if n_rois > P.SC_TILE:
        assert rows[P.SC_TILE:].sum() > 100  # rows of the second scan tile's RoIs


# ---- the oracle's early exit -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in P.NAMES if n not in ("e-batched", "f-strided")])  # (the oracle itself knows no batch index)
def test_oracle_stop_at_cap_is_the_plain_result(name):
    assert P.case(name)["pts_batch"] is None
    got = P.reference(P.case(name), stop_at_cap=True)
    for a, b in zip(got, P.want(name)):
        np.testing.assert_array_equal(a, b)
