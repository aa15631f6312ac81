"""CPU: every case of tests/project_cases.py reaches the decision it is named for, and the referees are decisive — a wrong variant of
the host arithmetic (round half away, floor(ix + 0.5), pz >= 1e-3, no depth clamp, non-strict image bounds, last maximum wins, a
clamped score lookup; for the bilinear gather a dropped small tap and an outside corner given an inside weight) disagrees with the
referee on the group named for it, while the inputs the suite had before (the golden nusc_small case, the batch-maximum criterion)
let it pass.  No GPU: what the kernels do on these cases is tests/test_project_gpu.py."""
import numpy as np
import pytest
import torch

import bilinear_cases as B
import project_cases as P
from conftest import golden_cases, load_golden


def cam_a(name="pixel"):
    """(oracle ids of camera 0 [n], grid [n, 2], the fp32 nearest-pixel coordinates ix, iy) of a case whose camera 0 is CAM_A."""
    w = P.id_want(name)
    g = w["pts_2d"][0]
    ix = (g[:, 0] + np.float32(1)) * np.float32(P.W / 2) - np.float32(0.5)
    iy = (g[:, 1] + np.float32(1)) * np.float32(P.H / 2) - np.float32(0.5)
    return w["obj"][:, 0, 0], g, ix, iy


def pixel_of(ids):
    return (ids - 1) % P.W, (ids - 1) // P.W  # column, row


# ------------------------------------------------------------------------------------------------------------------ the cameras
def test_the_exact_camera_is_exact_and_the_two_referees_agree():
    u = np.arange(0, 4 * P.W + 1) / 4.0
    pts = P.exact_points(np.stack([u, np.full_like(u, 10.75)], 1), 2.0)
    plane = P.id_plane()[None, None]
    obj, p2d = P.oracle_project(pts, plane, P.CAM_A[None])
    inside = (u > 0) & (u < P.W)
    ix = (p2d[0, :, 0] + np.float32(1)) * np.float32(P.W / 2) - np.float32(0.5)
    assert np.array_equal(ix[inside].astype(np.float64), u[inside] - 0.5)        # ix = u - 0.5 exactly
    assert np.array_equal(p2d[0, ~inside], np.full((2, 2), -2, dtype=np.float32)) and not obj[~inside].any()   # u = 0 and u = W
    col, row = pixel_of(obj[:, 0, 0])
    assert [int(col[u == k][0]) for k in (1, 2, 3)] == [0, 2, 2] and (row[inside] == 10).all()                    # half to even
    assert np.array_equal(P.torch_nearest_ids(plane, p2d), obj)


@pytest.mark.parametrize("name", [n for n in P.ID_CASES if "second_trip" not in n])
def test_oracle_torch_grid_sample_and_the_default_variant_agree_on_every_point(name):
    c, w = P.id_case(name), P.id_want(name)
    assert np.array_equal(P.torch_nearest_ids(c["mask"], w["pts_2d"]), w["obj"])
    assert np.array_equal(P.project_variant(c["pts"], c["L"], c["mask"]), w["obj"])
    ids, score = P.cam_select_variant(w["obj"], c["anno"], c["score_col"])
    assert np.array_equal(ids, w["ids"]) and np.array_equal(score, w["score"])


# ------------------------------------------------------------------------------------------------------------- pixel decisions
def test_ties_sit_on_k_plus_a_half_and_go_to_the_even_pixel():
    _, sl = P.pixel_points()
    ids, _, ix, iy = cam_a()
    col, row = pixel_of(ids)
    for group, on_x, on_y in (("ties_x", True, False), ("ties_y", False, True), ("ties_xy", True, True)):
        s = sl[group]
        assert (ids[s] > 0).all()
        if on_x:
            assert (ix[s] - np.floor(ix[s]) == 0.5).all() and (col[s] % 2 == 0).all()
            assert {int(np.floor(v)) % 2 for v in ix[s]} == {0, 1}            # both parities: rounded down and rounded up
        else:
            assert (ix[s] - np.floor(ix[s]) != 0.5).all()
        if on_y:
            assert (iy[s] - np.floor(iy[s]) == 0.5).all() and (row[s] % 2 == 0).all()
            assert {int(np.floor(v)) % 2 for v in iy[s]} == {0, 1}
        else:
            assert (iy[s] - np.floor(iy[s]) != 0.5).all()


def test_the_image_border_is_exclusive_and_a_quarter_pixel_inside_is_valid():
    c = P.id_case("pixel")
    _, sl = P.pixel_points()
    ids, g, _, _ = cam_a()
    # the unmasked grid values: exactly -1 / +1 on the border
    raw = P.project_variant(c["pts"][sl["border_out"]], c["L"][:1], c["mask"][:1], strict=False)[:, 0, 0]
    with np.errstate(all="ignore"):
        p = c["pts"][sl["border_out"], :3]
        gx = (p[:, 0] * np.float32(32) + p[:, 2] * np.float32(32)) / p[:, 2] / np.float32(P.W)
        gy = (p[:, 1] * np.float32(32) + p[:, 2] * np.float32(16)) / p[:, 2] / np.float32(P.H)
    assert [float((gx[0] - .5) * 2), float((gx[1] - .5) * 2), float((gy[2] - .5) * 2), float((gy[3] - .5) * 2)] == [-1.0, 1.0, -1.0, 1.0]
    assert not ids[sl["border_out"]].any() and (g[sl["border_out"]] == -2).all()
    assert (raw > 0).sum() >= 2                                     # non-strict bounds would read a pixel
    col, row = pixel_of(ids[sl["border_in"]])
    assert (ids[sl["border_in"]] > 0).all()
    assert [int(col[0]), int(col[1]), int(row[2]), int(row[3])] == [0, P.W - 1, 0, P.H - 1]


@pytest.mark.parametrize("side", [64, 800, 1600, 2048, 32, 450, 900, 1550])
def test_no_valid_projection_reaches_the_index_guards(side):
    valid, rx = P.guard_scan(side)
    assert valid[:256].all() and not valid[256:512 + 9].any() and valid[512 + 9:].all()   # below 1 | above 0 and up to 2^-26 | past 2^-26
    assert (rx[valid] >= 0).all() and (rx[valid] < side).all()
    assert rx[0] == side - 1 and rx[valid].min() == 0


def test_depth_threshold_and_clamp():
    c = P.id_case("pixel")
    _, sl = P.pixel_points()
    w = P.id_want("pixel")
    d = c["pts"][sl["depth"], 2]
    assert d[0] == np.float32(1e-3) and d[1] == np.nextafter(np.float32(1e-3), np.float32(1)) and d[2] == 0 and (d[3:] < 0).all()
    assert [bool(v) for v in (w["obj"][sl["depth"], 0, 0] > 0)] == [False, True, False, False, False]
    assert (w["pts_2d"][0, sl["depth"]][[0, 2, 3, 4]] == -2).all()
    # the clamp: 2^18 > 1e5 lands on CAM_B's principal point unclamped, on another valid pixel clamped
    s = sl["depth_clamp"]
    no_clamp = P.project_variant(c["pts"][s], c["L"], c["mask"], clamp=False)[:, 1, 0]
    clamped = w["obj"][s, 1, 0]
    assert c["pts"][s.start, 2] == 2.0 ** 18 and no_clamp[0] == 1 + 8 * P.W + 16 and clamped[0] > 0 and clamped[0] != no_clamp[0]
    assert c["pts"][s.start + 1, 2] == np.float32(1e5) and clamped[1] == no_clamp[1] == no_clamp[0]   # on the clamp's end: no change


def test_non_finite_coordinates_are_invalid_everywhere():
    c, w = P.id_case("pixel"), P.id_want("pixel")
    s = P.pixel_points()[1]["nonfinite"]
    p = c["pts"][s, :3]
    assert np.isnan(p[0, 0]) and np.isnan(p[1, 1]) and np.isnan(p[2, 2]) and p[3, 2] == np.inf and p[4, 2] == -np.inf
    assert not w["obj"][s].any() and (w["pts_2d"][:, s] == -2).all()
    assert not w["fg"][s].any() and not w["count"][s].any() and not w["max_id"][s].any() and not w["score"][s].any()


def test_camera_choice_first_maximum_wins():
    c, w = P.id_case("choice"), P.id_want("choice")
    assert [tuple(int(v) for v in r) for r in w["obj"].sum(-1)] == list(P.CHOICE_SUMS)
    assert (w["pts_2d"][0, 3] == -2).all() and (w["pts_2d"][1:, 3] > -1.5).all()       # CAM_B does not see point 3
    assert [tuple(int(v) for v in r) for r in w["ids"]] == list(P.CHOICE_IDS)
    for i, cam in enumerate(P.CHOICE_WINNER):
        assert np.array_equal(w["ids"][i], w["obj"][i, cam])
    last, _ = P.cam_select_variant(w["obj"], c["anno"], c["score_col"], last_max=True)
    assert (last != w["ids"]).any(1).tolist() == [True, True, False, True, True]


def test_score_lookup_reads_the_last_row_and_nothing_past_it():
    c, w = P.id_case("pixel"), P.id_want("pixel")
    s = P.pixel_points()[1]["lookup"]
    assert c["score_col"] != 4 and c["anno"].shape == (P.NUM_ANNO, P.ANNO_DIM) and P.ANNO_DIM != 9
    assert w["ids"][s, 0].tolist() == [P.NUM_ANNO, P.NUM_ANNO + 1, 0]
    assert w["score"][s, 0].tolist() == [float(c["anno"][-1, c["score_col"]]), 0.0, 0.0] and w["score"][s.start, 0] > 0
    _, clamped = P.cam_select_variant(w["obj"], c["anno"], c["score_col"], clamped_lookup=True)
    assert clamped[s.start + 1, 0] != 0 and clamped[s.start, 0] == w["score"][s.start, 0]
    wide, ww = P.id_case("i32_wide"), P.id_want("i32_wide")
    assert ww["ids"][s, 0].tolist() == [70000 + P.NUM_ANNO, 70001 + P.NUM_ANNO, 0] and ww["score"][s.start, 0] == wide["anno"][-1, 1]
    assert ww["score"][s.start + 1, 0] == 0 and wide["mask"].dtype == np.int32 and ww["obj"].max() > 2 ** 16


def test_second_camera_group_is_seen_by_cam_b_only():
    w = P.id_want("pixel")
    s = P.pixel_points()[1]["second_camera"]
    assert not w["obj"][s, 0].any() and (w["obj"][s, 1] > 0).all() and np.array_equal(w["ids"][s], w["obj"][s, 1])


def test_types_and_widths():
    pts, _ = P.pixel_points()
    assert pts.shape[1] == 5 and P.id_case("pixel")["pts"].shape[1] == 5
    for name, ncls in (("u8_ncls16", 16), ("u8_ncls17", 17)):
        c, w = P.id_case(name), P.id_want(name)
        assert c["mask"].dtype == np.uint8 and c["mask"].shape[:2] == (1, ncls) and w["obj"].max() == 255
        assert (w["obj"][0] == 255).all() and (w["obj"][1, 0, ::2] == 255).all()
        assert 0 < w["fg"].sum() < len(w["fg"]) and w["count"].max() == ncls
    c, w = P.id_case("cams64_second_trip"), P.id_want("cams64_second_trip")
    assert c["L"].shape[0] == 64 and c["pts"].shape[0] * 64 > 8192 * 256 and w["obj"].nbytes < 18e6
    tail = w["obj"].reshape(-1)[8192 * 256:]
    assert tail.size > 0 and (tail > 0).sum() >= 100
    c, w = P.id_case("pixel_second_trip"), P.id_want("pixel_second_trip")
    assert c["pts"].shape[0] == 2048 * 256 + 77
    assert (w["ids"][2048 * 256:] > 0).sum() >= 30 and (w["score"][2048 * 256:] > 0).any()


# ------------------------------------------------------------------------------------------------- the wrong variants disagree
def _differs(group, **variant):
    c, w = P.id_case("pixel"), P.id_want("pixel")
    s = P.pixel_points()[1][group]
    return bool((P.project_variant(c["pts"][s], c["L"], c["mask"], **variant) != w["obj"][s]).any())


def test_each_wrong_variant_disagrees_on_the_group_named_for_it():
    for group in ("ties_x", "ties_y", "ties_xy"):
        assert _differs(group, rounding="away") and _differs(group, rounding="floor")
    assert _differs("depth", depth_ge=True) and not _differs("ties_xy", depth_ge=True)
    assert _differs("depth_clamp", clamp=False) and not _differs("ties_xy", clamp=False)
    assert _differs("border_out", strict=False) and not _differs("border_in", strict=False)


def test_the_rounding_variants_pass_on_the_golden_case():
    """What the inputs the suite had miss: a random projection never lands on k + 0.5."""
    g = golden_cases(load_golden("project.npz"))["nusc_small"]
    assert np.array_equal(P.project_variant(g["points"], g["lidar2img"], g["mask"]), g["obj_id"])
    assert np.array_equal(P.project_variant(g["points"], g["lidar2img"], g["mask"], rounding="away"), g["obj_id"])
    assert np.array_equal(P.project_variant(g["points"], g["lidar2img"], g["mask"], rounding="floor"), g["obj_id"])


# ------------------------------------------------------------------------------------------------------------ row list, top-k
def test_row_list_cases_reach_what_they_are_named_for():
    w = P.row_want("one_cell")
    assert w["M"] == 0 and w["T"] == 0 and 0 < w["F"] < len(w["k"]) and int(w["k"].max()) == 1
    w = P.row_want("two_equal")
    k2 = w["k"] == 2
    assert w["M"] == w["T"] == int(k2.sum()) > 0 and set(w["k"].tolist()) == {0, 2} and not k2[0] and bool((w["obj"][k2, 0] == w["obj"][k2, 1]).all())
    assert torch.equal(w["ids"][w["F"]:], w["ids"][:w["F"]])                   # the appended row carries the id of the own row
    w = P.row_want("k235")
    assert w["k"][:10].tolist() == [3, 5, 1, 0, 2, 3, 5, 1, 0, 2] and {int(v) for v in w["k"]} == {0, 1, 2, 3, 5}
    assert w["T"] == int((w["k"] == 2).sum()) + 2 * int((w["k"] == 3).sum()) + 4 * int((w["k"] == 5).sum())
    w = P.row_want("cells_254")
    assert w["k"].tolist() == [254, 3, 0] and w["T"] == 253 + 2 and w["obj"].shape[1] == 256
    assert w["ids"][w["src"] == 1].tolist() == [200, 7, 7]                     # a duplicate id keeps its two entries
    for name, cells in zip(P.SATURATED_CASES, (255, 256)):
        assert P.row_want(name)["k"].tolist() == [cells, 3, 0]
    w = P.row_want("rows_second_trip")
    assert w["F"] == w["M"] == w["T"] == P.SECOND_TRIP_POINTS > 2048 * 256 and bool((w["k"] == 2).all())
    assert bool((w["ids"][w["F"]:] + 5000 == w["ids"][:w["F"]]).all())


@pytest.mark.parametrize("name", sorted(P.TOPK_CASES))
def test_topk_cases(name):
    x, k = P.topk_rows(name)
    n, w, kk, kind = P.TOPK_CASES[name]
    assert x.shape == (n, w) and k == kk <= w <= 128 and x.dtype == torch.int64 and int(x.min()) > torch.iinfo(torch.int64).min
    if name == "second_trip":
        assert n > 8192 * 16
        top = x[8192 * 16:].topk(k, dim=-1)[0]
        assert bool((top > 0).any())
    if kind == "equal":
        assert bool((x == x[:, :1]).all())
    if kind == "negative":
        assert int(x.max()) < 0
    if kind == "random":
        assert w < 3 or bool((x[:, 0] == x[:, 3]).all())


# ----------------------------------------------------------------------------------------------------- bilinear forward gather
@pytest.mark.parametrize("name", sorted(P.MAPS))
def test_crafted_points_reach_every_tap_edge(name):
    hf, wf = P.MAPS[name]
    pts, L, img_hw = P.bilinear_crafted()
    idx, w, inside, valid, x0, y0 = B.bilinear_taps_host(pts, L, img_hw, hf, wf, with_corner=True)
    v = valid[:, 0]
    assert v.sum() >= 80 and not valid[-3:].any()
    assert (x0[v, 0] == -1).any() and (x0[v, 0] == wf - 1).any() and (y0[v, 0] == -1).any() and (y0[v, 0] == hf - 1).any()
    assert x0[v, 0].min() >= -1 and x0[v, 0].max() <= wf - 1 and y0[v, 0].min() >= -1 and y0[v, 0].max() <= hf - 1
    # an integer ix: the right-hand taps weigh exactly 0 although they are inside
    assert (v[:, None] & inside[:, 0, [1, 3]] & (w[:, 0, [1, 3]] == 0) & (w[:, 0, [0, 2]] != 0)).any() or wf == 1
    assert (v & (w[:, 0, 1] == 0) & (w[:, 0, 0] != 0)).any()
    if hf > 1 and wf > 1:
        assert (v & inside[:, 0].all(-1)).any()                   # (a 1 x 1 map has no point with four taps inside)
    else:
        assert not (v & inside[:, 0].all(-1)).any()
    assert (valid.sum(1) == 2).any() and (valid.sum(1) == 1).any()


def test_crafted_points_sit_on_the_depth_threshold_of_the_tap_arithmetic():
    pts, L, img_hw = P.bilinear_crafted()
    valid = B.bilinear_taps_host(pts, L, img_hw, 3, 4)[3][P.BILINEAR_DEPTH]
    assert pts[P.BILINEAR_DEPTH, 2].tolist() == [float(np.float32(1e-3)), float(np.nextafter(np.float32(1e-3), np.float32(1))), 2.0 ** 18]
    assert valid.tolist() == [[False, False], [True, True], [False, True]]      # 2^18: clamped to 1e5, which moves it out of CAM_A only


def test_selection_has_one_two_and_no_camera_points():
    pts, L, img_hw = P.bilinear_selection()
    seen = B.bilinear_taps_host(pts, L, img_hw, 3, 4)[3].sum(1)
    assert pts.shape[0] == 346 and (seen[:200] == 1).all() and (seen[200:296] >= 2).all() and (seen[296:] == 0).all()


@pytest.mark.parametrize("reduce_cams", [False, True])
def test_the_budget_is_met_by_the_kernels_expression_in_fp32(reduce_cams):
    for pts, L, img_hw in (P.bilinear_crafted(), P.bilinear_selection()):
        for hf, wf in P.MAPS.values():
            feat = P.features(L.shape[0], 17, hf, wf)
            ref, tol = P.gather_budget(P.gather_referee(pts, L, img_hw, feat), reduce_cams)
            got = P.gather_fp32(pts, L, img_hw, feat, reduce_cams).astype(np.float64)
            assert (np.abs(got - ref) <= tol).all()


@pytest.mark.parametrize("kind", ["drop_smallest", "unclamped"])
def test_tap_mutants_exceed_the_budget_and_pass_the_batch_maximum(kind):
    pts, L, img_hw = P.bilinear_crafted()
    hf, wf = P.MAPS["32x64"]
    feat = P.features(2, 17, hf, wf)
    host = P.gather_referee(pts, L, img_hw, feat)
    ref, tol = P.gather_budget(host, False)
    wrong = P.gather_referee(pts, L, img_hw, feat, taps=P.taps_mutant(pts, L, img_hw, hf, wf, kind))["ref"]
    err = np.abs(wrong - ref)
    assert (err > tol).any()
    if kind == "drop_smallest":   # the 2^-15 taps alone: what the batch maximum lets through
        w = B.bilinear_taps_host(pts, L, img_hw, hf, wf)[1][:, 0]
        tiny = np.where(w != 0, w, np.float32(1)).min(-1) <= 2.0 ** -14
        assert tiny.sum() >= 10
        err_t, tol_t = err[tiny, 0], tol[tiny, 0]
        assert (err_t > tol_t).any() and err_t.max() <= 1e-4 * max(1.0, np.abs(ref).max())
    else:                         # the outside corners of weight 2^-15
        idx, w, inside, valid, x0, y0 = B.bilinear_taps_host(pts, L, img_hw, hf, wf, with_corner=True)
        small = valid[:, 0] & ((x0[:, 0] == wf - 1) | (y0[:, 0] == hf - 1)) & (x0[:, 0] >= 0) & (y0[:, 0] >= 0)
        wrong_w = P.gather_weights_without_inside_test(pts, L, img_hw, hf, wf)[:, 0]
        small &= (np.where(inside[:, 0], 0, wrong_w).max(-1) <= 2.0 ** -14)
        assert small.sum() >= 3
        assert (err[small, 0] > tol[small, 0]).any() and err[small, 0].max() <= 1e-4 * max(1.0, np.abs(ref).max())
