"""GPU: the camera projection family (csrc/project.hip, csrc/bilinear_taps.h) on the cases of tests/project_cases.py — points put exactly
on a rounding tie, on the image border, on the depth threshold and past the depth clamp, non-finite coordinates, equal camera sums, the
last annotation row and one past it, u8 / i32 planes, 1 to 64 cameras, 1 to 17 classes, and sizes at which every grid-stride loop takes
a second trip; the row list (K26) at 1, 2, 3, 5 and 254 cells and its refusal at 255; the row top-k at its widths; the bilinear forward
gather (K13b) judged per element against `bilinear_taps_host` times the features in float64, on maps from 1 x 1 up and 1 to 256 channels.

Ids, grid values and scores must equal the oracle bit for bit.  What each case reaches, and that a wrong kernel would not pass, is
asserted on the CPU in tests/test_project_cases_cpu.py."""
import numpy as np
import pytest
import torch

import project_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(device):
    from fullysparsefusion_amd import hip_ops

    return hip_ops


@pytest.fixture(scope="module")
def hip_error():
    from fullysparsefusion_amd._lib import FsfHipError

    return FsfHipError


def dev(a, device):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a))).to(device)


def stale(device, *shapes_dtypes):
    """The wrappers allocate their outputs with torch.empty: fill blocks of the same sizes with a pattern and free them first, so that
    an element the kernel does not write holds the pattern, not what an earlier, identical call left there."""
    for shape, dtype in shapes_dtypes:
        t = torch.empty(shape, dtype=dtype, device=device)
        t.view(torch.uint8).fill_(0x5A)
        del t


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def id_outputs(ops, device, name, fused=True):
    """(obj, pts_2d, cam-select score and ids, fused outputs or None) of one case."""
    c = P.id_case(name)
    pts, L, mask, anno = dev(c["pts"], device), dev(c["L"], device), dev(c["mask"], device), dev(c["anno"], device)
    n, (ncam, ncls) = pts.shape[0], c["mask"].shape[:2]
    stale(device, ((n, ncam, ncls), torch.int64), ((ncam, n, 2), torch.float32))
    obj, p2d = ops.project_gather_mask(pts, L, mask, return_pts_2d=True)
    stale(device, ((n, ncls), torch.float32), ((n, ncls), torch.int64))
    score, ids = ops.cam_select_score(obj, anno, score_col=c["score_col"], return_ids=True)
    fused_out = None
    if fused:
        stale(device, ((n, ncls), torch.float32), ((n, ncls), torch.int64), ((n,), torch.uint8), ((n,), torch.uint8), ((n,), torch.int32))
        fused_out = ops.project_score(pts, L, mask, anno, score_col=c["score_col"], return_ids=True, return_fg=True, return_overlap=True)
    return obj, p2d, score, ids, fused_out


def assert_id_case(name, got, groups=None):
    w = P.id_want(name)
    obj, p2d, score, ids, fused = got
    obj_h, p2d_h = obj.cpu().numpy(), p2d.cpu().numpy()
    for group, s in (groups or {"all": slice(None)}).items():       # (by group, so that a failure names the decision)
        np.testing.assert_array_equal(p2d_h[:, s], w["pts_2d"][:, s], err_msg=f"{name} {group}: pts_2d")
        np.testing.assert_array_equal(obj_h[s], w["obj"][s], err_msg=f"{name} {group}: ids")
    np.testing.assert_array_equal(p2d_h.view(np.int32), w["pts_2d"].view(np.int32))
    np.testing.assert_array_equal(obj_h, w["obj"])
    np.testing.assert_array_equal(ids.cpu().numpy(), w["ids"])
    np.testing.assert_array_equal(score.cpu().numpy().view(np.int32), w["score"].view(np.int32))
    if fused is None:
        return
    fscore, fids, ffg, (fg, count, max_id) = fused
    np.testing.assert_array_equal(fids.cpu().numpy(), w["ids"])
    np.testing.assert_array_equal(fscore.cpu().numpy().view(np.int32), w["score"].view(np.int32))
    np.testing.assert_array_equal(ffg.cpu().numpy(), w["fg"])
    np.testing.assert_array_equal(fg.cpu().numpy(), w["fg"].astype(np.uint8))
    np.testing.assert_array_equal(count.cpu().numpy().astype(np.int64), w["count"])
    np.testing.assert_array_equal(max_id.cpu().numpy().astype(np.int64), w["max_id"])
    assert torch.equal(fids, ids) and torch.equal(bits(fscore), bits(score))     # fused == cam_select_score(project_gather_mask(...))


# ------------------------------------------------------------------------------------------------------------------ the id path
def test_pixel_depth_and_non_finite_decisions_equal_the_oracle(ops, device):
    assert_id_case("pixel", id_outputs(ops, device, "pixel"), P.pixel_points()[1])


def test_equal_camera_sums_the_first_maximum_wins(ops, device):
    got = id_outputs(ops, device, "choice")
    assert_id_case("choice", got)
    assert [tuple(r) for r in got[3].cpu().tolist()] == list(P.CHOICE_IDS)
    assert [tuple(r) for r in got[4][1].cpu().tolist()] == list(P.CHOICE_IDS)


@pytest.mark.parametrize("name", ["u8_ncls16", "i32_wide"])
def test_plane_types_and_widths(ops, device, name):
    assert_id_case(name, id_outputs(ops, device, name), P.pixel_points()[1] if name == "i32_wide" else None)


def test_seventeen_classes_the_fused_kernel_refuses_and_the_gather_answers(ops, device, hip_error):
    c = P.id_case("u8_ncls17")
    assert_id_case("u8_ncls17", id_outputs(ops, device, "u8_ncls17", fused=False))
    with pytest.raises(hip_error):
        ops.project_score(dev(c["pts"], device), dev(c["L"], device), dev(c["mask"], device), dev(c["anno"], device), score_col=c["score_col"])


def test_second_trip_of_the_point_loops(ops, device):
    """n = 2048 * 256 + 77: project_score and cam_select_score take a second trip (the unfused gather does not, at two cameras)."""
    got = id_outputs(ops, device, "pixel_second_trip")
    assert_id_case("pixel_second_trip", got)
    w, first = P.id_want("pixel_second_trip"), 2048 * 256
    np.testing.assert_array_equal(got[4][1][first:].cpu().numpy(), w["ids"][first:])     # the rows past the first trip, named
    np.testing.assert_array_equal(got[2][first:].cpu().numpy(), w["score"][first:])


def test_second_trip_of_the_pair_loop_with_64_cameras(ops, device):
    """n * ncam = 32 800 * 64 > 8192 * 256: project_gather_kernel takes a second trip."""
    got = id_outputs(ops, device, "cams64_second_trip")
    assert_id_case("cams64_second_trip", got)
    tail = got[0].reshape(-1)[8192 * 256:].cpu().numpy()
    np.testing.assert_array_equal(tail, P.id_want("cams64_second_trip")["obj"].reshape(-1)[8192 * 256:])


# --------------------------------------------------------------------------------------------------------------- row list (K26)
def row_inputs(ops, device, name):
    c = P.row_case(name)
    pts, L, mask = dev(c["pts"], device), dev(c["L"], device), dev(c["mask"], device)
    anno = torch.zeros((1, 9), device=device)
    n = pts.shape[0]
    stale(device, ((n, 1), torch.float32), ((n,), torch.uint8), ((n,), torch.uint8), ((n,), torch.int32))
    _, _, overlap = ops.project_score(pts, L, mask, anno, return_overlap=True)
    return pts, L, mask, overlap


@pytest.mark.parametrize("name", P.ROW_CASES)
def test_row_list_equals_the_reference_loop(ops, device, name):
    w = P.row_want(name)
    pts, L, mask, (fg, count, max_id) = row_inputs(ops, device, name)
    n = pts.shape[0]
    assert torch.equal(count.cpu().long(), w["k"]) and torch.equal(fg.cpu().bool(), w["k"] > 0)
    assert torch.equal(max_id.cpu().long(), w["obj"].max(-1)[0])
    num_fg, num_multi, num_extra, ws = ops.overlap_plan(fg, count, min(mask.shape[0] * mask.shape[1], 254))
    assert (num_fg, num_multi, num_extra) == (w["F"], w["M"], w["T"])
    batch = (torch.arange(n, device=device) % 4).to(torch.int64)
    for b in (None, batch):
        stale(device, ((num_fg + num_extra,), torch.int64), ((num_fg + num_extra, 3), torch.int64))
        src, coors = ops.overlap_rows(pts, L, mask, max_id, b, ws, num_fg, num_multi, num_extra)
        src_h, coors_h = src.cpu(), coors.cpu()
        assert torch.equal(src_h, w["src"]) and torch.equal(coors_h[:, 2], w["ids"]) and bool((coors_h[:, 1] == 0).all())
        assert torch.equal(coors_h[:, 0], torch.zeros_like(src_h) if b is None else src_h % 4)


@pytest.mark.parametrize("name", P.SATURATED_CASES)
def test_a_saturated_cell_count_is_refused(ops, device, name, hip_error):
    w = P.row_want(name)
    _, _, mask, (fg, count, _) = row_inputs(ops, device, name)
    assert count.cpu().tolist() == [255, 3, 0] and int(w["k"][0]) in (255, 256)
    with pytest.raises(hip_error):
        ops.overlap_plan(fg, count, 254)


def test_max_cells_255_is_refused(ops, device, hip_error):
    _, _, _, (fg, count, _) = row_inputs(ops, device, "cells_254")
    assert ops.overlap_plan(fg, count, 254)[:3] == (2, 2, 255)
    with pytest.raises(hip_error):
        ops.overlap_plan(fg, count, 255)


@pytest.mark.parametrize("name", sorted(P.TOPK_CASES))
def test_row_topk_equals_torch_topk(ops, device, name):
    x, k = P.topk_rows(name)
    stale(device, ((x.shape[0], k), torch.int64))
    got = ops.row_topk_desc(x.to(device), k)
    assert torch.equal(got.cpu(), x.topk(k, dim=-1)[0])


# ------------------------------------------------------------------------------------------- bilinear forward gather (K13b)
WORST = {"ratio": 0.0}


def assert_gather(ops, device, tag, pts, L, img_hw, feat):
    """All four forms (NCHW / channels-last, per camera / summed over cameras) of one input, every element judged against its own budget."""
    host = P.gather_referee(pts, L, img_hw, feat)
    valid = host["valid"]
    d_pts, d_L = dev(pts, device), dev(L, device)
    nchw = dev(feat, device)
    last = nchw.permute(0, 2, 3, 1).contiguous()
    n, (ncam, c) = pts.shape[0], feat.shape[:2]
    outs = {}
    for reduce_cams in (False, True):
        ref, tol = P.gather_budget(host, reduce_cams)
        for layout, f in (("nchw", nchw), ("last", last)):
            stale(device, ((n, c) if reduce_cams else (n, ncam, c), torch.float32), ((n,), torch.uint8))
            got, count = ops.project_gather_bilinear(d_pts, d_L, f, img_hw, channels_last=layout == "last", reduce_cams=reduce_cams,
                                                     return_count=True)
            outs[layout, reduce_cams] = got
            g = got.cpu().numpy().astype(np.float64)
            err = np.abs(g - ref)
            ratio = float((err / np.where(tol > 0, tol, 1.0))[tol > 0].max()) if (tol > 0).any() else 0.0
            WORST["ratio"] = max(WORST["ratio"], ratio)
            print(f"{tag} C={c} {layout} reduce={int(reduce_cams)}: max err / budget {ratio:.3f} (worst so far {WORST['ratio']:.3f})")
            assert np.isfinite(g).all() and (err <= tol).all(), f"{tag} {layout} reduce={reduce_cams}: err / budget {ratio}"
            if reduce_cams:
                assert not g[~valid.any(1)].any()
            else:
                assert not g[~valid].any()                       # an invalid (point, camera) pair is exactly 0
            np.testing.assert_array_equal(count.cpu().numpy(), valid.sum(1).astype(np.uint8))
        assert torch.equal(bits(outs["nchw", reduce_cams]), bits(outs["last", reduce_cams])), f"{tag}: layouts differ, reduce={reduce_cams}"


@pytest.mark.parametrize("c", P.CHANNELS_SCALAR + P.CHANNELS_FLOAT4)
@pytest.mark.parametrize("map_name", list(P.MAPS))
def test_bilinear_gather_per_element(ops, device, map_name, c):
    hf, wf = P.MAPS[map_name]
    for tag, (pts, L, img_hw) in (("crafted", P.bilinear_crafted()), ("selection", P.bilinear_selection())):
        assert_gather(ops, device, f"{tag} {map_name}", pts, L, img_hw, P.features(L.shape[0], c, hf, wf))


def test_bilinear_gather_second_trip(ops, device):
    pts, L, img_hw = P.bilinear_crafted()
    assert_gather(ops, device, "second trip 3x4", P.tiled(pts, P.BILINEAR_TRIP_POINTS), L[:1], img_hw, P.features(1, 4, 3, 4))


def test_bilinear_gather_refuses_a_misaligned_float4_map(ops, device, hip_error):
    pts, L, img_hw = P.bilinear_crafted()
    feat = dev(P.features(2, 8, 3, 4), device).permute(0, 2, 3, 1).contiguous()
    shifted = torch.zeros(feat.numel() + 4, device=device)[1:1 + feat.numel()].view(feat.shape)
    shifted.copy_(feat)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    with pytest.raises(hip_error):
        ops.project_gather_bilinear(dev(pts, device), dev(L, device), shifted, img_hw, channels_last=True)
    feat7 = dev(P.features(2, 7, 3, 4), device).permute(0, 2, 3, 1).contiguous()      # C % 4 != 0 takes the scalar loop: no alignment asked
    shifted7 = torch.zeros(feat7.numel() + 4, device=device)[1:1 + feat7.numel()].view(feat7.shape)
    shifted7.copy_(feat7)
    assert shifted7.data_ptr() % 16 == 4
    assert torch.equal(bits(ops.project_gather_bilinear(dev(pts, device), dev(L, device), shifted7, img_hw, channels_last=True)),
                       bits(ops.project_gather_bilinear(dev(pts, device), dev(L, device), feat7, img_hw, channels_last=True)))
