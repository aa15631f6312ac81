"""The bilinear image-feature gather's backward (K13c, csrc/project_bwd.hip) on the device, against the host specification of
tests/bilinear_cases.py: the forward's taps are the specification's bit for bit, the backward is their exact transpose within the bound
of a fixed-order fp32 sum, the same bits on every run, and the public autograd op on top of both."""
import functools

import numpy as np
import pytest
import torch

import bilinear_cases as bc

pytestmark = pytest.mark.gpu

CHANNELS = (1, 3, 4, 64, 130)


@pytest.fixture(scope="module")
def ops(device):
    from fullysparsefusion_amd import hip_ops_project

    return hip_ops_project


def to_device(a, device):
    return torch.tensor(np.asarray(a)).to(device)  # (a copy: the shared host arrays are read-only)


@functools.lru_cache(maxsize=None)
def grad_rows(n, c, reduce, seed=0):
    u = np.random.default_rng(1000 * c + seed).standard_normal((n, c) if reduce else (n, 6, c)).astype(np.float32)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def host_case(sel, hw, c, reduce):
    """(points, matrices, u, host specification) of one (selection, map, channels, reduce): computed once, shared by the layouts."""
    pts, L = bc.selection(*sel)
    u = grad_rows(pts.shape[0], c, reduce)
    return pts, L, u, bc.bilinear_backward_host(pts, L, u, bc.IMG_HW, hw[0], hw[1], reduce_cams=reduce)


def run_backward(ops, device, pts, L, u, hw, channels_last, reduce, xyz=None):
    """The device result as float64 [ncam, Hf, Wf, C] whichever layout it was produced in."""
    d_xyz = to_device(pts, device) if xyz is None else xyz
    got = ops.project_gather_bilinear_backward(d_xyz, to_device(L, device), to_device(u, device), hw,
                                               bc.IMG_HW, channels_last=channels_last, reduce_cams=reduce)
    ncam, c = L.shape[0], u.shape[-1]
    assert got.shape == ((ncam, hw[0], hw[1], c) if channels_last else (ncam, c, hw[0], hw[1])) and got.dtype == torch.float32
    return (got if channels_last else got.permute(0, 2, 3, 1)).cpu().numpy().astype(np.float64), got


def assert_exact_transpose(got, host, what=""):
    """|got - ref| <= (m_t + 1) 2^-24 sum |a_k u_k| per element; texels without taps exactly 0."""
    err, tol = np.abs(got - host["ref"]), bc.tolerance(host)
    worst = np.unravel_index(np.argmax(err / np.where(tol > 0, tol, np.inf)), err.shape)
    print(f"{what}: largest error {err.max():.3g}, at the tightest element error {err[worst]:.3g} of bound {tol[worst]:.3g}, "
          f"max |ref| {np.abs(host['ref']).max():.3g}, largest texel run {host['taps'].max()}")
    assert np.isfinite(got).all()
    assert (err <= tol).all(), (worst, err[worst], tol[worst])
    assert not got[host["taps"] == 0].any()


# ------------------------------------------------------------------------------------------------ 1. the taps are the forward's
@pytest.mark.parametrize("hf,wf", [(3, 4), (1, 1)])
def test_forward_on_a_one_hot_map_returns_the_host_taps_bit_for_bit(device, hf, wf):
    from fullysparsefusion_amd import hip_ops

    pts, L = bc.selection(4000, 96, 200)
    idx, w, _, valid = bc.bilinear_taps_host(pts, L, bc.IMG_HW, hf, wf)
    t = hf * wf
    want = np.zeros((pts.shape[0], 6, t), dtype=np.float32)
    for k in range(4):  # (a texel takes one non-zero corner of a pair at most: clamped corners weigh zero)
        np.add.at(want, (np.arange(pts.shape[0])[:, None], np.arange(6)[None, :], idx[..., k]), w[..., k])
    live = np.sort(np.where(w != 0, idx, -1 - np.arange(4)), -1)
    assert (np.diff(live, axis=-1) != 0).all()
    feat = torch.eye(t).reshape(1, t, hf, wf).repeat(6, 1, 1, 1).to(device)  # feat[cam, t, y, x] = [t == y * Wf + x]
    d_pts, d_L = to_device(pts, device), to_device(L, device)
    got, count = hip_ops.project_gather_bilinear(d_pts, d_L, feat, bc.IMG_HW, return_count=True)
    assert np.array_equal(got.cpu().numpy(), want)
    got_cl = hip_ops.project_gather_bilinear(d_pts, d_L, feat.permute(0, 2, 3, 1).contiguous(), bc.IMG_HW, channels_last=True)
    assert np.array_equal(got_cl.cpu().numpy(), want)
    assert np.array_equal(count.cpu().numpy(), valid.sum(1).astype(np.uint8)) and (want != 0).sum() > 4000


# ------------------------------------------------------------------------------------------------ 2. exact transpose
@pytest.mark.parametrize("reduce", [False, True], ids=["per_camera", "reduce_cams"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "channels_last"])
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("row", sorted(bc.ROWS))
def test_backward_is_the_exact_transpose(ops, device, row, c, channels_last, reduce):
    sel, hw = bc.ROWS[row]
    pts, L, u, host = host_case(sel, hw, c, reduce)
    got, _ = run_backward(ops, device, pts, L, u, hw, channels_last, reduce)
    assert_exact_transpose(got, host, f"{row} C={c}")


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "channels_last"])
def test_points_as_a_strided_view(ops, device, channels_last):
    sel, hw = bc.ROWS["coarse_3x4"]
    pts, L, u, host = host_case(sel, hw, 4, False)
    wide = torch.full((pts.shape[0], 8), float("nan"), device=device)
    wide[:, 5:8] = to_device(pts, device)
    view = wide[:, 5:8]
    assert view.stride() == (8, 1) and not view.is_contiguous()
    got, _ = run_backward(ops, device, pts, L, u, hw, channels_last, False, xyz=view)
    assert_exact_transpose(got, host, "stride 8")


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "channels_last"])
@pytest.mark.parametrize("c", [3, 8])
def test_no_points_give_the_all_zero_map(ops, device, c, channels_last):
    L = bc.selection(1, 0, 0)[1]
    for reduce in (False, True):
        u = np.zeros((0, c) if reduce else (0, 6, c), dtype=np.float32)
        got, raw = run_backward(ops, device, np.zeros((0, 3), np.float32), L, u, (5, 7), channels_last, reduce)
        assert got.shape == (6, 5, 7, c) and not got.any()
        assert not raw.view(torch.int32).any()  # (+0.0 everywhere, whatever the buffer held)


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "channels_last"])
@pytest.mark.parametrize("visible", [True, False], ids=["visible", "invisible"])
def test_one_point(ops, device, visible, channels_last):
    pts, L = bc.selection(1, 0, 0) if visible else bc.selection(0, 0, 1)
    for c in (1, 4):
        for reduce in (False, True):
            u = grad_rows(1, c, reduce, seed=5)
            host = bc.bilinear_backward_host(pts, L, u, bc.IMG_HW, 3, 4, reduce_cams=reduce)
            assert (1 <= int(host["taps"].sum()) <= 4) if visible else int(host["taps"].sum()) == 0
            got, _ = run_backward(ops, device, pts, L, u, (3, 4), channels_last, reduce)
            assert_exact_transpose(got, host, f"one point C={c}")
            assert bool(got.any()) == visible


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "channels_last"])
@pytest.mark.parametrize("c", [1, 4])
def test_a_run_of_several_chunks(ops, device, c, channels_last):
    """The 1 x 1 row with more single-camera points: one corner's run spans whole chunks, middle ones included, and a tail."""
    from fullysparsefusion_amd import _lib

    chunk = _lib.DEFINES["FSF_BILINEAR_BWD_CHUNK"]
    assert ops.CHUNK == chunk
    pts, L, u, host = host_case(bc.LONG_RUN, (1, 1), c, False)
    run = bc.largest_cell_run(pts, L, 1, 1)
    assert int(host["taps"].max()) >= 2 * chunk + 1 and run >= 2 * chunk + 1 and run % chunk != 0
    got, _ = run_backward(ops, device, pts, L, u, (1, 1), channels_last, False)
    assert_exact_transpose(got, host, f"long run ({run} in one corner)")


# ------------------------------------------------------------------------------------------------ 3. the same bits every run
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "channels_last"])
def test_three_runs_with_differently_poisoned_scratch_give_the_same_bits(ops, device, channels_last):
    from fullysparsefusion_amd import _lib

    sel, hw = bc.ROWS["coarse_3x4"]
    pts, L, u, host = host_case(sel, hw, 64, True)
    d = [to_device(a, device) for a in (pts, L, u)]
    results = []
    for fill in (0x00, 0xFF, None):
        ws = _lib.workspace(1, device)  # the grow-only scratch buffer the wrapper is about to be handed
        if fill is None:
            ws.copy_(torch.randint(0, 256, (ws.numel(),), dtype=torch.uint8, generator=torch.Generator().manual_seed(7)).to(device))
        else:
            ws.fill_(fill)
        results.append(ops.project_gather_bilinear_backward(d[0], d[1], d[2], hw, bc.IMG_HW, channels_last=channels_last, reduce_cams=True))
    assert torch.equal(results[0].view(torch.int32), results[1].view(torch.int32))
    assert torch.equal(results[0].view(torch.int32), results[2].view(torch.int32))
    got = (results[0] if channels_last else results[0].permute(0, 2, 3, 1)).cpu().numpy().astype(np.float64)
    assert_exact_transpose(got, host, "poisoned scratch")


# ------------------------------------------------------------------------------------------------ 4. autograd
def test_autograd_through_a_conv_backbone(ops, device):
    from fullysparsefusion_amd import hip_ops
    from fullysparsefusion_amd.mmdet3d_plugin.ops import PointImageFeatureGather, point_image_gather

    pts, L = bc.selection(1500, 96, 100)
    n = pts.shape[0]
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(3, 8, 3, padding=1).to(device)
    images = torch.randn(6, 3, 24, 40, generator=torch.Generator().manual_seed(4)).to(device)
    d_pts, d_L = to_device(pts, device), to_device(L, device)
    for reduce in (False, True):
        u = grad_rows(n, 8, reduce, seed=9)
        conv.zero_grad()
        feat = conv(images)
        feat.retain_grad()
        out, count = point_image_gather(d_pts, d_L, feat, bc.IMG_HW, reduce_cams=reduce, return_count=True)
        assert out.requires_grad and not count.requires_grad and count.dtype == torch.uint8
        plain, plain_count = hip_ops.project_gather_bilinear(d_pts, d_L, feat.detach(), bc.IMG_HW, reduce_cams=reduce, return_count=True)
        assert torch.equal(out.detach(), plain) and torch.equal(count, plain_count)
        (out * to_device(u, device)).sum().backward()
        host = bc.bilinear_backward_host(pts, L, u, bc.IMG_HW, 24, 40, reduce_cams=reduce)
        assert_exact_transpose(feat.grad.permute(0, 2, 3, 1).cpu().numpy().astype(np.float64), host, f"autograd reduce={reduce}")
        gw = conv.weight.grad
        assert gw is not None and bool(torch.isfinite(gw).all()) and float(gw.abs().max()) > 0
    # no graph without a map that asks for one
    out = point_image_gather(d_pts, d_L, feat.detach(), bc.IMG_HW)
    assert not out.requires_grad and out.grad_fn is None
    # the module form: per-sample lists for B = 2
    mod = PointImageFeatureGather(bc.IMG_HW)
    points = [torch.cat([d_pts, torch.ones(n, 2, device=device)], 1), torch.cat([d_pts[:700], torch.ones(700, 2, device=device)], 1)]
    feat = conv(images)
    outs = mod(points, torch.stack([d_L, d_L]), torch.stack([feat, feat * 2]))
    assert isinstance(outs, list) and [tuple(o.shape) for o in outs] == [(n, 8), (700, 8)]
    want = hip_ops.project_gather_bilinear(d_pts, d_L, feat.detach(), bc.IMG_HW, reduce_cams=True)
    assert torch.equal(outs[0].detach(), want) and torch.equal(outs[1].detach(), want[:700] * 2)
    conv.zero_grad()
    (outs[0].sum() + outs[1].sum()).backward()
    assert float(conv.weight.grad.abs().max()) > 0
