"""GPU parity tests at the reference-shaped API level (fullysparsefusion_amd.mmdet3d_plugin): scatter_v2 and the FSF
glue against goldens produced by the reference's own Python; DynamicScatterVFE / SIR / SimpleSparseUNet / FSF stages
against the CPU oracle modules on the synthetic nuScenes-shape frame.  Index outputs bit-exact, fp32 features within
1e-4 (BASELINE.json north_star)."""
import copy
import os

import numpy as np
import pytest
import torch

import pool_cases
from conftest import build_test_fsf, golden_cases, load_golden, param_checksum
from oracle import modules as omod
from oracle import scatter as oscatter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plugin(device):
    from fullysparsefusion_amd import mmdet3d_plugin

    return mmdet3d_plugin


@pytest.fixture(scope="module")
def fsf_pair(plugin, device):
    """(model on the GPU in eval mode, CPU copy used by the oracle as a weight container)."""
    model = build_test_fsf()
    cpu = copy.deepcopy(model)
    return model.to(device), cpu


def close(a, b, tol=1e-4):
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max())
    assert err <= tol * scale, f"max abs err {err:.3e} (scale {scale:.3e})"


# --------------------------------------------------------------------------------------------- ops level
@pytest.mark.parametrize("case", sorted(golden_cases(load_golden("scatter_v2.npz"))))
def test_scatter_v2_reference_golden(plugin, device, case):
    g = golden_cases(load_golden("scatter_v2.npz"))[case]
    out = plugin.ops.scatter_v2(torch.from_numpy(g["feat"]).to(device), torch.from_numpy(g["coors"]).to(device), str(g["mode"]),
                                min_points=int(g["min_points"]))
    np.testing.assert_array_equal(out[1].cpu().numpy(), g["new_coors"])
    np.testing.assert_array_equal(out[2].cpu().numpy(), g["inv"])
    if str(g["mode"]) == "max":
        np.testing.assert_array_equal(out[0].cpu().numpy(), g["new_feat"])
    else:
        np.testing.assert_allclose(out[0].cpu().numpy(), g["new_feat"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("hint", ["exact", "wide", "too_narrow", "too_wide_for_64_bits"])
def test_unique_with_attached_key_bounds_equals_torch_unique(plugin, device, hint):
    """`with_key_bounds` is a hint: with bounds that hold the unique packs its sort key from them (no range pass, no host wait for it);
    a key outside them, or bounds whose bit widths exceed 64, send the call through the data-dependent range pass — same result."""
    from fullysparsefusion_amd.mmdet3d_plugin.ops.sst_ops import clear_unique_cache, with_key_bounds

    torch.manual_seed(3)
    coors = torch.stack([torch.randint(0, 2, (50000,)), torch.randint(-5, 40, (50000,)), torch.randint(0, 700, (50000,)),
                         torch.randint(0, 700, (50000,))], 1).to(device)
    want = torch.unique(coors, return_inverse=True, return_counts=True, dim=0)
    lo, hi = {"exact": ([0, -5, 0, 0], [1, 39, 699, 699]), "wide": ([0, -100, -100, -100], [7, 1000, 5000, 5000]),
              "too_narrow": ([0, 0, 0, 0], [1, 39, 699, 699]),
              "too_wide_for_64_bits": ([0, -2 ** 40, -2 ** 40, -2 ** 40], [1, 2 ** 40, 2 ** 40, 2 ** 40])}[hint]
    clear_unique_cache()
    got = plugin.ops.unique_with_plan(with_key_bounds(coors.clone(), lo, hi))
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    # explicit bounds (the argument form) stay a contract: a key outside them is an error, not a silent fallback
    if hint == "too_narrow":
        with pytest.raises(Exception, match="row key|bounds|KEY_RANGE|status -3"):
            plugin.ops.unique_with_plan(coors.clone(), lo, hi)


def test_point_linear_add_equals_linear_plus_addend(plugin, device):
    """`point_linear_add` (the 131-wide image-feature update + the LiDAR features in one K22 launch, FSF.py:789-792) against float64;
    the addend is a [:, :131] view of a 132-wide buffer whose last column holds NaN (never read into a result)."""
    from fullysparsefusion_amd.mmdet3d_plugin.ops.sst_ops import PointLinear, point_linear_add

    torch.manual_seed(2)
    n, k, c = 30011, 128, 131
    lin = PointLinear(k, c, bias=True).to(device)
    x = torch.randn(n, k, device=device)
    buf = torch.full((n, 132), float("nan"), device=device)
    buf[:, :c] = torch.randn(n, c, device=device)
    addend = buf[:, :c]
    with torch.no_grad():
        out = point_linear_add(lin, x, addend)
        assert out is not None and out.shape == (n, c) and out.stride(0) == 132
        want = torch.nn.functional.linear(x.double(), lin.weight.double(), lin.bias.double()) + addend.double()
        ref32 = torch.nn.functional.linear(x, lin.weight, lin.bias) + addend
    err, err32 = float((out.double() - want).abs().max()), float((ref32.double() - want).abs().max())
    assert err <= max(2.0 * err32, 2e-6 * float(want.abs().max())), (err, err32)
    assert point_linear_add(lin, x, buf[:, :c].contiguous()) is None  # (an addend without the padded rows: the caller's generic path)


@pytest.mark.parametrize("n,cp,cf,ce", [(50021, 3, 130, 0), (20000, 5, 175, 0), (7001, 3, 128, 13), (1, 3, 4, 2)])
def test_sir_product_training_function_equals_the_aten_chain(plugin, device, n, cp, cf, ce):
    """K28 (`_SirProductFn`: SIRLayer's two concatenations + the product with the position MLP's output, one kernel each way) against
    the ATen chain of SIRLayer.forward (true divisions) — values and the gradients of feats / extra / h bit for bit."""
    from fullysparsefusion_amd.mmdet3d_plugin.models.voxel_encoders.voxel_encoder import _SirProductFn

    torch.manual_seed(n)
    norm, div = (20.0, 20.0, 4.0), 10.0
    points = torch.randn(n, cp, device=device) * 30
    feats = torch.randn(n, cf, device=device, requires_grad=True)
    extra = torch.randn(n, ce, device=device, requires_grad=True) if ce else None
    c = cp + cf + ce
    h = torch.randn(n, c, device=device, requires_grad=True)
    go = torch.randn(n, c, device=device)

    def aten(points, feats, extra, h):
        # (a DEVICE-tensor divisor: ATen's CUDA kernel turns `t / python_scalar` into a multiplication by the rounded reciprocal, which is
        # not the division the reference computes on the CPU — K28, like K21, divides)
        x = torch.cat([points, feats] + ([extra / torch.tensor(div, device=device)] if extra is not None else []), 1)
        x = torch.cat([x[:, :3] / torch.tensor(norm, device=device)[None, :], x[:, 3:]], dim=1)
        return x * h

    leaves = [feats, h] + ([extra] if ce else [])
    want = aten(points, feats, extra, h)
    want_g = torch.autograd.grad(want, leaves, go)
    got = _SirProductFn.apply(points, feats, extra, h, norm, div)
    got_g = torch.autograd.grad(got, leaves, go)
    assert torch.equal(got, want)
    for a, b in zip(got_g, want_g):
        assert torch.equal(a, b)


def test_scatter_v2_precomputed_inverse_and_autograd(plugin, device):
    g = golden_cases(load_golden("scatter_v2.npz"))["k4_max"]
    feat = torch.from_numpy(g["feat"]).to(device).requires_grad_(True)
    coors = torch.from_numpy(g["coors"]).to(device)
    new_coors, inv, _ = plugin.ops.unique_with_plan(coors)
    for mode in ("max", "avg", "sum"):
        out, c2, i2 = plugin.ops.scatter_v2(feat, coors, mode, unq_inv=inv, new_coors=new_coors)
        assert i2 is inv and c2 is new_coors
        f_cpu = torch.from_numpy(g["feat"]).requires_grad_(True)
        ref = oscatter.scatter_v2(f_cpu, g["coors"], mode)[0]
        close(out, ref, 1e-5)
        go = torch.randn_like(ref)
        ref.backward(go)
        (gr,) = torch.autograd.grad(out, feat, go.to(device))
        close(gr, f_cpu.grad, 1e-5)
    with pytest.raises(AssertionError):
        plugin.ops.scatter_v2(feat, coors, "max", unq_inv=inv)  # new_coors must be passed (sst_ops.py:158)
    # an inverse that does not carry a plan (e.g. produced by torch.unique) still works
    c_cpu, i_cpu = torch.unique(torch.from_numpy(g["coors"]), return_inverse=True, dim=0)
    out = plugin.ops.scatter_v2(feat.detach(), coors, "max", unq_inv=i_cpu.to(device), new_coors=c_cpu.to(device))[0]
    np.testing.assert_array_equal(out.cpu().numpy(), g["new_feat"])


def test_voxelization_module(plugin, device):
    from oracle import voxelize as ovox

    v = plugin.ops.Voxelization(voxel_size=(0.2, 0.2, 0.2), point_cloud_range=[-51.2, -51.2, -5, 51.2, 51.2, 3],
                                max_num_points=-1, max_voxels=(-1, -1))
    assert v.grid_size.tolist() == [512, 512, 40]
    rng = np.random.default_rng(0)
    pts = np.concatenate([rng.uniform(-52, 52, (5000, 2)), rng.uniform(-5.2, 3.2, (5000, 1)), rng.random((5000, 2))], 1).astype(np.float32)
    c = v(torch.from_numpy(pts).to(device))
    assert c.dtype == torch.int32
    np.testing.assert_array_equal(c.cpu().numpy(), ovox.dynamic_voxelize(pts, (0.2, 0.2, 0.2), [-51.2, -51.2, -5, 51.2, 51.2, 3]))
    hard = plugin.ops.Voxelization((0.2, 0.2, 0.2), [-51.2, -51.2, -5, 51.2, 51.2, 3], max_num_points=10, max_voxels=1000)
    with pytest.raises(NotImplementedError):
        hard(torch.from_numpy(pts).to(device))


def test_voxel_downsample_vs_the_reference_expression(fsf_pair, device):
    """VoteSegmentor.voxel_downsample (single_stage_fsd.py:263-273): per sample `torch.div(points[:, :3] - range[:3], size,
    rounding_mode='floor').long()` keys (x, y, z order), then `scatter_v2(points, coors, 'avg', return_inv=False)` = rows in
    torch.unique's lexicographic key order, every column averaged.  The reference expression is evaluated here by CPU torch
    (keys bit-exact incl. points ON cell boundaries +-1 ulp, means 1e-5); FSF.forward_hot_path calls it when
    `voxel_downsampling_size` is set (FSF.py:1120-1121)."""
    model, _ = fsf_pair
    seg = model.segmentor
    rng = np.random.default_rng(21)
    size = (0.5, 0.25, 1.0)
    lo = np.array(seg.point_cloud_range[:3], dtype=np.float32)
    pts_list = []
    for n in (40000, 1, 777):
        xyz = rng.uniform([-50, -50, -4.9], [50, 50, 2.9], (n, 3)).astype(np.float32)
        k = min(n, 2000)  # a block of points exactly on cell boundaries and one ulp either side
        cell = rng.integers(1, 150, (k, 3)).astype(np.float32)
        edge = (lo[None] + cell * np.array(size, dtype=np.float32)[None]).astype(np.float32)
        edge = np.nextafter(edge, np.where(rng.random((k, 3)) < 0.5, -np.inf, np.inf).astype(np.float32)) if n > 1 else edge
        xyz[:k] = np.where(rng.random((k, 3)) < 0.7, edge, xyz[:k])
        pts_list.append(np.concatenate([xyz, rng.random((n, 5)).astype(np.float32)], 1))
    old = seg.voxel_downsampling_size
    seg.voxel_downsampling_size = size
    try:
        with torch.no_grad():
            got = seg.voxel_downsample([torch.from_numpy(p).to(device) for p in pts_list])
    finally:
        seg.voxel_downsampling_size = old
    assert len(got) == len(pts_list)
    for p, g in zip(pts_list, got):
        pt = torch.from_numpy(p)
        coors = torch.div(pt[:, :3] - torch.tensor(seg.point_cloud_range)[None, :3], torch.tensor(size)[None, :],
                          rounding_mode="floor").long()
        new_coors, inv = torch.unique(coors, return_inverse=True, dim=0)
        want = torch.zeros((new_coors.shape[0], pt.shape[1]), dtype=torch.float64).index_add_(0, inv, pt.double())
        want = want / torch.bincount(inv, minlength=new_coors.shape[0]).double()[:, None]
        assert g.shape == want.shape, (g.shape, want.shape)   # same number of cells <=> identical keys (the rows are in key order)
        np.testing.assert_allclose(g.cpu().double().numpy(), want.numpy(), rtol=0, atol=1e-5 * 51.2)


def test_get_inner_win_inds_contract(plugin, device):
    g = torch.randint(0, 50, (5000,), device=device)
    r = plugin.ops.get_inner_win_inds(g).cpu()
    gc = g.cpu()
    for v in gc.unique():
        rr = r[gc == v]
        assert sorted(rr.tolist()) == list(range(rr.numel()))  # permutation of 0..n_g-1 (sst_ops.py:225-235)
    assert int((r == 0).sum()) == gc.unique().numel()


def test_connected_components_equal_scipy(device):
    from fullysparsefusion_amd import hip_ops

    rng = np.random.default_rng(1)
    for n, dist in [(1, 0.6), (300, 0.6), (5000, 0.4), (777, 0.05)]:
        pts = torch.from_numpy(np.concatenate([rng.uniform(-10, 10, (n, 2)), rng.uniform(-1, 1, (n, 1))], 1).astype(np.float32))
        want = omod.connected_components_xy(pts, dist)
        got = hip_ops.connected_components(pts.to(device), dist).cpu()
        np.testing.assert_array_equal(got.numpy(), want.numpy())  # same LABELS as scipy, not just the same partition


# ------------------------------------------------------------------------------------- reference-pinned glue
def test_sir_block_wiring_golden(plugin, device):
    """SIR.forward control flow against the reference's own forward run with a recording stand-in layer."""
    g = load_golden("sir_flow.npz")

    class FakeLayer(torch.nn.Module):
        def __init__(self, idx):
            super().__init__()
            self.idx, self.seen = idx, None

        def forward(self, in_feats, coors, f_cluster, return_both=False, unq_inv_once=None, new_coors_once=None):
            self.seen = (in_feats.clone(), unq_inv_once.clone(), new_coors_once.clone())
            m = new_coors_once.size(0)
            pts = in_feats[:, :4] * (self.idx + 1)
            grp = torch.zeros(m, 3, device=in_feats.device).index_add_(0, unq_inv_once, in_feats[:, :3]) + self.idx
            return (pts, grp, new_coors_once) if return_both else (pts, grp)

    sir = plugin.models.SIR(num_blocks=3, in_channels=[12, 9, 9], feat_channels=[[8, 8]] * 3, rel_mlp_hidden_dims=[[4]] * 3,
                            unique_once=True)
    layers = torch.nn.ModuleList([FakeLayer(i) for i in range(3)])
    sir.block_list = layers
    t = lambda k: torch.from_numpy(g[k]).to(device)
    out_feats, cluster_feats, out_coors = sir(t("points"), t("feats"), t("coors"), t("f_cluster"))
    np.testing.assert_array_equal(out_coors.cpu().numpy(), g["out_coors"])
    np.testing.assert_array_equal(layers[0].seen[1].cpu().numpy(), g["unq_inv"])
    np.testing.assert_array_equal(layers[0].seen[2].cpu().numpy(), g["new_coors"])
    np.testing.assert_allclose(layers[1].seen[0].cpu().numpy(), g["block1_in"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(layers[2].seen[0].cpu().numpy(), g["block2_in"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(out_feats.cpu().numpy(), g["out_feats"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(cluster_feats.cpu().numpy(), g["cluster_feats"], rtol=1e-5, atol=1e-5)


def test_frustum_glue_golden(fsf_pair, device):
    model, _ = fsf_pair
    g = load_golden("frustum_glue.npz")
    t = lambda k: torch.from_numpy(g[k]).to(device)
    w = model.get_point_fg_weights(t("logits"))
    np.testing.assert_allclose(w.cpu().numpy(), g["fg_weights"], rtol=1e-6, atol=1e-6)
    a = model.extract_fg_pts(t("feat"), t("bz"), t("points"), t("obj_id"), t("fg_weights"))
    for got, key in zip(a, ["fg_feat", "fg_bz", "fg_points", "fg_obj", "fg_w"]):
        np.testing.assert_array_equal(got.cpu().numpy(), g[key])
    b = model.double_overlap_pts(*a)
    for got, key in zip(b, ["dup_feat", "dup_bz", "dup_points", "dup_obj", "dup_w"]):
        np.testing.assert_array_equal(got.cpu().numpy(), g[key])  # same rows in the same order
    sir_coors, _ = model.get_sir_coors(b[1], b[3], b[4])
    np.testing.assert_array_equal(sir_coors.cpu().numpy(), g["sir_coors"])
    f_cluster, center, ccoors = model.get_cluster_delta_weighted(b[2], sir_coors, b[4].unsqueeze(-1))
    if hasattr(f_cluster, "materialize"):  # (inference: the offsets are formed inside the SIR stack's permutation pass, K29a)
        f_cluster = f_cluster.materialize()
    np.testing.assert_array_equal(ccoors.cpu().numpy(), g["cluster_coors"])
    np.testing.assert_allclose(center.cpu().numpy(), g["cluster_center"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(f_cluster.cpu().numpy(), g["f_cluster"], rtol=1e-4, atol=1e-4)
    single = model.get_single_cls_preds_2d(t("mask_anno"), ccoors)
    np.testing.assert_array_equal(single.cpu().numpy(), g["single_preds"])


def test_neck_module_golden(plugin, device):
    g = load_golden("neck.npz")
    neck = plugin.models.Voxel2PointScatterNeck(point_cloud_range=g["pc_range"].tolist(), voxel_size=g["voxel_size"].tolist()).eval()
    t = lambda k: torch.from_numpy(g[k]).to(device)
    out, mask = neck(t("points"), t("coors"), t("voxel_feats"), t("inv"), -1)
    np.testing.assert_array_equal(mask.cpu().numpy(), g["mask"])
    np.testing.assert_array_equal(out.cpu().numpy(), g["out"])


def test_img_cross_attn_fused_equals_generic_path(fsf_pair, device):
    """The fused cam-select/score kernel against the reference-shaped torch path (get_all_cls_preds_2d + encode)."""
    model, _ = fsf_pair
    g = golden_cases(load_golden("project.npz"))["nusc_mid"]
    n = g["points"].shape[0]
    pts = torch.from_numpy(g["points"]).to(device)
    bidx = torch.zeros(n, dtype=torch.int64, device=device)
    mask = torch.from_numpy(g["mask"]).to(device)[None]
    anno = torch.from_numpy(g["mask_anno"]).to(device)[None]
    metas = [dict(lidar2img=g["lidar2img"])]
    ident = torch.nn.Identity()
    model._gather_cache = None
    fused = model.img_cross_attn([pts], bidx, anno, mask, metas, ident)
    np.testing.assert_array_equal(fused.cpu().numpy(), g["score"])
    model.is_argo, model._gather_cache = True, None  # forces the generic branch; encode_single_cls=True there
    try:
        obj = model.frustum_gather(bidx, pts, mask, anno, metas)
        np.testing.assert_array_equal(obj.cpu().numpy(), g["obj_id"])
        multi = obj.masked_select(torch.nn.functional.one_hot(obj.sum(-1).max(-1)[1], 6).bool().unsqueeze(-1)).reshape(-1, 10)
        preds = model.get_all_cls_preds_2d(anno, bidx, multi)
        assert preds.shape == (n, 10, 9)
        np.testing.assert_array_equal(preds[..., 4].cpu().numpy(), g["score"])
        assert bool((preds[..., 5][multi == 0] == 10).all())  # id 0 -> category = num_classes (FSF.py:528)
    finally:
        model.is_argo, model._gather_cache = False, None


# ------------------------------------------------------------------------------------------ module parity
@pytest.fixture(scope="module")
def frame1():
    from fullysparsefusion_amd import synthetic

    return synthetic.make_frame(num_sweeps=1, seed=0)


def test_vfe_vs_oracle(fsf_pair, frame1, device):
    model, cpu = fsf_pair
    pts = torch.from_numpy(frame1["points"][:, :5].copy())
    seg = model.segmentor
    p_dev, coors = seg.voxelize([pts.to(device)])
    vf, vc, inv = seg.voxel_encoder(p_dev, coors, return_inv=True)
    from oracle import voxelize as ovox

    _, ocoors = ovox.voxelize_batch([pts.numpy()], seg.voxel_size, seg.point_cloud_range)
    np.testing.assert_array_equal(coors.cpu().numpy(), ocoors)
    ovf, ovc, oinv = omod.vfe_forward(cpu.segmentor.voxel_encoder, pts, torch.from_numpy(ocoors))
    np.testing.assert_array_equal(vc.cpu().numpy(), ovc.numpy())
    np.testing.assert_array_equal(inv.cpu().numpy(), oinv.numpy())
    close(vf, ovf)


def test_sparse_unet_vs_oracle(fsf_pair, frame1, device):
    model, cpu = fsf_pair
    pts = torch.from_numpy(frame1["points"][:, :5].copy())
    ex = omod.segmentor_extract_feat(cpu.segmentor, [pts])
    with torch.no_grad():
        out = model.segmentor.backbone(dict(voxel_feats=ex["voxel_feats"].to(device), voxel_coors=ex["voxel_coors"].to(device),
                                            batch_size=1))[0]["voxel_feats"]
    assert out.shape == (ex["voxel_coors"].shape[0], 128)
    close(out, ex["unet"])
    with torch.no_grad():
        (neck_out, mask), coors, _ = model.segmentor.extract_feat([pts.to(device)], None)
    assert bool(mask.all())
    np.testing.assert_array_equal(coors.cpu().numpy(), ex["coors"].numpy())
    close(neck_out, ex["neck"])


def test_sparse_unet_on_the_planes_kernel_vs_oracle(fsf_pair, frame1, device, monkeypatch):
    """The same U-Net comparison with K9c (pre-split f16 planes) forced onto every submanifold layer it supports (the
    1-sweep levels are below its row threshold otherwise): plane-form hand-over between layers, the two-source merge
    layers, the 64 / 128 / 256-channel variants, small row blocks."""
    from fullysparsefusion_amd import hip_ops
    from fullysparsefusion_amd.mmdet3d_plugin.ops import spconv as sp

    model, cpu = fsf_pair
    pts = torch.from_numpy(frame1["points"][:, :5].copy())
    ex = omod.segmentor_extract_feat(cpu.segmentor, [pts])
    calls = []
    orig = hip_ops.spconv_forward_planes

    def spy(sources, *a, **k):
        calls.append(([p.c for p in sources], a[2]))
        return orig(sources, *a, **k)

    monkeypatch.setattr(hip_ops, "spconv_forward_planes", spy)
    monkeypatch.setattr(sp.SparseConvolution, "PLANES_MIN_ROWS", 64)
    with torch.no_grad():
        out = model.segmentor.backbone(dict(voxel_feats=ex["voxel_feats"].to(device), voxel_coors=ex["voxel_coors"].to(device),
                                            batch_size=1))[0]["voxel_feats"]
    close(out, ex["unet"])
    assert len(calls) >= 20 and ([128, 128], 128) in calls and ([64], 64) in calls and any(c[1] == 256 for c in calls)


def test_sparse_unet_layers_run_on_the_kernels_the_decision_names(fsf_pair, frame1, device, monkeypatch):
    """Every convolution of a U-Net inference, with the default row thresholds and with the plane kernel's lowered to 64: the
    hip_ops entry each layer calls, with (cin, cout, table rows), is the one `choose_kernel` names for the layer's kind and shape, the
    rows of its table and input and the plane sources handed to it; the two runs together reach all four entries."""
    from fullysparsefusion_amd import hip_ops, switches
    from fullysparsefusion_amd.mmdet3d_plugin.ops import spconv as sp

    model, cpu = fsf_pair
    pts = torch.from_numpy(frame1["points"][:, :5].copy())
    ex = omod.segmentor_extract_feat(cpu.segmentor, [pts])
    entry_of = {sp.PLANES: "spconv_forward_planes", sp.SPLIT_F16: "spconv_forward_split_planes", sp.SPLIT: "spconv_forward_split",
                sp.FP32: "spconv_forward"}
    shape_of = {  # entry -> (cin, cout, table rows) of a call's arguments
        "spconv_forward": lambda feat, weight_t, nbr, **k: (feat.size(1), weight_t.size(1), nbr.size(0)),
        "spconv_forward_split": lambda feat, planes, kvol, cout, nbr, **k: (feat.size(1), cout, nbr.size(0)),
        "spconv_forward_split_planes": lambda xp, planes, kvol, cout, nbr, **k: (xp.c, cout, nbr.size(0)),
        "spconv_forward_planes": lambda sources, wplanes, kvol, cout, nbr, **k: (sum(p.c for p in sources), cout, nbr.size(0)),
    }
    called, predicted = [], []

    def spy_on(name):
        orig = getattr(hip_ops, name)

        def spy(*a, **k):
            called.append((name, *shape_of[name](*a, **k)))
            return orig(*a, **k)

        monkeypatch.setattr(hip_ops, name, spy)

    for name in shape_of:
        spy_on(name)
    layer_forward = sp.SparseConvolution.forward

    def predicting_forward(self, x, *a, **k):
        rb = self._rulebook(x)
        rows = (rb.nbr_inv if self.inverse else rb.nbr).size(0)
        widths = None if x.plane_sources is None else [p.c for p in x.plane_sources]
        kind = "subm" if self.subm else "inverse" if self.inverse else "strided"
        kernel = sp.choose_kernel(kind, self.in_channels, self.out_channels, 27, rows, x.indices.size(0), widths, False, switches.PLANES,
                                  switches.TRAIN_PLANES)
        predicted.append((entry_of[kernel], self.in_channels, self.out_channels, rows))
        return layer_forward(self, x, *a, **k)

    monkeypatch.setattr(sp.SparseConvolution, "forward", predicting_forward)
    inputs = dict(voxel_feats=ex["voxel_feats"].to(device), voxel_coors=ex["voxel_coors"].to(device), batch_size=1)
    with torch.no_grad():
        model.segmentor.backbone(inputs)
        default_run = len(called)
        monkeypatch.setattr(sp.SparseConvolution, "PLANES_MIN_ROWS", 64)
        model.segmentor.backbone(inputs)
    assert default_run >= 20 and len(called) == 2 * default_run == len(predicted), (default_run, len(called), len(predicted))
    assert called == predicted, [(c, p) for c, p in zip(called, predicted) if c != p][:4]
    assert {c[0] for c in called} == set(shape_of), sorted({c[0] for c in called})
    assert called[:default_run] != called[default_run:]  # (the lowered threshold moved layers onto the plane kernel)


@pytest.mark.parametrize("norm,act,c", [(dict(type="LN", eps=1e-3), "gelu", 64), (dict(type="naiveSyncBN1d", eps=1e-3, momentum=0.01), "relu", 64),
                                        (dict(type="LN", eps=1e-3), "gelu", 16)])  # 16 channels: the library product + fsf_gather_rows_add
def test_grouped_concat_training_equals_the_concat_path(plugin, device, monkeypatch, norm, act, c):
    """Training: two DynamicVFELayer steps where the second layer's Linear over cat([point, group[inv]], 1) is taken as
    p W_left^T + (g W_right^T)[inv] (sst_ops._grouped_linear_training, fsf_gather_rows_add + segmented-sum adjoint).  Outputs and
    every gradient equal the materialised-concat path (itself pinned by the oracle tests) within fp32 rounding, and a float64
    torch restatement of the two layers within 1e-4."""
    from fullysparsefusion_amd.mmdet3d_plugin.models.voxel_encoders.voxel_encoder import DynamicVFELayer
    from fullysparsefusion_amd.mmdet3d_plugin.ops import sst_ops

    torch.manual_seed(5)
    rng = np.random.default_rng(6)
    n, cin = 40000, 32
    l1, l2 = DynamicVFELayer(cin, c, norm, act=act).to(device).train(), DynamicVFELayer(2 * c, c, norm, act=act).to(device).train()
    coors = torch.from_numpy(rng.integers(0, 14, size=(n, 3)).astype(np.int64)).to(device)
    x0 = torch.from_numpy(rng.standard_normal((n, cin)).astype(np.float32))
    probe = torch.from_numpy(rng.standard_normal((n, c)).astype(np.float32)).to(device)

    real_grouped = sst_ops._grouped_linear_training

    def run(grouped):
        # (reference form: the deferred concat is written out and the layer runs on the [n, 2C] tensor)
        monkeypatch.setattr(sst_ops, "_grouped_linear_training", real_grouped if grouped else (lambda *a, **k: None))
        for m in (l1, l2):
            m.zero_grad()
        x = x0.to(device).requires_grad_()
        _, _, gcoors, inv, cat = sst_ops.point_group_concat(l1, x, coors, "max", None, None, want_concat=True)
        assert isinstance(cat, sst_ops.GroupedConcat)
        pf, gf, _, _, _ = sst_ops.point_group_concat(l2, cat, coors, "max", inv, gcoors, want_concat=False)
        ((pf * probe).sum() + gf.sum()).backward()
        return [pf.detach(), gf.detach(), x.grad] + [p.grad.clone() for m in (l1, l2) for p in m.parameters()], inv

    got, inv = run(True)
    want, _ = run(False)
    for a, b in zip(got, want):
        scale = max(float(b.abs().max()), 1e-6)
        assert float((a - b).abs().max()) <= 2e-5 * scale, (a.shape, float((a - b).abs().max()), scale)
    # float64 restatement (training-mode norms: LayerNorm per row / batch statistics per column)
    d1, d2 = copy.deepcopy(l1).double().cpu(), copy.deepcopy(l2).double().cpu()
    for m in (d1, d2):
        m.zero_grad()
    x = x0.double().requires_grad_()
    inv_c = inv.cpu()
    ngroups = int(inv_c.max()) + 1

    def seg_max(t):
        out = torch.full((ngroups, t.size(1)), -float("inf"), dtype=t.dtype)
        return out.scatter_reduce(0, inv_c[:, None].expand(-1, t.size(1)), t, "amax", include_self=True)

    p1 = d1.act(d1.norm(d1.linear(x)))
    p2 = d2.act(d2.norm(d2.linear(torch.cat([p1, seg_max(p1)[inv_c]], 1))))
    ((p2 * probe.cpu().double()).sum() + seg_max(p2).sum()).backward()
    ref = [p2.detach(), seg_max(p2).detach(), x.grad] + [p.grad for m in (d1, d2) for p in m.parameters()]
    # (a group maximum whose two largest candidates differ by fp32 rounding picks another row in float64: the gradient of that
    # (group, channel) moves to a different point — a handful of rows may differ, the parameter gradients barely notice)
    for i, (a, b) in enumerate(zip(got, ref)):
        scale = max(float(b.abs().max()), 1e-6)
        err = (a.cpu().double() - b).abs()
        if i == 2:
            bad_rows = int((err.max(1)[0] > 1e-4 * scale).sum())
            assert bad_rows <= n // 500, (bad_rows, n)
        else:
            assert float(err.max()) <= (1e-4 if i < 2 else 2e-3) * scale, (i, a.shape, float(err.max()), scale)


def test_sparse_unet_training_backward_vs_oracle(plugin, device):
    """Config-3 'fwd+bwd' on the backbone: training-mode SimpleSparseUNet (batch-stat norms) forward and the gradients
    of every conv weight / norm parameter / the input features, against autograd through the CPU restatement."""
    torch.manual_seed(3)
    cfg = dict(type="SimpleSparseUNet", in_channels=64, sparse_shape=[16, 64, 64], order=("conv", "norm", "act"),
               norm_cfg=dict(type="naiveSyncBN1d", eps=1e-3, momentum=0.01), base_channels=64, output_channels=128,
               encoder_channels=((64,), (64, 64, 64), (128, 128, 128)), encoder_paddings=((1,), (1, 1, 1), (1, 1, 1)),
               decoder_channels=((128, 128, 64), (64, 64, 64), (64, 64, 64)), decoder_paddings=((1, 0), (1, 0), (0, 1)))
    net = plugin.registry.build_backbone(cfg).train()
    cpu = copy.deepcopy(net)
    net.to(device)
    rng = np.random.default_rng(4)
    cells = rng.choice(2 * 4 * 64 * 64, size=6000, replace=False)
    cells.sort()
    coors = np.stack([cells // (4 * 64 * 64), 5 + cells // (64 * 64) % 4, cells // 64 % 64, cells % 64], 1).astype(np.int64)
    feats = torch.from_numpy(rng.standard_normal((coors.shape[0], 64)).astype(np.float32))
    probe = torch.from_numpy(rng.standard_normal((coors.shape[0], 64)).astype(np.float32))  # fixed d(loss)/d(out)

    def run_oracle(module, dtype):
        f = feats.detach().clone().to(dtype).requires_grad_()
        o = omod.unet_forward(module, f, torch.from_numpy(coors), 2, train=True)
        (o * probe.to(dtype)).sum().backward()
        grads = {"input": f.grad}
        grads.update({n: p.grad for n, p in module.named_parameters()})
        return o.detach(), grads

    want, g32 = run_oracle(cpu, torch.float32)
    _, g64 = run_oracle(copy.deepcopy(cpu).double(), torch.float64)  # yardstick for how ill-conditioned each gradient is

    f_dev = feats.detach().clone().to(device).requires_grad_()
    out = net(dict(voxel_feats=f_dev, voxel_coors=torch.from_numpy(coors).to(device), batch_size=2))[0]["voxel_feats"]
    close(out.detach(), want)
    (out * probe.to(device)).sum().backward()
    got = {"input": f_dev.grad}
    got.update({n: p.grad for n, p in net.named_parameters()})

    def rel(a, b):
        return float((a.double().cpu() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))

    def rel_l2(a, b):
        return float((a.double().cpu() - b.double()).norm() / b.double().norm().clamp_min(1e-30))

    bad, loose = {}, {}
    for name, g in g64.items():
        assert got[name] is not None, name
        ours, cpu32 = rel(got[name], g), rel(g32[name], g)
        # a 20-layer net with batch-stat norms amplifies fp32 rounding; our gradient must be as close to the fp64 truth
        # as the CPU fp32 restatement is (same order of magnitude), and within 1e-4 where the problem is well conditioned
        if ours > max(1e-4, 10.0 * cpu32):
            loose[name] = (ours, cpu32)
            # ... except downstream of a ReLU input within rounding of zero that lands on the other side of it than on
            # the CPU (the split-bf16 kernel sums in a different order than the fp32 one): that perturbs the gradients
            # behind it by a few 1e-4 — and ONE entry of a bias / norm gradient (a 6000-row column sum) by the flipped element's
            # own upstream gradient, 1-2 % of that entry (which element flips changes with any 1-ulp change upstream, e.g. the
            # rsqrt of the batch variance).  A wiring error is O(1) everywhere; bound those by relative L2 <= 5e-3 with at most
            # 5 % of the entries (2 at least) off by more than 1e-3 of the scale, and allow them on at most a fifth of the
            # parameters (seen: the four tensors of lateral_layer1).
            l2 = rel_l2(got[name], g)
            err = (got[name].double().cpu() - g.double()).abs()
            off = int((err > 1e-3 * float(g.double().abs().max())).sum())
            print(f"loose {name}: max-rel {ours:.2e} (cpu fp32 {cpu32:.2e}), rel-L2 {l2:.2e}, {off} of {err.numel()} entries off")
            if l2 > 5e-3 or off > max(2, err.numel() // 20):
                bad[name] = (ours, cpu32, l2, off)
    assert not bad, bad
    assert len(loose) <= len(g64) // 5, loose


def test_sir_vs_oracle(fsf_pair, device):
    model, cpu = fsf_pair
    rng = np.random.default_rng(5)
    n = 20000
    points = torch.from_numpy(rng.uniform(-30, 30, (n, 5)).astype(np.float32))
    feats = torch.from_numpy(rng.standard_normal((n, 131)).astype(np.float32))
    ids = rng.integers(0, 180, n)
    ids[:7000] = 3  # one giant group, like a truck's frustum
    coors = torch.from_numpy(np.stack([np.zeros(n), np.zeros(n), ids], 1).astype(np.int64))
    f_cluster = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32))
    from fullysparsefusion_amd import switches

    sir = model.frustum_sir
    assert sir.point_feats_needed is False  # the detector only reads the group features (FSF.py:436-447)
    with torch.no_grad():
        none_pf, cf_fast, _ = sir(points.to(device), feats.to(device), coors.to(device), f_cluster.to(device))
        sir.point_feats_needed = True
        try:
            pf, cf, oc = sir(points.to(device), feats.to(device), coors.to(device), f_cluster.to(device))
            switches.SIR_SORTED = False  # the segment-plan path (rows in input order, separate segmented-max launches)
            try:
                pf_plan, cf_plan, oc_plan = sir(points.to(device), feats.to(device), coors.to(device), f_cluster.to(device))
            finally:
                switches.SIR_SORTED = True
        finally:
            sir.point_feats_needed = False
        opf, ocf, ooc = omod.sir_forward(cpu.frustum_sir, points, feats, coors, f_cluster)
    np.testing.assert_array_equal(oc.cpu().numpy(), ooc.numpy())
    assert cf.shape == (ooc.shape[0], 768)
    close(pf, opf)
    close(cf, ocf)
    # rows sorted by group + K22s (the default) == rows in input order + fsf_segment_reduce: every row's arithmetic is the same and
    # max is exact, so the two paths agree bit for bit
    assert none_pf is None and torch.equal(cf_fast, cf) and torch.equal(cf, cf_plan) and torch.equal(pf, pf_plan)
    assert torch.equal(oc, oc_plan)


def test_fsf_hot_path_vs_oracle(fsf_pair, frame1, device):
    """Stages 1-3 of FSF.simple_test on a synthetic single-sweep frame with the 6 x 10 x 900 x 1600 u8 masks.
    Stage 1 is compared end to end; stages 2 and 3 are then run on the ORACLE's stage-1 output so that their
    integer decisions (fg thresholds, voxel keys, cluster ids) see identical inputs and must match bit-exactly —
    a 1e-6 GEMM rounding difference upstream may legitimately move a point across a 0.05 m voxel boundary."""
    model, cpu = fsf_pair
    f = frame1
    pts8 = torch.from_numpy(f["points"])
    mask = torch.from_numpy(f["mask_data"])
    anno = torch.from_numpy(f["mask_anno"])
    L = torch.from_numpy(f["lidar2img"])
    metas = [dict(lidar2img=f["lidar2img"])]
    with torch.no_grad():
        out = model.forward_hot_path([pts8.to(device)], metas, mask.to(device)[None], anno.to(device)[None])
        s1 = omod.fsf_stage1(cpu, pts8, mask, anno, L)
        s2 = omod.fsf_stage2(cpu, s1, anno, (900, 1600))
        s3 = omod.fsf_stage3(cpu, s1)
    seg = out["seg"]
    close(seg["seg_feats"], s1["seg_feats"])
    close(seg["seg_logits"], s1["seg_logits"])
    close(seg["offsets"], s1["offsets"])
    # camera-query grouping depends only on the (bit-exact) projection: must match even end to end
    np.testing.assert_array_equal(out["frustum_obj_coors"].cpu().numpy(), s2["obj_coors"].numpy())
    assert out["frustum_obj_feats"].shape == (s2["obj_coors"].shape[0], 896)
    assert torch.isfinite(out["fsd_obj_feats"]).all() and out["fsd_obj_feats"].shape[1] == 768

    seg_dev = {k: s1[k].to(device) for k in ["seg_points", "seg_logits", "seg_vote_preds", "offsets", "seg_feats", "batch_idx"]}
    infos = [pts8[:, -3:].to(device)]
    with torch.no_grad():
        model._gather_cache = None
        f_feats, f_centers, f_coors, _, f_preds = model.frustum_forward(seg_dev, anno.to(device)[None], mask.to(device)[None], infos,
                                                                        metas, run_head=False)
        # capture what the LiDAR-query SIR receives inside the real pipeline
        cap = {}
        sir_fwd = model.backbone.forward

        def capture(points, features, coors, f_cluster=None):
            cap["in"] = (points, features.materialize() if hasattr(features, "materialize") else features, coors,
                         f_cluster.materialize() if hasattr(f_cluster, "materialize") else f_cluster)
            return sir_fwd(points, features, coors, f_cluster)

        model.backbone.forward = capture
        try:
            l_feats, l_xyz, l_inds, _ = model.fsd_forward(seg_dev, metas, run_head=False)
        finally:
            model.backbone.forward = sir_fwd
        model._gather_cache = None
    np.testing.assert_array_equal(f_coors.cpu().numpy(), s2["obj_coors"].numpy())
    np.testing.assert_array_equal(f_preds.cpu().numpy(), s2["preds_2d"].numpy())
    close(f_centers, s2["obj_centers"])
    close(f_feats, s2["obj_feat"])
    # LiDAR queries: every integer decision (pre-voxel keys, fg sampling, cluster voxels, component labels) bit-exact
    np.testing.assert_array_equal(l_inds.cpu().numpy(), s3["cluster_inds"].numpy())
    np.testing.assert_array_equal(cap["in"][2].cpu().long().numpy(), s3["pts_cluster_inds"].long().numpy())
    # centroids: fp32 means whose summation order differs (deterministic chunks here, sequential index_add in the
    # oracle, atomics upstream): a few ulp of the 50 m coordinate range
    assert float((l_xyz.cpu() - s3["cluster_xyz"]).abs().max()) < 5e-5
    # The SIR output is ill-conditioned in f_cluster near 0 (three LayerNorm(eps=1e-3) layers in rel_mlp amplify a
    # 1e-5 m centroid rounding difference ~30x each), so features are compared on IDENTICAL SIR inputs: the ones the
    # GPU pipeline actually produced, replayed through the oracle SIR.
    gp, gfe, gco, gfc = [t.cpu() for t in cap["in"]]
    with torch.no_grad():
        _, want_feats, want_coors = omod.sir_forward(cpu.backbone, gp, gfe, gco, gfc)
    np.testing.assert_array_equal(l_inds.cpu().numpy(), want_coors.numpy())
    close(l_feats, want_feats)
    assert s3["cluster_inds"].shape[0] > 10 and s2["obj_coors"].shape[0] > 10


# ------------------------------------------------------------------------ Argoverse-2 shape (BASELINE config 5)
AV2_RANGE = [-204.8, -204.8, -3.2, 204.8, 204.8, 3.2]
AV2_SEGMENTOR = dict(
    type="VoteSegmentor", tanh_dims=[],
    voxel_layer=dict(voxel_size=(0.2, 0.2, 0.2), max_num_points=-1, point_cloud_range=AV2_RANGE, max_voxels=(-1, -1)),
    voxel_encoder=dict(type="DynamicScatterVFE", in_channels=4, feat_channels=[64, 64], voxel_size=(0.2, 0.2, 0.2),
                       with_cluster_center=True, with_voxel_center=True, point_cloud_range=AV2_RANGE,
                       norm_cfg=dict(type="naiveSyncBN1d", eps=1e-3, momentum=0.01)),
    middle_encoder=dict(type="PseudoMiddleEncoderForSpconvFSD"),
    backbone=dict(type="SimpleSparseUNet", in_channels=64, sparse_shape=[32, 2048, 2048], order=("conv", "norm", "act"),
                  norm_cfg=dict(type="naiveSyncBN1d", eps=1e-3, momentum=0.01), base_channels=64, output_channels=128,
                  encoder_channels=((64,), (64, 64, 64), (64, 64, 64), (128, 128, 128)),
                  encoder_paddings=((1,), (1, 1, 1), (1, 1, 1), ((0, 1, 1), 1, 1)),
                  decoder_channels=((128, 128, 64), (64, 64, 64), (64, 64, 64), (64, 64, 64)),
                  decoder_paddings=((1, 0), (1, 0), (0, 0), (0, 1))),
    decode_neck=dict(type="Voxel2PointScatterNeck", voxel_size=(0.2, 0.2, 0.2), point_cloud_range=AV2_RANGE),
    segmentation_head=dict(type="VoteSegHead", in_channel=67, hidden_dims=[128, 128], num_classes=26, dropout_ratio=0.0,
                           norm_cfg=dict(type="naiveSyncBN1d"), act_cfg=dict(type="ReLU"),
                           loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=3.0),
                           loss_vote=dict(type="L1Loss", loss_weight=1.0)),
)


def test_av2_long_range_segmentor_vs_oracle(plugin, device):
    """±204.8 m range, 2048 x 2048 x 32 grid (spconv v1 would allocate a 537 MB dense grid per sample; the hash
    rulebook does not care), 4-d points, VFE without unique_once, 4-stage U-Net with 64-wide layers."""
    torch.manual_seed(1)
    seg = plugin.registry.build_detector(AV2_SEGMENTOR).eval()
    for m in seg.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    cpu = copy.deepcopy(seg)
    seg.to(device)
    rng = np.random.default_rng(2)
    n = 40000
    r = rng.uniform(2.0, 200.0, n) ** 1.0
    a = rng.uniform(-np.pi, np.pi, n)
    pts = np.stack([r * np.cos(a), r * np.sin(a), rng.normal(-1.5, 0.4, n).clip(-3.1, 3.1), rng.random(n)], 1).astype(np.float32)
    pts = pts[(np.abs(pts[:, 0]) < 204.7) & (np.abs(pts[:, 1]) < 204.7)]
    t = torch.from_numpy(pts)
    ex = omod.segmentor_extract_feat(cpu, [t])
    with torch.no_grad():
        (neck_out, mask), coors, _ = seg.extract_feat([t.to(device)], None)
    np.testing.assert_array_equal(coors.cpu().numpy(), ex["coors"].numpy())
    assert int(ex["coors"][:, 3].max()) > 1500 and int(ex["coors"][:, 2].max()) > 1500  # really uses the 2048^2 grid
    assert neck_out.shape == (pts.shape[0], 67)
    close(neck_out, ex["neck"])


# ----------------------------------------------------------------------------------- query refinement (f2 / f3)
def test_refine_head_vs_oracle(plugin, device):
    """DynamicPointROIExtractor (K17) + FullySparseBboxHead on the same pooled points as the oracle."""
    from oracle import refine as orefine

    torch.manual_seed(5)
    rng = np.random.default_rng(6)
    head = plugin.registry.build_head(dict(
        type="FullySparseBboxHead", num_classes=10, num_blocks=3, in_channels=[5 + 40 + 13, 5 + 128 + 13, 5 + 128 + 13],
        feat_channels=[[128, 128]] * 3, with_distance=False, with_cluster_center=False, with_rel_mlp=True,
        rel_mlp_hidden_dims=[[16, 32]] * 3, rel_mlp_in_channels=[13] * 3, reg_mlp=[512, 512], cls_mlp=[512, 512], mode="max",
        xyz_normalizer=[20, 20, 4], cat_voxel_feats=True, pos_fusion="mul", fusion="cat", act="gelu", geo_input=True,
        use_middle_cluster_feature=True, norm_cfg=dict(type="LN", eps=1e-3), unique_once=True)).eval()
    cpu = copy.deepcopy(head)
    head.to(device)
    r, p = 60, 20000
    rois = np.concatenate([np.zeros((r, 1)), rng.uniform(-30, 30, (r, 2)), rng.uniform(-2.5, -1.0, (r, 1)),
                           rng.uniform(1.5, 2.5, (r, 1)), rng.uniform(3.0, 6.0, (r, 1)), rng.uniform(1.2, 2.5, (r, 1)),
                           rng.uniform(-3.1, 3.1, (r, 1))], 1).astype(np.float32)
    rois[7, 1:3] = 400.0  # an RoI with no points: its feature row must stay zero
    which = rng.integers(0, r, p // 2)
    which[which == 7] = 0
    near = rois[which, 1:4] + rng.normal(0, 1.2, (p // 2, 3)) + np.array([0, 0, 1.0])
    pts = np.concatenate([near, np.concatenate([rng.uniform(-35, 35, (p - p // 2, 2)), rng.uniform(-3, 1, (p - p // 2, 1))], 1)])
    pts = np.concatenate([pts, rng.random((p, 2))], 1).astype(np.float32)
    pts[:, :3], parked, _ = pool_cases.margin_clean(rois[:, 1:], pts[:, :3], [1.0, 1.0, 1.0])  # no pair within 1e-3 of a face
    assert parked.size <= 0.02 * p
    feats = rng.standard_normal((p, 40)).astype(np.float32)

    ext = plugin.registry.build_roi_extractor(dict(type="DynamicPointROIExtractor", extra_wlh=[1.0, 1.0, 1.0], max_inbox_point=512,
                                                   debug=True))
    d_pts, d_rois = torch.from_numpy(pts).to(device), torch.from_numpy(rois).to(device)
    inds, roi_inds, info = ext(d_pts[:, :3], torch.zeros(p, dtype=torch.long, device=device), d_rois)
    wp, wr, wf = orefine.dynamic_point_pool(rois[:, 1:], pts[:, :3], [1.0, 1.0, 1.0], 512)
    np.testing.assert_array_equal(inds.cpu().numpy(), wp)
    np.testing.assert_array_equal(roi_inds.cpu().numpy(), wr)
    with torch.no_grad():
        out, mask = head(d_pts[inds], torch.from_numpy(feats).to(device)[inds], info, roi_inds, d_rois)
        # the groups indexed by RoI directly (default) and through a unique + scatter: the same rows, bit for bit
        from fullysparsefusion_amd import switches
        assert switches.REFINE_DIRECT and getattr(roi_inds, "_fsf_real_rows", False)
        switches.REFINE_DIRECT = False
        try:
            out_u, mask_u = head(d_pts[inds], torch.from_numpy(feats).to(device)[inds], info, roi_inds, d_rois)
        finally:
            switches.REFINE_DIRECT = True
        assert torch.equal(out, out_u) and torch.equal(mask, mask_u)
    c = lambda x: x.cpu()  # noqa: E731
    want, wmask = omod.refine_head_forward(cpu, c(d_pts[inds]), torch.from_numpy(feats)[c(inds)],
                                           {k: c(v) for k, v in info.items()}, c(roi_inds), torch.from_numpy(rois))
    assert out.shape == (r, 128 * 2 * 3)
    np.testing.assert_array_equal(mask.cpu().numpy(), wmask.numpy())
    assert not bool(mask[7]) and not out[7].any()
    close(out, want)


def test_multiclass_nms_path_vs_oracle(plugin, device):
    """box3d_multiclass_nms (per class: threshold, score sort, K20 rotated NMS, concat, top max_num) against the float64
    oracle on clustered boxes."""
    from fullysparsefusion_amd.mmdet3d_plugin.core.bbox import LiDARInstance3DBoxes, box3d_multiclass_nms, xywhr2xyxyr
    from oracle import refine as orefine

    rng = np.random.default_rng(12)
    n, ncls = 260, 3
    ctr = rng.uniform(-30, 30, (40, 2))[rng.integers(0, 40, n)] + rng.normal(0, 0.6, (n, 2))
    boxes = np.concatenate([ctr, rng.uniform(-2, 0, (n, 1)), rng.uniform(1.6, 2.2, (n, 1)), rng.uniform(3.8, 5.0, (n, 1)),
                            rng.uniform(1.4, 2.0, (n, 1)), rng.uniform(-3.1, 3.1, (n, 1)), rng.normal(0, 1, (n, 2))], 1).astype(np.float32)
    scores = rng.random((n, ncls)).astype(np.float32)
    cfg = dict(use_rotate_nms=True, nms_thr=0.3, score_thr=0.2, max_num=120)
    tb, ts = torch.from_numpy(boxes).to(device), torch.from_numpy(scores).to(device)
    for_nms = xywhr2xyxyr(LiDARInstance3DBoxes(tb, box_dim=9).bev)
    ob, osc, ol = box3d_multiclass_nms(tb, for_nms, torch.cat([ts, ts.new_zeros(n, 1)], 1), cfg["score_thr"], cfg["max_num"], cfg)
    rows, wsc, wl = omod.multiclass_nms(torch.from_numpy(boxes), torch.from_numpy(scores), cfg["score_thr"], cfg["nms_thr"],
                                        cfg["max_num"])
    # the comparison is only meaningful if no pair sits within rounding of the IoU threshold
    bev = boxes[:, [0, 1, 3, 4, 6]].astype(np.float64)
    xyxyr = np.stack([bev[:, 0] - bev[:, 2] / 2, bev[:, 1] - bev[:, 3] / 2, bev[:, 0] + bev[:, 2] / 2, bev[:, 1] + bev[:, 3] / 2,
                      bev[:, 4]], 1)
    iou = orefine.iou_bev_matrix(xyxyr)
    assert not (np.abs(iou - cfg["nms_thr"]) < 1e-5).any()
    assert ob.shape[0] == cfg["max_num"] == rows.numel()
    np.testing.assert_array_equal(ob.cpu().numpy(), boxes[rows.numpy()])
    np.testing.assert_array_equal(osc.cpu().numpy(), wsc.numpy())
    np.testing.assert_array_equal(ol.cpu().numpy(), wl.numpy())


def test_simple_test_end_to_end_boxes(fsf_pair, frame1, device):
    """FSF.simple_test = stages 1-3 + heads + query combination + refine stage + decode + NMS: shape / range / determinism
    contract of the result (values are checked module by module above)."""
    model, _ = fsf_pair
    pts = [torch.from_numpy(frame1["points"]).to(device)]
    metas = [dict(lidar2img=torch.from_numpy(frame1["lidar2img"]).to(device))]
    mask = torch.from_numpy(frame1["mask_data"]).to(device)[None]
    anno = torch.from_numpy(frame1["mask_anno"]).to(device)[None]
    with torch.no_grad():
        res = model.simple_test(pts, metas, mask, anno)
        again = model.simple_test(pts, metas, mask, anno)
    assert isinstance(res, list) and len(res) == 1
    r = res[0]
    boxes, scores, labels = r["boxes_3d"].tensor, r["scores_3d"], r["labels_3d"]
    assert boxes.device.type == "cpu" and boxes.shape[1] == 9 and 0 < boxes.shape[0] <= 500
    assert scores.shape == (boxes.shape[0],) and labels.shape == (boxes.shape[0],)
    assert torch.isfinite(boxes).all() and (scores > 0.01).all() and (scores <= 1).all()
    assert (labels >= 0).all() and (labels < 10).all() and (boxes[:, 3:6] > 0).all()
    assert torch.equal(again[0]["boxes_3d"].tensor, boxes) and torch.equal(again[0]["scores_3d"], scores)
    hot = model.simple_test(pts, metas, mask, anno, hot_path_only=True)
    assert "frustum_obj_feats" in hot and "fsd_obj_feats" in hot


def test_concurrent_query_branches_equal_sequential(fsf_pair, frame1, device):
    """The camera-query and LiDAR-query branches run on two streams / two host threads at inference
    (FSF._query_branches); the boxes must be bit-identical to the back-to-back order upstream uses, call after call."""
    model, _ = fsf_pair
    pts = [torch.from_numpy(frame1["points"]).to(device)]
    metas = [dict(lidar2img=torch.from_numpy(frame1["lidar2img"]).to(device))]
    mask = torch.from_numpy(frame1["mask_data"]).to(device)[None]
    anno = torch.from_numpy(frame1["mask_anno"]).to(device)[None]
    cfg = model.test_cfg
    try:
        with torch.no_grad():
            cfg["concurrent_query_branches"] = False
            seq = model.simple_test(pts, metas, mask, anno)[0]
            seq_hot = model.simple_test(pts, metas, mask, anno, hot_path_only=True)
            cfg["concurrent_query_branches"] = True
            for _ in range(3):
                con = model.simple_test(pts, metas, mask, anno)[0]
                assert torch.equal(con["boxes_3d"].tensor, seq["boxes_3d"].tensor)
                assert torch.equal(con["scores_3d"], seq["scores_3d"]) and torch.equal(con["labels_3d"], seq["labels_3d"])
            con_hot = model.simple_test(pts, metas, mask, anno, hot_path_only=True)
            for k in ("frustum_obj_feats", "frustum_obj_centers", "fsd_obj_feats", "fsd_obj_centers", "fsd_obj_coors"):
                assert torch.equal(con_hot[k], seq_hot[k]), k
    finally:
        cfg.pop("concurrent_query_branches", None)


def test_av2_full_detector_end_to_end(plugin, device):
    """BASELINE config 5 through the whole detector: +-200 m cloud of 4-d points, 7 cameras, ONE int32 id plane per camera
    (ids > 255), 26 classes, the `is_argo` image branch (box + score + one-hot, FSF.py:540-548), 8-d box code."""
    from fullysparsefusion_amd import synthetic
    from fullysparsefusion_amd.compat import Config

    torch.manual_seed(11)
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "fsf_av2.py"))
    model = plugin.build_model(cfg.model).eval()
    torch.nn.init.normal_(model.segmentor_updated_mlp[-1].weight, std=0.05)
    model.to(device)
    rng = np.random.default_rng(13)
    n = 60000
    r = rng.uniform(2.0, 200.0, n)
    a = rng.uniform(-np.pi, np.pi, n)
    xyz = np.stack([r * np.cos(a), r * np.sin(a), rng.normal(-1.5, 0.5, n).clip(-3.1, 3.1)], 1)
    xyz = xyz[(np.abs(xyz[:, 0]) < 204.7) & (np.abs(xyz[:, 1]) < 204.7)]
    pts = np.concatenate([xyz, rng.random((xyz.shape[0], 1)), xyz], 1).astype(np.float32)  # x y z i | no-aug xyz
    L = synthetic.make_lidar2img(7, fx=1780.0, cx=1024.0, cy=775.0)
    mask, anno = synthetic.make_mask_data(rng, 7, 1, 1550, 2048, 400, dtype=np.int32)
    anno[:, 5] = rng.integers(0, 26, anno.shape[0])  # category: one of the 26 classes
    pts_t = [torch.from_numpy(pts).to(device)]
    metas = [dict(lidar2img=torch.from_numpy(L).to(device))]
    with torch.no_grad():
        hot = model.forward_hot_path(pts_t, metas, torch.from_numpy(mask).to(device)[None], torch.from_numpy(anno).to(device)[None])
        res = model.simple_test(pts_t, metas, torch.from_numpy(mask).to(device)[None], torch.from_numpy(anno).to(device)[None])
    seg = hot["seg"]
    assert seg["seg_logits"].shape == (pts.shape[0], 27) and seg["seg_vote_preds"].shape == (pts.shape[0], 27 * 3)
    assert hot["frustum_obj_feats"].shape[1] == 128 * 3 * 2 + 128 and hot["fsd_obj_feats"].shape[1] == 128 * 3 * 2
    assert hot["frustum_obj_feats"].shape[0] > 0 and int(hot["frustum_obj_coors"][:, 2].max()) > 255  # ids beyond u8 survive
    boxes, scores, labels = res[0]["boxes_3d"].tensor, res[0]["scores_3d"], res[0]["labels_3d"]
    assert boxes.shape[1] == 7 and 0 < boxes.shape[0] <= 500 and torch.isfinite(boxes).all()
    assert (labels >= 0).all() and (labels < 26).all() and float(boxes[:, :2].abs().max()) > 60.0  # long-range boxes exist


def test_simple_test_edge_cases(fsf_pair, frame1, device):
    """Batch of two frames, a frame without any mask (no camera queries -> the fake frustum object of FSF.py:407-414) and a
    tiny cloud all go through the complete simple_test."""
    model, _ = fsf_pair
    L = torch.from_numpy(frame1["lidar2img"]).to(device)
    mask = torch.from_numpy(frame1["mask_data"]).to(device)
    anno = torch.from_numpy(frame1["mask_anno"]).to(device)
    pts = torch.from_numpy(frame1["points"]).to(device)
    with torch.no_grad():
        two = model.simple_test([pts, pts[:20000].contiguous()], [dict(lidar2img=L), dict(lidar2img=L)],
                                torch.stack([mask, mask]), torch.stack([anno, anno]))
        assert len(two) == 2 and all(r["boxes_3d"].tensor.shape[1] == 9 for r in two)
        assert len(two[0]["boxes_3d"]) > 0
        none = model.simple_test([pts], [dict(lidar2img=L)], torch.zeros_like(mask)[None], anno[None])
        assert len(none) == 1 and torch.isfinite(none[0]["boxes_3d"].tensor).all()
        tiny = model.simple_test([pts[:300].contiguous()], [dict(lidar2img=L)], mask[None], anno[None])
        assert len(tiny) == 1 and torch.isfinite(tiny[0]["boxes_3d"].tensor).all()


def test_device_point_assembly_equals_the_host_pipeline(device, tmp_path):
    """K0 (`fsf_assemble_sweeps` behind `DevicePointAssembler`): raw .bin sweeps -> ONE host->device copy -> sweep transform,
    time lag, close-point removal, concatenation, no-aug xyz columns, range filter, intensity normalisation ON THE DEVICE —
    bit-identical to the host classes, which tests/test_input_pipeline.py pins bit-exactly to the reference's own loaders
    (tests/golden/input_pipeline.npz); the golden's `normed` rows are compared directly as well."""
    import json

    from fullysparsefusion_amd.mmdet3d_plugin import datasets as D

    g = load_golden("input_pipeline.npz")
    g["key"].tofile(tmp_path / "key.bin")
    meta = json.loads(bytes(g["sweep_meta_json"]).decode())
    for k, m in enumerate(meta):
        g["sweeps"][k].tofile(tmp_path / f"sweep{k}.bin")
        m["data_path"] = str(tmp_path / f"sweep{k}.bin")
    rng_box = [-51.2, -51.2, -5, 51.2, 51.2, 3]

    def host(sweeps, sweeps_num, pc_range):
        r = D.LoadPointsFromFile(coord_type="LIDAR", load_dim=5, use_dim=[0, 1, 2, 3, 4])(dict(pts_filename=str(tmp_path / "key.bin")))
        r.update(timestamp=1.5e9, sweeps=sweeps)
        r = D.LoadPointsFromMultiSweeps(sweeps_num=sweeps_num, use_dim=[0, 1, 2, 3, 4], pad_empty_sweeps=True, remove_close=True,
                                        test_mode=True)(r)
        r = D.SaveNoAugPoints()(r)
        if pc_range is not None:
            r = D.PointsRangeFilter(pc_range)(r)
        return D.NormalizePoints()(r)["points"].tensor.numpy()

    for sweeps, sweeps_num, pc_range in [(meta, 9, None), (meta, 9, rng_box), (meta, 2, rng_box), ([], 2, None), ([], 3, [-20, -20, -5, 20, 20, 3])]:
        asm = D.DevicePointAssembler(load_dim=5, sweeps_num=sweeps_num, pad_empty_sweeps=True, remove_close=True, test_mode=True,
                                     point_cloud_range=pc_range)
        got = asm(dict(pts_filename=str(tmp_path / "key.bin"), timestamp=1.5e9, sweeps=sweeps), device)
        want = host(sweeps, sweeps_num, pc_range)
        assert got.is_cuda and got.shape[1] == 8
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    got = D.DevicePointAssembler(sweeps_num=9, test_mode=True)(dict(pts_filename=str(tmp_path / "key.bin"), timestamp=1.5e9, sweeps=meta), device)
    np.testing.assert_array_equal(got.cpu().numpy(), g["normed"])  # the reference's own output, bit for bit


def test_files_to_boxes_through_the_input_pipeline(fsf_pair, frame1, device, tmp_path):
    """On-disk formats -> test pipeline -> one host->device copy -> FSF.simple_test: the same boxes as feeding the
    tensors directly (the pipeline's range filter / intensity scaling applied to both)."""
    import json

    from PIL import Image

    from fullysparsefusion_amd.mmdet3d_plugin import datasets as D

    model, _ = fsf_pair
    classes = model.class_names
    pts5 = frame1["points"][:, :5].copy()
    pts5[:, 3] *= 255.0                       # stored intensity is 0..255; NormalizePoints divides it back
    pts5.tofile(tmp_path / "key.bin")
    sdir = tmp_path / "masks" / "s0"
    sdir.mkdir(parents=True)
    for cam in range(6):
        for ci, name in enumerate(classes):
            Image.fromarray(frame1["mask_data"][cam, ci]).save(sdir / f"{cam}_{name}.png")
    anno = [dict() for _ in range(6)]
    for row in frame1["mask_anno"]:
        cam, cls = int(row[6]), int(row[5])
        anno[cam].setdefault(classes[cls], []).append(dict(bbox=[float(v) for v in row[:4]], score=float(row[4]), category=cls,
                                                           cam_id=cam, obj_id=int(row[7])))
    (sdir / "anno.json").write_text(json.dumps(anno))
    pipeline = D.Compose([
        dict(type="LoadPointsFromFile", coord_type="LIDAR", load_dim=5, use_dim=[0, 1, 2, 3, 4]),
        dict(type="LoadPointsFromMultiSweeps", sweeps_num=9, use_dim=[0, 1, 2, 3, 4], pad_empty_sweeps=False, remove_close=True),
        dict(type="SaveNoAugPoints"),
        dict(type="LoadMaskFromFiles", data_path=str(tmp_path / "masks"), class_names=classes),
        dict(type="MultiScaleFlipAug3D", img_scale=(1333, 800), pts_scale_ratio=1, flip=False, transforms=[
            dict(type="PointsRangeFilter", point_cloud_range=[-51.2, -51.2, -5, 51.2, 51.2, 3]),
            dict(type="NormalizePoints"),
            dict(type="DefaultFormatBundle3D", class_names=classes, with_label=False),
            dict(type="Collect3D", keys=["points", "mask_data", "mask_anno"])])])
    data = pipeline(dict(pts_filename=str(tmp_path / "key.bin"), timestamp=0.0, sweeps=[], sample_idx="s0",
                         lidar2img=list(frame1["lidar2img"])))
    points, metas, mask, anno_t = D.frame_to_device(data, device)
    assert mask.dtype == torch.uint8 and mask.is_cuda and points[0].shape[1] == 8
    np.testing.assert_array_equal(mask[0].cpu().numpy(), frame1["mask_data"])
    np.testing.assert_allclose(anno_t[0].cpu().numpy(), frame1["mask_anno"], rtol=1e-6)
    with torch.no_grad():
        res = model.simple_test(points, metas, mask, anno_t)
        direct_pts = points[0].clone()
        ref = model.simple_test([direct_pts], [dict(lidar2img=torch.from_numpy(frame1["lidar2img"]).to(device))], mask, anno_t)
    assert torch.equal(res[0]["boxes_3d"].tensor, ref[0]["boxes_3d"].tensor) and len(res[0]["boxes_3d"]) > 0


def test_stage1_gradients_vs_oracle(fsf_pair, device, monkeypatch):
    """Config-3 backward on stage 1 (eval-mode norms, gradients on): VFE, sparse U-Net (K10), neck gather, image MLP and
    segmentation head.
    (1) Every sparse-conv backward call of the real graph is checked IN SITU against a float64 torch restatement on the
        very tensors it received (data gradient through the transposed rulebook, weight gradient over the pairs): 1e-5.
    (2) End to end against autograd through the CPU oracle.  One ReLU input within rounding of zero flips between GPU
        and CPU and perturbs every gradient downstream of it by ~1e-3 (seen on this cloud: 1 element of 164 608 after
        upsample_layer3) — so: relative L2 error <= 2e-2 for every parameter (a wiring error is O(1)), and the parameters
        no flip reaches must be as close to a float64 run as the oracle's own fp32 run is (x10, floor 1e-4)."""
    from fullysparsefusion_amd import synthetic
    from fullysparsefusion_amd.mmdet3d_plugin.ops import spconv as sp

    model, cpu = fsf_pair
    f = synthetic.make_frame(num_sweeps=1, seed=3)
    pts8 = torch.from_numpy(f["points"][:12000].copy())
    mask, anno, L = torch.from_numpy(f["mask_data"]), torch.from_numpy(f["mask_anno"]), torch.from_numpy(f["lidar2img"])
    probe_l = torch.from_numpy(np.random.default_rng(1).standard_normal((pts8.shape[0], 11)).astype(np.float32))
    probe_v = torch.from_numpy(np.random.default_rng(2).standard_normal((pts8.shape[0], 33)).astype(np.float32))

    checked = []
    orig_bwd = sp._SparseConvFn.backward

    def checking_backward(ctx, grad):
        res = orig_bwd(ctx, grad)
        g_feat, g_w = res[:2]
        feat, weight = ctx.saved_tensors
        rb, inverse = ctx.rb, ctx.inverse
        kvol = rb.nbr.size(1)
        w = weight.detach().reshape(kvol, weight.shape[-2], weight.shape[-1]).double()
        table = rb.table(inverse).long()           # out row o, offset k -> in row
        want_feat = torch.zeros(feat.shape, dtype=torch.float64, device=feat.device)
        want_w = torch.zeros_like(w)
        g64, f64 = grad.double(), feat.detach().double()
        for k in range(kvol):
            o = (table[:, k] >= 0).nonzero().squeeze(1)
            i = table[o, k]
            want_feat.index_add_(0, i, g64[o] @ w[k].t())
            want_w[k] = f64[i].t() @ g64[o]
        for got, want in ((g_feat, want_feat), (g_w.reshape(w.shape), want_w)):
            if got is not None:
                err = float((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-30))
                assert err < 1e-5, (rb.kind, inverse, tuple(feat.shape), tuple(grad.shape), err)
        checked.append((rb.kind, inverse))
        return res

    monkeypatch.setattr(sp._SparseConvFn, "backward", staticmethod(checking_backward))

    def names(m):
        return [n for n, _ in m.named_parameters() if n.startswith(("segmentor.", "segmentor_updated_mlp."))]

    def run_oracle(module, dtype):
        module.zero_grad(set_to_none=True)
        s1 = omod.fsf_stage1(module, pts8, mask, anno, L, grad=True, dtype=dtype)
        ((s1["seg_logits"] * probe_l.to(dtype)).sum() + (s1["seg_vote_preds"] * probe_v.to(dtype)).sum()).backward()
        params = dict(module.named_parameters())
        return {n: params[n].grad.detach().clone() for n in names(module) if params[n].grad is not None}

    g32 = run_oracle(copy.deepcopy(cpu), torch.float32)
    g64 = run_oracle(copy.deepcopy(cpu).double(), torch.float64)

    model.zero_grad(set_to_none=True)
    model._gather_cache = None
    points, infos = model.split_points_last_3dim([pts8.to(device)])
    metas = [dict(lidar2img=L.to(device))]
    seg_tuple = model.segmentor.simple_test(points, metas, extract_feat_only=True, rescale=False)
    seg = model.segmentor_feat_inhance_test(seg_tuple, infos, anno.to(device)[None], mask.to(device)[None], metas)
    ((seg["seg_logits"] * probe_l.to(device)).sum() + (seg["seg_vote_preds"] * probe_v.to(device)).sum()).backward()
    params = dict(model.named_parameters())
    assert len(checked) == 34 and {("subm", False), ("strided", False), ("strided", True)} <= set(checked)

    def rel_max(a, b):
        return float((a.double().cpu() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))

    def rel_l2(a, b):
        return float((a.double().cpu() - b.double()).norm() / b.double().norm().clamp_min(1e-30))

    assert len(g64) > 60
    tight, loose_bad = 0, {}
    for n, g in g64.items():
        assert params[n].grad is not None, n
        if rel_max(params[n].grad, g) <= max(1e-4, 10.0 * rel_max(g32[n], g)):
            tight += 1
        if rel_l2(params[n].grad, g) > 2e-2:
            loose_bad[n] = rel_l2(params[n].grad, g)
    model.zero_grad(set_to_none=True)
    assert not loose_bad, loose_bad
    assert tight >= 0.4 * len(g64), (tight, len(g64))  # VFE, image MLP, seg head, neck and the two finest U-Net levels


def test_sir_layer_deferred_concat_equals_materialised(plugin, device, monkeypatch):
    """SIRLayer at inference with the concat deferred to fsf_linear_norm_act_grouped == the same layer with the
    [n, 2C] concat materialised (both through K22): point feats, group feats, group order."""
    from fullysparsefusion_amd.mmdet3d_plugin.ops import sst_ops

    torch.manual_seed(5)
    layer = plugin.registry.build_voxel_encoder(dict(
        type="SIRLayer", in_channels=133, feat_channels=[128, 128], with_distance=False, with_cluster_center=False,
        with_rel_mlp=True, rel_mlp_hidden_dims=[16, 32], rel_mlp_in_channel=3, with_voxel_center=False,
        norm_cfg=dict(type="LN", eps=1e-3), mode="max", return_point_feats=True, rel_dist_scaler=10.0,
        xyz_normalizer=[20.0, 20.0, 4.0], act="gelu", dropout=0.0)).to(device).eval()
    n, g = 60000, 900
    feats = torch.randn(n, 133, device=device)
    f_cluster = torch.randn(n, 3, device=device)
    gid = torch.randint(0, g, (n,), device=device)
    coors = torch.stack([torch.zeros_like(gid), gid % 7, gid], 1)
    outs = []
    real = sst_ops._grouped_linear_norm_act
    with torch.no_grad():
        for deferred in (True, False):
            monkeypatch.setattr(sst_ops, "_grouped_linear_norm_act", real if deferred else (lambda *a, **k: None))
            outs.append(layer(feats, coors, f_cluster=f_cluster, return_both=True))
    for a, b in zip(outs[0], outs[1]):
        if a.dtype.is_floating_point:
            assert float((a - b).abs().max()) <= 2e-5 * max(1.0, float(b.abs().max()))
        else:
            assert torch.equal(a, b)


@pytest.mark.gpu
def test_training_step_two_frames_per_gpu_in_a_process_group(device):
    """BASELINE config 4 on the device, as far as one GPU allows: two frames per GPU through the data-parallel step bench.py times
    (training-mode norms, flat gradient buckets whose views are the `.grad` tensors, AdamW) inside an initialised RCCL process
    group of one rank — the wrapper then issues no collective, so the step must equal the plain autograd step: gradients == an
    undistributed backward of the same loss, AdamW moves the parameters, a second step runs on the re-armed buckets.  (Two ranks
    need two GPUs; the collectives themselves are covered by the world-size-2 gloo tests.)"""
    import socket

    import torch.distributed as dist

    import bench

    if dist.is_initialized():
        pytest.skip("a process group is already initialised in this process")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        torch.manual_seed(0)
        model = bench.build_model(device)
        _, inp = bench.make_inputs(1, 3, device, frames=2)
        # reference: the same model, training mode, plain autograd
        model.train()
        out = model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"])
        loss = bench.dummy_loss(out)
        params = [p for p in model.parameters() if p.requires_grad]
        want = torch.autograd.grad(loss, params, allow_unused=True)
        before = [p.detach().clone() for p in params]
        # bench.py's step (FrameDataParallel buckets + AdamW); BatchNorm running statistics moved once already, which does not
        # enter training-mode outputs
        stepper = bench.TrainStep(model)
        stepper(inp)
        torch.cuda.synchronize()
        assert stepper.dp.world == 1
        n_checked = 0
        for p, g in zip(params, want):
            if g is None:
                assert p.grad is None or not p.grad.any()
                continue
            scale = max(float(g.abs().max()), 1e-12)
            assert float((p.grad - g).abs().max()) <= 1e-5 * scale + 1e-12, "gradient differs from the undistributed backward"
            n_checked += 1
        assert n_checked > 100
        moved = sum(int((p.detach() != b).any()) for p, b in zip(params, before))
        assert moved > 100
        loss2 = float(bench.dummy_loss(stepper(inp)).detach())
        assert loss2 == loss2  # finite: the second step ran on re-armed buckets
    finally:
        dist.destroy_process_group()
