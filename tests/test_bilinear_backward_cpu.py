"""The bilinear image-feature gather's backward (K13c, docs/kernels/K13c_bilinear_backward.md) on the host: the specification the
kernels are held to (tests/bilinear_cases.py) against float64 autograd through F.grid_sample, the case rows of the GPU tests against
the counts they were chosen for, the C ABI surface, the static guard-band check of the new wrapper module and the public op's refusals."""
import ast
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bilinear_cases as bc
from oracle import project as oproj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ host specification
@pytest.mark.parametrize("sel,hf,wf", [((3000, 96, 300), 29, 50), ((3000, 96, 300), 57, 100), ((4000, 96, 200), 3, 4), ((4000, 96, 200), 1, 1)])
def test_host_specification_against_float64_grid_sample_autograd(sel, hf, wf):
    """Reference: float64 F.grid_sample autograd through the map, on the fp32 oracle grid cast to float64; per element within
    1e-4 * max(1, max |ref|), the forward test's own convention.  The only difference is the fp32 rounding of ix, iy."""
    pts, L = bc.selection(*sel)
    c = 3
    rng = np.random.default_rng(hf * 1000 + wf)
    u = rng.standard_normal((pts.shape[0], 6, c)).astype(np.float32)
    grid = oproj.prj_points_2d(pts, L, *bc.IMG_HW)  # [ncam, n, 2]
    feat = torch.zeros(6, c, hf, wf, dtype=torch.float64, requires_grad=True)
    out = F.grid_sample(feat, torch.from_numpy(grid).double()[:, None], mode="bilinear", align_corners=False, padding_mode="zeros")
    (out[:, :, 0].permute(2, 0, 1) * torch.from_numpy(u).double()).sum().backward()  # out [ncam, C, 1, n] -> [n, ncam, C]
    ref = feat.grad.permute(0, 2, 3, 1).numpy()
    for reduce in (False, True):
        uu = u[:, 0] if reduce else u
        want = ref
        if reduce:
            feat2 = torch.zeros(6, c, hf, wf, dtype=torch.float64, requires_grad=True)
            out2 = F.grid_sample(feat2, torch.from_numpy(grid).double()[:, None], mode="bilinear", align_corners=False, padding_mode="zeros")
            (out2[:, :, 0].permute(2, 0, 1).sum(1) * torch.from_numpy(uu).double()).sum().backward()
            want = feat2.grad.permute(0, 2, 3, 1).numpy()
        got = bc.bilinear_backward_host(pts, L, uu, bc.IMG_HW, hf, wf, reduce_cams=reduce)["ref"]
        err, top = float(np.abs(got - want).max()), float(np.abs(want).max())
        print(f"{hf} x {wf} reduce={reduce}: largest error {err:.3g}, max |ref| {top:.3g}")
        assert top > 1.0 and err <= 1e-4 * max(1.0, top)


def test_selection_classes_of_the_frame():
    assert bc.class_sizes() == (21213, 612, 9210)


# the issue's table: (rows, valid pairs, non-zero taps, outside corners, largest texel run, empty texels)
TABLE = {"coarse_3x4": (4296, 4192, 7833, 8935, 440, 32), "single_1x1": (4296, 4192, 4192, 12576, 767, 0),
         "sparse_29x50": (3396, 3192, 11864, 904, 16, 7445)}


@pytest.mark.parametrize("name", sorted(bc.ROWS))
def test_case_rows_keep_what_they_were_chosen_for(name):
    """A regenerated frame must not hollow the cases out: the counts are asserted as inequalities (half the table's figure at least)."""
    sel, (hf, wf) = bc.ROWS[name]
    pts, L = bc.selection(*sel)
    s = bc.case_stats(pts, L, hf, wf)
    print(name, s)
    rows, pairs, taps, outside, run, empty = TABLE[name]
    assert s["rows"] == rows == sum(sel)
    assert s["two_camera_points"] >= sel[1] and s["unseen_points"] >= sel[2]  # points seen by two cameras, and by none, are present
    assert s["valid_pairs"] >= sel[0] + 2 * sel[1] and s["nonzero_taps"] >= taps // 2
    assert s["outside_corners"] >= outside // 2 and s["largest_run"] >= run // 2 and s["empty_texels"] >= empty // 2
    if name == "coarse_3x4":
        assert s["texels_256"] >= 7 and s["largest_run"] >= 256 and 0 < s["empty_texels"] < s["texels"]
    if name == "single_1x1":
        assert s["min_run"] >= 256 and s["nonzero_taps"] == s["valid_pairs"]  # every camera's single texel takes every pair's one tap
    if name == "sparse_29x50":
        assert s["largest_run"] <= 64 and s["empty_texels"] > s["texels"] // 2


def test_long_run_selection_reaches_a_middle_chunk_and_a_tail():
    from fullysparsefusion_amd import _lib

    chunk = _lib.DEFINES["FSF_BILINEAR_BWD_CHUNK"]
    pts, L = bc.selection(*bc.LONG_RUN)
    assert bc.LONG_RUN[0] <= bc.class_sizes()[0]
    assert bc.case_stats(pts, L, 1, 1)["largest_run"] >= 2 * chunk + 1
    assert bc.largest_cell_run(pts, L, 1, 1) >= 2 * chunk + 1  # (one corner's run, the piece the device cuts into chunks)


def test_taps_sum_to_one_inside_the_map():
    pts, L = bc.selection(3000, 96, 300)
    _, w, inside, valid = bc.bilinear_taps_host(pts, L, bc.IMG_HW, 29, 50)
    full = valid & inside.all(-1)
    assert full.sum() > 2000 and float(np.abs(w[full].sum(-1) - 1.0).max()) <= 4 * 2.0 ** -24 * 4
    assert not w[~valid].any() and not w[~inside].any() and (w >= 0).all()


# ------------------------------------------------------------------------------------------------ C ABI surface and guard-band cover
def test_entry_points_are_declared_documented_and_the_abi_version_stays():
    from fullysparsefusion_amd import _lib

    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for name in ("fsf_project_gather_bilinear_backward", "fsf_project_gather_bilinear_backward_workspace_bytes"):
        assert name in _lib.SIGNATURES and name in doc, name
    assert _lib.DEFINES["FSF_ABI_VERSION"] == 23
    assert _lib.DEFINES["FSF_BILINEAR_BWD_CHUNK"] >= 16
    P, I32, I64 = _lib.c_p, _lib.c_i32, _lib.c_i64
    assert _lib.SIGNATURES["fsf_project_gather_bilinear_backward_workspace_bytes"] == ([I64, I32, I32, I32, I32], I64)
    assert _lib.SIGNATURES["fsf_project_gather_bilinear_backward"] == ([P, I64, I32, P, I32, P, I32, I32, I32, I32, I32, I32, I32, P, P, I64, P], I32)


def test_size_function_and_refusals_without_a_device():
    """The size function and the argument checks run on the host: FSF_ERR_UNSUPPORTED past u32 entries or 2^31 cells (0 bytes), and a
    short workspace is refused before anything is launched."""
    from fullysparsefusion_amd import _lib, build

    build.build()
    h = _lib.lib()
    size = h.fsf_project_gather_bilinear_backward_workspace_bytes
    assert size(1000, 6, 29, 50, 64) > 0 and size(0, 6, 29, 50, 64) > 0 and size(1000, 6, 29, 50, 64) == size(1000, 6, 29, 50, 1)
    assert size(-1, 6, 29, 50, 64) == 0 and size(10, 0, 29, 50, 64) == 0 and size(10, 65, 29, 50, 64) == 0 and size(10, 6, 0, 50, 64) == 0
    assert size((1 << 32) // 6 + 1, 6, 29, 50, 64) == 0 and size(10, 64, 8191, 4095, 1) == 0
    unsupported, workspace, invalid = (_lib.DEFINES[k] for k in ("FSF_ERR_UNSUPPORTED", "FSF_ERR_WORKSPACE", "FSF_ERR_INVALID_ARG"))
    fake = _lib.c_p(4096)  # (never dereferenced: every call below is refused on the host)

    def call(n, ncam, hf, wf, c, ws_bytes, xyz=fake, grad_feat=fake, stride=3):
        return h.fsf_project_gather_bilinear_backward(xyz, n, stride, fake, ncam, fake, c, hf, wf, 0, 900, 1600, 0, grad_feat, fake, ws_bytes, None)

    assert call((1 << 32) // 6 + 1, 6, 29, 50, 64, 1 << 40) == unsupported
    assert call(10, 64, 8191, 4095, 1, 1 << 40) == unsupported
    assert call(10, 6, 29, 50, 64, size(10, 6, 29, 50, 64) - 1) == workspace
    assert call(10, 6, 29, 50, 64, 1 << 40, stride=2) == invalid and call(10, 6, 29, 50, 64, 1 << 40, xyz=_lib.c_p(None)) == invalid
    assert call(0, 6, 29, 50, 64, 1 << 40, grad_feat=_lib.c_p(None)) == invalid and call(-1, 6, 29, 50, 64, 1 << 40) == invalid


_ALLOCATES = re.compile(r"torch\.empty|empty_like|torch\.zeros|torch\.full|_lib\.workspace\(|_workspace_bytes|_arena_bytes")
_SCRATCH = re.compile(r"_lib\.workspace\(|_workspace_bytes|_arena_bytes")


def test_every_allocating_wrapper_of_the_new_module_has_guard_band_cases():
    import test_guard_bands_project_gpu as gb
    from fullysparsefusion_amd import hip_ops_project

    with open(os.path.join(ROOT, "fullysparsefusion_amd", "hip_ops_project.py")) as f:
        src = f.read()
    alloc, scratch = set(), set()
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef):
            body = ast.get_source_segment(src, node)
            if _ALLOCATES.search(body):
                alloc.add(node.name)
                if _SCRATCH.search(body):
                    scratch.add(node.name)
    assert alloc == {"project_gather_bilinear_backward"} and scratch == {"project_gather_bilinear_backward"}
    assert sorted(alloc - set(gb.CASES)) == []
    for name, cases in gb.CASES.items():
        assert hasattr(hip_ops_project, name)
        kinds = [k for k, _ in cases]
        assert "ragged" in kinds and "minimal" in kinds and "empty" in kinds, name
    assert not re.search(r"torch\.zeros|torch\.full|empty_like|torch\.ones|new_zeros|new_empty|new_full", src)


# ------------------------------------------------------------------------------------------------ the public op
def test_point_image_gather_refuses_a_gradient_for_the_points_and_the_matrices_by_name():
    from fullysparsefusion_amd.mmdet3d_plugin import ops
    from fullysparsefusion_amd.mmdet3d_plugin.ops import PointImageFeatureGather, point_image_gather

    assert ops.point_image_gather is point_image_gather and "point_image_gather" in ops.__all__ and "PointImageFeatureGather" in ops.__all__
    xyz, L, feat = torch.zeros(4, 3), torch.eye(4).repeat(2, 1, 1), torch.zeros(2, 3, 5, 7)
    with pytest.raises(NotImplementedError, match="xyz"):
        point_image_gather(xyz.clone().requires_grad_(True), L, feat, (900, 1600))
    with pytest.raises(NotImplementedError, match="lidar2img"):
        point_image_gather(xyz, L.clone().requires_grad_(True), feat, (900, 1600))
    mod = PointImageFeatureGather((900, 1600))
    assert mod.reduce_cams is True and mod.img_hw == (900, 1600) and list(mod.parameters()) == [] and mod.state_dict() == {}


def test_product_still_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "fullysparsefusion_amd")
    seen = 0
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                seen += 1
                with open(os.path.join(dirpath, f)) as fh:
                    assert not re.search(r"^\s*(from|import)\s+oracle\b", fh.read(), flags=re.M), os.path.join(dirpath, f)
    assert seen > 20
    for rel in ("hip_ops_project.py", os.path.join("mmdet3d_plugin", "ops", "image_gather.py")):
        assert os.path.exists(os.path.join(pkg, rel))
