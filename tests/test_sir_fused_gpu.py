"""The fused K21 + first K22s layer (fsf_sir_input_linear_segmax, csrc/sir_linear.hip) inside K31 (fsf_sir_stack_forward): with
FSF_OPT_SIR_FUSED on (2: in every stack, whatever its row count) the stack must return the very bits it returns with the option off
(0: K21 and the layer as two launches) — group table, and point rows where they are wanted —, on the same inputs, for the three stacks
of a frame (LiDAR queries 180 / 133 / 133 input columns through an index, camera queries 133 / 133 / 133, the refine head 181 / 146 / 146
with `extra` columns and a direct part), for row counts around the kernel's 16-row groups and 128-row blocks, and for the segment
layouts the segmented max can go wrong on.  The hand-over buffer of the two-kernel path (the front of the arena) is poisoned with NaN:
the fused path neither reads nor writes it, which also shows WHICH path ran."""
import pytest
import torch

from fullysparsefusion_amd import _lib, hip_ops, switches
from fullysparsefusion_amd.mmdet3d_plugin import models  # noqa: F401  (registers the modules)
from fullysparsefusion_amd.mmdet3d_plugin.ops import sst_ops
from fullysparsefusion_amd.mmdet3d_plugin.registry import build_backbone, build_head

pytestmark = pytest.mark.gpu
LN3 = dict(type="LN", eps=1e-3)
BLOCK_ROWS = _lib.DEFINES["FSF_SIR_FUSED_BLOCK_ROWS"]  # rows a workgroup of the fused kernel takes per iteration
WIDTH = 768  # 3 blocks x 2 layers x 128 group columns


def _sir(first_in, device):
    torch.manual_seed(first_in)
    sir = build_backbone(dict(type="SIR", num_blocks=3, in_channels=[first_in, 133, 133], feat_channels=[[128, 128]] * 3,
                              rel_mlp_hidden_dims=[[16, 32]] * 3, norm_cfg=LN3, mode="max", xyz_normalizer=[20, 20, 4], act="gelu",
                              unique_once=True)).to(device).eval()
    return sir


@pytest.fixture(scope="module")
def lidar(device):
    return _sir(5 + 11 + 33 + 131, device)


@pytest.fixture(scope="module")
def camera(device):
    return _sir(5 + 128, device)


@pytest.fixture(scope="module")
def refine(device):
    torch.manual_seed(181)
    return build_head(dict(
        type="FullySparseBboxHead", num_classes=10, num_blocks=3, in_channels=[67 + 5 + 13 + 32 + 64, 131 + 13 + 2, 131 + 13 + 2],
        feat_channels=[[128, 128]] * 3, with_distance=False, with_cluster_center=False, with_rel_mlp=True,
        rel_mlp_hidden_dims=[[16, 32]] * 3, rel_mlp_in_channels=[13] * 3, reg_mlp=[512, 512], cls_mlp=[512, 512], mode="max",
        xyz_normalizer=[20, 20, 4], cat_voxel_feats=True, pos_fusion="mul", fusion="cat", act="gelu", geo_input=True,
        use_middle_cluster_feature=True, norm_cfg=LN3, unique_once=True)).to(device).eval()


def _desc(module):
    desc = sst_ops.sir_stack_descriptor(module, module.block_list)
    assert desc is not None and sum(sum(w) for w in desc.widths) == WIDTH
    return desc


def _lidar_inputs(device, n, seed=0):
    """The LiDAR-query stack's first block: 5 point columns + three feature tensors (11 | 33 | 131 columns, two of them column slices of
    one buffer, the third of a padded one) read through an index — the part boundaries fall inside 16-column tiles and 32-column chunks."""
    g = torch.Generator().manual_seed(1000 + n + seed)
    P = 5003
    both = torch.randn(P, 44, generator=g).to(device)
    parts = [both[:, :11], both[:, 11:], torch.randn(P, 132, generator=g).to(device)[:, :131]]
    idx = torch.randint(0, P, (n,), generator=g).to(device)
    points = (torch.randn(n, 5, generator=g) * 10).to(device)
    fcl = torch.randn(n, 3, generator=g).to(device)
    return dict(points=points, feats=parts, f_cluster=fcl, feats_index=idx)


def _camera_inputs(device, n):
    g = torch.Generator().manual_seed(2000 + n)
    return dict(points=(torch.randn(n, 5, generator=g) * 10).to(device), feats=torch.randn(n, 128, generator=g).to(device),
                f_cluster=torch.randn(n, 3, generator=g).to(device))


def _refine_inputs(device, n):
    """The refine head's stack: 5 + (131 gathered + 32 direct) + 13 `extra` columns (divided by 10), a 13-column f_cluster."""
    g = torch.Generator().manual_seed(3000 + n)
    P = 4001
    fcl = torch.randn(n, 13, generator=g).to(device)
    return dict(points=(torch.randn(n, 5, generator=g) * 10).to(device),
                feats=[torch.randn(P, 132, generator=g).to(device)[:, :131], torch.randn(n, 32, generator=g).to(device)],
                f_cluster=fcl, extra=fcl, extra_div=10.0, feats_index=torch.randint(0, P, (n,), generator=g).to(device), direct_parts=(1,))


def _random_segments(device, n, m, seed=0):
    g = torch.Generator().manual_seed(seed + n + m)
    seg = torch.randint(0, m, (n,), generator=g)
    seg[:min(n, m)] = torch.arange(min(n, m))  # (every group has a row where n >= m)
    return torch.sort(seg)[0].to(device).contiguous()


def _x_buffer_floats(desc, n):
    return n * max((int(b.in_cols) + 3) // 4 * 4 for b in desc.blocks)


def _run(desc, inputs, seg, m, want_rows, fused, groups=None, rows_out=None):
    """One fsf_sir_stack_forward with the option set to `fused` (0 | 2) on a NaN-filled arena.  Returns (rows, groups, whether the two-
    kernel hand-over buffer at the front of the arena was written)."""
    n = inputs["points"].size(0)
    nbytes = int(_lib.lib().fsf_sir_stack_arena_bytes(desc.blocks, desc.num_blocks, n, m))
    arena = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=seg.device)
    if groups is None:
        groups = torch.full((m, WIDTH), float("-inf"), device=seg.device)
    old = hip_ops.set_option(hip_ops.OPT_SIR_FUSED, fused)
    mirror, switches.SIR_FUSED = switches.SIR_FUSED, None  # (None: the wrapper leaves the library's setting alone)
    try:
        with torch.no_grad():
            rows = hip_ops.sir_stack_forward(desc, seg_ids=seg, groups=groups, want_rows=want_rows, rows_out=rows_out,
                                             arena=arena.view(torch.uint8), **inputs)
    finally:
        switches.SIR_FUSED = mirror
        hip_ops.set_option(hip_ops.OPT_SIR_FUSED, old)
    xbuf = arena[:_x_buffer_floats(desc, n)]
    return rows, groups, bool((~torch.isnan(xbuf)).any())


def _same(desc, inputs, seg, m, want_rows, expect_fused=True):
    r0, g0, wrote0 = _run(desc, inputs, seg, m, want_rows, 0)
    r1, g1, wrote1 = _run(desc, inputs, seg, m, want_rows, 2)
    assert wrote0, "the two-kernel path hands over through the arena"
    assert wrote1 != expect_fused, "every block of the stack took the fused launch: nothing touched the hand-over buffer"
    assert torch.isfinite(g1[seg.unique()]).all() and torch.equal(g0, g1)
    if want_rows:
        assert torch.isfinite(r1).all() and torch.equal(r0, r1)
    else:
        assert r0 is None and r1 is None
    return g1


def test_the_option_is_a_library_switch_with_a_python_mirror():
    assert hip_ops.OPT_SIR_FUSED == 3 and int(_lib.lib().fsf_get_option(3)) in (0, 1, 2)
    old = hip_ops.set_option(hip_ops.OPT_SIR_FUSED, 0)
    assert int(_lib.lib().fsf_get_option(hip_ops.OPT_SIR_FUSED)) == 0
    hip_ops.set_option(hip_ops.OPT_SIR_FUSED, old)
    assert hasattr(switches, "SIR_FUSED") and BLOCK_ROWS % 16 == 0


@pytest.mark.parametrize("n,m,rows", [(1, 1, True), (17, 3, False), (129, 16, False), (1009, 37, True), (40003, 2500, False)])
def test_row_counts(device, lidar, n, m, rows):
    _same(_desc(lidar), _lidar_inputs(device, n), _random_segments(device, n, m), m, rows)


def test_every_row_its_own_segment(device, lidar):
    n = 3 * BLOCK_ROWS + 21
    _same(_desc(lidar), _lidar_inputs(device, n), torch.arange(n, device=device), n, False)


def test_one_segment_only(device, lidar):
    n = 5 * BLOCK_ROWS + 7
    _same(_desc(lidar), _lidar_inputs(device, n), torch.zeros(n, dtype=torch.int64, device=device), 1, True)


def test_sixteen_groups(device, lidar):
    n = 2 * BLOCK_ROWS + 77  # (16: the smallest group count the modules send to the native stack)
    _same(_desc(lidar), _lidar_inputs(device, n), _random_segments(device, n, 16, seed=5), 16, False)


def test_a_segment_that_straddles_several_row_blocks(device, lidar):
    # segment 1 begins 5 rows before the end of block 0, covers blocks 1 and 2 whole and ends 9 rows into block 3; short segments around
    n = 4 * BLOCK_ROWS + 50
    seg = torch.empty(n, dtype=torch.int64)
    a, b = BLOCK_ROWS - 5, 3 * BLOCK_ROWS + 9
    seg[:a] = 0
    seg[a:b] = 1
    seg[b:] = 2 + torch.arange(n - b) // 7
    m = int(seg[-1]) + 1
    g = _same(_desc(lidar), _lidar_inputs(device, n), seg.to(device), m, True)
    assert torch.isfinite(g).all()


def test_a_last_block_with_a_single_row(device, lidar):
    n = 2 * BLOCK_ROWS + 1
    seg = torch.cat([_random_segments(device, n - 1, 9, seed=7), torch.tensor([9], device=device)])  # (that row is a segment of its own)
    _same(_desc(lidar), _lidar_inputs(device, n), seg, 10, True)
    seg[-1] = 8  # ... and the tail of the segment in front of it
    _same(_desc(lidar), _lidar_inputs(device, n), seg, 9, True)


@pytest.mark.parametrize("n,m", [(1009, 40), (BLOCK_ROWS * 3, 16)])
def test_refine_head_widths(device, refine, n, m):
    desc = _desc(refine)
    assert [int(b.in_cols) for b in desc.blocks] == [181, 146, 146]
    _same(desc, _refine_inputs(device, n), _random_segments(device, n, m, seed=11), m, False)


@pytest.mark.parametrize("n,m", [(1009, 40), (BLOCK_ROWS + 16, 16)])
def test_camera_stack_widths(device, camera, n, m):
    desc = _desc(camera)
    assert [int(b.in_cols) for b in desc.blocks] == [133, 133, 133]
    _same(desc, _camera_inputs(device, n), _random_segments(device, n, m, seed=13), m, True)


def test_a_shape_outside_the_scope_falls_back_to_the_two_kernels(device, monkeypatch):
    """bf16 x 6 weights (switches.K22F off) are outside the fused kernel's scope: with the option on the stack runs the two kernels, and
    returns what it returns with the option off."""
    monkeypatch.setattr(switches, "K22F", False)
    sir = _sir(5 + 11 + 33 + 131, device)  # (fresh: the prepared weights are cached per module in the format the switch chose)
    desc = _desc(sir)
    assert not any(int(b.layer[0].left_f16) for b in desc.blocks)
    n, m = 1009, 37
    _same(desc, _lidar_inputs(device, n), _random_segments(device, n, m), m, True, expect_fused=False)


def test_guard_bands(device, lidar):
    """A strided group table and the rows inside larger zero-filled buffers: nothing outside the written columns / rows changes."""
    n, m = 2 * BLOCK_ROWS + 33, 19
    desc, inputs, seg = _desc(lidar), _lidar_inputs(device, n), _random_segments(device, n, m, seed=17)
    res = {}
    for fused in (0, 2):
        table = torch.zeros((m + 2, 4 + WIDTH + 8), device=device)
        table[1:m + 1, 4:4 + WIDTH] = float("-inf")
        rows_buf = torch.zeros((n + 3, 128), device=device)
        rows, _, _ = _run(desc, inputs, seg, m, True, fused, groups=table[1:m + 1, 4:4 + WIDTH], rows_out=rows_buf[1:n + 1])
        assert rows.data_ptr() == rows_buf[1:].data_ptr()
        assert (table[0] == 0).all() and (table[m + 1] == 0).all() and (table[:, :4] == 0).all() and (table[:, 4 + WIDTH:] == 0).all()
        assert (rows_buf[0] == 0).all() and (rows_buf[n + 1:] == 0).all()
        assert torch.isfinite(table).all() and torch.isfinite(rows_buf).all()
        res[fused] = (table, rows_buf)
    assert torch.equal(res[0][0], res[2][0]) and torch.equal(res[0][1], res[2][1])
