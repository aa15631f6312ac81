"""Guard bands and poison around the allocating C-ABI wrapper of hip_ops_mask.py (K34c), in the manner of
tests/test_guard_bands_project_gpu.py: each case calls the wrapper plain, under `guarded(0xFF)` and under `guarded(0x00)`; no guard byte of
the output may change, the wrapper asks for no scratch, and the planes are bit-identical across the three runs."""
import numpy as np
import pytest
import torch

from test_guard_bands_gpu import G, three_runs

pytestmark = pytest.mark.gpu

CASES = {}  # wrapper name -> [(kind, build)], build(ops, dev) -> run


def cases(name, **kinds):
    def deco(factory):
        for kind, kw in kinds.items():
            CASES.setdefault(name, []).append((kind, lambda ops, dev, _kw=kw: factory(ops, dev, **_kw)))
        return factory
    return deco


@pytest.fixture(scope="module")
def ops(device):
    from fullysparsefusion_amd import hip_ops_mask

    return hip_ops_mask


@cases("paint_roi_masks", ragged=dict(rows=5, m=7, dst=(37, 272), out_dtype=torch.int32, tex=torch.float16),
       minimal=dict(rows=1, m=1, dst=(1, 16), out_dtype=torch.uint8, tex=torch.float32),
       empty=dict(rows=0, m=28, dst=(3, 16), out_dtype=torch.uint8, tex=torch.float32))
def _paint_roi_masks(ops, dev, rows, m, dst, out_dtype, tex):
    """Two planes of source size 30 x 48 (plane 1 resized on the fly when dst differs); the maps lie in a NaN-filled buffer of which
    only every other map is pointed at."""
    from fullysparsefusion_amd.mmdet3d_plugin.datasets import mask_paint as mp

    sh, sw = 30, 48
    g = G(6)
    boxes = torch.tensor([[-4.2, 3.1, 20.7, 25.9], [10.5, 8.0, 47.9, 33.0], [30.0, 2.0, 30.4, 28.0], [5.0, 5.0, 5.0, 9.0],
                          [-20.0, -20.0, 70.0, 50.0]], dtype=torch.float32)[:rows]
    if rows == 1:
        boxes = torch.tensor([[-1.0, -1.0, 20.0, 3.0]], dtype=torch.float32)
    maps = torch.full((2 * max(rows, 1), m, m), float("nan"))
    maps[::2] = torch.sigmoid(torch.randn(max(rows, 1), m, m, generator=g) * 3.0) if rows != 1 else 1.0
    plane = [0, 0, 0, 1, 1][:rows]
    table = torch.zeros((rows, 8), dtype=torch.int32)
    for r in range(rows):
        table[r] = torch.tensor([plane[r], *mp.roi_rect(boxes[r].numpy(), (sh, sw)), 0, -1, 300 + r])
    plane_ptr = torch.tensor(np.searchsorted(np.asarray(plane), [0, 1, 2]), dtype=torch.int32)
    roi_off = torch.arange(rows, dtype=torch.int64) * (2 * m * m)
    hw = torch.tensor([[sh, sw]] * 2, dtype=torch.int32)
    scale = torch.tensor([[np.float32(sh / dst[0]), np.float32(sw / dst[1])]] * 2, dtype=torch.float32)
    args = [t.to(dev) for t in (table, boxes.reshape(-1, 4), roi_off, plane_ptr, hw, scale)]
    rois = maps.to(tex).to(dev)
    return lambda: ops.paint_roi_masks(*args, dst, out_dtype, rois, m, 0.5)


@pytest.mark.parametrize("name,kind", [(n, k) for n in sorted(CASES) for k, _ in CASES[n]])
def test_wrapper_under_guard_bands_and_poison(ops, device, name, kind):
    run = dict(CASES[name])[kind](ops, device)

    def scratch_expected(g):
        assert g.workspace_sizes == [] and sum(r["kind"] == "empty" and r["site"] == name for r in g.records) == 1

    (planes,) = three_runs(run, scratch_expected)
    assert planes.dim() == 3 and planes.size(0) == 2
    if kind == "ragged":
        assert planes[0].unique().numel() >= 3 and bool((planes[0] == 0).any()) and bool(planes[1].any())
    if kind == "minimal":
        assert bool(planes[0].any()) and not bool(planes[1].any())
    if kind == "empty":
        assert not bool(planes.any())
