"""GPU: the dynamic point pooling (K17, csrc/point_pool.hip) on the cases of tests/pool_cases.py — the suite's eight old shapes made
margin-clean, one RoI's hits on both sides of PB_CAP, one, two and three rounds of the index-range narrowing, the global cap inside the
binned fill, rectangles of cells on both sides of the table-walk threshold, border cells, integer / -0.0 / non-finite points, a batch
whose samples share cells, sizes at the tile edges, column offsets, and both forms of the scan behind the brute-force passes.

Each case runs both paths in one process; each path must return the referee's rows — point indices, RoI indices, the xyz columns and
is_in_margin exactly, local coordinates and face distances within `pool_cases.feature_tolerance` — the cell-binned path must equal the
brute-force passes bit for bit, and a second call must return the same bits.  What each case reaches is asserted on the CPU in
tests/test_pool_cases_cpu.py."""
import numpy as np
import pytest
import torch

import pool_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(device):
    from fullysparsefusion_amd import hip_ops

    return hip_ops


def device_rows(ops, device, c, brute):
    """One call of the public op on a case, on the path asked for (max_inbox above PB_CAP takes the brute-force passes either way)."""
    rois = torch.from_numpy(c["rois"].copy()).to(device)
    pts = torch.from_numpy(c["pts"].copy()).to(device)
    if c["xyz_col"]:
        pts = pts[:, c["xyz_col"]:c["xyz_col"] + 3]  # a row-strided view
    pb = None if c["pts_batch"] is None else torch.from_numpy(c["pts_batch"].copy()).to(device)
    old = ops.set_option(ops.OPT_POOL_BRUTE, int(brute))  # (fsf_set_option: the library reads no environment variable per call)
    try:
        return ops.dynamic_point_pool(rois, pts, list(c["extra"]), c["max_inbox"], c["max_all"], roi_batch_col=c["batch_col"],
                                      box_col=c["box_col"], pts_batch=pb)
    finally:
        ops.set_option(ops.OPT_POOL_BRUTE, old)


def assert_rows_equal_the_referee(name, path, got, c, want):
    gp, gr, gf = (t.cpu().numpy() for t in got)
    wp, wr, wf = want
    assert gp.dtype == np.int64 and gr.dtype == np.int64 and gf.dtype == np.float32 and gf.shape == (gp.size, 13)
    np.testing.assert_array_equal(gr, wr)
    np.testing.assert_array_equal(gp, wp)
    np.testing.assert_array_equal(gf[:, :3], wf[:, :3])
    np.testing.assert_array_equal(gf[:, :3], P.xyz(c)[wp])
    tol, own = P.feature_tolerance(c, wp, wr, wf)
    err = float(np.abs(gf[:, 3:12] - wf[:, 3:12]).max()) if gp.size else 0.0
    print(f"{name} {path}: rows {gp.size}, feature error {err:.3e}, allowed {tol:.3e} (oracle vs float64 {own:.3e}), ratio {err / tol:.3f}")
    assert err <= tol
    np.testing.assert_array_equal(gf[:, 12], wf[:, 12])


@pytest.mark.parametrize("name", P.NAMES)
def test_both_paths_equal_the_referee_and_each_other(ops, device, name):
    c, want = P.case(name), P.want(name)
    brute = device_rows(ops, device, c, True)
    binned = device_rows(ops, device, c, False)
    again = device_rows(ops, device, c, False)
    assert_rows_equal_the_referee(name, "brute", brute, c, want)
    assert_rows_equal_the_referee(name, "binned", binned, c, want)
    for a, b in zip(binned, brute):   # bit for bit, NaN-safe: compare the bytes
        assert a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                  b.view(torch.int32) if b.dtype == torch.float32 else b)
    for a, b in zip(again, binned):  # a second call returns the same bits
        assert a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                  b.view(torch.int32) if b.dtype == torch.float32 else b)
