"""GPU: the device connected components (K19) on the layouts of tests/ccl_cases.py — tile edges, pruned strips, sorted chains, a
bridge that arrives last, blobs that overflow the link queue, pairs exactly at the threshold, degenerate distances and rows, samples
and groups that share coordinates — through all three entry forms.  The labels must be the referee's own (numbered by first member),
not merely the same partition; each entry point is called once per case.  What the layouts reach is asserted on the CPU in
tests/test_ccl_cases_cpu.py."""
import numpy as np
import pytest
import torch

import ccl_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(device):
    from fullysparsefusion_amd import hip_ops

    return hip_ops


def _device_labels(ops, device, c):
    pts = torch.from_numpy(c["points"].copy()).to(device)
    if c["kind"] == "plain":
        return ops.connected_components(pts, c["dist"])
    idx = torch.from_numpy(c["idx"].copy()).to(device)
    if c["kind"] == "batched":
        return ops.connected_components(pts, c["dist"], batch_idx=idx)
    return ops.connected_components_grouped(pts, idx, torch.from_numpy(c["table"].copy()).to(device))


@pytest.mark.parametrize("name", C.NAMES)
def test_labels_equal_the_referee(ops, device, name):
    c = C.case(name)
    got = _device_labels(ops, device, c)
    assert got.dtype == torch.int32 and got.shape == (c["points"].shape[0],)
    np.testing.assert_array_equal(got.cpu().numpy(), c["want"])


def _raw_call(ops, device, c, n=None):
    """The C entry point of the case's kind, straight through the library handle: (labels i32 [n], num_components_dev i64 [1])."""
    from fullysparsefusion_amd import _lib

    n = c["points"].shape[0] if n is None else n
    pts = torch.from_numpy(c["points"][:n].copy()).to(device)
    idx = None if c["idx"] is None else torch.from_numpy(c["idx"][:n].copy()).to(device)
    labels = torch.full((n,), -7, dtype=torch.int32, device=device)
    count = torch.full((1,), -7, dtype=torch.int64, device=device)
    h = ops._L()
    ws = _lib.workspace(h.fsf_connected_components_workspace_bytes(n), device)
    if c["kind"] == "grouped":
        table = torch.from_numpy(c["table"].copy()).to(device)
        rc = h.fsf_connected_components_grouped(_lib.ptr(pts), n, pts.size(1), _lib.ptr(idx), _lib.ptr(table), table.numel(), _lib.ptr(labels),
                                                _lib.ptr(count), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    else:
        rc = h.fsf_connected_components(_lib.ptr(pts), n, pts.size(1), _lib.ptr(idx), float(c["dist"]), _lib.ptr(labels), _lib.ptr(count),
                                        _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "connected components")
    return labels.cpu().numpy(), int(count.cpu()[0])


@pytest.mark.parametrize("name", ["tile_edges-2049", "batch_shared-3", "group_sorted"])
def test_component_count_is_written(ops, device, name):
    """`num_components_dev` of each entry form equals labels.max() + 1 (= the referee's count), and 0 for no points."""
    c = C.case(name)
    labels, count = _raw_call(ops, device, c)
    np.testing.assert_array_equal(labels, c["want"])
    assert count == int(labels.max()) + 1 == int(c["want"].max()) + 1
    labels, count = _raw_call(ops, device, c, n=0)
    assert count == 0 and labels.size == 0


@pytest.mark.parametrize("name", ["batch_shared-2", "batch_shared-3"])
def test_find_connected_componets_numbers_sample_by_sample(ops, device, name):
    """The detector's batched helper against the reference's rule: per-sample components, sample 0's numbered first."""
    from fullysparsefusion_amd.mmdet3d_plugin.models.detectors.single_stage_fsd import find_connected_componets

    c = C.case(name)
    pts = torch.from_numpy(c["points"].copy()).to(device)
    idx = torch.from_numpy(c["idx"].copy()).to(device)
    got = find_connected_componets(pts, idx, c["dist"])
    np.testing.assert_array_equal(got.cpu().numpy(), C.batched_reference_order(c["points"], c["idx"], c["dist"]))


def test_grouped_call_as_the_cluster_assigner_makes_it(ops, device):
    """ClusterAssigner hands over [n, 3] voxel centres in group order, the group of every voxel (int32 from the survival kernel,
    int64 on the generic tail) and the per-class distances as a float32 device tensor."""
    c = C.case("group_sorted")
    assert c["points"].shape[1] == 3 and (np.diff(c["idx"]) >= 0).all()
    vox_centers = torch.from_numpy(c["points"].copy()).to(device)
    dist = torch.tensor(c["table"].tolist(), dtype=torch.float32).to(device)
    vox_group_i32 = torch.from_numpy(c["idx"].copy()).to(device)
    labels = ops.connected_components_grouped(vox_centers, vox_group_i32, dist)
    np.testing.assert_array_equal(labels.cpu().numpy(), c["want"])
    labels = ops.connected_components_grouped(vox_centers, vox_group_i32.long(), dist).long()
    np.testing.assert_array_equal(labels.cpu().numpy(), c["want"].astype(np.int64))
