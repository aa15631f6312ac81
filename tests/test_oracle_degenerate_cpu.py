"""The oracle chain on degenerate frames and on batches (oracle/modules.py: `simple_test`, `simple_test_batch`), on the CPU.

The un-restarted oracle chain is the referee of tests/test_batch_inference_gpu.py.  Before it may judge the device it has to
(1) return on frames with nothing in them, through the reference's own empty branches, (2) reproduce itself — a batch of one
is the single-sample chain, a batch whose samples decide nothing jointly is its samples' chains, bit for bit — and (3) state the
reference's batch-wide rules where they do fire.  (4) checks the GPU test's inputs: the answers a cross-wired detector would
give have to FAIL that test's criterion, otherwise the inputs are too alike to catch the bug.
"""
import numpy as np
import pytest
import torch

import batch_cases as bc
from conftest import build_test_fsf
from oracle import modules as omod


@pytest.fixture(scope="module")
def cpu():
    return build_test_fsf()


@pytest.fixture(scope="module")
def a():
    return bc.sample_a()


@pytest.fixture(scope="module")
def b():
    return bc.sample_b()


def crop(sample, n, start=0):
    return (sample[0][start:start + n].contiguous(),) + tuple(sample[1:])


def same_result(x, y):
    """Bit-identical final rows and refinement intermediates (the RoIs without their sample column)."""
    return (all(torch.equal(x[k], y[k]) for k in ("boxes", "scores", "labels", "refined_query", "cls_logits", "reg_preds"))
            and torch.equal(x["rois"][:, 1:], y["rois"][:, 1:]))


# ------------------------------------------------------------------------------------------- (1) degenerate frames
@pytest.mark.parametrize("name", ["zeroed_masks", "points_300", "one_point", "masks_in_the_sky"])
def test_the_chain_returns_on_a_degenerate_frame_through_the_fake_camera_query(cpu, a, name):
    s = bc.degenerate_samples(a)[name]
    with torch.no_grad():
        o = omod.simple_test(cpu, *s)
    # no point inside any mask -> FSF.py:407-414: exactly one camera query, key (0, 0, 0), centre 0, the all-zero 2-D row with the
    # "no class" category
    assert int((o["s1"]["obj_id"] > 0).sum()) == 0 and o["s2"]["fake"]
    assert o["s2"]["obj_coors"].tolist() == [[0, 0, 0]]
    assert o["s2"]["obj_centers"].tolist() == [[0.0, 0.0, 0.0]]
    want_2d = torch.zeros(1, 9)
    want_2d[0, 5] = cpu.num_classes
    assert torch.equal(o["s2"]["preds_2d"], want_2d)
    assert int(o["query_coors"].shape[0]) == 1 + int(o["s3"]["cluster_inds"].shape[0])
    # one sample always keeps at least one LiDAR query per class group (single_stage_fsd.py:832-834, :952-954)
    assert sorted(set(o["s3"]["cluster_inds"][:, 0].tolist())) == list(range(len(cpu.cfg["group_names"])))
    assert o["boxes"].shape[1] == 9 and bool(torch.isfinite(o["boxes"]).all()) and o["boxes"].shape[0] == o["scores"].shape[0]
    if name == "one_point":  # one pre-voxel: it is every group's forced foreground point and no cell holds `min_points` centres
        assert all(o["s3"]["rules"]["inverted"]) and o["s3"]["cluster_inds"].shape[0] == len(cpu.cfg["group_names"])
        assert o["s3"]["points"].shape[0] == len(cpu.cfg["group_names"])


def test_a_cloud_under_every_score_threshold_keeps_one_forced_query_per_group(cpu, a):
    s = crop(a, 5000)
    bias = cpu.segmentor.segmentation_head.conv_seg.bias
    before = bias.detach().clone()
    with torch.no_grad(), bc.background_only(cpu):
        o = omod.simple_test(cpu, *s)
    assert torch.equal(bias.detach(), before)
    assert all(o["s3"]["rules"]["forced_first"]) and all(o["s3"]["rules"]["inverted"])
    ng = len(cpu.cfg["group_names"])
    assert o["s3"]["cluster_inds"].tolist() == [[g, 0, 0] for g in range(ng)]
    first = o["s3"]["pre_voxel_coors"][0]  # every group's one point is the sample's first pre-voxel (get_sample_beg_position)
    assert int(o["s3"]["points"].shape[0]) == ng and bool((o["s3"]["points"] == o["s3"]["points"][0]).all())
    z, y, x = (int(v) for v in first[1:])
    cell = np.floor((o["s3"]["points"][0, :3].numpy() - np.array(cpu.cluster_assigner.point_cloud_range[:3], np.float32))
                    / np.array(cpu.cfg["pre_voxelization_size"], np.float32)).astype(int)
    assert cell.tolist() == [x, y, z]


def test_a_sample_without_points_raises_in_the_oracle_and_in_the_product(cpu, a):
    """The reference raises on an empty cloud (`batch_idx.max()` of an empty tensor, single_stage_fsd.py:803-804); the oracle and the
    product say so before anything is computed — the product on any device, this is the host-side check."""
    empty = (a[0][:0].contiguous(),) + tuple(a[1:])
    with pytest.raises(ValueError, match="without points"):
        omod.simple_test(cpu, *empty)
    with pytest.raises(ValueError, match="without points"):
        omod.simple_test_batch(cpu, [crop(a, 300), empty])
    for pts in ([empty[0]], [a[0][:300].contiguous(), empty[0]]):
        n = len(pts)
        with pytest.raises(ValueError, match="has no points"), torch.no_grad():
            cpu.simple_test(pts, [dict(lidar2img=a[3])] * n, torch.stack([a[1]] * n), torch.stack([a[2]] * n))
        with pytest.raises(ValueError, match="has no points"), torch.no_grad():
            cpu.simple_test(pts, [dict(lidar2img=a[3])] * n, torch.stack([a[1]] * n), torch.stack([a[2]] * n), hot_path_only=True)


# ------------------------------------------------------------------------------------------- (2) the chain reproduces itself
def test_a_batch_of_one_is_the_single_sample_chain_bit_for_bit(cpu, b):
    s = crop(b, 8000)
    with torch.no_grad():
        one, (bat,) = omod.simple_test(cpu, *s), omod.simple_test_batch(cpu, [s])
    assert same_result(one, bat) and one["boxes"].shape[0] > 0
    assert torch.equal(one["s2"]["obj_coors"], bat["s2"]["obj_coors"]) and torch.equal(one["s3"]["cluster_inds"], bat["s3"]["cluster_inds"])
    assert torch.equal(one["query_feats"], bat["query_feats"])


def test_a_batch_that_decides_nothing_jointly_is_its_samples_chains_bit_for_bit(cpu, a, b):
    """Two well-filled samples on opposite sides of the car (|y| > 3 m each: farther apart than any `connected_dist`, votes
    included — asserted through `bridged`), with the same groups forced in both: none of the batch-wide rules of
    `simple_test_batch` changes anything, so each sample's result is its single-sample result exactly; the LiDAR ids may be
    renumbered (batch-wide component labels), the groups they name may not."""
    x, y = bc.half(crop(a, 16000, start=8000), +1), bc.half(crop(b, 16000, start=4000), -1)
    with torch.no_grad():
        singles = [omod.simple_test(cpu, *x), omod.simple_test(cpu, *y)]
        batch = omod.simple_test_batch(cpu, [x, y])
    rules = batch[0]["s3"]["rules"]
    assert sum(rules["bridged"]) == 0, rules
    for s in singles:  # the precondition, not the result: both samples alone take the forced point / the inversion in the same groups
        assert s["s3"]["rules"]["forced_first"] == rules["forced_first"] and s["s3"]["rules"]["inverted"] == rules["inverted"]
    for i, (s, r) in enumerate(zip(singles, batch)):
        assert s["boxes"].shape[0] > 100 and s["s2"]["obj_coors"].shape[0] > 5 and s["s3"]["cluster_inds"].shape[0] > 40
        assert same_result(s, r), i
        assert torch.equal(s["s2"]["obj_coors"][:, 1:], r["s2"]["obj_coors"][:, 1:]) and bool((r["s2"]["obj_coors"][:, 0] == i).all())
        assert bool((r["s3"]["cluster_inds"][:, 1] == i).all())
        cols = [0, 2]
        assert (omod.query_partition(s["s3"]["pts_cluster_inds"][:, cols], s["s3"]["points"])
                == omod.query_partition(r["s3"]["pts_cluster_inds"][:, cols], r["s3"]["points"]))
        assert torch.equal(s["s3"]["cluster_xyz"], r["s3"]["cluster_xyz"])  # (same groups in the same order: same centres)


# ------------------------------------------------------------------------------------------- (3) the batch-wide rules
def test_the_fake_camera_query_is_a_property_of_the_batch(cpu, a):
    """FSF.py:400-414 tests the batch's tensor: one fake query (sample 0) when NO sample has a camera point, none otherwise."""
    with_cam, no_cam = crop(a, 3000, start=12000), crop(a, 300)
    with torch.no_grad():
        s1 = [omod.fsf_stage1(cpu, *s) for s in (with_cam, no_cam)]
        assert int((s1[0]["obj_id"] > 0).sum()) > 0 and int((s1[1]["obj_id"] > 0).sum()) == 0
        mixed = omod.simple_test_batch(cpu, [with_cam, no_cam])
        none = omod.simple_test_batch(cpu, [no_cam, no_cam])
    assert mixed[0]["s2"]["obj_coors"].shape[0] > 0 and not mixed[0]["s2"]["fake"]
    assert mixed[1]["s2"]["obj_coors"].shape == (0, 3) and mixed[1]["s2"]["obj_feat"].shape[0] == 0 and not mixed[1]["s2"]["fake"]
    assert mixed[1]["query_coors"].shape[0] == mixed[1]["s3"]["cluster_inds"].shape[0] > 0  # LiDAR queries only
    assert none[0]["s2"]["fake"] and none[0]["s2"]["obj_coors"].tolist() == [[0, 0, 0]]
    assert none[1]["s2"]["obj_coors"].shape == (0, 3)


def test_connected_components_and_the_density_mask_are_taken_over_the_batch(cpu, a, b):
    """single_stage_fsd.py:69-82 / :952-954: two overlapping clouds bridge each other's components (never more LiDAR queries per sample
    than alone); a one-point sample next to a dense one keeps no point in the groups where the dense one has a dense cell (its
    density mask is not inverted there) — alone it keeps one query in every group."""
    x, y, one = crop(a, 8000), crop(b, 8000), crop(a, 1, start=20000)
    ng = len(cpu.cfg["group_names"])
    with torch.no_grad():
        sx, sy, so = (omod.fsf_stage1(cpu, *s) for s in (x, y, one))
        alone_x, alone_one = omod.fsf_stage3(cpu, sx), omod.fsf_stage3(cpu, so)
        both = omod.fsf_stage3_batch(cpu, [sx, _with_batch(sy, 1)])
        pair = omod.fsf_stage3_batch(cpu, [sx, _with_batch(so, 1)])
    assert sum(both[0]["rules"]["bridged"]) > 0
    assert both[0]["cluster_inds"].shape[0] <= alone_x["cluster_inds"].shape[0]  # (components only ever merge)
    assert bool((both[1]["cluster_inds"][:, 1] == 1).all())
    assert alone_one["cluster_inds"].shape[0] == ng and all(alone_one["rules"]["inverted"])
    dense_groups = [g for g in range(ng) if not pair[0]["rules"]["inverted"][g]]
    assert dense_groups and sorted(set(pair[1]["cluster_inds"][:, 0].tolist())) == [g for g in range(ng) if g not in dense_groups]


def _with_batch(s1, b):
    s1 = dict(s1)
    s1["batch_idx"] = torch.full_like(s1["batch_idx"], b)
    return s1


# ------------------------------------------------------------------------------------------- (4) the GPU test can fail
def test_cross_wired_answers_fail_the_gpu_tests_criterion(cpu, a, b):
    """tests/test_batch_inference_gpu.py compares the device's result for sample 1 of [A, B] with the oracle's.  Here: the oracle's
    answer for sample 1 when it is given A's masks, A's `mask_anno` or A's calibration instead of B's, and A's answer in B's slot,
    each FAIL that comparison against B's true answer (and the true answer passes against itself).  Also the conditions that test
    states for its samples: both have camera and LiDAR queries, 500 boxes, and no NMS decision near the threshold."""
    _, report = bc.assert_inputs_discriminate(cpu, a, b)
    print("\ncross-wiring:", report)
