"""Batched and degenerate-frame inference on the device against the un-restarted oracle chain.

Every other value check of `FSF.simple_test` runs ONE well-filled sample.  A batch takes other code (the `batch_size == 1` / `bsz == 1`
gates of detectors/fsf.py, detectors/single_stage_fsd.py and dense_heads/cluster_heads.py: the per-sample `frustum_gather` loop,
`combine_by_batch`, `get_all_cls_preds_2d`, the Python clustering sequence instead of K30, `split_by_batch` before the box tail, no
frame front), and a frame with nothing in it takes the branches written for emptiness.  Here:

 (a) [A, B] — two samples that share no per-sample input (tests/batch_cases.py) — against `oracle.modules.simple_test_batch`, with the
     matching and the frozen thresholds of tests/test_e2e_agreement_gpu.py (tests/e2e_matching.py) and identical query keys;
 (b) before anything runs on the device: the answers a cross-wired detector would give FAIL (a) (`assert_inputs_discriminate`);
 (c) order ([B, A] against the oracle's [B, A]; swapped results where no pooling capacity binds — see that test) and isolation (a sample
     inside a batch against the same sample alone) on the device;
 (d) three samples with an empty one in the middle;
 (e) degenerate single frames, each shown to enter the branch it is named for;
 (f) a batch through `set_next_frame` (declined: bit-identical, nothing left queued) and through `forward_hot_path`.

What "a sample's own result" means inside a batch is `simple_test_batch`'s docstring: the reference clusters the voted centres of
ALL samples together at test time, so two clouds that overlap bridge each other's components — sample 0 of [A, B] has fewer LiDAR
queries than A alone, by the reference's rule, and the product follows it.  Isolation against "alone" is therefore asserted in full
on a pair that the oracle certifies to decide nothing jointly (opposite sides of the car), and for [A, B] on everything upstream of
the clustering.

One JSON report per case: batch_inference_<case>.json in the directory FSF_TEST_REPORT_DIR names (default: test_reports/ in the repository).
"""
import contextlib
import copy
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import batch_cases as bc
from conftest import ROOT, build_test_fsf
from e2e_matching import E2E_MAX_CAMERA_SIR_DEV_P999, E2E_MAX_LIDAR_SIR_DEV_P999, E2E_MAX_UNMATCHED, _feature_deviation
from oracle import modules as omod
from oracle import refine as orefine

pytestmark = pytest.mark.gpu


def write_report(case, report):
    out_dir = os.environ.get("FSF_TEST_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    os.makedirs(out_dir, exist_ok=True)
    print(f"\nbatch inference [{case}]:", json.dumps(report, indent=1, default=str))
    with open(os.path.join(out_dir, f"batch_inference_{case}.json"), "w") as fh:
        json.dump(report, fh, indent=1, default=str)


@pytest.fixture(scope="module")
def ctx(device):
    model = build_test_fsf()
    cpu = copy.deepcopy(model)
    a, b = bc.sample_a(), bc.sample_b()
    # (b): on the CPU, before the device sees anything — the oracle's [A, B] answers and the proof that (a) can fail on them
    truth, wiring = bc.assert_inputs_discriminate(cpu, a, b)
    write_report("cross_wiring_cpu", dict(boxes_of_500_that_still_agree_with_b=wiring))
    return SimpleNamespace(model=model.to(device), cpu=cpu, a=a, b=b, truth=truth, device=device)


def dev_args(samples, device):
    return ([s[0].to(device) for s in samples], [dict(lidar2img=s[3].to(device)) for s in samples],
            torch.stack([s[1] for s in samples]).to(device), torch.stack([s[2] for s in samples]).to(device))


def run(model, samples, device, hot_path_only=False):
    """`simple_test` on the device with taps on every structure a wiring bug would show in; tensors come back on the CPU."""
    cap = {}
    taps = []

    def tap(obj, name, key, keep):
        orig = getattr(obj, name)

        def wrapped(*a, **k):
            out = orig(*a, **k)
            cap[key] = keep(a, k, out)
            return out

        obj.__dict__[name] = wrapped
        taps.append((obj, name))

    c = lambda t: t.detach().cpu()  # noqa: E731
    tap(model.segmentor, "voxelize", "voxel", lambda a, k, out: (c(out[0]), c(out[1])))
    tap(model.frustum_sir, "forward", "cam_rows", lambda a, k, out: (c(a[0])[:, :3], c(a[2])))
    tap(model.backbone, "forward", "lid_rows", lambda a, k, out: (c(a[0])[:, :3], c(a[2])))
    tap(model, "combine_frustum_and_fsd", "combine", lambda a, k, out: ([c(a[i]) for i in (0, 1, 3, 5, 6, 8)], c(out[1])))
    tap(model.roi_extractor, "forward", "roi", lambda a, k, out: (c(a[1]), c(a[2]), c(out[0]), c(out[1])))
    tap(model.frustum_refined_head[0], "get_bboxes", "tail", lambda a, k, out: ([c(t) for t in a[0]], [c(t) for t in a[1]], c(a[3]), c(a[4])))
    try:
        with torch.no_grad():
            res = model.simple_test(*dev_args(samples, device), hot_path_only=hot_path_only)
        torch.cuda.synchronize()
    finally:
        for obj, name in taps:
            del obj.__dict__[name]
    if hot_path_only:
        return {k: (c(v) if torch.is_tensor(v) else v) for k, v in res.items() if k != "seg"}, cap
    return [bc.device_result(r) for r in res], cap


# ------------------------------------------------------------------------------------------------ per-sample structure
def _groups(keys, ident):
    """{key row: frozenset of the identities of its rows}"""
    out = {}
    for k, i in zip(keys.tolist(), ident):
        out.setdefault(tuple(k), []).append(i)
    return {k: frozenset(v) for k, v in out.items()}


def _raw_points(xyz):
    """Identity of an INPUT point: its coordinates' bytes (the camera branch groups the cloud's own rows)."""
    xyz = np.ascontiguousarray(xyz.numpy().astype(np.float32))
    return [xyz[i].tobytes() for i in range(xyz.shape[0])]


def _pre_voxels(model, xyz):
    """Identity of a LiDAR-branch row: the 0.1 m pre-voxelization cell it is the mean of (single_stage_fsd.py:585-605).  The mean's
    floats depend on the summation order — device against oracle, batch against alone — its cell does not."""
    lo = np.array(model.cluster_assigner.point_cloud_range[:3], np.float64)
    size = np.array(model.cfg["pre_voxelization_size"], np.float64)
    return [tuple(r) for r in np.floor((xyz.numpy().astype(np.float64) - lo) / size).astype(np.int64).tolist()]


def lidar_partition(model, pts_cluster_inds, points, sample=None):
    """{(group, cells of the cluster)} of the rows (group, sample, id) of one sample (all rows when `sample` is None)."""
    g = _groups(pts_cluster_inds, _pre_voxels(model, points[:, :3]))
    return {(k[0], v) for k, v in g.items() if sample is None or k[1] == sample}


def structure(model, cap, n_samples):
    """Per sample, every integer decision of a run in a form that does not depend on the sample's slot or on id numbering: voxel keys,
    the camera queries as {instance id: points}, the LiDAR queries as {(group, points)}, the RoI membership as {(query, point)}."""
    pts, coors = cap["voxel"]
    cam = _groups(cap["cam_rows"][1], _raw_points(cap["cam_rows"][0]))          # (sample, 0, id)
    lid = _groups(cap["lid_rows"][1], _pre_voxels(model, cap["lid_rows"][0]))   # (group, sample, id)
    q_coors = cap["combine"][1]                               # (sample, 0 | group, id | id + begin) per query = per RoI
    n_cam = cap["combine"][0][1].shape[0]
    lid_keys = cap["combine"][0][4]
    ident = []
    for r in range(q_coors.shape[0]):
        if r < n_cam:
            ident.append(("cam", int(q_coors[r, 2])))
        else:
            g, b, i = (int(v) for v in lid_keys[r - n_cam])
            ident.append(("lid", g, lid[(g, b, i)]))
    pooled = {}
    if "roi" in cap:
        p_batch, rois, inds, roi_inds = cap["roi"]
        first = {b: int((p_batch == b).nonzero()[0]) for b in range(n_samples) if bool((p_batch == b).any())}
        for p, r in zip(inds.tolist(), roi_inds.tolist()):
            if r >= 0:
                b = int(rois[r, 0])
                pooled.setdefault(b, set()).add((ident[r], p - first[b]))
    out = []
    for b in range(n_samples):
        rows = coors[:, 0] == b
        out.append(dict(
            points=int(rows.sum()), voxel_keys=coors[rows][:, 1:].clone(),
            camera={k[2]: v for k, v in cam.items() if k[0] == b and k[2] > 0},
            lidar={(k[0], v) for k, v in lid.items() if k[1] == b},
            pooled=pooled.get(b, set())))
    return out


def same_structure(x, y, what=("voxel_keys", "camera", "lidar", "pooled")):
    return {k: (torch.equal(x[k], y[k]) if torch.is_tensor(x[k]) else x[k] == y[k]) for k in what}


def keys_vs_oracle(cap, results):
    """Camera and LiDAR query keys as `combine_frustum_and_fsd` received them against the oracle's (batch column included), and the
    SIR group features on the common keys with the bounds of the single-sample end-to-end test."""
    (f_centers, f_coors, f_feats, l_centers, l_coors, l_feats), _ = cap["combine"]
    o_cam, o_lid = omod.batch_query_keys(results)
    o_cam_feats = torch.cat([r["s2"]["obj_feat"] for r in results])
    o_lid_all = torch.cat([r["s3"]["cluster_inds"] for r in results])
    o_lid_feats = torch.cat([r["s3"]["cluster_feats"] for r in results])
    cam = _feature_deviation(f_feats.numpy()[:, :768], f_coors.numpy(), o_cam_feats[:, :768].numpy(), o_cam.numpy())
    lid = _feature_deviation(l_feats.numpy(), l_coors.numpy(), o_lid_feats.numpy(), o_lid_all.numpy())
    return dict(camera=dict(gpu=int(f_coors.shape[0]), oracle=int(o_cam.shape[0]), keys_identical=bool(torch.equal(f_coors, o_cam.to(f_coors.dtype))),
                            sir_feature_dev=cam),
                lidar=dict(gpu=int(l_coors.shape[0]), oracle=int(o_lid.shape[0]), keys_identical=bool(torch.equal(l_coors, o_lid.to(l_coors.dtype))),
                           sir_feature_dev=lid))


def assert_batch_vs_oracle(case, got, cap, oracle, full=None):
    """(a) for the samples in `full` (default: all), the few-boxes rule for the others; identical keys for the whole batch."""
    keys = keys_vs_oracle(cap, oracle)
    report = dict(samples=len(oracle), query_keys=keys, per_sample=[])
    ok_all = True
    for i, (g, o) in enumerate(zip(got, oracle)):
        ok, rep = bc.criterion_a(g, bc.oracle_result(o))
        rep.update(oracle_nms_margin=float(o["margin"]), camera_queries=int(o["s2"]["obj_coors"].shape[0]),
                   lidar_queries=int(o["s3"]["cluster_inds"].shape[0]), criterion_a=ok)
        report["per_sample"].append(rep)
        if full is None or i in full:
            ok_all &= ok
    write_report(case, report)
    assert keys["camera"]["keys_identical"] and keys["lidar"]["keys_identical"], keys
    assert keys["camera"]["sir_feature_dev"]["p999"] <= E2E_MAX_CAMERA_SIR_DEV_P999, keys
    assert keys["lidar"]["sir_feature_dev"]["p999"] <= E2E_MAX_LIDAR_SIR_DEV_P999, keys
    assert ok_all, report
    return report


def restarted_tail_rule(model, cap, got, sample=0, n_samples=1):
    """The rule of tests/test_fullsize_gpu.py::test_final_boxes_vs_oracle_chain on the last discontinuity: the oracle's get_bboxes on
    the DEVICE's refined head outputs of one sample; with its NMS margin above 1e-5 the device's rows are the oracle's (labels equal,
    scores and boxes within 1e-6), otherwise every returned box is one of the decoded candidates."""
    cls, reg, centers, coors = cap["tail"]
    rows = coors[:, 0] == sample
    cfg = model.frustum_refined_head[0].test_cfg
    r, scs, labs, boxes, margin = omod.get_bboxes_single(cfg, cls[0][rows], reg[0][rows], centers[rows])
    o = dict(boxes=boxes[r], scores=scs, labels=labs, margin=margin, all_boxes=boxes)
    return bc.few_boxes_rule(got, o), float(margin)


# ------------------------------------------------------------------------------------------------ (a), (f: hot path)
@pytest.fixture(scope="module")
def ab(ctx):
    return run(ctx.model, [ctx.a, ctx.b], ctx.device)


def test_a_two_sample_batch_against_the_oracle(ctx, ab):
    got, cap = ab
    assert len(got) == 2
    rep = assert_batch_vs_oracle("a_b", got, cap, ctx.truth)
    assert all(r["oracle_nms_margin"] > bc.NEAR_THRESHOLD_MARGIN and r["camera_queries"] > 0 and r["lidar_queries"] > 0 for r in rep["per_sample"])
    # the batch took the reference's batch-wide clustering: components bridged between the two clouds
    assert sum(ctx.truth[0]["s3"]["rules"]["bridged"]) > 0


def test_forward_hot_path_of_a_batch_has_the_oracles_keys(ctx):
    out, cap = run(ctx.model, [ctx.a, ctx.b], ctx.device, hot_path_only=True)
    o_cam, o_lid = omod.batch_query_keys(ctx.truth)
    assert torch.equal(out["frustum_obj_coors"], o_cam.to(out["frustum_obj_coors"].dtype))
    assert torch.equal(out["fsd_obj_coors"], o_lid.to(out["fsd_obj_coors"].dtype))
    n_cam, n_lid = o_cam.shape[0], o_lid.shape[0]
    # the documented widths: camera query features 768 + 128, centres 3, 2-D rows 9; LiDAR query features 768, centres 3
    assert out["frustum_obj_feats"].shape == (n_cam, ctx.model.lidar_img_input_dim) and out["frustum_obj_centers"].shape == (n_cam, 3)
    assert out["frustum_preds_2d"].shape == (n_cam, 9)
    assert out["fsd_obj_feats"].shape == (n_lid, ctx.model.lidar_input_dim) and out["fsd_obj_centers"].shape == (n_lid, 3)
    o_p2d = torch.cat([r["s2"]["preds_2d"] for r in ctx.truth])
    assert torch.equal(out["frustum_preds_2d"], o_p2d)  # B's queries carry B's `mask_anno` rows


# ------------------------------------------------------------------------------------------------ (c)
def disjoint_pair(ctx):
    """Two samples on opposite sides of the car (tests/batch_cases.py::half): no component spans them, and neither fills its pooling capacity."""
    return (bc.half((ctx.a[0][8000:24000],) + tuple(ctx.a[1:]), +1), bc.half((ctx.b[0][4000:20000],) + tuple(ctx.b[1:]), -1))


def test_order_of_the_samples_only_swaps_the_results(ctx, ab):
    """[B, A] against [A, B] swapped.  Every integer decision up to the queries is the same per sample — voxel keys, camera and LiDAR
    partitions — but the LiDAR ids are batch-wide component labels, numbered in the order of the batch's (sample, x, y, z) cells
    (single_stage_fsd.py:962, :69-82): swapping the samples renumbers them, the queries of a sample come out in another order, and
    the pooling capacity (`max_all_pts` per sample, filled in RoI order; A pools 79 767 rows against 50 000) is spent on other RoIs.
    So where the capacity binds the boxes are NOT the swapped ones, by the reference's own rules: the oracle's [B, A] differs from its
    [A, B] in exactly the same way (493 / 500 and 484 / 500 boxes agree under (a), on the oracle and on the device alike).  Asserted:
    [B, A] against the oracle's [B, A] under (a) with identical keys; the integer decisions up to the queries identical to [A, B]'s;
    the device's [A, B] / [B, A] agreement equal to the oracle's own, box count for box count; and on the pair that fills no capacity
    and shares no component, [Y, X] IS [X, Y] swapped: every integer decision, RoI membership included, and the boxes under (a)."""
    got, cap = ab
    with torch.no_grad():
        o_ba = omod.simple_test_batch(ctx.cpu, [ctx.b, ctx.a])
    assert all(o["margin"] > bc.NEAR_THRESHOLD_MARGIN for o in o_ba)
    swapped, cap_s = run(ctx.model, [ctx.b, ctx.a], ctx.device)
    assert_batch_vs_oracle("b_a", swapped, cap_s, o_ba)
    st, st_s = structure(ctx.model, cap, 2), structure(ctx.model, cap_s, 2)
    report = dict(per_sample=[], disjoint_pair=[])
    for i in range(2):
        same = same_structure(st[i], st_s[1 - i])
        ok, rep = bc.criterion_a(swapped[1 - i], got[i])
        _, o_rep = bc.criterion_a(bc.oracle_result(o_ba[1 - i]), bc.oracle_result(ctx.truth[i]))
        rep.update(same_integer_decisions=same, criterion_a=ok, oracle_swapped_agreement=o_rep["matched_iou99_dscore1e3"],
                   capacity_binds=bool(ctx.truth[i]["pooled_points"] >= ctx.model.roi_extractor.max_all_pts), bitwise_equal=dict(
            boxes=bool(np.array_equal(swapped[1 - i][0], got[i][0])), scores=bool(np.array_equal(swapped[1 - i][1], got[i][1]))))
        report["per_sample"].append(rep)
    x, y = disjoint_pair(ctx)
    xy, cap_xy = run(ctx.model, [x, y], ctx.device)
    yx, cap_yx = run(ctx.model, [y, x], ctx.device)
    sd, sd_s = structure(ctx.model, cap_xy, 2), structure(ctx.model, cap_yx, 2)
    for i in range(2):
        ok, rep = bc.criterion_a(yx[1 - i], xy[i])
        rep.update(same_integer_decisions=same_structure(sd[i], sd_s[1 - i]), criterion_a=ok, pooled_pairs=len(sd[i]["pooled"]), bitwise_equal=dict(
            boxes=bool(np.array_equal(yx[1 - i][0], xy[i][0])), scores=bool(np.array_equal(yx[1 - i][1], xy[i][1]))))
        report["disjoint_pair"].append(rep)
    write_report("order_b_a", report)
    for rep in report["per_sample"]:
        same = rep["same_integer_decisions"]
        assert same["voxel_keys"] and same["camera"] and same["lidar"], rep
        assert rep["capacity_binds"] or (same["pooled"] and rep["criterion_a"]), rep
        # (measured equal; asserted to within the unmatched-box allowance of (a): a box at the edge of IoU 0.99 may fall either way)
        assert abs(rep["matched_iou99_dscore1e3"] - rep["oracle_swapped_agreement"]) <= E2E_MAX_UNMATCHED, rep
    for i, rep in enumerate(report["disjoint_pair"]):
        assert 0 < rep["pooled_pairs"] < ctx.model.roi_extractor.max_all_pts
        assert all(rep["same_integer_decisions"].values()) and rep["criterion_a"], rep
        np.testing.assert_array_equal(np.sort(yx[1 - i][2]), np.sort(xy[i][2]))  # labels


def test_a_sample_in_a_batch_against_the_same_sample_alone(ctx, ab):
    """[A, B][i] against [A] / [B] alone: everything upstream of the clustering is the sample's own (voxel keys, camera-query
    partition); the LiDAR partition is the batch's by the reference's rule, so its difference is recorded, and asserted to be exactly
    the oracle's: the oracle's single-sample and batch partitions differ in the same way."""
    got, cap = ab
    st = structure(ctx.model, cap, 2)
    report = dict(per_sample=[])
    for i, s in enumerate((ctx.a, ctx.b)):
        alone, cap1 = run(ctx.model, [s], ctx.device)
        st1 = structure(ctx.model, cap1, 1)[0]
        same = same_structure(st[i], st1)
        o_batch = lidar_partition(ctx.model, ctx.truth[i]["s3"]["pts_cluster_inds"], ctx.truth[i]["s3"]["points"])
        report["per_sample"].append(dict(same_integer_decisions=same, lidar_queries_in_batch=len(st[i]["lidar"]), lidar_queries_alone=len(st1["lidar"]),
                                         batch_lidar_partition_is_the_oracles=bool(st[i]["lidar"] == o_batch),
                                         boxes_alone=int(alone[0][0].shape[0])))
        assert same["voxel_keys"] and same["camera"], same
        assert st[i]["lidar"] == o_batch
        assert len(st[i]["lidar"]) <= len(st1["lidar"])
    write_report("a_b_vs_alone", report)


def test_a_batch_that_decides_nothing_jointly_is_isolated(ctx):
    """Two samples on opposite sides of the car: the oracle certifies (CPU, stages 1-3) that no batch-wide rule changes anything, so on
    the device every integer decision of [X, Y][i] is that of [X] / [Y] alone — voxel keys, camera and LiDAR query partitions, RoI
    membership (a pair may differ only where the point sits within 1e-5 of a box face: the pooling tolerance of
    tests/test_fullsize_gpu.py) — labels equal, boxes one-to-one under (a).  Bit-identity of the floats is recorded, not asserted:
    fp32 means are summed in position-dependent chunks."""
    x, y = disjoint_pair(ctx)
    with torch.no_grad():
        o = omod.simple_test_batch(ctx.cpu, [x, y], only=[])
        s1 = [omod.fsf_stage1(ctx.cpu, *s) for s in (x, y)]
        rules = omod.fsf_stage3_batch(ctx.cpu, [s1[0], dict(s1[1], batch_idx=torch.ones_like(s1[1]["batch_idx"]))])[0]["rules"]
        singles = [omod.fsf_stage3(ctx.cpu, s)["rules"] for s in s1]
    assert o == [None, None] and sum(rules["bridged"]) == 0
    assert all(s["forced_first"] == rules["forced_first"] and s["inverted"] == rules["inverted"] for s in singles)
    got, cap = run(ctx.model, [x, y], ctx.device)
    st = structure(ctx.model, cap, 2)
    report = dict(per_sample=[])
    for i, s in enumerate((x, y)):
        alone, cap1 = run(ctx.model, [s], ctx.device)
        st1 = structure(ctx.model, cap1, 1)[0]
        same = same_structure(st[i], st1)
        diff = st[i]["pooled"] ^ st1["pooled"]
        near_ok = True
        if diff:  # only then: the oracle's margins of this sample's RoIs (1-3 s)
            p_batch, rois, _, _ = cap1["roi"]
            ext = ctx.model.roi_extractor
            near = orefine.dynamic_point_pool(rois[:, 1:8].numpy(), s[0][:, :3].numpy(), ext.extra_wlh, ext.max_inbox_point, ext.max_all_pts,
                                              return_margin=True, near_tol=1e-5)[3]
            near_pts = {int(p) for p in near[:, 1]}
            near_ok = all(p in near_pts for _, p in diff)
        ok, rep = bc.criterion_a(got[i], alone[0])
        rep.update(same_integer_decisions=same, pooled_pairs_that_differ=len(diff), criterion_a=ok, bitwise_equal=dict(
            boxes=bool(np.array_equal(got[i][0], alone[0][0])), scores=bool(np.array_equal(got[i][1], alone[0][1]))))
        report["per_sample"].append(rep)
        assert same["voxel_keys"] and same["camera"] and same["lidar"], same
        assert near_ok, (len(diff), rep)
        assert ok, rep
        np.testing.assert_array_equal(np.sort(got[i][2]), np.sort(alone[0][2]))
    write_report("isolation_disjoint_pair", report)


# ------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("middle", ["zeroed_masks", "points_300"])
def test_three_samples_with_an_empty_one_in_the_middle(ctx, middle):
    mid = bc.degenerate_samples(ctx.a)[middle]
    samples = [ctx.a, mid, ctx.b]
    with torch.no_grad():
        oracle = omod.simple_test_batch(ctx.cpu, samples)
    # the middle sample has no point inside a mask; inside a batch that has camera points it gets NO camera query (no fake object)
    assert int((oracle[1]["s1"]["obj_id"] > 0).sum()) == 0 and oracle[1]["s2"]["obj_coors"].shape[0] == 0 and not oracle[1]["s2"]["fake"]
    for i in (0, 2):
        assert oracle[i]["margin"] > bc.NEAR_THRESHOLD_MARGIN and oracle[i]["s2"]["obj_coors"].shape[0] > 0 and oracle[i]["s3"]["cluster_inds"].shape[0] > 0
    got, cap = run(ctx.model, samples, ctx.device)
    assert len(got) == 3
    rep = assert_batch_vs_oracle(f"a_{middle}_b", got, cap, oracle, full=(0, 2))
    which, margin = restarted_tail_rule(ctx.model, cap, got[1], sample=1)
    # (e)'s rule for the middle one: few boxes, so every one of them has to be the oracle's
    assert got[1][0].shape[0] == oracle[1]["boxes"].shape[0]
    assert rep["per_sample"][1]["matched_iou99_dscore1e3"] == oracle[1]["boxes"].shape[0], rep["per_sample"][1]
    assert which == "exact" or margin <= bc.NEAR_THRESHOLD_MARGIN


# ------------------------------------------------------------------------------------------------ (e)
def _degenerate(ctx, name):
    if name == "under_every_threshold":
        return (ctx.a[0][:5000].contiguous(),) + tuple(ctx.a[1:])
    return bc.degenerate_samples(ctx.a)[name]


@pytest.mark.parametrize("name", ["zeroed_masks", "points_300", "one_point", "masks_in_the_sky", "under_every_threshold"])
def test_a_degenerate_frame_against_the_oracle(ctx, name):
    s = _degenerate(ctx, name)
    forced = name == "under_every_threshold"
    ng = len(ctx.cpu.cfg["group_names"])
    with (bc.background_only(ctx.cpu, ctx.model) if forced else contextlib.nullcontext()):
        with torch.no_grad():
            o = omod.simple_test(ctx.cpu, *s)
        # the branch the case is named for, on the oracle's intermediates
        if forced:  # no pre-voxel above any threshold: the forced first pre-voxel, the inverted density mask, one query per group
            assert all(o["s3"]["rules"]["forced_first"]) and all(o["s3"]["rules"]["inverted"]) and o["s3"]["cluster_inds"].shape[0] == ng
        else:       # no point inside any mask: the fake camera query
            assert int((o["s1"]["obj_id"] > 0).sum()) == 0 and o["s2"]["fake"] and o["s2"]["obj_coors"].tolist() == [[0, 0, 0]]
        if name == "masks_in_the_sky":
            assert int((s[1] > 0).sum()) > 0
        if name == "one_point":
            assert all(o["s3"]["rules"]["inverted"]) and o["s3"]["points"].shape[0] == ng
        got, cap = run(ctx.model, [s], ctx.device)
        hot, _ = run(ctx.model, [s], ctx.device, hot_path_only=True)
    keys = keys_vs_oracle(cap, [o])
    ok, rep = bc.criterion_a(got[0], bc.oracle_result(o))
    which, margin = restarted_tail_rule(ctx.model, cap, got[0])
    rep.update(query_keys=keys, oracle_nms_margin=float(o["margin"]), restarted_tail=which, restarted_tail_margin=margin,
               pooled_points=o["pooled_points"], rules=o["s3"]["rules"])
    write_report(f"degenerate_{name}", rep)
    assert keys["camera"]["keys_identical"] and keys["lidar"]["keys_identical"], keys
    assert min(margin, o["margin"]) > bc.NEAR_THRESHOLD_MARGIN  # (the near-threshold escape is taken by none of these cases)
    assert which == "exact"
    # un-restarted: every box the device returns is the oracle chain's (the per-box thresholds of (a); a few boxes, so all of them)
    assert rep["boxes"] == rep["oracle_boxes"] == rep["matched_iou99_dscore1e3"], rep
    # hot_path_only: the documented widths, the oracle's keys
    n_cam, n_lid = o["s2"]["obj_coors"].shape[0], o["s3"]["cluster_inds"].shape[0]
    assert torch.equal(hot["frustum_obj_coors"], o["s2"]["obj_coors"].to(hot["frustum_obj_coors"].dtype))
    assert torch.equal(hot["fsd_obj_coors"], o["s3"]["cluster_inds"].to(hot["fsd_obj_coors"].dtype))
    assert hot["frustum_obj_feats"].shape == (n_cam, ctx.model.lidar_img_input_dim) and hot["frustum_obj_centers"].shape == (n_cam, 3)
    assert hot["frustum_preds_2d"].shape == (n_cam, 9) and torch.equal(hot["frustum_preds_2d"], o["s2"]["preds_2d"])
    assert hot["fsd_obj_feats"].shape == (n_lid, ctx.model.lidar_input_dim) and hot["fsd_obj_centers"].shape == (n_lid, 3)


def test_no_pooled_point_gives_the_fake_row_with_a_readable_index(ctx):
    """RoIs that hold no point: the extractor returns the reference's one fake row.  Its RoI index is -1 (the head drops that group); its
    point index names the last point — what index -1 reads — as a non-negative index, because the native row gathers take indices as they
    are."""
    from fullysparsefusion_amd import hip_ops

    pts = ctx.a[0][:1000, :3].to(ctx.device).contiguous()
    rois = torch.tensor([[0, 500.0, 500.0, 0.0, 2.0, 4.0, 1.5, 0.3], [0, -500.0, 500.0, 0.0, 2.0, 4.0, 1.5, 0.0]], device=ctx.device)
    inds, roi_inds, info = ctx.model.roi_extractor(pts, torch.zeros(1000, dtype=torch.int64, device=ctx.device), rois)
    assert inds.tolist() == [999] and roi_inds.tolist() == [-1] and not roi_inds._fsf_real_rows
    assert float(info["local_xyz"].abs().sum()) == 0.0
    assert torch.equal(hip_ops.gather_rows(pts, inds), pts[-1:])


def pooling_case():
    """Two samples of 1 500 points each, four RoIs each, INTERLEAVED in the RoI list as the (camera, LiDAR) query order interleaves them,
    with a capacity (120 rows per sample) that binds in both samples."""
    rng = np.random.default_rng(5)
    pts = rng.uniform(-6, 6, (3000, 3)).astype(np.float32)
    pts[:, 2] = rng.uniform(-1, 1, 3000)
    batch = np.repeat([0, 1], 1500)
    boxes = np.array([[-3, -3, -1, 3.0, 4.0, 2.0, 0.3], [3, 3, -1, 2.5, 3.5, 2.0, -0.7], [0, 0, -1, 4.0, 4.0, 2.0, 1.1], [3, -3, -1, 3.0, 3.0, 2.0, 0.0]],
                     dtype=np.float32)
    rois = np.concatenate([np.array([0, 1, 1, 0, 0, 1, 1, 0], np.float32)[:, None], np.concatenate([boxes, boxes[::-1]])], 1)
    return pts, batch, rois


def test_the_pooling_capacity_is_per_sample(ctx):
    """`max_all_pts` is the pooling op's capacity per call, i.e. per sample (ops/dynamic_point_pool_op.py:27-29 under the per-sample loop of
    dynamic_point_roi_extractor.py:45-59).  Found by (a): one launch over the batch shared one capacity in RoI order, so the later RoIs of
    both samples lost their points whenever the batch pooled more than one sample's capacity (A alone pools 79 767 rows against 50 000)."""
    from fullysparsefusion_amd import mmdet3d_plugin as plugin

    pts, batch, rois = pooling_case()
    cap = 120
    ext = plugin.registry.build_roi_extractor(dict(type="DynamicPointROIExtractor", extra_wlh=[0.5, 0.5, 0.5], max_inbox_point=64, max_all_pts=cap))
    want, feats = [], []
    for b in (0, 1):
        r_idx, p_idx = np.nonzero(rois[:, 0] == b)[0], np.nonzero(batch == b)[0]
        wp, wr, wf, near = orefine.dynamic_point_pool(rois[r_idx, 1:], pts[p_idx], ext.extra_wlh, ext.max_inbox_point, cap, return_margin=True,
                                                      near_tol=1e-4)
        assert len(near) == 0 and len(wp) == cap  # (no point within 1e-4 of a face: membership is not a rounding question; the cap binds)
        want += [(int(r_idx[r]), int(p_idx[p])) for p, r in zip(wp, wr)]
        feats.append(wf)
    dev = ctx.device
    for batch_size in (2, None):  # told by the caller / read from the batch column
        inds, roi_inds, info = ext(torch.from_numpy(pts).to(dev), torch.from_numpy(batch).to(dev), torch.from_numpy(rois).to(dev), batch_size=batch_size)
        got = list(zip(roi_inds.tolist(), inds.tolist()))
        assert got == sorted(want)  # ascending (RoI, point), every sample's own first `cap` rows
        assert roi_inds._fsf_real_rows and roi_inds._fsf_sorted
        order = np.lexsort((np.array(want)[:, 1], np.array(want)[:, 0]))
        np.testing.assert_allclose(info["local_xyz"].cpu().numpy(), np.concatenate(feats)[order][:, 3:6], atol=1e-5)  # (tolerance of _compare_pool)


# ------------------------------------------------------------------------------------------------ (f)
def test_an_announced_batch_is_declined_and_changes_nothing(ctx, ab):
    """`set_next_frame` with a two-sample batch: the frame front is a one-sample path and declines (fsf.py `_prefetch_front`); the
    announced call returns the plain result bit for bit and nothing stays queued."""
    got, _ = ab
    model = ctx.model
    args = dev_args([ctx.a, ctx.b], ctx.device)
    with torch.no_grad():
        model.set_next_frame(*args)
        first = [bc.device_result(r) for r in model.simple_test(*args)]  # (its tail fires the prefetch of the announced batch: declined)
        assert model._front_ready is None and "_next_frame" not in model.__dict__
        second = [bc.device_result(r) for r in model.simple_test(*args)]
        assert model._front_ready is None and "_next_frame" not in model.__dict__
    for res in (first, second):
        for g, w in zip(res, got):
            for x, y in zip(g, w):
                np.testing.assert_array_equal(x, y)
