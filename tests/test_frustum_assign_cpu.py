"""The refine-stage heads' frustum + distance assignment on the host (the restatement K38 is checked against).

`frustum_targets_host` against an independent transcription written here: K37's transcription of the 3-D / 2-D steps
(tests/test_hybrid_assign_cpu.py) followed by a float64 per-class loop over `torch.cdist`, as upstream's DistAssigner walks its assign
tasks.  Assignment and source must be equal for every query the transcription does not call marginal: its minimum distance within
2e-3 m of the radius, or its two nearest same-class GT within 2e-3 m of each other (about twice the deviation of cdist's matmul form
from the direct form on +-51.2 m coordinates, docs/kernels/K38_frustum_assign.md), or marginal in K37's sense; at most 1 % of the
queries, asserted.  Then the targeted cases with the expected rows written out, the refusals, the configs, the detector's public
surface and the static guard-band check."""
import ast
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from fullysparsefusion_amd.compat import Config
from fullysparsefusion_amd.mmdet3d_plugin import build_model
from fullysparsefusion_amd.mmdet3d_plugin.core.assigners import DistAssigner, FrustumAssigner, HybridAssigner, gt_boxes_2d_host
from fullysparsefusion_amd.mmdet3d_plugin.models.dense_heads.cluster_heads import frustum_targets_host, hybrid_targets_host
from test_cluster_losses_cpu import NUS_CLASSES, make_head, reference_losses_f64
from test_hybrid_assign_cpu import ASSIGNER_CFG, LOSS_NAMES, frame_case, loss_case, make_assigner, regroup, targeted_cases, transcribed_assign

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
# the nuScenes config's radii (reference FSF_nuScenes_config.py:343-360), by class name
RADII = dict(car=1.0, truck=1.0, trailer=2.0, bus=4.0, construction_vehicle=0.5, bicycle=0.5, motorcycle=0.5, pedestrian=0.5,
             traffic_cone=0.5, barrier=0.0)
ASSIGN_ORDER = ["car", "truck", "trailer", "bus", "construction_vehicle", "bicycle", "motorcycle", "pedestrian", "traffic_cone", "barrier"]


def dist_cfg(names=ASSIGN_ORDER, class_names=NUS_CLASSES, radii=RADII):
    return dict(type="DistAssigner", assign_tasks=[dict(num_class=1, class_names=[n]) for n in names],
                max_dist=[[radii[n]] for n in names], class_names=list(class_names))


FRUSTUM_CFG = dict(ASSIGNER_CFG, type="FrustumAssigner", assigner_dist=dist_cfg())
C = len(NUS_CLASSES)
CLS = {name: i for i, name in enumerate(NUS_CLASSES)}


def make_frustum_assigner(**extra):
    cfg = {k: v for k, v in FRUSTUM_CFG.items() if k != "type"}
    cfg.update(extra)
    return FrustumAssigner(**cfg)


def make_refine_head(**extra):
    kw = dict(head_type="FrustumClusterHead", train_cfg=dict(), test_cfg=dict(), assigner=dict(FRUSTUM_CFG))
    kw.update(extra)
    return make_head(**kw)


def regroup_keep(boxes, labels):
    """The rows in the task's order with the rows of label < 0 LAST (what modify_gt_for_single_task leaves of device-resident GT)."""
    boxes, labels = np.asarray(boxes), np.asarray(labels, np.int64)
    order = np.argsort(np.where(labels < 0, C, labels), kind="stable")
    return boxes[order], labels[order]


def host_targets(assigner, centres, bidx, preds, na_list, aug_list, l2i, old, code=10, parts=False, fn=frustum_targets_host):
    """frustum_targets_host on per-sample (boxes, labels) pairs that are NOT yet in the task's order (rows of label < 0 kept, last)."""
    na = [regroup_keep(b, l) for b, l in na_list]
    au = [regroup_keep(b, l) for b, l in aug_list]
    extra = dict(old_cls_logits=torch.from_numpy(old)) if fn is frustum_targets_host and old is not None else {}
    return fn(assigner, torch.from_numpy(centres), torch.from_numpy(bidx), torch.from_numpy(preds),
              [torch.from_numpy(b) for b, _ in na], [torch.from_numpy(l) for _, l in na],
              [torch.from_numpy(b) for b, _ in au], [torch.from_numpy(l) for _, l in au],
              torch.from_numpy(np.asarray(l2i, np.float64)).float(), C, code, return_parts=parts, **extra)


def source_of(parts, bidx):
    src = np.zeros(len(bidx), np.int64)
    for b, part in enumerate(parts):
        if part is not None:
            src[np.flatnonzero(bidx == b)] = part["source"].numpy()
    return src


# ------------------------------------------------------------------------------------------------ the transcription (float64, cdist)
def transcribed_dist_assign(centres, logits, gt_rows, gt_labels, margin=2e-3):
    """DistAssigner.assign for one sample, GT in the task's order with task labels = global class indices: per assign task the
    queries whose arg-max class is the task's, the GT of that class, cdist, minimum, negated on >=.  -> (rows or -1, marginal)."""
    n = len(centres)
    out, marginal = np.full(n, -1, np.int64), np.zeros(n, bool)
    pred = np.asarray(logits).argmax(1) if n else np.zeros(0, np.int64)
    gt_rows = np.asarray(gt_rows, np.float64)
    q, g = torch.from_numpy(np.asarray(centres, np.float64)[:, :2]), torch.from_numpy(gt_rows[:, :2] if len(gt_rows) else np.zeros((0, 2)))
    for name in ASSIGN_ORDER:
        cid, radius = CLS[name], float(F32(RADII[name]))
        gi, qi = np.flatnonzero(np.asarray(gt_labels) == cid), np.flatnonzero(pred == cid)
        if len(gi) == 0 or len(qi) == 0:
            continue
        d = torch.cdist(q[qi][None], g[gi][None])[0].numpy()
        for row, i in enumerate(qi):
            j = int(d[row].argmin())
            if not d[row, j] >= radius:
                out[i] = gi[j]
            srt = np.sort(d[row])
            marginal[i] = abs(srt[0] - radius) < margin or (len(srt) > 1 and srt[1] - srt[0] < margin)
    return out, marginal


def frustum_frame_case(seed, box_dim=9):
    """K37's frame (tests/test_hybrid_assign_cpu.py::frame_case) with 60 of the centres that sit in no box moved next to a GT centre,
    up to twice its class radius away and above the box, and synthetic previous-stage logits that name that GT's class for most of them."""
    boxes, labels, aug, l2i, preds, centres = frame_case(seed, box_dim)
    rng = np.random.default_rng(seed + 900)
    ra, rl = regroup(aug, labels)
    n = len(centres)
    old = rng.normal(0.0, 1.0, (n, C)).astype(F32)
    outside = np.flatnonzero(centres[:, 2] == F32(30.0))
    for i in rng.choice(outside, 60, replace=False):
        k = int(rng.integers(len(ra)))
        c = int(rl[k])
        r = max(RADII[NUS_CLASSES[c]], 0.5) * rng.uniform(0.0, 2.0)
        th = rng.uniform(0.0, 2 * np.pi)
        centres[i, :2] = ra[k, :2] + (r * np.array([np.cos(th), np.sin(th)])).astype(F32)
        if rng.random() < 0.8:
            old[i, c] = 6.0
    return boxes, labels, aug, l2i, preds, centres, old


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_host_restatement_equals_the_transcription_on_a_frame(seed):
    boxes, labels, aug, l2i, preds, centres, old = frustum_frame_case(seed)
    n = len(centres)
    bidx = np.zeros(n, np.int64)
    out = host_targets(make_frustum_assigner(), centres, bidx, preds, [(boxes, labels)], [(aug, labels)], l2i[None], old, parts=True)
    part = out[-1][0]
    rb, _ = regroup(boxes, labels)
    ra, rl = regroup(aug, labels)
    hybrid, rows_3d, rows_2d, marg_h = transcribed_assign(preds, centres, rb, ra, l2i.astype(F32))
    rows_d, marg_d = transcribed_dist_assign(centres, old, ra, rl)
    final = np.where(hybrid >= 0, hybrid, rows_d)
    source = np.where(rows_3d >= 0, 1, np.where(rows_2d >= 0, 2, np.where(rows_d >= 0, 3, 0)))
    marginal = marg_h | ((hybrid < 0) & marg_d)
    counts = [int((source == k).sum()) for k in range(4)]
    print(f"K38 seed {seed}: n = {n}, GT rows {len(ra)}, none / 3-D / 2-D / distance {counts}, marginal {int(marginal.sum())} "
          f"(share {marginal.mean():.4f}; distance-marginal {int(((hybrid < 0) & marg_d).sum())})")
    assert marginal.mean() <= 0.01
    ok = ~marginal
    assert np.array_equal(out[4].numpy()[ok], final[ok])
    assert np.array_equal(part["source"].numpy()[ok], source[ok])
    assert np.array_equal(part["rows_3d"].numpy(), rows_3d) and np.array_equal(part["rows_dist"].numpy()[ok & (hybrid < 0)], rows_d[ok & (hybrid < 0)])
    assert counts[3] >= 5 and counts[1] >= 1 and counts[2] >= 1
    lab = out[0].numpy()
    assert np.array_equal(lab[ok], np.where(final >= 0, rl[np.maximum(final, 0)], C)[ok])
    pos = np.flatnonzero(ok & (source == 3))
    assert np.array_equal(out[2].numpy()[pos, :3], (ra[final[pos], :3] - centres[pos]).astype(F32))
    assert float(out[5][2]) == len(ra) and float(out[5][1]) == int((out[4] >= 0).sum())


def test_without_an_assigner_dist_the_result_is_the_hybrid_one():
    boxes, labels, aug, l2i, preds, centres, old = frustum_frame_case(3)
    bidx = np.zeros(len(centres), np.int64)
    args = (centres, bidx, preds, [(boxes, labels)], [(aug, labels)], l2i[None])
    want = host_targets(make_assigner(), *args, None, fn=hybrid_targets_host)
    got = host_targets(make_frustum_assigner(assigner_dist=None), *args, old, parts=True)
    for a, b in zip(got[:6], want):
        assert torch.equal(a, b)
    assert set(np.unique(got[-1][0]["source"].numpy())) == {0, 1, 2} and int((got[-1][0]["rows_dist"] >= 0).sum()) == 0
    with_dist = host_targets(make_frustum_assigner(), *args, old)
    assert int((with_dist[4] >= 0).sum()) > int((want[4] >= 0).sum())


# ------------------------------------------------------------------------------------------------ targeted cases
def rounded_root(s):
    """The correctly rounded f32 root of an f32: the float64 root (correctly rounded, 53 >= 2 * 24 + 2 bits) rounded once more."""
    return F32(np.sqrt(np.float64(F32(s))))


def xy_with_square_sum(s):
    """f32 (x, y) with fl(fl(x x) + fl(y y)) == s exactly, found by a walk over x from 0.3 in steps of 64 ulps."""
    s = F32(s)
    x = F32(0.3)
    for _ in range(20000):
        y0 = F32(np.sqrt(np.float64(s) - np.float64(x) ** 2))
        for y in (y0, np.nextafter(y0, F32(0.0)), np.nextafter(y0, F32(1.0))):
            if F32(F32(x * x) + F32(y * y)) == s:
                return np.array([x, y], F32)
        x = F32(x + F32(64 * 2.0 ** -25))
    raise AssertionError(f"no f32 pair squares and sums to {s!r}")


def neighbouring_squares(same_root):
    """The largest f32 s < 0.2 whose correctly rounded root equals (same_root) or exceeds (not same_root) that of the f32 below it."""
    s = F32(0.2)
    while (rounded_root(s) == rounded_root(np.nextafter(s, F32(0.0)))) != same_root:
        s = np.nextafter(s, F32(0.0))
    assert rounded_root(s) < F32(0.5)
    return s


def frustum_targeted_cases():
    """name -> dict(centres, bidx, preds, old, na, aug, l2i, expect = assigned rows, source, assigner = extra FrustumAssigner kwargs)."""
    cases = {}
    base = targeted_cases()
    l2i = base["no_gt"]["l2i"]
    nowhere = [1500.0, 800.0, 1510.0, 810.0, 0.9, 0, 0, 0, 1]  # a 2-D box that overlaps no projection
    box = lambda x, y, w=2.0, l=4.0, yaw=0.0, flag=None: [x, y, -1.0, w, l, 1.6, yaw, 0.5, -0.5] + ([] if flag is None else [flag])  # noqa: E731

    def logits(*classes):
        rows = np.full((len(classes), C), -2.0, F32)
        for i, names in enumerate(classes):
            for name in ([names] if isinstance(names, str) else names):
                rows[i, CLS[name]] = 3.0
        return rows

    def case(name, centres, old, gt, labels, expect, source, preds=None, bidx=None, l2i_=l2i, assigner=None, gts=None):
        n = len(centres)
        gts = [(gt, labels)] if gts is None else gts
        lists = [(np.array(b, F32).reshape(len(l), -1) if len(l) else np.zeros((0, 9), F32), np.array(l, np.int64)) for b, l in gts]
        cases[name] = dict(centres=np.array(centres, F32).reshape(n, 3), preds=np.array(preds if preds is not None else [nowhere] * n, F32).reshape(n, 9),
                           old=old, na=[(b[:, :9], l) for b, l in lists], aug=lists, l2i=l2i_, bidx=np.zeros(n, np.int64) if bidx is None else np.array(bidx, np.int64),
                           expect=expect, source=source, assigner=assigner or {})

    # 1. the centre above the box top, xy inside: 3-D misses, the distance step assigns
    case("above_the_box", [[10.3, 20.0, 5.0]], logits("car"), [box(10.0, 20.0)], [CLS["car"]], [0], [3])
    # 2. inside GT A (row 0) while GT B (row 1, a small box) is nearer in BEV: 3-D wins
    case("3d_hit_while_another_gt_is_nearer", [[11.8, 20.0, 0.0]], logits("car"), [box(10.0, 20.0), box(12.3, 20.0, w=0.5, l=0.5)],
         [CLS["car"]] * 2, [0], [1])
    # 3. the 2-D box sits on GT 1's projection while the centre is above GT 0's centre: 2-D wins over distance
    c3 = base["3d_beats_2d"]
    case("2d_hit_wins_over_distance", [[12.0, 4.0, 50.0]], logits("car"), c3["aug"][0][0], [CLS["car"]] * 2, [1], [2], preds=[c3["preds"][1]],
         l2i_=c3["l2i"])
    # 4. d == max_dist exactly is not assigned (bicycle: 0.5); one ulp below it is
    below = float(np.nextafter(F32(10.5), F32(0.0)))
    case("exactly_the_radius", [[10.5, 20.0, 50.0], [below, 20.0, 50.0]], logits("bicycle", "bicycle"), [box(10.0, 20.0, w=0.6, l=1.8)],
         [CLS["bicycle"]], [-1, 0], [0, 3])
    # 5. barrier: radius 0, never assigned, not even at d = 0
    case("barrier_never", [[10.0, 20.0, 50.0]], logits("barrier"), [box(10.0, 20.0)], [CLS["barrier"]], [-1], [0])
    # 6. the arg-max class differs from the only near GT's class
    case("other_class_predicted", [[10.2, 20.0, 50.0]], logits("truck"), [box(10.0, 20.0)], [CLS["car"]], [-1], [0])
    # 7. a tie in the logits goes to the lowest class: car (0) and truck (1) tie, the car is taken although the truck is nearer
    case("logit_tie_lowest_class", [[10.0, 20.0, 50.0]], logits(["car", "truck"]), [box(10.5, 20.0), box(10.2, 20.0)], [CLS["car"], CLS["truck"]],
         [0], [3])
    # 8. two cars at the same distance: the first in task order
    case("equidistant_first_row", [[10.0, 20.0, 50.0]], logits("car"), [box(10.5, 20.0), box(9.5, 20.0)], [CLS["car"]] * 2, [0], [3])
    # 9. the nearest car is in the OTHER sample of the batch
    case("other_sample_ignored", [[10.0, 20.0, 50.0], [10.0, 20.0, 50.0]], logits("car", "car"), None, None, [-1, 0], [0, 3], bidx=[0, 1],
         l2i_=np.concatenate([l2i, l2i]), gts=[([box(30.0, 30.0)], [CLS["car"]]), ([box(10.0, 20.0)], [CLS["car"]])])
    # 10. a row of label -1 is skipped although it is nearest
    case("unlabelled_row_skipped", [[10.0, 20.0, 50.0]], logits("car"), [box(10.0, 20.0), box(10.6, 20.0)], [-1, CLS["car"]], [0], [3])
    # 11. a class that no assign task names never assigns
    case("class_in_no_assign_task", [[10.0, 20.0, 50.0], [30.0, 5.0, 50.0]], logits("car", "truck"), [box(10.0, 20.0), box(30.2, 5.0)],
         [CLS["car"], CLS["truck"]], [-1, 1], [0, 3], assigner=dict(assigner_dist=dist_cfg([n for n in ASSIGN_ORDER if n != "car"])))
    # 12. the copy-paste flag (column 9) of the assigned box switches the velocity weights of a distance-assigned query
    case("copy_paste_flag", [[10.0, 20.0, 50.0], [30.0, 5.0, 50.0]], logits("car", "car"), [box(10.0, 20.0, flag=0.0), box(30.2, 5.0, flag=1.0)],
         [CLS["car"]] * 2, [0, 1], [3, 3])
    # the root is the correctly rounded one.  s = fl(fl(dx dx) + fl(dy dy)) one f32 below 0.25 has the exact root 0.5 - 2^-26 - 2^-52...,
    # a hair under the midpoint of [0.5 - 2^-25, 0.5]: it rounds DOWN, below the bicycle's radius 0.5, and is assigned; a root one ulp
    # high reaches the radius.  s one f32 above 0.25 has the root 0.5 + 2^-25 - ..., a hair under the midpoint of [0.5, 0.5 + 2^-24]: it
    # rounds to 0.5 and is not assigned; a root one ulp low would be.  (The query is the origin, so dx, dy are the GT's coordinates.)
    s_below, s_above = np.nextafter(F32(0.25), F32(0.0)), np.nextafter(F32(0.25), F32(1.0))
    assert rounded_root(s_below) == np.nextafter(F32(0.5), F32(0.0)) and rounded_root(s_above) == F32(0.5)
    bike = lambda xy: box(float(xy[0]), float(xy[1]), w=0.6, l=1.8)  # noqa: E731
    case("rounding_root_just_below_the_radius", [[0.0, 0.0, 50.0]], logits("bicycle"), [bike(xy_with_square_sum(s_below))], [CLS["bicycle"]], [0], [3])
    case("rounding_root_rounds_to_the_radius", [[0.0, 0.0, 50.0]], logits("bicycle"), [bike(xy_with_square_sum(s_above))], [CLS["bicycle"]], [-1], [0])
    # two bicycles whose s differ by one f32 step.  Where both roots round to the same f32 the first row stays (strict <) although the
    # second is nearer in exact arithmetic; where the rounded roots differ the second row wins.
    s_tie, s_step = neighbouring_squares(same_root=True), neighbouring_squares(same_root=False)
    for name, s_hi, expect in (("rounding_equal_rounded_roots_first_row", s_tie, 0), ("rounding_smaller_rounded_root_wins", s_step, 1)):
        s_lo = np.nextafter(s_hi, F32(0.0))
        case(name, [[0.0, 0.0, 50.0]], logits("bicycle"), [bike(xy_with_square_sum(s_hi)), bike(-xy_with_square_sum(s_lo))],
             [CLS["bicycle"]] * 2, [expect], [3])
    # a row of NaN logits is class 0; NaN coordinates leave the query background
    nan = logits("car", "car")
    nan[0, :] = np.nan
    case("nan_logits_and_nan_centre", [[10.0, 20.0, 50.0], [np.nan, 20.0, 50.0]], nan, [box(10.0, 20.0)], [CLS["car"]], [0, -1], [3, 0])
    return cases


def run_case(c, code=10):
    return host_targets(make_frustum_assigner(**c["assigner"]), c["centres"], c["bidx"], c["preds"], c["na"], c["aug"], c["l2i"], c["old"],
                        code=code, parts=True)


@pytest.mark.parametrize("name", sorted(frustum_targeted_cases()))
def test_targeted_case_on_the_host(name):
    c = frustum_targeted_cases()[name]
    out = run_case(c)
    assert out[4].tolist() == list(c["expect"]), (name, out[4].tolist())
    assert source_of(out[-1], c["bidx"]).tolist() == list(c["source"]), name
    if name == "copy_paste_flag":
        assert out[3][:, 8:].tolist() == [[0.0, 0.0], [1.0, 1.0]] and out[3][:, :8].eq(1).all()
    if "nan" not in name and not c["assigner"]:  # and the transcription agrees, sample by sample
        for b in range(len(c["aug"])):
            mine = np.flatnonzero(c["bidx"] == b)
            ra, rl = regroup(*c["aug"][b])
            hybrid, _, _, _ = transcribed_assign(c["preds"][mine], c["centres"][mine], regroup(*c["na"][b])[0], ra[:, :9], c["l2i"][b].astype(F32))
            rows_d, _ = transcribed_dist_assign(c["centres"][mine], c["old"][mine], ra[:, :9], rl, margin=0.0)
            if name != "exactly_the_radius" and not name.startswith("rounding_"):  # (cdist's own rounding decides a distance one ulp
                # from the radius or from another candidate's)
                assert np.where(hybrid >= 0, hybrid, rows_d).tolist() == [c["expect"][i] for i in mine], name


def test_dist_assigner_on_its_own_and_its_class_table():
    a = DistAssigner(**{k: v for k, v in dist_cfg().items() if k != "type"})
    assert not a.OUT_OF_SCOPE
    table = a.class_table(C)
    assert table.dtype == torch.float32 and table.tolist() == [RADII[n] for n in NUS_CLASSES]
    partial = DistAssigner(**{k: v for k, v in dist_cfg(["bus", "car"]).items() if k != "type"})
    assert partial.class_table(C).tolist() == [1.0, 0, 0, 4.0, 0, 0, 0, 0, 0, 0]
    gt = torch.tensor([[10.0, 20.0, -1, 2, 4, 1.6, 0, 0, 0], [13.0, 20.0, -1, 2, 4, 1.6, 0, 0, 0]])
    xyz = torch.tensor([[10.9, 20.0, 9.0], [12.9, 20.0, 9.0], [11.5, 20.0, 9.0]])
    z = torch.full((3, C), -1.0)
    z[:, 0] = 1.0
    assert a.assign_rows(xyz, z, gt, torch.tensor([0, 0])).tolist() == [0, 1, -1]
    res = a.assign(xyz, z, gt, torch.tensor([0, 0]))
    assert res.gt_inds.tolist() == [1, 2, 0] and res.num_gts == 2
    assert a.assign_rows(xyz, z, gt[:0], torch.zeros(0, dtype=torch.long)).tolist() == [-1, -1, -1]


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("option,assigner", [
    ("more than one class", dict(assigner_dist=dict(type="DistAssigner", assign_tasks=[dict(class_names=["car", "truck"])], max_dist=[[1.0, 1.0]],
                                                    class_names=NUS_CLASSES))),
    ("two assign_tasks", dict(assigner_dist=dist_cfg(["car", "bus", "car"]))),
    ("global class indices", dict(assigner_dist=dist_cfg(class_names=list(reversed(NUS_CLASSES))))),
    ("global class indices", dict(tasks=[dict(class_names=NUS_CLASSES[:5]), dict(class_names=NUS_CLASSES[5:])])),
    ("ignore_bev_dist", dict(ignore_bev_dist=2.0)),
    ("vis_dir", dict(vis_dir="pictures")),
    ("is_frustum", dict(is_frustum=True)),
    ("assigner_3d", dict(assigner_3d=None)),
    ("match_low_quality", dict(assigner_2d=dict(ASSIGNER_CFG["assigner_2d"], match_low_quality=False)))])
def test_what_is_not_built_is_refused_by_name(option, assigner):
    a = make_frustum_assigner(**assigner)
    assert a.OUT_OF_SCOPE
    with pytest.raises(NotImplementedError, match=option):
        a.check()
    head = make_refine_head(assigner=dict(FRUSTUM_CFG, **assigner))
    with pytest.raises(NotImplementedError, match=option):
        head.loss(None, None, None, None, None, None, None, None)


def test_a_head_whose_task_labels_are_not_global_indices_is_refused():
    head = make_refine_head(task_names=NUS_CLASSES[:4])
    with pytest.raises(NotImplementedError, match="global class indices"):
        head._check_loss_cfg()
    assert not make_refine_head().assigner.OUT_OF_SCOPE
    make_refine_head()._check_loss_cfg()


def test_bare_constructions_build_and_are_out_of_scope():
    """What tests/test_hybrid_assign_cpu.py pins: a FrustumAssigner without assigner_3d around a DistAssigner without arguments builds,
    says it is out of scope, and its head refuses before it looks at an argument."""
    bare = DistAssigner()
    assert bare.OUT_OF_SCOPE and bare.tasks is None
    with pytest.raises(NotImplementedError, match="assign_tasks"):
        bare.check()
    a = FrustumAssigner(num_cams=6, assigner_2d=dict(type="MaxIoUAssigner", pos_iou_thr=0.7, neg_iou_thr=0.3), assigner_dist=dict(type="DistAssigner"))
    assert a.OUT_OF_SCOPE and type(a.assigner_dist) is DistAssigner and isinstance(a, HybridAssigner)
    head = make_refine_head(assigner=dict(type="FrustumAssigner", num_cams=6, assigner_2d=dict(type="MaxIoUAssigner", pos_iou_thr=0.7, neg_iou_thr=0.3),
                                          assigner_dist=dict(type="DistAssigner")))
    with pytest.raises(NotImplementedError, match="FrustumClusterHead.loss: FrustumAssigner"):
        head.loss(None, None, None, None, None, None, None, None)
    hybrid = make_assigner(assigner_dist=dist_cfg())  # a HybridAssigner keeps refusing an assigner_dist
    with pytest.raises(NotImplementedError, match="assigner_dist"):
        hybrid.check()


# ------------------------------------------------------------------------------------------------ the head's loss on the host
def refine_loss_case(seed=3, box_dim=10):
    c = loss_case(seed, box_dim)
    boxes, labels, aug, l2i, preds, centres, old = frustum_frame_case(seed, box_dim)
    c.update(xyz=torch.from_numpy(centres), old=torch.from_numpy(old), raw=(boxes, labels, aug, l2i, preds, centres, old))
    return c


def refine_head_loss(head, c, z, r, fused, dev="cpu", **extra):
    put = lambda t: t.to(dev)  # noqa: E731
    return head.loss([z], [r], put(c["xyz"]), put(c["inds"]), c["na_b"], c["na_l"], c["gt_b"], c["gt_l"], put(c["preds"]), c["metas"],
                     None, [put(c["old"])], [r.detach()], fused=fused, **extra)


def test_unfused_loss_matches_float64_autograd_and_needs_the_old_logits():
    c = refine_loss_case()
    head = make_refine_head()
    z, r = c["z"].clone().requires_grad_(), c["r"].clone().requires_grad_()
    out = refine_head_loss(head, c, z, r, fused=False)
    names = LOSS_NAMES + ["num_preds", "num_pos_preds", "num_gts", "assigned_gts"]
    assert set(out) == {k + f"{NUS_CLASSES}" for k in names}
    got = {k: out[k + f"{NUS_CLASSES}"] for k in names}
    boxes, labels, aug, l2i, preds, centres, old = c["raw"]
    lab, _, tgt, wgt, asg, stats = host_targets(make_frustum_assigner(), centres, np.zeros(len(centres), np.int64), preds, [(boxes, labels)],
                                                [(aug, labels)], l2i[None], old)
    assert [float(got[k]) for k in names[5:]] == stats[:4].tolist()
    counts = head._last_assignment["source_counts"].tolist()
    assert sum(counts) == len(centres) and counts[3] >= 5 and counts[1] + counts[2] + counts[3] == int(stats[1])
    grads = [1.0, 0.7, 1.3, 0.9, 1.1]
    want, gz, gr = reference_losses_f64(c["z"], c["r"], lab, tgt, wgt, 4.0, 0.25, [1.0, 0.5, 0.5, 0.2, 0.2], True, grads)
    for k, w in zip(LOSS_NAMES, want):
        assert abs(float(got[k].detach()) - float(w)) <= 1e-5 * abs(float(w)), k
    sum(g * got[k] for g, k in zip(grads, LOSS_NAMES)).backward()
    assert float((z.grad.double() - gz).abs().max()) <= 1e-7 + 1e-5 * float(gz.abs().max())
    assert float((r.grad.double() - gr).abs().max()) <= 1e-7 + 1e-5 * float(gr.abs().max())
    with pytest.raises(ValueError, match="old_cls_logits"):
        head.loss([z], [r], c["xyz"], c["inds"], c["na_b"], c["na_l"], c["gt_b"], c["gt_l"], c["preds"], c["metas"], fused=False)
    no_dist = make_refine_head(assigner={k: v for k, v in FRUSTUM_CFG.items() if k != "assigner_dist"})  # no distance step: no old logits needed
    plain = no_dist.loss([z], [r], c["xyz"], c["inds"], c["na_b"], c["na_l"], c["gt_b"], c["gt_l"], c["preds"], c["metas"], fused=False)
    assert float(plain["num_pos_preds" + f"{NUS_CLASSES}"]) < float(got["num_pos_preds"])


# ------------------------------------------------------------------------------------------------ configs and the detector
@pytest.fixture(scope="module")
def nus_model():
    return build_model(Config.fromfile(os.path.join(ROOT, "configs", "fsf_nuscenes.py")).model)


def test_nuscenes_refined_head_has_the_reference_assigner(nus_model):
    from conftest import state_shapes_digest

    with open(os.path.join(ROOT, "tests", "golden", "reference_configs.json")) as f:
        golden = json.load(f)
    assert state_shapes_digest(nus_model) == (golden["nuscenes"]["state_dict_entries"], golden["nuscenes"]["state_dict_shapes"])
    for head in nus_model.frustum_refined_head:
        a = head.assigner
        assert type(a) is FrustumAssigner and not a.OUT_OF_SCOPE and type(a.assigner_dist) is DistAssigner
        head._check_loss_cfg()
        table = dict(zip(head.class_names, a.assigner_dist.class_table(len(head.class_names)).tolist()))
        assert table == RADII
        assert (a.assigner_2d.pos_iou_thr, a.assigner_2d.min_pos_iou, a.assigner_3d.extra_height, a.num_cams) == (0.7, 0.3, 0.0, 6)
    assert type(nus_model.frustum_obj_head.assigner) is HybridAssigner


def test_av2_refined_head_still_refuses_its_smooth_l1():
    from conftest import state_shapes_digest

    model = build_model(Config.fromfile(os.path.join(ROOT, "configs", "fsf_av2.py")).model)
    with open(os.path.join(ROOT, "tests", "golden", "reference_configs.json")) as f:
        golden = json.load(f)
    assert state_shapes_digest(model) == (golden["av2"]["state_dict_entries"], golden["av2"]["state_dict_shapes"])
    for head in model.frustum_refined_head:
        assert type(head.assigner) is FrustumAssigner and head.assigner.assigner_dist is None and not head.assigner.OUT_OF_SCOPE
        with pytest.raises(NotImplementedError, match="SmoothL1Loss"):
            head._check_loss_cfg()


def test_forward_train_graph_has_the_flag_and_forward_train_the_reference_signature(nus_model):
    model = nus_model
    sig = inspect.signature(model.forward_train_graph)
    assert sig.parameters["refine_head_losses"].default is False
    gt = ([torch.zeros((0, 9))], [torch.zeros(0, dtype=torch.long)])
    given = dict(gt_bboxes_3d=gt[0], gt_labels_3d=gt[1], no_aug_gt_bboxes_3d=gt[0], no_aug_gt_labels_3d=gt[1])
    for name in given:
        with pytest.raises(ValueError, match=r"refine_head_losses=True\) needs " + name):
            model.forward_train_graph(None, None, None, None, refine_head_losses=True, **{k: v for k, v in given.items() if k != name})
    assert list(inspect.signature(model.forward_train).parameters) == [
        "points", "img_metas", "no_aug_gt_bboxes_3d", "no_aug_gt_labels_3d", "gt_bboxes_3d", "gt_labels_3d", "mask_data", "mask_anno",
        "gt_bboxes_ignore", "img"]
    with pytest.raises(NotImplementedError, match="gt_bboxes_3d") as e:
        model.forward_train([torch.zeros((4, 8))], [dict()])
    assert "lidar_head_losses" in str(e.value) and "refine_head_losses" in str(e.value) and "no_aug_gt_labels_3d" in str(e.value)
    with pytest.raises(NotImplementedError, match="missing: gt_labels_3d"):
        model.forward_train([torch.zeros((4, 8))], [dict()], gt[0], gt[1], gt[0])


# ------------------------------------------------------------------------------------------------ C ABI surface and guard-band cover
def test_entry_points_are_declared_documented_and_the_abi_version_stays():
    from fullysparsefusion_amd import _lib

    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for name in ("fsf_frustum_assign", "fsf_frustum_assign_workspace_bytes"):
        assert name in _lib.SIGNATURES and name in doc, name
    assert _lib.DEFINES["FSF_ABI_VERSION"] == 23
    assert len(_lib.SIGNATURES["fsf_frustum_assign"][0]) == 37 and len(_lib.SIGNATURES["fsf_hybrid_assign"][0]) == 33
    # every input of fsf_hybrid_assign, in its order, up to min_pos_iou
    assert _lib.SIGNATURES["fsf_frustum_assign"][0][:25] == _lib.SIGNATURES["fsf_hybrid_assign"][0][:25]


_ALLOCATES = re.compile(r"torch\.empty|empty_like|torch\.zeros|torch\.full|_lib\.workspace\(|_workspace_bytes|_arena_bytes")
_SCRATCH = re.compile(r"_lib\.workspace\(|_workspace_bytes|_arena_bytes")


def test_every_allocating_wrapper_of_the_new_module_has_guard_band_cases():
    import test_guard_bands_frustum_gpu as gb
    from fullysparsefusion_amd import hip_ops_frustum

    with open(os.path.join(ROOT, "fullysparsefusion_amd", "hip_ops_frustum.py")) as f:
        src = f.read()
    alloc, scratch = set(), set()
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef):
            body = ast.get_source_segment(src, node)
            if _ALLOCATES.search(body):
                alloc.add(node.name)
                if _SCRATCH.search(body):
                    scratch.add(node.name)
    assert alloc == {"frustum_assign"} and scratch == {"frustum_assign"}
    assert sorted(alloc - set(gb.CASES)) == []
    for name, cases in gb.CASES.items():
        assert hasattr(hip_ops_frustum, name)
        kinds = [k for k, _ in cases]
        assert "ragged" in kinds and "minimal" in kinds and "empty" in kinds, name
    assert not re.search(r"torch\.zeros|torch\.full|empty_like|torch\.ones|new_zeros|new_empty|new_full", src)
