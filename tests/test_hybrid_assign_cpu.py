"""The camera-query head's hybrid 3-D / 2-D assignment on the host (the restatement K37 is checked against).

`hybrid_targets_host` against an independent transcription written here: a literal per-sample / per-camera / per-GT loop in float64
whose 2-D boxes come from scipy's `ConvexHull` + Sutherland-Hodgman clipping against the canvas (upstream: shapely's hull and
intersection), whose IoUs are float64 and whose MaxIoUAssigner is the published loop.  Assignments must be equal for every query that
the transcription itself does not call marginal (an IoU within 1e-5 of 0.3 / 0.7, or two candidates within 1e-6 of each other): at
most 1 % of the queries, asserted.  Then the targeted cases, the corners, the losses' public surface and the static guard-band check.

Loss tolerances are K36's (tests/test_cluster_losses_cpu.py): the fp32 restatement within 1e-5 of float64, gradients 1e-7 absolute +
1e-5 of the largest float64 gradient."""
import ast
import itertools
import json
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy.spatial import ConvexHull, QhullError

from fullysparsefusion_amd import synthetic
from fullysparsefusion_amd.compat import Config
from fullysparsefusion_amd.mmdet3d_plugin import build_model
from fullysparsefusion_amd.mmdet3d_plugin.core.assigners import (HybridAssigner, MaxIoUAssigner, PointInBoxAssigner, bbox_overlaps_host,
                                                                 gt_boxes_2d_host, max_iou_assign_host)
from fullysparsefusion_amd.mmdet3d_plugin.core.bbox import LiDARInstance3DBoxes, box_corners_host
from fullysparsefusion_amd.mmdet3d_plugin.models.decode_heads.segmentation_head import points_in_boxes_first_host
from fullysparsefusion_amd.mmdet3d_plugin.models.dense_heads.cluster_heads import hybrid_targets_host
from test_cluster_losses_cpu import NUS_CLASSES, make_head, reference_losses_f64, with_flags
from test_seg_losses_cpu import check_pt_in_box3d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
W, H = 1600.0, 900.0
ASSIGNER_CFG = dict(type="HybridAssigner", num_cams=6,
                    assigner_2d=dict(type="MaxIoUAssigner", pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True,
                                     ignore_iof_thr=-1),
                    assigner_3d=dict(type="PointInBoxAssigner"), class_names=NUS_CLASSES, tasks=[dict(class_names=NUS_CLASSES)])
LOSS_NAMES = ["loss_cls", "loss_center", "loss_size", "loss_rot", "loss_vel"]


def make_assigner(**extra):
    cfg = {k: v for k, v in ASSIGNER_CFG.items() if k != "type"}
    cfg.update(extra)
    return HybridAssigner(**cfg)


def make_frustum_head(**extra):
    kw = dict(head_type="FrustumClusterHead", train_cfg=dict(), test_cfg=dict(), assigner=dict(ASSIGNER_CFG))
    kw.update(extra)
    return make_head(**kw)


# ------------------------------------------------------------------------------------------------ the transcription (float64, loops)
def transcribed_corners(box):
    x, y, z, w, l, h, rz = (float(v) for v in box[:7])
    c, s = math.cos(rz), math.sin(rz)
    return np.array([(x + dx * c - dy * s, y + dx * s + dy * c, z + dz) for dx in (-l / 2, l / 2) for dy in (-w / 2, w / 2)
                     for dz in (0.0, h)], F32)


def transcribed_projection(corners, lidar2img):
    """prj_lidar_bbox3d_on_img for one box: f32 matmul, depth clip, divide."""
    p = np.concatenate([corners, np.ones((8, 1), F32)], 1) @ np.asarray(lidar2img, F32).T
    valid = bool((p[:, 2] > 1e-5).any())
    d = np.clip(p[:, 2], F32(1e-5), F32(1e5))
    return np.stack([p[:, 0] / d, p[:, 1] / d], 1).astype(F32), valid


def clip_polygon(poly):
    """Sutherland-Hodgman against [0, W] x [0, H]."""
    def clip(poly, inside, inter):
        out = []
        for j in range(len(poly)):
            cur, prev = poly[j], poly[j - 1]
            if inside(cur):
                if not inside(prev):
                    out.append(inter(prev, cur))
                out.append(cur)
            elif inside(prev):
                out.append(inter(prev, cur))
        return out

    def at_x(x0):
        return lambda a, b: (x0, a[1] + (b[1] - a[1]) * (x0 - a[0]) / (b[0] - a[0]))

    def at_y(y0):
        return lambda a, b: (a[0] + (b[0] - a[0]) * (y0 - a[1]) / (b[1] - a[1]), y0)

    for inside, inter in ((lambda p: p[0] >= 0, at_x(0.0)), (lambda p: p[0] <= W, at_x(W)), (lambda p: p[1] >= 0, at_y(0.0)),
                          (lambda p: p[1] <= H, at_y(H))):
        poly = clip(poly, inside, inter)
        if not poly:
            return None
    return poly


def transcribed_box_2d(pts):
    """post_process_coords: hull of the eight points, intersected with the canvas, its bounding box (None when they do not meet)."""
    pts = pts.astype(np.float64)
    try:
        hull = ConvexHull(pts)
    except QhullError:
        return None
    poly = clip_polygon([tuple(pts[i]) for i in hull.vertices])
    if not poly:
        return None
    a = np.array(poly)
    box = (a[:, 0].min(), a[:, 1].min(), a[:, 0].max(), a[:, 1].max())
    return box if box[2] > box[0] and box[3] > box[1] else None


def iou64(g, d):
    ag, ad = (g[2] - g[0]) * (g[3] - g[1]), (d[2] - d[0]) * (d[3] - d[1])
    w, h = max(min(g[2], d[2]) - max(g[0], d[0]), 0.0), max(min(g[3], d[3]) - max(g[1], d[1]), 0.0)
    return w * h / max(ag + ad - w * h, 1e-6)


def transcribed_assign(preds_2d, centres, na_boxes, aug_boxes, lidar2img, pos_thr=0.7, min_pos=0.3):
    """HybridAssigner.assign for one sample and task (GT in the task's order): -> (final rows of the augmented list or -1,
    rows_3d, rows_2d, marginal bool [n])."""
    n = len(centres)
    rows_3d = np.full(n, -1, np.int64)
    for i in range(n):
        for k in range(len(aug_boxes)):
            if check_pt_in_box3d(centres[i], aug_boxes[k]):
                rows_3d[i] = k
                break
    rows_2d = np.full(n, -1, np.int64)
    marginal = np.zeros(n, bool)
    for cam in range(len(lidar2img)):
        gts, gt_idx = [], []
        for k in range(len(na_boxes)):
            pts, valid = transcribed_projection(transcribed_corners(na_boxes[k]), lidar2img[cam])
            box = transcribed_box_2d(pts) if valid else None
            if box is not None:
                gts.append(np.array([float(F32(v)) for v in box]))  # (torch.tensor(list): rounded to f32)
                gt_idx.append(k)
        mine = [i for i in range(n) if preds_2d[i, 6] == cam]
        if not gts or not mine:
            continue
        ov = np.array([[iou64(g, preds_2d[i, :4].astype(np.float64)) for i in mine] for g in gts])
        assigned = np.full(len(mine), -1, np.int64)
        max_ov, arg = ov.max(0), ov.argmax(0)
        gt_max = ov.max(1)
        for q in range(len(mine)):
            if max_ov[q] >= pos_thr:
                assigned[q] = arg[q]
        for j in range(len(gts)):
            if gt_max[j] >= min_pos:
                assigned[ov[j] == gt_max[j]] = j
        for q, i in enumerate(mine):
            if assigned[q] >= 0:
                rows_2d[i] = gt_idx[assigned[q]]
            col = np.sort(ov[:, q])[::-1]
            near = [v for v in ov[:, q] if v > 0] + [gt_max[j] for j in range(len(gts)) if ov[j, q] > 0]
            marginal[i] = (any(abs(v - t) < 1e-5 for v in near for t in (min_pos, pos_thr))
                           or (len(col) > 1 and col[0] >= min_pos and col[0] - col[1] < 1e-6)
                           or any(0 < gt_max[j] - ov[j, q] < 1e-6 for j in range(len(gts))))
    rows_2d[rows_2d >= len(aug_boxes)] = -1
    return np.where(rows_3d >= 0, rows_3d, rows_2d), rows_3d, rows_2d, marginal


# ------------------------------------------------------------------------------------------------ cases
def regroup(boxes, labels):
    """The valid rows in the task's order (all ten classes, the task's order = label order): what modify_gt_for_single_task leaves."""
    keep = labels >= 0
    boxes, labels = boxes[keep], labels[keep]
    order = np.argsort(labels, kind="stable")
    return boxes[order], labels[order]


def augment(boxes, angle=0.15, scale=1.04):
    """A global rotation + scaling of the GT (what the augmented list is): the order is kept."""
    out = boxes.copy()
    c, s = math.cos(angle), math.sin(angle)
    out[:, 0], out[:, 1] = (boxes[:, 0] * c - boxes[:, 1] * s) * scale, (boxes[:, 0] * s + boxes[:, 1] * c) * scale
    out[:, 2] *= scale
    out[:, 3:6] *= scale
    out[:, 6] += angle
    return out.astype(F32)


def frame_case(seed, box_dim=9):
    """(no-aug boxes, labels, augmented boxes, lidar2img, preds_2d f32 [n, 9], centres f32 [n, 3]) for one 1-sweep frame.  Detections:
    per visible (box, camera) a tight one (IoU >= 0.7), a shifted one (0.3 .. 0.7) and a far one (< 0.3), plus random boxes in every
    camera (those that see no GT included).  A third of the centres sit in an augmented box (3-D wins), the rest in none."""
    frame = synthetic.make_frame(num_sweeps=1, seed=seed, mask_instances=10)
    boxes, labels = synthetic.make_gt_boxes(frame["points"], seed=seed, box_dim=9)
    if box_dim == 10:
        boxes = with_flags(boxes, seed)
    aug = augment(boxes)
    l2i = np.asarray(frame["lidar2img"], np.float64)
    rng = np.random.default_rng(seed + 500)
    rb, _ = regroup(boxes, labels)
    b2d, keep = gt_boxes_2d_host(torch.from_numpy(rb), torch.from_numpy(l2i))
    dets = []
    for k, cam in zip(*np.nonzero(keep.numpy())):
        x0, y0, x1, y1 = b2d[k, cam].tolist()
        w, h = x1 - x0, y1 - y0
        for shift, grow in ((0.03, 0.97), (0.22, 1.0), (0.75, 1.1)):
            sx, sy = rng.uniform(-1, 1, 2) * shift
            cx, cy = (x0 + x1) / 2 + sx * w, (y0 + y1) / 2 + sy * h
            dets.append([cx - w * grow / 2, cy - h * grow / 2, cx + w * grow / 2, cy + h * grow / 2, rng.uniform(), labels[0] % 10, cam, len(dets), 1])
    for cam in range(6):
        for _ in range(12):
            x, y = rng.uniform(0, W - 50), rng.uniform(0, H - 50)
            dets.append([x, y, x + rng.uniform(20, 400), y + rng.uniform(20, 300), rng.uniform(), 0, cam, len(dets), 1])
    preds = np.array(dets, F32)
    n = len(preds)
    ra, _ = regroup(aug, labels)
    centres = np.stack([rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), np.full(n, 30.0)], 1)
    inside = rng.random(n) < 0.33
    pick = rng.integers(0, len(ra), n)
    grav = ra[pick, :3].astype(np.float64)
    grav[:, 2] += ra[pick, 5] / 2
    centres[inside] = grav[inside] + rng.normal(0, 0.1, (int(inside.sum()), 3))
    return boxes, labels, aug, l2i, preds, centres.astype(F32)


def host_targets(assigner, centres, bidx, preds, na_list, aug_list, l2i, code=10, parts=False):
    """hybrid_targets_host on per-sample (boxes, labels) pairs that are NOT yet in the task's order."""
    na = [regroup(b, l) for b, l in na_list]
    au = [regroup(b, l) for b, l in aug_list]
    return hybrid_targets_host(assigner, torch.from_numpy(centres), torch.from_numpy(bidx), torch.from_numpy(preds),
                               [torch.from_numpy(b) for b, _ in na], [torch.from_numpy(l) for _, l in na],
                               [torch.from_numpy(b) for b, _ in au], [torch.from_numpy(l) for _, l in au],
                               torch.from_numpy(np.asarray(l2i, np.float64)).float(), 10, code, return_parts=parts)


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_host_restatement_equals_the_transcription_on_a_frame(seed):
    boxes, labels, aug, l2i, preds, centres = frame_case(seed)
    out = host_targets(make_assigner(), centres, np.zeros(len(centres), np.int64), preds, [(boxes, labels)], [(aug, labels)], l2i[None], parts=True)
    part = out[-1][0]
    rb, _ = regroup(boxes, labels)
    ra, rl = regroup(aug, labels)
    final, rows_3d, rows_2d, marginal = transcribed_assign(preds, centres, rb, ra, l2i.astype(F32))
    share = marginal.mean()
    print(f"K37 seed {seed}: n = {len(centres)}, 3-D {int((rows_3d >= 0).sum())}, 2-D {int((rows_2d >= 0).sum())}, 2-D only "
          f"{int(((rows_3d < 0) & (rows_2d >= 0)).sum())}, marginal share {share:.4f}")
    assert share <= 0.01
    ok = ~marginal
    assert np.array_equal(part["rows_3d"].numpy(), rows_3d)
    assert np.array_equal(part["rows_2d"].numpy()[ok], rows_2d[ok])
    assert np.array_equal(out[4].numpy()[ok], final[ok])
    assert int(((rows_3d < 0) & (rows_2d >= 0)).sum()) >= 20 and int((rows_3d >= 0).sum()) >= 20
    # all three IoU bands occur among the detections' maxima
    b2d, keep = part["boxes_2d"], part["keep"]
    mx = []
    for cam in range(6):
        kept = torch.nonzero(keep[:, cam]).reshape(-1)
        mine = np.flatnonzero(preds[:, 6] == cam)
        if len(kept) and len(mine):
            mx.append(bbox_overlaps_host(b2d[kept, cam], torch.from_numpy(preds[mine, :4])).max(0)[0])
    mx = torch.cat(mx)
    assert int((mx >= 0.7).sum()) >= 5 and int(((mx >= 0.3) & (mx < 0.7)).sum()) >= 5 and int((mx < 0.3).sum()) >= 5
    # labels and targets follow the assignment on the AUGMENTED list
    lab = out[0].numpy()
    assert np.array_equal(lab[ok], np.where(final >= 0, rl[np.maximum(final, 0)], 10)[ok])
    pos = np.flatnonzero(ok & (final >= 0))
    assert np.array_equal(out[2].numpy()[pos, :3], (ra[final[pos], :3] - centres[pos]).astype(F32))
    assert float(out[5][2]) == len(ra) and float(out[5][1]) == int((out[4] >= 0).sum())


def test_2d_boxes_equal_the_hull_construction():
    """The hull-free construction against scipy's hull + polygon clipping, on every (box, camera) of the three frames."""
    worst, seen = 0.0, 0
    for seed in (3, 4, 5):
        boxes, labels, _, l2i, _, _ = frame_case(seed)
        rb, _ = regroup(boxes, labels)
        b2d, keep = gt_boxes_2d_host(torch.from_numpy(rb), torch.from_numpy(l2i))
        for k in range(len(rb)):
            for cam in range(6):
                pts, valid = transcribed_projection(transcribed_corners(rb[k]), l2i[cam].astype(F32))
                box = transcribed_box_2d(pts) if valid else None
                assert (box is not None) == bool(keep[k, cam]), (seed, k, cam)
                if box is not None:
                    seen += 1
                    worst = max(worst, float(np.abs(np.array(box) - b2d[k, cam].double().numpy()).max()))
    print(f"K37 2-D boxes: {seen} visible, largest difference to hull + clipping {worst:.3e} px")
    assert seen >= 100 and worst <= 1e-3  # (f32 rounding of coordinates up to 1600: 6e-5; the corners' cos / sin: a few ulp more)


# ------------------------------------------------------------------------------------------------ targeted cases
CAM0 = np.array([[1000.0, 0, 800, 0], [0, 1000.0, 450, 0], [0, 0, 1, 0], [0, 0, 0, 1]])  # looks along +z: u = 1000 x / z + 800


def cam_along_x(yaw):
    """lidar2img of a pinhole camera at the origin looking along (cos yaw, sin yaw), z up."""
    c, s = math.cos(yaw), math.sin(yaw)
    r = np.array([[s, -c, 0, 0], [0, 0, -1, 0], [c, s, 0, 0], [0, 0, 0, 1.0]])
    return CAM0 @ r


def targeted_cases():
    """name -> dict(centres, bidx, preds, na=[(boxes, labels)], aug=[(boxes, labels)], l2i [B, ncam, 4, 4], expect=assigned rows)."""
    cases = {}
    far = [0.0, 0.0, 50.0]
    box = lambda x, y, yaw=0.3, w=2.0, l=4.0, h=1.6: [x, y, -1.0, w, l, h, yaw, 0.5, -0.5]  # noqa: E731
    l2i = np.stack([cam_along_x(0.0), cam_along_x(math.pi / 2)] + [cam_along_x(math.pi)] * 4)[None]
    a = make_assigner()

    def b2d_of(boxes, l2i_b):
        return gt_boxes_2d_host(torch.tensor(boxes, dtype=torch.float32), torch.from_numpy(l2i_b))

    def det(b, cam, dx=0.0, grow=1.0):
        x0, y0, x1, y1 = b.tolist()
        w, h = (x1 - x0) * grow, (y1 - y0) * grow
        cx, cy = (x0 + x1) / 2 + dx * (x1 - x0), (y0 + y1) / 2
        return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, 0.9, 0, cam, 0, 1]

    def case(name, centres, preds, na, aug=None, l2i_=l2i, bidx=None, expect=None):
        na = [(np.array(b, F32).reshape(-1, 9), np.array(l, np.int64)) for b, l in na]
        aug = na if aug is None else [(np.array(b, F32).reshape(-1, 9), np.array(l, np.int64)) for b, l in aug]
        n = len(centres)
        cases[name] = dict(centres=np.array(centres, F32).reshape(n, 3), preds=np.array(preds, F32).reshape(n, 9), na=na, aug=aug, l2i=l2i_,
                           bidx=np.zeros(n, np.int64) if bidx is None else np.array(bidx, np.int64), expect=expect)

    # a box straddling the left image border of camera 0 (x forward 10 m, y = 8 m is u = 0)
    g = [box(10.0, 8.0)]
    b, k = b2d_of(g, l2i[0])
    assert bool(k[0, 0]) and float(b[0, 0, 0]) == 0.0 and float(b[0, 0, 2]) > 50
    case("straddling_border", [far], [det(b[0, 0], 0)], [(g, [0])], expect=[0])
    # corners behind the camera: the box surrounds the camera plane (x from -1 to 5)
    g = [box(2.0, 0.5, yaw=0.0, l=6.0)]
    b, k = b2d_of(g, l2i[0])
    assert bool(k[0, 0])
    case("corners_behind_camera", [far], [det(b[0, 0], 0)], [(g, [0])], expect=[0])
    # a box seen by cameras 0 (along +x) and 1 (along +y): one query in each
    g = [box(9.0, 9.0, l=3.0)]
    b, k = b2d_of(g, l2i[0])
    assert bool(k[0, 0]) and bool(k[0, 1])
    case("two_cameras", [far, far], [det(b[0, 0], 0), det(b[0, 1], 1)], [(g, [0])], expect=[0, 0])
    # low-quality matching overrides a >= 0.7 match: the only query overlaps box 0 by >= 0.7 and box 1 by 0.3 .. 0.7; it is box 1's
    # maximum too, and box 1 comes later, so box 1 claims it
    g = [box(12.0, 1.0), box(12.0, -0.2)]
    b, k = b2d_of(g, l2i[0])
    q = det(b[0, 0], 0, dx=0.05)
    ov = bbox_overlaps_host(b[:, 0], torch.tensor([q[:4]], dtype=torch.float32))
    assert float(ov[0, 0]) >= 0.7 and 0.3 <= float(ov[1, 0]) < 0.7
    case("low_quality_overrides_pos", [far], [q], [(g, [0, 0])], expect=[1])
    # a later box overrides an earlier one: two identical boxes, both claim the query, the second stands
    g = [box(12.0, 1.0), box(12.0, 1.0)]
    b, k = b2d_of(g, l2i[0])
    case("later_box_overrides", [far], [det(b[0, 0], 0, dx=0.2)], [(g, [0, 1])], expect=[1])
    # two queries tie for a box's maximum (mirror images, IoU in the 0.3 .. 0.7 band): both are claimed
    g = [box(12.0, 0.0, yaw=0.0)]
    b, k = b2d_of(g, l2i[0])
    x0, y0, x1, y1 = b[0, 0].tolist()
    w = x1 - x0
    ql = [x0 - 0.25 * w, y0, x1 - 0.25 * w, y1, 0.9, 0, 0, 0, 1]
    qr = [x0 + 0.25 * w, y0, x1 + 0.25 * w, y1, 0.9, 0, 0, 1, 1]
    ov = bbox_overlaps_host(b[:, 0], torch.tensor([ql[:4], qr[:4]], dtype=torch.float32))
    if float(ov[0, 0]) != float(ov[0, 1]):  # (an exact tie needs exactly mirrored roundings: fall back to the same box twice)
        qr = list(ql)
    case("two_queries_tie", [far, far], [ql, qr], [(g, [0])], expect=[0, 0])
    # 3-D beats 2-D: the centre is inside box 0, the 2-D box sits on box 1
    g = [box(12.0, 4.0), box(12.0, -4.0)]
    b, k = b2d_of(g, l2i[0])
    case("3d_beats_2d", [[12.0, 4.0, -0.2], far], [det(b[1, 0], 0), det(b[1, 0], 0)], [(g, [0, 1])], expect=[0, 1])
    # a no-aug index beyond the augmented list: two no-aug boxes, one augmented box; the query matches no-aug row 1
    case("index_beyond_augmented", [far, far], [det(b[1, 0], 0), det(b[0, 0], 0)], [(g, [0, 1])], aug=[([g[0]], [0])], expect=[-1, 0])
    # an empty sample in a batch of two (sample 0 has no GT at all)
    l2 = np.concatenate([l2i, l2i])
    case("empty_sample_in_batch", [far, far], [det(b[0, 0], 0), det(b[0, 0], 0)], [([], []), (g, [0, 1])], l2i_=l2, bidx=[0, 1], expect=[-1, 0])
    case("no_queries", np.zeros((0, 3)), np.zeros((0, 9)), [(g, [0, 1])], expect=[])
    case("no_gt", [far], [det(b[0, 0], 0)], [([], [])], expect=[-1])
    return cases


@pytest.mark.parametrize("name", sorted(targeted_cases()))
def test_targeted_case_on_the_host(name):
    c = targeted_cases()[name]
    out = host_targets(make_assigner(), c["centres"], c["bidx"], c["preds"], c["na"], c["aug"], c["l2i"])
    assert out[4].tolist() == list(c["expect"]), (name, out[4].tolist())
    for b in range(len(c["na"])):  # and the transcription agrees, sample by sample
        mine = np.flatnonzero(c["bidx"] == b)
        final, _, _, _ = transcribed_assign(c["preds"][mine], c["centres"][mine], regroup(*c["na"][b])[0], regroup(*c["aug"][b])[0],
                                            c["l2i"][b].astype(F32))
        assert final.tolist() == [c["expect"][i] for i in mine], name


def test_low_quality_and_tie_rules_of_max_iou():
    ov = torch.tensor([[0.75, 0.4, 0.1], [0.5, 0.4, 0.2], [0.5, 0.1, 0.2]])
    # query 0: max 0.75 with GT 0, but GTs 1 and 2 have their maximum (0.5) there too: the last claim stands
    assert max_iou_assign_host(ov, 0.7, 0.3).tolist() == [2, -1, -1]
    assert max_iou_assign_host(ov, 0.7, 0.3, match_low_quality=False).tolist() == [0, -1, -1]
    tie = torch.tensor([[0.45, 0.45, 0.1]])
    assert max_iou_assign_host(tie, 0.7, 0.3).tolist() == [0, 0, -1]
    assert max_iou_assign_host(tie, 0.7, 0.3, gt_max_assign_all=False).tolist() == [0, -1, -1]
    assert max_iou_assign_host(torch.zeros((0, 3)), 0.7, 0.3).tolist() == [-1, -1, -1]
    a = MaxIoUAssigner(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3)
    res = a.assign(torch.tensor([[0.0, 0, 10, 10], [0, 0, 10, 5], [50, 50, 60, 60]]), torch.tensor([[0.0, 0, 10, 10]]), gt_labels=torch.tensor([4]))
    assert res.gt_inds.tolist() == [1, -1, 0] and res.labels.tolist() == [4, -1, -1]


# ------------------------------------------------------------------------------------------------ corners
def test_corners_are_the_vertices_of_the_solid_the_containment_test_tests():
    rng = np.random.default_rng(0)
    m = 200
    rows = np.concatenate([rng.uniform(-40, 40, (m, 2)), rng.uniform(-3, 1, (m, 1)), rng.uniform(0.5, 5, (m, 3)),
                           rng.uniform(-2 * math.pi, 2 * math.pi, (m, 1))], 1).astype(F32)
    boxes = LiDARInstance3DBoxes(torch.from_numpy(rows))
    corners = boxes.corners
    assert corners.shape == (m, 8, 3) and torch.equal(corners, box_corners_host(boxes.tensor))
    centre = boxes.gravity_center[:, None, :]
    for k in range(m):
        inner = centre[k] + (corners[k] - centre[k]) * 0.99
        outer = centre[k] + (corners[k] - centre[k]) * 1.01
        assert points_in_boxes_first_host(inner, boxes.tensor[k:k + 1, :7]).tolist() == [0] * 8
        assert points_in_boxes_first_host(outer, boxes.tensor[k:k + 1, :7]).tolist() == [-1] * 8
    assert len({tuple(np.round(v, 4)) for v in corners[0].tolist()}) == 8


# ------------------------------------------------------------------------------------------------ losses and the public surface
def loss_case(seed=3, box_dim=10):
    boxes, labels, aug, l2i, preds, centres = frame_case(seed, box_dim)
    metas = [dict(lidar2img=[m for m in l2i])]
    n = len(centres)
    g = torch.Generator().manual_seed(seed)
    z, r = torch.randn((n, 10), generator=g) * 2, torch.randn((n, 10), generator=g)
    inds = torch.zeros((n, 3), dtype=torch.long)
    return dict(z=z, r=r, xyz=torch.from_numpy(centres), inds=inds, na_b=[torch.from_numpy(boxes)], na_l=[torch.from_numpy(labels)],
                gt_b=[torch.from_numpy(aug)], gt_l=[torch.from_numpy(labels)], preds=torch.from_numpy(preds), metas=metas,
                raw=(boxes, labels, aug, l2i, preds, centres))


def head_loss(head, c, z, r, fused, dev="cpu"):
    put = lambda t: t.to(dev)  # noqa: E731
    return head.loss([z], [r], put(c["xyz"]), put(c["inds"]), c["na_b"], c["na_l"], c["gt_b"], c["gt_l"], put(c["preds"]), c["metas"],
                     fused=fused)


def test_unfused_loss_matches_float64_autograd_and_names_its_keys():
    c = loss_case()
    head = make_frustum_head()
    z, r = c["z"].clone().requires_grad_(), c["r"].clone().requires_grad_()
    out = head_loss(head, c, z, r, fused=False)
    names = LOSS_NAMES + ["num_preds", "num_pos_preds", "num_gts", "assigned_gts"]
    assert set(out) == {k + f"{NUS_CLASSES}" for k in names}
    got = {k: out[k + f"{NUS_CLASSES}"] for k in names}
    boxes, labels, aug, l2i, preds, centres = c["raw"]
    lab, _, tgt, wgt, asg, stats = host_targets(make_assigner(), centres, np.zeros(len(centres), np.int64), preds, [(boxes, labels)],
                                                [(aug, labels)], l2i[None])
    assert [float(got[k]) for k in names[5:]] == stats[:4].tolist() and float(stats[1]) >= 40
    assert bool(((wgt[:, 8] == 0) & (lab < 10)).any()) and bool(((wgt[:, 8] == 1) & (lab < 10)).any())  # the copy-paste flag at work
    grads = [1.0, 0.7, 1.3, 0.9, 1.1]
    want, gz, gr = reference_losses_f64(c["z"], c["r"], lab, tgt, wgt, 4.0, 0.25, [1.0, 0.5, 0.5, 0.2, 0.2], True, grads)
    for k, w in zip(LOSS_NAMES, want):
        assert abs(float(got[k].detach()) - float(w)) <= 1e-5 * abs(float(w)), k
    sum(g * got[k] for g, k in zip(grads, LOSS_NAMES)).backward()
    assert float((z.grad.double() - gz).abs().max()) <= 1e-7 + 1e-5 * float(gz.abs().max())
    assert float((r.grad.double() - gr).abs().max()) <= 1e-7 + 1e-5 * float(gr.abs().max())
    same = head_loss(head, c, z, r, fused=True)  # fused=True, but nothing here is on a GPU
    assert all(torch.equal(out[k].detach(), same[k].detach()) for k in out)


def test_loss_without_queries_is_zero():
    c = loss_case()
    head = make_frustum_head()
    z, r = torch.zeros((0, 10), requires_grad=True), torch.zeros((0, 10), requires_grad=True)
    out = head.loss([z], [r], torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.long), c["na_b"], c["na_l"], c["gt_b"], c["gt_l"],
                    torch.zeros((0, 9)), c["metas"])
    got = {k[:-len(f"{NUS_CLASSES}")]: v for k, v in out.items()}
    assert all(float(got[k].detach()) == 0.0 for k in LOSS_NAMES + ["num_preds", "num_pos_preds"]) and float(got["num_gts"]) == 41.0
    sum(got[k] for k in LOSS_NAMES).backward()
    assert z.grad.shape == (0, 10)


@pytest.mark.parametrize("option,kwargs", [
    ("use_one_to_one", dict(use_one_to_one=True)),
    ("is_frustum", dict(assigner=dict(ASSIGNER_CFG, is_frustum=True))),
    ("match_low_quality", dict(assigner=dict(ASSIGNER_CFG, assigner_2d=dict(ASSIGNER_CFG["assigner_2d"], match_low_quality=False)))),
    ("assigner_3d", dict(assigner={k: v for k, v in ASSIGNER_CFG.items() if k != "assigner_3d"})),
    ("loss_iou", dict(loss_iou=dict(type="L1Loss"))),
    ("code_weight", dict(train_cfg=dict(code_weight=[1.0] * 10)))])
def test_options_no_config_sets_are_refused_by_name(option, kwargs):
    c = loss_case()
    head = make_frustum_head(**kwargs)
    with pytest.raises(NotImplementedError, match=option):
        head_loss(head, c, c["z"], c["r"], fused=False)


def test_heads_without_a_hybrid_assigner_still_refuse_before_touching_their_arguments():
    refine = make_frustum_head(assigner=dict(type="FrustumAssigner", num_cams=6, assigner_2d=dict(type="MaxIoUAssigner", pos_iou_thr=0.7,
                                                                                                neg_iou_thr=0.3),
                                             assigner_dist=dict(type="DistAssigner")))
    assert getattr(refine.assigner, "OUT_OF_SCOPE", False)
    bare = make_head(head_type="FrustumClusterHead", train_cfg=dict(), test_cfg=dict())
    for head in (refine, bare):
        with pytest.raises(NotImplementedError, match="FrustumClusterHead"):
            head.loss(None, None, None, None, None, None, None, None)
    real = make_frustum_head()
    assert type(real.assigner) is HybridAssigner and type(real.assigner.assigner_3d) is PointInBoxAssigner
    assert type(real.assigner.assigner_2d) is MaxIoUAssigner and not getattr(real.assigner, "OUT_OF_SCOPE", False)
    assert (real.assigner.assigner_2d.pos_iou_thr, real.assigner.assigner_2d.min_pos_iou, real.assigner.assigner_3d.extra_height) == (0.7, 0.3, 0.0)


@pytest.mark.parametrize("config", ["fsf_nuscenes.py", "fsf_av2.py"])
def test_both_configs_still_build_with_unchanged_state(config):
    cfg = Config.fromfile(os.path.join(ROOT, "configs", config))
    model = build_model(cfg.model)
    with open(os.path.join(ROOT, "tests", "golden", "reference_configs.json")) as f:
        golden = json.load(f)["nuscenes" if "nuscenes" in config else "av2"]
    from conftest import state_shapes_digest

    assert state_shapes_digest(model) == (golden["state_dict_entries"], golden["state_dict_shapes"])
    if "nuscenes" in config:
        assert type(model.frustum_obj_head.assigner) is HybridAssigner
        model.frustum_obj_head._check_loss_cfg()  # the config sets no refused option
    for head in model.frustum_refined_head if hasattr(model, "frustum_refined_head") else []:
        assert type(getattr(head, "assigner", None)) is not HybridAssigner


def test_forward_train_graph_has_the_flag_and_names_the_missing_argument():
    import inspect

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "fsf_nuscenes.py"))
    model = build_model(cfg.model)
    sig = inspect.signature(model.forward_train_graph)
    assert sig.parameters["camera_head_losses"].default is False
    assert sig.parameters["no_aug_gt_bboxes_3d"].default is None and sig.parameters["no_aug_gt_labels_3d"].default is None
    gt = ([torch.zeros((0, 9))], [torch.zeros(0, dtype=torch.long)])
    with pytest.raises(ValueError, match="no_aug_gt_bboxes_3d"):
        model.forward_train_graph(None, None, None, None, gt_bboxes_3d=gt[0], gt_labels_3d=gt[1], camera_head_losses=True)
    with pytest.raises(ValueError, match="no_aug_gt_labels_3d"):
        model.forward_train_graph(None, None, None, None, gt_bboxes_3d=gt[0], gt_labels_3d=gt[1], camera_head_losses=True,
                                  no_aug_gt_bboxes_3d=gt[0])
    with pytest.raises(ValueError, match="gt_bboxes_3d"):
        model.forward_train_graph(None, None, None, None, camera_head_losses=True)
    with pytest.raises(NotImplementedError, match="lidar_head_losses"):
        model.forward_train([torch.zeros((4, 8))], [dict()])


# ------------------------------------------------------------------------------------------------ C ABI surface and guard-band cover
def test_entry_points_are_declared_documented_and_the_abi_version_stays():
    from fullysparsefusion_amd import _lib

    for name in ("fsf_gt_boxes_2d", "fsf_hybrid_assign", "fsf_hybrid_assign_workspace_bytes"):
        assert name in _lib.SIGNATURES
        with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
            assert name in f.read(), name
    assert _lib.DEFINES["FSF_ABI_VERSION"] == 23
    assert len(_lib.SIGNATURES["fsf_hybrid_assign"][0]) == 33 and len(_lib.SIGNATURES["fsf_gt_boxes_2d"][0]) == 13


_ALLOCATES = re.compile(r"torch\.empty|empty_like|torch\.zeros|torch\.full|_lib\.workspace\(|_workspace_bytes|_arena_bytes")
_SCRATCH = re.compile(r"_lib\.workspace\(|_workspace_bytes|_arena_bytes")


def allocating_wrappers():
    """tests/test_guarded_alloc_cpu.py's scan, pointed at hip_ops_assign.py."""
    with open(os.path.join(ROOT, "fullysparsefusion_amd", "hip_ops_assign.py")) as f:
        src = f.read()
    alloc, scratch = set(), set()
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef):
            body = ast.get_source_segment(src, node)
            if _ALLOCATES.search(body):
                alloc.add(node.name)
                if _SCRATCH.search(body):
                    scratch.add(node.name)
    return alloc, scratch


def test_every_allocating_wrapper_of_the_new_module_has_guard_band_cases():
    import test_guard_bands_assign_gpu as gb

    alloc, scratch = allocating_wrappers()
    assert alloc == {"gt_boxes_2d", "hybrid_assign"} and scratch == {"hybrid_assign"}
    assert sorted(alloc - set(gb.CASES)) == []
    from fullysparsefusion_amd import hip_ops_assign

    for name, cases in gb.CASES.items():
        assert hasattr(hip_ops_assign, name)
        kinds = [k for k, _ in cases]
        assert "ragged" in kinds and "minimal" in kinds and "empty" in kinds, name
    # the wrappers allocate with torch.empty and _lib.workspace only
    with open(os.path.join(ROOT, "fullysparsefusion_amd", "hip_ops_assign.py")) as f:
        src = f.read()
    assert not re.search(r"torch\.zeros|torch\.full|empty_like|torch\.ones|new_zeros|new_empty|new_full", src)
