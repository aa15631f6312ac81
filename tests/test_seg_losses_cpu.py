"""The segmentation head's targets and losses on the host (the torch restatement K35 is checked against): targets against a
literal transcription of mmdet3d 0.x check_pt_in_box3d written here, losses against the reference `losses` expression in float64,
and the loss modules both configs build."""
import json
import math
import os

import numpy as np
import pytest
import torch

from fullysparsefusion_amd import synthetic
from fullysparsefusion_amd.compat import Config
from fullysparsefusion_amd.mmdet3d_plugin import build_model
from fullysparsefusion_amd.mmdet3d_plugin.core.bbox import LiDARInstance3DBoxes
from fullysparsefusion_amd.mmdet3d_plugin.models.decode_heads.segmentation_head import points_in_boxes_first_host, seg_targets_host
from fullysparsefusion_amd.mmdet3d_plugin.models.losses import CrossEntropyLoss, L1Loss
from fullysparsefusion_amd.mmdet3d_plugin.registry import build_head

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def check_pt_in_box3d(pt, box):
    """mmdet3d 0.x points_in_boxes_gpu's device function, one f32 operation at a time (cos / sin in float64, rounded once)."""
    x, y, z = (F32(v) for v in pt)
    cx, cy, cz, w, l, h, rz = (F32(v) for v in box[:7])
    cz = F32(cz + h / F32(2))
    if abs(F32(z - cz)) > h / 2.0:
        return False
    cosa, sina = F32(math.cos(-float(rz))), F32(math.sin(-float(rz)))
    sx, sy = F32(x - cx), F32(y - cy)
    lx = F32(F32(sx * cosa) + F32(sy * -sina))
    ly = F32(F32(sx * sina) + F32(sy * cosa))
    return bool((lx > -l / 2.0) & (lx < l / 2.0) & (ly > -w / 2.0) & (ly < w / 2.0))


def transcribed_targets(points, boxes, labels, bg):
    """get_targets / get_point_labels / get_vote_target for one sample, point by point."""
    keep = labels >= 0
    boxes, labels = boxes[keep], labels[keep]
    n = points.shape[0]
    lab = np.full(n, bg, np.int64)
    tgt = np.zeros((n, 3), np.float32)
    msk = np.zeros(n, bool)
    for i in range(n):
        for k in range(boxes.shape[0]):
            if check_pt_in_box3d(points[i, :3], boxes[k]):
                lab[i], msk[i] = labels[k], True
                g = (F32(boxes[k, 0]), F32(boxes[k, 1]), F32(F32(boxes[k, 2]) + F32(boxes[k, 5]) * F32(0.5)))
                for c in range(3):
                    d = F32(g[c] - F32(points[i, c]))
                    tgt[i, c] = F32(np.sign(d) * np.sqrt(abs(d)))
                break
    return lab, tgt, msk


def edge_case():
    """Points on every face of an axis-aligned and of a rotated box, and one f32 ulp to either side; two overlapping boxes; a
    label -1 row covering everything (dropped)."""
    boxes = np.array([[100.0, -50.0, -1.0, 1.0, 2.0, 2.0, 0.0, 0, 0],
                      [1.0, 2.0, -1.5, 2.0, 4.0, 1.5, 0.0, 0, 0],
                      [1.5, 2.5, -1.2, 2.0, 3.0, 2.0, 0.3, 0, 0],
                      [5.0, -3.0, -1.0, 1.6, 3.6, 1.8, 0.7, 0, 0]], np.float32)
    labels = np.array([-1, 3, 7, 2])
    boxes[0, 3:6] = 1000.0  # the ignored row would contain every point
    pts = []
    for k in (1, 3):
        cx, cy, zb, w, l, h, yaw = (float(v) for v in boxes[k, :7])
        c, s = math.cos(yaw), math.sin(yaw)
        for lx, ly, z in ((l / 2, 0.0, zb + h / 2), (-l / 2, 0.0, zb + h / 2), (0.0, w / 2, zb + h / 2), (0.0, -w / 2, zb + h / 2),
                          (0.0, 0.0, zb), (0.0, 0.0, zb + h), (0.1, 0.1, zb + 0.3)):
            p = np.array([cx + lx * c - ly * s, cy + lx * s + ly * c, z], np.float32)
            for axis in range(3):
                for direction in (-np.inf, np.inf):
                    q = p.copy()
                    q[axis] = np.nextafter(q[axis], F32(direction))
                    pts.append(q)
            pts.append(p)
    pts = np.stack(pts)
    return np.concatenate([pts, np.zeros((pts.shape[0], 2), np.float32)], 1), boxes, labels


def test_host_targets_equal_the_transcribed_formula_on_face_points():
    pts, boxes, labels = edge_case()
    want = transcribed_targets(pts, boxes, labels, 10)
    got = seg_targets_host(torch.from_numpy(pts), torch.from_numpy(boxes), torch.from_numpy(labels), 10)
    assert np.array_equal(got[0].numpy(), want[0])
    assert np.array_equal(got[1].numpy(), want[1])
    assert np.array_equal(got[2].numpy(), want[2])
    inside = want[2]
    assert 0 < inside.sum() < len(inside)  # the faces really split the points
    assert set(want[0][inside]) == {3, 7, 2}  # both boxes of the overlap take points; the label -1 row takes none


def test_get_targets_batch_with_an_empty_sample_equals_the_transcription():
    head = build_head(dict(type="VoteSegHead", in_channel=16, num_classes=10, hidden_dims=[16],
                           loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, class_weight=[1.0] * 10 + [0.1], loss_weight=10.0),
                           loss_vote=dict(type="L1Loss", loss_weight=1.0)))
    rng = np.random.default_rng(3)
    p0, b0, l0 = edge_case()
    p1 = np.concatenate([rng.uniform(-8, 8, (400, 2)), rng.uniform(-2.5, 1.0, (400, 1)), np.zeros((400, 2))], 1).astype(np.float32)
    b1, l1 = synthetic.make_gt_boxes(p1, num_boxes=6, num_overlap=2, num_ignored=1, box_dim=9, min_range=0.0, max_range=9.0)
    p2 = p1[:50].copy()
    points = [torch.from_numpy(p0), torch.from_numpy(p1), torch.from_numpy(p2)]
    gts = [LiDARInstance3DBoxes(torch.from_numpy(b0), box_dim=9), torch.from_numpy(b1[:, :7]), torch.zeros((0, 7))]
    labels = [torch.from_numpy(l0), torch.from_numpy(l1), torch.zeros((0,), dtype=torch.long)]
    got = head.get_targets(points, gts, labels)
    want = [transcribed_targets(p, b, l, 10) for p, b, l in ((p0, b0, l0), (p1, b1, l1), (p2, np.zeros((0, 9), np.float32), np.zeros(0, int)))]
    for k in range(3):
        assert np.array_equal(got[k].numpy(), np.concatenate([w[k] for w in want]))
    assert got[0].dtype == torch.int64 and got[2].dtype == torch.bool
    assert not want[2][2].any() and (want[2][0] == 10).all()
    # the flat form (rows of several samples in any order) gives every row the same targets
    order = torch.from_numpy(rng.permutation(sum(len(p) for p in points)))
    flat = torch.cat(points)[order]
    bidx = torch.cat([torch.full((len(p),), b) for b, p in enumerate(points)])[order]
    got_flat = head.get_targets_flat(flat, bidx, gts, labels)
    for k in range(3):
        assert torch.equal(got_flat[k], got[k][order])


def reference_losses_f64(logits, votes, labels, targets, mask, class_weight, lw_ce, lw_vote):
    """segmentation_head.py:106-150 with mmdet 2.14's cross_entropy (class_weight, reduction 'none', then .mean()) and l1_loss."""
    logits, votes = logits.double(), votes.double()
    c = logits.shape[1]
    ce = torch.nn.functional.cross_entropy(logits, labels, weight=torch.tensor(class_weight, dtype=torch.float64), reduction="none")
    loss_ce = lw_ce * ce.mean()
    v = votes.reshape(-1, c, 3)[mask].reshape(-1, 3)
    n_valid = int(mask.sum())
    if n_valid > 0:
        idx = torch.arange(n_valid) * c + labels[mask]
        loss_vote = lw_vote * (v[idx] - targets[mask].double()).abs().mean()
    else:
        loss_vote = votes.sum() * 0
    return loss_ce, loss_vote


@pytest.mark.parametrize("config", ["fsf_nuscenes.py", "fsf_av2.py"])
@pytest.mark.parametrize("n_valid_zero", [False, True])
def test_host_losses_equal_the_reference_expression(config, n_valid_zero):
    cfg = Config.fromfile(os.path.join(ROOT, "configs", config))
    head = build_head(dict(cfg.model.segmentor.segmentation_head))
    c = head.num_classes
    g = torch.Generator().manual_seed(5)
    n = 3000
    logits = torch.randn((n, c), generator=g) * 2
    votes = torch.randn((n, 3 * c), generator=g)
    labels = torch.randint(0, c, (n,), generator=g)
    labels[:7] = c - 1
    mask = (labels < c - 1) & (torch.rand(n, generator=g) < 0.7)
    if n_valid_zero:
        mask[:] = False
    targets = torch.randn((n, 3), generator=g) * mask[:, None]
    lw_ce, lw_vote = head.loss_decode.loss_weight, head.loss_vote.loss_weight
    want = reference_losses_f64(logits, votes, labels, targets, mask, head.loss_decode.class_weight, lw_ce, lw_vote)
    lg, vt = logits.clone().requires_grad_(), votes.clone().requires_grad_()
    got = head.losses(lg, vt, labels, targets, mask, fused=False)
    assert set(got) == {"loss_sem_seg", "loss_vote"}
    got_ce, got_vote = float(got["loss_sem_seg"].detach()), float(got["loss_vote"].detach())
    assert abs(got_ce - float(want[0])) <= 1e-6 * abs(float(want[0]))
    assert abs(got_vote - float(want[1])) <= 1e-6 * abs(float(want[1]))
    # the mean runs over N, not over the sum of the class weights (the background weight is 0.1)
    w = torch.tensor(head.loss_decode.class_weight, dtype=torch.float64)[labels]
    assert abs(float(want[0]) * n / float(w.sum()) - got_ce) > 1e-3 * float(want[0])
    (got["loss_sem_seg"] + got["loss_vote"]).backward()
    assert torch.isfinite(lg.grad).all() and torch.isfinite(vt.grad).all()
    if n_valid_zero:
        assert got_vote == 0.0 and not vt.grad.any()


@pytest.mark.parametrize("config,num_classes,lw", [("fsf_nuscenes.py", 10, 10.0), ("fsf_av2.py", 26, 3.0)])
def test_both_configs_build_real_loss_modules_without_state(config, num_classes, lw):
    cfg = Config.fromfile(os.path.join(ROOT, "configs", config))
    model = build_model(cfg.model)
    head = model.segmentor.segmentation_head
    assert type(head.loss_decode) is CrossEntropyLoss and type(head.loss_vote) is L1Loss
    assert not getattr(head.loss_decode, "OUT_OF_SCOPE", False)
    assert head.loss_decode.class_weight == [1.0] * num_classes + [0.1] and head.loss_decode.loss_weight == lw
    assert head.loss_vote.loss_weight == 1.0 and head.num_classes == num_classes + 1
    for mod in (head.loss_decode, head.loss_vote):
        assert list(mod.parameters()) == [] and list(mod.buffers()) == []
    sd = model.state_dict()
    assert not any("loss" in k for k in sd)
    with open(os.path.join(ROOT, "tests", "golden", "reference_configs.json")) as f:
        golden = json.load(f)["nuscenes" if "nuscenes" in config else "av2"]
    assert len(sd) == golden["state_dict_entries"]


def test_make_gt_boxes_has_overlaps_ignored_rows_and_both_forms():
    pts = synthetic.make_frame(num_sweeps=1, seed=0)["points"]
    b9, l9 = synthetic.make_gt_boxes(pts, seed=1)
    b7, l7 = synthetic.make_gt_boxes(pts, seed=1, box_dim=7, num_classes=26)
    assert b9.shape == (44, 9) and b7.shape == (44, 7) and b9.dtype == np.float32 and l9.dtype == np.int64
    assert (l9 == -1).sum() == 3 and l9.max() < 10 and l7.max() < 26
    assert np.array_equal(b9[:, :7], b7)
    lab, _, msk = seg_targets_host(torch.from_numpy(pts), torch.from_numpy(b9), torch.from_numpy(l9), 10)
    assert 0.002 < float(msk.float().mean()) < 0.1
    # the shifted copies (rows 40-43) overlap earlier boxes: some of their points go to the earlier box (first hit wins)
    xyz = torch.from_numpy(pts[:, :3])
    first = points_in_boxes_first_host(xyz, torch.from_numpy(b9[:, :7]))
    copies = torch.cat([points_in_boxes_first_host(xyz, torch.from_numpy(b9[k:k + 1, :7])) == 0 for k in range(40, 44)])
    assert ((first.repeat(4) < 40) & copies).any()


def test_fsf_forward_train_still_raises_and_names_the_new_argument():
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "fsf_nuscenes.py"))
    model = build_model(cfg.model)
    with pytest.raises(NotImplementedError, match="gt_bboxes_3d"):
        model.forward_train([torch.zeros((4, 8))], [dict()])
