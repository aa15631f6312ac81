"""GPU: test-time augmentation (K33) — K33a against the host pipeline, the K33a / K33b sign conventions against each other, and
`FSF.aug_test` against `simple_test` and the host merge, with the K32 announcements around it."""
import numpy as np
import pytest
import torch

import bench
from fullysparsefusion_amd import hip_ops
from fullysparsefusion_amd.mmdet3d_plugin.core import bbox as B
from fullysparsefusion_amd.mmdet3d_plugin.datasets import pipelines as D

pytestmark = pytest.mark.gpu

PC_RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
FLIPS4 = [(0.0, 1.0, False, False), (0.0, 1.0, True, False), (0.0, 1.0, False, True), (0.0, 1.0, True, True)]


def _meta(rot, scale, fh, fv):
    return dict(pcd_rot_factor=float(np.float32(rot)), pcd_scale_factor=scale, pcd_horizontal_flip=fh, pcd_vertical_flip=fv)


def _host_aug(pts_cpu, rot, scale, fh, fv, pc_range=PC_RANGE):
    steps = [dict(type="GlobalRotScaleTrans", rot_range=[0, 0], scale_ratio_range=[1.0, 1.0]), dict(type="RandomFlip3D", sync_2d=False)]
    if pc_range is not None:
        steps.append(dict(type="PointsRangeFilter", point_cloud_range=pc_range))
    r = dict(points=D.LiDARPoints(pts_cpu.clone()), **_meta(rot, scale, fh, fv))
    return D.Compose(steps)(r)["points"].tensor


@pytest.fixture(scope="module")
def model(device):
    return bench.build_model(device)


@pytest.fixture(scope="module")
def frame(device):
    return bench.make_inputs(1, 3, device)[1]


def _aug_args(frame, augs, device):
    """Per-augmentation argument lists of aug_test, the clouds made on the host (the Compose route) and uploaded."""
    cpu = frame["points"][0].cpu()
    pts = [[_host_aug(cpu, *a).to(device)] for a in augs]
    metas = [[dict(frame["img_metas"][0], **_meta(*a))] for a in augs]
    return pts, metas, [frame["mask_data"]] * len(augs), [frame["mask_anno"]] * len(augs)


def test_k33a_matches_the_host_pipeline_bit_for_bit(frame, device):
    augs = [(0.0, 1.0, True, False), (0.0, 1.0, False, True), (0.0, 1.0, True, True), (0.0, 0.95, False, False),
            (np.pi / 7, 1.05, False, False), (0.0, 1.0, False, False)]
    pts = frame["points"][0]
    got = hip_ops.augment_points(pts, [D.meta_descriptor(_meta(*a)) for a in augs], PC_RANGE)
    cpu = pts.cpu()
    for a, g in zip(augs, got):
        want = _host_aug(cpu, *a)
        assert g.shape == want.shape and 0 < len(want) < len(cpu) + 1
        assert torch.equal(g.cpu(), want), a


def test_device_point_assembler_augmentations_equal_the_host_compose_route(tmp_path, device):
    rng = np.random.default_rng(5)
    n = 30000
    raw = np.concatenate([rng.uniform(-60, 60, (n, 2)), rng.uniform(-6, 4, (n, 1)), rng.uniform(0, 255, (n, 1)), np.zeros((n, 1))],
                         1).astype(np.float32)
    raw.tofile(tmp_path / "key.bin")
    augs = [_meta(0.0, 1.0, False, False), _meta(0.0, 1.0, True, True), _meta(np.pi / 7, 1.05, True, False)]
    results = dict(pts_filename=str(tmp_path / "key.bin"), timestamp=0.0, sweeps=[])
    dev = D.DevicePointAssembler(load_dim=5, sweeps_num=2, pad_empty_sweeps=True, remove_close=True, point_cloud_range=PC_RANGE,
                                 augmentations=augs)(dict(results), device)
    host = D.Compose([
        dict(type="LoadPointsFromFile", coord_type="LIDAR", load_dim=5, use_dim=[0, 1, 2, 3, 4]),
        dict(type="LoadPointsFromMultiSweeps", sweeps_num=2, use_dim=[0, 1, 2, 3, 4], pad_empty_sweeps=True, remove_close=True),
        dict(type="SaveNoAugPoints")])(dict(results))
    assert len(dev) == len(augs)
    for a, d in zip(augs, dev):
        r = dict(points=D.LiDARPoints(host["points"].tensor.clone()), **a)
        r = D.Compose([dict(type="GlobalRotScaleTrans", rot_range=[0, 0], scale_ratio_range=[1.0, 1.0]),
                       dict(type="RandomFlip3D", sync_2d=False), dict(type="PointsRangeFilter", point_cloud_range=PC_RANGE),
                       dict(type="NormalizePoints")])(r)
        assert torch.equal(d.cpu(), r["points"].tensor), a


def _in_box(pts, boxes):
    """[p, 3] float64 points inside [b, 7+] boxes, the RoI pooling's convention (oracle/refine.py: local frame at yaw + pi / 2)."""
    cx, cy, cz, w, l, h, rz = (boxes[:, i][:, None] for i in range(7))
    rot = rz + np.pi / 2
    dx, dy, dz = pts[None, :, 0] - cx, pts[None, :, 1] - cy, pts[None, :, 2] - (cz + h / 2)
    lx = dx * np.cos(rot) - dy * np.sin(rot)
    ly = dx * np.sin(rot) + dy * np.cos(rot)
    return (np.abs(lx) < l / 2) & (np.abs(ly) < w / 2) & (np.abs(dz) <= h / 2)


def _forward_boxes64(t, rot, scale, fh, fv):
    t = t.copy()
    a = float(np.float32(rot))
    c, s = np.cos(a), np.sin(a)
    pairs = ((0, 1), (7, 8)) if t.shape[1] >= 9 else ((0, 1),)
    for i, j in pairs:
        t[:, i], t[:, j] = t[:, i] * c - t[:, j] * s, t[:, i] * s + t[:, j] * c
    t[:, 6] -= a
    t[:, :6] *= scale
    t[:, 7:] *= scale
    if fh:
        t[:, 1], t[:, 6] = -t[:, 1], -t[:, 6] + np.pi
        if t.shape[1] >= 9:
            t[:, 8] = -t[:, 8]
    if fv:
        t[:, 0], t[:, 6] = -t[:, 0], -t[:, 6]
        if t.shape[1] >= 9:
            t[:, 7] = -t[:, 7]
    return t


@pytest.mark.parametrize("dim", [9, 7])
def test_k33a_and_k33b_sign_conventions_round_trip(device, dim):
    rng = np.random.default_rng(dim)
    nb = 24
    boxes = np.concatenate([(np.arange(nb)[:, None] % 6) * 12.0 - 30 + rng.uniform(-1, 1, (nb, 1)),
                            (np.arange(nb)[:, None] // 6) * 12.0 - 20 + rng.uniform(-1, 1, (nb, 1)), rng.uniform(-2, 0, (nb, 1)),
                            rng.uniform(1, 3, (nb, 1)), rng.uniform(3, 6, (nb, 1)), rng.uniform(1, 2, (nb, 1)),
                            rng.uniform(-3, 3, (nb, 1)), rng.uniform(-5, 5, (nb, 2))], 1)[:, :dim]
    boxes = boxes.astype(np.float32).astype(np.float64)
    # points inside each box (local frame of the pooling convention, inverted), 40 per box
    lx, ly, lz = rng.uniform(-0.4, 0.4, (3, nb, 40))
    rot = boxes[:, 6:7] + np.pi / 2
    px = boxes[:, 0:1] + lx * boxes[:, 4:5] * np.cos(rot) + ly * boxes[:, 3:4] * np.sin(rot)
    py = boxes[:, 1:2] - lx * boxes[:, 4:5] * np.sin(rot) + ly * boxes[:, 3:4] * np.cos(rot)
    pz = boxes[:, 2:3] + boxes[:, 5:6] * (0.5 + lz)
    pts = np.stack([px.ravel(), py.ravel(), pz.ravel()], 1)
    owner = np.repeat(np.arange(nb), 40)
    assert _in_box(pts, boxes)[owner, np.arange(len(pts))].all()
    cloud = torch.from_numpy(np.concatenate([pts, pts], 1).astype(np.float32)).to(device)
    augs = [(0.0, 1.0, True, False), (0.0, 1.0, False, True), (np.pi / 7, 1.05, False, False), (-0.4, 0.95, True, True)]
    got = hip_ops.augment_points(cloud, [D.meta_descriptor(_meta(*a)) for a in augs], None)
    fwd = [_forward_boxes64(boxes, *a) for a in augs]
    for a, g, f in zip(augs, got, fwd):
        gp = g.cpu().double().numpy()
        assert len(gp) == len(pts)
        inside = _in_box(gp[:, :3], f)
        assert inside[owner, np.arange(len(pts))].all(), a  # the augmented points stay in the forward-transformed boxes
    # K33b maps every pass's boxes back onto the originals
    bt = torch.from_numpy(np.concatenate(fwd).astype(np.float32)).to(device)
    m = bt.size(0)
    pidx = torch.from_numpy(np.repeat(np.arange(len(augs)), nb).astype(np.int32)).to(device)
    scores = torch.rand(m, device=device)
    labels = torch.from_numpy(np.arange(m) % 3).to(device)
    out, bnms, st = hip_ops.aug_boxes_map_back(bt, scores, labels, pidx, [D.meta_descriptor(_meta(*a), inverse=True) for a in augs], 4)
    np.testing.assert_allclose(out.cpu().double().numpy(), np.tile(boxes, (len(augs), 1)), atol=1e-5, rtol=2e-6)
    want_nms = B.xywhr2xyxyr(out[:, [0, 1, 3, 4, 6]])
    assert torch.equal(bnms, want_nms)
    st = st.cpu()
    for c in range(4):
        sel = labels.cpu() == c
        assert torch.equal(st[c][sel], scores.cpu()[sel]) and torch.isinf(st[c][~sel]).all()
    for k, (rot, scale, fh, fv) in enumerate(augs):  # host restatement == K33b bit for bit, every pass (flips, scale, rotation)
        host = B.bbox3d_mapping_back(bt[k * nb: (k + 1) * nb].cpu(), scale, fh, fv, float(np.float32(rot)))
        assert torch.equal(host, out[k * nb: (k + 1) * nb].cpu()), (rot, scale, fh, fv)


def _stable_by_score(r):
    o = r["scores_3d"].sort(descending=True, stable=True)[1]
    return r["boxes_3d"].tensor[o], r["scores_3d"][o], r["labels_3d"][o]


def test_aug_test_identity_equals_simple_test(model, frame, device):
    args = (frame["points"], frame["img_metas"], frame["mask_data"], frame["mask_anno"])
    ident = [dict(frame["img_metas"][0], **_meta(0.0, 1.0, False, False))]
    with torch.no_grad():
        ref = model.simple_test(*args)[0]
        # one identity pass, straight into aug_test (forward_test keeps len(points) == 1 on simple_test)
        got = model.aug_test([frame["points"]], [ident], [frame["mask_data"]], [frame["mask_anno"]])[0]
        # two identical identity passes through forward_test's TTA route: every box meets its copy (IoU 1) and the
        # first copy (pass 0, concatenation order) wins the tie, so the merged set is the one-pass set again
        twice = model.forward_test([frame["points"]] * 2, [ident] * 2, [frame["mask_data"]] * 2, [frame["mask_anno"]] * 2)[0]
        with pytest.raises(ValueError):
            model.aug_test([frame["points"]] * 2, [ident] * 2, [frame["mask_data"]] * 2, [frame["mask_anno"]] * 2, hot_path_only=True)
    rb, rs, rl = _stable_by_score(ref)  # the documented order: descending score, ties class-major then concatenation order
    assert len(rb) > 0
    for r in (got, twice):
        assert torch.equal(r["boxes_3d"].tensor, rb) and torch.equal(r["scores_3d"], rs) and torch.equal(r["labels_3d"], rl)
    host = B.merge_aug_bboxes_3d([ref], [ident], model.frustum_refined_head[-1].test_cfg)
    assert torch.equal(host["boxes_3d"].tensor, rb) and torch.equal(host["scores_3d"], rs) and torch.equal(host["labels_3d"], rl)


def _back64(t, rot, scale, fh, fv):
    """bbox3d_mapping_back + the rotation, in float64: undo V flip, H flip, scale, rotation."""
    t = t.copy()
    vel = t.shape[1] >= 9
    if fv:
        t[:, 0], t[:, 6] = -t[:, 0], -t[:, 6]
        if vel:
            t[:, 7] = -t[:, 7]
    if fh:
        t[:, 1], t[:, 6] = -t[:, 1], -t[:, 6] + np.pi
        if vel:
            t[:, 8] = -t[:, 8]
    t[:, :6] /= scale
    t[:, 7:] /= scale
    a = float(np.float32(rot))
    c, s = np.cos(a), np.sin(a)
    for i, j in ((0, 1), (7, 8)) if vel else ((0, 1),):
        t[:, i], t[:, j] = t[:, i] * c + t[:, j] * s, -t[:, i] * s + t[:, j] * c
    t[:, 6] += a
    return t


def _match(dev, host):
    assert len(dev["scores_3d"]) == len(host["scores_3d"])
    db, hb = dev["boxes_3d"].tensor, host["boxes_3d"].tensor
    iou = B.bev_iou_host(B.xywhr2xyxyr(db[:, [0, 1, 3, 4, 6]]), B.xywhr2xyxyr(hb[:, [0, 1, 3, 4, 6]]))
    used = set()
    for i in range(len(db)):
        cand = [j for j in torch.argsort(iou[i], descending=True).tolist()[:4]
                if j not in used and iou[i, j] >= 0.999 and int(dev["labels_3d"][i]) == int(host["labels_3d"][j])
                and abs(float(dev["scores_3d"][i]) - float(host["scores_3d"][j])) <= 1e-6]
        assert cand, i
        used.add(cand[0])


def test_aug_test_four_flips_equals_the_host_merge(device):
    m = bench.build_model(device)
    inp = bench.make_inputs(1, 11, device, trained_like=True)[1]
    bench.calibrate_trained_like(m, inp)
    pts, metas, masks, annos = _aug_args(inp, FLIPS4, device)
    with torch.no_grad():
        per_pass = [m.simple_test(p, mt, mk, an)[0] for p, mt, mk, an in zip(pts, metas, masks, annos)]
        got = m.aug_test(pts, metas, masks, annos)[0]
        again = m.aug_test(pts, metas, masks, annos)[0]
    assert sum(len(r["scores_3d"]) for r in per_pass) > len(got["scores_3d"]) > 0  # boxes overlapped across passes
    # the reference: every pass's simple_test boxes mapped back in float64, then the host merge with nothing left to map back
    ident = dict(pcd_rot_factor=0.0, pcd_scale_factor=1.0, pcd_horizontal_flip=False, pcd_vertical_flip=False)
    mapped = []
    for r, mt in zip(per_pass, metas):
        mt = mt[0]
        t = _back64(r["boxes_3d"].tensor.double().numpy(), mt["pcd_rot_factor"], mt["pcd_scale_factor"], mt["pcd_horizontal_flip"],
                    mt["pcd_vertical_flip"])
        mapped.append(dict(r, boxes_3d=B.LiDARInstance3DBoxes(torch.from_numpy(t).float(), box_dim=t.shape[1])))
    host = B.merge_aug_bboxes_3d(mapped, [ident] * len(mapped), m.frustum_refined_head[-1].test_cfg)
    _match(got, host)
    assert torch.equal(got["boxes_3d"].tensor, again["boxes_3d"].tensor) and torch.equal(got["scores_3d"], again["scores_3d"])


def test_aug_test_keeps_the_callers_announcement(model, frame, device):
    f1 = bench.make_inputs(1, 7, device)[1]
    a1 = (f1["points"], f1["img_metas"], f1["mask_data"], f1["mask_anno"])
    pts, metas, masks, annos = _aug_args(frame, FLIPS4[:2], device)
    with torch.no_grad():
        plain = model.simple_test(*a1)[0]
        model.set_next_frame(*a1)
        announced = model.aug_test(pts, metas, masks, annos)[0]
        # the caller's frame was prefetched under the last pass's box tail ...
        pre = model.__dict__.get("_front_ready")
        assert pre is not None and model._same_frame(pre["key"], model._frame_key(*a1))
        after = model.simple_test(*a1)[0]
        # ... and simple_test took that prefetched front instead of computing its own
        assert model.__dict__.get("_front_hold") is pre
        quiet = model.aug_test(pts, metas, masks, annos, announce=False)[0]
    assert torch.equal(after["boxes_3d"].tensor, plain["boxes_3d"].tensor) and torch.equal(after["scores_3d"], plain["scores_3d"])
    assert torch.equal(announced["boxes_3d"].tensor, quiet["boxes_3d"].tensor) and torch.equal(announced["scores_3d"], quiet["scores_3d"])
