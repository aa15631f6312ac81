"""K37 on the device: `fsf_gt_boxes_2d` (boxes, keep flags) and `fsf_hybrid_assign` (labels, targets, weights, assignment, stats)
against the host restatement bit for bit; the fused losses through them against float64 autograd under K36's bounds (losses relative
1e-6, gradients 1e-7 absolute + 1e-5 of the largest float64 gradient); run-to-run identity; no host synchronisation; and the whole
detector with `camera_head_losses=True` (K36's model tolerances: 1e-6 against float64, 1e-5 against the unfused path)."""
import math

import numpy as np
import pytest
import torch

from fullysparsefusion_amd.mmdet3d_plugin.core.assigners import gt_boxes_2d_host
from test_cluster_losses_cpu import NUS_CLASSES, reference_losses_f64
from test_hybrid_assign_cpu import (ASSIGNER_CFG, LOSS_NAMES, frame_case, head_loss, host_targets, loss_case, make_assigner, make_frustum_head, regroup,
                                    targeted_cases)

pytestmark = pytest.mark.gpu
SUFFIX = f"{NUS_CLASSES}"


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def device_targets(head, c, device, gt_on_device, strided):
    """modify_gt_for_single_task (both lists) + get_targets (K37a + K37b) on device queries; the GT on the host (pinned uploads) or on
    the device; the batch index as a column of the [n, 3] query table or on its own."""
    put = (lambda t: t.to(device)) if gt_on_device else (lambda t: t)
    lists = [[put(torch.from_numpy(np.asarray(b, np.float32))) for b, _ in c[key]] for key in ("na", "aug")]
    labs = [[put(torch.from_numpy(np.asarray(l, np.int64))) for _, l in c[key]] for key in ("na", "aug")]
    na = head.modify_gt_for_single_task(lists[0], labs[0], 0)
    au = head.modify_gt_for_single_task(lists[1], labs[1], 0)
    n = len(c["centres"])
    inds = torch.zeros((n, 3), dtype=torch.long)
    inds[:, 0] = torch.from_numpy(c["bidx"])
    inds = inds.to(device)
    metas = [dict(lidar2img=[m for m in l]) for l in c["l2i"]]
    head.task_info = {}
    out = head.get_targets(10, na[0], na[1], au[0], au[1], torch.from_numpy(c["preds"]).to(device), torch.from_numpy(c["centres"]).to(device),
                           inds if strided else inds[:, 0].contiguous(), task_id=0, img_metas_list=metas)
    info = head.task_info["0"]
    stats = [float(info[k]) for k in ("num_preds", "num_pos_preds", "num_gts", "assigned_gts")]
    return list(out[:4]) + [head._last_assignment["assigned"]], stats, head._last_assignment["avg_factors"].cpu().tolist()


def assert_device_equals_host(c, device, code=10):
    want = host_targets(make_assigner(), c["centres"], c["bidx"], c["preds"], c["na"], c["aug"], c["l2i"], code=code)
    for gt_on_device in (False, True):
        for strided in (True, False):
            got, stats, avg = device_targets(make_frustum_head(), c, device, gt_on_device, strided)
            lab, lw, tgt, wgt, asg = (t.cpu() for t in got)
            assert lab.dtype == torch.int64 and torch.equal(lab, want[0])
            assert torch.equal(lw, want[1])
            assert torch.equal(bits(tgt), bits(want[2])) and torch.equal(bits(wgt), bits(want[3]))  # bit for bit
            assert torch.equal(asg.long(), want[4])
            assert stats == want[5][:4].tolist() and avg == want[5][4:].tolist()
    return want


def as_case(seed, box_dim=9):
    boxes, labels, aug, l2i, preds, centres = frame_case(seed, box_dim)
    return dict(centres=centres, bidx=np.zeros(len(centres), np.int64), preds=preds, na=[(boxes[:, :9], labels)], aug=[(aug, labels)],
                l2i=l2i[None])


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_boxes_2d_and_targets_on_a_frame_equal_the_host_bit_for_bit(device, seed):
    from fullysparsefusion_amd import hip_ops_assign

    c = as_case(seed)
    rb, rl = regroup(*c["na"][0])
    want_b, want_k = gt_boxes_2d_host(torch.from_numpy(rb), torch.from_numpy(c["l2i"][0]))
    got_b, got_k = hip_ops_assign.gt_boxes_2d(torch.from_numpy(rb).to(device), torch.from_numpy(rl).int().to(device),
                                              torch.tensor([0, len(rb)], dtype=torch.int32, device=device),
                                              torch.from_numpy(c["l2i"]).float().to(device))
    assert torch.equal(got_k.cpu().bool(), want_k) and int(want_k.sum()) >= 30
    assert torch.equal(bits(got_b.cpu()), bits(want_b))
    want = assert_device_equals_host(c, device)
    assert int((want[4] >= 0).sum()) >= 80


def test_targets_with_the_copy_paste_flag_equal_the_host(device):
    c = as_case(4, box_dim=10)
    assert c["aug"][0][0].shape[1] == 10
    want = host_targets(make_assigner(), c["centres"], c["bidx"], c["preds"], c["na"], c["aug"], c["l2i"])
    head = make_frustum_head()
    na = head.modify_gt_for_single_task([torch.from_numpy(c["na"][0][0])], [torch.from_numpy(c["na"][0][1])], 0)
    au = head.modify_gt_for_single_task([torch.from_numpy(c["aug"][0][0])], [torch.from_numpy(c["aug"][0][1])], 0)
    n = len(c["centres"])
    out = head.get_targets(10, na[0], na[1], au[0], au[1], torch.from_numpy(c["preds"]).to(device), torch.from_numpy(c["centres"]).to(device),
                           torch.zeros(n, dtype=torch.long, device=device), task_id=0, img_metas_list=[dict(lidar2img=list(c["l2i"][0]))])
    assert torch.equal(bits(out[3].cpu()), bits(want[3])) and torch.equal(bits(out[2].cpu()), bits(want[2]))
    assert bool((want[3][:, 8] == 0)[want[0] < 10].any())


def assert_boxes_2d_equal_host(c, device):
    """K37a against `gt_boxes_2d_host`, boxes and keep flags bit for bit, on the regrouped un-augmented list of every sample (the
    whole batch in one call, as the head makes it)."""
    from fullysparsefusion_amd import hip_ops_assign

    lists = [regroup(np.asarray(b, np.float32).reshape(-1, 9), np.asarray(l, np.int64)) for b, l in c["na"]]
    want = [gt_boxes_2d_host(torch.from_numpy(rb), torch.from_numpy(c["l2i"][b])) for b, (rb, _) in enumerate(lists)]
    ptr = np.concatenate([[0], np.cumsum([len(rb) for rb, _ in lists])])
    rows = torch.from_numpy(np.concatenate([rb for rb, _ in lists])).to(device)
    labs = torch.from_numpy(np.concatenate([rl for _, rl in lists])).int().to(device)
    got_b, got_k = hip_ops_assign.gt_boxes_2d(rows, labs, torch.tensor(ptr, dtype=torch.int32, device=device),
                                              torch.from_numpy(c["l2i"]).float().to(device))
    want_b, want_k = torch.cat([w[0] for w in want]), torch.cat([w[1] for w in want])
    assert got_b.shape == want_b.shape and torch.equal(got_k.cpu().bool(), want_k)
    assert torch.equal(bits(got_b.cpu()), bits(want_b))
    return want_b, want_k


@pytest.mark.parametrize("name", sorted(targeted_cases()))
def test_targeted_case_equals_the_host_bit_for_bit(device, name):
    c = targeted_cases()[name]
    boxes_2d, keep = assert_boxes_2d_equal_host(c, device)
    if name in ("straddling_border", "corners_behind_camera", "two_cameras"):
        assert int(keep.sum()) >= (2 if name == "two_cameras" else 1)
    if name == "straddling_border":
        assert float(boxes_2d[0, 0, 0]) == 0.0
    want = assert_device_equals_host(c, device)
    assert want[4].tolist() == list(c["expect"])


def test_extra_height_grows_the_box_in_z_only(device):
    """`PointInBoxAssigner.extra_height` e = 0.4 on the device against `enlarge_box_height` on the host: centres just inside and just
    outside the grown top and bottom faces, and centres just outside the UNGROWN footprint (w and l must not grow)."""
    e = 0.4
    box = np.array([[12.0, 3.0, -1.0, 2.0, 4.0, 1.6, 0.3, 0.5, -0.5]], np.float32)
    c, s = math.cos(0.3), math.sin(0.3)
    centres = [[12.0, 3.0, 0.6 + e - 0.01], [12.0, 3.0, 0.6 + e + 0.01], [12.0, 3.0, -1.0 - e + 0.01], [12.0, 3.0, -1.0 - e - 0.01],
               [12.0 + 2.05 * c, 3.0 + 2.05 * s, 0.0], [12.0 - 1.05 * s, 3.0 + 1.05 * c, 0.0], [12.0 + 1.95 * c, 3.0 + 1.95 * s, 0.7 + e / 2]]
    n = len(centres)
    preds = np.zeros((n, 9), np.float32)
    preds[:, :4] = [1500.0, 800.0, 1510.0, 810.0]  # a 2-D box that overlaps no projection: only the 3-D half can assign
    case = dict(centres=np.array(centres, np.float32), bidx=np.zeros(n, np.int64), preds=preds, na=[(box, np.array([0]))],
                aug=[(box, np.array([0]))], l2i=targeted_cases()["no_gt"]["l2i"])
    cfg = dict(ASSIGNER_CFG, assigner_3d=dict(type="PointInBoxAssigner", extra_height=e))
    want = host_targets(make_assigner(assigner_3d=cfg["assigner_3d"]), case["centres"], case["bidx"], case["preds"], case["na"], case["aug"],
                        case["l2i"])
    assert want[4].tolist() == [0, -1, 0, -1, -1, -1, 0]
    for gt_on_device in (False, True):
        got, stats, _ = device_targets(make_frustum_head(assigner=cfg), case, device, gt_on_device, True)
        assert torch.equal(got[4].cpu().long(), want[4]) and torch.equal(got[0].cpu(), want[0])
        assert torch.equal(bits(got[2].cpu()), bits(want[2])) and stats == want[5][:4].tolist()
    plain, _, _ = device_targets(make_frustum_head(), case, device, False, True)  # e = 0: the grown slabs are outside
    assert plain[4].cpu().tolist() == [-1, -1, -1, -1, -1, -1, -1]


def test_batch_of_two_frames_with_a_strided_batch_column(device):
    a, b = as_case(3), as_case(5)
    c = dict(centres=np.concatenate([a["centres"], b["centres"]]), preds=np.concatenate([a["preds"], b["preds"]]),
             bidx=np.concatenate([np.zeros(len(a["centres"]), np.int64), np.ones(len(b["centres"]), np.int64)]),
             na=a["na"] + b["na"], aug=a["aug"] + b["aug"], l2i=np.concatenate([a["l2i"], b["l2i"]]))
    perm = np.random.default_rng(0).permutation(len(c["bidx"]))  # the samples' queries interleaved
    for k in ("centres", "preds", "bidx"):
        c[k] = np.ascontiguousarray(c[k][perm])
    assert_device_equals_host(c, device)


# ------------------------------------------------------------------------------------------------ losses
def test_fused_losses_match_float64_autograd(device):
    c = loss_case()
    head = make_frustum_head().to(device)
    n = len(c["z"])
    buf = torch.zeros((n, 23))
    buf[:, 1:11], buf[:, 12:22] = c["z"], c["r"]
    buf = buf.to(device).requires_grad_()
    z, r = buf[:, 1:11], buf[:, 12:22]  # column views of one buffer: their own row strides
    out = head_loss(head, c, z, r, fused=True, dev=device)
    boxes, labels, aug, l2i, preds, centres = c["raw"]
    lab, _, tgt, wgt, _, stats = host_targets(make_assigner(), centres, np.zeros(n, np.int64), preds, [(boxes, labels)], [(aug, labels)], l2i[None])
    grads = [1.0, 0.7, 1.3, 0.9, 1.1]
    want, gz, gr = reference_losses_f64(c["z"], c["r"], lab, tgt, wgt, 4.0, 0.25, [1.0, 0.5, 0.5, 0.2, 0.2], True, grads)
    g = torch.autograd.grad(sum(k * out[name + SUFFIX] for k, name in zip(grads, LOSS_NAMES)), buf)[0].cpu()
    figures = {name: abs(float(out[name + SUFFIX].detach()) - float(w)) / abs(float(w)) for name, w in zip(LOSS_NAMES, want)}
    e_cls, e_reg = float((g[:, 1:11].double() - gz).abs().max()), float((g[:, 12:22].double() - gr).abs().max())
    print(f"K37 fused n={n} positives={int(stats[1])}: relative loss errors " + ", ".join(f"{k}={v:.3e}" for k, v in figures.items())
          + f"; grad errors cls {e_cls:.3e} (max |g| {float(gz.abs().max()):.3e}), reg {e_reg:.3e} (max |g| {float(gr.abs().max()):.3e})")
    assert float(stats[1]) >= 40 and [float(out[k + SUFFIX]) for k in ("num_preds", "num_pos_preds", "num_gts", "assigned_gts")] == stats[:4].tolist()
    for name in LOSS_NAMES:
        assert figures[name] <= 1e-6, (name, figures[name])
    assert e_cls <= 1e-7 + 1e-5 * float(gz.abs().max()) and e_reg <= 1e-7 + 1e-5 * float(gr.abs().max())
    assert not g[:, 0].any() and not g[:, 11].any() and not g[:, 22].any()
    unfused = head_loss(head, c, z, r, fused=False, dev=device)
    for name in LOSS_NAMES:
        a, b = float(out[name + SUFFIX].detach()), float(unfused[name + SUFFIX].detach())
        assert abs(a - b) <= 1e-5 * abs(b), name


def test_fused_path_is_bit_identical_from_run_to_run(device):
    c = loss_case(4)
    head = make_frustum_head().to(device)
    z, r = c["z"].to(device).requires_grad_(), c["r"].to(device).requires_grad_()
    runs = []
    for _ in range(2):
        out = head_loss(head, c, z, r, fused=True, dev=device)
        vals = [out[k + SUFFIX] for k in LOSS_NAMES]
        gz, gr = torch.autograd.grad(sum(vals), (z, r))
        runs.append([v.detach().clone() for v in vals] + [gz, gr] + [out[k + SUFFIX].clone() for k in ("num_pos_preds", "assigned_gts")]
                    + [head._last_assignment["assigned"].clone()])
    assert float(runs[0][-3]) >= 40
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(bits(a), bits(b))


def test_device_path_never_synchronises(device):
    c = loss_case(5)
    head = make_frustum_head().to(device)
    z, r = c["z"].to(device).requires_grad_(), c["r"].to(device).requires_grad_()
    xyz, inds, preds = c["xyz"].to(device), c["inds"].to(device), c["preds"].to(device)
    host_gt = (c["na_b"], c["na_l"], c["gt_b"], c["gt_l"])
    dev_gt = tuple([t.to(device) for t in lst] for lst in host_gt)
    dev_metas = [dict(lidar2img=torch.from_numpy(np.stack(c["metas"][0]["lidar2img"])).to(device))]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for gts, metas in ((host_gt, c["metas"]), (dev_gt, dev_metas)):  # host GT + host matrices (pinned uploads), and all on the device
            out = head.loss([z], [r], xyz, inds, *gts, preds, metas)
            sum(out[k + SUFFIX] for k in LOSS_NAMES).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(z.grad).all() and torch.isfinite(r.grad).all() and float(out["num_pos_preds" + SUFFIX]) >= 40


# ------------------------------------------------------------------------------------------------ through the model
@pytest.fixture(scope="module")
def train_graph(device):
    import bench

    torch.manual_seed(0)
    model = bench.build_model(device).train()
    _, inp = bench.make_inputs(1, 3, device, frames=1)
    torch.manual_seed(11)
    with torch.no_grad():
        out = model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"])
    centres = out["frustum_obj_centers"][::20].detach().cpu()
    m = centres.shape[0]
    assert m >= 5, m
    k = torch.arange(m, dtype=torch.float32)
    planted = torch.stack([centres[:, 0], centres[:, 1], centres[:, 2] - 0.75, 1.0 + 0.1 * (k % 5), 1.6 + 0.2 * (k % 3), torch.full((m,), 1.5),
                           0.3 * k - 1.0, 0.1 * k, -0.05 * k], 1)
    # "detections made as above", the other way round: for every 20th query from the 10th on, a thin GT box 15 m down the ray of its
    # 2-D detection's centre, facing the camera, whose projection is that detection
    preds = out["frustum_preds_2d"][10::20].detach().cpu().double()
    l2i = inp["img_metas"][0]["lidar2img"].detach().cpu().double()
    rows = []
    for p in preds:
        cam, d = int(p[6]), 15.0
        u, v, w, h = (p[0] + p[2]) / 2, (p[1] + p[3]) / 2, p[2] - p[0], p[3] - p[1]
        inv = torch.linalg.inv(l2i[cam])
        ctr = inv @ torch.tensor([u * d, v * d, d, 1.0], dtype=torch.float64)
        right = inv @ torch.tensor([(u + 1.0) * d, v * d, d, 1.0], dtype=torch.float64) - ctr  # one pixel to the right, in metres
        down = inv @ torch.tensor([u * d, (v + 1.0) * d, d, 1.0], dtype=torch.float64) - ctr
        width, height = float(right[:3].norm() * w), float(down[:3].norm() * h)
        yaw = math.atan2(float(right[1]), float(right[0])) + math.pi / 2  # the box's WIDTH runs along `right`: its length axis across
        rows.append([float(ctr[0]), float(ctr[1]), float(ctr[2]) - height / 2, width, 0.05, height, yaw, 0.3, -0.2])
    seen = torch.tensor(rows, dtype=torch.float32).reshape(-1, 9)
    boxes = torch.cat([planted, seen])
    labels = torch.arange(boxes.shape[0]) % 10
    return model, inp, [boxes], [labels], m


def test_forward_train_graph_camera_head_losses_match_the_unfused_path(train_graph):
    model, inp, gt_boxes, gt_labels, planted = train_graph
    model.zero_grad(set_to_none=True)
    torch.manual_seed(11)
    out = model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"], gt_bboxes_3d=gt_boxes,
                                    gt_labels_3d=gt_labels, camera_head_losses=True, no_aug_gt_bboxes_3d=gt_boxes, no_aug_gt_labels_3d=gt_labels)
    names = LOSS_NAMES + ["num_preds", "num_pos_preds", "num_gts", "assigned_gts"]
    head = model.frustum_obj_head
    suffix = f"{head.tasks[0]['class_names']}"
    assert set(out["losses"]) == {"loss_sem_seg", "loss_vote"} | {"frustum_" + k + suffix for k in names}
    res = out["frustum_obj_result"]
    args = (out["frustum_obj_centers"], out["frustum_obj_coors"], gt_boxes, gt_labels, gt_boxes, gt_labels, out["frustum_preds_2d"], inp["img_metas"])
    host = head.loss(res["cls_logits"], res["reg_preds"], *args, fused=False)
    assert float(host["num_pos_preds" + suffix]) >= planted
    for k in names[5:]:
        assert float(out["losses"]["frustum_" + k + suffix]) == float(host[k + suffix]), k
    # the 2-D half assigned something the 3-D half did not
    from fullysparsefusion_amd.mmdet3d_plugin.models.dense_heads.cluster_heads import hybrid_targets_host

    na = head.modify_gt_for_single_task(gt_boxes, gt_labels, 0)
    parts = hybrid_targets_host(head.assigner, out["frustum_obj_centers"].cpu(), out["frustum_obj_coors"][:, 0].cpu(), out["frustum_preds_2d"].cpu(),
                                na[0], na[1], na[0], na[1], inp["img_metas"][0]["lidar2img"].cpu()[None], 10, 10, return_parts=True)
    lab, _, tgt, wgt, _, _, per_sample = parts
    only_2d = int(((per_sample[0]["rows_3d"] < 0) & (per_sample[0]["rows_2d"] >= 0)).sum())
    print(f"K37 model: queries {lab.numel()}, positives {int((lab < 10).sum())}, assigned by the 2-D half alone {only_2d}")
    assert only_2d >= 1
    want, _, _ = reference_losses_f64(res["cls_logits"][0].cpu(), res["reg_preds"][0].cpu(), lab, tgt, wgt, 4.0, 0.25, [1.0, 0.5, 0.5, 0.2, 0.2], True)
    for k, w in zip(LOSS_NAMES, want):
        a, b = float(out["losses"]["frustum_" + k + suffix].detach()), float(host[k + suffix].detach())
        print(f"K37 model {k}: fused {a:.9g} unfused {b:.9g} float64 {float(w):.12g}")
        assert abs(a - float(w)) <= 1e-6 * abs(float(w)), k
        assert abs(a - b) <= 1e-5 * abs(b), k
    params = [(n, p) for n, p in model.named_parameters() if p.requires_grad and n.startswith("frustum_obj_head.")]
    assert any(n.startswith("frustum_obj_head.task_heads.0.vel") for n, _ in params) and any("shared_mlp" in n for n, _ in params)
    fused = torch.autograd.grad(sum(out["losses"]["frustum_" + k + suffix] for k in LOSS_NAMES), [p for _, p in params], retain_graph=True,
                                allow_unused=True)
    ref = torch.autograd.grad(sum(host[k + suffix] for k in LOSS_NAMES), [p for _, p in params], allow_unused=True)
    missing = [n for (n, _), g in zip(params, fused) if g is None]
    assert missing == [], missing[:10]
    for (n, _), g, r in zip(params, fused, ref):
        assert torch.isfinite(g).all(), n
        assert torch.allclose(g, r, rtol=1e-3, atol=1e-6 * float(r.abs().max()) + 1e-9), (n, float((g - r).abs().max()))


def test_forward_train_graph_without_the_flag_keeps_todays_keys(train_graph):
    model, inp, gt_boxes, gt_labels, _ = train_graph
    out = model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"], gt_bboxes_3d=gt_boxes,
                                    gt_labels_3d=gt_labels, no_aug_gt_bboxes_3d=gt_boxes, no_aug_gt_labels_3d=gt_labels)
    assert set(out["losses"]) == {"loss_sem_seg", "loss_vote"}
    both = model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"], gt_bboxes_3d=gt_boxes,
                                     gt_labels_3d=gt_labels, lidar_head_losses=True, camera_head_losses=True, no_aug_gt_bboxes_3d=gt_boxes,
                                     no_aug_gt_labels_3d=gt_labels)
    assert any(k.startswith("fsd_loss_cls") for k in both["losses"]) and any(k.startswith("frustum_loss_cls") for k in both["losses"])
    assert "losses" not in model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"])
    with pytest.raises(ValueError, match="no_aug_gt_bboxes_3d"):
        model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"], gt_bboxes_3d=gt_boxes,
                                  gt_labels_3d=gt_labels, camera_head_losses=True)
