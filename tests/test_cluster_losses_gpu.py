"""K36 on the MI355X: the device targets (fsf_cluster_targets) against the host restatement bit for bit, the fused focal + L1 losses
(fsf_cluster_loss_forward / _backward) against float64 autograd of the formulas, run-to-run bit equality, no host sync, and
`FSF.forward_train_graph(..., lidar_head_losses=True)` against the unfused path on the same head outputs.

Tolerances: the project's K35 bounds.  The losses are fp64 terms of the fp32 inputs summed in fp64 and rounded to fp32 once, so they
match float64 to a relative 1e-6; the gradients are fp64 values rounded to fp32 once, within 1e-7 absolute + 1e-5 of the largest
float64 gradient.  Every comparison prints its figures before it asserts (docs/kernels/K36_cluster_losses.md records them).  The
fp32 torch restatement (`fused=False`) is held to test_cluster_losses_cpu's reasoned 1e-5."""
import numpy as np
import pytest
import torch

from fullysparsefusion_amd import synthetic  # noqa: F401
from test_cluster_losses_cpu import (NUS_CLASSES, batch_case, cluster_case, face_case, head_losses_from_targets, loss_inputs, make_head,
                                     reference_losses_f64, regroup_case, restated_targets)

pytestmark = pytest.mark.gpu
AV2_CLASSES = [f"c{i}" for i in range(26)]
LOSS_NAMES = ["loss_cls", "loss_center", "loss_size", "loss_rot", "loss_vel"]


def device_targets(head, xyz, bidx, gts, device, gt_on_device):
    """modify_gt_for_single_task + get_targets (K36a) on device clusters; the GT on the host (one pinned upload) or on the device."""
    put = (lambda t: t.to(device)) if gt_on_device else (lambda t: t)
    gt_b, gt_l = head.modify_gt_for_single_task([put(torch.from_numpy(b)) for b, _ in gts], [put(torch.from_numpy(l)) for _, l in gts], 0)
    head.task_info = {}
    out = head.get_targets(len(head.tasks[0]["class_names"]), xyz.to(device), bidx.to(device), gt_b, gt_l, None, 0)
    info = head.task_info["0"]
    stats = [float(info[k]) for k in ("num_preds", "num_pos_preds", "num_gts", "assigned_gts")]
    return list(out[:4]) + [head._last_assignment["assigned"]], np.array(stats), head._last_assignment["avg_factors"].cpu()


def assert_device_targets_equal_host(head_kwargs, xyz, bidx, gts, device):
    want, want_info = restated_targets(make_head(**head_kwargs), xyz, bidx, gts)
    for gt_on_device in (False, True):
        got, info, avg = device_targets(make_head(**head_kwargs), xyz, bidx, gts, device, gt_on_device)
        lab, lw, tgt, wgt, asg = (t.cpu() for t in got)
        assert lab.dtype == torch.int64 and torch.equal(lab, want[0])
        assert torch.equal(lw, want[1])
        assert torch.equal(tgt.view(torch.int32), want[2].view(torch.int32))  # bit for bit
        assert torch.equal(wgt.view(torch.int32), want[3].view(torch.int32))
        assert torch.equal(asg.long(), want[4])
        assert np.array_equal(info, want_info), (info, want_info)
        assert avg.tolist() == [want_info[0], want_info[1]]
    return want, want_info


@pytest.mark.parametrize("seed,num_sweeps", [(3, 1), (4, 1), (3, 10)])
def test_targets_on_a_frame_equal_the_host_bit_for_bit(device, seed, num_sweeps):
    centres, boxes, labels = cluster_case(seed, num_sweeps)
    xyz, bidx = torch.from_numpy(centres), torch.zeros(len(centres), dtype=torch.long)
    _, info = assert_device_targets_equal_host({}, xyz, bidx, [(boxes, labels)], device)
    assert info[1] >= 300 and info[3] < info[2]


def test_targets_batch_with_an_empty_sample_flags_and_a_strided_batch_column(device):
    xyz, bidx, gts = batch_case()
    xyz, bidx = torch.from_numpy(xyz), torch.from_numpy(bidx)
    want, _ = assert_device_targets_equal_host({}, xyz, bidx, gts, device)
    # the batch column of the [n, 3] cluster index table as it lies (row stride 3), and an int32 column
    head = make_head()
    inds = torch.zeros((len(xyz), 3), dtype=torch.long)
    inds[:, 1] = bidx
    for col in (inds.to(device)[:, 1], bidx.to(device).int()):
        gt_b, gt_l = head.modify_gt_for_single_task([torch.from_numpy(b) for b, _ in gts], [torch.from_numpy(l) for _, l in gts], 0)
        head.task_info = {}
        out = head.get_targets(10, xyz.to(device), col, gt_b, gt_l, None, 0)
        assert torch.equal(out[0].cpu(), want[0]) and torch.equal(out[2].cpu().view(torch.int32), want[2].view(torch.int32))


def test_targets_argoverse_form_equal_the_host_bit_for_bit(device):
    centres, boxes, labels = cluster_case(2, av2=True, num_classes=26)
    xyz, bidx = torch.from_numpy(centres), torch.zeros(len(centres), dtype=torch.long)
    kwargs = dict(class_names=AV2_CLASSES, code_size=8, gamma=1.0, cls_weight=4.0, loss_vel=False)
    _, info = assert_device_targets_equal_host(kwargs, xyz, bidx, [(boxes, labels)], device)
    assert info[1] >= 300


def test_targets_without_clusters_without_positives_on_faces_and_regrouped(device):
    _, boxes, labels = cluster_case(3, 1)
    zero = torch.zeros(0, dtype=torch.long)
    assert_device_targets_equal_host({}, torch.zeros((0, 3)), zero, [(boxes, labels)], device)
    far = torch.full((64, 3), 500.0) + torch.arange(64)[:, None]
    _, info = assert_device_targets_equal_host({}, far, torch.zeros(64, dtype=torch.long), [(boxes, labels)], device)
    assert list(info) == [64, 0, 41, 0]
    centres, fboxes, flabels = face_case()
    xyz, bidx = torch.from_numpy(centres), torch.zeros(len(centres), dtype=torch.long)
    want, _ = assert_device_targets_equal_host({}, xyz, bidx, [(fboxes, flabels)], device)
    assert 0 < int((want[0] < 10).sum()) < len(centres)
    assert_device_targets_equal_host(dict(enlarge_width=0.05), xyz, bidx, [(fboxes, flabels)], device)
    centres, rboxes, rlabels = regroup_case()
    xyz, bidx = torch.from_numpy(centres), torch.zeros(len(centres), dtype=torch.long)
    want, info = assert_device_targets_equal_host(dict(task_names=["car", "pedestrian", "truck"]), xyz, bidx, [(rboxes, rlabels)], device)
    assert info[2] == 3 and int(want[4].max()) <= 2


# ------------------------------------------------------------------------------------------------ losses
def strided_inputs(device, c, code, n, seed=0, no_pos=False, scale=2.0):
    """loss_inputs with cls_logits / reg_preds as column views of one wider buffer (their own row strides)."""
    cls_logits, reg_preds, labels, targets, weights = loss_inputs(c, code, n=n, seed=seed, no_pos=no_pos, scale=scale)
    buf = torch.zeros((n, c + code + 3))
    buf[:, 1:1 + c], buf[:, 2 + c:2 + c + code] = cls_logits, reg_preds
    buf = buf.to(device).requires_grad_()
    return buf, buf[:, 1:1 + c], buf[:, 2 + c:2 + c + code], labels.to(device), targets.to(device), weights.to(device)


def check_losses_against_float64(head, device, c, code, gamma, weights5, n, no_pos, fused, loss_tol, tag):
    buf, z, r, labels, targets, weights = strided_inputs(device, c, code, n, no_pos=no_pos)
    assert not z.is_contiguous()
    got = head_losses_from_targets(head, z, r, labels, targets, weights, fused=fused)
    names = LOSS_NAMES[:5 if code == 10 else 4]
    grads = [1.0, 0.7, 1.3, 0.9, 1.1][:len(names)]
    want, gz, gr = reference_losses_f64(z.cpu(), r.cpu(), labels.cpu(), targets.cpu(), weights.cpu(), gamma, 0.25, weights5, code == 10, grads)
    g = torch.autograd.grad(sum(k * got[name] for k, name in zip(grads, names)), buf)[0].cpu()
    g_cls, g_reg = g[:, 1:1 + c], g[:, 2 + c:2 + c + code]
    figures = {}
    for name, w in zip(names, want):
        a = float(got[name].detach())
        figures[name] = abs(a - float(w)) / abs(float(w)) if float(w) != 0 else abs(a)
    e_cls, e_reg = float((g_cls.double() - gz).abs().max()), float((g_reg.double() - gr).abs().max())
    print(f"K36 {tag} fused={fused} n={n} C={c} code={code} gamma={gamma} no_pos={no_pos}: relative loss errors "
          + ", ".join(f"{k}={v:.3e}" for k, v in figures.items())
          + f"; grad errors cls {e_cls:.3e} (max |g| {float(gz.abs().max()):.3e}), reg {e_reg:.3e} (max |g| {float(gr.abs().max()):.3e})")
    for name, w in zip(names, want):
        if no_pos and name != "loss_cls":
            assert float(got[name].detach()) == 0.0
        else:
            assert figures[name] <= loss_tol, (name, figures[name])
    assert torch.isfinite(g).all()
    assert e_cls <= 1e-7 + 1e-5 * float(gz.abs().max())
    assert e_reg <= 1e-7 + 1e-5 * float(gr.abs().max())
    if no_pos:
        assert not g_reg.any()
    else:
        assert int((g_reg != 0).sum()) == int(torch.count_nonzero(gr))  # only weighted columns of positive rows
    assert not g[:, 0].any() and not g[:, 1 + c].any() and not g[:, 2 + c + code:].any()  # the buffer's other columns


@pytest.mark.parametrize("form", ["nuscenes", "av2"])
@pytest.mark.parametrize("no_pos", [False, True])
@pytest.mark.parametrize("n", [3328, 50000])
def test_fused_losses_match_float64_autograd(device, form, no_pos, n):
    if form == "nuscenes":
        head, c, code, gamma, w5 = make_head(), 10, 10, 4.0, [1.0, 0.5, 0.5, 0.2, 0.2]
    else:
        head, c, code, gamma, w5 = make_head(AV2_CLASSES, code_size=8, gamma=1.0, cls_weight=4.0, loss_vel=False), 26, 8, 1.0, [4.0, 0.5, 0.5, 0.2, 0.2]
    check_losses_against_float64(head, device, c, code, gamma, w5, n, no_pos, True, 1e-6, form)


def test_unfused_restatement_on_the_same_gpu_for_the_record(device):
    """The fp32 torch restatement against the same float64 values (its reasoned bound, 1e-5): the figure the fused path is compared with."""
    check_losses_against_float64(make_head(), device, 10, 10, 4.0, [1.0, 0.5, 0.5, 0.2, 0.2], 3328, False, False, 1e-5, "nuscenes")


def test_extreme_logits_give_finite_losses_and_gradients(device):
    head = make_head()
    buf, z, r, labels, targets, weights = strided_inputs(device, 10, 10, 2048, seed=2)
    with torch.no_grad():
        sign = torch.where(torch.rand((2048, 10), device=device) < 0.5, -1.0, 1.0)
        buf[:, 1:11] = 80.0 * sign
    got = head_losses_from_targets(head, z, r, labels, targets, weights, fused=True)
    g = torch.autograd.grad(sum(got[k] for k in LOSS_NAMES), buf)[0]
    assert all(torch.isfinite(got[k]) for k in LOSS_NAMES) and torch.isfinite(g).all()
    want, gz, _ = reference_losses_f64(z.cpu(), r.cpu(), labels.cpu(), targets.cpu(), weights.cpu(), 4.0, 0.25, [1.0, 0.5, 0.5, 0.2, 0.2], True)
    assert abs(float(got["loss_cls"].detach()) - float(want[0])) <= 1e-6 * float(want[0]) and float(want[0]) > 1.0
    assert float((g[:, 1:11].cpu().double() - gz).abs().max()) <= 1e-7 + 1e-5 * float(gz.abs().max())


def test_fused_path_is_bit_identical_from_run_to_run(device):
    centres, boxes, labels = cluster_case(3, 1)
    head = make_head()
    n = len(centres)
    xyz = torch.from_numpy(centres).to(device)
    inds = torch.zeros((n, 3), dtype=torch.long, device=device)
    z = torch.randn((n, 10), device=device, requires_grad=True)
    r = torch.randn((n, 10), device=device, requires_grad=True)
    runs = []
    for _ in range(2):
        out = head.loss([z], [r], xyz, inds, [torch.from_numpy(boxes)], [torch.from_numpy(labels)])
        vals = [out[k + f"{NUS_CLASSES}"] for k in LOSS_NAMES]
        gz, gr = torch.autograd.grad(sum(vals), (z, r))
        runs.append([v.detach().clone() for v in vals] + [gz, gr] + [out[k + f"{NUS_CLASSES}"].clone() for k in ("num_pos_preds", "assigned_gts")])
    assert float(runs[0][-2]) >= 300
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_device_path_never_synchronises(device):
    xyz_np, bidx_np, gts = batch_case()
    head = make_head()
    n = len(xyz_np)
    xyz = torch.from_numpy(xyz_np).to(device)
    inds = torch.zeros((n, 3), dtype=torch.long, device=device)
    inds[:, 1] = torch.from_numpy(bidx_np).to(device)
    z = torch.randn((n, 10), device=device, requires_grad=True)
    r = torch.randn((n, 10), device=device, requires_grad=True)
    host_gt = ([torch.from_numpy(b) for b, _ in gts], [torch.from_numpy(l) for _, l in gts])
    dev_gt = ([b.to(device) for b in host_gt[0]], [l.to(device) for l in host_gt[1]])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for gt_b, gt_l in (host_gt, dev_gt):  # host GT (one pinned upload) and device GT (regrouped where it is)
            out = head.loss([z], [r], xyz, inds, gt_b, gt_l)
            sum(out[k + f"{NUS_CLASSES}"] for k in LOSS_NAMES).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(z.grad).all() and torch.isfinite(r.grad).all() and float(out["num_pos_preds" + f"{NUS_CLASSES}"]) >= 300


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
    centres = out["fsd_obj_centers"][::20].detach().cpu()
    m = centres.shape[0]
    assert m >= 5, m
    k = torch.arange(m, dtype=torch.float32)
    boxes = torch.stack([centres[:, 0], centres[:, 1], centres[:, 2] - 0.75, 1.0 + 0.1 * (k % 5), 1.6 + 0.2 * (k % 3), torch.full((m,), 1.5),
                         0.3 * k - 1.0, 0.1 * k, -0.05 * k], 1)
    return model, inp, [boxes], [(torch.arange(m) % 10)]


def test_forward_train_graph_lidar_head_losses_match_the_unfused_path(train_graph):
    model, inp, gt_boxes, gt_labels = train_graph
    model.zero_grad(set_to_none=True)
    torch.manual_seed(11)
    out = model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"], gt_bboxes_3d=gt_boxes,
                                    gt_labels_3d=gt_labels, lidar_head_losses=True)
    names = LOSS_NAMES + ["num_preds", "num_pos_preds", "num_gts", "assigned_gts"]
    suffix = f"{model.bbox_head.tasks[0]['class_names']}"  # (the config's class order)
    assert set(out["losses"]) == {"loss_sem_seg", "loss_vote"} | {"fsd_" + k + suffix for k in names}
    head = model.bbox_head
    res = out["fsd_obj_result"]
    host = head.loss(res["cls_logits"], res["reg_preds"], out["fsd_obj_centers"], out["fsd_obj_coors"], gt_boxes, gt_labels, fused=False)
    assert float(host["num_pos_preds" + suffix]) > 0
    for k in names[5:]:
        assert float(out["losses"]["fsd_" + k + suffix]) == float(host[k + suffix]), k
    # float64 values of the same head outputs on the same targets
    labels, _, tgt, wgt, _ = head.get_targets(10, out["fsd_obj_centers"], out["fsd_obj_coors"][:, 1],
                                              *head.modify_gt_for_single_task(gt_boxes, gt_labels, 0), None, 0)
    want, _, _ = reference_losses_f64(res["cls_logits"][0].cpu(), res["reg_preds"][0].cpu(), labels.cpu(), tgt.cpu(), wgt.cpu(), 4.0, 0.25,
                                      [1.0, 0.5, 0.5, 0.2, 0.2], True)
    for k, w in zip(LOSS_NAMES, want):
        a, b = float(out["losses"]["fsd_" + k + suffix].detach()), float(host[k + suffix].detach())
        print(f"K36 model {k}: fused {a:.9g} unfused {b:.9g} float64 {float(w):.12g}")
        assert abs(a - float(w)) <= 1e-6 * abs(float(w)), k
        assert abs(a - b) <= 1e-5 * abs(b), k
    params = [(n, p) for n, p in model.named_parameters() if p.requires_grad and (n.startswith("bbox_head.") or n.startswith("backbone."))]
    assert any(n.startswith("backbone.") for n, _ in params) and any(n.startswith("bbox_head.task_heads.0.vel") for n, _ in params)
    fused = torch.autograd.grad(sum(out["losses"]["fsd_" + k + suffix] for k in LOSS_NAMES), [p for _, p in params], retain_graph=True,
                                allow_unused=True)
    ref = torch.autograd.grad(sum(host[k + suffix] for k in LOSS_NAMES), [p for _, p in params], allow_unused=True)
    missing = [n for (n, _), g in zip(params, fused) if g is None]
    assert missing == [], missing[:10]
    for (n, _), g, r in zip(params, fused, ref):
        assert torch.isfinite(g).all(), n
        assert torch.allclose(g, r, rtol=1e-3, atol=1e-6 * float(r.abs().max()) + 1e-9), (n, float((g - r).abs().max()))


def test_forward_train_graph_without_the_flag_keeps_todays_keys(train_graph):
    model, inp, gt_boxes, gt_labels = train_graph
    out = model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"], gt_bboxes_3d=gt_boxes,
                                    gt_labels_3d=gt_labels)
    assert set(out["losses"]) == {"loss_sem_seg", "loss_vote"}
    assert "losses" not in model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"])
    with pytest.raises(ValueError, match="lidar_head_losses"):
        model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"], lidar_head_losses=True)
