"""K35 on the MI355X: the device targets (fsf_seg_targets) against the host restatement bit for bit, the fused CE + L1
(fsf_seg_loss_forward / _backward) against float64 autograd of the reference expression, run-to-run bit equality, no host sync, and
`FSF.forward_train_graph(..., gt_bboxes_3d, gt_labels_3d)` against the host path on the same segmentor outputs.

Tolerances: the losses are fp32 per-row terms summed in fp64, so they match float64 to a relative 1e-6; the gradients are fp32
(softmax - onehot) * scale and sign * scale, within 1e-7 absolute (and 1e-5 relative) of float64."""
import numpy as np
import pytest
import torch

from fullysparsefusion_amd import hip_ops, synthetic
from fullysparsefusion_amd.mmdet3d_plugin.models.decode_heads.segmentation_head import seg_targets_host
from fullysparsefusion_amd.mmdet3d_plugin.registry import build_head
from test_seg_losses_cpu import edge_case

pytestmark = pytest.mark.gpu


def make_head(num_classes, lw):
    return build_head(dict(type="VoteSegHead", in_channel=16, num_classes=num_classes, hidden_dims=[16],
                           loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, class_weight=[1.0] * num_classes + [0.1],
                                            loss_weight=lw),
                           loss_vote=dict(type="L1Loss", loss_weight=1.0)))


def host_targets(samples, bg):
    """Per-sample host restatement on CPU tensors, concatenated."""
    out = [seg_targets_host(torch.from_numpy(p), torch.from_numpy(b), torch.from_numpy(l), bg) for p, b, l in samples]
    return [torch.cat([o[k] for o in out]) for k in range(3)]


def device_targets(samples, bg, device, batch_dtype=torch.int64, order=None):
    head = make_head(bg, 10.0)
    points = torch.cat([torch.from_numpy(p) for p, _, _ in samples]).to(device)
    bidx = torch.cat([torch.full((len(p),), b, dtype=batch_dtype) for b, (p, _, _) in enumerate(samples)]).to(device)
    if order is not None:
        points, bidx = points[order.to(device)], bidx[order.to(device)]
    return head.get_targets_flat(points, bidx, [torch.from_numpy(b) for _, b, _ in samples],
                                 [torch.from_numpy(l) for _, _, l in samples])


def assert_targets_equal(got, want):
    lab, tgt, msk = (t.cpu() for t in got)
    assert torch.equal(lab, want[0])
    assert torch.equal(tgt.view(torch.int32), want[1].view(torch.int32))  # bit for bit
    assert torch.equal(msk, want[2])


def edge_samples():
    """test_seg_losses_cpu's face points (padded to the frame's 8 columns) and boxes."""
    pts, boxes, labels = edge_case()
    return [(np.concatenate([pts, np.zeros((pts.shape[0], 8 - pts.shape[1]), np.float32)], 1), boxes, labels)]


@pytest.mark.parametrize("batch_dtype", [torch.int64, torch.int32])
def test_targets_on_the_10_sweep_frame_equal_the_host_bit_for_bit(device, batch_dtype):
    pts = synthetic.make_frame(num_sweeps=10, seed=0)["points"]
    boxes, labels = synthetic.make_gt_boxes(pts, seed=0)
    samples = [(pts, boxes, labels)]
    want = host_targets(samples, 10)
    got = device_targets(samples, 10, device, batch_dtype)
    assert_targets_equal(got, want)
    assert 0.005 < float(want[2].float().mean()) < 0.1


def test_targets_on_the_av2_frame_equal_the_host_bit_for_bit(device):
    pts = synthetic.make_frame_av2(seed=0)["points"]
    boxes, labels = synthetic.make_gt_boxes(pts, seed=2, box_dim=7, num_classes=26, num_boxes=60, max_range=120.0)
    samples = [(pts, boxes, labels)]
    assert_targets_equal(device_targets(samples, 26, device), host_targets(samples, 26))


def test_targets_batch_with_unequal_boxes_an_empty_sample_edges_and_any_row_order(device):
    a = synthetic.make_frame(num_sweeps=1, seed=1)["points"]
    b = synthetic.make_frame(num_sweeps=1, seed=2)["points"]
    ba, la = synthetic.make_gt_boxes(a, seed=1, num_boxes=30)
    bb, lb = synthetic.make_gt_boxes(b, seed=2, num_boxes=8, num_overlap=2, num_ignored=1)
    samples = [(a, ba, la), (b[:5000], np.zeros((0, 9), np.float32), np.zeros(0, np.int64)), (b, bb, lb)] + edge_samples()
    want = host_targets(samples, 10)
    n = sum(len(s[0]) for s in samples)
    order = torch.randperm(n, generator=torch.Generator().manual_seed(0))
    got = device_targets(samples, 10, device, order=order)
    assert_targets_equal(got, [w[order] for w in want])
    # the count output of K35a
    head = make_head(10, 10.0)
    from fullysparsefusion_amd.mmdet3d_plugin.models.decode_heads.segmentation_head import pack_gt_for_device

    pts = torch.cat([torch.from_numpy(s[0]) for s in samples]).to(device)
    bidx = torch.cat([torch.full((len(s[0]),), i, dtype=torch.int64) for i, s in enumerate(samples)]).to(device)
    box_ptr, boxes, labels = pack_gt_for_device([torch.from_numpy(s[1]) for s in samples], [torch.from_numpy(s[2]) for s in samples],
                                                device)
    _, _, mask, count = hip_ops.seg_targets(pts, bidx, box_ptr, boxes, labels, head.bg_label)
    assert int(count.item()) == int(want[2].sum()) == int(mask.sum().item())
    assert not want[2][len(a):len(a) + 5000].any()


def reference_f64(logits, votes, labels, targets, mask, cw, lw_ce, lw_vote):
    lg = logits.detach().double().requires_grad_()
    vt = votes.detach().double().requires_grad_()
    c = lg.shape[1]
    ce = torch.nn.functional.cross_entropy(lg, labels, weight=torch.tensor(cw, dtype=torch.float64, device=lg.device), reduction="none")
    loss_ce = lw_ce * ce.mean()
    n_valid = int(mask.sum())
    if n_valid:
        v = vt.reshape(-1, c, 3)[mask].reshape(-1, 3)
        idx = torch.arange(n_valid, device=lg.device) * c + labels[mask]
        loss_vote = lw_vote * (v[idx] - targets[mask].double()).abs().mean()
    else:
        loss_vote = vt.sum() * 0
    gl, gv = torch.autograd.grad(loss_ce + 0.5 * loss_vote, (lg, vt))
    return loss_ce.detach(), loss_vote.detach(), gl, gv


def loss_inputs(device, c, n=20000, n_valid_zero=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn((n, 4 * c + 5), generator=g) * 2  # one buffer: logits and votes are strided column views of it
    labels = torch.randint(0, c, (n,), generator=g)
    mask = (labels < c - 1) & (torch.rand(n, generator=g) < 0.6)
    if n_valid_zero:
        mask[:] = False
    targets = torch.randn((n, 3), generator=g) * mask[:, None]
    buf = buf.to(device).requires_grad_()
    logits, votes = buf[:, 1:1 + c], buf[:, 1 + c:1 + 4 * c]
    return buf, logits, votes, labels.to(device), targets.to(device), mask.to(device)


@pytest.mark.parametrize("num_classes,lw", [(10, 10.0), (26, 3.0)])
@pytest.mark.parametrize("n_valid_zero", [False, True])
def test_fused_losses_match_float64_autograd(device, num_classes, lw, n_valid_zero):
    head = make_head(num_classes, lw)
    c = head.num_classes
    buf, logits, votes, labels, targets, mask = loss_inputs(device, c, n_valid_zero=n_valid_zero)
    assert logits.stride(0) == 4 * c + 5 and not logits.is_contiguous()
    got = head.losses(logits, votes, labels, targets, mask)
    want = reference_f64(logits, votes, labels, targets, mask, head.loss_decode.class_weight, lw, 1.0)
    assert abs(float(got["loss_sem_seg"].detach()) - float(want[0])) <= 1e-6 * abs(float(want[0]))
    if n_valid_zero:
        assert float(got["loss_vote"].detach()) == 0.0
    else:
        assert abs(float(got["loss_vote"].detach()) - float(want[1])) <= 1e-6 * abs(float(want[1]))
    gl, gv = torch.autograd.grad(got["loss_sem_seg"] + 0.5 * got["loss_vote"], (logits, votes))
    for g, w in ((gl, want[2]), (gv, want[3])):
        assert torch.isfinite(g).all()
        err = (g.double() - w).abs()
        assert float(err.max()) <= 1e-7 + 1e-5 * float(w.abs().max()), float(err.max())
    if n_valid_zero:
        assert not gv.any()
    else:
        assert int((gv != 0).sum()) == int(torch.count_nonzero(want[3]))  # only the 3 own-class columns of masked rows


def test_fused_losses_are_bit_identical_from_run_to_run(device):
    head = make_head(10, 10.0)
    buf, logits, votes, labels, targets, mask = loss_inputs(device, 11, n=310000, seed=3)
    runs = []
    for _ in range(2):
        out = head.losses(logits, votes, labels, targets, mask)
        g = torch.autograd.grad(out["loss_sem_seg"] + out["loss_vote"], buf)[0]
        runs.append((out["loss_sem_seg"].detach().clone(), out["loss_vote"].detach().clone(), g))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_device_path_never_synchronises(device):
    head = make_head(10, 10.0)
    pts = synthetic.make_frame(num_sweeps=1, seed=4)["points"]
    boxes, labels = synthetic.make_gt_boxes(pts, seed=4)
    points = torch.from_numpy(pts).to(device)
    bidx = torch.zeros(len(pts), dtype=torch.int64, device=device)
    logits = torch.randn((len(pts), 11), device=device, requires_grad=True)
    votes = torch.randn((len(pts), 33), device=device, requires_grad=True)
    dev_boxes = torch.from_numpy(boxes).to(device)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for gt in (torch.from_numpy(boxes), dev_boxes):  # host boxes (one upload) and device boxes
            lab, tgt, msk = head.get_targets_flat(points, bidx, [gt], [torch.from_numpy(labels)])
            out = head.losses(logits, votes, lab, tgt, msk)
            (out["loss_sem_seg"] + out["loss_vote"]).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(logits.grad).all()


@pytest.fixture(scope="module")
def train_graph(device):
    import bench

    torch.manual_seed(0)
    model = bench.build_model(device).train()
    _, inp = bench.make_inputs(1, 3, device, frames=1)
    boxes, labels = synthetic.make_gt_boxes(inp["points"][0].cpu().numpy(), seed=3)
    return model, inp, [torch.from_numpy(boxes)], [torch.from_numpy(labels)]


def test_forward_train_graph_losses_and_gradients_match_the_host_path(train_graph):
    model, inp, gt_boxes, gt_labels = train_graph
    model.zero_grad(set_to_none=True)
    out = model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"], gt_bboxes_3d=gt_boxes,
                                    gt_labels_3d=gt_labels)
    assert set(out["losses"]) == {"loss_sem_seg", "loss_vote"}
    seg, head = out["seg"], model.segmentor.segmentation_head
    lab, tgt, msk = head.get_targets_flat(seg["seg_points"], seg["batch_idx"], gt_boxes, gt_labels, fused=False)
    dlab, dtgt, dmsk = head.get_targets_flat(seg["seg_points"], seg["batch_idx"], gt_boxes, gt_labels)
    assert torch.equal(lab, dlab) and torch.equal(msk, dmsk) and torch.allclose(tgt, dtgt, rtol=0, atol=1e-6)
    assert int(msk.sum()) > 0
    host = head.losses(seg["seg_logits"], seg["seg_vote_preds"], lab, tgt, msk, fused=False)
    for k in ("loss_sem_seg", "loss_vote"):
        a, b = float(out["losses"][k].detach()), float(host[k].detach())
        assert abs(a - b) <= 1e-5 * abs(b), (k, a, b)
    params = [(n, p) for n, p in model.named_parameters()
              if p.requires_grad and (n.startswith("segmentor.") or n.startswith("segmentor_updated_mlp."))]
    assert any(n.startswith("segmentor.backbone.") for n, _ in params)
    fused = torch.autograd.grad(out["losses"]["loss_sem_seg"] + out["losses"]["loss_vote"], [p for _, p in params], retain_graph=True,
                                allow_unused=True)
    ref = torch.autograd.grad(host["loss_sem_seg"] + host["loss_vote"], [p for _, p in params], allow_unused=True)
    missing = [n for (n, _), g in zip(params, fused) if g is None]
    assert missing == [], missing[:10]
    for (n, _), g, r in zip(params, fused, ref):
        assert torch.isfinite(g).all(), n
        assert torch.allclose(g, r, rtol=1e-3, atol=1e-6 * float(r.abs().max()) + 1e-9), (n, float((g - r).abs().max()))


def test_forward_train_graph_without_gt_keeps_its_keys(train_graph):
    model, inp, _, _ = train_graph
    out = model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"])
    keys = {"seg", "frustum_obj_feats", "frustum_obj_centers", "frustum_obj_coors", "frustum_preds_2d", "frustum_obj_result",
            "fsd_obj_feats", "fsd_obj_centers", "fsd_obj_coors", "fsd_obj_result", "stage_results", "obj_centers", "obj_coors",
            "obj_feats", "preds_2d"}
    if model.num_extra_stages > 0:
        keys.add("stage_centers")
    assert set(out) == keys


def test_vote_segmentor_forward_train_as_subsegmentor(train_graph):
    model, inp, gt_boxes, gt_labels = train_graph
    points, _ = model.split_points_last_3dim(inp["points"])
    out = model.segmentor.forward_train(points, inp["img_metas"], gt_boxes, gt_labels, as_subsegmentor=True)
    assert {"seg_points", "seg_logits", "seg_vote_preds", "offsets", "seg_feats", "batch_idx", "losses"} <= set(out)
    assert set(out["losses"]) == {"loss_sem_seg", "loss_vote"}
    assert all(torch.isfinite(v).all() for v in out["losses"].values())
    losses = model.segmentor.forward_train(points, inp["img_metas"], gt_boxes, gt_labels)
    assert set(losses) == {"loss_sem_seg", "loss_vote"}
