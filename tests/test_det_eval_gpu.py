"""The detection-metric kernels (K41, docs/kernels/K41_det_eval.md) against the host specification of mmdet3d_plugin/core/det_eval.py on
the shared cases of tests/det_eval_cases.py (7 samples, 3 classes, every path of the kernels; ties frequent and exact in binary).

Exact: the matched GT row of every prediction at every threshold, the tp counts, npos, the prediction counts and which (class,
threshold) pairs took the `no_predictions` path.  Every other value (curves, AP, TP errors, means, NDS) within 1e-8 relative + 1e-12
absolute in fp64 — derived, not tuned: the only order-dependent step is a prefix sum of at most 2^22 non-negative fp64 terms (error <=
N 2^-53 ~ 5e-10 relative), followed by a handful of correctly rounded operations; a miss means an ordering or interpolation-bracket bug.
Largest error observed on an MI355X: see the figures in docs/kernels/K41_det_eval.md."""
import numpy as np
import pytest
import torch

from det_eval_cases import CLASSES, DIST_THS, case_and_reference
from fullysparsefusion_amd.mmdet3d_plugin.core.det_eval import HEAD, DeviceDetectionEval

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-8, 1e-12
C, T = len(CLASSES), len(DIST_THS)
COUNTS = HEAD + C * (T + 5)  # the result block from here on holds counts and flags: exact


def feed(ev, frames, device):
    """update() frame by frame; `device=None` hands host tensors in."""
    move = (lambda a: torch.from_numpy(a).to(device)) if device is not None else torch.from_numpy
    for f in frames:
        ev.update(dict(boxes_3d=move(f["pred"]), scores_3d=move(f["score"]), labels_3d=move(f["label"]), attrs_3d=move(f["attr"])),
                  move(f["gt"]), move(f["gt_label"]), move(f["gt_attr"]))
    return ev


def compare(got, ref, what):
    match, curves, result = (t.cpu().numpy() for t in got)
    rmatch, rcurves, rresult = ref
    assert np.array_equal(match, rmatch), f"{what}: {(match != rmatch).sum()} of {match.size} matches differ"
    assert np.array_equal(result[COUNTS:], rresult[COUNTS:]), f"{what}: counts / no_predictions flags differ"
    worst = 0.0
    for name, a, b in (("curves", curves, rcurves), ("result", result[:COUNTS], rresult[:COUNTS])):
        assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: {name} NaN pattern"
        err = np.abs(np.nan_to_num(a) - np.nan_to_num(b))
        rel = float((err / np.maximum(np.abs(np.nan_to_num(b)), 1e-300)).max())
        print(f"{what}: {name} max abs err {err.max():.3e}, max rel err {rel:.3e}")
        worst = max(worst, float(err.max()))
        assert np.all(err <= ATOL + RTOL * np.abs(np.nan_to_num(b))), f"{what}: {name} max abs err {err.max():.3e}"
    return worst


@pytest.mark.parametrize("kind,class_range", [("lattice", None), ("continuous", None), ("lattice", (6.0, 9.0, 12.0))])
def test_device_against_the_specification(device, kind, class_range):
    case, ref = case_and_reference(kind, class_range)
    ev = feed(DeviceDetectionEval(CLASSES, DIST_THS, class_range=class_range), case["frames"], device)
    metrics = ev.compute()
    assert ev.last[0].is_cuda and ev.last[0].dtype == torch.int32
    compare(ev.last, ref, f"{kind} range={class_range}")
    rmatch, _, rresult = ref
    assert 0 < (rmatch >= 0).sum() < rmatch.size and metrics["mAP"] == pytest.approx(rresult[0], rel=RTOL)
    if kind == "lattice" and class_range is None:  # the set holds what it is built for
        frames = case["frames"]
        assert rresult[COUNTS + 2] > 0 and rresult[COUNTS + C + 2] == 0  # a class with GT and no predictions
        assert any(f["score"].size > 0 and f["gt_label"].size == 0 for f in frames)  # a sample with predictions and no GT
        assert any(np.isnan(f["gt"][:, 7]).any() for f in frames) and any((f["gt_attr"] < 0).any() for f in frames)
        first = rmatch[:, :frames[0]["score"].size]
        assert (first[3] >= 64).any() and (first[3] >= 128).any()  # GT beyond the first pass of the lanes and the second
        # exact-threshold ties are in the set: a matched distance at a larger threshold that equals a smaller threshold
        pred = np.concatenate([f["pred"] for f in frames]).astype(np.float64)
        gt = np.concatenate([f["gt"] for f in frames]).astype(np.float64)
        hit = rmatch[3] >= 0
        d = np.hypot(*(pred[hit, :2] - gt[rmatch[3][hit], :2]).T)
        assert sum(int((d == th).sum()) for th in DIST_THS[:3]) > 0


def test_two_computes_give_the_same_bits_and_chunking_does_not_matter(device):
    case, ref = case_and_reference("lattice")
    ev = feed(DeviceDetectionEval(CLASSES, DIST_THS), case["frames"], device)
    ev.compute()
    first = [t.clone() for t in ev.last]
    ev.compute()
    for a, b in zip(first, ev.last):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # the same frames handed over from the host, and after a reset: the same result
    other = DeviceDetectionEval(CLASSES, DIST_THS, device=device)
    feed(other, case["frames"][:3], None)
    feed(other, case["frames"][3:], device)
    other.compute()
    for a, b in zip(first, other.last):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    ev.reset()
    feed(ev, case["frames"], device).compute()
    assert torch.equal(first[2].view(torch.uint8), ev.last[2].view(torch.uint8))


def test_update_never_waits_for_the_device(device):
    case, _ = case_and_reference("continuous")
    ev = DeviceDetectionEval(CLASSES, DIST_THS, device=device)
    dev_frames = [{k: torch.from_numpy(v).to(device) for k, v in f.items()} for f in case["frames"]]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        feed(ev, case["frames"], None)  # host inputs
        for f in dev_frames:            # device inputs
            ev.update(dict(boxes_3d=f["pred"], scores_3d=f["score"], labels_3d=f["label"], attrs_3d=f["attr"]), f["gt"], f["gt_label"], f["gt_attr"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert ev.num_samples == 2 * len(case["frames"]) and ev.compute()["mAP"] > 0


def test_a_frame_from_simple_test_agrees_with_the_host_path(device):
    import bench

    model = bench.build_model(device)
    frame = bench.make_inputs(1, 3, device)[1]
    with torch.no_grad():
        res = model.simple_test(frame["points"], frame["img_metas"], frame["mask_data"], frame["mask_anno"])[0]
    boxes = res["boxes_3d"].tensor  # (bbox3d2result hands host tensors out)
    names = list(model.frustum_refined_head[model.num_extra_stages - 1].class_names)
    assert boxes.shape[0] > 20
    # ground truth: every other detection, nudged; the labels as predicted
    gt = boxes[::2].clone()
    gt[:, :2] += 0.3
    gt_labels = res["labels_3d"][::2]
    fused, host = DeviceDetectionEval(names, device=device), DeviceDetectionEval(names, fused=False)
    fused.update(dict(pts_bbox=res), gt.to(device), gt_labels.to(device))
    host.update(res, res["boxes_3d"].__class__(gt.cpu(), box_dim=gt.shape[1]), gt_labels.cpu())
    got, want = fused.compute(), host.compute()
    assert fused.last[0].is_cuda and not host.last[0].is_cuda
    assert torch.equal(fused.last[0].cpu().long(), host.last[0])
    assert want["mAP"] > 0 and got["mAP"] == pytest.approx(want["mAP"], rel=RTOL, abs=ATOL) and got["NDS"] == pytest.approx(want["NDS"], rel=RTOL, abs=ATOL)
    assert fused.as_mmdet3d_dict().keys() == host.as_mmdet3d_dict().keys()
