"""Inputs and criteria of the batched / degenerate-frame inference tests (tests/test_oracle_degenerate_cpu.py on the CPU,
tests/test_batch_inference_gpu.py on the device).  A plain module: no fixtures, no test collection.

A sample is the tuple (points8, mask_data, mask_anno, lidar2img) of CPU tensors `oracle.modules.simple_test` takes.
"""
import contextlib

import numpy as np
import torch

from e2e_matching import E2E_MAX_UNMATCHED, E2E_MIN_MATCHED_FRACTION, match_boxes
from fullysparsefusion_amd import synthetic
from oracle import modules as omod

NEAR_THRESHOLD_MARGIN = 1e-5  # tests/test_fullsize_gpu.py::test_final_boxes_vs_oracle_chain: below it an NMS decision may flip in fp32


def _sample(points, mask, anno, lidar2img):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in (points, mask, anno, lidar2img))


def sample_a():
    """The 1-sweep frame every single-sample test uses: 31 k points, 250 painted instances, the default calibration."""
    f = synthetic.make_frame(num_sweeps=1, seed=0)
    return _sample(f["points"], f["mask_data"], f["mask_anno"], f["lidar2img"])


def sample_b():
    """A sample that shares NO per-sample input with `sample_a`: another cloud (seed 97) of another length (its first 20 000
    points), its own masks and `mask_anno` rows (another generator; 200 painted instances + 50 rows of the loader's zero padding,
    so the row count stacks with A's 250), its own calibration (focal length and principal point)."""
    pts = synthetic.make_points(1, seed=97)[:20000]
    mask, anno = synthetic.make_mask_data(np.random.default_rng(97 + 7000), painted=200)
    return _sample(pts, mask, anno, synthetic.make_lidar2img(6, fx=1100.0, cx=760.0, cy=430.0))


def cross_wired(a, b):
    """B with ONE of its per-sample inputs replaced by A's: what a detector computes for sample 1 when it reads `mask_data[0]`,
    `mask_anno[0]` or `img_metas[0]["lidar2img"]` for every sample."""
    return dict(masks_of_a=(b[0], a[1], b[2], b[3]), anno_of_a=(b[0], b[1], a[2], b[3]), lidar2img_of_a=(b[0], b[1], b[2], a[3]))


def half(sample, side, gap=3.0):
    """The points of `sample` with y beyond +-gap (side = +1 / -1): two such halves of opposite sides are farther apart than any
    `connected_dist`, so no connected component spans them and a batch of the two decides nothing jointly."""
    pts = sample[0]
    keep = pts[:, 1] * side > gap
    return (pts[keep].contiguous(),) + tuple(sample[1:])


def degenerate_samples(a):
    """name -> sample; each enters the empty branch it is named for (asserted on the oracle's intermediates by the tests)."""
    pts, mask, anno, L = a
    out = dict(
        zeroed_masks=(pts[:5000].contiguous(), torch.zeros_like(mask), anno, L),   # no 2-D detection at all
        points_300=(pts[:300].contiguous(), mask, anno, L),                        # a sensor drop-out: 300 returns
        one_point=(pts[:1].contiguous(), mask, anno, L),
    )
    # masks present, but no point projects into any: the instances are painted into the top 40 image rows, above the highest beam
    # (10.67 degrees over the horizon: v ~ cy - fy * tan(10.67 deg) = 211) — the tests assert that no point gets an id
    sky = torch.zeros_like(mask)
    sky[:, :, :40, :] = mask[:, :, 400:440, :]
    out["masks_in_the_sky"] = (pts[:5000].contiguous(), sky, anno, L)
    return out


# ------------------------------------------------------------------------------------------------ criteria
def criterion_a(got, want):
    """Criterion (a): tests/test_e2e_agreement_gpu.py's matching and its frozen thresholds between two (boxes [n, >=7], scores,
    labels) results.  Returns (passes, report)."""
    gb, gs, gl = (np.asarray(t) for t in got)
    ob, os_, ol = (np.asarray(t) for t in want)
    pairs, iou, ds = match_boxes(gb, gs, gl, ob, os_, ol)
    good = (iou >= 0.99) & (ds <= 1e-3)
    n = max(gb.shape[0], ob.shape[0])
    report = dict(boxes=int(gb.shape[0]), oracle_boxes=int(ob.shape[0]), matched=int(len(pairs)), matched_iou99_dscore1e3=int(good.sum()),
                  unmatched=int(gb.shape[0] - len(pairs)), unmatched_oracle=int(ob.shape[0] - len(pairs)),
                  min_matched_iou=float(iou.min()) if len(iou) else None, max_dscore=float(ds.max()) if len(ds) else None)
    ok = (gb.shape[0] == ob.shape[0] > 0 and good.sum() >= E2E_MIN_MATCHED_FRACTION * n
          and report["unmatched"] <= E2E_MAX_UNMATCHED and report["unmatched_oracle"] <= E2E_MAX_UNMATCHED)
    return bool(ok), report


def oracle_result(o):
    return o["boxes"].numpy(), o["scores"].numpy(), o["labels"].numpy()


def device_result(r):
    return r["boxes_3d"].tensor.cpu().numpy(), r["scores_3d"].cpu().numpy(), r["labels_3d"].cpu().numpy()


def few_boxes_rule(got, o):
    """The rule of test_final_boxes_vs_oracle_chain for results too small for criterion (a)'s fractions: with the oracle's NMS
    margin above 1e-5 the rows are the oracle's (labels equal, scores and boxes within 1e-6 of the scale, `close` of that test);
    otherwise every returned box is one of the decoded candidates.  Returns which of the two was asserted."""
    gb, gs, gl = got
    if o["margin"] > NEAR_THRESHOLD_MARGIN:
        ob, os_, ol = oracle_result(o)
        assert gb.shape[0] == ob.shape[0], (gb.shape, ob.shape)
        np.testing.assert_array_equal(gl, ol)
        for g, w in ((gs, os_), (gb, ob)):
            if w.size:
                assert float(np.abs(g - w).max()) <= 1e-6 * max(1.0, float(np.abs(w).max())), float(np.abs(g - w).max())
        return "exact"
    dec = o["all_boxes"].numpy()
    if gb.shape[0]:
        d = np.abs(gb[:, None, :7] - dec[None, :, :7]).max(-1)
        assert float(d.min(1).max()) < 1e-5
    return "candidates"


@contextlib.contextmanager
def background_only(*models):
    """Every point's class scores under every group's threshold: +30 on the background logit's bias (an in-place write on the
    parameter: its version counter moves, so weights a model prepared from it are prepared again)."""
    saved = []
    with torch.no_grad():
        for m in models:
            bias = m.segmentor.segmentation_head.conv_seg.bias
            saved.append((bias, bias.detach().clone()))
            bias[-1] += 30.0
    try:
        yield
    finally:
        with torch.no_grad():
            for bias, old in saved:
                bias.copy_(old)


def assert_inputs_discriminate(cpu, a, b):
    """The oracle's [A, B] answers, and the proof that criterion (a) can fail on them: (truth, {wrong wiring: boxes still agreeing})."""
    with torch.no_grad():
        truth = omod.simple_test_batch(cpu, [a, b])
        wrong = {k: omod.simple_test_batch(cpu, [a, s], only=[1])[1] for k, s in cross_wired(a, b).items()}
    for o in truth:
        assert o["margin"] > NEAR_THRESHOLD_MARGIN and o["boxes"].shape[0] > 100
        assert o["s2"]["obj_coors"].shape[0] > 0 and not o["s2"]["fake"] and o["s3"]["cluster_inds"].shape[0] > 0
    want = oracle_result(truth[1])
    ok, rep = criterion_a(want, want)
    assert ok, rep
    wrong["result_of_a"] = truth[0]
    report = {}
    for k, o in wrong.items():
        ok, rep = criterion_a(oracle_result(o), want)
        report[k] = f"{rep['matched_iou99_dscore1e3']} of {rep['oracle_boxes']}"
        assert not ok, (k, rep)
    return truth, report
