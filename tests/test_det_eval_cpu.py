"""The host specification of the nuScenes detection metrics (K41, docs/kernels/K41_det_eval.md), no GPU: hand-worked cases with their
numbers written out, the `no_predictions` paths, a literal list-and-loop transcription of the published `accumulate` held against the
vectorised specification, the tie rules one by one, the barrier period, the cone / barrier exclusions in NDS, NaN GT velocity through
`cummean`; the C ABI surface and the static guard-band check of the new wrapper module."""
import ast
import os
import re

import numpy as np
import pytest
import torch

from det_eval_cases import CLASSES, DIST_THS, case_and_reference, concatenated
from fullysparsefusion_amd.mmdet3d_plugin.core import DeviceDetectionEval
from fullysparsefusion_amd.mmdet3d_plugin.core import det_eval as de

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = np.linspace(0, 1, 101)


def box(x, y, size=(2.0, 4.0, 1.5), yaw=0.0, v=(0.0, 0.0)):
    return [x, y, 0.0, *size, yaw, *v]


def evaluate(frames, class_names=("car",), **kw):
    """frames: [(pred rows, scores, labels, attrs, gt rows, gt labels, gt attrs)] -> the evaluator (fused=False) after compute()."""
    ev = DeviceDetectionEval(class_names, fused=False, **kw)
    for pred, score, label, attr, gt, gl, ga in frames:
        ev.update(dict(boxes_3d=torch.tensor(pred, dtype=torch.float32).reshape(-1, 9), scores_3d=torch.tensor(score, dtype=torch.float32),
                       labels_3d=torch.tensor(label, dtype=torch.long), attrs_3d=torch.tensor(attr, dtype=torch.long)),
                  torch.tensor(gt, dtype=torch.float32).reshape(-1, 9), torch.tensor(gl, dtype=torch.long), torch.tensor(ga, dtype=torch.long))
    ev.compute()
    return ev


# ------------------------------------------------------------------------------------------------ hand-worked
def test_two_gt_three_predictions_one_miss_by_arithmetic():
    """GT at (0, 0) and (10, 0); A (0.6, 0) score 0.9, B (10, 0.3) score 0.8, C far away score 0.7.
    0.5 m: A misses (0.6), B hits: tp 0 1 1, prec 0 1/2 1/3, rec 0 1/2 1/2 -> precision(x) = x below 0.5, 1/3 at 0.5 (the LARGEST j
    with rec <= x), 0 beyond.  1 / 2 / 4 m: A and B hit: prec 1 1 2/3, rec 1/2 1 1 -> 1 below 1.0, 2/3 at 1.0.
    2 m errors: cummean(0.6, 0.3) = 0.6, 0.45 at confidences 0.9, 0.8; confidence(x) = 0.9 up to 0.5, 0.9 - 0.2 (x - 0.5) to 1, 0.7 at 1."""
    frame = ([box(np.float32(0.6), 0), box(10, np.float32(0.3)), box(50, 50)], [0.9, 0.8, 0.7], [0, 0, 0], [0, 0, 0],
             [box(0, 0), box(10, 0)], [0, 0], [0, 0])
    ev = evaluate([frame])
    match, curves, result = (t.numpy() for t in ev.last)
    assert match.tolist() == [[-1, 1, -1], [0, 1, -1], [0, 1, -1], [0, 1, -1]]
    ap_half = (sum(i * 0.01 - 0.1 for i in range(11, 50)) + (1 / 3 - 0.1)) / 90 / 0.9
    ap_rest = (89 * 0.9 + (2 / 3 - 0.1)) / 90 / 0.9
    aps = ev.metrics["label_aps"]["car"]
    assert aps[0.5] == pytest.approx(ap_half, abs=1e-12) and 0.099 < ap_half < 0.0993
    for th in (1.0, 2.0, 4.0):
        assert aps[th] == pytest.approx(ap_rest, abs=1e-12)
    assert ev.metrics["mAP"] == pytest.approx((ap_half + 3 * ap_rest) / 4, abs=1e-12)
    a, b = float(np.float32(0.6)), float(np.float32(0.3))
    s9, s8, s7 = (float(np.float32(v)) for v in (0.9, 0.8, 0.7))
    conf = np.where(X <= 0.5, s9, s9 + (s8 - s9) / 0.5 * (X - 0.5))
    conf[100] = s7
    assert np.allclose(curves[0, 4 + 2], conf, rtol=0, atol=1e-12)
    cm = [a, (a + b) / 2]
    err = np.where(conf >= s9, cm[0], cm[1] + (cm[0] - cm[1]) / (s9 - s8) * (conf - s8))
    err[100] = cm[1]  # confidence 0.7 lies below every match: the left end
    assert np.allclose(curves[0, 8 + 0], err, rtol=0, atol=1e-12)
    assert ev.metrics["label_tp_errors"]["car"]["trans_err"] == pytest.approx(err[11:].mean(), abs=1e-12)
    assert ev.metrics["label_tp_errors"]["car"]["scale_err"] == 0.0 and ev.metrics["npos"]["car"] == 2


@pytest.mark.parametrize("what", ["no_gt", "no_predictions", "no_match"])
def test_no_predictions_paths(what):
    pred = [] if what == "no_predictions" else [box(0, 0)]
    gt = [] if what == "no_gt" else [box(30 if what == "no_match" else 0, 0)]
    frame = (pred, [0.5] * len(pred), [0] * len(pred), [0] * len(pred), gt, [0] * len(gt), [0] * len(gt))
    ev = evaluate([frame])
    match, curves, result = (t.numpy() for t in ev.last)
    assert np.all(curves[0, :8] == 0) and np.all(curves[0, 8:] == 1)
    assert ev.metrics["mAP"] == 0.0 and all(v == 1.0 for v in ev.metrics["label_tp_errors"]["car"].values())
    assert ev.metrics["NDS"] == 0.0
    none = result[de.HEAD + 4 + 5 + 2 + 4:]
    assert none.tolist() == [1.0] * 4
    md = de.accumulate_host(np.zeros((0, 9)), [], [], [], [], np.zeros((0, 9)), [], [], [], 0, 2.0)
    assert md["no_predictions"] and np.array_equal(de.recall_points(), X)


# ------------------------------------------------------------------------------------------------ the published loop, literally
def accumulate_transcribed(frames, cls, dist_th, period):
    """nuscenes/eval/detection/algo.py::accumulate with lists and loops: boxes are dicts, `gt_boxes[token]` is a frame's GT list."""
    gt_boxes = {k: [dict(name=int(n), row=r.astype(np.float64), attr=int(a)) for r, n, a in zip(f["gt"], f["gt_label"], f["gt_attr"])]
                for k, f in enumerate(frames)}
    pred_all = [dict(token=k, name=int(n), row=r.astype(np.float64), score=float(s), attr=int(a))
                for k, f in enumerate(frames) for r, s, n, a in zip(f["pred"], f["score"], f["label"], f["attr"])]
    npos = len([1 for boxes in gt_boxes.values() for b in boxes if b["name"] == cls])
    empty = dict(tp=[], match=[], precision=np.zeros(101), confidence=np.zeros(101), errors=np.ones((5, 101)), none=True, npos=npos)
    if npos == 0:
        return empty
    pred_boxes_list = [b for b in pred_all if b["name"] == cls]
    pred_confs = [b["score"] for b in pred_boxes_list]
    sortind = [i for (v, i) in sorted((v, i) for (i, v) in enumerate(pred_confs))][::-1]
    tp, fp, conf = [], [], []
    match_data = {k: [] for k in de.TP_METRICS + ("conf",)}
    taken = set()
    for ind in sortind:
        pred_box = pred_boxes_list[ind]
        min_dist, match_gt_idx = np.inf, None
        for gt_idx, gt_box in enumerate(gt_boxes[pred_box["token"]]):
            if gt_box["name"] == cls and (pred_box["token"], gt_idx) not in taken:
                dx, dy = gt_box["row"][0] - pred_box["row"][0], gt_box["row"][1] - pred_box["row"][1]
                this_distance = np.sqrt(dx * dx + dy * dy)
                if this_distance < min_dist:
                    min_dist, match_gt_idx = this_distance, gt_idx
        if min_dist < dist_th:
            taken.add((pred_box["token"], match_gt_idx))
            tp.append(1)
            fp.append(0)
            conf.append(pred_box["score"])
            g = gt_boxes[pred_box["token"]][match_gt_idx]
            for name, v in zip(de.TP_METRICS, de.match_errors(g["row"], pred_box["row"], g["attr"], pred_box["attr"], period)):
                match_data[name].append(v)
            match_data["conf"].append(pred_box["score"])
        else:
            tp.append(0)
            fp.append(1)
            conf.append(pred_box["score"])
    if len(match_data["trans_err"]) == 0:
        return dict(empty, tp=tp)
    flags = list(tp)
    tp, fp, conf = np.cumsum(tp).astype(float), np.cumsum(fp).astype(float), np.array(conf)
    prec, rec = tp / (fp + tp), tp / float(npos)
    prec = np.interp(X, rec, prec, right=0)
    conf = np.interp(X, rec, conf, right=0)
    errors = np.stack([np.interp(conf[::-1], match_data["conf"][::-1], de.cummean(np.array(match_data[k]))[::-1])[::-1] for k in de.TP_METRICS])
    return dict(tp=flags, precision=prec, confidence=conf, errors=errors, none=False, npos=npos)


@pytest.mark.parametrize("kind", ["lattice", "continuous"])
def test_vectorised_specification_agrees_with_the_transcribed_loop(kind):
    case, (match, curves, result) = case_and_reference(kind)
    arrays = concatenated(case)
    pcls = de.effective_class(arrays[0], arrays[2], 3)
    gcls = de.effective_class(arrays[5], arrays[6], 3)
    T = len(DIST_THS)
    none = result[de.HEAD + 3 * (T + 5) + 6 + 3 * T:].reshape(3, T)
    for c in range(3):
        period = np.pi if CLASSES[c] == "barrier" else 2 * np.pi
        for t, th in enumerate(DIST_THS):
            want = accumulate_transcribed(case["frames"], c, th, period)
            md = de.accumulate_host(arrays[0], arrays[1], pcls, arrays[3], arrays[4], arrays[5], gcls, arrays[7], arrays[8], c, th, period)
            if want["npos"] > 0:
                assert (md["match"] >= 0).astype(int).tolist() == want["tp"], (c, th)  # flags exact
            assert md["no_predictions"] == want["none"] == bool(none[c, t])
            assert np.allclose(md["precision"], want["precision"], rtol=0, atol=1e-12) and np.array_equal(md["precision"], curves[c, t])
            assert np.allclose(md["confidence"], want["confidence"], rtol=0, atol=1e-12)
            assert np.allclose(md["errors"], want["errors"], rtol=0, atol=1e-12)
    if kind == "lattice":  # the cases the set is built for are in it
        assert none[2].all() and result[de.HEAD + 3 * (T + 5) + 2] > 0  # class 2: GT and no predictions
        assert 0 < (match >= 0).sum() < match.size and not none[:2].any()


# ------------------------------------------------------------------------------------------------ tie rules
def test_equal_scores_the_later_prediction_is_processed_first():
    """Two predictions of score 0.5: sample 0's hits, sample 1's misses.  The later (the miss) goes first: tp 0 1, prec 0 1/2, rec 0 1 ->
    precision(x) = x / 2.  The other order would give prec 1 1/2 at rec 1 1: precision 1 below x = 1."""
    hit = ([box(0, 0)], [0.5], [0], [0], [box(0, 0)], [0], [0])
    miss = ([box(0, 0)], [0.5], [0], [0], [], [], [])
    ev = evaluate([hit, miss])
    curves = ev.last[1].numpy()
    assert np.allclose(curves[0, 2], X / 2, rtol=0, atol=1e-15)
    assert ev.metrics["label_aps"]["car"][2.0] == pytest.approx(sum(i * 0.01 / 2 - 0.1 for i in range(20, 101)) / 90 / 0.9, abs=1e-12)
    swapped = evaluate([miss, hit])  # now the hit is the later one and goes first
    assert np.all(swapped.last[1].numpy()[0, 2, :100] == 1.0) and swapped.last[1].numpy()[0, 2, 100] == 0.5


def test_two_gt_at_the_same_distance_the_first_is_taken():
    frame = ([box(0, 0), box(0, 0)], [0.9, 0.8], [0, 0], [0, 0], [box(1, 0), box(-1, 0), box(0, 1)], [0, 0, 0], [0, 0, 0])
    ev = evaluate([frame])
    assert ev.last[0].numpy()[2].tolist() == [0, 1]  # then the next of the three equal distances
    reordered = evaluate([(frame[0], frame[1], frame[2], frame[3], [box(0, 1), box(1, 0), box(-1, 0)], [0, 0, 0], [0, 0, 0])])
    assert reordered.last[0].numpy()[2].tolist() == [0, 1]


def test_a_distance_equal_to_the_threshold_is_a_miss():
    frame = ([box(2, 0)], [0.9], [0], [0], [box(0, 0)], [0], [0])
    ev = evaluate([frame])
    assert ev.last[0].numpy()[:, 0].tolist() == [-1, -1, -1, 0]  # 2.0 < 2.0 is false; 4 m matches
    lattice = evaluate([([box(0.25, 0.75), box(3, 4)], [0.9, 0.8], [0, 0], [0, 0], [box(0.25, 0.25), box(0, 0)], [0, 0], [0, 0])])
    assert lattice.last[0].numpy().tolist() == [[-1, -1], [0, -1], [0, -1], [0, -1]]  # 0.5 exactly misses at 0.5; the 3-4-5 pair never matches


# ------------------------------------------------------------------------------------------------ classes
def test_barrier_period_exclusions_in_nds_and_nan_velocity():
    names = ("car", "barrier", "traffic_cone")
    gt = [box(0, 0, yaw=0.0, v=(1.0, 0.0)), box(10, 0, yaw=0.0, v=(np.nan, np.nan)), box(20, 0, yaw=0.0), box(30, 0, yaw=0.0), box(40, 0)]
    pred = [box(0, 0, yaw=np.pi, v=(0.0, 0.0)), box(10, 0, yaw=0.0, v=(5.0, 5.0)), box(20, 0, yaw=np.pi), box(30, 0, yaw=np.pi / 2), box(40, 0, yaw=1.0)]
    labels = [0, 0, 1, 1, 2]
    frame = (pred, [0.9, 0.8, 0.9, 0.8, 0.9], labels, [0, 1, 0, 0, 0], gt, labels, [0, 0, -1, -1, -1])
    ev = evaluate([frame], names)
    m = ev.metrics
    pi32 = float(np.float32(np.pi))
    # car: yaw differences ~pi (full period 2 pi) and 0 -> cummean ~pi, ~pi / 2; barrier (period pi): pi -> 0, pi / 2 -> pi / 2
    car, bar, cone = (m["label_tp_errors"][n] for n in names)
    curves = ev.last[1].numpy()
    wrapped = 2 * np.pi - pi32  # (f32(pi) lies just above pi: the difference wraps)
    assert curves[0, 8 + 2, 50] == pytest.approx(wrapped, abs=1e-12) and curves[0, 8 + 2, 100] == pytest.approx(wrapped / 2, abs=1e-12)
    assert curves[1, 8 + 2, 50] == pytest.approx(abs(de.angle_diff(0.0, pi32, np.pi)), abs=1e-12) and curves[1, 8 + 2, 50] < 1e-6
    assert curves[1, 8 + 2, 100] == pytest.approx(np.float32(np.pi / 2) / 2, abs=1e-6)
    # the second car GT has NaN velocity: cummean skips it, the running mean stays 1.0 (|(1, 0) - (0, 0)|)
    assert np.all(curves[0, 8 + 3] == 1.0) and car["vel_err"] == 1.0
    assert car["attr_err"] == pytest.approx(np.mean(np.where(X[11:] <= 0.5, 0.0, np.nan_to_num(curves[0, 8 + 4, 11:]))), abs=1e-12)
    assert curves[0, 8 + 4, 100] == 0.5 and curves[0, 8 + 4, 50] == 0.0
    # attributes all -1 on barrier / cone GT: cummean of an all-NaN input is ones — and the class excludes the error anyway
    assert np.all(curves[1, 8 + 4] == 1.0) and np.isnan(bar["attr_err"]) and np.isnan(bar["vel_err"]) and not np.isnan(bar["orient_err"])
    assert np.isnan(cone["attr_err"]) and np.isnan(cone["vel_err"]) and np.isnan(cone["orient_err"]) and cone["trans_err"] == 0.0
    want = {"mATE": np.mean([car["trans_err"], bar["trans_err"], cone["trans_err"]]), "mASE": np.mean([car["scale_err"], bar["scale_err"], cone["scale_err"]]),
            "mAOE": np.mean([car["orient_err"], bar["orient_err"]]), "mAVE": car["vel_err"], "mAAE": car["attr_err"]}
    for k, v in want.items():
        assert m[k] == pytest.approx(v, abs=1e-12), k
    nds = (5 * m["mAP"] + sum(max(1 - v, 0.0) for v in want.values())) / 10
    assert m["NDS"] == pytest.approx(nds, abs=1e-12) and want["mAOE"] > 1.0  # (a clamped score is in the sum)
    d = ev.as_mmdet3d_dict()
    assert d["pts_bbox_NuScenes/NDS"] == m["NDS"] and d["pts_bbox_NuScenes/mAP"] == m["mAP"]
    assert d["pts_bbox_NuScenes/car_AP_dist_0.5"] == float(f"{m['label_aps']['car'][0.5]:.4f}") and "pts_bbox_NuScenes/barrier_trans_err" in d
    assert set(k.split("/")[1] for k in d if "/m" in k) == {"mATE", "mASE", "mAOE", "mAVE", "mAAE", "mAP"}


def test_class_range_drops_rows_beyond_it_and_ignored_labels_are_skipped():
    frame = ([box(3, 4), box(30, 40), box(0, 1)], [0.9, 0.8, 0.7], [0, 0, -1], [0, 0, 0], [box(3, 4), box(30, 40), box(0, 1)], [0, 0, -1], [0, 0, 0])
    full = evaluate([frame])
    assert full.metrics["npos"]["car"] == 2 and full.last[0].numpy()[0].tolist() == [0, 1, -1]
    near = evaluate([frame], class_range=dict(car=5.0))  # sqrt(9 + 16) = 5 is not beyond 5
    assert near.metrics["npos"]["car"] == 1 and near.metrics["num_predictions"]["car"] == 1 and near.last[0].numpy()[0].tolist() == [0, -1, -1]
    assert evaluate([frame], class_range=[4.99]).metrics["npos"]["car"] == 0


def test_update_takes_the_pts_bbox_level_boxes_without_velocity_and_resets():
    ev = DeviceDetectionEval(("car",), fused=False)
    res = dict(pts_bbox=dict(boxes_3d=torch.tensor([box(0, 0)[:7]]), scores_3d=torch.tensor([0.5]), labels_3d=torch.tensor([0])))
    ev.update(res, torch.tensor([box(0, 0)[:7]]), torch.tensor([0]))
    m = ev.compute()
    assert m["label_aps"]["car"][0.5] == pytest.approx(1.0, abs=1e-12) and m["label_tp_errors"]["car"]["vel_err"] == 1.0  # (all-NaN: ones)
    ev.reset()
    assert ev.compute()["mAP"] == 0.0 and ev.num_samples == 0
    with pytest.raises(AssertionError):
        DeviceDetectionEval(("car",), dist_th_tp=3.0)


# ------------------------------------------------------------------------------------------------ C ABI surface and guard-band cover
def test_entry_points_are_declared_documented_and_the_abi_version_stays():
    from fullysparsefusion_amd import _lib

    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for name in ("fsf_det_eval_compute", "fsf_det_eval_scratch_bytes", "fsf_det_eval_result_words"):
        assert name in _lib.SIGNATURES and name in doc, name
    assert _lib.DEFINES["FSF_ABI_VERSION"] == 23
    assert _lib.DEFINES["FSF_DET_EVAL_HEAD"] == de.HEAD and _lib.DEFINES["FSF_DET_EVAL_MAX_THRESHOLDS"] >= 4
    P, I32, I64 = _lib.c_p, _lib.c_i32, _lib.c_i64
    assert _lib.SIGNATURES["fsf_det_eval_scratch_bytes"] == ([I64, I64, I64, I32, I32], I64)
    assert _lib.SIGNATURES["fsf_det_eval_result_words"] == ([I32, I32], I64)
    assert _lib.SIGNATURES["fsf_det_eval_compute"] == ([P, P, P, P, P, I64, P, P, P, P, I64, I64, I32, P, P, P, I32, I32, I32, P, P, P, P, P, I64, P], I32)
    assert de.result_words(10, 4) == 8 + 10 * 19
    assert de.class_flags(("car", "barrier", "traffic_cone")) == [0, 1 | 2 << 3 | 2 << 4, 2 << 2 | 2 << 3 | 2 << 4]


def test_the_size_query_measures_the_layout_and_one_byte_short_is_refused_on_the_host():
    """What tests/test_workspace_layout_cpu.py holds the *_workspace_bytes queries to, for this one: the query is the layout struct's
    measure, and the entry refuses a workspace one byte short (and none at all) with FSF_ERR_WORKSPACE before anything reaches HIP:
    every pointer below but the host arrays is an address that is never followed."""
    import ctypes

    from fullysparsefusion_amd import _lib, build

    build.build()
    lib = _lib.lib()
    with open(os.path.join(ROOT, "fullysparsefusion_amd", "csrc", "det_eval.hip")) as f:
        src = f.read()
    body = re.search(r'extern "C" int64_t fsf_det_eval_scratch_bytes\([^)]*\)\s*\{(.*?)\n\}', src, flags=re.S).group(1)
    assert "fsf_layout_bytes<DetEvalLayout>" in body and "fsf_align_up" not in body
    assert src.count("DetEvalLayout") == 4 and "FSF_CARVE(DetEvalLayout" in src  # the struct, its constructor, the query, the carve
    P, G, S, C, T = 1000, 90, 7, 3, 4
    size = int(lib.fsf_det_eval_scratch_bytes(P, G, S, C, T))
    assert size > 0 and size % 256 == 0
    assert lib.fsf_det_eval_scratch_bytes(P + 2048, G, S, C, T) > size > lib.fsf_det_eval_scratch_bytes(0, 0, 0, C, T) > 0
    assert lib.fsf_det_eval_scratch_bytes(1 << 28, G, S, C, T) == 0 and lib.fsf_det_eval_scratch_bytes(-1, G, S, C, T) == 0  # P T >= 2^30
    fake = ctypes.c_void_p(4096)
    flags, ths, params = (ctypes.c_int32 * C)(), (ctypes.c_double * T)(0.5, 1, 2, 4), (ctypes.c_double * 2)(0.1, 5.0)

    def call(ws_bytes, num_pred=P):
        return lib.fsf_det_eval_compute(fake, fake, fake, fake, fake, num_pred, fake, fake, fake, fake, G, S, C, flags, None, ths, T, 2, 11, params,
                                        fake, fake, fake, fake, ws_bytes, None)
    assert call(size - 1) == _lib.DEFINES["FSF_ERR_WORKSPACE"] and call(0) == _lib.DEFINES["FSF_ERR_WORKSPACE"]
    assert call(size, num_pred=1 << 28) == _lib.DEFINES["FSF_ERR_UNSUPPORTED"]


_ALLOCATES = re.compile(r"torch\.empty|empty_like|torch\.zeros|torch\.full|_lib\.workspace\(|_workspace_bytes|_arena_bytes")
_SCRATCH = re.compile(r"_lib\.workspace\(|_workspace_bytes|_arena_bytes")


def test_every_allocating_wrapper_of_the_new_module_has_guard_band_cases():
    import test_guard_bands_eval_gpu as gb
    from fullysparsefusion_amd import hip_ops_eval

    with open(os.path.join(ROOT, "fullysparsefusion_amd", "hip_ops_eval.py")) as f:
        src = f.read()
    alloc, scratch = set(), set()
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef):
            body = ast.get_source_segment(src, node)
            if _ALLOCATES.search(body):
                alloc.add(node.name)
                if _SCRATCH.search(body):
                    scratch.add(node.name)
    assert alloc == {"det_eval"} and scratch == {"det_eval"}
    assert sorted(alloc - set(gb.CASES)) == []
    for name, cases in gb.CASES.items():
        assert hasattr(hip_ops_eval, name)
        kinds = [k for k, _ in cases]
        assert "ragged" in kinds and "minimal" in kinds and "empty" in kinds, name
    assert not re.search(r"torch\.zeros|torch\.full|empty_like|torch\.ones|new_zeros|new_empty|new_full", src)
