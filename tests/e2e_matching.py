"""Box matching and the frozen end-to-end agreement thresholds, shared by tests/test_e2e_agreement_gpu.py (one sample) and
tests/test_batch_inference_gpu.py (batches, degenerate frames).  A plain module: no fixtures, no test collection."""
import numpy as np

from oracle import refine as orefine


def _xyxyr(b):
    b = np.asarray(b, dtype=np.float64)
    return np.stack([b[:, 0] - b[:, 3] / 2, b[:, 1] - b[:, 4] / 2, b[:, 0] + b[:, 3] / 2, b[:, 1] + b[:, 4] / 2, b[:, 6]], 1)


def _pair_iou(a, b):
    """Rotated BEV IoU of a[i] with b[i] (float64 polygon intersection, oracle/refine.py)."""
    a, b = _xyxyr(a), _xyxyr(b)
    out = np.zeros(a.shape[0])
    for i in range(a.shape[0]):
        ov = float(orefine.rotated_overlap_batch(a[i], b[i:i + 1])[0])
        ua = (a[i, 2] - a[i, 0]) * (a[i, 3] - a[i, 1]) + (b[i, 2] - b[i, 0]) * (b[i, 3] - b[i, 1]) - ov
        out[i] = ov / max(ua, 1e-12)
    return out


def match_boxes(gb, gs, gl, ob, os_, ol):
    """Greedy one-to-one matching in descending GPU score: a GPU box takes the nearest (BEV centre) unmatched oracle box
    of its label within 0.5 m; returns (index pairs, IoU per pair, |dscore| per pair)."""
    gb, ob = np.asarray(gb, np.float64), np.asarray(ob, np.float64)
    taken = np.zeros(ob.shape[0], dtype=bool)
    pairs = []
    for i in np.argsort(-np.asarray(gs), kind="stable"):
        cand = np.nonzero((np.asarray(ol) == gl[i]) & ~taken)[0]
        if cand.size == 0:
            continue
        d = np.hypot(ob[cand, 0] - gb[i, 0], ob[cand, 1] - gb[i, 1])
        j = cand[int(np.argmin(d))]
        if d.min() <= 0.5:
            taken[j] = True
            pairs.append((int(i), int(j)))
    pairs = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    iou = _pair_iou(gb[pairs[:, 0]], ob[pairs[:, 1]]) if len(pairs) else np.zeros(0)
    ds = np.abs(np.asarray(gs, np.float64)[pairs[:, 0]] - np.asarray(os_, np.float64)[pairs[:, 1]]) if len(pairs) else np.zeros(0)
    return pairs, iou, ds


def _feature_deviation(g_feats, g_keys, o_feats, o_keys):
    """Deviation of group features on the keys both sides hold, relative to the oracle's feature scale."""
    gk = {tuple(r): i for i, r in enumerate(np.asarray(g_keys).tolist())}
    rows = [(gk[tuple(r)], j) for j, r in enumerate(np.asarray(o_keys).tolist()) if tuple(r) in gk]
    if not rows:
        return dict(common=0, p999=float("nan"), max=float("nan"), scale=float("nan"))
    rows = np.array(rows)
    g, o = np.asarray(g_feats, np.float64)[rows[:, 0]], np.asarray(o_feats, np.float64)[rows[:, 1]]
    scale = max(1.0, float(np.abs(o).max()))
    d = np.abs(g - o).max(1) / scale
    return dict(common=int(len(rows)), p999=float(np.quantile(d, 0.999)), max=float(d.max()), median=float(np.median(d)),
                scale=scale)


# Thresholds: measured first (round 4, MI355X, the test's e2e_agreement_*.json reports -> DESIGN.md section 3), then frozen with margin.
# Measured: 500 / 500 boxes matched on all three frames, worst matched IoU 0.99957, worst |dscore| 2.1e-5; query keys identical;
# SIR group features 99.9th percentile 5.6e-3 (camera stack: rel_mlp's LayerNorms amplify the 1e-5 m centroid rounding) and
# 3.4e-4 (LiDAR stack) of the feature scale.
E2E_MIN_MATCHED_FRACTION = 0.99      # of the 500 returned boxes, matched at BEV IoU >= 0.99 with |dscore| <= 1e-3
E2E_MAX_UNMATCHED = 5
E2E_MAX_CAMERA_SIR_DEV_P999 = 2e-2   # vs the fp32 ORACLE chain — whose own distance to the float64 chain is 5.7e-3 (10 sweeps), 3.5e-3 (AV2):
#                                      this bound limits the oracle's conditioning, the next three limit the device
# Round 5, measured on MI355X (profiles/r5_e2e_agreement_*.json): camera-stack SIR group features, 99.9th percentile of the row
# maximum relative to the feature scale — device vs the float64 chain 1.8e-4 / 9.0e-5 / 5.5e-5 (1 sweep / 10 sweeps / AV2), the fp32
# oracle vs the float64 chain 1.8e-4 / 5.7e-3 / 3.5e-3: the device is as close to float64 as the fp32 oracle on the small frame and
# 60 x closer on the large ones (its centroids and LayerNorm statistics are accumulated in blocked / pairwise order).
E2E_F64_RATIO = 3.0                  # |gpu - float64 chain| <= ratio x |fp32 oracle - float64 chain| + floor
E2E_F64_FLOOR = 1e-5
E2E_MAX_CAMERA_SIR_DEV_VS_F64_P999 = 3.6e-4  # = 2 x the largest measured (1.8e-4: the 1-sweep frame, where the fp32 ORACLE sits the same 1.8e-4
#                                             from float64 — groups of one to three points put f_cluster at ~0 in front of three LayerNorm(eps=1e-3))
# Round 6: the LiDAR stack arbitrated the same way (stage 3 in float64 on the fp32 chain's integer structure).  Measured on MI355X
# (profiles/r6_e2e_agreement_*.json; 1 sweep / 10 sweeps / AV2), 99.9th percentile of the row maximum relative to the feature scale:
#   device vs the fp32 oracle chain   3.2e-4 / 3.4e-4 / 2.5e-5
#   device vs the float64 chain       3.3e-4 / 3.8e-4 / 2.3e-4
#   fp32 ORACLE vs the float64 chain  3.4e-4 / 5.1e-4 / 2.3e-4   <- the frame's conditioning term: what ANY fp32 evaluation of the reference's
# arithmetic shows on these clusters (centroid rounding amplified by the position MLP's LayerNorms).  The device is never farther from
# float64 than the fp32 oracle is; the 1e-4 contract is asserted beyond that term.
E2E_MAX_LIDAR_SIR_DEV_P999 = 7e-4            # vs the fp32 oracle chain (was 2e-3): <= 2 x the measured 3.4e-4
E2E_MAX_LIDAR_SIR_DEV_VS_F64_P999 = 7.5e-4   # vs the float64 chain: <= 2 x the measured 3.8e-4
E2E_CONTRACT = 1e-4                          # north_star's feature tolerance, beyond the frame's fp32 conditioning term
