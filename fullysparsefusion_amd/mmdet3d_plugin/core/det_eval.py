"""The nuScenes detection protocol (`detection_cvpr_2019`): centre-distance matching, AP, the five true-positive errors, mAP and NDS
(K41, docs/kernels/K41_det_eval.md).

The first half is the HOST SPECIFICATION in numpy float64 (inputs are f32 and are promoted once): the yardstick the kernels of
csrc/det_eval.hip are tested against.  The nuScenes devkit is un-vendored and on no machine this project builds on, so the functions
restate the published algorithm (`nuscenes/eval/detection/algo.py::accumulate / calc_ap / calc_tp`, `nuscenes/eval/common/utils.py`,
`DetectionMetrics`); parity with the devkit itself is UNPINNED.  Only x, y enter the matching and every quantity (centre distance,
velocity difference, size ratio, yaw difference) is invariant under a rigid motion of the frame, so rows in the LiDAR frame serve; the
optional `class_range` filter measures sqrt(x^2 + y^2) in the rows' own frame, which equals the devkit's `filter_eval_boxes` (on the
ego translation) only for ego-frame rows.  The devkit's data-side pre-filters (GT without points, bike racks) are not restated.

The second half is `DeviceDetectionEval`: predictions and ground truth accumulate in device buffers frame by frame, `compute()` runs
the kernels and reads one result block back.

Rows are `[x, y, z, w, l, h, yaw, vx, vy]`; a prediction has a score, a label and an attribute id (-1 = none), a GT row a label and an
attribute id; rows with a label outside [0, num_classes) are ignored.
"""
import numpy as np
import torch

TP_METRICS = ("trans_err", "scale_err", "orient_err", "vel_err", "attr_err")  # the order of the kernels' error index
MEAN_NAMES = ("mATE", "mASE", "mAOE", "mAVE", "mAAE")
ERR_NAMES = dict(zip(TP_METRICS, MEAN_NAMES))
POINTS = 101
HEAD = 8  # FSF_DET_EVAL_HEAD
_UNDEFINED = {"traffic_cone": ("attr_err", "vel_err", "orient_err"), "barrier": ("attr_err", "vel_err")}


def class_flags(class_names):
    """Per class: bit 0 = the orientation period is pi (barrier), bit 1 + e = TP error e is NaN for the class."""
    return [(1 if name == "barrier" else 0) | sum(2 << TP_METRICS.index(m) for m in _UNDEFINED.get(name, ())) for name in class_names]


def recall_points():
    return np.linspace(0, 1, POINTS)


def first_recall_index(min_recall):
    return int(round(100 * min_recall)) + 1


def effective_class(rows, labels, num_classes, class_range=None, none=-1):
    """The class each row counts for: its label, or `none` when the label names no class or the row lies beyond the class's range."""
    rows, labels = np.asarray(rows, dtype=np.float64).reshape(-1, 9), np.asarray(labels).astype(np.int64).reshape(-1)
    ok = (labels >= 0) & (labels < num_classes)
    if class_range is not None:
        x, y = rows[:, 0], rows[:, 1]
        reach = np.asarray(class_range, dtype=np.float64)[np.where(ok, labels, 0)]
        ok &= ~(np.sqrt(x * x + y * y) > reach)
    return np.where(ok, labels, none)


def angle_diff(a, b, period):
    diff = np.mod(a - b + period / 2, period) - period / 2
    return np.where(diff > np.pi, diff - 2 * np.pi, diff)


def cummean(x):
    """The devkit's NaN-skipping running mean: a prefix without a finite value gives 0, an all-NaN input gives ones."""
    x = np.asarray(x, dtype=np.float64)
    nan = np.isnan(x)
    if nan.sum() == x.size:
        return np.ones(x.size)
    sums, counts = np.cumsum(np.where(nan, 0.0, x)), np.cumsum(~nan)
    return np.divide(sums, counts, out=np.zeros_like(sums), where=counts != 0)


def match_errors(gt_row, pred_row, gt_attr, pred_attr, period):
    """The five errors of one match, in TP_METRICS order (trans_err is the centre distance)."""
    dx, dy = gt_row[0] - pred_row[0], gt_row[1] - pred_row[1]
    dvx, dvy = gt_row[7] - pred_row[7], gt_row[8] - pred_row[8]
    small = np.minimum(gt_row[3:6], pred_row[3:6])
    inter = small[0] * small[1] * small[2]
    union = gt_row[3] * gt_row[4] * gt_row[5] + pred_row[3] * pred_row[4] * pred_row[5] - inter
    return (np.sqrt(dx * dx + dy * dy), 1.0 - inter / union, float(np.abs(angle_diff(gt_row[6], pred_row[6], period))),
            np.sqrt(dvx * dvx + dvy * dvy), np.nan if gt_attr < 0 else float(gt_attr != pred_attr))


def accumulate_host(pred, score, pred_cls, pred_attr, pred_sample, gt, gt_cls, gt_attr, gt_sample, cls, dist_th, period=2 * np.pi):
    """`accumulate` for one class and one threshold.  `pred_cls` / `gt_cls` are effective classes; the sample ids are non-decreasing.
    -> dict(order: the class's predictions (indices) in processing order, match: the matched GT row per entry of `order` or -1, npos,
    no_predictions, precision / confidence [101], errors [5, 101])."""
    pred, gt = np.asarray(pred, dtype=np.float64).reshape(-1, 9), np.asarray(gt, dtype=np.float64).reshape(-1, 9)
    score64, pred_sample = np.asarray(score, dtype=np.float64), np.asarray(pred_sample)
    idx = np.flatnonzero(np.asarray(pred_cls) == cls)
    order = idx[np.argsort(score64[idx], kind="stable")][::-1]  # descending score, the LATER position first among equal scores
    gidx = np.flatnonzero(np.asarray(gt_cls) == cls)  # (stored order)
    npos = gidx.size
    gsamp = np.asarray(gt_sample)[gidx]
    gx, gy = gt[gidx, 0], gt[gidx, 1]
    taken = np.zeros(npos, dtype=bool)
    match = np.full(order.size, -1, dtype=np.int64)
    for k, p in enumerate(order):
        lo, hi = np.searchsorted(gsamp, pred_sample[p], "left"), np.searchsorted(gsamp, pred_sample[p], "right")
        if hi == lo:
            continue
        dx, dy = gx[lo:hi] - pred[p, 0], gy[lo:hi] - pred[p, 1]
        dist = np.sqrt(dx * dx + dy * dy)
        dist[taken[lo:hi] | np.isnan(dist)] = np.inf
        j = int(np.argmin(dist))  # the first of equal distances
        if dist[j] < dist_th:  # strict
            taken[lo + j] = True
            match[k] = gidx[lo + j]
    out = dict(order=order, match=match, npos=npos, no_predictions=True, precision=np.zeros(POINTS), confidence=np.zeros(POINTS),
               errors=np.ones((len(TP_METRICS), POINTS)))
    hit = match >= 0
    if npos == 0 or order.size == 0 or not hit.any():
        return out
    tp = np.cumsum(hit).astype(np.float64)
    fp = np.cumsum(~hit).astype(np.float64)
    conf = score64[order]
    prec, rec = tp / (fp + tp), tp / float(npos)
    rec_interp = recall_points()
    out["no_predictions"] = False
    out["precision"] = np.interp(rec_interp, rec, prec, right=0)
    out["confidence"] = conf_interp = np.interp(rec_interp, rec, conf, right=0)
    pa, ga = np.asarray(pred_attr), np.asarray(gt_attr)
    errs = np.array([match_errors(gt[g], pred[p], ga[g], pa[p], period) for p, g in zip(order[hit], match[hit])], dtype=np.float64)
    match_conf = conf[hit]
    for e in range(len(TP_METRICS)):
        out["errors"][e] = np.interp(conf_interp[::-1], match_conf[::-1], cummean(errs[:, e])[::-1])[::-1]
    return out


def calc_ap(precision, min_recall, min_precision):
    prec = np.copy(precision)[first_recall_index(min_recall):] - min_precision
    prec[prec < 0] = 0
    return float(np.mean(prec)) / (1.0 - min_precision)


def calc_tp(confidence, error, min_recall):
    first = first_recall_index(min_recall)
    nonzero = np.nonzero(confidence)[0]
    last = int(nonzero[-1]) if nonzero.size else 0
    return 1.0 if last < first else float(np.mean(error[first:last + 1]))


def result_words(num_classes, num_thresholds):
    return HEAD + num_classes * (3 * num_thresholds + len(TP_METRICS) + 2)


def evaluate_host(pred, score, pred_label, pred_attr, pred_sample, gt, gt_label, gt_attr, gt_sample, class_names, dist_ths=(0.5, 1, 2, 4),
                  dist_th_tp=2.0, min_recall=0.1, min_precision=0.1, mean_ap_weight=5, class_range=None):
    """The whole protocol on the host, in the layout of `hip_ops_eval.det_eval`: (match i64 [T, P], curves f64 [C, 2 T + 5, 101], result f64
    [result_words]).  numpy arrays in, numpy arrays out."""
    C, T, E = len(class_names), len(dist_ths), len(TP_METRICS)
    t_tp = [float(t) for t in dist_ths].index(float(dist_th_tp))
    pred = np.asarray(pred, dtype=np.float32).reshape(-1, 9)
    gt = np.asarray(gt, dtype=np.float32).reshape(-1, 9)
    pcls = effective_class(pred, pred_label, C, class_range)
    gcls = effective_class(gt, gt_label, C, class_range)
    flags = class_flags(class_names)
    match = np.full((T, pred.shape[0]), -1, dtype=np.int64)
    curves = np.zeros((C, 2 * T + E, POINTS))
    result = np.zeros(result_words(C, T))
    ap = result[HEAD:HEAD + C * T].reshape(C, T)
    tpe = result[HEAD + C * T:HEAD + C * (T + E)].reshape(C, E)
    tail = result[HEAD + C * (T + E):]
    npos, npred = tail[:C], tail[C:2 * C]
    ntp, none = tail[2 * C:2 * C + C * T].reshape(C, T), tail[2 * C + C * T:].reshape(C, T)
    for c in range(C):
        period = np.pi if flags[c] & 1 else 2 * np.pi
        for t, th in enumerate(dist_ths):
            md = accumulate_host(pred, score, pcls, pred_attr, pred_sample, gt, gcls, gt_attr, gt_sample, c, float(th), period)
            match[t, md["order"]] = md["match"]
            curves[c, t], curves[c, T + t] = md["precision"], md["confidence"]
            ap[c, t] = calc_ap(md["precision"], min_recall, min_precision)
            npos[c], npred[c] = md["npos"], md["order"].size
            ntp[c, t], none[c, t] = (md["match"] >= 0).sum(), md["no_predictions"]
            if t == t_tp:
                curves[c, 2 * T:] = md["errors"]
                for e in range(E):
                    tpe[c, e] = np.nan if (flags[c] >> (1 + e)) & 1 else calc_tp(md["confidence"], md["errors"][e], min_recall)
    result[0] = ap.mean()
    scores = []
    for e in range(E):
        col = tpe[:, e]
        result[1 + e] = col[~np.isnan(col)].mean() if (~np.isnan(col)).any() else np.nan
        scores.append(max(1.0 - float(result[1 + e]), 0.0))  # (Python's max keeps a NaN first argument, as the devkit's does)
    result[6] = (mean_ap_weight * result[0] + np.sum(scores)) / float(mean_ap_weight + E)
    return match, curves, result


def unpack_result(result, class_names, dist_ths):
    """The result block as a dict: per-class AP per threshold, per-class TP errors, mAP, mATE ... mAAE, NDS and the counts."""
    r = np.asarray(result, dtype=np.float64)
    C, T, E = len(class_names), len(dist_ths), len(TP_METRICS)
    ap = r[HEAD:HEAD + C * T].reshape(C, T)
    tpe = r[HEAD + C * T:HEAD + C * (T + E)].reshape(C, E)
    tail = r[HEAD + C * (T + E):]
    out = dict(mAP=float(r[0]), NDS=float(r[6]))
    out.update({name: float(r[1 + e]) for e, name in enumerate(MEAN_NAMES)})
    out["label_aps"] = {n: {float(th): float(ap[c, t]) for t, th in enumerate(dist_ths)} for c, n in enumerate(class_names)}
    out["label_tp_errors"] = {n: {m: float(tpe[c, e]) for e, m in enumerate(TP_METRICS)} for c, n in enumerate(class_names)}
    out["npos"] = {n: int(tail[c]) for c, n in enumerate(class_names)}
    out["num_predictions"] = {n: int(tail[C + c]) for c, n in enumerate(class_names)}
    return out


# ------------------------------------------------------------------------------------------------ the public class
def _box_rows(boxes, missing_velocity):
    """Boxes of one frame -> f32 [n, 9]: `LiDARInstance3DBoxes` or a tensor / array of >= 7 columns; rows without velocity columns get
    `missing_velocity` (0 for predictions, NaN for ground truth: the velocity error then skips the match)."""
    t = torch.as_tensor(getattr(boxes, "tensor", boxes))
    t = t.reshape(-1, t.shape[-1]) if t.numel() else t.reshape(0, 9)
    t = t.to(torch.float32)
    if t.shape[1] >= 9:
        return t[:, :9]
    assert t.shape[1] >= 7, "a box row needs x y z w l h yaw"
    return torch.cat([t[:, :7], t.new_full((t.shape[0], 2), missing_velocity)], 1)


class _Rows:
    """Columns that grow together by doubling; counts come from shapes, never from the device."""

    def __init__(self, device, **columns):  # name -> (trailing shape, dtype)
        self.device, self.spec, self.n = device, columns, 0
        self.buf = {k: torch.empty((0,) + shape, dtype=dtype, device=device) for k, (shape, dtype) in columns.items()}

    def append(self, **cols):
        k = next(iter(cols.values())).shape[0]
        cap = self.buf[next(iter(self.buf))].shape[0]
        if self.n + k > cap:
            cap = max(2 * cap, self.n + k, 1024)
            for name, (shape, dtype) in self.spec.items():
                grown = torch.empty((cap,) + shape, dtype=dtype, device=self.device)
                grown[:self.n] = self.buf[name][:self.n]
                self.buf[name] = grown
        for name, value in cols.items():
            self.buf[name][self.n:self.n + k] = value
        self.n += k

    def view(self, name):
        return self.buf[name][:self.n]


class DeviceDetectionEval:
    """nuScenes detection metrics of a validation pass.  `update(result, gt_bboxes_3d, gt_labels_3d, gt_attrs=None)` once per frame with
    what `FSF.simple_test` returns for it (host tensors: pass `device=` to accumulate them on the GPU all the same), `compute()` at the end (the kernels of K41 and one read-back), `as_mmdet3d_dict()` for the keys
    mmdet3d logs, `reset()` before the next pass.  `fused=False`, or CPU inputs, runs the host specification of this module.
    Not built: the Argoverse 2 protocol (CDS, the av2 package), the devkit's data-side filters, merging the state of several ranks."""

    def __init__(self, class_names, dist_ths=(0.5, 1, 2, 4), dist_th_tp=2.0, min_recall=0.1, min_precision=0.1, mean_ap_weight=5,
                 class_range=None, fused=True, device=None):
        self.class_names = list(class_names)
        self.dist_ths = tuple(float(t) for t in dist_ths)
        assert float(dist_th_tp) in self.dist_ths, "dist_th_tp must be one of dist_ths (as the devkit's config asserts)"
        self.dist_th_tp, self.min_recall, self.min_precision = float(dist_th_tp), float(min_recall), float(min_precision)
        self.mean_ap_weight = float(mean_ap_weight)
        if isinstance(class_range, dict):
            class_range = [class_range[n] for n in self.class_names]
        self.class_range = None if class_range is None else [float(v) for v in class_range]
        self.fused = bool(fused)
        self.device = None if device is None or not self.fused else torch.device(device)  # else: the device of the first frame's tensors
        self.reset()

    def reset(self):
        self._pred = self._gt = None
        self.num_samples = 0
        self.last = None  # (match, curves, result) of the last compute()

    def _start(self, device):
        i32 = ((), torch.int32)
        self._pred = _Rows(device, rows=((9,), torch.float32), score=((), torch.float32), label=i32, attr=i32, sample=i32)
        self._gt = _Rows(device, rows=((9,), torch.float32), label=i32, attr=i32, sample=i32)

    def _to(self, t, dtype):
        t = torch.as_tensor(t)
        dev = self._pred.device
        if t.device == dev:
            return t.to(dtype)
        if dev.type == "cuda" and not t.is_cuda:
            if t.numel() == 0:
                return torch.zeros(t.shape, dtype=dtype, device=dev)
            return t.to(dtype).pin_memory().to(dev, non_blocking=True)
        return t.to(device=dev, dtype=dtype)

    def update(self, result, gt_bboxes_3d, gt_labels_3d, gt_attrs=None):
        result = result.get("pts_bbox", result)
        boxes = _box_rows(result["boxes_3d"], 0.0)
        gt = _box_rows(gt_bboxes_3d, float("nan"))
        if self._pred is None:
            cuda = [t.device for t in (boxes, gt, torch.as_tensor(result["scores_3d"])) if t.is_cuda]
            self._start(self.device or (cuda[0] if self.fused and cuda else torch.device("cpu")))
        n, g, s = boxes.shape[0], gt.shape[0], self.num_samples
        dev = self._pred.device
        attrs = result.get("attrs_3d", None)
        self._pred.append(rows=self._to(boxes, torch.float32), score=self._to(result["scores_3d"], torch.float32).reshape(n),
                          label=self._to(result["labels_3d"], torch.int32).reshape(n),
                          attr=self._to(attrs, torch.int32).reshape(n) if attrs is not None else torch.full((n,), -1, dtype=torch.int32, device=dev),
                          sample=torch.full((n,), s, dtype=torch.int32, device=dev))
        self._gt.append(rows=self._to(gt, torch.float32), label=self._to(gt_labels_3d, torch.int32).reshape(g),
                        attr=self._to(gt_attrs, torch.int32).reshape(g) if gt_attrs is not None else torch.full((g,), -1, dtype=torch.int32, device=dev),
                        sample=torch.full((g,), s, dtype=torch.int32, device=dev))
        self.num_samples += 1

    def compute(self):
        if self._pred is None:
            self._start(torch.device("cpu"))
        p, g = self._pred, self._gt
        if p.device.type == "cuda":
            from ... import hip_ops_eval

            match, curves, result = hip_ops_eval.det_eval(
                p.view("rows"), p.view("score"), p.view("label"), p.view("attr"), p.view("sample"), g.view("rows"), g.view("label"),
                g.view("attr"), g.view("sample"), self.num_samples, class_flags(self.class_names), self.dist_ths,
                self.dist_ths.index(self.dist_th_tp), first_recall_index(self.min_recall), self.min_precision, self.mean_ap_weight,
                self.class_range)
            self.last = (match, curves, result)
            host = result.cpu().numpy()  # the one read-back
        else:
            match, curves, host = evaluate_host(
                p.view("rows").numpy(), p.view("score").numpy(), p.view("label").numpy(), p.view("attr").numpy(), p.view("sample").numpy(),
                g.view("rows").numpy(), g.view("label").numpy(), g.view("attr").numpy(), g.view("sample").numpy(), self.class_names,
                self.dist_ths, self.dist_th_tp, self.min_recall, self.min_precision, self.mean_ap_weight, self.class_range)
            self.last = (torch.from_numpy(match), torch.from_numpy(curves), torch.from_numpy(host))
        self.metrics = unpack_result(host, self.class_names, self.dist_ths)
        return self.metrics

    def as_mmdet3d_dict(self, prefix="pts_bbox_NuScenes"):
        """The keys `NuScenesDataset._evaluate_single` logs, from the last `compute()`."""
        m, out = self.metrics, {}
        for name in self.class_names:
            for th, v in m["label_aps"][name].items():
                out[f"{prefix}/{name}_AP_dist_{th}"] = float(f"{v:.4f}")
            for err, v in m["label_tp_errors"][name].items():
                out[f"{prefix}/{name}_{err}"] = float(f"{v:.4f}")
        for name in MEAN_NAMES:
            out[f"{prefix}/{name}"] = float(f"{m[name]:.4f}")
        out[f"{prefix}/NDS"] = m["NDS"]
        out[f"{prefix}/mAP"] = m["mAP"]
        return out
