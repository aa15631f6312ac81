"""Times the detection metrics (K41) on a synthetic validation set of nuScenes-val size: 6 019 samples, 500 predictions and ~30 GT boxes
each, 10 classes (the GT scattered over +-50 m, 60 % of the predictions near a GT box of their class, the rest anywhere):

    compute_wall     `DeviceDetectionEval.compute()` on the accumulated buffers, its one read-back included: host clock between two
                     device synchronisations
    device           the launches of `hip_ops_eval.det_eval` alone: device events
    host_spec_wall   the host specification (`evaluate_host`, numpy float64) on this machine's CPU for the first `--host-samples` samples;
                     its matching loop is linear in the predictions, so `host_spec_wall_s_scaled` = that time x samples / host samples;
                     with `--host-samples` = `--samples` the two results are compared as well (matches_differing, result_max_abs_diff)

    python tools/profiling/det_eval_time.py [--steps 10] [--warmup 2] [--samples 6019] [--host-samples 300] [--out FILE.json] [--only-device]

Prints one JSON line.  `--only-device` runs the device path alone, `--steps` times (for a kernel trace)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from fullysparsefusion_amd.mmdet3d_plugin.core.det_eval import DeviceDetectionEval, evaluate_host  # noqa: E402

CLASSES = ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone")
PRED, GT = 500, 30


def make_set(samples, seed=0):
    """Per sample (pred f32 [500, 9], score, label, attr, gt f32 [g, 9], gt_label, gt_attr) as numpy arrays."""
    rng = np.random.default_rng(seed)
    frames = []
    for _ in range(samples):
        g = int(rng.integers(GT - 10, GT + 11))
        gt = np.zeros((g, 9), dtype=np.float32)
        gt[:, :2] = rng.uniform(-50, 50, (g, 2))
        gt[:, 3:6] = rng.uniform(0.5, 5, (g, 3))
        gt[:, 6] = rng.uniform(-np.pi, np.pi, g)
        gt[:, 7:] = rng.normal(size=(g, 2))
        gt[rng.random(g) < 0.1, 7:] = np.nan
        gt_label = rng.integers(0, len(CLASSES), g)
        near = rng.random(PRED) < 0.6
        src = rng.integers(0, g, PRED)
        pred = gt[src].copy()
        pred[:, :2] += rng.normal(scale=0.8, size=(PRED, 2)).astype(np.float32)
        pred[:, 3:7] += rng.normal(scale=0.1, size=(PRED, 4)).astype(np.float32)
        pred[:, 7:] = rng.normal(size=(PRED, 2))
        pred[~near, :2] = rng.uniform(-50, 50, (int((~near).sum()), 2))
        label = np.where(near, gt_label[src], rng.integers(0, len(CLASSES), PRED))
        score = np.where(near, rng.beta(4, 2, PRED), rng.beta(1, 6, PRED)).astype(np.float32)
        frames.append((pred, score, label, rng.integers(0, 8, PRED), gt, gt_label, rng.integers(-1, 8, g)))
    return frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=6019)
    ap.add_argument("--host-samples", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-device", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    frames = make_set(args.samples)
    ev = DeviceDetectionEval(CLASSES, device=dev)
    t0 = time.perf_counter()
    for pred, score, label, attr, gt, gl, ga in frames:
        ev.update(dict(boxes_3d=torch.from_numpy(pred), scores_3d=torch.from_numpy(score), labels_3d=torch.from_numpy(label),
                       attrs_3d=torch.from_numpy(attr)), torch.from_numpy(gt), torch.from_numpy(gl), torch.from_numpy(ga))
    torch.cuda.synchronize()
    update_ms = (time.perf_counter() - t0) * 1e3 / max(args.samples, 1)

    from fullysparsefusion_amd import hip_ops_eval
    from fullysparsefusion_amd.mmdet3d_plugin.core.det_eval import class_flags, first_recall_index

    p, g = ev._pred, ev._gt

    def device():
        return hip_ops_eval.det_eval(p.view("rows"), p.view("score"), p.view("label"), p.view("attr"), p.view("sample"), g.view("rows"),
                                     g.view("label"), g.view("attr"), g.view("sample"), ev.num_samples, class_flags(CLASSES), ev.dist_ths, 2,
                                     first_recall_index(0.1), 0.1, 5.0, None)

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    for _ in range(args.warmup):
        device()
    times = dict(device=[], compute_wall=[])
    for _ in range(args.steps):
        times["device"].append(events(device))
        if not args.only_device:
            times["compute_wall"].append(wall(ev.compute))
    torch.cuda.synchronize()
    result = dict(samples=args.samples, num_pred=p.n, num_gt=g.n, num_classes=len(CLASSES), steps=args.steps, cpu_threads=torch.get_num_threads(),
                  update_wall_ms_per_frame=round(update_ms, 4))
    for k, v in times.items():
        if v:
            result[f"{k}_ms_median"] = round(statistics.median(v), 3)
            result[f"{k}_ms_min"] = round(min(v), 3)
    if not args.only_device:
        m = ev.compute()
        result.update(mAP=round(m["mAP"], 6), NDS=round(m["NDS"], 6))
        hs = min(args.host_samples, args.samples)
        sub = frames[:hs]
        cat = lambda k: np.concatenate([f[k] for f in sub])  # noqa: E731
        psample = np.repeat(np.arange(hs), [f[1].size for f in sub])
        gsample = np.repeat(np.arange(hs), [f[5].size for f in sub])
        t = time.perf_counter()
        hmatch, _, hresult = evaluate_host(cat(0), cat(1), cat(2), cat(3), psample, cat(4), cat(5), cat(6), gsample, CLASSES)
        host_s = time.perf_counter() - t
        if hs == args.samples:  # the whole set on both sides: how far the device is from the specification at this size
            dmatch, dresult = ev.last[0].cpu().numpy(), ev.last[2].cpu().numpy()
            result.update(matches_differing=int((dmatch != hmatch).sum()),
                          result_max_abs_diff=float(np.nanmax(np.abs(dresult - hresult))))
        result.update(host_samples=hs, host_spec_wall_s=round(host_s, 3), host_spec_wall_s_scaled=round(host_s * args.samples / max(hs, 1), 1))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
