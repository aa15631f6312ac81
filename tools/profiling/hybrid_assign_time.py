"""Times the camera-query head's hybrid assignment + loss forward + loss backward (K37 + K36b / K36c) on a synthetic frame's worth of
camera queries (the 1-sweep frame's 44 GT rows; per visible (box, camera) pair three detections at IoU >= 0.7 / 0.3 .. 0.7 / < 0.3, plus
200 random detections per camera; a third of the query centres inside an augmented GT box), against the torch restatement of the same
steps (`loss(..., fused=False)` + autograd) on the same GPU.

    python tools/profiling/hybrid_assign_time.py [--steps 50] [--warmup 10] [--out FILE.json] [--only-fused]

The two paths alternate step by step in one process, so both see the same clocks.  Each step (regrouping and upload of the host GT and
of the camera matrices, 2-D boxes, assignment, forward, backward) is timed with the host's clock between two device synchronisations.
Prints one JSON line (median / min per step, in ms).  `--only-fused` runs the K37 path alone (for a kernel trace)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from fullysparsefusion_amd import synthetic  # noqa: E402
from fullysparsefusion_amd.compat import Config  # noqa: E402
from fullysparsefusion_amd.mmdet3d_plugin.core.assigners import gt_boxes_2d_host  # noqa: E402
from fullysparsefusion_amd.mmdet3d_plugin.registry import build_head  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_queries(seed=3, random_per_cam=200):
    frame = synthetic.make_frame(num_sweeps=1, seed=seed, mask_instances=10)
    boxes, labels = synthetic.make_gt_boxes(frame["points"], seed=seed)
    angle, scale = 0.15, 1.04  # the augmented list: a global rotation and scaling, the order kept
    aug = boxes.copy()
    c, s = math.cos(angle), math.sin(angle)
    aug[:, 0], aug[:, 1] = (boxes[:, 0] * c - boxes[:, 1] * s) * scale, (boxes[:, 0] * s + boxes[:, 1] * c) * scale
    aug[:, 2] *= scale
    aug[:, 3:6] *= scale
    aug[:, 6] += angle
    l2i = np.asarray(frame["lidar2img"], np.float64)
    rng = np.random.default_rng(seed + 500)
    valid = boxes[labels >= 0]
    b2d, keep = gt_boxes_2d_host(torch.from_numpy(valid), torch.from_numpy(l2i))
    dets = []
    for k, cam in zip(*np.nonzero(keep.numpy())):
        x0, y0, x1, y1 = b2d[k, cam].tolist()
        w, h = x1 - x0, y1 - y0
        for shift, grow in ((0.03, 0.97), (0.22, 1.0), (0.75, 1.1)):
            sx, sy = rng.uniform(-1, 1, 2) * shift
            cx, cy = (x0 + x1) / 2 + sx * w, (y0 + y1) / 2 + sy * h
            dets.append([cx - w * grow / 2, cy - h * grow / 2, cx + w * grow / 2, cy + h * grow / 2, rng.uniform(), 0, cam, len(dets), 1])
    for cam in range(6):
        for _ in range(random_per_cam):
            x, y = rng.uniform(0, 1550), rng.uniform(0, 850)
            dets.append([x, y, x + rng.uniform(20, 400), y + rng.uniform(20, 300), rng.uniform(), 0, cam, len(dets), 1])
    preds = np.array(dets, np.float32)
    n = len(preds)
    va = aug[labels >= 0]
    centres = np.stack([rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), np.full(n, 30.0)], 1)
    inside = rng.random(n) < 0.33
    pick = rng.integers(0, len(va), n)
    grav = va[pick, :3].astype(np.float64)
    grav[:, 2] += va[pick, 5] / 2
    centres[inside] = grav[inside] + rng.normal(0, 0.1, (int(inside.sum()), 3))
    return centres.astype(np.float32), preds, boxes, aug.astype(np.float32), labels, l2i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-fused", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "fsf_nuscenes.py"))
    head = build_head(dict(cfg.model.frustum_obj_head)).to(dev)
    centres, preds, boxes, aug, labels, l2i = make_queries()
    n = centres.shape[0]
    xyz, preds_2d = torch.from_numpy(centres).to(dev), torch.from_numpy(preds).to(dev)
    inds = torch.zeros((n, 3), dtype=torch.int64, device=dev)
    na_b, gt_b, gt_l = [torch.from_numpy(boxes)], [torch.from_numpy(aug)], [torch.from_numpy(labels)]
    metas = [dict(lidar2img=[m for m in l2i])]
    g = torch.Generator(device=dev).manual_seed(0)
    cls_logits = (torch.randn((n, 10), generator=g, device=dev) * 2).requires_grad_()
    reg_preds = torch.randn((n, 10), generator=g, device=dev).requires_grad_()
    suffix = f"{head.tasks[0]['class_names']}"
    names = [k + suffix for k in ("loss_cls", "loss_center", "loss_size", "loss_rot", "loss_vel")]
    last = {}

    def step(fused):
        cls_logits.grad = reg_preds.grad = None
        out = head.loss([cls_logits], [reg_preds], xyz, inds, na_b, gt_l, gt_b, gt_l, preds_2d, metas, fused=fused)
        sum(out[k] for k in names).backward()
        last[fused] = out

    paths = [("k37", True)] + ([] if args.only_fused else [("torch_restatement", False)])
    for _ in range(args.warmup):
        for _, fused in paths:
            step(fused)
    times = {name: [] for name, _ in paths}
    for _ in range(args.steps):
        for name, fused in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(fused)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    result = dict(n_queries=n, num_boxes=int(boxes.shape[0]), num_cams=6, num_classes=10, code_size=10, steps=args.steps,
                  num_pos=float(last[True]["num_pos_preds" + suffix]), assigned_gts=float(last[True]["assigned_gts" + suffix]))
    for name, _ in paths:
        result[f"{name}_ms_median"] = round(statistics.median(times[name]), 4)
        result[f"{name}_ms_min"] = round(min(times[name]), 4)
    if not args.only_fused:
        result["speedup_median"] = round(result["torch_restatement_ms_median"] / result["k37_ms_median"], 2)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
