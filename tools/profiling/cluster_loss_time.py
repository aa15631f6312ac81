"""Times the LiDAR-query head's targets + loss forward + loss backward (K36) on a synthetic frame's worth of clusters (3000 random
points of the 1-sweep frame + 8 centres per GT box), against the torch restatement of the same steps (`loss(..., fused=False)` +
autograd) on the same GPU.

    python tools/profiling/cluster_loss_time.py [--steps 50] [--warmup 10] [--out FILE.json] [--only-fused]

The two paths alternate step by step in one process, so both see the same clocks.  Each step (regrouping and upload of the host GT,
targets, forward, backward) is timed with the host's clock between two device synchronisations: the restatement's cost is mostly host
waits (`.item()` asserts, `nonzero`, boolean indexing), which device events alone would not separate from launch gaps.  Prints one JSON
line (median / min per step, in ms).  `--only-fused` runs the K36 path alone (for a kernel trace)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from fullysparsefusion_amd import synthetic  # noqa: E402
from fullysparsefusion_amd.compat import Config  # noqa: E402
from fullysparsefusion_amd.mmdet3d_plugin.registry import build_head  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_clusters(seed=3):
    pts = synthetic.make_frame(num_sweeps=1, seed=seed)["points"]
    boxes, labels = synthetic.make_gt_boxes(pts, seed=seed)
    rng = np.random.default_rng(seed + 9000)
    centres = pts[rng.choice(len(pts), 3000, replace=False), :3]
    valid = boxes[labels >= 0]
    gravity = valid[:, :3].astype(np.float64)
    gravity[:, 2] += valid[:, 5] / 2.0
    near = (gravity[:, None, :] + rng.normal(0, 0.25, (len(valid), 8, 3))).reshape(-1, 3)
    return np.concatenate([centres, near]).astype(np.float32), boxes, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-fused", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "fsf_nuscenes.py"))
    head_cfg = dict(cfg.model.bbox_head)
    head_cfg.update(train_cfg=dict(cfg.model.train_cfg), test_cfg=None)
    head = build_head(head_cfg).to(dev)
    centres, boxes, labels = make_clusters()
    n = centres.shape[0]
    xyz = torch.from_numpy(centres).to(dev)
    inds = torch.zeros((n, 3), dtype=torch.int64, device=dev)
    gt_b, gt_l = [torch.from_numpy(boxes)], [torch.from_numpy(labels)]
    g = torch.Generator(device=dev).manual_seed(0)
    cls_logits = (torch.randn((n, 10), generator=g, device=dev) * 2).requires_grad_()
    reg_preds = torch.randn((n, 10), generator=g, device=dev).requires_grad_()
    suffix = f"{head.tasks[0]['class_names']}"
    names = [k + suffix for k in ("loss_cls", "loss_center", "loss_size", "loss_rot", "loss_vel")]

    def step(fused):
        cls_logits.grad = reg_preds.grad = None
        out = head.loss([cls_logits], [reg_preds], xyz, inds, gt_b, gt_l, fused=fused)
        sum(out[k] for k in names).backward()

    paths = [("k36", True)] + ([] if args.only_fused else [("torch_restatement", False)])
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
    result = dict(n_clusters=n, num_boxes=int(boxes.shape[0]), num_classes=10, code_size=10, steps=args.steps)
    for name, _ in paths:
        result[f"{name}_ms_median"] = round(statistics.median(times[name]), 4)
        result[f"{name}_ms_min"] = round(min(times[name]), 4)
    if not args.only_fused:
        result["speedup_median"] = round(result["torch_restatement_ms_median"] / result["k36_ms_median"], 2)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
