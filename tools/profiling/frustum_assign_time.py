"""Times a refine stage's frustum + distance assignment + loss forward + loss backward (K38 + K36b / K36c) on the queries of
tools/profiling/hybrid_assign_time.py (1 344 queries, the 1-sweep frame's 44 GT rows, 6 cameras), with synthetic previous-stage logits
and the nuScenes radii; 240 of the centres that sit in no box are moved next to a GT centre, above the box, so that the distance step
has work.  Three paths alternate step by step in one process, so all see the same clocks:

    k38                the refine head's fused path (`fsf_gt_boxes_2d`, `fsf_frustum_assign`, K36b / K36c)
    torch_restatement  `loss(..., fused=False)` + autograd on the same GPU
    k37                the camera-query head's fused step (`fsf_hybrid_assign`) on the same inputs: k38 - k37 is what the distance step costs

    python tools/profiling/frustum_assign_time.py [--steps 50] [--warmup 10] [--out FILE.json] [--only-fused]

Each step (regrouping and upload of the host GT and of the camera matrices, 2-D boxes, assignment, forward, backward) is timed with the
host's clock between two device synchronisations.  Prints one JSON line (median / min per step, in ms).  `--only-fused` runs the K38 path
alone (for a kernel trace)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from hybrid_assign_time import make_queries  # noqa: E402
from fullysparsefusion_amd.compat import Config  # noqa: E402
from fullysparsefusion_amd.mmdet3d_plugin.registry import build_head  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def add_distance_work(centres, aug, labels, radii, seed=3, moved=240):
    """Moves `moved` of the centres outside every box next to a GT centre (up to twice its class radius away) -> (centres, old logits)."""
    rng = np.random.default_rng(seed + 900)
    valid = np.flatnonzero(labels >= 0)
    n = len(centres)
    old = rng.normal(0.0, 1.0, (n, len(radii))).astype(np.float32)
    outside = np.flatnonzero(centres[:, 2] == np.float32(30.0))
    for i in rng.choice(outside, min(moved, len(outside)), replace=False):
        k = int(valid[rng.integers(len(valid))])
        c = int(labels[k])
        r = max(radii[c], 0.5) * rng.uniform(0.0, 2.0)
        th = rng.uniform(0.0, 2 * np.pi)
        centres[i, :2] = aug[k, :2] + (r * np.array([np.cos(th), np.sin(th)])).astype(np.float32)
        if rng.random() < 0.8:
            old[i, c] = 6.0
    return centres, old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-fused", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "fsf_nuscenes.py"))
    refine = build_head(dict(cfg.model.refined_obj_head[0])).to(dev)
    camera = build_head(dict(cfg.model.frustum_obj_head)).to(dev)
    centres, preds, boxes, aug, labels, l2i = make_queries()
    radii = refine.assigner.assigner_dist.class_table(len(refine.class_names)).tolist()
    centres, old = add_distance_work(centres, aug, labels, radii)
    n = centres.shape[0]
    xyz, preds_2d, old_logits = torch.from_numpy(centres).to(dev), torch.from_numpy(preds).to(dev), torch.from_numpy(old).to(dev)
    inds = torch.zeros((n, 3), dtype=torch.int64, device=dev)
    na_b, gt_b, gt_l = [torch.from_numpy(boxes)], [torch.from_numpy(aug)], [torch.from_numpy(labels)]
    metas = [dict(lidar2img=[m for m in l2i])]
    g = torch.Generator(device=dev).manual_seed(0)
    cls_logits = (torch.randn((n, 10), generator=g, device=dev) * 2).requires_grad_()
    reg_preds = torch.randn((n, 10), generator=g, device=dev).requires_grad_()
    suffix = f"{refine.tasks[0]['class_names']}"
    names = [k + suffix for k in ("loss_cls", "loss_center", "loss_size", "loss_rot", "loss_vel")]
    last = {}

    def step(path):
        cls_logits.grad = reg_preds.grad = None
        if path == "k37":
            out = camera.loss([cls_logits], [reg_preds], xyz, inds, na_b, gt_l, gt_b, gt_l, preds_2d, metas)
        else:
            out = refine.loss([cls_logits], [reg_preds], xyz, inds, na_b, gt_l, gt_b, gt_l, preds_2d, metas, None, [old_logits], None,
                              fused=path == "k38")
        sum(out[k] for k in names).backward()
        last[path] = out
        if path == "k38":
            last["source_counts"] = refine._last_assignment["source_counts"]

    paths = ["k38"] + ([] if args.only_fused else ["torch_restatement", "k37"])
    for _ in range(args.warmup):
        for path in paths:
            step(path)
    times = {path: [] for path in paths}
    for _ in range(args.steps):
        for path in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(path)
            torch.cuda.synchronize()
            times[path].append((time.perf_counter() - t0) * 1e3)
    result = dict(n_queries=n, num_boxes=int(boxes.shape[0]), num_cams=6, num_classes=10, code_size=10, steps=args.steps,
                  num_pos=float(last["k38"]["num_pos_preds" + suffix]), assigned_gts=float(last["k38"]["assigned_gts" + suffix]),
                  source_counts=[int(v) for v in last["source_counts"].tolist()])
    for path in paths:
        result[f"{path}_ms_median"] = round(statistics.median(times[path]), 4)
        result[f"{path}_ms_min"] = round(min(times[path]), 4)
    if not args.only_fused:
        result["speedup_median"] = round(result["torch_restatement_ms_median"] / result["k38_ms_median"], 2)
        result["distance_step_ms_median"] = round(result["k38_ms_median"] - result["k37_ms_median"], 4)
        result["num_pos_k37"] = float(last["k37"]["num_pos_preds" + suffix])
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
