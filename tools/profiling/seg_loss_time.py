"""Times the segmentation head's targets + loss forward + loss backward (K35) on the synthetic 10-sweep frame, against the torch
restatement of the same steps (`get_targets_flat(..., fused=False)` + `losses(..., fused=False)` + autograd) on the same GPU.

    python tools/profiling/seg_loss_time.py [--steps 50] [--warmup 10] [--out FILE.json]

Each step is timed with device events around the whole step (targets, forward, backward); the host restatement's step includes
its host waits (`.item()` asserts, boolean indexing).  Prints one JSON line (median / min per step, in ms)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from fullysparsefusion_amd import synthetic  # noqa: E402
from fullysparsefusion_amd.compat import Config  # noqa: E402
from fullysparsefusion_amd.mmdet3d_plugin.registry import build_head  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "fsf_nuscenes.py"))
    head = build_head(dict(cfg.model.segmentor.segmentation_head)).to(dev)
    pts = synthetic.make_frame(num_sweeps=10, seed=0)["points"]
    boxes, labels = synthetic.make_gt_boxes(pts, seed=0)
    points = torch.from_numpy(pts).to(dev)
    bidx = torch.zeros(points.shape[0], dtype=torch.int64, device=dev)
    gt_b, gt_l = [torch.from_numpy(boxes)], [torch.from_numpy(labels)]
    c = head.num_classes
    g = torch.Generator(device=dev).manual_seed(0)
    # the inference head writes logits and votes as column blocks of one [N, 44] buffer: time those strided views
    buf = (torch.randn((points.shape[0], 4 * c), generator=g, device=dev) * 2).requires_grad_()
    logits, votes = buf[:, :c], buf[:, c:]

    def step(fused):
        buf.grad = None
        lab, tgt, msk = head.get_targets_flat(points, bidx, gt_b, gt_l, fused=fused)
        out = head.losses(logits, votes, lab, tgt, msk, fused=fused)
        (out["loss_sem_seg"] + out["loss_vote"]).backward()

    result = dict(n_points=int(points.shape[0]), num_boxes=int(boxes.shape[0]), num_logits=c, steps=args.steps)
    for name, fused in (("k35", True), ("torch_restatement", False)):
        for _ in range(args.warmup):
            step(fused)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(fused)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        result[f"{name}_ms_median"] = round(statistics.median(times), 4)
        result[f"{name}_ms_min"] = round(min(times), 4)
    result["speedup_median"] = round(result["torch_restatement_ms_median"] / result["k35_ms_median"], 2)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
