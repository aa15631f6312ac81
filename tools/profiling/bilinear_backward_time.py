"""Times the bilinear image-feature gather's backward (K13c) on the 10-sweep synthetic frame (`synthetic.make_frame`, ~310 k points,
6 cameras) with a C = 64 map at 113 x 200, in both layouts, `reduce_cams` off and on, against what a PyTorch user has without it:

    k13c_<layout>_<reduce>   `hip_ops_project.project_gather_bilinear_backward` (keys -> radix sort -> starts -> sum): device events
    torch_<layout>_<reduce>  the autograd backward of ONE batched `F.grid_sample(feat [6, C, Hf, Wf], grid [6, 1, n, 2])` on the same grid
                             (float atomics; the forward and the grid are built outside the timed region; one call for all cameras is
                             the form most favourable to it): device events

    python tools/profiling/bilinear_backward_time.py [--steps 100] [--warmup 20] [--runs 2] [--channels 64] [--out FILE.json] [--only-ours]

The paths alternate step by step in one process.  Prints one JSON line per run (median / min in ms, the bytes the algorithm moves)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from fullysparsefusion_amd import hip_ops, hip_ops_project, synthetic  # noqa: E402

IMG_HW = (900, 1600)
MAP_HW = (113, 200)


def device_grid(xyz, L, img_hw):
    """FSF.prj_points_2d in plain torch ops on the device: grid f32 [ncam, 1, n, 2], -2 where invalid (timing input only)."""
    p4 = torch.cat([xyz, torch.ones_like(xyz[:, :1])], 1)
    q = torch.einsum("ni,cji->cnj", p4, L)
    depth = q[..., 2]
    ok = depth > 1e-3
    d = depth.clamp(1e-5, 1e5)
    g = torch.stack([(q[..., 0] / d / img_hw[1] - 0.5) * 2, (q[..., 1] / d / img_hw[0] - 0.5) * 2], -1)
    ok = ok & (g > -1).all(-1) & (g < 1).all(-1)
    return torch.where(ok[..., None], g, torch.full_like(g, -2.0))[:, None].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-ours", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    frame = synthetic.make_frame(num_sweeps=10, seed=0)
    xyz = torch.from_numpy(np.ascontiguousarray(frame["points"][:, 5:8])).to(dev)
    L = torch.from_numpy(np.asarray(frame["lidar2img"], dtype=np.float32)).to(dev)
    n, ncam, c = xyz.size(0), L.size(0), args.channels
    hf, wf = MAP_HW
    gen = torch.Generator().manual_seed(0)
    u = {False: torch.randn(n, ncam, c, generator=gen).to(dev), True: torch.randn(n, c, generator=gen).to(dev)}
    grid = device_grid(xyz, L, IMG_HW)
    feat = torch.randn(ncam, c, hf, wf, generator=gen).to(dev)
    _, count = hip_ops.project_gather_bilinear(xyz, L, feat, IMG_HW, return_count=True)
    pairs = int(count.sum())

    paths = {}
    for last in (False, True):
        for reduce in (False, True):
            tag = f"{'channels_last' if last else 'nchw'}_{'reduce' if reduce else 'per_camera'}"
            paths[f"k13c_{tag}"] = (lambda last=last, reduce=reduce: hip_ops_project.project_gather_bilinear_backward(
                xyz, L, u[reduce], MAP_HW, IMG_HW, channels_last=last, reduce_cams=reduce))
            if args.only_ours:
                continue
            leaf = feat.clone().requires_grad_(True)
            if last:
                leaf = feat.clone().contiguous(memory_format=torch.channels_last).requires_grad_(True)
            out = F.grid_sample(leaf, grid, mode="bilinear", align_corners=False, padding_mode="zeros")  # [ncam, C, 1, n]
            gout = (u[reduce][:, None, :].expand(n, ncam, c) if reduce else u[reduce]).permute(1, 2, 0)[:, :, None].contiguous()
            paths[f"torch_{tag}"] = (lambda leaf=leaf, out=out, gout=gout: torch.autograd.grad(out, leaf, gout, retain_graph=True))

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    # what the algorithm needs: K13c-a reads a point once (12 B, its cameras share the line) and writes a 20-byte entry (key 8, value 4,
    # fractions 8); the sort reads the keys once for its histograms and reads + writes the 12-byte pairs in each pass; the starts are
    # 4 B per cell; K13c-b reads, per valid pair and corner, an index, the fractions and a row of C floats, and writes every texel
    cells = ncam * (hf + 1) * (wf + 1)
    passes = (max(cells, 1).bit_length() + 7) // 8
    entries = n * ncam
    moved = 12 * n + 20 * entries + 8 * entries + passes * 24 * entries + 4 * (cells + 1) + 4 * pairs * (4 + 8 + 4 * c) + 4 * c * ncam * hf * wf
    lines = []
    for run in range(args.runs):
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        times = {k: [] for k in paths}
        for _ in range(args.steps):  # the paths alternate step by step: all see the same clocks
            for k, fn in paths.items():
                times[k].append(events(fn))
        torch.cuda.synchronize()
        result = dict(run=run, n_points=n, ncam=ncam, channels=c, map_hw=list(MAP_HW), valid_pairs=pairs, sort_passes=passes, steps=args.steps,
                      warmup=args.warmup, bytes_moved_k13c=moved, device=torch.cuda.get_device_name(0))
        for k, v in times.items():
            result[f"{k}_ms_median"] = round(statistics.median(v), 4)
            result[f"{k}_ms_min"] = round(min(v), 4)
        lines.append(json.dumps(result))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
