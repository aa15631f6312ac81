"""Times the train-time augmentation (K40) on the 10-sweep synthetic frame (`synthetic.make_frame`, ~310 k x 8) with 44 GT rows
(`synthetic.make_gt_boxes`), the nuScenes train pipeline's parameters:

    call_wall        one `DeviceTrainAugment` call, draws to sliced outputs, including its one host wait (the count read-back): host clock
                     between two device synchronisations
    points_device    the K40a -> radix sort -> K40b sequence alone (`hip_ops_augment.train_augment_points`, no read-back): device events
    boxes_device     K40c alone (`hip_ops_augment.train_augment_boxes`): device events
    host_spec_wall   the host specification (`augment_points_host` + `augment_boxes_host`) for the same frame and draws on this machine's CPU

    python tools/profiling/train_augment_time.py [--steps 50] [--warmup 10] [--host-steps 5] [--out FILE.json] [--only-device]

Prints one JSON line (median / min in ms).  `--only-device` runs the two device paths alone, `--steps` times each (for a kernel trace)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from fullysparsefusion_amd import hip_ops_augment, synthetic  # noqa: E402
from fullysparsefusion_amd.mmdet3d_plugin.datasets.train_augment import (DeviceTrainAugment, augment_boxes_host,  # noqa: E402
                                                                         augment_points_host, train_descriptor)

RANGE = [-50, -50, -4.99, 50, 50, 2.99]
FLIP = dict(flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5)
RST = dict(rot_range=[-0.785, 0.785], scale_ratio_range=[0.9, 1.1], translation_std=[0.5, 0.5, 0.5])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-device", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    frame = synthetic.make_frame(num_sweeps=10, seed=0)
    boxes, labels = synthetic.make_gt_boxes(frame["points"], seed=0)
    pts_host, boxes_host, labels_host = torch.from_numpy(frame["points"]), torch.from_numpy(boxes), torch.from_numpy(labels)
    pts, gt_b, gt_l = pts_host.to(dev), boxes_host.to(dev), labels_host.to(dev)
    augment = DeviceTrainAugment(FLIP, RST, RANGE)
    rng = np.random.RandomState(0)
    aug = augment.draw(rng)
    desc = train_descriptor(aug)
    offsets = [0, boxes.shape[0]]

    def points_device():
        return hip_ops_augment.train_augment_points(pts, desc, RANGE, aug["shuffle_seed"])

    def boxes_device():
        return hip_ops_augment.train_augment_boxes(gt_b, gt_l, gt_b, gt_l, offsets, [desc], RANGE)

    def call_wall():
        return augment([pts], [gt_b], [gt_l], [dict()], rng=rng)

    def host_spec_wall():
        augment_points_host(pts_host, aug, RANGE)
        augment_boxes_host(boxes_host, labels_host, boxes_host, labels_host, aug, RANGE)

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def wall(fn, sync=True):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    device_paths = dict(points_device=points_device, boxes_device=boxes_device)
    for _ in range(args.warmup):
        for fn in device_paths.values():
            fn()
        if not args.only_device:
            call_wall()
    times = {k: [] for k in list(device_paths) + ([] if args.only_device else ["call_wall", "host_spec_wall"])}
    for _ in range(args.steps):  # the paths alternate step by step: all see the same clocks
        for k, fn in device_paths.items():
            times[k].append(events(fn))
        if not args.only_device:
            times["call_wall"].append(wall(call_wall))
    if not args.only_device:
        for _ in range(args.host_steps):
            times["host_spec_wall"].append(wall(host_spec_wall, sync=False))
    torch.cuda.synchronize()
    kept = int(points_device()[1])
    n, cols = int(pts.shape[0]), int(pts.shape[1])
    # what the algorithm needs: K40a reads xyz and writes a 12-byte pair per row, the sort reads the keys once for its histograms and
    # reads + writes the pairs in each of 4 passes, K40b reads an index and a row and writes a row per survivor
    moved = n * (12 + 12 + 8 + 4 * 2 * 12) + kept * (4 + 2 * 4 * cols)
    result = dict(n_points=n, cols=cols, kept_points=kept, num_boxes=int(boxes.shape[0]), steps=args.steps, host_steps=args.host_steps,
                  cpu_threads=torch.get_num_threads(), bytes_moved_points=moved)
    for k, v in times.items():
        result[f"{k}_ms_median"] = round(statistics.median(v), 4)
        result[f"{k}_ms_min"] = round(min(v), 4)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
