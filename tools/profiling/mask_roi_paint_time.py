"""K34c timing (docs/kernels/K34_mask_paint.md): a mask head's RoI maps painted directly (fsf_paint_roi_masks) against the route the
same detections took before it, one nuScenes frame at mask_paint_time.py's two densities (250 instances up to 5 % area, 40 up to 2 %).

    python tools/profiling/mask_roi_paint_time.py time --out profiles/k34c_roi_paint_time.json
        alternates two routes in one process on the same detections, device events around each, STEPS steps after WARMUP:
          (A) the paste on the device in torch (mmdet's _do_paste_mask restated: grid_sample over the whole image + `>= 0.5`, per
              camera, chunked by mmdet's 1 GiB rule), then PaintMasksFromDetections on `masks=` (K34a + K34b);
          (B) PaintMasksFromDetections on `mask_rois=` (K34c).
        Both include the host planner.  Also written: the bytes each route moves and how the two results compare.
    python tools/profiling/mask_roi_paint_time.py kernels --density default|trained
        (run under `rocprofv3 --kernel-trace --stats -d DIR/prof_<density> -o k34c -- ...`): ITERS frames of each route
    python tools/profiling/mask_roi_paint_time.py summarize --out DIR
        per-kernel averages from the rocprofv3 databases under DIR/prof_* -> stdout (profiles/k34c_roi_paint_kernel_stats.txt)
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mask_paint_time import DENSITY, HBM_PEAK, detections, kernel_times  # noqa: E402

STEPS, WARMUP, ITERS = 100, 20, 30
ROI, THR = 28, 0.5
WRITE_FLOOR_US = 11.0  # 86.4 MB at 8 TB/s (K34's write-up)
GPU_MEM_LIMIT, BYTES_PER_FLOAT = 1024 ** 3, 4  # mmdet's chunking rule of the paste


def roi_detections(density, seed=0):
    """mask_paint_time.detections with a soft 28 x 28 map per box instead of its crop: an ellipse with a sigmoid edge."""
    d = detections(density, seed)
    rng = np.random.default_rng(seed + 1)
    n = len(d["scores"])
    t = (np.arange(ROI) + 0.5) / ROI * 2 - 1
    r2 = (t[None, :, None] / rng.uniform(0.6, 1.0, (n, 1, 1))) ** 2 + (t[None, None, :] / rng.uniform(0.6, 1.0, (n, 1, 1))) ** 2
    rois = (1.0 / (1.0 + np.exp(8.0 * (r2 - 1.0)))).astype(np.float32)
    return dict(boxes=d["boxes"], scores=d["scores"], labels=d["labels"], cams=d["cams"], mask_rois=rois)


def torch_paste(rois, boxes, h, w, thr):
    """mmdet's _do_paste_mask (skip_empty=False, as on a device) + mask_thr_binary for the detections of one image, chunked as
    FCNMaskHead.get_seg_masks chunks them."""
    import torch
    import torch.nn.functional as F

    n = rois.size(0)
    out = torch.zeros((n, h, w), dtype=torch.bool, device=rois.device)
    if n == 0:
        return out
    chunks = torch.chunk(torch.arange(n, device=rois.device), int(math.ceil(n * h * w * BYTES_PER_FLOAT / GPU_MEM_LIMIT)))
    for inds in chunks:
        x0, y0, x1, y1 = torch.split(boxes[inds], 1, dim=1)
        img_y = torch.arange(0, h, device=rois.device, dtype=torch.float32) + 0.5
        img_x = torch.arange(0, w, device=rois.device, dtype=torch.float32) + 0.5
        img_y = (img_y - y0) / (y1 - y0) * 2 - 1
        img_x = (img_x - x0) / (x1 - x0) * 2 - 1
        k = img_y.size(0)
        grid = torch.stack([img_x[:, None, :].expand(k, h, w), img_y[:, :, None].expand(k, h, w)], dim=3)
        out[inds] = F.grid_sample(rois[inds][:, None], grid, align_corners=False)[:, 0] >= thr
    return out


def routes(density, dev):
    import torch

    from fullysparsefusion_amd.mmdet3d_plugin.datasets import mask_paint as mp

    d = roi_detections(density)
    h, w = mp.NUSC_IMG
    rois, boxes = torch.from_numpy(d["mask_rois"]).to(dev), torch.from_numpy(d["boxes"]).to(dev)
    per_cam = [torch.from_numpy(np.flatnonzero(d["cams"] == c)).to(dev) for c in range(mp.NUSC_CAMS)]
    small = dict(boxes=d["boxes"], scores=d["scores"], labels=d["labels"], cams=d["cams"])
    paint = mp.PaintMasksFromDetections(device=dev, mask_thr=THR)

    def route_a():
        masks = torch.empty((len(d["scores"]), h, w), dtype=torch.bool, device=dev)
        for idx in per_cam:
            masks[idx] = torch_paste(rois[idx], boxes[idx], h, w, THR)
        return paint(dict(mask_detections=dict(small, masks=masks)))["mask_data"]

    def route_b():
        return paint(dict(mask_detections=dict(small, mask_rois=rois)))["mask_data"]

    return d, route_a, route_b


def route_bytes(d, plan, mp):
    """Bytes each route moves through device memory (the planner's small tables left out)."""
    n, painted = len(d["scores"]), len(plan.obj_index)
    px = mp.NUSC_IMG[0] * mp.NUSC_IMG[1]
    out = mp.NUSC_CAMS * 10 * px
    rects = int(sum(mp.roi_rect(plan.boxes[k], mp.NUSC_IMG)[2] * mp.roi_rect(plan.boxes[k], mp.NUSC_IMG)[3] for k in plan.obj_index))
    a = dict(paste_grid_write_read=2 * n * px * 8, paste_sample_write_read=2 * n * px * 4, paste_mask_write=2 * n * px,
             k34a_read=painted * px, k34b_rect_read=rects, k34b_write=out)
    b = dict(k34c_roi_read=painted * ROI * ROI * 4, k34c_write=out)
    return dict(route_a=a, route_a_total=int(sum(a.values())), route_b=b, route_b_total=int(sum(b.values())))


def cmd_time(args):
    import torch

    from fullysparsefusion_amd.mmdet3d_plugin.datasets import mask_paint as mp

    dev = torch.device("cuda:0")
    res = dict(steps=STEPS, warmup=WARMUP, roi_size=ROI, device=torch.cuda.get_device_name(0))
    for density in DENSITY:
        d, route_a, route_b = routes(density, dev)
        plan = mp.plan_masks(d)
        want = mp.paint_numpy(plan).reshape(mp.NUSC_CAMS, 10, *mp.NUSC_IMG)
        got_b, got_a = route_b().cpu(), route_a().cpu()
        assert torch.equal(got_b, want), "K34c differs from the host painter"
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(STEPS + WARMUP)]
        for e0, e1, e2 in ev:
            e0.record()
            route_a()
            e1.record()
            route_b()
            e2.record()
        torch.cuda.synchronize()
        ta = np.array([e0.elapsed_time(e1) for e0, e1, _ in ev[WARMUP:]]) * 1e3
        tb = np.array([e1.elapsed_time(e2) for _, e1, e2 in ev[WARMUP:]]) * 1e3
        res[density] = dict(detections=len(d["scores"]), painted=len(plan.obj_index), covered_fraction=float((want != 0).float().mean()),
                            route_a_us=dict(median=float(np.median(ta)), mean=float(ta.mean()), min=float(ta.min()), p90=float(np.percentile(ta, 90))),
                            route_b_us=dict(median=float(np.median(tb)), mean=float(tb.mean()), min=float(tb.min()), p90=float(np.percentile(tb, 90))),
                            pixels_where_torch_paste_differs=int((got_a != got_b).sum()), bytes=route_bytes(d, plan, mp))
        print(density, json.dumps(res[density]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


def cmd_kernels(args):
    import torch

    _, route_a, route_b = routes(args.density, torch.device("cuda:0"))
    for _ in range(ITERS):
        route_a()
        route_b()
    torch.cuda.synchronize()


def cmd_summarize(args):
    lines = ["# K34c kernel times, rocprofv3 --kernel-trace (one nuScenes frame; route A = torch paste + K34a + K34b, route B = K34c;",
             f"# averages over all {ITERS} calls of each route)"]
    for density in DENSITY:
        times = kernel_times(os.path.join(args.out, f"prof_{density}", "**", "*.db"))
        if not times:
            continue
        lines.append(f"## density {density}: {DENSITY[density][0]} detections")
        per_frame = {}
        for name, ts in sorted(times.items(), key=lambda kv: -sum(kv[1])):
            avg, mn = float(np.mean(ts)), float(np.min(ts))
            lines.append(f"{len(ts):6d} calls  avg {avg:9.1f} us  min {mn:9.1f} us  per frame {sum(ts) / ITERS:9.1f} us  {name[:110]}")
            per_frame[name] = sum(ts) / ITERS
        roi = [float(np.mean(ts)) for name, ts in times.items() if "paint_roi_kernel" in name]
        old = [float(np.mean(ts)) for name, ts in times.items() if "paint_kernel" in name]
        if roi and old:
            lines.append(f"K34c {roi[0]:.1f} us against K34b alone on the pre-pasted masks {old[0]:.1f} us; K34c reaches "
                         f"{100 * WRITE_FLOOR_US / roi[0]:.0f} % of the {WRITE_FLOOR_US:.0f} us write floor (86.4 MB at {HBM_PEAK / 1e12:.0f} TB/s)")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["time", "kernels", "summarize"])
    ap.add_argument("--density", choices=list(DENSITY), default="default")
    ap.add_argument("--out", default=None, help="time: the JSON file; summarize: the directory holding prof_<density>")
    args = ap.parse_args()
    dict(time=cmd_time, kernels=cmd_kernels, summarize=cmd_summarize)[args.cmd](args)


if __name__ == "__main__":
    main()
