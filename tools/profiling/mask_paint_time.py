"""K34 timing (docs/kernels/K34_mask_paint.md).  Three steps, each its own process on an MI355X:

    python tools/profiling/mask_paint_time.py kernels --density default|trained --out DIR
        (run under `rocprofv3 --kernel-trace --stats -d DIR/prof_<density> -o k34 -- ...`): plans one nuScenes frame of synthetic
        detections (default: 250 instances up to 5 % area each, as synthetic.make_mask_data; trained: 40 up to 2 %), full-size
        device masks, and paints it ITERS times; writes DIR/bytes_<density>.json (bytes K34a reads, bytes K34b reads and writes)
    python tools/profiling/mask_paint_time.py wall --out DIR
        wall time of paint_device (plan + upload + K34a + K34b, synchronised) against the file route: LoadMaskFromFiles decoding the
        60 PNG planes + anno.json, then the 86.4 MB pinned host -> device copy; writes DIR/wall.json
    python tools/profiling/mask_paint_time.py summarize --out DIR
        per-kernel averages from the rocprofv3 databases + achieved bytes/s against the HBM peak -> stdout
"""
import argparse
import glob
import json
import os
import sqlite3
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12  # B/s, MI355X spec (MI355X_MICROARCH: ~6.3 TB/s achievable)
DENSITY = dict(default=(250, 0.05), trained=(40, 0.02))
ITERS, WARMUP = 50, 5


def detections(density, seed=0):
    """Packed detections of one nuScenes frame: rectangle-shaped masks like synthetic.make_mask_data, scores above 0.1."""
    from fullysparsefusion_amd.mmdet3d_plugin.datasets import mask_paint as mp

    n, max_area = DENSITY[density]
    rng = np.random.default_rng(seed)
    H, W = mp.NUSC_IMG
    boxes, crops, origins = [], [], []
    for _ in range(n):
        area = rng.uniform(0.002, max_area) * H * W
        h = int(min(H - 1, max(4, np.sqrt(area * rng.uniform(0.5, 2.0)))))
        w = int(min(W - 1, max(4, area / h)))
        y0, x0 = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
        boxes.append([x0, y0, x0 + w, y0 + h])
        crops.append(np.ones((h, w), bool))
        origins.append((y0, x0))
    scores = rng.permutation(np.linspace(0.15, 0.99, n)).astype(np.float32)
    return dict(boxes=np.asarray(boxes, np.float32), scores=scores, labels=rng.integers(0, 10, n), cams=rng.integers(0, 6, n),
                mask_crops=crops, mask_origins=np.asarray(origins))


def full_device_masks(d, device):
    import torch

    from fullysparsefusion_amd.mmdet3d_plugin.datasets import mask_paint as mp

    m = torch.zeros((len(d["scores"]),) + mp.NUSC_IMG, dtype=torch.uint8, device=device)
    for k, (crop, (y0, x0)) in enumerate(zip(d["mask_crops"], d["mask_origins"])):
        m[k, y0:y0 + crop.shape[0], x0:x0 + crop.shape[1]] = 1
    dd = {k: v for k, v in d.items() if k not in ("mask_crops", "mask_origins")}
    dd["masks"] = m
    return dd


def cmd_kernels(args):
    import torch

    from fullysparsefusion_amd.mmdet3d_plugin.datasets import mask_paint as mp

    dev = torch.device("cuda:0")
    d = detections(args.density)
    dd = full_device_masks(d, dev)
    plan = mp.plan_masks(dd)
    want = mp.paint_numpy(mp.plan_masks(d))
    for _ in range(WARMUP):
        out = mp.paint_device(plan, dev)
    assert torch.equal(out.cpu(), want), "K34 differs from the host painter"
    torch.cuda.synchronize()
    for _ in range(ITERS):
        mp.paint_device(plan, dev)
    torch.cuda.synchronize()
    geom = mp.host_geometry(mp.plan_masks(d))
    rect_bytes = int(sum(h * w for (_, _, h, w, _) in geom))
    out_bytes = int(out.numel() * out.element_size())
    info = dict(density=args.density, objects=len(d["scores"]), painted=len(plan.obj_index), iters=ITERS + WARMUP,
                k34a_read_bytes=int(len(plan.obj_index) * mp.NUSC_IMG[0] * mp.NUSC_IMG[1]),
                k34b_write_bytes=out_bytes, k34b_mask_rect_bytes=rect_bytes,
                covered_fraction=float((want != 0).float().mean()))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"bytes_{args.density}.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps(info))


def cmd_wall(args):
    import tempfile

    import torch
    from PIL import Image

    from fullysparsefusion_amd.mmdet3d_plugin.datasets import mask_paint as mp
    from fullysparsefusion_amd.mmdet3d_plugin.datasets.pipelines import LoadMaskFromFiles

    dev = torch.device("cuda:0")
    res = {}
    for density in DENSITY:
        d = detections(density)
        dd = full_device_masks(d, dev)
        t = mp.PaintMasksFromDetections(device=dev)
        for _ in range(WARMUP):
            t(dict(mask_detections=dd))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            t(dict(mask_detections=dd))
        torch.cuda.synchronize()
        res[f"device_paint_ms_{density}"] = (time.perf_counter() - t0) / 20 * 1e3
        # the file route: the writer's PNGs + anno.json, decoded by LoadMaskFromFiles, then one pinned H2D copy
        host = mp.PaintMasksFromDetections()(dict(mask_detections=d))
        with tempfile.TemporaryDirectory() as tmp:
            sd = os.path.join(tmp, "frame")
            os.makedirs(sd)
            planes = host["mask_data"].reshape(60, *mp.NUSC_IMG).numpy()
            order = mp.NUIM_CLASS_NAMES
            for p in range(60):
                Image.fromarray(planes[p]).save(os.path.join(sd, f"{p // 10}_{order[p % 10]}.png"))
            anno = [{n: [] for n in mp.NAME_NUSC} for _ in range(6)]
            for r in host["mask_anno"][host["mask_anno"][:, 8] > 0].tolist():
                anno[int(r[6])][mp.NAME_NUSC[int(r[5])]].append(dict(bbox=r[:4], score=r[4], category=int(r[5]), cam_id=int(r[6]),
                                                                      obj_id=int(r[7])))
            with open(os.path.join(sd, "anno.json"), "w") as f:
                json.dump(anno, f)
            loader = LoadMaskFromFiles(tmp)
            dst = torch.empty((6, 10) + mp.NUSC_IMG, dtype=torch.uint8, device=dev)
            for _ in range(2):
                loader(dict(sample_idx="frame"))
            t0 = time.perf_counter()
            for _ in range(5):
                r = loader(dict(sample_idx="frame"))
            decode = (time.perf_counter() - t0) / 5 * 1e3
            pinned = r["mask_data"].pin_memory()
            for _ in range(3):
                dst.copy_(pinned, non_blocking=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                dst.copy_(pinned, non_blocking=True)
            torch.cuda.synchronize()
            h2d = (time.perf_counter() - t0) / 20 * 1e3
            assert torch.equal(dst.cpu(), t(dict(mask_detections=dd))["mask_data"].cpu())
        res[f"png_decode_ms_{density}"] = decode
        res[f"h2d_pinned_ms_{density}"] = h2d
    res["mask_bytes"] = 6 * 10 * mp.NUSC_IMG[0] * mp.NUSC_IMG[1]
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "wall.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def kernel_times(db_glob):
    out = {}
    for db in glob.glob(db_glob, recursive=True):
        rows = sqlite3.connect(db).cursor().execute("select name, start, end from kernels").fetchall()
        for name, s, e in rows:
            out.setdefault(name, []).append((e - s) / 1e3)
    return out


def cmd_summarize(args):
    lines = ["# K34 kernel times, rocprofv3 --kernel-trace (one nuScenes frame, full-size device masks, averages over all calls)"]
    for density in DENSITY:
        bpath = os.path.join(args.out, f"bytes_{density}.json")
        if not os.path.exists(bpath):
            continue
        info = json.load(open(bpath))
        times = kernel_times(os.path.join(args.out, f"prof_{density}", "**", "*.db"))
        lines.append(f"## density {density}: {info['objects']} detections, {info['painted']} painted, "
                     f"{100 * info['covered_fraction']:.2f} % of pixels covered")
        for name, ts in sorted(times.items()):
            if "mask_extents" in name or "paint_kernel" in name:
                avg, mn = float(np.mean(ts)), float(np.min(ts))
                line = f"{len(ts):5d} calls  avg {avg:9.1f} us  min {mn:9.1f} us  {name[:90]}"
                if "paint_kernel" in name:
                    b = info["k34b_write_bytes"] + info["k34b_mask_rect_bytes"]
                    line += f"  | {b / 1e6:.1f} MB -> {b / (avg * 1e-6) / 1e12:.2f} TB/s = {100 * b / (avg * 1e-6) / HBM_PEAK:.0f} % of 8 TB/s"
                if "mask_extents" in name:
                    b = info["k34a_read_bytes"]
                    line += f"  | {b / 1e6:.1f} MB -> {b / (avg * 1e-6) / 1e12:.2f} TB/s = {100 * b / (avg * 1e-6) / HBM_PEAK:.0f} % of 8 TB/s"
                lines.append(line)
    wpath = os.path.join(args.out, "wall.json")
    if os.path.exists(wpath):
        w = json.load(open(wpath))
        lines.append("# wall time per frame (host clock, synchronised)")
        for k, v in w.items():
            lines.append(f"{k:28s} {v:.3f}" if isinstance(v, float) else f"{k:28s} {v}")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["kernels", "wall", "summarize"])
    ap.add_argument("--density", choices=list(DENSITY), default="default")
    ap.add_argument("--out", required=True, help="output directory")
    args = ap.parse_args()
    dict(kernels=cmd_kernels, wall=cmd_wall, summarize=cmd_summarize)[args.cmd](args)


if __name__ == "__main__":
    main()
