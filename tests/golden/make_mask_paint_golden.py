#!/usr/bin/env python
"""Generates tests/golden/mask_paint.npz by RUNNING THE REFERENCE'S OWN MASK WRITERS on seeded synthetic 2-D detections.

Needs a checkout of the reference repository (BraveGroup/FullySparseFusion), named on the command line.  Nothing of the
reference's source is copied: paint_obj, paint_obj_bbox_only, collect_obj_list, get_instance_mask, get_score_thre_topk and
save_result_format are lifted with `ast` from tools/mask_tools/save_mask_nusc.py and save_mask_argo2.py and executed with
cv2.imwrite, json.dump and os.makedirs stubbed to capture what they receive (np.bool is aliased for NumPy 2).
Only inputs and outputs are saved:

    inputs   boxes f32 [N, 4], scores f32 [N], labels i64 [N] (nuImages index), cams i64 [N], mask crops (origin, shape, packed bits)
    outputs  the written planes as nonzero runs (plane, row, col0, length, id) and the anno.json rows in file order
             (x1, y1, x2, y2, score, category, cam_id, obj_id), f64

    python tests/golden/make_mask_paint_golden.py <reference checkout>    # rewrites tests/golden/mask_paint.npz

The data avoids scores equal to float32(0.1) / float32(0.2) (NumPy 2 compares them in float32, the reference's NumPy 1 in
float64) and has distinct scores in every plane (the reference's np.argsort is unstable).
"""
import ast
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
NUIM = ["car", "truck", "trailer", "bus", "construction_vehicle", "bicycle", "motorcycle", "pedestrian", "traffic_cone", "barrier"]
NAME_TO_NUM = {"car": 0, "truck": 1, "construction_vehicle": 2, "bus": 3, "trailer": 4, "barrier": 5, "motorcycle": 6, "bicycle": 7,
               "pedestrian": 8, "traffic_cone": 9}
NAME_NUSC = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone"]
LIFT = ["paint_obj", "paint_obj_bbox_only", "collect_obj_list", "get_instance_mask", "get_score_thre_topk", "save_result_format"]


def lift(ref, script, **globs):
    """The functions LIFT names from the reference script, compiled into a namespace with stubbed cv2 / json / os."""
    src = open(os.path.join(ref, "tools/mask_tools", script)).read()
    tree = ast.parse(src)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in LIFT]
    captured = dict(planes={}, anno=None)
    cv2 = types.SimpleNamespace(imwrite=lambda path, arr: captured["planes"].__setitem__(os.path.basename(path), arr.copy()))
    json = types.SimpleNamespace(dump=lambda obj, f, **k: captured.__setitem__("anno", obj))

    class _F:
        def __init__(self, *a, **k):
            pass

    fake_os = types.SimpleNamespace(makedirs=lambda *a, **k: None, path=os.path)
    np.bool = bool  # noqa: NPY001  (removed alias the reference uses)
    ns = dict(np=np, cv2=cv2, json=json, os=fake_os, open=lambda *a, **k: _F(), nuim_class_names=NUIM, name_to_num_nusc=NAME_TO_NUM,
              name_nusc=NAME_NUSC, out_path="out", num_classes=10)
    ns.update(globs)
    exec(compile(ast.Module(body=fns, type_ignores=[]), script, "exec"), ns)
    return ns, captured


def make_dets(rng, n, cam_shapes, empty_cams, score_lo, half_boxes=True):
    """n detections over the cameras (none on empty_cams): boxes, distinct scores, labels, cams, and (origin, crop) masks."""
    cams_ok = [c for c in range(len(cam_shapes)) if c not in empty_cams]
    grid = np.arange(1, 1000, dtype=np.float64) / 1000.0
    grid = grid[(grid >= score_lo) & (np.abs(grid - 0.1) > 1e-6) & (np.abs(grid - 0.2) > 1e-6)]
    scores = rng.choice(grid, size=n, replace=False).astype(np.float32)
    cams = rng.choice(cams_ok, size=n).astype(np.int64)
    labels = rng.integers(0, 10, size=n).astype(np.int64)
    boxes, origins, crops = [], [], []
    prev = {}
    for k in range(n):
        H, W = cam_shapes[cams[k]]
        key = (cams[k], labels[k])
        if key in prev and rng.random() < 0.3:  # overlap (or hide behind) an earlier object of the same plane
            y0, x0, h, w = prev[key]
            y0, x0 = y0 + int(rng.integers(-h // 3, h // 3 + 1)), x0 + int(rng.integers(-w // 3, w // 3 + 1))
            h, w = max(2, h + int(rng.integers(-h // 2, 2))), max(2, w + int(rng.integers(-w // 2, 2)))
        else:
            h, w = int(rng.integers(4, H // 8)), int(rng.integers(4, W // 8))
            y0, x0 = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
        y0, x0 = min(max(y0, 0), H - h), min(max(x0, 0), W - w)
        prev[key] = (y0, x0, h, w)
        yy, xx = np.mgrid[0:h, 0:w]
        ell = ((yy - (h - 1) / 2) / (h / 2)) ** 2 + ((xx - (w - 1) / 2) / (w / 2)) ** 2 <= 1.0
        crop = ell & (rng.random((h, w)) < 0.97)
        origins.append((y0, x0))
        crops.append(crop)
        b = np.array([x0 - 0.5, y0 - 0.5, x0 + w + 0.5, y0 + h + 0.5], np.float64)  # exact halves: Python round is half-even
        if not half_boxes or rng.random() < 0.5:
            b += rng.uniform(-0.45, 0.45, 4)
        if rng.random() < 0.04:  # a box off the image edge: negative indices wrap, an empty slice paints nothing
            b[0], b[1] = -float(rng.integers(1, 6)) - 0.2, -float(rng.integers(1, 6)) + 0.3
        boxes.append(b)
    return dict(boxes=np.asarray(boxes, np.float32), scores=scores, labels=labels, cams=cams, origins=np.asarray(origins, np.int64),
                crops=crops)


def full_mask(d, k, shape):
    m = np.zeros(shape, dtype=bool)
    (y0, x0), c = d["origins"][k], d["crops"][k]
    m[y0:y0 + c.shape[0], x0:x0 + c.shape[1]] = c
    return m


def mmdet_results(d, cam_shapes):
    """The per-camera (bbox_result, segm_result) mmdet returns, objects of a class in input order."""
    out = []
    for cam in range(len(cam_shapes)):
        bbox, segm = [], []
        for i in range(10):
            ks = np.flatnonzero((d["cams"] == cam) & (d["labels"] == i))
            bbox.append(np.concatenate([d["boxes"][ks], d["scores"][ks, None]], 1).astype(np.float32) if len(ks) else
                        np.zeros((0, 5), np.float32))
            segm.append([full_mask(d, k, cam_shapes[cam]) for k in ks])
        out.append((bbox, segm))
    return out


def runs(planes):
    """[(plane, row, col0, length, id)] of the nonzero runs of each plane."""
    out = []
    for p, a in enumerate(planes):
        a = np.asarray(a).astype(np.int64)
        for y in np.flatnonzero(a.any(1)):
            row = a[y]
            edges = np.flatnonzero(np.diff(np.concatenate([[0], row, [0]])) != 0)
            for s, e in zip(edges[:-1], edges[1:]):
                if row[s]:
                    out.append((p, y, s, e - s, row[s]))
    return np.asarray(out, np.int32).reshape(-1, 5)


def anno_rows(anno):
    rows = []
    for cam in anno:
        objs = [o for name in NAME_NUSC for o in cam[name]] if isinstance(cam, dict) else cam
        rows += [list(o["bbox"]) + [o["score"], o["category"], o["cam_id"], o["obj_id"]] for o in objs]
    return np.asarray(rows, np.float64).reshape(-1, 8)


def pack_inputs(prefix, d, store):
    store[f"{prefix}_boxes"], store[f"{prefix}_scores"] = d["boxes"], d["scores"]
    store[f"{prefix}_labels"], store[f"{prefix}_cams"], store[f"{prefix}_origins"] = d["labels"], d["cams"], d["origins"]
    store[f"{prefix}_crop_shapes"] = np.asarray([c.shape for c in d["crops"]], np.int32)
    store[f"{prefix}_crop_bits"] = np.packbits(np.concatenate([c.reshape(-1) for c in d["crops"]]))


def main(ref):
    assert os.path.isfile(os.path.join(ref, "tools/mask_tools/save_mask_nusc.py")), f"{ref} is not a checkout of the reference"
    store = {}
    rng = np.random.default_rng(34)
    nusc_shapes = [(900, 1600)] * 6
    d = make_dets(rng, 330, nusc_shapes, empty_cams={3}, score_lo=0.02)
    pack_inputs("nusc", d, store)
    results = mmdet_results(d, nusc_shapes)
    for case, bbox_only in (("nusc", False), ("nusc_bbox", True)):
        ns, cap = lift(ref, "save_mask_nusc.py", score_thre_init=0.1, bbox_only=bbox_only)
        ns["save_result_format"](results, dict(token="frame"))
        planes = [cap["planes"][f"{cam}_{name}.png"] for cam in range(6) for name in NAME_NUSC]
        assert all(p.dtype == np.uint8 for p in planes)
        store[f"{case}_runs"], store[f"{case}_anno"] = runs(planes), anno_rows(cap["anno"])
        print(case, "painted", len(store[f"{case}_anno"]), "runs", len(store[f"{case}_runs"]))

    av2_shapes = [(2048, 1550)] + [(1550, 2048)] * 6  # ring_front_center is portrait
    d = make_dets(rng, 330, av2_shapes, empty_cams={5}, score_lo=0.05)
    pack_inputs("av2", d, store)
    results = mmdet_results(d, av2_shapes)
    ns, cap = lift(ref, "save_mask_argo2.py", score_thre_init=0.2)
    imgs = [np.zeros(s + (3,), np.uint8) for s in av2_shapes]
    ns["save_result_format"](results, imgs, dict(uuid="frame"))
    planes = [cap["planes"][f"{cam}.png"] for cam in range(7)]
    assert all(p.dtype == np.uint16 for p in planes)
    store["av2_runs"], store["av2_anno"] = runs(planes), anno_rows(cap["anno"])
    store["av2_img_shapes"] = np.asarray(av2_shapes, np.int32)
    print("av2 painted", len(store["av2_anno"]), "max id", int(store["av2_runs"][:, 4].max()), "runs", len(store["av2_runs"]))
    path = os.path.join(OUT, "mask_paint.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(f"usage: {sys.argv[0]} <reference checkout>")
    main(sys.argv[1])
