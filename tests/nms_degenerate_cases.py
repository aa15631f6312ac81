"""Pair-probe layouts for the rotated BEV NMS (K20) on degenerate box pairs: shared by tests/test_nms_degenerate_cpu.py (the float64
reference alone: closed forms against the oracle, the cap on undecided decisions) and tests/test_nms_degenerate_gpu.py.

A layout holds K pairs.  A_p sits on a square grid whose spacing exceeds the reach of a pair (A's circumscribed radius + the largest
offset of B + B's radius + another A's radius), so the A boxes never overlap each other and B_p overlaps A_p only.  With the A boxes
first ("ab") the greedy scan keeps every A and keeps B_p iff IoU(A_p, B_p) <= thresh; with the B boxes first ("ba") the roles swap.
Pads (small boxes far from every pair, only there to push a call over the cell-grid threshold) are always kept.

Tolerance (derived, docs/kernels/K17_K20_K24_refine_tail.md): tol = 64 * 2^-23 * max|coordinate| / min side over the layout's pairs;
a decision with |IoU - thresh| <= tol is undecided and may go either way.  The 0.05 m-in-3 x 12 m family has the bound of its own
geometry.  Every layout keeps |coordinate| <= 100 m and sides >= 0.5 m (except that family's small boxes)."""
import functools

import numpy as np

from oracle import refine as orefine

FAMILIES = ("identical", "pi_flip", "swap_wl", "jitter", "nested_same_yaw", "nested_other_yaw", "slid", "shared_edge", "shared_corner",
            "cross90", "exact_yaw", "tiny_in_huge", "generic")
THRESHOLDS = tuple(np.round(np.linspace(0.05, 0.95, 19), 3)) + (0.999,)
EPS32 = 2.0 ** -23
MAX_UNDECIDED = 0.01

# (name, pairs per side of the grid, grid spacing [m], (w range), (l range), pads): "small" takes the all-pairs mask kernel (n = 512),
# "grid" the cell-grid path (n = 2048), "big" the cell-grid path's big list (radius > 4 m; n = 32 + 1105 pads)
SIZES = {
    "small": dict(side=16, spacing=6.2, w=(1.0, 1.4), l=(1.0, 2.0), pads=False),
    "grid": dict(side=32, spacing=6.2, w=(1.0, 1.4), l=(1.0, 2.0), pads=False),
    "big": dict(side=4, spacing=50.0, w=(2.0, 3.0), l=(8.5, 12.0), pads=True),
}


def _shift_local(cx, cy, yaw, ox, oy):
    """Centre moved by (ox, oy) in the box's own frame: the kernel's corner = centre + [[c, s], [-s, c]] @ offset."""
    c, s = np.cos(yaw), np.sin(yaw)
    return cx + c * ox + s * oy, cy - s * ox + c * oy


def _xyxyr(cx, cy, w, l, yaw):
    return np.stack([cx - w / 2, cy - l / 2, cx + w / 2, cy + l / 2, yaw], 1).astype(np.float32)


def make_pairs(family, cx, cy, w_rng, l_rng, rng):
    """K pairs of `family` with A centred at (cx, cy): (A [K,5] f32, B [K,5] f32, closed-form IoU [K] float64 or None)."""
    k = cx.shape[0]
    u = lambda lo, hi: rng.uniform(lo, hi, k)
    aw, al, ayaw = u(*w_rng), u(*l_rng), u(-3.2, 3.2)
    bx, by, bw, bl, byaw = cx, cy, aw, al, ayaw
    iou = None
    if family == "identical":
        iou = np.ones(k)
    elif family == "pi_flip":
        byaw, iou = ayaw + np.pi, np.ones(k)
    elif family == "swap_wl":
        bw, bl, byaw, iou = al, aw, ayaw + np.pi / 2, np.ones(k)
    elif family == "jitter":
        j = 10.0 ** u(-6, -4)
        bx, by, bw, bl, byaw = cx + j * u(-1, 1), cy + j * u(-1, 1), aw + j * u(-1, 1), al + j * u(-1, 1), ayaw + j * u(-1, 1)
    elif family == "nested_same_yaw":
        s = u(0.5, 0.9)
        bw, bl = aw * s, al * s
        bx, by = _shift_local(cx, cy, ayaw, u(-0.9, 0.9) * (aw - bw) / 2, u(-0.9, 0.9) * (al - bl) / 2)
        iou = bw * bl / (aw * al)
    elif family == "nested_other_yaw":
        # B's half diagonal is <= 0.43 and its centre stays (half side - 0.45) from A's centre: B lies inside A at any yaw
        bw, bl, byaw = u(0.5, 0.6), u(0.5, 0.6), u(-3.2, 3.2)
        bx, by = _shift_local(cx, cy, ayaw, u(-1, 1) * (aw / 2 - 0.45), u(-1, 1) * (al / 2 - 0.45))
        iou = bw * bl / (aw * al)
    elif family == "slid":
        d = u(0, 1.2) * al
        bx, by = _shift_local(cx, cy, ayaw, 0.0, d)
        ov = aw * np.maximum(al - d, 0.0)
        iou = ov / (2 * aw * al - ov)
    elif family == "shared_edge":
        bx, by = _shift_local(cx, cy, ayaw, 0.0, al)
        iou = np.zeros(k)
    elif family == "shared_corner":
        bx, by = _shift_local(cx, cy, ayaw, aw, al)
        iou = np.zeros(k)
    elif family == "cross90":
        byaw = ayaw + np.pi / 2
        ov = np.minimum(aw, al) ** 2
        iou = ov / (2 * aw * al - ov)
    elif family == "exact_yaw":
        yaws = np.array([0.0, np.pi / 2, -np.pi / 2, np.pi])
        ia, ib = rng.integers(0, 4, k), rng.integers(0, 4, k)
        ayaw, byaw = yaws[ia], yaws[ib]
        bw, bl = u(*w_rng), u(*l_rng)
        bx, by = cx + u(-1, 1) * w_rng[0], cy + u(-1, 1) * w_rng[0]
        ta, tb = (ia == 1) | (ia == 2), (ib == 1) | (ib == 2)  # a quarter turn swaps the extents
        ex, ey = np.where(ta, al, aw), np.where(ta, aw, al)
        fx, fy = np.where(tb, bl, bw), np.where(tb, bw, bl)
        ox = np.maximum(np.minimum(cx + ex / 2, bx + fx / 2) - np.maximum(cx - ex / 2, bx - fx / 2), 0.0)
        oy = np.maximum(np.minimum(cy + ey / 2, by + fy / 2) - np.maximum(cy - ey / 2, by - fy / 2), 0.0)
        iou = ox * oy / (aw * al + bw * bl - ox * oy)
    elif family == "tiny_in_huge":
        aw, al = np.full(k, 3.0), np.full(k, 12.0)
        bw, bl, byaw = np.full(k, 0.05), np.full(k, 0.05), u(-3.2, 3.2)
        bx, by = _shift_local(cx, cy, ayaw, u(-1.4, 1.4), u(-5.9, 5.9))
        iou = bw * bl / (aw * al)
    elif family == "generic":
        bw, bl, byaw = u(*w_rng), u(*l_rng), u(-3.2, 3.2)
        bx, by = cx + u(-1, 1) * w_rng[0], cy + u(-1, 1) * w_rng[0]
    else:
        raise KeyError(family)
    return _xyxyr(cx, cy, aw, al, ayaw), _xyxyr(bx, by, bw, bl, byaw), iou


def oracle_iou_pairs(a, b):
    """Float64 IoU of the fp32 boxes a[p], b[p] through the oracle's polygon overlap."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    ov = orefine.rotated_overlap_pairs(a, b)
    area = lambda q: (q[:, 2] - q[:, 0]) * (q[:, 3] - q[:, 1])
    return ov / np.maximum(area(a) + area(b) - ov, 1e-8)


def _pads():
    """1105 boxes of 0.6 x 0.6 m on five rows between (and outside) the rows of the `big` layout's pairs, 0.9 m apart."""
    x = -99.0 + 0.9 * np.arange(221)
    rows = np.array([-99.0, -50.0, 0.0, 50.0, 99.0])
    cx, cy = np.tile(x, rows.size), np.repeat(rows, x.size)
    return _xyxyr(cx, cy, np.full(cx.size, 0.6), np.full(cx.size, 0.6), np.linspace(-3.0, 3.0, cx.size))


@functools.lru_cache(maxsize=None)
def layout(family, size, seed=0):
    """dict(a, b, pads: f32 boxes; iou: float64 [K] reference; tol: float).  Built once per (family, size, seed) and shared."""
    cfg = SIZES[size]
    rng = np.random.default_rng([FAMILIES.index(family), sorted(SIZES).index(size), seed])
    g = (np.arange(cfg["side"]) - (cfg["side"] - 1) / 2) * cfg["spacing"]
    cx, cy = [v.ravel() for v in np.meshgrid(g, g)]
    w_rng, l_rng = cfg["w"], cfg["l"]
    if family == "tiny_in_huge":  # 3 x 12 m boxes (always on the big list): 15 x 15 pairs 13.2 m apart, or the `big` grid with its pads
        cfg = dict(SIZES["big"], side=15, spacing=13.2, pads=False) if size == "small" else SIZES["big"]
        g = (np.arange(cfg["side"]) - (cfg["side"] - 1) / 2) * cfg["spacing"]
        cx, cy = [v.ravel() for v in np.meshgrid(g, g)]
    a, b, closed = make_pairs(family, cx, cy, w_rng, l_rng, rng)
    iou = oracle_iou_pairs(a, b)  # (of the fp32 boxes as the kernel gets them; `closed` is the ideal pair's, checked on the CPU)
    pads = _pads() if cfg["pads"] else np.zeros((0, 5), np.float32)
    allb = np.concatenate([a, b])  # (the pads take part in no decision: their circles touch nothing)
    assert float(np.abs(pads[:, :4]).max(initial=0.0)) <= 100.0
    coord = float(np.abs(allb[:, :4]).max())
    sides = np.concatenate([allb[:, 2] - allb[:, 0], allb[:, 3] - allb[:, 1]])
    if family == "tiny_in_huge":
        # overlap error <= perimeter of the small box (0.2 m) x vertex error (16 ulp of the largest coordinate), union >= 36 m^2
        tol = 0.2 * 16 * EPS32 * coord / 36.0
    else:
        assert sides.min() >= 0.5 - 1e-4, (family, size, float(sides.min()))
        tol = 64 * EPS32 * coord / float(sides.min())
    assert coord <= 100.0, (family, size, coord)
    return dict(a=a, b=b, pads=pads, iou=iou, tol=tol, closed=closed)


def identical_layout(seed):
    """4096 boxes (sides 1-1.5 x 1-2.5 m, a 64 x 64 grid 3.1 m apart) and their exact copies: IoU 1 by construction."""
    rng = np.random.default_rng([99, seed])
    g = (np.arange(64) - 31.5) * 3.1
    cx, cy = [v.ravel() for v in np.meshgrid(g, g)]
    a = _xyxyr(cx, cy, rng.uniform(1.0, 1.5, 4096), rng.uniform(1.0, 2.5, 4096), rng.uniform(-3.2, 3.2, 4096))
    assert float(np.abs(a[:, :4]).max()) <= 100.0
    return a, 64 * EPS32 * float(np.abs(a[:, :4]).max()) / 1.0


def boxes_in_order(lay, order):
    first, second = (lay["a"], lay["b"]) if order == "ab" else (lay["b"], lay["a"])
    return np.concatenate([first, second, lay["pads"]])


def expected(lay, thresh):
    """(must_keep, must_drop, undecided) boolean [K] for the second box of every pair at `thresh`."""
    iou, tol = lay["iou"], lay["tol"]
    return iou < thresh - tol, iou > thresh + tol, np.abs(iou - thresh) <= tol


def undecided_fraction(lay):
    return float(np.mean([expected(lay, t)[2].mean() for t in THRESHOLDS]))
