"""Inputs and host referees of the LiDAR -> camera projection family (K13-K16 fused and unfused, K13b, K26 and the row top-k of
csrc/project.hip), shared by tests/test_project_cases_cpu.py and tests/test_project_gpu.py (a plain helper module; test
infrastructure, so it may import `oracle`).

EXACT CAMERAS.  The image is W x H = 64 x 32, a camera's rows are [f, 0, cx, 0], [0, f, cy, 0], [0, 0, 1, 0] with f = 32, and a point is
((u - W/2) / f * z, (v - H/2) / f * z, z) with z a power of two and u, v multiples of 1/4 (a few carry 2^-15 more).  Every step of the
reference's arithmetic is then exact: px = u * z, px / pz = u, the grid value u / 32 - 1, and the nearest-pixel coordinate ix = u - 0.5.
So a point can be put exactly ON a decision: u integer is a rounding tie, u = 0 is the grid value -1.  CAM_A has (cx, cy) = (W/2, H/2);
CAM_B has (W/4, H/4) and sees the point of CAM_A's (u, v) at (u - 16, v - 8).  The id plane holds 1 + row * W + column, so an id names
its pixel.

REFEREES.  `oracle.project` is the primary one; torch's own CPU grid_sample(mode='nearest') on the oracle's grid is the independent one
(`torch_nearest_ids`).  `project_variant` restates the oracle's arithmetic with one decision switched at a time: the CPU file shows that
each wrong variant disagrees with the oracle on the group named for that decision, which is what makes the cases decisive.

THE `rx < fw`, `ry < fh`, `rx >= 0` GUARDS ARE DEFENSIVE.  A valid normalised px lies in (0, 1); in [0.5, 1) it is a multiple of 2^-24, so
gx = (px - 0.5) * 2 is a multiple of 2^-23 and at most 1 - 2^-23.  Then (gx + 1) * (W / 2) is W - W * 2^-24 before rounding, and the
deficit W * 2^-24 is at least half an ulp of the floats just below W (their ulp is at most W * 2^-23, and exactly that only above a
power of two), so the product stays below W, ix below W - 0.5, and rint gives W - 1 at most.  At the other end a valid gx + 1 is
positive, so ix >= -0.5 and rint gives -0.0 >= 0 at least.  No valid projection reaches the guards; `guard_scan` checks that on the
last 256 fp32 values at either end, for the image sizes in use, instead of hunting for an input.

OUTSIDE THE CONTRACT.  A row of `row_topk_desc` that holds INT64_MIN: the kernel uses that value as "taken", so it would be returned
once and then repeated as padding — the ids the detector passes are >= 0.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import bilinear_cases as B
from oracle import project as oproj

W, H, FOCAL = 64, 32, 32.0
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- exact cameras
def exact_camera(cx=W / 2, cy=H / 2):
    L = np.zeros((4, 4), dtype=np.float32)
    L[0, 0], L[0, 2] = FOCAL, cx
    L[1, 1], L[1, 2] = FOCAL, cy
    L[2, 2] = 1.0
    L[3, 3] = 1.0
    return L


CAM_A = exact_camera()
CAM_B = exact_camera(W / 4, H / 4)


def exact_points(uv, z=1.0):
    """Points that CAM_A projects to exactly (u, v): f32 [k, 3]; asserts that the fp32 coordinates are the exact values."""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    z = np.broadcast_to(np.asarray(z, dtype=np.float64), (uv.shape[0],))
    p = np.stack([(uv[:, 0] - W / 2) / FOCAL * z, (uv[:, 1] - H / 2) / FOCAL * z, z], 1)
    p32 = p.astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), p), "not exact in fp32"
    return p32


def id_plane():
    return (1 + np.arange(H, dtype=np.int32)[:, None] * W + np.arange(W, dtype=np.int32)[None, :]).astype(np.int32)


def oracle_project(points, mask, L):
    """oracle.project.points_in_mask (non-finite coordinates make numpy warn; the values are what the reference computes)."""
    with np.errstate(all="ignore"):
        return oproj.points_in_mask(np.ascontiguousarray(points[:, :3]), mask, L)


def torch_nearest_ids(mask, pts_2d):
    """The independent referee: torch's CPU F.grid_sample(mode='nearest', align_corners=False) on the oracle's grid -> i64 [n, ncam, ncls]."""
    out = F.grid_sample(torch.from_numpy(np.array(mask)).float(), torch.from_numpy(np.array(pts_2d))[:, None], mode="nearest",
                        align_corners=False, padding_mode="zeros")  # [ncam, ncls, 1, n]
    return out[:, :, 0].permute(2, 0, 1).long().numpy()


def score_referee(obj, anno, score_col):
    """oracle.project.cam_select_score; an id past the last annotation row scores 0 (the kernels' `id <= num_anno` guard), which is
    stated to the oracle, whose lookup has no guard, as zero rows appended to the table."""
    top = int(obj.max()) if obj.size else 0
    pad = np.zeros((max(top - anno.shape[0], 0), anno.shape[1]), dtype=np.float32)
    return oproj.cam_select_score(obj, np.concatenate([anno, pad], 0), score_col=score_col)


def project_variant(points, L, mask, rounding="even", depth_ge=False, clamp=True, strict=True):
    """The oracle's arithmetic (prj_points_2d + the nearest-pixel rule) with one decision switched: `rounding` 'even' (rintf) | 'away'
    (roundf) | 'floor' (floor(ix + 0.5)); `depth_ge`: pz >= 1e-3; `clamp`: the [1e-5, 1e5] depth clamp; `strict`: the image bounds.
    With the defaults it equals the oracle bit for bit (asserted on every case by the CPU file) -> obj i64 [n, ncam, ncls]."""
    p = np.asarray(points[:, :3], dtype=np.float32)
    ncam, ncls, h, w = mask.shape
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.zeros((p.shape[0], ncam, ncls), dtype=np.int64)
    with np.errstate(all="ignore"):
        for c in range(ncam):
            rows = []
            for j in range(3):
                m = L[c, j]
                acc = x * m[0]
                for t, k in ((y, 1), (z, 2), (np.ones_like(x), 3)):
                    acc = (t.astype(np.float64) * np.float64(m[k]) + acc.astype(np.float64)).astype(np.float32)
                rows.append(acc)
            u, v, d = rows
            dv = (d >= F32(1e-3)) if depth_ge else (d > F32(1e-3))
            if clamp:
                d = np.clip(d, F32(1e-5), F32(1e5))
            gu = (u / d / F32(w) - F32(0.5)) * F32(2)
            gv = (v / d / F32(h) - F32(0.5)) * F32(2)
            if strict:
                iv = (gu > -1.0) & (gu < 1.0) & (gv > -1.0) & (gv < 1.0)
            else:
                iv = (gu >= -1.0) & (gu <= 1.0) & (gv >= -1.0) & (gv <= 1.0)
            valid = dv & iv
            gu, gv = np.where(valid, gu, F32(-2)), np.where(valid, gv, F32(-2))
            ix = (gu + F32(1)) * (F32(w) / F32(2)) - F32(0.5)
            iy = (gv + F32(1)) * (F32(h) / F32(2)) - F32(0.5)
            if rounding == "even":
                rx, ry = np.rint(ix), np.rint(iy)
            elif rounding == "away":
                rx, ry = np.trunc(ix + np.copysign(F32(0.5), ix)), np.trunc(iy + np.copysign(F32(0.5), iy))
            else:
                rx, ry = np.floor(ix + F32(0.5)), np.floor(iy + F32(0.5))
            inb = (rx >= 0) & (rx < w) & (ry >= 0) & (ry < h)
            xi, yi = np.where(inb, rx, 0).astype(np.int64), np.where(inb, ry, 0).astype(np.int64)
            ids = mask[c][:, yi, xi].astype(np.int64)
            ids[:, ~inb] = 0
            out[:, c, :] = ids.T
    return out


def cam_select_variant(obj, anno, score_col, last_max=False, clamped_lookup=False):
    """The camera choice and score lookup with one decision switched: the LAST maximum wins; the lookup clamps an id past the table to
    its last row instead of scoring 0."""
    s = obj.sum(-1)
    cam = (s.shape[1] - 1 - s[:, ::-1].argmax(-1)) if last_max else s.argmax(-1)
    ids = obj[np.arange(obj.shape[0]), cam, :]
    score = np.zeros(ids.shape, dtype=np.float32)
    if clamped_lookup:
        ok = ids > 0
        score[ok] = anno[np.minimum(ids[ok], anno.shape[0]) - 1, score_col]
    else:
        ok = (ids > 0) & (ids <= anno.shape[0])
        score[ok] = anno[ids[ok] - 1, score_col]
    return ids, score


def guard_scan(w, count=256):
    """For an image side `w`: the last `count` fp32 values of the normalised px below 1 and above 0, and the floats around px = 2^-26 (8 below it, it, `count`
    above: the smallest px whose grid value is above -1) -> (valid bool, rx f32) of all of them, by the oracle's expressions."""
    hi = [F32(1)]
    lo = [F32(0)]
    for _ in range(count):
        hi.append(np.nextafter(hi[-1], F32(0)))
        lo.append(np.nextafter(lo[-1], F32(1)))
    first_valid = [F32(2.0 ** -26)]  # px - 0.5 rounds to -0.5 up to the tie at px = 2^-26 (half to even): the first valid px is the next float
    for _ in range(8):
        first_valid.insert(0, np.nextafter(first_valid[0], F32(0)))
    for _ in range(count):
        first_valid.append(np.nextafter(first_valid[-1], F32(1)))
    px = np.array(hi[1:] + lo[1:] + first_valid, dtype=np.float32)
    gx = (px - F32(0.5)) * F32(2)
    valid = (gx > -1.0) & (gx < 1.0)
    ix = (gx + F32(1)) * (F32(w) / F32(2)) - F32(0.5)
    return valid, np.rint(ix)


# ------------------------------------------------------------------------------------------------------------------ id-path cases
NAN, INF = float("nan"), float("inf")
NUM_ANNO = 1000      # the id plane's pixel (row 15, column 39) holds id 1000 = the last annotation row, column 40 one past it
ANNO_DIM, SCORE_COL = 6, 2


def _pixel_groups():
    zs = (1.0, 2.0, 4.0, 0.5, 8.0)
    g = {}
    g["ties_x"] = exact_points([(u, 10.75) for u in (1, 2, 3, 4, 63)], zs)
    g["ties_y"] = exact_points([(20.75, v) for v in (1, 2, 3, 4, 31)], zs)
    g["ties_xy"] = exact_points([(1, 1), (2, 2), (3, 2), (2, 3), (33, 17)], zs)
    g["border_out"] = exact_points([(0, 10.75), (W, 10.75), (20.75, 0), (20.75, H)], (1.0, 2.0, 4.0, 0.5))
    g["border_in"] = exact_points([(0.25, 10.75), (W - 0.25, 10.75), (20.75, 0.25), (20.75, H - 0.25)], (1.0, 2.0, 4.0, 0.5))
    t = F32(1e-3)
    g["depth"] = np.array([[0, 0, t], [0, 0, np.nextafter(t, F32(1))], [0, 0, 0], [0, 0, -1], [0, 0, -0.125]], dtype=np.float32)
    big = F32(1e5)
    g["depth_clamp"] = np.array([[0, 0, 2.0 ** 18], [0, 0, big], [0, 0, np.nextafter(big, F32(np.inf))]], dtype=np.float32)
    x, y, z = exact_points([(40.25, 20.25)], 2.0)[0]
    g["nonfinite"] = np.array([[NAN, y, z], [x, NAN, z], [x, y, NAN], [x, y, INF], [x, y, -INF], [INF, y, z], [x, -INF, z]], dtype=np.float32)
    g["lookup"] = np.concatenate([exact_points([(39.75, 15.75), (40.75, 15.75)], (1.0, 2.0)), np.array([[0, 0, -1]], dtype=np.float32)])
    g["second_camera"] = exact_points([(70, 20.75), (70.25, 33), (79.75, 39.75)], (1.0, 2.0, 4.0))  # outside CAM_A, inside CAM_B
    return g


@functools.lru_cache(maxsize=None)
def pixel_points():
    """(points f32 [n, 5] — xyz and two more columns —, {group: slice})."""
    g = _pixel_groups()
    sl, rows, at = {}, [], 0
    for name, p in g.items():
        sl[name] = slice(at, at + len(p))
        rows.append(p)
        at += len(p)
    xyz = np.concatenate(rows)
    pts = np.concatenate([xyz, np.full((at, 2), 7.5, dtype=np.float32)], 1)
    pts.setflags(write=False)
    return pts, sl


def tiled(points, n):
    return np.ascontiguousarray(points[np.arange(n) % points.shape[0]])


def _anno(rows, dim=ANNO_DIM, seed=1):
    return np.random.default_rng(seed).uniform(0.05, 1.0, (rows, dim)).astype(np.float32)


def _choice_case():
    """Cameras (CAM_B, CAM_A, CAM_A), two class planes: per point the per-camera id sums of CHOICE_SUMS; the splits over the two classes
    differ between cameras, so the chosen ids name the chosen camera.  Point 3 is outside CAM_B (a camera that does not see the point
    counts as 0)."""
    mask = np.zeros((3, 2, H, W), dtype=np.uint8)
    cells = [((2, 3), (1, 4), (3, 0)), ((3, 0), (2, 3), (1, 4)), ((0, 0), (0, 0), (0, 0)), (None, (3, 4), (7, 0)), ((2, 0), (4, 5), (9, 0))]
    uv = [(24.75, 12.75), (28.75, 12.75), (32.75, 12.75), (4.75, 12.75), (40.75, 12.75)]
    for (u, v), per_cam in zip(uv, cells):
        ca, ra = int(u), int(v)
        for cam, ids in enumerate(per_cam):
            if ids is None:
                continue
            col, row = (ca - 16, ra - 8) if cam == 0 else (ca, ra)
            mask[cam, :, row, col] = ids
    return dict(pts=exact_points(uv, (1.0, 2.0, 4.0, 1.0, 0.5)), L=np.stack([CAM_B, CAM_A, CAM_A]), mask=mask, anno=_anno(9), score_col=SCORE_COL)


CHOICE_SUMS = ((5, 5, 3), (3, 5, 5), (0, 0, 0), (0, 7, 7), (2, 9, 9))
CHOICE_WINNER = (0, 1, 0, 1, 1)
CHOICE_IDS = ((2, 3), (2, 3), (0, 0), (3, 4), (4, 5))


def _u8_case(ncls, seed=4):
    """One camera, `ncls` u8 planes of random ids with 255 planted under the first points."""
    rng = np.random.default_rng(seed)
    mask = rng.integers(0, 256, (1, ncls, H, W)).astype(np.uint8)
    mask[0, rng.random((ncls, H, W)) < 0.4] = 0
    uv = [(10.75, 5.75), (11.75, 5.75), (50.25, 30.25), (2, 3), (63.75, 0.25), (0, 5.75), (33.25, 17.75)]
    mask[0, :, 5, 10] = 255
    mask[0, ::2, 5, 11] = 255
    return dict(pts=exact_points(uv, (1.0, 2.0, 4.0, 1.0, 0.5, 1.0, 2.0)), L=CAM_A[None].copy(), mask=mask, anno=_anno(255, 3), score_col=1)


SECOND_TRIP_POINTS = 2048 * 256 + 77     # fsf_stream_grid caps at 2048 blocks of 256
GATHER_TRIP_POINTS, GATHER_TRIP_CAMS = 32800, 64   # n * ncam > 8192 * 256 (project_gather_kernel's cap)

ID_CASES = ("pixel", "choice", "u8_ncls16", "u8_ncls17", "i32_wide", "pixel_second_trip", "cams64_second_trip")


@functools.lru_cache(maxsize=None)
def id_case(name):
    """dict(pts f32 [n, >= 3], L f32 [ncam, 4, 4], mask [ncam, ncls, H, W], anno f32 [A, D], score_col), read-only."""
    pts, _ = pixel_points()
    two = np.stack([CAM_A, CAM_B])
    planes = np.stack([id_plane()[None], id_plane()[None]])  # [2, 1, H, W]
    if name == "pixel":
        c = dict(pts=pts, L=two, mask=planes, anno=_anno(NUM_ANNO), score_col=SCORE_COL)
    elif name == "pixel_second_trip":
        c = dict(pts=tiled(pts, SECOND_TRIP_POINTS), L=two, mask=planes, anno=_anno(NUM_ANNO), score_col=SCORE_COL)
    elif name == "i32_wide":  # ids above 2^16; id 70000 + 1000 is the last annotation row
        c = dict(pts=pts, L=two, mask=planes + 70000, anno=_anno(70000 + NUM_ANNO, 3), score_col=1)
    elif name == "cams64_second_trip":
        cams = np.stack([CAM_A if k % 2 == 0 else CAM_B for k in range(GATHER_TRIP_CAMS)])
        mask = np.stack([id_plane()[None] + 3 * k for k in range(GATHER_TRIP_CAMS)]).astype(np.int32)
        c = dict(pts=tiled(np.ascontiguousarray(pts[:, :3]), GATHER_TRIP_POINTS), L=cams, mask=mask, anno=_anno(NUM_ANNO), score_col=SCORE_COL)
    elif name == "choice":
        c = _choice_case()
    elif name == "u8_ncls16":
        c = _u8_case(16)
    elif name == "u8_ncls17":
        c = _u8_case(17)
    else:
        raise KeyError(name)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def id_want(name):
    """The oracle's answers for a case: obj i64 [n, ncam, ncls], pts_2d f32 [ncam, n, 2], ids i64 / score f32 [n, ncls] of the chosen
    camera, and what the fused kernel derives from obj: fg, count, max_id."""
    c = id_case(name)
    obj, p2d = oracle_project(c["pts"], c["mask"], c["L"])
    ids, score = score_referee(obj, c["anno"], c["score_col"])
    flat = obj.reshape(obj.shape[0], -1)
    out = dict(obj=obj, pts_2d=p2d, ids=ids, score=score, fg=flat.sum(-1) > 0, count=(flat > 0).sum(-1), max_id=flat.max(-1))
    for v in out.values():
        v.setflags(write=False)
    return out


# -------------------------------------------------------------------------------------------------------------- row list (K26)
def overlap_rows_reference(obj):
    """extract_fg_pts + double_overlap_pts + get_sir_coors of the reference (FSF.py:299-308, :260-297, :373-376) on an [n, cells]
    id tensor, as index lists: (src_pt, id) per output row."""
    fg_idx = (obj.sum(-1) > 0).nonzero().squeeze(1)
    rows = obj[fg_idx]
    k = (rows > 0).sum(-1)
    src, ids = [fg_idx], [rows.max(-1)[0]]
    for kk in range(2, int(k.max()) + 1 if k.numel() else 0):
        sel = k == kk
        if int(sel.sum()) == 0:
            continue
        top = rows[sel].topk(kk, dim=-1)[0]
        for j in range(1, kk):
            src.append(fg_idx[sel])
            ids.append(top[:, j])
    return torch.cat(src), torch.cat(ids)


ROW_CASES = ("one_cell", "two_equal", "k235", "cells_254", "rows_second_trip")
SATURATED_CASES = ("cells_255", "cells_256")
K235 = (2, 3, 5, 1, 0)   # cells per point by pixel column % 5: k = 2, 3 and 5 interleaved by point index, with k = 1 and background between


def _interior(count, row0=3):
    """`count` points on distinct pixels, no ties: column 1 + i % 60, rows from `row0`."""
    i = np.arange(count)
    return exact_points(np.stack([1.75 + i % 60, row0 + 0.75 + (i // 60) % 24], 1), 2.0 ** (i % 4))


def _cells_case(zero):
    """16 cameras x 16 classes; point 0 is inside all cells but the `zero` first of (3, 200, 77): 254, 255 or 256 cells.  Point 1 is
    inside three cells, point 2 inside none."""
    mask = np.zeros((16, 16, H, W), dtype=np.uint8)
    vals = (1 + (np.arange(256) * 37) % 255).astype(np.uint8).reshape(16, 16)  # 1 .. 255, all different but the last, which repeats the first
    for j in (3, 200, 77)[:zero]:
        vals[j // 16, j % 16] = 0
    mask[:, :, 12, 20] = vals
    mask[2, 5, 12, 30], mask[9, 0, 12, 30], mask[9, 15, 12, 30] = 7, 200, 7
    return dict(pts=exact_points([(20.75, 12.75), (30.75, 12.75), (40.75, 12.75)], (1.0, 2.0, 4.0)), L=np.stack([CAM_A] * 16), mask=mask)


@functools.lru_cache(maxsize=None)
def row_case(name):
    """dict(pts, L, mask) of a row-list case."""
    border = _pixel_groups()["border_out"]
    if name == "one_cell":     # every foreground point inside exactly one cell (M = 0); even columns are background
        plane = id_plane().copy()
        plane[:, ::2] = 0
        c = dict(pts=np.concatenate([_interior(90), border]), L=CAM_A[None].copy(), mask=plane[None, None])
    elif name == "two_equal":  # two cameras, equal planes: the appended row carries the id of the own row
        c = dict(pts=np.concatenate([border, _interior(70)]), L=np.stack([CAM_A, CAM_A]), mask=np.stack([id_plane()[None]] * 2))
    elif name == "k235":
        mask = np.zeros((1, 5, H, W), dtype=np.uint8)
        col, row = np.meshgrid(np.arange(W), np.arange(H))
        for cls in range(5):
            mask[0, cls] = np.where(cls < np.array(K235)[col % 5], 1 + (col * 7 + cls * 13 + row) % 250, 0)
        c = dict(pts=_interior(150), L=CAM_A[None].copy(), mask=mask)
    elif name == "rows_second_trip":  # F and M above 524 288: every point inside two cells with different ids
        c = dict(pts=tiled(_interior(1000), SECOND_TRIP_POINTS), L=np.stack([CAM_A, CAM_A]),
                 mask=np.stack([id_plane()[None], id_plane()[None] + 5000]).astype(np.int32))
    elif name.startswith("cells_"):
        c = _cells_case(256 - int(name[6:]))
    else:
        raise KeyError(name)
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def row_want(name):
    """dict(obj i64 tensor [n, cells], src i64, ids i64 (the reference's rows), F, M, T, k i64 [n])."""
    c = row_case(name)
    obj = torch.from_numpy(oracle_project(c["pts"], c["mask"], c["L"])[0]).reshape(c["pts"].shape[0], -1)
    src, ids = overlap_rows_reference(obj)
    k = (obj > 0).sum(-1)
    return dict(obj=obj, src=src, ids=ids, k=k, F=int((k > 0).sum()), M=int((k >= 2).sum()), T=int((k - 1).clamp(min=0).sum()))


# (n, w, k, kind): the row top-k against torch.topk
TOPK_CASES = {
    "w128_k128": (33, 128, 128, "random"),
    "w1": (50, 1, 1, "random"),
    "w17_k16": (40, 17, 16, "random"),
    "all_equal": (19, 60, 4, "equal"),
    "negative": (35, 60, 5, "negative"),
    "second_trip": (8192 * 16 + 5, 60, 2, "ids"),   # row_topk_kernel: 16 rows per block, at most 8192 blocks
}


def topk_rows(name):
    n, w, k, kind = TOPK_CASES[name]
    g = torch.Generator().manual_seed(n + w)
    if kind == "equal":
        x = torch.randint(-5, 6, (n, 1), generator=g).expand(n, w).contiguous()
    elif kind == "negative":
        x = -torch.randint(1, 2 ** 40, (n, w), generator=g)
    elif kind == "ids":   # like a point's cells: a handful of small ids, duplicates among them, the rest 0
        x = torch.randint(1, 30, (n, w), generator=g) * (torch.rand((n, w), generator=g) < 0.08)
    else:
        x = torch.randint(-2 ** 62, 2 ** 62, (n, w), generator=g)
        x[:, ::3] = x[:, :1].clone()  # duplicates in every row
    return x.to(torch.int64), k


# ------------------------------------------------------------------------------------------- bilinear forward gather (K13b)
MAPS = {"1x1": (1, 1), "3x4": (3, 4), "29x50": (29, 50), "32x64": (H, W)}
CHANNELS_SCALAR = (1, 3, 15, 17, 130)      # the scalar loop: 16 lanes, one channel each
CHANNELS_FLOAT4 = (4, 64, 68, 128, 256)    # channels-last with C % 4 == 0: float4 loads, 64 channels a trip
BILINEAR_TRIP_POINTS = 16384 * 16 + 17     # project_bilinear_kernel: 16 points per block, at most 16 384 blocks
TINY = 2.0 ** -15
BILINEAR_DEPTH = slice(-6, -3)


@functools.lru_cache(maxsize=None)
def bilinear_crafted():
    """(points f32 [n, 3], lidar2img [CAM_A, CAM_B], (H, W)): a grid of exact (u, v) that on every map of MAPS reaches, in CAM_A,
    x0 = -1, x0 = Wf - 1, y0 = -1, y0 = Hf - 1, an integer ix (wx1 == 0) and four taps inside; u = k + 0.5 + 2^-15 gives a tap of
    weight 2^-15 (inside at 32.5, outside the 64-wide map at 63.5).  Then the depth
    threshold, the next float above it and a depth past the clamp (rows BILINEAR_DEPTH), then three points no camera sees."""
    us = (0.25, 63.75, 16, 32, 24, 40.5, 10.25, 47.25, 0.5, 32.5 + TINY, 63.5 + TINY)
    vs = (0.25, 31.75, 8, 16, 12.5, 20.25, 16.5 + TINY, 31.5 + TINY)
    uv = [(u, v) for v in vs for u in us]
    t = F32(1e-3)
    pts = np.concatenate([exact_points(uv, 2.0 ** (np.arange(len(uv)) % 3)),
                          np.array([[0, 0, t], [0, 0, np.nextafter(t, F32(1))], [0, 0, 2.0 ** 18]], dtype=np.float32),   # BILINEAR_DEPTH
                          np.array([[0, 0, -1], [NAN, 0, 1], [-40, 0, 1]], dtype=np.float32)])
    pts.setflags(write=False)
    return pts, np.stack([CAM_A, CAM_B]), (H, W)


@functools.lru_cache(maxsize=None)
def bilinear_selection():
    """S(200, 96, 50) of tests/bilinear_cases.py: (points, lidar2img [6, 4, 4], (900, 1600))."""
    pts, L = B.selection(200, 96, 50)
    return pts, L, B.IMG_HW


def features(ncam, c, hf, wf, seed=0):
    """f32 [ncam, C, Hf, Wf] (NCHW); the channels-last form is its permutation."""
    return np.random.default_rng(seed + 131 * c + hf).standard_normal((ncam, c, hf, wf)).astype(np.float32)


def gamma(k):
    u = 2.0 ** -24
    return k * u / (1.0 - k * u)


def gather_referee(pts, L, img_hw, feat, taps=None):
    """`bilinear_taps_host` (the fp32 weights and clamped texels, bit for bit) times the features, in float64: dict(ref = sum w * f and
    mag = sum |w * f| over a (point, camera)'s four taps, f64 [n, ncam, C]; valid bool [n, ncam]).  `taps`: (idx, w) to use instead."""
    ncam, c, hf, wf = feat.shape
    idx, w, _, valid = B.bilinear_taps_host(np.ascontiguousarray(pts[:, :3]), L, img_hw, hf, wf)
    if taps is not None:
        idx, w = taps
    texels = feat.transpose(0, 2, 3, 1).reshape(ncam, hf * wf, c).astype(np.float64)
    f = texels[np.arange(ncam)[None, :, None], idx]              # [n, ncam, 4, C]
    prod = w.astype(np.float64)[..., None] * f
    return dict(ref=prod.sum(2), mag=np.abs(prod).sum(2), valid=valid)


def gather_budget(host, reduce_cams):
    """(ref, allowed error) per output element: an output is four products, each rounded once, added left to right (the library is built
    with -ffp-contract=off): |got - ref| <= gamma_4 * mag; with `reduce_cams` each further camera adds one rounding to what came before it:
    gamma_(4 + ncam - 1) on the sums over the cameras."""
    if not reduce_cams:
        return host["ref"], gamma(4) * host["mag"]
    ncam = host["ref"].shape[1]
    return host["ref"].sum(1), gamma(4 + ncam - 1) * host["mag"].sum(1)


def gather_fp32(pts, L, img_hw, feat, reduce_cams=False):
    """The kernel's expression in numpy fp32 — ((w00 f00 + w01 f01) + w10 f10) + w11 f11, cameras added in order: shows on the CPU that
    the budget is one a correct kernel meets."""
    ncam, c, hf, wf = feat.shape
    idx, w, _, _ = B.bilinear_taps_host(np.ascontiguousarray(pts[:, :3]), L, img_hw, hf, wf)
    texels = feat.transpose(0, 2, 3, 1).reshape(ncam, hf * wf, c)
    f = texels[np.arange(ncam)[None, :, None], idx]
    p = w[..., None] * f
    assert p.dtype == np.float32
    out = ((p[:, :, 0] + p[:, :, 1]) + p[:, :, 2]) + p[:, :, 3]
    if reduce_cams:
        acc = out[:, 0]
        for cam in range(1, ncam):
            acc = out[:, cam] + acc
        return acc
    return out


def taps_mutant(pts, L, img_hw, hf, wf, kind):
    """Wrong taps: 'drop_smallest' zeroes each (point, camera)'s smallest non-zero weight; 'unclamped' gives a corner outside the map the
    weight of an inside one (it then reads the clamped neighbour texel): what dropping an `inx1` test does."""
    idx, w, inside, valid, x0, y0 = B.bilinear_taps_host(np.ascontiguousarray(pts[:, :3]), L, img_hw, hf, wf, with_corner=True)
    w = w.copy()
    if kind == "drop_smallest":
        big = np.where(w != 0, w, np.float32(np.inf))
        k = big.argmin(-1)
        has = (w != 0).any(-1)
        n, ncam = np.nonzero(has)
        w[n, ncam, k[n, ncam]] = 0
    elif kind == "unclamped":
        w2 = gather_weights_without_inside_test(pts, L, img_hw, hf, wf)
        w = np.where(valid[..., None], w2, np.float32(0))
    else:
        raise KeyError(kind)
    return idx, w


def gather_weights_without_inside_test(pts, L, img_hw, hf, wf):
    grid = oproj.prj_points_2d(np.ascontiguousarray(pts[:, :3]), L, img_hw[0], img_hw[1])
    one, half = F32(1), F32(0.5)
    gx, gy = grid[:, :, 0].T, grid[:, :, 1].T
    ix = ((gx + one) * F32(wf) - one) * half
    iy = ((gy + one) * F32(hf) - one) * half
    wx1, wy1 = ix - np.floor(ix), iy - np.floor(iy)
    wx0, wy0 = one - wx1, one - wy1
    return np.stack([wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1], -1).astype(np.float32)
