"""Inputs and the host specification of the bilinear image-feature gather's backward (K13c), shared by
tests/test_bilinear_backward_cpu.py and tests/test_bilinear_backward_gpu.py (a plain helper module; test infrastructure, so it may
import `oracle`).

Selections `S(n1, n2, n0)` of the 1-sweep synthetic frame (seed 3): the first n1 points seen by exactly one camera, then the first n2
seen by two or more, then the first n0 seen by none — with a coarse map the near-range points pile hundreds of taps on one texel, which
is where a gather-by-texel backward can go wrong (long runs, chunk boundaries), the two-camera points exercise `reduce_cams`, the
unseen ones the sentinel.

`bilinear_taps_host` restates the kernel's tap arithmetic (csrc/bilinear_taps.h) as separately rounded numpy fp32 steps on the oracle's
grid; `bilinear_backward_host` is its exact transpose accumulated in float64.
"""
import functools

import numpy as np

from fullysparsefusion_amd import synthetic
from oracle import project as oproj

IMG_HW = (900, 1600)

# (n1, n2, n0), (Hf, Wf): the three rows every backward test runs
ROWS = {
    "coarse_3x4": ((4000, 96, 200), (3, 4)),
    "single_1x1": ((4000, 96, 200), (1, 1)),
    "sparse_29x50": ((3000, 96, 300), (29, 50)),
}


# the 1 x 1 row scaled up: one corner's run (the piece the device cuts into chunks) spans several whole chunks and a tail
LONG_RUN = (6000, 96, 200)


@functools.lru_cache(maxsize=None)
def frame():
    f = synthetic.make_frame(num_sweeps=1, seed=3)
    pts = np.ascontiguousarray(f["points"][:, 5:8]).astype(np.float32)
    L = np.asarray(f["lidar2img"], dtype=np.float32)
    seen = (oproj.prj_points_2d(pts, L, *IMG_HW)[:, :, 0] > -1.5).sum(0)  # cameras that see each point
    pts.setflags(write=False)
    L.setflags(write=False)
    return pts, L, seen


@functools.lru_cache(maxsize=None)
def selection(n1, n2, n0):
    """S(n1, n2, n0): (points f32 [n1 + n2 + n0, 3], lidar2img f32 [6, 4, 4]), read-only."""
    pts, L, seen = frame()
    one, two, none = np.nonzero(seen == 1)[0], np.nonzero(seen >= 2)[0], np.nonzero(seen == 0)[0]
    assert len(one) >= n1 and len(two) >= n2 and len(none) >= n0, (len(one), len(two), len(none))
    sel = np.ascontiguousarray(pts[np.concatenate([one[:n1], two[:n2], none[:n0]])])
    sel.setflags(write=False)
    return sel, L


def class_sizes():
    seen = frame()[2]
    return int((seen == 1).sum()), int((seen >= 2).sum()), int((seen == 0).sum())


def bilinear_taps_host(pts, L, img_hw, Hf, Wf, with_corner=False):
    """(texel index i64 [n, ncam, 4] = y * Wf + x of the clamped corner, weight f32 [n, ncam, 4], inside bool [n, ncam, 4], valid bool
    [n, ncam]); corners in the order (dy, dx) = 00, 01, 10, 11.  The weight is zero when the corner is outside the map or the projection
    is invalid; every step is one fp32 operation, in the kernel's order.  `with_corner`: also the top-left corner (x0, y0) i64 [n, ncam]."""
    grid = oproj.prj_points_2d(pts, L, img_hw[0], img_hw[1])  # [ncam, n, 2]; -2 where invalid
    valid = (grid[:, :, 0] > -1.5).T
    one, half = np.float32(1.0), np.float32(0.5)
    gx, gy = np.ascontiguousarray(grid[:, :, 0].T), np.ascontiguousarray(grid[:, :, 1].T)  # [n, ncam]
    ix = ((gx + one) * np.float32(Wf) - one) * half
    iy = ((gy + one) * np.float32(Hf) - one) * half
    x0f, y0f = np.floor(ix), np.floor(iy)
    wx1, wy1 = ix - x0f, iy - y0f
    wx0, wy0 = one - wx1, one - wy1
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    assert all(a.dtype == np.float32 for a in (ix, iy, wx1, wy1, wx0, wy0))
    idx = np.empty(gx.shape + (4,), dtype=np.int64)
    w = np.empty(gx.shape + (4,), dtype=np.float32)
    inside = np.empty(gx.shape + (4,), dtype=bool)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        xk, yk = x0 + dx, y0 + dy
        inside[..., k] = (xk >= 0) & (xk < Wf) & (yk >= 0) & (yk < Hf)
        prod = (wx1 if dx else wx0) * (wy1 if dy else wy0)
        w[..., k] = np.where(valid & inside[..., k], prod, np.float32(0.0))
        idx[..., k] = np.clip(yk, 0, Hf - 1) * Wf + np.clip(xk, 0, Wf - 1)
    if with_corner:
        return idx, w, inside, valid, x0, y0
    return idx, w, inside, valid


def largest_cell_run(pts, L, Hf, Wf):
    """The longest run the device walks in one piece: valid (point, camera) pairs sharing a camera and a top-left corner (x0, y0)."""
    _, _, _, valid, x0, y0 = bilinear_taps_host(pts, L, IMG_HW, Hf, Wf, with_corner=True)
    assert valid.any() and x0[valid].min() >= -1 and x0[valid].max() <= Wf - 1 and y0[valid].min() >= -1 and y0[valid].max() <= Hf - 1
    cam = np.broadcast_to(np.arange(valid.shape[1])[None, :], valid.shape)
    cell = cam * ((Hf + 1) * (Wf + 1)) + (y0 + 1) * (Wf + 1) + (x0 + 1)
    return int(np.bincount(cell[valid]).max())


def bilinear_backward_host(pts, L, u, img_hw, Hf, Wf, reduce_cams=False):
    """The exact transpose of the gather on `bilinear_taps_host`'s fp32 weights, in float64: u f32 [n, ncam, C] (or [n, C] with
    `reduce_cams`) -> dict(ref f64 [ncam, Hf, Wf, C] = sum a * u, mag f64 [ncam, Hf, Wf, C] = sum |a * u|, taps i64 [ncam, Hf, Wf] =
    the non-zero taps on each texel)."""
    u = np.asarray(u, dtype=np.float32)
    idx, w, _, _ = bilinear_taps_host(pts, L, img_hw, Hf, Wf)
    n, ncam = idx.shape[:2]
    C = u.shape[-1]
    rows = np.broadcast_to(u[:, None, :], (n, ncam, C)) if reduce_cams else u
    assert rows.shape == (n, ncam, C)
    flat = idx + (np.arange(ncam, dtype=np.int64) * (Hf * Wf))[None, :, None]  # [n, ncam, 4]
    ref = np.zeros((ncam * Hf * Wf, C), dtype=np.float64)
    mag = np.zeros((ncam * Hf * Wf, C), dtype=np.float64)
    taps = np.zeros((ncam * Hf * Wf,), dtype=np.int64)
    nz = w != 0
    ii, cc, kk = np.nonzero(nz)
    contrib = w[ii, cc, kk].astype(np.float64)[:, None] * rows[ii, cc].astype(np.float64)
    np.add.at(ref, flat[ii, cc, kk], contrib)
    np.add.at(mag, flat[ii, cc, kk], np.abs(contrib))
    np.add.at(taps, flat[ii, cc, kk], 1)
    return dict(ref=ref.reshape(ncam, Hf, Wf, C), mag=mag.reshape(ncam, Hf, Wf, C), taps=taps.reshape(ncam, Hf, Wf))


def case_stats(pts, L, Hf, Wf):
    """The counts of the issue's case table for one (selection, map)."""
    idx, w, inside, valid = bilinear_taps_host(pts, L, IMG_HW, Hf, Wf)
    ncam = idx.shape[1]
    flat = (idx + (np.arange(ncam, dtype=np.int64) * (Hf * Wf))[None, :, None])[w != 0]
    taps = np.bincount(flat, minlength=ncam * Hf * Wf)
    return dict(rows=int(pts.shape[0]), valid_pairs=int(valid.sum()), nonzero_taps=int((w != 0).sum()),
                outside_corners=int((valid[..., None] & ~inside).sum()), largest_run=int(taps.max()), empty_texels=int((taps == 0).sum()),
                texels=int(taps.size), texels_256=int((taps >= 256).sum()), min_run=int(taps.min()),
                two_camera_points=int((valid.sum(1) >= 2).sum()), unseen_points=int((valid.sum(1) == 0).sum()))


def tolerance(host):
    """Per element: (m_t + 1) * 2^-24 * sum |a_k u_k| — the bound of a fixed-order fp32 sum of m_t rounded products under any
    association (each product rounds once, a sum of m terms rounds m - 1 times)."""
    return (host["taps"][..., None] + 1) * 2.0 ** -24 * host["mag"]
