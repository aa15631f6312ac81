"""CPU: what the degenerate-pair NMS tests stand on.

* csrc/bev_overlap.h (the overlap text K20's kernels compile) built for the host with the address / undefined-behaviour sanitizers
  as a stand-alone program and run over the degenerate pair families plus 2 000 000 identical pairs (tests/host/bev_overlap_check.cpp).
* The float64 oracle (`oracle.refine.rotated_overlap`, `rotated_overlap_batch`, `rotated_overlap_pairs`) against closed-form areas.
* The pair-probe layouts of tests/nms_degenerate_cases.py: reference against the ideal pair's closed form, the cap on undecided
  (pair, threshold) decisions."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import nms_degenerate_cases as C
from conftest import ROOT
from oracle import refine as R

HOST_SRC = os.path.join(ROOT, "tests", "host", "bev_overlap_check.cpp")


def _host_compiler():
    for exe in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(exe)
        if path:
            return path
    return None


def test_bev_overlap_header_is_sanitizer_clean_on_the_host(tmp_path):
    """The stand-alone host build of the kernels' overlap routine: no sanitizer report, every fp32 IoU within the derived tolerance of
    its float64 value (both argument orders), non-finite / non-positive boxes never overlap, and the worst clip-polygon vertex count
    stays inside the header's capacity and at or below the count the header records."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "bev_overlap_check")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []  # (clang++ links them so by default)
    cmd = [cxx, *static, "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wno-unknown-pragmas", "-o", exe, HOST_SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    # the sanitizer runtimes are linked statically: the program runs in the environment as it is
    r = subprocess.run([exe, "2000000"], capture_output=True, text=True)
    out = r.stdout + r.stderr
    print(out)
    assert "Sanitizer" not in out and "runtime error" not in out, out
    assert r.returncode == 0, out
    m = re.search(r"worst_vertices=(\d+) beyond_eight=(\d+) pairs=(\d+) capacity=(\d+) worst_seen=(\d+) mismatches=(\d+)", out)
    assert m, out
    worst, beyond, pairs, cap, seen, bad = map(int, m.groups())
    assert bad == 0 and pairs >= 2000000 and worst <= seen <= cap  # (seen: the header's BEV_CLIP_WORST_SEEN)
    assert worst > 8 and beyond > 0  # the population does contain the polygons eight slots could not hold


# ---- the oracle against closed forms ---------------------------------------------------------------------------------------------

def _box(cx, cy, w, l, yaw):
    return np.array([cx - w / 2, cy - l / 2, cx + w / 2, cy + l / 2, yaw], dtype=np.float64)


def _shift(box, ox, oy, w=None, l=None, yaw=None):
    """A box whose centre is `box`'s moved by (ox, oy) in box's own frame (the kernel's / oracle's corner rotation)."""
    cx, cy = (box[0] + box[2]) / 2, (box[1] + box[3]) / 2
    c, s = np.cos(box[4]), np.sin(box[4])
    return _box(cx + c * ox + s * oy, cy - s * ox + c * oy, box[2] - box[0] if w is None else w, box[3] - box[1] if l is None else l,
                box[4] if yaw is None else yaw)


def _closed_form_pairs():
    """(name, a, b, area) over the table of closed forms, random poses within +-10 m."""
    rng = np.random.default_rng(3)
    out = []
    for _ in range(25):
        w, l, yaw = rng.uniform(0.5, 3.0), rng.uniform(0.5, 12.0), rng.uniform(-3.2, 3.2)
        a = _box(rng.uniform(-10, 10), rng.uniform(-10, 10), w, l, yaw)
        out.append(("identical", a, a.copy(), w * l))
        out.append(("pi_flip", a, _shift(a, 0, 0, yaw=yaw + np.pi), w * l))
        s = rng.uniform(0.3, 0.9)
        out.append(("nested_same_yaw", a, _shift(a, rng.uniform(-1, 1) * (1 - s) * w / 2, rng.uniform(-1, 1) * (1 - s) * l / 2, s * w, s * l),
                    s * w * s * l))
        d = 0.4 * min(w, l)  # a square of diagonal <= 0.57 min side around A's centre, at any yaw
        out.append(("nested_other_yaw", a, _shift(a, 0, 0, d, d, rng.uniform(-3.2, 3.2)), d * d))
        ox, oy = rng.uniform(-1.2, 1.2) * w, rng.uniform(-1.2, 1.2) * l
        w2, l2 = rng.uniform(0.5, 3.0), rng.uniform(0.5, 12.0)
        ovx = max(min(w / 2, ox + w2 / 2) - max(-w / 2, ox - w2 / 2), 0.0)
        ovy = max(min(l / 2, oy + l2 / 2) - max(-l / 2, oy - l2 / 2), 0.0)
        out.append(("aligned_offset", a, _shift(a, ox, oy, w2, l2), ovx * ovy))
        a0 = _box(a[0], a[1], w, l, 0.0)  # yaw exactly 0: world axes
        out.append(("aligned_offset_yaw0", a0, _shift(a0, ox, oy, w2, l2), ovx * ovy))
        out.append(("cross90", a, _shift(a, 0, 0, yaw=yaw + np.pi / 2), min(w, l) ** 2))
        sq = _box(a[0], a[1], w, w, yaw)
        out.append(("square_45", sq, _shift(sq, 0, 0, yaw=yaw + np.pi / 4), 8 * (np.sqrt(2) - 1) * (w / 2) ** 2))
        out.append(("shared_edge", a, _shift(a, 0, l), 0.0))
        out.append(("shared_edge_x", a, _shift(a, w, 0), 0.0))
        out.append(("shared_corner", a, _shift(a, w, l), 0.0))
    return out


def _rounding_bound(a, b):
    """What rounding both boxes to fp32 can move the overlap by: every coordinate moves by <= 2^-24 |coordinate| and the yaw by
    <= 2^-24 |yaw|, so a corner moves by delta <= 2^-24 (sqrt 2 M + |yaw| diag / 2); a boundary that moves by delta sweeps at most
    perimeter x delta of area, for each box.  (4e-7 of the area at these poses; ~1e-6 m^2 for the zero-area pairs.)"""
    m = max(np.abs(a[:4]).max(), np.abs(b[:4]).max())
    tot = 0.0
    for q in (a, b):
        w, l = q[2] - q[0], q[3] - q[1]
        tot += 2 * (w + l) * 2.0 ** -24 * (np.sqrt(2) * m + abs(q[4]) * np.hypot(w, l) / 2)
    return tot


@pytest.mark.parametrize("rounded", [False, True], ids=["float64", "fp32_rounded"])
def test_oracle_rotated_overlap_matches_closed_forms(rounded):
    """Scalar, batched and pairwise oracle overlap against the closed-form area, both argument orders.  On float64 inputs: 1e-9 of
    the larger box area (relative where the area is not 0).  On inputs rounded to fp32: the movement the rounding itself allows."""
    cases = _closed_form_pairs()
    for name, a, b, want in cases:
        scale = max((a[2] - a[0]) * (a[3] - a[1]), (b[2] - b[0]) * (b[3] - b[1]))
        if rounded:
            a, b = a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
            bound = 1e-9 * scale + _rounding_bound(a, b)
        else:
            bound = 1e-9 * (want if want > 0 else scale)
        for p, q in ((a, b), (b, a)):
            got = (R.rotated_overlap(p, q), float(R.rotated_overlap_batch(p, q[None])[0]), float(R.rotated_overlap_pairs(p[None], q[None])[0]))
            for g in got:
                assert abs(g - want) <= bound, (name, rounded, g, want, bound)
    # batched over all pairs at once == one by one
    aa, bb = np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])
    one = np.array([R.rotated_overlap(p, q) for p, q in zip(aa, bb)])
    np.testing.assert_allclose(R.rotated_overlap_pairs(aa, bb), one, rtol=0, atol=1e-9)


# ---- the GPU test's layouts, reference only --------------------------------------------------------------------------------------

def _gaps(q, r):
    """[len(q), len(r)] distance between the circumscribed circles of every box of q and every box of r (> 0: they cannot overlap)."""
    ctr = lambda v: np.stack([(v[:, 0] + v[:, 2]) / 2, (v[:, 1] + v[:, 3]) / 2], 1)
    rad = lambda v: 0.5 * np.hypot(v[:, 2] - v[:, 0], v[:, 3] - v[:, 1])
    d = ctr(q)[:, None, :] - ctr(r)[None, :, :]
    return np.hypot(d[..., 0], d[..., 1]) - rad(q)[:, None] - rad(r)[None, :]


@pytest.mark.parametrize("family", C.FAMILIES)
def test_pair_probe_layouts_are_decidable(family):
    """Per layout: inside |coordinate| <= 100 m, tol no wider than 64 * 2^-23 * 100 / 0.5; the A boxes' circles do not touch, B_p's
    circle touches no other A; the reference agrees with the ideal pair's closed form to well inside tol; at most 1 % of the
    (pair, threshold) decisions are undecided."""
    for size in C.SIZES:
        lay = C.layout(family, size)
        a, b = lay["a"].astype(np.float64), lay["b"].astype(np.float64)
        assert lay["tol"] <= 64 * C.EPS32 * 100 / 0.5
        pads = lay["pads"].astype(np.float64)
        k = len(a)
        off = ~np.eye(k, dtype=bool)
        assert _gaps(a, a)[off].min() > 1e-3 and _gaps(b, a)[off].min() > 1e-3, (family, size)
        if len(pads):
            assert min(_gaps(pads, a).min(), _gaps(pads, b).min(), _gaps(pads, pads)[~np.eye(len(pads), dtype=bool)].min()) > 1e-3
        if lay["closed"] is not None:
            assert np.abs(lay["closed"] - lay["iou"]).max() <= 0.05 * lay["tol"], (family, size)
        assert C.undecided_fraction(lay) <= C.MAX_UNDECIDED, (family, size, C.undecided_fraction(lay))


def test_identical_layouts_are_decided_at_every_threshold():
    for seed in range(8):
        a, tol = C.identical_layout(seed)
        assert tol < 1.0 - max(C.THRESHOLDS) and a.shape == (4096, 5)
        ctr = np.stack([(a[:, 0] + a[:, 2]) / 2, (a[:, 1] + a[:, 3]) / 2], 1).astype(np.float64)
        rad = 0.5 * np.hypot(a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]).astype(np.float64)
        near = np.abs(ctr[:, None, 0] - ctr[None, :, 0]) + np.abs(ctr[:, None, 1] - ctr[None, :, 1]) < 3.2  # the 4 grid neighbours
        np.fill_diagonal(near, False)
        i, j = np.nonzero(near)
        assert (np.hypot(*(ctr[i] - ctr[j]).T) - rad[i] - rad[j]).min() > 1e-3
