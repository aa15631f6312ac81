"""The fused K21 + first K22s layer (fsf_sir_input_linear_segmax) against the two launches it replaces, at the nine call shapes of a
nuScenes 10-sweep frame (profiles/r6_k22_family_calls.txt): a ONE-block, ONE-layer stack through fsf_sir_stack_forward with
FSF_OPT_SIR_FUSED = 0 (K21, then K22s) and = 2 (one launch), alternating in one process, warm, timed with events.  One line per shape."""
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.environ.get("FSF_ROOT") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")))
from fullysparsefusion_amd import hip_ops as ops  # noqa: E402

dev = torch.device("cuda:0")
ROUNDS, ITERS = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("ITERS", 10))


def mk(o, i):
    return (torch.randn(o, i, device=dev) / i ** 0.5, torch.rand(o, device=dev) + 0.5, torch.randn(o, device=dev) * 0.1)


def shape(stack, block, n, m, k, r):
    """(descriptor, keyword arguments of sir_stack_forward) of one block's K21 + first layer."""
    pts, fcl = torch.randn(n, 5, device=dev) * 10, torch.randn(n, r, device=dev)
    kw = dict(points=pts, f_cluster=fcl)
    if stack == "refine":
        kw.update(extra=fcl, extra_div=10.0)
    if block == 0 and stack == "lidar":  # 11 | 33 | 131 feature columns of the frame's points through the sampling index
        P = 280000
        both = torch.randn(P, 44, device=dev)
        kw.update(feats=[both[:, :11], both[:, 11:], torch.randn(P, 132, device=dev)[:, :131]], feats_index=torch.randint(0, P, (n,), device=dev))
    elif block == 0 and stack == "refine":  # 131 point-feature columns through the pooling index + 32 image columns as they stand
        P = 280000
        kw.update(feats=[torch.randn(P, 132, device=dev)[:, :131], torch.randn(n, 32, device=dev)], feats_index=torch.randint(0, P, (n,), device=dev),
                  direct_parts=(1,))
    else:
        fc = k - 5 - (r if stack == "refine" else 0)
        kw.update(feats=torch.randn(n, (fc + 3) // 4 * 4, device=dev)[:, :fc])
    w = torch.randn(128, k, device=dev) / k ** 0.5
    layer = dict(planes_left=ops.linear_prepare_weight(w), planes_right=None, bias=None, gamma=torch.rand(128, device=dev) + 0.5,
                 beta=torch.randn(128, device=dev) * 0.1, eps=1e-3, norm="ln", act="gelu", c=128)
    desc = ops.SirStackDescriptor([dict(mlp=(mk(16, r), mk(32, 16), mk(k, 32)), mlp_eps=1e-3, mlp_act="gelu", xyz_normalizer=[20.0, 20.0, 4.0],
                                        rel_div=10.0, in_cols=k, layers=[layer])])
    kw["seg_ids"] = torch.sort(torch.randint(0, m, (n,), device=dev))[0]
    return desc, kw, m


def timed(desc, kw, m, fused):
    n = kw["points"].size(0)
    groups = torch.full((m, 128), float("-inf"), device=dev)
    rows = torch.empty((n, 128), device=dev)
    arena = torch.empty((int(ops._L().fsf_sir_stack_arena_bytes(desc.blocks, 1, n, m)),), dtype=torch.uint8, device=dev)
    old = ops.set_option(ops.OPT_SIR_FUSED, fused)
    try:
        f = lambda: ops.sir_stack_forward(desc, groups=groups, want_rows=True, rows_out=rows, arena=arena, **kw)  # noqa: E731
        f()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            f()
        e1.record()
        torch.cuda.synchronize()
    finally:
        ops.set_option(ops.OPT_SIR_FUSED, old)
    return e0.elapsed_time(e1) / ITERS * 1e3, groups, rows


SHAPES = [("lidar", 510652, 10397, [180, 133, 133], 3), ("camera", 250992, 5000, [136, 133, 133], 3), ("refine", 50000, 500, [181, 146, 146], 13)]
if os.environ.get("ROWS"):  # the same widths at other row counts (the driver's row threshold): ROWS=2000,8000,...
    SHAPES = [("lidar", int(v), max(16, int(v) // 50), [180, 133], 3) for v in os.environ["ROWS"].split(",")]
torch.manual_seed(0)
print(f"# us per call, median of {ROUNDS} rounds of {ITERS} calls each, pair and fused alternating; spread = max - min over the rounds")
print(f"# {'stack':7s} {'block':5s} {'rows':>7s} {'k':>4s} | {'pair':>7s} {'(spread)':>9s} | {'fused':>7s} {'(spread)':>9s} | fused - pair")
for stack, n, m, ks, r in SHAPES:
    for b, k in enumerate(ks):
        desc, kw, m_ = shape(stack, b, n, m, k, r)
        t = {0: [], 2: []}
        for _ in range(ROUNDS):
            for fused in (0, 2):
                us, g, rows = timed(desc, kw, m_, fused)
                t[fused].append(us)
                if fused == 0:
                    ref = (g.clone(), rows.clone())
                else:
                    assert torch.equal(ref[0], g) and torch.equal(ref[1], rows), "fused and pair differ"
        med = {f: sorted(v)[len(v) // 2] for f, v in t.items()}
        print(f"  {stack:7s} {b:5d} {n:7d} {k:4d} | {med[0]:7.1f} ({max(t[0]) - min(t[0]):7.1f}) | {med[2]:7.1f} ({max(t[2]) - min(t[2]):7.1f}) | "
              f"{med[2] - med[0]:+7.1f}", flush=True)
        del desc, kw
        torch.cuda.empty_cache()
