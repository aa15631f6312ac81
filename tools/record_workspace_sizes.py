"""Records what every fsf_*_workspace_bytes / fsf_*_arena_bytes query of the built library answers on a table of argument tuples:
tests/golden/workspace_sizes.json, rows of {"query", "args", "bytes"}.  tests/test_workspace_layout_cpu.py holds later builds to it
(a size may shrink, never grow, and stays 0 / negative exactly where it is here).  Runs without a device.

    python tools/record_workspace_sizes.py            # rewrites the table from the library as built now

The tuples are chosen where a layout can go wrong, not from the workload: n in {0, 1, 2, 63, 64, 65}, both sides of a radix-sort
tile (RS_TILE = 2048 rows: one more block of histograms) and of a 256-byte step of the scan's tile words (64 scan tiles = 131072
rows), one large n, and every argument a query refuses.  fsf_sir_stack_arena_bytes takes its blocks as [[in_cols, [widths]], ...]."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")

N = [0, 1, 2, 63, 64, 65, 2048, 2049, 131072, 131073, 310000]
NEG = [-1]


def table():
    t = []

    def add(query, *rows):
        t.extend((query, list(r)) for r in rows)

    add("fsf_unique_rows_workspace_bytes", *[(n, 4) for n in N + NEG], (1000, 1), (1000, 3), (1000, 0))
    add("fsf_segment_plan_workspace_bytes", *[(n, max(n // 3, 0)) for n in N + NEG], (1000, 0), (1000, -1))
    add("fsf_segment_reduce_workspace_bytes", *[(n, max(n // 3, 1), c) for n in N for c in (3, 64)], (511, 7, 1), (512, 7, 1), (513, 7, 1),
        (1000, 0, 4))
    add("fsf_norm_act_backward_workspace_bytes", (1,), (3,), (64,), (65,), (256,), (0,), (-1,))
    add("fsf_column_stats_workspace_bytes", (1,), (3,), (64,), (65,), (256,), (0,), (-1,))
    add("fsf_assemble_sweeps_workspace_bytes", *[(n,) for n in N + NEG])
    add("fsf_augment_points_workspace_bytes", *[(n, a) for n in N for a in (1, 4)], (-1, 1), (100, 0), (100, -1))
    add("fsf_train_augment_points_workspace_bytes", *[(n,) for n in N + NEG])
    add("fsf_seg_targets_workspace_bytes", *[(b, n) for n in N for b in (0, 1, 65)], (-1, 10), (10, -1))
    add("fsf_seg_loss_workspace_bytes", *[(n,) for n in N + NEG])
    add("fsf_cluster_targets_workspace_bytes", *[(b, n) for n in N for b in (0, 1, 65)], (-1, 10), (10, -1))
    add("fsf_cluster_loss_workspace_bytes", *[(n,) for n in N + NEG])
    for q in ("fsf_hybrid_assign_workspace_bytes", "fsf_frustum_assign_workspace_bytes"):
        add(q, *[(b, b2, 6, n) for n in N for (b, b2) in ((0, 0), (1, 2), (65, 130))], (-1, 0, 6, 10), (1, -1, 6, 10), (1, 1, 0, 10),
            (1, 1, 6, -1), (3, 5, 1, 100))
    add("fsf_optim_workspace_bytes", (0,), (1,), (2,), (63,), (64,), (65,), (310000,), (-1,))
    add("fsf_overlap_plan_workspace_bytes", *[(n,) for n in N + NEG])
    add("fsf_project_gather_bilinear_backward_workspace_bytes", *[(n, 6, 29, 50, 64) for n in N + NEG], (341, 6, 1, 1, 1), (342, 6, 1, 1, 1),
        (10, 0, 29, 50, 64), (10, 65, 29, 50, 64), (10, 6, 0, 50, 64), (10, 6, 29, 0, 64), (10, 6, 29, 50, 0), ((1 << 32) // 6 + 1, 6, 29, 50, 64),
        (10, 64, 8191, 4095, 1))
    add("fsf_rulebook_workspace_bytes", *[(n, k) for n in N for k in (1, 8, 27)], (1000, 0))
    add("fsf_order_by_neighbor_mask_workspace_bytes", *[(n,) for n in N + NEG])
    add("fsf_rulebook_to_pairs_workspace_bytes", *[(n, k) for n in N + NEG for k in (1, 27)], (100, 0), (100, -1))
    # (ksplit > 1: few tiles and kvol >= 3; ksplit == 1: kvol < 3, or enough tiles to fill the chip)
    add("fsf_spconv_workspace_bytes", *[(n, 64, 64, 27) for n in N + NEG], (64, 64, 128, 27), (1000, 64, 128, 27), (5000, 32, 64, 27),
        (20000, 16, 16, 27), (310000, 16, 16, 27), (100, 64, 64, 1), (100, 64, 64, 2), (100, 64, 64, 3), (100, 0, 64, 27), (100, 64, 0, 27),
        (100, 64, 64, 0), (100, 64, 64, 28))
    add("fsf_spconv_split_workspace_bytes", *[(n, 64, 64, 27) for n in N + NEG], (64, 64, 128, 27), (1000, 64, 128, 27), (100, 64, 64, 1),
        (100, 0, 64, 27), (100, 64, 0, 27), (100, 64, 64, 0), (100, 64, 64, 28))
    # (this query refuses nothing and divides by its channel and offset counts: they stay >= 1 here, as its entry point demands)
    add("fsf_spconv_backward_weight_workspace_bytes", *[(n, 64, 64, 27) for n in N + NEG], (1000, 16, 128, 27), (100, 64, 64, 1),
        (100, 64, 64, 28))
    add("fsf_connected_components_workspace_bytes", *[(n,) for n in N + NEG], (255,), (256,), (257,))
    one, two, three = [[12, [64, 64]]], [[12, [64, 64]], [131, [128, 128]]], [[12, [64, 64]], [131, [128, 128]], [259, [256, 256, 128]]]
    add("fsf_sir_stack_arena_bytes", *[(b, n, max(n // 7, 1)) for b in (one, two, three) for n in (1, 2, 63, 64, 65, 310000)],
        (one, 0, 0), (one, -1, 1), (one, 1, -1), ([], 10, 2), ([[0, [64]]], 10, 2), ([[12, [6]]], 10, 2), ([[12, []]], 10, 2),
        ([[12, [64, 64, 64, 64, 64]]], 10, 2))
    add("fsf_dynamic_point_pool_workspace_bytes", *[(n, r) for n in N for r in (0, 1, 65, 300)], (-1, 10), (10, -1), (4095, 3), (4096, 3), (4097, 3))
    add("fsf_nms_bev_workspace_bytes", *[(n,) for n in N + NEG], (1023,), (1024,), (1025,), (4095,), (4096,), (4097,))
    add("fsf_nms_bev_multiclass_workspace_bytes", *[(n, c) for n in N[:8] + [4096, 4097] for c in (1, 10)], (-1, 3), (100, 0), (100, -1))
    add("fsf_nms_bev_multiclass_capped_workspace_bytes", *[(n, c, k) for n in N[:8] + [4096, 4097, 20000] for c in (1, 10) for k in (0, 100, 1000)],
        (-1, 3, 100), (100, 0, 100), (100, 3, -1))
    add("fsf_class_rank_desc_workspace_bytes", *[(n, c) for n in N for c in (1, 10)], (-1, 3), (100, 0), (100, -1))
    add("fsf_ingroup_rank_workspace_bytes", *[(n,) for n in N + NEG])
    add("fsf_cluster_key_survival_workspace_bytes", *[(m, n) for n in N for m in (0, 1, max(n // 2, 1), n)], (-1, 10), (10, -1))
    add("fsf_group_pairs_workspace_bytes", *[(n, g) for n in N for g in (1, 6)], (-1, 6), (100, 0), (100, -1), (21845, 6), (21846, 6))
    add("fsf_lidar_cluster_frontend_arena_bytes", *[(n, g, c) for n in N for (g, c) in ((1, 3), (6, 5))], (-1, 6, 5), (100, 0, 5), (100, 6, 2),
        (100, 6, 3))
    return t


def sir_blocks(spec):
    """The ctypes FsfSirBlock array of [[in_cols, [widths]], ...] (weights: a non-null address the size query never follows)."""
    from fullysparsefusion_amd import hip_ops

    arr = (hip_ops._SirBlockC * max(len(spec), 1))()
    for blk, (in_cols, widths) in zip(arr, spec):
        blk.in_cols, blk.num_layers = in_cols, len(widths)
        for layer, c in zip(blk.layer, widths):
            layer.c, layer.planes_left, layer.planes_right = c, 4096, 4096
    return arr


def ask(h, query, args):
    if query == "fsf_sir_stack_arena_bytes":
        spec, n, groups = args
        return int(h.fsf_sir_stack_arena_bytes(ctypes.byref(sir_blocks(spec)), len(spec), n, groups))
    return int(getattr(h, query)(*args))


def main():
    from fullysparsefusion_amd import _lib, build

    build.build()
    h = _lib.lib()
    queries = sorted(n for n in _lib.SIGNATURES if n.endswith(("_workspace_bytes", "_arena_bytes")))
    rows = table()
    assert sorted({q for q, _ in rows}) == queries, sorted(set(queries) ^ {q for q, _ in rows})
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps({"query": q, "args": a, "bytes": ask(h, q, a)}) for q, a in rows) + "\n]\n")
    print(f"{len(rows)} rows of {len(queries)} queries -> {OUT}")


if __name__ == "__main__":
    main()
