"""CPU: every scratch workspace of the C ABI has ONE layout, which its size query measures and its entry point carves.

* The size table (tests/golden/workspace_sizes.json, recorded by tools/record_workspace_sizes.py before the queries were derived from the
  layouts): a size may shrink where the hand-written sum carried slack, never grow, and is 0 / negative exactly where it was.
* One byte less than the query's answer is refused on the host with FSF_ERR_WORKSPACE, before any HIP call.
* Source: no size query adds up fsf_align_up terms, no second bump allocator, no raw pointer carving.
* FsfArena itself, as a stand-alone host program under the address / undefined-behaviour sanitizers (tests/host/arena_check.cpp)."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_workspace_sizes as rec  # noqa: E402

CSRC = os.path.join(ROOT, "fullysparsefusion_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    from fullysparsefusion_amd import _lib, build

    build.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ the size table
def test_no_size_query_grew_and_zero_stays_zero(lib):
    from fullysparsefusion_amd import _lib

    with open(os.path.join(GOLDEN, "workspace_sizes.json")) as f:
        rows = json.load(f)
    queries = sorted(n for n in _lib.SIGNATURES if n.endswith(("_workspace_bytes", "_arena_bytes")))
    assert len(queries) == 34 and sorted({r["query"] for r in rows}) == queries  # every query of the header has rows
    assert [(r["query"], r["args"]) for r in rows] == [(q, json.loads(json.dumps(a))) for q, a in rec.table()]  # ... the tool's rows
    shrunk = {}
    for r in rows:
        new, old = rec.ask(lib, r["query"], r["args"]), r["bytes"]
        if old <= 0:
            assert new == old, (r, new)  # a refusal (0, or -1 from the loss / assignment queries) stays that refusal
        else:
            assert 0 < new <= old, (r, new)
            if new < old:
                shrunk.setdefault(r["query"], set()).add(old - new)
    print({q: sorted(d) for q, d in shrunk.items()})
    # what shrank is the fixed slack of the hand-written sums (a few 256-byte slices nobody took), the same at every shape
    assert all(len(d) == 1 and min(d) % 256 == 0 for d in shrunk.values()), shrunk


# ------------------------------------------------------------------------------------------------ a short workspace, on the host
def _params(name):
    """Parameter names of a function of include/fsf_hip.h, in order."""
    from fullysparsefusion_amd import _lib

    with open(_lib.HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
    return [re.sub(r"\[\d*\]", "", p).replace("*", " ").split()[-1] for p in m.group(1).split(",")]


FAKE = 4096  # a non-null, 256-byte aligned address that is never followed: every call below is refused on the host


def _call(lib, name, ws_bytes, **kw):
    """`name` with `kw` by parameter name; every other pointer = FAKE, every other number = 0, the workspace = FAKE of ws_bytes."""
    from fullysparsefusion_amd import _lib

    args = []
    assert set(kw) <= set(_params(name)), sorted(set(kw) - set(_params(name)))
    for pname, typ in zip(_params(name), _lib.SIGNATURES[name][0]):
        if pname in ("workspace_bytes", "arena_bytes"):
            args.append(ws_bytes)
        elif pname in kw:
            args.append(kw[pname])
        elif pname in ("stream", "stream_"):
            args.append(None)
        else:
            args.append(FAKE if typ is _lib.c_p else 0)
    assert len(args) == len(_lib.SIGNATURES[name][0])
    return getattr(lib, name)(*args)


def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _f32(*v):
    return (ctypes.c_float * len(v))(*v)


def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


_SIR = [[12, [64, 64]], [131, [128, 128]]]
_SHAPE = dict(spatial_shape=_i32(41, 400, 400), ksize=_i32(3, 3, 3), dilation=_i32(1, 1, 1))
_ASSIGN = dict(n=300, xyz_stride=3, batch_idx_bytes=8, batch_stride=1, preds_stride=7, num_boxes_2d=9, ncam=6, num_samples=1, num_boxes=5,
               box_stride=7, box_cols=7, num_classes=10, code_size=8, min_pos_iou=0.1)
# (entry point, its size query, the query's arguments, the entry's arguments).  Host arrays the entry reads or writes before its
# workspace check are real; everything else is FAKE.  Left out, with the line that reaches HIP before the workspace is looked at:
#   fsf_class_rank_desc         csrc/box_tail.hip: hipMemsetAsync(count, ...) ahead of the takes (it has no up-front check)
# `less`: bytes of the query's answer that this call does not take.  fsf_connected_components (no distance table) skips the grouped
# form's tile_range slice: int2 [ceil(1000 / 256) = 4 tiles] = 32 bytes, one 256-byte slice.
SHORT = [
    ("fsf_unique_rows", "fsf_unique_rows_workspace_bytes", (1000, 4), dict(n=1000, k=4, col_min=None, col_max=None)),
    ("fsf_segment_plan_from_inverse", "fsf_segment_plan_workspace_bytes", (1000, 300), dict(n=1000, m=300)),
    ("fsf_ingroup_rank", "fsf_ingroup_rank_workspace_bytes", (1000,), dict(n=1000)),
    ("fsf_cluster_key_survival", "fsf_cluster_key_survival_workspace_bytes", (300, 1000),
     dict(m=300, n=1000, key_cols=4, batch_size=1, min_points=2, num_groups=6, counts_host=_i64(0, 0))),
    ("fsf_group_pairs", "fsf_group_pairs_workspace_bytes", (1000, 6),
     dict(n=1000, ng=6, score_stride=6, group_class_masks=None, capacity=6000, count_host=_i64(0))),
    ("fsf_rulebook_subm", "fsf_rulebook_workspace_bytes", (1000, 27), dict(m=1000, batch_size=1, **_SHAPE)),
    ("fsf_rulebook_strided", "fsf_rulebook_workspace_bytes", (1000, 27),
     dict(m=1000, batch_size=1, stride=_i32(2, 2, 2), padding=_i32(1, 1, 1), cap=8000, m_out_host=_i64(0), **_SHAPE)),
    ("fsf_order_by_neighbor_mask", "fsf_order_by_neighbor_mask_workspace_bytes", (1000,), dict(m=1000, batch_size=1, spatial_shape=_i32(41, 400, 400))),
    ("fsf_connected_components_grouped", "fsf_connected_components_workspace_bytes", (1000,), dict(n=1000, point_stride=3, num_groups=6)),
    ("fsf_connected_components", "fsf_connected_components_workspace_bytes", (1000,), dict(n=1000, point_stride=3, dist=0.5, less=256)),
    ("fsf_nms_bev", "fsf_nms_bev_workspace_bytes", (1500,), dict(n=1500, thresh=0.3)),
    ("fsf_nms_bev_multiclass", "fsf_nms_bev_multiclass_workspace_bytes", (1500, 10), dict(n=1500, num_classes=10, thresh=0.3)),
    ("fsf_nms_bev_multiclass_capped", "fsf_nms_bev_multiclass_capped_workspace_bytes", (5000, 10, 100),
     dict(n=5000, num_classes=10, thresh=0.3, max_keep=100)),
    ("fsf_hybrid_assign", "fsf_hybrid_assign_workspace_bytes", (5, 9, 6, 300), _ASSIGN),
    ("fsf_frustum_assign", "fsf_frustum_assign_workspace_bytes", (5, 9, 6, 300), dict(_ASSIGN, logits_stride=10)),
    ("fsf_dynamic_point_pool", "fsf_dynamic_point_pool_workspace_bytes", (5000, 70),
     dict(n_rois=70, roi_stride=7, box_col=0, batch_col=-1, n_pts=5000, pts_stride=3, extra_wlh=_f32(1, 1, 1), max_inbox_point=512, max_all_pts=100000)),
    ("fsf_overlap_plan", "fsf_overlap_plan_workspace_bytes", (1000,), dict(n=1000, max_cells=8, counts_host=_i64(0, 0, 0))),
    ("fsf_overlap_rows", "fsf_overlap_plan_workspace_bytes", (1000,),
     dict(n=1000, xyz_stride=3, ncam=6, elem_bytes=1, ncls=10, img_h=900, img_w=1600, num_fg=100, num_multi=10, num_extra=20)),
    ("fsf_project_gather_bilinear_backward", "fsf_project_gather_bilinear_backward_workspace_bytes", (1000, 6, 29, 50, 64),
     dict(n=1000, xyz_stride=3, ncam=6, channels=64, feat_h=29, feat_w=50, img_h=900, img_w=1600)),
    ("fsf_seg_targets", "fsf_seg_targets_workspace_bytes", (5, 1000),
     dict(n=1000, pt_stride=3, batch_idx_bytes=8, num_samples=1, num_boxes=5, box_stride=7, num_classes=10)),
    ("fsf_seg_loss_forward", "fsf_seg_loss_workspace_bytes", (1000,), dict(n=1000, num_classes=10, ld_logits=10, ld_votes=30)),
    ("fsf_cluster_targets", "fsf_cluster_targets_workspace_bytes", (5, 300),
     dict(n=300, xyz_stride=3, batch_idx_bytes=8, batch_stride=1, num_samples=1, num_boxes=5, box_stride=7, box_cols=7, num_classes=10, code_size=8)),
    ("fsf_cluster_loss_forward", "fsf_cluster_loss_workspace_bytes", (300,), dict(n=300, num_classes=10, code_size=8, ld_cls=10, ld_reg=8)),
    ("fsf_segment_reduce", "fsf_segment_reduce_workspace_bytes", (1000, 300, 64), dict(n=1000, m=300, c=64, feat_stride=64, mode=1)),
    ("fsf_assemble_sweeps", "fsf_assemble_sweeps_workspace_bytes", (1000,), dict(n_rows=1000, load_dim=5, num_sweeps=2, norm_col=-1)),
    ("fsf_augment_points", "fsf_augment_points_workspace_bytes", (1000, 2),
     dict(n_rows=1000, cols=5, num_augs=2, aug_desc=_f32(1, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 1, 0))),
    ("fsf_train_augment_points", "fsf_train_augment_points_workspace_bytes", (1000,),
     dict(n_rows=1000, cols=5, desc=_f32(1, 0, 1, 0, 0, 0, 0, 0, 0, 0), shuffle_seed=3)),
    ("fsf_spconv_forward", "fsf_spconv_workspace_bytes", (1000, 64, 128, 27), dict(m_in=1000, m_out=1000, cin=64, cout=128, kvol=27)),  # ksplit > 1
    ("fsf_spconv_forward", "fsf_spconv_workspace_bytes", (310000, 16, 16, 27), dict(m_in=310000, m_out=310000, cin=16, cout=16, kvol=27)),  # the queue alone
    ("fsf_sir_stack_forward", "fsf_sir_stack_arena_bytes", (_SIR, 1000, 40),
     dict(blocks=None, num_blocks=2, n=1000, num_groups=40)),  # (blocks: filled in below)
    ("fsf_lidar_cluster_frontend", "fsf_lidar_cluster_frontend_arena_bytes", (1000, 6, 5),
     dict(m=1000, ng=6, num_classes=10, score_stride=10, point_stride=5, point_cols=5, logit_stride=10, offset_stride=30)),
]


@pytest.mark.parametrize("entry,query,qargs,kw", SHORT, ids=[f"{c[0]}-{i}" for i, c in enumerate(SHORT)])
def test_one_byte_short_is_refused_on_the_host(lib, entry, query, qargs, kw):
    from fullysparsefusion_amd import _lib

    kw = dict(kw)
    size = rec.ask(lib, query, list(qargs)) - kw.pop("less", 0)
    assert size > 0
    if entry == "fsf_sir_stack_forward":
        blocks = rec.sir_blocks(_SIR)
        kw["blocks"] = ctypes.cast(blocks, ctypes.c_void_p)
    assert _call(lib, entry, size - 1, **kw) == _lib.DEFINES["FSF_ERR_WORKSPACE"]
    assert _call(lib, entry, 0, **kw) == _lib.DEFINES["FSF_ERR_WORKSPACE"]


# ------------------------------------------------------------------------------------------------ one definition, in the source
# queries whose entry point uses the workspace as ONE buffer and carves nothing: no layout to drift from.  Routing them through the
# 256-byte arena would change their sizes for no gain.
SINGLE_BUFFER = {
    "fsf_optim_workspace_bytes": "float64 [W] partials, indexed by the kernels (optim.hip)",
    "fsf_column_stats_workspace_bytes": "CS_BLOCKS x 2 x c partials + one counter at a fixed offset the kernels compute (batch_norm.hip)",
    "fsf_norm_act_backward_workspace_bytes": "per-workgroup column partials read back by formula (norm_act.hip)",
    "fsf_spconv_split_workspace_bytes": "the k-split partial tiles alone, `a.partial` (spconv_split.hip)",
    "fsf_spconv_backward_weight_workspace_bytes": "the nsplit partial weight gradients alone, `(float*)workspace` (spconv_bwd.hip)",
    "fsf_rulebook_to_pairs_workspace_bytes": "the [segments, kvol] counts alone, `(int32_t*)workspace` (rulebook.hip)",
}


def _query_bodies():
    out = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".hip"):
            with open(os.path.join(CSRC, f)) as fh:
                src = fh.read()
            for m in re.finditer(r'extern "C" int64_t (fsf_\w+_(?:workspace|arena)_bytes)\([^)]*\)\s*\{', src):
                depth, i = 1, m.end()
                while depth:
                    depth += {"{": 1, "}": -1}.get(src[i], 0)
                    i += 1
                out[m.group(1)] = (f, src[m.end():i])
    return out


def test_size_queries_state_no_layout_of_their_own():
    bodies = _query_bodies()
    assert len(bodies) == 34
    by_hand = {q for q, (_, body) in bodies.items() if "fsf_align_up" in body}
    assert by_hand <= set(SINGLE_BUFFER), sorted(by_hand - set(SINGLE_BUFFER))
    for q in SINGLE_BUFFER:
        assert q in bodies and "FsfArena" not in bodies[q][1] and "fsf_layout_bytes" not in bodies[q][1], q
    for q, (f, body) in bodies.items():  # every other query measures a layout (directly, through the sort's, or through another query)
        if q not in SINGLE_BUFFER:
            assert re.search(r"fsf_layout_bytes<|FsfArena::measure\(\)|radix_sort_scratch_bytes\(|fsf_\w+_workspace_bytes\(", body), (f, q)


def test_one_arena_and_no_raw_carving():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            with open(os.path.join(CSRC, f)) as fh:
                src = fh.read()
            assert "struct Bump" not in src, f
            assert not re.search(r"\+=\s*fsf_align_up", src), f  # (`base += fsf_align_up(...)` pointer carving)
            if f != "common.h":
                assert not re.search(r"struct\s+\w*Arena\b", src), f
    with open(os.path.join(CSRC, "radix_sort.h")) as fh:
        assert "struct RadixScratch" in fh.read()
    # the sorter's five buffers are taken in ONE place: nobody else sizes its histogram
    users = [f for f in sorted(os.listdir(CSRC)) if f.endswith(".hip") and "radix_num_tiles" in open(os.path.join(CSRC, f)).read()]
    assert users == [], users


# ------------------------------------------------------------------------------------------------ the arena itself
def test_arena_measures_what_it_carves_under_host_sanitizers(tmp_path):
    """tests/host/arena_check.cpp: a few hundred random take sequences (1- to 16-byte types, counts including 0 and negative) — the
    measuring arena and a real one over exactly the measured bytes agree on every offset, one byte less poisons from the failing take
    on.  Host code only, built with the host address / undefined-behaviour sanitizers and run here as a program of its own."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "arena_check")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "host", "arena_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(exe, "rb") as f:
        assert b"__asan_init" in f.read()  # the sanitizer runtime is in the program
    r = subprocess.run([exe, "400"], capture_output=True, text=True)
    out = r.stdout + r.stderr
    print(out)
    assert "Sanitizer" not in out and "runtime error" not in out, out
    assert r.returncode == 0, out
    m = re.search(r"sequences=(\d+) takes=(\d+) mismatches=(\d+)", out)
    assert m and int(m.group(1)) == 400 and int(m.group(2)) > 1000 and int(m.group(3)) == 0, out
