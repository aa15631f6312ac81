"""Guard bands and poison around every allocating C-ABI wrapper of hip_ops.py, and around whole passes of the detector.

Each case builds inputs once, then calls its wrapper three times: plain (as every other test does), under `guarded(0xFF)` and under
`guarded(0x00)` (tests/guarded.py).  Asserted: no guard byte of any output or scratch buffer changed; something was intercepted, and
for wrappers that take scratch a request of exactly `fsf_*_workspace_bytes` was; every returned tensor is bit-identical across the
three runs as the caller sees it (uint8 views, so NaN payloads count).  The plain run is the value reference: the rest of the suite
ties it to the oracle.  Every wrapper has a ragged case (prime row counts, channel counts that divide no tile, column slices of
NaN-filled wider buffers where the ABI takes a row stride), a minimal one (one row) and an empty one (no rows, with segments / groups /
source rows left where the two are independent) unless `NO_EMPTY` names the argument check that refuses it.

`CASES` is keyed by wrapper name; tests/test_guarded_alloc_cpu.py fails when a wrapper of hip_ops.py that allocates or takes scratch
has no key here."""
import dataclasses

import numpy as np
import pytest
import torch

from guarded import FILLS, guarded
from test_hip_ops import cloud, random_rois, sparse_sites
from test_query_glue_gpu import _gen as G  # (seed -> CPU generator)

pytestmark = pytest.mark.gpu

PC_RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]

CASES = {}   # wrapper name -> [(kind, build)], build(ops, dev) -> run() -> outputs
EXEMPT = {}  # wrapper name -> reason (only wrappers that cannot be called in isolation at all)

# key -> the argument check that refuses an input of no rows: every other key has an `empty` set (n = 0, with m > 0 where the two are
# independent).  tests/test_guarded_alloc_cpu.py holds the table to that.
_WEIGHTS = "a weight has no row count: kvol / cin / cout / k / c < 1 is FSF_ERR_INVALID_ARG in every fsf_*_prepare_weight* / transpose"
NO_EMPTY = {
    "spconv_transpose_weight": _WEIGHTS, "spconv_prepare_weight_split": _WEIGHTS, "spconv_prepare_weight_split_f16": _WEIGHTS,
    "spconv_prepare_weight_planes": _WEIGHTS, "linear_prepare_weight": _WEIGHTS, "linear_prepare_weight_f16": _WEIGHTS,
    "linear_prepare_weight_sliced": _WEIGHTS,
    "spconv_backward_weight": "the wrapper answers m_in == 0 or m_out == 0 with torch.zeros itself; the entry point is not called",
    "batch_norm_train_stats": "the wrapper asserts n >= 1 (training-mode statistics of no rows are undefined)",
    "sir_stack_forward": "n < 1 or num_groups < 1 is FSF_ERR_INVALID_ARG (sir_stack.hip, fsf_sir_stack_forward) and the wrapper asserts it",
    "lidar_cluster_frontend": "no points give no (group, point) pair: P < 1 is FSF_ERR_INVALID_ARG (lidar_frontend.hip), keep_one needs a point 0",
}


@pytest.fixture(scope="module")
def ops(device):
    from fullysparsefusion_amd import hip_ops

    return hip_ops


def cases(name, **kinds):
    """Register `factory(ops, dev, **kwargs)` once per kind (ragged=dict(...), minimal=dict(...), ...)."""
    def deco(factory):
        for kind, kw in kinds.items():
            CASES.setdefault(name, []).append((kind, lambda ops, dev, _kw=kw: factory(ops, dev, **_kw)))
        return factory
    return deco


# ------------------------------------------------------------------------------------------------ input helpers
def randn(dev, g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def randint(dev, g, lo, hi, shape, dtype=torch.int64):
    return torch.randint(lo, hi, shape, generator=g).to(dtype).to(dev)


def wide(t, left=1, right=2):
    """`t` [n, c] as a column slice of a wider NaN-filled buffer (the ABI's row stride at work)."""
    n, c = t.shape
    buf = torch.full((n, left + c + right), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, left:left + c] = t
    return buf[:, left:left + c]


def wide4(t):
    """The same with 16-byte aligned rows: 4 columns in front, row stride a multiple of 4 (the fused Linear kernels' operand form)."""
    c = t.size(1)
    return wide(t, 4, 4 + (-c) % 4)


def points5(dev, n, seed):
    return torch.from_numpy(cloud(n, seed=seed)).to(dev)


def voxel_keys(dev, n, seed, span=6):
    g = G(seed)
    return torch.stack([torch.randint(0, 2, (n,), generator=g)] + [torch.randint(0, span, (n,), generator=g) for _ in range(3)], 1).to(dev)


def gt_boxes(dev, pts, m, dim, seed):
    """m boxes (x, y, z_bottom, w, l, h, yaw[, vx, vy]) sitting on points of `pts`."""
    g = G(seed)
    if m == 0:
        return torch.zeros((0, dim), device=dev)
    ctr = pts[torch.randint(0, pts.size(0), (m,), generator=g).to(dev), :3]
    rest = torch.cat([torch.rand(m, 3, generator=g) * 4 + 1.0, torch.randn(m, dim - 6, generator=g)], 1).to(dev)
    b = torch.cat([ctr, rest], 1)
    b[:, 2] -= 1.0
    return b.contiguous()


def nms_boxes(dev, n, seed):
    rng = np.random.default_rng(seed)
    nclu = max(1, n // 6)
    ctr = rng.uniform(-40, 40, (nclu, 2))[rng.integers(0, nclu, n)] + rng.normal(0, 0.7, (n, 2))
    wl = np.stack([rng.uniform(1.5, 2.5, n), rng.uniform(3.5, 5.5, n)], 1)
    return torch.from_numpy(np.concatenate([ctr - wl / 2, ctr + wl / 2, rng.uniform(-np.pi, np.pi, (n, 1))], 1).astype(np.float32)).to(dev)


def sites(dev, m, shape, seed, batch=2):
    return torch.from_numpy(sparse_sites(np.random.default_rng(seed), batch, shape, m)).to(dev)


def camera_inputs(dev, n, ncam, ncls, H, W, seed, dtype=np.uint8):
    from fullysparsefusion_amd.synthetic import make_lidar2img, make_mask_data

    rng = np.random.default_rng(seed)
    L = torch.from_numpy(make_lidar2img(ncam, fx=0.8 * W, cx=W / 2, cy=H / 2).astype(np.float32)).to(dev)
    mask, anno = make_mask_data(rng, ncam, ncls, H, W, 12, dtype=dtype, max_area=0.3)
    anno = np.concatenate([np.zeros((1, 9), np.float32), np.asarray(anno, dtype=np.float32)])  # (a row for every id, 0 included)
    return points5(dev, n, seed), L, torch.from_numpy(mask).to(dev), torch.from_numpy(anno).to(dev)


def mlp3(dev, g, r, c):
    dims = [r, 16, 32, c]
    return [(randn(dev, g, dims[i + 1], dims[i], scale=dims[i] ** -0.5), torch.rand(dims[i + 1], generator=g).to(dev) + 0.5,
             randn(dev, g, dims[i + 1], scale=0.1)) for i in range(3)]


# ------------------------------------------------------------------------------------------------ the case table
@cases("assemble_sweeps", ragged=dict(sizes=(1009, 503, 257)), minimal=dict(sizes=(1,)), empty=dict(sizes=(0,)))
def _assemble_sweeps(ops, dev, sizes):
    raw = points5(dev, sum(sizes), 1)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    identity = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0, 0.0]
    c, s = np.cos(0.1), np.sin(0.1)
    params = [identity] + [[c, -s, 0, s, c, 0, 0, 0, 1.0, 0.3 * k, -0.2, 0.01, 0.05 * k] for k in range(1, len(sizes))]
    flags = [False] + [True] * (len(sizes) - 1)
    return lambda: ops.assemble_sweeps(raw, offsets, params, flags, flags, 1.0, PC_RANGE[:2] + [-5.0, 40.0, 40.0, 3.0], 3, 0.0, 255.0)


@cases("augment_points", ragged=dict(n=1009, augs=[(0.0, 1.0, True, False), (np.pi / 7, 1.05, False, True), (0.0, 0.95, False, False)]),
       minimal=dict(n=1, augs=[(0.0, 1.0, False, False)]), empty=dict(n=0, augs=[(0.0, 1.0, True, False)]))
def _augment_points(ops, dev, n, augs):
    from fullysparsefusion_amd.mmdet3d_plugin.datasets import pipelines as D
    from test_tta_gpu import _meta

    p = points5(dev, n, 2)
    pts = torch.cat([p, p[:, :3]], 1).contiguous()
    desc = [D.meta_descriptor(_meta(*a)) for a in augs]
    return lambda: ops.augment_points(pts, desc, [-40.0, -40.0, -5.0, 40.0, 40.0, 3.0])


@cases("aug_boxes_map_back", ragged=dict(m=1013, dim=9), minimal=dict(m=1, dim=7), empty=dict(m=0, dim=9))
def _aug_boxes_map_back(ops, dev, m, dim):
    from fullysparsefusion_amd.mmdet3d_plugin.datasets import pipelines as D
    from test_tta_gpu import _meta

    g = G(3)
    boxes = wide(randn(dev, g, m, dim, scale=5.0))
    scores, labels = torch.rand(m, generator=g).to(dev), randint(dev, g, -1, 11, (m,))
    pass_idx = randint(dev, g, 0, 3, (m,), torch.int32)
    desc = [D.meta_descriptor(_meta(*a), inverse=True) for a in [(0.0, 1.0, True, False), (np.pi / 7, 1.05, False, True), (0.0, 0.95, True, True)]]
    return lambda: ops.aug_boxes_map_back(boxes, scores, labels, pass_idx, desc, 10)


@cases("mask_extents", ragged=dict(n=5, h=37, w=48, pick=[4, 0, 3]), minimal=dict(n=1, h=1, w=16, pick=None), empty=dict(n=0, h=1, w=16, pick=None))
def _mask_extents(ops, dev, n, h, w, pick):
    g = G(4)
    masks = (torch.rand(n, h, w, generator=g) > 0.97).to(dev)
    masks[:1] = False
    idx = torch.tensor(pick, dtype=torch.int32, device=dev) if pick is not None else None
    return lambda: ops.mask_extents(masks, idx)


@cases("paint_instance_masks", ragged=dict(rows=3, dst=(20, 48), out_dtype=torch.int32), minimal=dict(rows=1, dst=(1, 16), out_dtype=torch.uint8),
       empty=dict(rows=0, dst=(1, 16), out_dtype=torch.uint8), golden=dict(rows=-1, dst=None, out_dtype=None))
def _paint_instance_masks(ops, dev, rows, dst, out_dtype):
    if rows < 0:  # the committed nuScenes detections through the planner of test_mask_paint_gpu.py (60 planes of 900 x 1600)
        from fullysparsefusion_amd.mmdet3d_plugin.datasets import mask_paint as mp
        from test_mask_paint_cpu import golden_dets

        plan = mp.plan_masks(golden_dets("nusc"))
        return lambda: mp.paint_device(plan, dev)
    sh, sw = 30, 48
    g = G(5)
    masks = (torch.rand(2, sh, sw, generator=g) > 0.4).to(torch.uint8).to(dev)
    if rows == 1:  # one solid rectangle on one plane
        table = torch.tensor([[0, 2, 3, 11, 17, 0, -1, 9]], dtype=torch.int32, device=dev)
        src_off = torch.zeros((1,), dtype=torch.int64, device=dev)
        plane_ptr = torch.tensor([0, 1], dtype=torch.int32, device=dev)
        extents = None
    elif rows:  # plane 0: a solid box under a masked object; plane 1 (resized on the fly): a masked object whose extent comes from K34a
        table = torch.tensor([[0, 2, 3, 11, 17, 0, -1, 300], [0, 5, 7, 13, 29, sw, -1, 2], [1, 0, 0, 0, 0, sw, 1, 7]], dtype=torch.int32, device=dev)
        src_off = torch.tensor([0, 0, sh * sw], dtype=torch.int64, device=dev)
        plane_ptr = torch.tensor([0, 2, 3], dtype=torch.int32, device=dev)
        extents = ops.mask_extents(masks)
    else:
        table = torch.zeros((0, 8), dtype=torch.int32, device=dev)
        src_off = torch.zeros((0,), dtype=torch.int64, device=dev)
        plane_ptr = torch.tensor([0, 0], dtype=torch.int32, device=dev)
        extents = None
    p = plane_ptr.numel() - 1
    hw = torch.tensor([[sh, sw]] * p, dtype=torch.int32, device=dev)
    scale = torch.tensor([[np.float32(sh / dst[0]), np.float32(sw / dst[1])]] * p, dtype=torch.float32, device=dev)
    return lambda: ops.paint_instance_masks(table, src_off, plane_ptr, hw, scale, dst, out_dtype, masks=masks if rows == 3 else None, extents=extents)


def _gt_csr(dev, pts, per_sample, dim, seed):
    boxes = torch.cat([gt_boxes(dev, pts, m, dim, seed + k) for k, m in enumerate(per_sample)])
    box_ptr = torch.tensor(np.concatenate([[0], np.cumsum(per_sample)]), dtype=torch.int32, device=dev)
    labels = randint(dev, G(seed), 0, 10, (boxes.size(0),), torch.int32)
    if labels.numel() > 2:
        labels[1] = -1
    return box_ptr, boxes, labels


@cases("seg_targets", ragged=dict(n=1009, per_sample=(3, 0, 4)), minimal=dict(n=1, per_sample=(0,)), empty=dict(n=0, per_sample=(2,)))
def _seg_targets(ops, dev, n, per_sample):
    pts = points5(dev, max(n, 1), 6)
    box_ptr, boxes, labels = _gt_csr(dev, pts, per_sample, 9, 6)
    p = wide(pts[:n, :4])
    bidx = randint(dev, G(6), 0, len(per_sample), (n,), torch.int32)
    return lambda: ops.seg_targets(p, bidx, box_ptr, wide(boxes) if boxes.size(0) else boxes, labels, 10)


def _seg_loss_inputs(dev, n, c):
    from test_seg_losses_gpu import loss_inputs

    _, logits, votes, labels, targets, mask = loss_inputs(dev, c, n=max(n, 1), seed=7)
    cw = torch.tensor([1.0] * (c - 1) + [0.1], device=dev)
    return logits.detach()[:n], votes.detach()[:n], labels[:n], targets[:n], mask[:n], cw


@cases("seg_loss_forward", ragged=dict(n=1009, c=11), minimal=dict(n=1, c=11), empty=dict(n=0, c=27))
def _seg_loss_forward(ops, dev, n, c):
    a = _seg_loss_inputs(dev, n, c)
    return lambda: ops.seg_loss_forward(*a, 10.0, 1.0)


@cases("seg_loss_backward", ragged=dict(n=1009, c=11), minimal=dict(n=1, c=27), empty=dict(n=0, c=11))
def _seg_loss_backward(ops, dev, n, c):
    a = _seg_loss_inputs(dev, n, c)
    counts = ops.seg_loss_forward(*a, 10.0, 1.0)[2]
    g1, g2 = torch.tensor(1.0, device=dev), torch.tensor(0.5, device=dev)
    return lambda: ops.seg_loss_backward(*a, 10.0, 1.0, counts, g1, g2)


@cases("cluster_targets", ragged=dict(n=1009, per_sample=(3, 0, 4), code=10), minimal=dict(n=1, per_sample=(0,), code=8),
       empty=dict(n=0, per_sample=(2,), code=8))
def _cluster_targets(ops, dev, n, per_sample, code):
    pts = points5(dev, max(n, 1), 8)
    box_ptr, boxes, labels = _gt_csr(dev, pts, per_sample, 9 if code == 10 else 7, 8)
    xyz = wide(pts[:n, :3])
    table = torch.zeros((n, 3), dtype=torch.int64, device=dev)
    table[:, 1] = randint(dev, G(8), 0, len(per_sample), (n,))
    return lambda: ops.cluster_targets(xyz, table[:, 1], box_ptr, boxes, labels, 10, code, 0.05)


def _cluster_loss_inputs(dev, n, c, code):
    from test_cluster_losses_cpu import loss_inputs

    z, r, labels, targets, weights = loss_inputs(c, code, n=n, seed=9)
    lw = torch.rand(n, generator=G(9)).to(dev)
    avg = torch.tensor([max(float((labels < c).sum()), 1.0)] * 2, device=dev)
    return wide(z.to(dev)), wide(r.to(dev)), labels.to(dev), lw, targets.to(dev), weights.to(dev), avg


@cases("cluster_loss_forward", ragged=dict(n=1009, c=10, code=10), minimal=dict(n=1, c=26, code=8), empty=dict(n=0, c=10, code=10))
def _cluster_loss_forward(ops, dev, n, c, code):
    a = _cluster_loss_inputs(dev, n, c, code)
    return lambda: ops.cluster_loss_forward(*a, 4.0, 0.25, [1.0, 0.5, 0.5, 0.2, 0.2], code == 10)


@cases("cluster_loss_backward", ragged=dict(n=1009, c=10, code=10), minimal=dict(n=1, c=26, code=8), empty=dict(n=0, c=10, code=10))
def _cluster_loss_backward(ops, dev, n, c, code):
    a = _cluster_loss_inputs(dev, n, c, code)
    lw5 = [1.0, 0.5, 0.5, 0.2, 0.2]
    counts = ops.cluster_loss_forward(*a, 4.0, 0.25, lw5, code == 10)[1]
    grads = [torch.tensor([v], device=dev) for v in (1.0, 0.7, 1.3, 0.9)] + [None]
    return lambda: ops.cluster_loss_backward(*a, 4.0, 0.25, lw5, code == 10, counts, grads)


@cases("voxelize_dynamic", ragged=dict(n=1009), minimal=dict(n=1), empty=dict(n=0))
def _voxelize_dynamic(ops, dev, n):
    from oracle import voxelize as ovox

    pts = torch.from_numpy(cloud(n, seed=10, oob_frac=0.3)).to(dev)
    vs, pr = (0.2, 0.2, 0.2), [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
    return lambda: ops.voxelize_dynamic(pts, vs, pr, ovox.grid_size(vs, pr), batch_idx=3, want_zyx=True, want_bzyx=True)


@cases("voxelize_divfloor", ragged=dict(n=1009), minimal=dict(n=1), empty=dict(n=0))
def _voxelize_divfloor(ops, dev, n):
    pts = points5(dev, n, 11)
    b = randint(dev, G(11), 0, 2, (n,))
    return lambda: (ops.voxelize_divfloor(pts, (0.1, 0.1, 0.1), (-51.2, -51.2, -5.0), "zyx", b),
                    ops.voxelize_divfloor(pts, (0.5, 0.5, 6.0), (-51.2, -51.2, -5.0), "xyz"))


@cases("vfe_decorate", ragged=dict(n=1009, p=5, m=37), minimal=dict(n=1, p=4, m=1), empty=dict(n=0, p=5, m=1))
def _vfe_decorate(ops, dev, n, p, m):
    g = G(12)
    feats = wide(randn(dev, g, n, p))
    mean = wide(randn(dev, g, m, 3))
    inv = randint(dev, g, 0, m, (n,))
    coors = randint(dev, g, 0, 40, (n, 4))
    vs, off = (0.2, 0.2, 0.2), (-51.1, -51.1, -4.9)
    return lambda: (ops.vfe_decorate(feats, mean, inv, coors, vs, off), ops.vfe_decorate(feats, mean, inv, coors, vs, off, True, False),
                    ops.vfe_decorate(feats, mean, inv, coors, vs, off, False, True))


@cases("vote_centers_keys", ragged=dict(p=509, n=1013), minimal=dict(p=4, n=1), empty=dict(p=4, n=0))
def _vote_centers_keys(ops, dev, p, n):
    g = G(13)
    logits, offsets, pts = wide(randn(dev, g, p, 11)), wide(randn(dev, g, p, 33)), points5(dev, p, 13)
    batch = randint(dev, g, 0, 2, (p,))
    g_ids, p_ids = randint(dev, g, 0, 2, (n,)), randint(dev, g, 0, p, (n,))
    return lambda: ops.vote_centers_keys(logits, offsets, pts, batch, g_ids, p_ids, 10, [1, 6], [[0.4, 0.4, 0.8]] * 2, [-54, -54, -5], 2)


def _plan_outputs(plan):
    return plan.inv, plan.order, plan.seg_offsets, plan.cnt


@cases("unique_rows", ragged=dict(n=1009, k=4), minimal=dict(n=1, k=3), empty=dict(n=0, k=4), bounded=dict(n=4099, k=4, bounds=True))
def _unique_rows(ops, dev, n, k, bounds=False):
    keys = voxel_keys(dev, n, 14)[:, :k].contiguous()
    if n > 2:
        keys[1] = keys[0]
    lo, hi = ([0] * k, [5] * k) if bounds else (None, None)

    def run():
        new, plan = ops.unique_rows(keys, lo, hi)
        return new, _plan_outputs(plan)
    return run


@cases("segment_plan_from_inverse", ragged=dict(n=1009, m=131), minimal=dict(n=1, m=1), empty=dict(n=0, m=3))
def _segment_plan_from_inverse(ops, dev, n, m):
    inv = randint(dev, G(15), 0, max(m - 2, 1), (n,))  # (the last segments stay empty)
    return lambda: _plan_outputs(ops.segment_plan_from_inverse(inv, m, return_counts=True))


def _plan(ops, dev, n, m, seed):
    inv = randint(dev, G(seed), 0, m, (n,))
    inv[:min(n, m)] = torch.arange(min(n, m), device=dev)
    return ops.segment_plan_from_inverse(inv, m, return_counts=True)


@cases("segment_reduce", ragged=dict(n=1009, m=37, c=131), minimal=dict(n=1, m=1, c=1), long=dict(n=40009, m=3, c=180), empty=dict(n=0, m=3, c=5))
def _segment_reduce(ops, dev, n, m, c):
    plan = _plan(ops, dev, n, m, 16)
    feat = wide(randn(dev, G(16), n, c))
    return lambda: (ops.segment_reduce(feat, plan, "sum"), ops.segment_reduce(feat, plan, "mean"), ops.segment_reduce(feat, plan, "max", True))


@cases("segment_reduce_short", ragged=dict(n=1009, m=401, cs=(3, 131, 5)), minimal=dict(n=1, m=1, cs=(1,)), empty=dict(n=0, m=3, cs=(5, 8)))
def _segment_reduce_short(ops, dev, n, m, cs):
    plan = _plan(ops, dev, n, m, 17) if n else ops.segment_plan_from_inverse(torch.zeros((0,), dtype=torch.int64, device=dev), m)
    g = G(17)
    feats = [wide(randn(dev, g, n, c)) for c in cs]
    if n == 0:
        return lambda: (ops.segment_reduce_short(feats, plan, "mean"), ops.segment_reduce_short(feats, plan, "sum"))
    return lambda: (ops.segment_reduce_short(feats, plan, "mean"), ops.segment_reduce_short(feats, plan, "sum"),
                    ops.segment_reduce_short(feats[:1], plan, "max", True))


@cases("segment_reduce_backward", ragged=dict(n=1009, m=37, c=131), minimal=dict(n=1, m=1, c=1), empty=dict(n=0, m=3, c=5))
def _segment_reduce_backward(ops, dev, n, m, c):
    plan = _plan(ops, dev, n, m, 18)
    g = G(18)
    argmax = ops.segment_reduce(randn(dev, g, n, c), plan, "max", True)[1]
    go = randn(dev, g, m, c)
    return lambda: (ops.segment_reduce_backward(go, plan, "sum"), ops.segment_reduce_backward(go, plan, "mean"),
                    ops.segment_reduce_backward(go, plan, "max", argmax))


@cases("gather_rows", ragged=dict(m=509, n=1013, c=131), minimal=dict(m=1, n=1, c=1), empty=dict(m=10, n=0, c=7))
def _gather_rows(ops, dev, m, n, c):
    g = G(19)
    src, idx = wide(randn(dev, g, m, c)), randint(dev, g, 0, m, (n,))

    def run():
        dst = torch.zeros((n, c + 5), device=dev)
        ops.gather_rows(src, idx, out=dst[:, 2:2 + c])
        return ops.gather_rows(src, idx), dst
    return run


@cases("gather_rows_add", ragged=dict(m=509, n=1013, c=131), minimal=dict(m=1, n=1, c=1), empty=dict(m=5, n=0, c=7))
def _gather_rows_add(ops, dev, m, n, c):
    g = G(20)
    src, idx, add = randn(dev, g, m, c), randint(dev, g, 0, m, (n,)), randn(dev, g, n, c)
    return lambda: ops.gather_rows_add(src, idx, add)


@cases("channel_group_sum_add", ragged=dict(n=1009, cin=264, cout=132), minimal=dict(n=1, cin=8, cout=4), empty=dict(n=0, cin=8, cout=4))
def _channel_group_sum_add(ops, dev, n, cin, cout):
    g = G(21)
    feat, add = randn(dev, g, n, cin), randn(dev, g, n, cout)
    return lambda: (ops.channel_group_sum_add(feat, cout, add), ops.channel_group_sum_add(feat, cout))


@cases("channel_pair_sum_add2", ragged=dict(n=1009, ca=136, cb=24), minimal=dict(n=1, ca=16, cb=8), empty=dict(n=0, ca=16, cb=8))
def _channel_pair_sum_add2(ops, dev, n, ca, cb):
    g = G(22)
    a, b, add = randn(dev, g, n, ca), randn(dev, g, n, cb), randn(dev, g, n, (ca + cb) // 2)
    assert ops.channel_pair_sum_add2_supported(a, b)
    return lambda: (ops.channel_pair_sum_add2(a, b, add), ops.channel_pair_sum_add2(a, b))


def _planes_outputs(p):
    return None if p is None else (p.data, p.scales)


@cases("channel_pair_sum_add2_planes", ragged=dict(n=1009, ca=32, cb=96), minimal=dict(n=1, ca=16, cb=16), empty=dict(n=0, ca=128, cb=128))
def _channel_pair_sum_add2_planes(ops, dev, n, ca, cb):
    g = G(23)
    a, b, add = randn(dev, g, n, ca), randn(dev, g, n, cb), randn(dev, g, n, (ca + cb) // 2)
    return lambda: (_planes_outputs(ops.channel_pair_sum_add2_planes(a, b, add)), _planes_outputs(ops.channel_pair_sum_add2_planes(a, b)))


@cases("voxel2point", ragged=dict(n=1009, m=131, c=67), minimal=dict(n=1, m=1, c=1), empty=dict(n=0, m=1, c=3))
def _voxel2point(ops, dev, n, m, c):
    g = G(24)
    pts, coors = points5(dev, n, 24), randint(dev, g, 0, 40, (n, 4))
    vf, inv = randn(dev, g, m, c), randint(dev, g, 0, m, (n,))
    return lambda: ops.voxel2point(pts, coors, vf, inv, (0.2, 0.2, 0.2), (-51.2, -51.2, -5.0))


@cases("project_gather_mask", ragged=dict(n=1009, ncam=3, ncls=3, H=37, W=53), minimal=dict(n=1, ncam=1, ncls=1, H=2, W=2), empty=dict(n=0, ncam=2, ncls=2, H=4, W=4))
def _project_gather_mask(ops, dev, n, ncam, ncls, H, W):
    pts, L, mask, _ = camera_inputs(dev, n, ncam, ncls, H, W, 25)
    return lambda: ops.project_gather_mask(pts, L, mask, return_pts_2d=True)


@cases("project_score", ragged=dict(n=1009, ncam=3, ncls=3, H=37, W=53, dtype=np.int32), minimal=dict(n=1, ncam=1, ncls=1, H=2, W=2, dtype=np.uint8),
       empty=dict(n=0, ncam=2, ncls=2, H=4, W=4, dtype=np.uint8))
def _project_score(ops, dev, n, ncam, ncls, H, W, dtype):
    pts, L, mask, anno = camera_inputs(dev, n, ncam, ncls, H, W, 26, dtype)
    return lambda: ops.project_score(pts, L, mask, anno, return_ids=True, return_fg=True, return_overlap=True)


@cases("concat_mul", ragged=dict(n=1009, cf=131, ce=13), minimal=dict(n=1, cf=1, ce=0), empty=dict(n=0, cf=3, ce=0))
def _concat_mul(ops, dev, n, cf, ce):
    g = G(27)
    pts, feats = wide(points5(dev, n, 27)), wide(randn(dev, g, n, cf))
    extra = wide(randn(dev, g, n, ce)) if ce else None
    h = randn(dev, g, n, 5 + cf + ce)
    return lambda: ops.concat_mul(pts, feats, extra, h, [20.0, 20.0, 4.0], 10.0)


@cases("concat_mul_backward", ragged=dict(n=1009, cf=131, ce=13), minimal=dict(n=1, cf=1, ce=0), empty=dict(n=0, cf=3, ce=2))
def _concat_mul_backward(ops, dev, n, cf, ce):
    g = G(28)
    pts, feats = wide(points5(dev, n, 28)), wide(randn(dev, g, n, cf))
    extra = wide(randn(dev, g, n, ce)) if ce else None
    h, go = randn(dev, g, n, 5 + cf + ce), randn(dev, g, n, 5 + cf + ce)
    return lambda: ops.concat_mul_backward(pts, feats, extra, h, go, [20.0, 20.0, 4.0], 10.0, True, True)


@cases("group_pairs", ragged=dict(n=1009, ng=7), minimal=dict(n=1, ng=1), empty=dict(n=0, ng=3))
def _group_pairs(ops, dev, n, ng):
    g = G(29)
    score = wide(torch.rand(n, ng, generator=g).to(dev))
    thresh = torch.full((ng,), 0.7, device=dev)
    if n == 0:
        return lambda: ops.group_pairs(score, thresh, keep_one=False)
    thresh[-1] = 2.0  # a group nobody passes: point 0 is kept
    cls = wide(torch.rand(n, ng + 1, generator=g).to(dev))
    cols = [[k, k + 1] if k % 2 else [k] for k in range(ng)]
    return lambda: (ops.group_pairs(score, thresh), ops.group_pairs(score, thresh, keep_one=False), ops.group_pairs(cls, thresh, True, cols))


def _overlap_inputs(ops, dev, n, minimal):
    pts, L, mask, anno = camera_inputs(dev, n, *((1, 1, 2, 2) if minimal else (3, 5, 37, 53)), 30)
    if not minimal:
        mask[:, 1] = mask[:, 0]  # every masked pixel lies in two class planes: points inside >= 2 masks exist
    _, (fg, count, max_id) = ops.project_score(pts, L, mask, anno, return_fg=False, return_overlap=True)
    return pts, L, mask, fg, count, max_id


@cases("overlap_plan", ragged=dict(n=1009, minimal=False), minimal=dict(n=1, minimal=True), empty=dict(n=0, minimal=True))
def _overlap_plan(ops, dev, n, minimal):
    import ctypes

    from fullysparsefusion_amd._lib import c_p, check, ptr, stream_ptr

    pts, L, mask, fg, count, max_id = _overlap_inputs(ops, dev, n, minimal)
    cells = mask.size(0) * mask.size(1)

    def run():
        f, m, t, ws = ops.overlap_plan(fg, count, cells)
        rows = ops.overlap_rows(pts, L, mask, max_id, None, ws, f, m, t)
        # the wrapper's own max(..., 256) floor would hide an overrun of a smaller figure: the entry point on exactly what it asks for
        h = ops._L()
        exact = int(h.fsf_overlap_plan_workspace_bytes(n))
        ws2 = torch.empty((max(exact, 1),), dtype=torch.uint8, device=dev)
        counts = (ctypes.c_int64 * 3)()
        check(h.fsf_overlap_plan(ptr(fg), ptr(count), n, cells, ctypes.cast(counts, c_p), ptr(ws2), exact, stream_ptr()), "fsf_overlap_plan")
        assert (int(counts[0]), int(counts[1]), int(counts[2])) == (f, m, t)
        rows2 = ops.overlap_rows(pts, L, mask, max_id, None, ws2, f, m, t)
        return torch.tensor([f, m, t]), rows, rows2
    return run


@cases("overlap_rows", ragged=dict(n=1009, minimal=False), minimal=dict(n=1, minimal=True), empty=dict(n=0, minimal=True))
def _overlap_rows(ops, dev, n, minimal):
    pts, L, mask, fg, count, max_id = _overlap_inputs(ops, dev, n, minimal)
    f, m, t, ws = ops.overlap_plan(fg, count, mask.size(0) * mask.size(1))
    assert minimal or (f > 0 and m > 0 and t > 0)
    batch = torch.full((n,), 3, dtype=torch.int64, device=dev)
    return lambda: (ops.overlap_rows(pts, L, mask, max_id, None, ws, f, m, t), ops.overlap_rows(pts, L, mask, max_id, batch, ws, f, m, t))


@cases("project_gather_bilinear", ragged=dict(n=1009, ncam=3, c=131, hf=29, wf=53), minimal=dict(n=1, ncam=1, c=1, hf=1, wf=1), empty=dict(n=0, ncam=2, c=3, hf=2, wf=2))
def _project_gather_bilinear(ops, dev, n, ncam, c, hf, wf):
    pts, L, _, _ = camera_inputs(dev, n, ncam, 1, 450, 800, 31)
    g = G(31)
    feat, feat_cl = randn(dev, g, ncam, c, hf, wf), randn(dev, g, ncam, hf, wf, c)
    return lambda: (ops.project_gather_bilinear(pts, L, feat, (450, 800)),
                    ops.project_gather_bilinear(pts, L, feat_cl, (450, 800), channels_last=True, reduce_cams=True, return_count=True))


@cases("cam_select_score", ragged=dict(n=1009, ncam=3, ncls=7), minimal=dict(n=1, ncam=1, ncls=1), empty=dict(n=0, ncam=2, ncls=3))
def _cam_select_score(ops, dev, n, ncam, ncls):
    g = G(32)
    obj = randint(dev, g, 0, 20, (n, ncam, ncls)) * (torch.rand(n, ncam, ncls, generator=g) > 0.6).to(dev)
    anno = torch.rand(20, 9, generator=g).to(dev)
    return lambda: ops.cam_select_score(obj, anno, return_ids=True)


@cases("rulebook_subm", ragged=dict(m=401, shape=(8, 12, 10)), minimal=dict(m=1, shape=(3, 3, 3)), empty=dict(m=0, shape=(3, 3, 3)))
def _rulebook_subm(ops, dev, m, shape):
    idx = sites(dev, m, shape, 33)
    return lambda: ops.rulebook_subm(idx, 2, shape)


@cases("rulebook_strided", ragged=dict(m=401, shape=(8, 12, 10)), minimal=dict(m=1, shape=(3, 3, 3)), empty=dict(m=0, shape=(3, 3, 3)))
def _rulebook_strided(ops, dev, m, shape):
    idx = sites(dev, m, shape, 34)
    return lambda: (ops.rulebook_strided(idx, 2, shape, (3, 3, 3), (2, 2, 2), (1, 1, 1))[:3],
                    ops.rulebook_strided(idx, 2, shape, (3, 3, 3), (2, 2, 2), (0, 1, 1), want_inverse=False)[:3])


@cases("order_by_neighbor_mask", ragged=dict(m=401, shape=(8, 12, 10)), minimal=dict(m=1, shape=(3, 3, 3)), empty=dict(m=0, shape=(3, 3, 3)))
def _order_by_neighbor_mask(ops, dev, m, shape):
    idx = sites(dev, m, shape, 35)
    return lambda: ops.order_by_neighbor_mask(idx, 2, shape)


@cases("remap_indices", ragged=dict(shape=(401, 27), m=131), minimal=dict(shape=(1,), m=1), empty=dict(shape=(0,), m=1))
def _remap_indices(ops, dev, shape, m):
    g = G(36)
    table = randint(dev, g, -1, m, shape, torch.int32)
    index_map = torch.randperm(m, generator=g).to(torch.int32).to(dev)
    return lambda: ops.remap_indices(table, index_map)


@cases("rulebook_to_pairs", ragged=dict(m=401, shape=(8, 12, 10)), minimal=dict(m=1, shape=(3, 3, 3)), empty=dict(m=0, shape=(3, 3, 3)))
def _rulebook_to_pairs(ops, dev, m, shape):
    nbr = ops.rulebook_subm(sites(dev, m, shape, 37), 2, shape)
    return lambda: ops.rulebook_to_pairs(nbr)


def _conv_inputs(ops, dev, m, shape, cin, cout, seed, epilogue=True):
    g = G(seed)
    m_out, m = m, max(m, 5)  # (m = 0: no output rows over five input rows; an input of no rows has no row 0 for a missing neighbour)
    nbr = ops.rulebook_subm(sites(dev, m, shape, seed), 2, shape)[:m_out].contiguous()
    feat = randn(dev, g, m, cin) * torch.exp(randn(dev, g, m, 1))
    w = randn(dev, g, 27, cin, cout, scale=(cin * 6) ** -0.5)
    ep = dict(scale=torch.rand(cout, generator=g).to(dev) + 0.5, shift=randn(dev, g, cout), residual=randn(dev, g, m_out, cout), relu=True)
    return nbr, feat, w, ep


@cases("spconv_transpose_weight", ragged=dict(kvol=27, cin=20, cout=37), minimal=dict(kvol=1, cin=1, cout=1))
def _spconv_transpose_weight(ops, dev, kvol, cin, cout):
    w = randn(dev, G(38), kvol, cin, cout)
    return lambda: ops.spconv_transpose_weight(w)


@cases("spconv_forward", ragged=dict(m=401, shape=(8, 12, 10), cin=32, cout=20), minimal=dict(m=1, shape=(3, 3, 3), cin=16, cout=16),
       empty=dict(m=0, shape=(3, 3, 3), cin=16, cout=16))
def _spconv_forward(ops, dev, m, shape, cin, cout):
    nbr, feat, w, ep = _conv_inputs(ops, dev, m, shape, cin, cout, 39)
    wt = ops.spconv_transpose_weight(w)
    return lambda: (ops.spconv_forward(feat, wt, nbr), ops.spconv_forward(feat, wt, nbr, **ep))


@cases("spconv_prepare_weight_split", ragged=dict(cin=48, cout=36), minimal=dict(cin=16, cout=16))
def _spconv_prepare_weight_split(ops, dev, cin, cout):
    w = randn(dev, G(40), 27, cin, cout)
    return lambda: ops.spconv_prepare_weight_split(w)


@cases("spconv_forward_split", ragged=dict(m=401, shape=(8, 12, 10), cin=44, cout=36), minimal=dict(m=1, shape=(3, 3, 3), cin=16, cout=16),
       deep=dict(m=1517, shape=(16, 24, 24), cin=512, cout=512), empty=dict(m=0, shape=(3, 3, 3), cin=16, cout=16))
def _spconv_forward_split(ops, dev, m, shape, cin, cout):
    nbr, feat, w, ep = _conv_inputs(ops, dev, m, shape, cin, cout, 41)
    planes = ops.spconv_prepare_weight_split(w)
    return lambda: (ops.spconv_forward_split(feat, planes, 27, cout, nbr), ops.spconv_forward_split(feat, planes, 27, cout, nbr, **ep))


@cases("spconv_prepare_weight_split_f16", ragged=dict(cin=64, cout=132), minimal=dict(cin=32, cout=68, kvol=1))
def _spconv_prepare_weight_split_f16(ops, dev, cin, cout, kvol=27):
    w = randn(dev, G(42), kvol, cin, cout)
    return lambda: ops.spconv_prepare_weight_split_f16(w)


@cases("spconv_forward_split_planes", ragged=dict(m=401, shape=(8, 12, 10), cin=32, cout=68), minimal=dict(m=1, shape=(3, 3, 3), cin=32, cout=68),
       deep=dict(m=1517, shape=(16, 24, 24), cin=512, cout=512), empty=dict(m=0, shape=(3, 3, 3), cin=32, cout=68))
def _spconv_forward_split_planes(ops, dev, m, shape, cin, cout):
    assert ops.spconv_split_planes_supported(cin, cout)
    nbr, feat, w, ep = _conv_inputs(ops, dev, m, shape, cin, cout, 43)
    wp, xp = ops.spconv_prepare_weight_split_f16(w), ops.rows_to_planes(feat)
    return lambda: (ops.spconv_forward_split_planes(xp, wp, 27, cout, nbr), ops.spconv_forward_split_planes(xp, wp, 27, cout, nbr, **ep))


@cases("planes_empty", ragged=dict(m=257, c=72), minimal=dict(m=1, c=8), empty=dict(m=0, c=32))
@cases("to_planes", ragged=dict(m=257, c=72), minimal=dict(m=1, c=8), empty=dict(m=0, c=32))
def _to_planes(ops, dev, m, c):
    """(`planes_empty` only allocates: it is checked through the kernels that fill what it returns.)"""
    g = G(44)
    x = wide4(randn(dev, g, m, c) * torch.exp(randn(dev, g, m, 1) * 3.0))
    src = randn(dev, g, 509, c)
    rows = randint(dev, g, 0, 509, (m,))
    return lambda: (_planes_outputs(ops.to_planes(x)), _planes_outputs(ops.to_planes(src, rows)))


@cases("spconv_prepare_weight_planes", ragged=dict(cin=96, cout=64), minimal=dict(cin=32, cout=64, kvol=1))
def _spconv_prepare_weight_planes(ops, dev, cin, cout, kvol=27):
    w = randn(dev, G(45), kvol, cin, cout)
    return lambda: ops.spconv_prepare_weight_planes(w)


@cases("spconv_forward_planes", ragged=dict(m=401, shape=(8, 12, 10), cins=(64, 32), cout=128), minimal=dict(m=1, shape=(3, 3, 3), cins=(32,), cout=64),
       empty=dict(m=0, shape=(3, 3, 3), cins=(32,), cout=64))
def _spconv_forward_planes(ops, dev, m, shape, cins, cout):
    assert ops.spconv_planes_supported(cins, cout, 27)
    nbr, feat, w, ep = _conv_inputs(ops, dev, m, shape, sum(cins), cout, 46)
    wp = ops.spconv_prepare_weight_planes(w)
    src = [ops.to_planes(f.contiguous()) for f in torch.split(feat, list(cins), 1)]

    def run():
        a, _ = ops.spconv_forward_planes(src, wp, 27, cout, nbr)
        b, bp = ops.spconv_forward_planes(src, wp, 27, cout, nbr, want_out=True, want_planes=True, **ep)
        _, cp = ops.spconv_forward_planes(src, wp, 27, cout, nbr, want_out=False, want_planes=True)
        return a, b, _planes_outputs(bp), _planes_outputs(cp)
    return run


@cases("linear_backward_weight", ragged=dict(n=1009, cin=180, cout=132), minimal=dict(n=1, cin=4, cout=4), wide=dict(n=20011, cin=180, cout=128),
       empty=dict(n=0, cin=4, cout=8))
def _linear_backward_weight(ops, dev, n, cin, cout):
    g = G(47)
    x, go = randn(dev, g, n, cin), randn(dev, g, n, cout)
    return lambda: ops.linear_backward_weight(x, go)


@cases("spconv_backward_weight", ragged=dict(m=401, shape=(8, 12, 10), cin=48, cout=36), minimal=dict(m=1, shape=(3, 3, 3), cin=4, cout=4),
       wide=dict(m=1517, shape=(16, 24, 24), cin=128, cout=256))
def _spconv_backward_weight(ops, dev, m, shape, cin, cout):
    nbr, feat, _, ep = _conv_inputs(ops, dev, m, shape, cin, cout, 48)
    pairs, num = ops.rulebook_to_pairs(nbr)
    return lambda: ops.spconv_backward_weight(feat, ep["residual"], pairs, num)


@cases("ingroup_rank", ragged=dict(n=1009, groups=37), minimal=dict(n=1, groups=1), empty=dict(n=0, groups=1))
def _ingroup_rank(ops, dev, n, groups):
    gi = randint(dev, G(49), 0, groups, (n,))
    return lambda: ops.ingroup_rank(gi)


@cases("row_topk_desc", ragged=dict(n=1009, w=61, k=5), minimal=dict(n=1, w=1, k=1), empty=dict(n=0, w=7, k=3))
def _row_topk_desc(ops, dev, n, w, k):
    x = randint(dev, G(50), -50, 50, (n, w))
    return lambda: ops.row_topk_desc(x, k)


def _sir_input_args(dev, n, seed, cfs=(11, 33, 131), ce=0, r=3):
    g = G(seed)
    p = max(n // 2, 1)
    parts = [wide(randn(dev, g, p, c)) for c in cfs[:-1]] + [wide(randn(dev, g, p, cfs[-1]), 0, 1)]
    idx = randint(dev, g, 0, p, (n,))
    points, fcl = wide(randn(dev, g, n, 5)), wide(randn(dev, g, n, r))
    extra = wide(randn(dev, g, n, ce)) if ce else None
    layers = mlp3(dev, g, r, 5 + sum(cfs) + ce)
    return points, parts, fcl, idx, extra, layers


@cases("sir_input", ragged=dict(n=1009), minimal=dict(n=1), extra=dict(n=509, cfs=(163,), ce=13, r=13), empty=dict(n=0))
def _sir_input(ops, dev, n, cfs=(11, 33, 131), ce=0, r=3):
    points, parts, fcl, idx, extra, layers = _sir_input_args(dev, n, 51, cfs, ce, r)
    return lambda: ops.sir_input(points, parts, fcl, [20.0, 20.0, 4.0], (*layers, 1e-3), "gelu", 10.0, extra=extra, extra_div=10.0, feats_index=idx)


@cases("linear_prepare_weight", ragged=dict(c=132, k=133), minimal=dict(c=4, k=1))
def _linear_prepare_weight(ops, dev, c, k):
    w = randn(dev, G(52), c, k)
    return lambda: (ops.linear_prepare_weight(w, "bf16x6"), ops.linear_prepare_weight(w))


@cases("linear_prepare_weight_f16", ragged=dict(c=180, k=160, slice_c=100), minimal=dict(c=68, k=32, slice_c=68))
def _linear_prepare_weight_f16(ops, dev, c, k, slice_c):
    w = randn(dev, G(53), c, k)
    return lambda: ops.linear_prepare_weight_f16(w, slice_c)


def _linear_tail(dev, g, c):
    return dict(bias=randn(dev, g, c), gamma=torch.rand(c, generator=g).to(dev) + 0.5, beta=randn(dev, g, c), eps=1e-3)


@cases("linear_norm_act", ragged=dict(n=1009, k=133, c=124, norm="ln"), minimal=dict(n=1, k=1, c=4, norm="none"), empty=dict(n=0, k=128, c=128, norm="ln"),
       wide=dict(n=1013, k=180, c=260, norm="affine"))
def _linear_norm_act(ops, dev, n, k, c, norm):
    g = G(54)
    x = wide4(randn(dev, g, n, k))
    assert ops.linear_norm_act_supported(x, c)
    w = randn(dev, g, c, k, scale=k ** -0.5)
    tail = _linear_tail(dev, g, c)
    groups = max(n // 7, 1)
    row_add, row_idx = randn(dev, g, groups, c), randint(dev, g, 0, groups, (n,))

    def run():
        outs = []
        for fmt in ("bf16x6", "f16x3") if c > 32 else ("bf16x6",):
            pl = ops.linear_prepare_weight(w, fmt)
            outs.append(ops.linear_norm_act(x, pl, c, norm=norm, act="gelu", **tail))
            outs.append(ops.linear_norm_act(x, pl, c, norm=norm, act="relu", row_add=row_add, row_add_index=row_idx, **tail))
            dst = torch.zeros((n, c + 8), device=dev)
            ops.linear_norm_act(x, pl, c, out=dst[:, 4:4 + c])
            outs.append(dst)
        return outs
    return run


@cases("linear_norm_act_segmax", ragged=dict(n=1009, m=37, k=133, c=124), minimal=dict(n=1, m=1, k=4, c=36), long=dict(n=40009, m=3, k=180, c=128),
       empty=dict(n=0, m=3, k=8, c=36))
def _linear_norm_act_segmax(ops, dev, n, m, k, c):
    g = G(55)
    x = wide4(randn(dev, g, n, k))
    w = randn(dev, g, c, k, scale=k ** -0.5)
    tail = _linear_tail(dev, g, c)
    seg = torch.sort(randint(dev, g, 0, m, (n,)))[0]
    seg[:min(n, m)] = torch.arange(min(n, m), device=dev)
    seg = torch.sort(seg)[0].contiguous()
    row_add = randn(dev, g, m, c)

    def run():
        outs = []
        for fmt in ("bf16x6", "f16x3") if c > 32 else ("bf16x6",):
            pl = ops.linear_prepare_weight(w, fmt)
            table = torch.full((m, 2 * c + 4), float("-inf"), device=dev)
            outs.append(ops.linear_norm_act_segmax(x, pl, c, seg, table[:, :c], **tail))
            outs.append(ops.linear_norm_act_segmax(x, pl, c, seg, table[:, c + 4:], row_add=row_add, row_add_index=seg, want_rows=False, **tail))
            outs.append(table)
        return outs
    return run


@cases("linear_prepare_weight_sliced", ragged=dict(k=133, ns=3, sc=20), minimal=dict(k=1, ns=1, sc=1))
def _linear_prepare_weight_sliced(ops, dev, k, ns, sc):
    w = randn(dev, G(56), ns * sc, k)
    return lambda: ops.linear_prepare_weight_sliced(w, ns, sc)


@cases("linear_norm_act_sliced", ragged=dict(n=1009, k=96, ns=3, sc=20, off=96), minimal=dict(n=1, k=4, ns=1, sc=4, off=0),
       empty=dict(n=0, k=128, ns=2, sc=128, off=0), shared=dict(n=777, k=132, ns=5, sc=16, off=0))
def _linear_norm_act_sliced(ops, dev, n, k, ns, sc, off):
    g = G(57)
    x = wide4(randn(dev, g, n, k + (ns - 1) * off))
    pl = ops.linear_prepare_weight_sliced(randn(dev, g, ns * sc, k, scale=k ** -0.5), ns, sc)
    tail = _linear_tail(dev, g, ns * sc)
    return lambda: (ops.linear_norm_act_sliced(x, k, off, pl, ns, sc, norm="ln", act="gelu", **tail), ops.linear_norm_act_sliced(x, k, off, pl, ns, sc))


def _row_planes_outputs(rp):
    return rp.data[:rp.n * rp.c * 4], rp.inv_scales[:rp.n]  # (the documented extents: both buffers have a floor for n = 0)


@cases("rows_to_planes", ragged=dict(n=1009, c=136, norm="ln"), minimal=dict(n=1, c=8, norm="none"), empty=dict(n=0, c=128, norm="none"))
def _rows_to_planes(ops, dev, n, c, norm):
    g = G(58)
    x = wide4(randn(dev, g, n, c))
    gamma, beta = torch.rand(c, generator=g).to(dev) + 0.5, randn(dev, g, c)

    def run():
        a = ops.rows_to_planes(x)
        b, rows = ops.rows_to_planes(x, norm, gamma, beta, 1e-3, "gelu", want_rows=True)
        return _row_planes_outputs(a), _row_planes_outputs(b), rows
    return run


@cases("linear_planes_norm_act", ragged=dict(n=1009, k=160, c=180, slice_c=100, norm="none"), minimal=dict(n=1, k=32, c=68, slice_c=68, norm="ln"),
       empty=dict(n=0, k=32, c=68, slice_c=68, norm="none"))
def _linear_planes_norm_act(ops, dev, n, k, c, slice_c, norm):
    assert ops.linear_planes_supported(k, c, slice_c)
    g = G(59)
    xp = ops.rows_to_planes(randn(dev, g, n, k))
    wp = ops.linear_prepare_weight_f16(randn(dev, g, c, k, scale=k ** -0.5), slice_c)
    tail = _linear_tail(dev, g, c)

    def run():
        dst = torch.zeros((n, c + 8), device=dev)
        ops.linear_planes_norm_act(xp, wp, c, slice_c, out=dst[:, 4:4 + c])
        return ops.linear_planes_norm_act(xp, wp, c, slice_c, norm=norm, act="gelu", **tail), dst
    return run


@cases("dynamic_point_pool", ragged=dict(r=37, p=2003, max_inbox=16, max_all=701), no_points=dict(r=3, p=0, max_inbox=16, max_all=100), minimal=dict(r=1, p=1, max_inbox=512, max_all=1),
       chunks=dict(r=1103, p=8009, max_inbox=4, max_all=907), batched=dict(r=37, p=2003, max_inbox=512, max_all=50000, batched=True),
       empty=dict(r=0, p=5, max_inbox=512, max_all=100))
def _dynamic_point_pool(ops, dev, r, p, max_inbox, max_all, batched=False):
    rng = np.random.default_rng(60)
    rois = random_rois(rng, r)
    near = (rois[rng.integers(0, r, p), :3] if r else 0.0) + rng.normal(0, 1.5, (p, 3)) + np.array([0, 0, 1.0])
    pts = wide(torch.from_numpy(near.astype(np.float32)).to(dev))
    rois_t = torch.from_numpy(rois).to(dev)
    if batched:
        rb = randint(dev, G(60), 0, 2, (r, 1)).float()
        rois_t, pb = torch.cat([rb, rois_t], 1).contiguous(), randint(dev, G(61), 0, 2, (p,))
        return lambda: ops.dynamic_point_pool(rois_t, pts, [0.5, 0.5, 0.5], max_inbox, max_all, roi_batch_col=0, box_col=1, pts_batch=pb)
    return lambda: ops.dynamic_point_pool(rois_t, pts, [0.5, 0.5, 0.5], max_inbox, max_all)


@cases("nms_bev", ragged=dict(n=1009), minimal=dict(n=1), empty=dict(n=0), binned=dict(n=4001))
def _nms_bev(ops, dev, n):
    boxes = nms_boxes(dev, n, 62)
    return lambda: (ops.nms_bev(boxes, 0.25, True), ops.nms_bev(boxes, 0.25, False))


def _ranked(ops, dev, n, c, seed, thr=0.3):
    scores = torch.rand(c, n, generator=G(seed)).to(dev)
    if c > 2:
        scores[1] = 0.0  # a class with nothing above the threshold
    return scores, ops.class_rank_desc(scores, thr)


def _kept_only(keep, num):
    """keep i64 [C, n] up to each class's num_keep (the rest of a row is capacity, not output)."""
    k = keep.clone()
    k[torch.arange(k.size(1), device=k.device)[None, :] >= num[:, None]] = -7
    return k


@cases("nms_bev_multiclass", ragged=dict(n=1009, c=5), minimal=dict(n=1, c=1), windowed=dict(n=6007, c=3), empty=dict(n=0, c=3))
def _nms_bev_multiclass(ops, dev, n, c):
    boxes = nms_boxes(dev, n, 63)
    _, (order, rank, count) = _ranked(ops, dev, n, c, 63)

    def run():
        outs = []
        for kw in (dict(), dict(max_keep=37), dict(max_keep=100, windowed=True)):
            res = ops.nms_bev_multiclass(boxes, rank, count, 0.25, True, **kw)
            outs.append((_kept_only(res[0], res[1]),) + tuple(res[1:]))
        return outs
    return run


@cases("decode_cluster_boxes", ragged=dict(n=1009, c=3, code=10), minimal=dict(n=1, c=1, code=8), empty=dict(n=0, c=3, code=10))
def _decode_cluster_boxes(ops, dev, n, c, code):
    g = G(64)
    cls, reg, xyz = wide(randn(dev, g, n, c)), wide(randn(dev, g, n, code, scale=0.5)), wide(randn(dev, g, n, 3, scale=20.0))
    return lambda: ops.decode_cluster_boxes(cls, reg, xyz, 1e-6)


@cases("class_rank_desc", ragged=dict(n=4099, c=7), minimal=dict(n=1, c=1), odd=dict(n=1009, c=3), empty=dict(n=0, c=3))
def _class_rank_desc(ops, dev, n, c):
    scores = torch.rand(c, n, generator=G(65)).to(dev)
    scores[:, ::7] = scores[:, :1].clone()  # ties
    if n > 3:
        scores[0] = 0.0
    return lambda: ops.class_rank_desc(scores, 0.3)


def _key_survival_inputs(ops, dev, n, ng, seed):
    g = G(seed)
    grp = randint(dev, g, 0, ng, (n,))
    vox = randint(dev, g, 0, max(n // 3, 1), (n, 1))
    keys = torch.cat([grp[:, None], vox, vox % 7, vox % 3], 1)
    new_keys, plan = ops.unique_rows(keys)
    return new_keys, plan.cnt, plan.inv


@cases("cluster_key_survival", ragged=dict(n=1009, ng=6), minimal=dict(n=1, ng=1), empty=dict(n=0, ng=1))
def _cluster_key_survival(ops, dev, n, ng):
    new_keys, cnt, inv = _key_survival_inputs(ops, dev, n, ng, 66)
    return lambda: ops.cluster_key_survival(new_keys, cnt, inv, 1, 2, ng)


@cases("cluster_point_ids", ragged=dict(n=1009, ng=6), minimal=dict(n=1, ng=1), empty=dict(n=0, ng=1))
def _cluster_point_ids(ops, dev, n, ng):
    new_keys, cnt, inv = _key_survival_inputs(ops, dev, n, ng, 67)
    k_idx, k_group, v_idx, vox_inv = ops.cluster_key_survival(new_keys, cnt, inv, 1, 2, ng)
    labels = torch.cumsum(randint(dev, G(67), 0, 2, (k_idx.numel(),)), 0).int()
    gp = (torch.arange(v_idx.numel(), device=dev) % ng).long()
    bp = torch.zeros_like(gp)
    return lambda: ops.cluster_point_ids(labels, k_group, vox_inv, gp, bp, ng)


@cases("nms_select", ragged=dict(n=1009, c=5, max_num=83), minimal=dict(n=1, c=1, max_num=1), few=dict(n=131, c=3, max_num=500), empty=dict(n=0, c=3, max_num=5))
def _nms_select(ops, dev, n, c, max_num):
    g = G(68)
    boxes = randn(dev, g, n, 9)
    scores, (order, rank, count) = _ranked(ops, dev, n, c, 68)
    keep, num, flag = ops.nms_bev_multiclass(nms_boxes(dev, n, 68), rank, count, 0.25, True, max_keep=max_num, windowed=True)
    lut = torch.arange(c, device=dev).flip(0).contiguous()

    def run():
        buf = ops.nms_select(boxes, scores, order, keep, num, max_num, max_num, lut, flag)
        meta = buf[max_num * 11:].view(torch.int32)
        rows = int(meta[0])  # rows written: the rest of the max_num rows is capacity
        return buf[:rows * 11], meta
    return run


@cases("connected_components", ragged=dict(n=1009), minimal=dict(n=1), empty=dict(n=0))
def _connected_components(ops, dev, n):
    g = G(69)
    pts = randn(dev, g, n, 3, scale=8.0)
    batch = randint(dev, g, 0, 2, (n,))
    return lambda: (ops.connected_components(pts, 0.6), ops.connected_components(pts, 0.6, batch))


@cases("connected_components_grouped", ragged=dict(n=1009, ng=6), minimal=dict(n=1, ng=1), empty=dict(n=0, ng=1))
def _connected_components_grouped(ops, dev, n, ng):
    g = G(70)
    pts = randn(dev, g, n, 3, scale=8.0)
    grp = torch.sort(randint(dev, g, 0, ng, (n,)))[0]
    dist = torch.rand(ng, generator=g).to(dev) + 0.3
    return lambda: ops.connected_components_grouped(pts, grp, dist)


@cases("norm_act", ragged=dict(n=1009, c=133), minimal=dict(n=1, c=1), wide=dict(n=509, c=1000), empty=dict(n=0, c=12))
def _norm_act(ops, dev, n, c):
    g = G(71)
    x, gamma, beta = randn(dev, g, n, c), torch.rand(c, generator=g).to(dev) + 0.5, randn(dev, g, c)

    def run():
        dst = torch.zeros((n, c + 3), device=dev)
        ops.norm_act(x, gamma, beta, 1e-3, "affine", "relu", out=dst[:, 1:1 + c])
        return ops.norm_act(x, gamma, beta, 1e-3, "ln", "gelu", inplace=False), dst
    return run


@cases("column_sum", ragged=dict(n=1009, c=131), minimal=dict(n=1, c=1), empty=dict(n=0, c=12), wide=dict(n=8191, c=300))
def _column_sum(ops, dev, n, c):
    x = randn(dev, G(72), n, c)
    return lambda: ops.column_sum(x)


@cases("column_mean_var", ragged=dict(n=1009, c=131), minimal=dict(n=1, c=1), empty=dict(n=0, c=12), wide=dict(n=8191, c=300))
def _column_mean_var(ops, dev, n, c):
    x = randn(dev, G(73), n, c)
    return lambda: ops.column_mean_var(x)


@cases("batch_norm_train_stats", ragged=dict(n=1009, c=131), minimal=dict(n=1, c=1), wide=dict(n=8191, c=300))
def _batch_norm_train_stats(ops, dev, n, c):
    g = G(74)
    x, w, b = randn(dev, g, n, c), torch.rand(c, generator=g).to(dev) + 0.5, randn(dev, g, c)
    rm0, rv0 = randn(dev, g, c), torch.rand(c, generator=g).to(dev) + 0.5

    def run():
        rm, rv = rm0.clone(), rv0.clone()
        return ops.batch_norm_train_stats(x, w, b, 1e-3, 0.1, rm, rv), rm, rv
    return run


@cases("batch_norm_act_forward", ragged=dict(n=1009, c=131), minimal=dict(n=1, c=1), empty=dict(n=0, c=12))
def _batch_norm_act_forward(ops, dev, n, c):
    g = G(75)
    x, sc, sh = randn(dev, g, n, c), torch.rand(c, generator=g).to(dev) + 0.5, randn(dev, g, c)
    return lambda: ops.batch_norm_act_forward(x, sc, sh, True)


@cases("batch_norm_act_backward", ragged=dict(n=1009, c=131), minimal=dict(n=1, c=1), empty=dict(n=0, c=12), wide=dict(n=8191, c=300))
def _batch_norm_act_backward(ops, dev, n, c):
    g = G(76)
    x, go = randn(dev, g, n, c), randn(dev, g, n, c)
    mean, invstd, sc, sh = randn(dev, g, c, scale=0.1), torch.rand(c, generator=g).to(dev) + 0.5, torch.rand(c, generator=g).to(dev) + 0.5, randn(dev, g, c)
    return lambda: ops.batch_norm_act_backward(x, go, mean, invstd, sc, sh, True)


@cases("norm_act_backward", ragged=dict(n=1009, c=133), minimal=dict(n=1, c=1), wide=dict(n=2003, c=768), empty=dict(n=0, c=12))
def _norm_act_backward(ops, dev, n, c):
    g = G(77)
    x, go, gamma, beta = randn(dev, g, n, c), randn(dev, g, n, c), torch.rand(c, generator=g).to(dev) + 0.5, randn(dev, g, c)
    return lambda: ops.norm_act_backward(x, go, gamma, beta, 1e-3, "gelu")


@cases("sorted_rows", ragged=dict(n=1009, m=37, cols=5, lazy=True), minimal=dict(n=1, m=1, cols=3, lazy=False), empty=dict(n=0, m=3, cols=5, lazy=False))
def _sorted_rows(ops, dev, n, m, cols, lazy):
    g = G(78)
    inv = randint(dev, g, 0, m, (n,))
    inv[:min(n, m)] = torch.arange(min(n, m), device=dev)
    order = torch.argsort(inv, stable=True).to(torch.int32)
    pts, fcl, centers = wide(randn(dev, g, n, cols)), wide(randn(dev, g, n, 3)), wide(randn(dev, g, m, 3))
    index = randint(dev, g, 0, 3 * n + 1, (n,))

    def run():
        table = torch.zeros((m, 13), device=dev)
        return ops.sorted_rows(order, inv, pts, f_cluster=None if lazy else fcl, centers=centers if lazy else None, index=index, fill=table), table
    return run


@cases("sir_stack_forward", ragged=dict(n=1009, groups=37, rows=True), minimal=dict(n=1, groups=1, rows=True), sparse=dict(n=787, groups=701, rows=False))
def _sir_stack_forward(ops, dev, n, groups, rows):
    from fullysparsefusion_amd.mmdet3d_plugin import models  # noqa: F401  (registers the modules)
    from fullysparsefusion_amd.mmdet3d_plugin.ops import sst_ops
    from fullysparsefusion_amd.mmdet3d_plugin.registry import build_backbone

    torch.manual_seed(79)
    sir = build_backbone(dict(type="SIR", num_blocks=3, in_channels=[5 + 11 + 33 + 131, 133, 133], feat_channels=[[128, 128]] * 3,
                              rel_mlp_hidden_dims=[[16, 32]] * 3, norm_cfg=dict(type="LN", eps=1e-3), mode="max", xyz_normalizer=[20, 20, 4],
                              act="gelu", unique_once=True)).to(dev).eval()
    desc = sst_ops.sir_stack_descriptor(sir, sir.block_list)
    assert desc is not None and sum(sum(w) for w in desc.widths) == 768
    points, parts, fcl, idx, _, _ = _sir_input_args(dev, n, 79)
    seg = randint(dev, G(79), 0, groups, (n,))
    seg[:min(n, groups)] = torch.arange(min(n, groups), device=dev)
    seg = torch.sort(seg)[0].contiguous()

    def run():
        table = torch.full((groups, 772), float("-inf"), device=dev)
        with torch.no_grad():
            out = ops.sir_stack_forward(desc, points, parts, fcl, seg, table[:, :768], rows, feats_index=idx)
        return out, table
    return run


@cases("compact_pairs", ragged=dict(k=401, p=1009), minimal=dict(k=1, p=1), empty=dict(k=5, p=7, none=True))
def _compact_pairs(ops, dev, k, p, none=False):
    g = G(80)
    means, centers = wide(randn(dev, g, k, 3)), randn(dev, g, p, 3)
    g_ids, p_ids, b_pts = (randint(dev, g, 0, 1 << 40, (p,)) for _ in range(3))
    k_idx = torch.nonzero(torch.rand(k, generator=g) > (2.0 if none else 0.3 if k > 1 else -1.0)).squeeze(1).to(dev)
    v_idx = torch.nonzero(torch.rand(p, generator=g) > (2.0 if none else 0.2 if p > 1 else -1.0)).squeeze(1).to(dev)
    return lambda: ops.compact_pairs(means, k_idx, g_ids, p_ids, b_pts, centers, v_idx)


@cases("combine_queries", ragged=dict(mf=241, ml=1009), minimal=dict(mf=1, ml=1), no_frustum=dict(mf=0, ml=5), no_lidar=dict(mf=3, ml=0), empty=dict(mf=0, ml=0))
def _combine_queries(ops, dev, mf, ml):
    g = G(81)
    fc, lc = randn(dev, g, mf, 3), randn(dev, g, ml, 3)
    fco, lco, fp = randint(dev, g, 0, 300, (mf, 3)), randint(dev, g, 0, 5000, (ml, 3)), randn(dev, g, mf, 8)
    return lambda: ops.combine_queries(fc, lc, fco, lco, fp, 1000)


@cases("decode_rois", ragged=dict(m=1009, code=10), minimal=dict(m=1, code=8), empty=dict(m=0, code=10))
def _decode_rois(ops, dev, m, code):
    g = G(82)
    reg, centers, coors = wide(randn(dev, g, m, code, scale=0.7)), wide(randn(dev, g, m, 3, scale=30.0)), randint(dev, g, 0, 4, (m, 3))
    return lambda: ops.decode_rois(reg, centers, coors[:, 0], 1e-6)


@cases("refine_rows", ragged=dict(n=2003, k=1009, r=37), minimal=dict(n=1, k=1, r=1), empty=dict(n=5, k=0, r=1))
def _refine_rows(ops, dev, n, k, r):
    g = G(83)
    points, info, roi_xyz = wide(randn(dev, g, n, 5)), randn(dev, g, k, 13), wide(randn(dev, g, r, 3))  # (`info` has no stride in the ABI)
    pts_idx, roi_idx = randint(dev, g, 0, n, (k,)), torch.sort(randint(dev, g, 0, r, (k,)))[0]
    return lambda: ops.refine_rows(info, points, pts_idx, roi_idx, roi_xyz)


@cases("encode_preds_2d", ragged=dict(a=61, m=1009), minimal=dict(a=1, m=1), empty=dict(a=1, m=0))
def _encode_preds_2d(ops, dev, a, m):
    g = G(84)
    anno = torch.rand(a, 8, generator=g)
    anno[:, :4] *= torch.tensor([1600.0, 900.0, 1600.0, 900.0])
    anno[:, 5], anno[:, 6] = torch.randint(0, 10, (a,), generator=g).float(), torch.randint(0, 6, (a,), generator=g).float()
    coors = torch.zeros((m, 3), dtype=torch.int64)
    coors[:, 2] = torch.randint(0, a + 1, (m,), generator=g)  # 0 = no object
    anno, coors = anno.to(dev), coors.to(dev)
    return lambda: ops.encode_preds_2d(anno, coors, 10, 1600, 900)


@cases("weighted_xyz", ragged=dict(n=1009), minimal=dict(n=1), empty=dict(n=0))
def _weighted_xyz(ops, dev, n):
    g = G(85)
    pts, w = wide(randn(dev, g, n, 5, scale=20.0)), torch.rand(n, 1, generator=g).to(dev)
    w[::7] = 0.0
    return lambda: ops.weighted_xyz(pts, w, 1e-5)


@cases("centroid_divide", ragged=dict(m=1009), minimal=dict(m=1), empty=dict(m=0))
def _centroid_divide(ops, dev, m):
    mean = torch.rand(m, 4, generator=G(86)).to(dev) + 0.1
    return lambda: ops.centroid_divide(mean)


@cases("lidar_cluster_frontend", ragged=dict(m=4099, spread=12.0), minimal=dict(m=1, spread=1.0), sparse=dict(m=1009, spread=50.0))
def _lidar_cluster_frontend(ops, dev, m, spread):
    g = G(87)
    ng, nc = 6, 10
    cols = [[0], [1, 2], [3], [4, 5], [6], [7, 8]]
    scores = wide(torch.rand(m, nc, generator=g).to(dev))
    logits, offsets = wide(randn(dev, g, m, nc + 1)), wide(randn(dev, g, m, 3 * nc, scale=0.3))
    pts = wide(torch.cat([randn(dev, g, m, 3, scale=spread).clamp(-50, 50) * torch.tensor([1.0, 1.0, 0.05], device=dev), randn(dev, g, m, 2)], 1))
    thresh = torch.full((ng,), 0.6, device=dev)
    thresh[-1] = 2.0
    vs = [[0.4, 0.4, 6.0]] * ng
    cells = [int(np.ceil(108.0 / 0.4)), int(np.ceil(108.0 / 0.4)), int(np.ceil(8.0 / 6.0))]
    key_min, key_max = [0] + [-(c // 2) - 8 for c in cells], [ng - 1] + [c + c // 2 + 8 for c in cells]
    dist = torch.full((ng,), 0.6, device=dev)

    def run():
        res = ops.lidar_cluster_frontend(scores, thresh, cols, logits, offsets, pts, None, nc, vs, PC_RANGE[:3], key_min, key_max, 2, dist)
        c = res["counts"]
        return [res[k] for k in ("p_ids", "centers", "cluster_inds", "points", "new_coors", "cluster_xyz")], _plan_outputs(res["plan"]), \
            torch.tensor([c[k] for k in ("pairs", "keys", "kept_keys", "rows", "clusters")])
    return run


# ------------------------------------------------------------------------------------------------ the checks
def flatten(out):
    """Every tensor of a wrapper's result, in order (tuples, lists, dicts, dataclasses; None and numbers kept as markers)."""
    if torch.is_tensor(out):
        return [out]
    if out is None or isinstance(out, (int, float, bool, str)):
        return [out]
    if dataclasses.is_dataclass(out):
        return flatten([getattr(out, f.name) for f in dataclasses.fields(out)])
    if isinstance(out, dict):
        return flatten([out[k] for k in sorted(out)])
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in flatten(o)]
    raise TypeError(f"unexpected result type {type(out)}")


def same_bits(a, b):
    if not torch.is_tensor(a) or not torch.is_tensor(b):
        return type(a) is type(b) and a == b
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def describe_difference(a, b):
    if not torch.is_tensor(a) or not torch.is_tensor(b) or a.shape != b.shape or a.dtype != b.dtype:
        return f"{a if not torch.is_tensor(a) else (tuple(a.shape), a.dtype)} vs {b if not torch.is_tensor(b) else (tuple(b.shape), b.dtype)}"
    x, y = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    diff = (x.view(torch.uint8).view(-1, a.element_size()) != y.view(torch.uint8).view(-1, a.element_size())).any(1).nonzero().squeeze(1)
    k = int(diff[0])
    return f"{diff.numel()} of {x.numel()} elements of {tuple(a.shape)} {a.dtype} differ, first at flat index {k}: {x[k].item()} vs {y[k].item()}"


def three_runs(run, scratch_expected=None):
    """run() plain, under guarded(0xFF), under guarded(0x00): the flattened plain result; guards, interception and bits asserted."""
    plain = flatten(run())
    torch.cuda.synchronize()
    for fill in FILLS:
        with guarded(fill) as g:
            got = flatten(run())
            bad = g.violations()
        assert bad == [], f"fill 0x{fill:02X}: guard bytes overwritten: {bad[:4]}"
        assert g.counts["empty"] + g.counts["workspace"] >= 1, "nothing was intercepted"
        if scratch_expected is not None:
            scratch_expected(g)
        assert len(got) == len(plain)
        for i, (a, b) in enumerate(zip(plain, got)):
            assert same_bits(a, b), f"fill 0x{fill:02X}: result {i} differs from the plain run: {describe_difference(a, b)}"
    return plain


def _uses_scratch(name):
    from test_guarded_alloc_cpu import allocating_wrappers

    return name in allocating_wrappers()[1]


# wrappers that size their scratch themselves (a torch.empty of their own) instead of asking _lib.workspace; `seg_targets` and
# `nms_bev_multiclass` go through _lib.workspace in this tree
OWN_SCRATCH = {"overlap_plan", "sir_stack_forward", "lidar_cluster_frontend"}


@pytest.mark.parametrize("name,kind", [(n, k) for n in sorted(CASES) for k, _ in CASES[n]])
def test_wrapper_under_guard_bands_and_poison(ops, device, name, kind):
    build = dict(CASES[name])[kind]
    run = build(ops, device)

    def scratch_expected(g):
        if name in OWN_SCRATCH:
            assert any(r["site"] == name and r["kind"] == "empty" for r in g.records), "the wrapper's own scratch was not intercepted"
        elif _uses_scratch(name):
            # (that the helper serves a request at exactly its size is tests/test_guarded_alloc_cpu.py's; here: the wrapper itself asked)
            assert any(r["kind"] == "workspace" and r["site"] == name for r in g.records), "no scratch request of the wrapper was intercepted"

    three_runs(run, scratch_expected)


# ------------------------------------------------------------------------------------------------ whole passes
def _frame(device):
    import bench

    return bench.make_inputs(1, 3, device)[1]


def test_simple_test_under_guard_bands_and_poison(device):
    """A whole FSF.simple_test (smallest synthetic nuScenes-shape frame, nothing announced, no graph capture): the argument shapes the
    model really produces, for the arena ops and the fused stacks above all."""
    import bench

    model = bench.build_model(device)
    frame = _frame(device)

    def run():
        with torch.no_grad():
            r = model.simple_test(frame["points"], frame["img_metas"], frame["mask_data"], frame["mask_anno"])[0]
        return r["boxes_3d"].tensor, r["scores_3d"], r["labels_3d"]

    boxes, scores, labels = three_runs(run)
    assert boxes.size(0) > 20 and scores.size(0) == boxes.size(0) == labels.size(0)


def test_training_step_under_guard_bands_and_poison(device):
    """forward_train_graph with the segmentation and LiDAR-query head losses, then backward(): losses and every parameter's gradient.
    torch's own autograd buffers are not intercepted."""
    import bench

    torch.manual_seed(0)
    model = bench.build_model(device).train()
    _, inp = bench.make_inputs(1, 3, device, frames=1)
    torch.manual_seed(11)
    with torch.no_grad():
        out = model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"])
    centres = out["fsd_obj_centers"][::20].detach().cpu()
    m = centres.shape[0]
    assert m >= 5, m
    k = torch.arange(m, dtype=torch.float32)
    boxes = torch.stack([centres[:, 0], centres[:, 1], centres[:, 2] - 0.75, 1.0 + 0.1 * (k % 5), 1.6 + 0.2 * (k % 3), torch.full((m,), 1.5),
                         0.3 * k - 1.0, 0.1 * k, -0.05 * k], 1)
    labels = torch.arange(m) % 10
    state = {n: b.clone() for n, b in model.named_buffers()}  # (BatchNorm running statistics move in a training forward)
    names = [n for n, _ in model.named_parameters()]

    def run():
        with torch.no_grad():
            for n, b in model.named_buffers():
                b.copy_(state[n])
        model.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        o = model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"], gt_bboxes_3d=[boxes],
                                      gt_labels_3d=[labels], lidar_head_losses=True)
        losses = o["losses"]
        loss_names = sorted(k_ for k_ in losses if "loss" in k_ and torch.is_tensor(losses[k_]) and losses[k_].requires_grad)
        sum(losses[k_] for k_ in loss_names).backward()
        grads = [p.grad for _, p in model.named_parameters()]
        assert sum(g is not None for g in grads) > 50
        return [losses[k_].detach() if torch.is_tensor(losses[k_]) else losses[k_] for k_ in sorted(losses)], grads

    plain = three_runs(run)
    assert len(plain) > len(names) // 2
