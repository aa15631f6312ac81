"""Train-time augmentation on the device (K40, docs/kernels/K40_train_augment.md): K40a -> radix sort -> K40b and K40c against the host
specification of datasets/train_augment.py, `torch.equal` on the float bits; determinism; and `DeviceTrainAugment` end to end — the
losses of `FSF.forward_train` on the device-augmented frame (dropped boxes as label -1, everything on the device) are the bits of the
losses on the host-specification frame with compacted GT lists."""
import itertools

import numpy as np
import pytest
import torch

from fullysparsefusion_amd.mmdet3d_plugin.datasets.train_augment import (DeviceTrainAugment, augment_boxes_host, augment_points_host,
                                                                         shuffle_permutation_host, train_descriptor)
from test_frustum_assign_gpu import train_graph  # noqa: F401  (the small training frame's builder)

pytestmark = pytest.mark.gpu

RANGE = [-50.0, -50.0, -4.99, 50.0, 50.0, 2.99]
TRANS = (0.5, -0.3, 0.2)
DESCRIPTORS = list(itertools.product((False, True), (False, True), (0.0, 0.3), (1.0, 0.95), ((0.0, 0.0, 0.0), TRANS)))


def bits(t):
    return t.contiguous().view(torch.int32)


def aug_of(flip_h=False, flip_v=False, rot=0.0, scale=1.0, trans=(0.0, 0.0, 0.0), seed=-1):
    return dict(pcd_horizontal_flip=flip_h, pcd_vertical_flip=flip_v, pcd_rot_factor=rot, pcd_scale_factor=scale,
                pcd_trans=np.asarray(trans, dtype=np.float64), shuffle_seed=seed)


@pytest.fixture(scope="module")
def ops(device):
    from fullysparsefusion_amd import hip_ops_augment

    return hip_ops_augment


def cloud(n, cols, seed, spread=(60.0, 60.0, 6.0)):
    """Host cloud f32 [n, cols]: xyz across and beyond RANGE, a NaN x / y / z row each where there is room."""
    g = torch.Generator().manual_seed(seed)
    pts = torch.cat([(torch.rand(n, 3, generator=g) * 2 - 1) * torch.tensor(spread), torch.rand(n, cols - 3, generator=g)], 1)
    for k, row in enumerate((5, n // 2, n - 2)):
        if n > 16:
            pts[row, k] = float("nan")
    return pts


def check_points(ops, dev, pts, aug, pc_range=RANGE):
    """One call against the specification: the count, and the bits of the rows below it (rows beyond `count` are not compared)."""
    want, order = augment_points_host(pts, aug, pc_range)
    out, count = ops.train_augment_points(pts.to(dev), train_descriptor(aug), pc_range, aug["shuffle_seed"])
    k = int(count)
    assert out.shape == pts.shape and k == want.shape[0], (k, want.shape[0], aug)
    assert torch.equal(bits(out[:k].cpu()), bits(want)), aug
    return want, order


@pytest.mark.parametrize("n", [0, 1, 2047, 2048, 2049, 3 * 2048 + 5, 20001])  # the sorter's tile edges, a multi-tile look-back
def test_points_equal_the_specification_bit_for_bit(ops, device, n):
    dropped_nan = 0
    for cols in (3, 7, 8):
        pts = cloud(n, cols, 100 + cols)
        for i, (fh, fv, rot, scale, t) in enumerate(DESCRIPTORS):
            for seed in (-1, 1000003 * i + cols + (i << 40)):  # source order; shuffled (a seed with a high half)
                want, order = check_points(ops, device, pts, aug_of(fh, fv, rot, scale, t, seed))
                if seed < 0:
                    assert torch.equal(order, torch.sort(order).values)
                elif n > 16:
                    perm = torch.from_numpy(shuffle_permutation_host(n, seed))
                    keep = torch.zeros(n, dtype=torch.bool)
                    keep[order] = True
                    assert torch.equal(order, perm[keep[perm]]) and not torch.equal(order, torch.sort(order).values)
                if n > 16:
                    assert 0 < order.numel() < n - 2 and not bool(torch.isin(torch.tensor([5, n // 2, n - 2]), order).any())
                    dropped_nan += 1
    assert n <= 16 or dropped_nan == 3 * len(DESCRIPTORS) * 2  # NaN xyz rows are dropped: the strict comparisons are false
    if n == 1:  # the one row kept, and the one row dropped
        one = torch.tensor([[1.0, 2.0, 0.5, 0.25, 7.0, 1.0, 2.0, 0.5]])
        for seed in (-1, 9):
            assert check_points(ops, device, one, aug_of(True, True, 0.3, 0.95, TRANS, seed))[1].tolist() == [0]
            assert check_points(ops, device, one * 100, aug_of(True, True, 0.3, 0.95, TRANS, seed))[1].tolist() == []


def on_the_bound(bound, t):
    """An fp32 x with fp32(x + fp32(t)) == bound exactly, found by inverting the translation in fp32 and checked on the host."""
    t32 = np.float32(t)
    x = np.float32(np.float32(bound) - t32)
    for cand in (x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))):
        if np.float32(cand + t32) == np.float32(bound):
            return float(cand)
    raise AssertionError((bound, t))


@pytest.mark.parametrize("cols", [3, 8])
def test_rows_all_out_all_in_and_exactly_on_a_bound(ops, device, cols):
    n = 2 * 2048 + 77
    for seed in (-1, 4242):
        # every row out of range
        out_pts = cloud(n, cols, 7)
        out_pts[:, 0] = out_pts[:, 0].abs() + 51.0
        want, _ = check_points(ops, device, out_pts, aug_of(False, True, 0.0, 1.0, (0.0, 0.0, 0.0), seed))
        assert want.shape[0] == 0
        # none out of range
        in_pts = cloud(n, cols, 8, spread=(30.0, 30.0, 2.0))
        in_pts = torch.where(torch.isnan(in_pts), torch.zeros(()), in_pts)
        want, _ = check_points(ops, device, in_pts, aug_of(True, False, 0.3, 0.95, TRANS, seed))
        assert want.shape[0] == n
        # rows whose augmented coordinate equals a bound exactly (dropped: the test is strict), beside rows one ulp inside (kept)
        aug = aug_of(trans=TRANS, seed=seed)
        rows = []
        for axis in range(3):
            for bound in (RANGE[axis], RANGE[axis + 3]):
                v = np.float32(on_the_bound(bound, TRANS[axis]))
                inside = np.nextafter(v, np.float32(0.0))
                assert np.float32(inside + np.float32(TRANS[axis])) != np.float32(bound)
                for value in (v, inside):
                    row = [1.0, 2.0, 0.5] + [0.25] * (cols - 3)
                    row[axis] = float(value)
                    rows.append(row)
        edge = torch.tensor(rows, dtype=torch.float32)
        host = edge[:, :3] + torch.tensor([np.float32(v) for v in TRANS])
        assert int(((host == torch.tensor(RANGE[:3])) | (host == torch.tensor(RANGE[3:]))).any(1).sum()) == 6  # verified on the host first
        pts = torch.cat([in_pts[:1000], edge, in_pts[1000:]])
        want, order = check_points(ops, device, pts, aug)
        kept_edges = sorted(int(r) - 1000 for r in order.tolist() if 1000 <= r < 1012)
        assert kept_edges == [1, 3, 5, 7, 9, 11] and want.shape[0] == n + 6


def box_batch(sizes, dim, seed):
    g = torch.Generator().manual_seed(seed)
    total = sum(sizes)
    boxes = torch.zeros(total, dim)
    boxes[:, :2] = (torch.rand(total, 2, generator=g) * 2 - 1) * 58
    boxes[:, 2] = torch.rand(total, generator=g) * 3 - 3
    boxes[:, 3:6] = torch.rand(total, 3, generator=g) * 4 + 0.5
    boxes[:, 6] = (torch.rand(total, generator=g) * 2 - 1) * 7
    boxes[:, 7:] = torch.randn(total, dim - 7, generator=g) * 3
    no_aug = boxes + torch.randn(total, dim, generator=g)
    labels = torch.randint(-1, 10, (total,), generator=g)
    return boxes, labels, no_aug, labels.clone()


def boxes_on_host(boxes, labels, no_aug, na_labels, sizes, augs, form="in_place"):
    parts = []
    for chunk, aug in zip(zip(*(torch.split(t, list(sizes)) for t in (boxes, labels, no_aug, na_labels))), augs):
        parts.append(augment_boxes_host(*chunk, aug, RANGE)[form])
    return [torch.cat(p) for p in zip(*parts)]


BATCH_AUGS = [aug_of(True, False, 0.3, 0.95, TRANS), aug_of(False, True, -0.785, 1.1), aug_of(True, True, 0.0, 1.0, (-0.25, 0.75, 0.0))]


@pytest.mark.parametrize("dim", [7, 9])
@pytest.mark.parametrize("sizes", [(0, 1, 300), (300, 0, 1), (1, 300, 0)])
def test_boxes_equal_the_specification_bit_for_bit(ops, device, dim, sizes):
    boxes, labels, no_aug, na_labels = box_batch(sizes, dim, 31 + dim)
    edge = sizes[0] + sizes[1]
    if sizes[2] == 300:  # a box whose augmented x equals the bound exactly (both flips, t = (-0.25, 0.75, 0): -(-50.25) - 0.25 = 50): dropped
        boxes[edge, 0], boxes[edge, 1], labels[edge], na_labels[edge] = -50.25, 1.0, 4, 4
    want = boxes_on_host(boxes, labels, no_aug, na_labels, sizes, BATCH_AUGS)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    descs = [train_descriptor(a) for a in BATCH_AUGS]
    wide = torch.full((sum(sizes), dim + 5), 9.0)
    wide[:, 2:2 + dim] = boxes
    strided = wide.to(device)[:, 2:2 + dim]  # a strided box view
    assert not strided.is_contiguous()
    got = ops.train_augment_boxes(strided, labels.to(device), no_aug.to(device), na_labels.to(device), offsets, descs, RANGE)
    again = ops.train_augment_boxes(boxes.to(device), labels.to(device), no_aug.to(device), na_labels.to(device), offsets, descs, RANGE)
    for g, a, w in zip(got, again, want):
        assert g.shape == w.shape and g.dtype == w.dtype
        same = torch.equal(bits(g.cpu()), bits(w)) if w.dtype == torch.float32 else torch.equal(g.cpu(), w)
        assert same and torch.equal(g, a)  # the specification's bits; two runs, strided and contiguous, the same bits
    b, l, nb, nl = (t.cpu() for t in got)
    assert torch.equal(l < 0, nl < 0) and bool((l[labels < 0] == labels[labels < 0]).all())  # labels already < 0 stay
    dropped = (l < 0) & (labels >= 0)
    assert 0 < int(dropped.sum()) < int((labels >= 0).sum())
    assert bool(((b[:, 6] >= -np.pi - 1e-6) & (b[:, 6] < np.pi + 1e-6)).all()) and bool(((nb[:, 6] >= -np.pi - 1e-6) & (nb[:, 6] < np.pi + 1e-6)).all())
    if sizes[2] == 300:
        assert float(b[edge, 0]) == RANGE[3] and int(l[edge]) == -1 and int(nl[edge]) == -1


def test_an_empty_batch_and_invalid_arguments(ops, device):
    from fullysparsefusion_amd._lib import FsfHipError

    empty = torch.zeros(0, 9, device=device)
    none = torch.zeros(0, dtype=torch.int64, device=device)
    desc = train_descriptor(aug_of())
    out = ops.train_augment_boxes(empty, none, empty, none, [0, 0, 0], [desc, desc], RANGE)
    assert [tuple(t.shape) for t in out] == [(0, 9), (0,), (0, 9), (0,)]
    bad = list(desc)
    bad[2] = 0.0  # scale must be positive
    with pytest.raises(FsfHipError):
        ops.train_augment_boxes(empty, none, empty, none, [0, 0], [bad], RANGE)
    with pytest.raises(FsfHipError):
        ops.train_augment_points(torch.zeros(4, 8, device=device), bad, RANGE, 3)
    with pytest.raises(FsfHipError):
        ops.train_augment_boxes(empty, none, empty, none, [0] * 34, [desc] * 33, RANGE)  # more samples than FSF_TRAIN_AUGMENT_MAX_BATCH


def test_count_on_the_host_and_a_short_workspace_through_the_c_abi(ops, device):
    import ctypes

    from fullysparsefusion_amd import _lib

    h = _lib.lib()
    pts = cloud(2049, 7, 5)
    aug = aug_of(True, False, 0.3, 0.95, TRANS, 17)
    want, _ = augment_points_host(pts, aug, RANGE)
    dpts, out = pts.to(device), torch.zeros(2049, 7, device=device)
    count, host = torch.zeros(1, dtype=torch.int64, device=device), ctypes.c_int64(-1)
    nbytes = int(h.fsf_train_augment_points_workspace_bytes(2049))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    args = (_lib.ptr(dpts), 2049, 7, _lib.f32_array(train_descriptor(aug)), _lib.f32_array(RANGE), 17, _lib.ptr(out), _lib.ptr(count),
            ctypes.cast(ctypes.byref(host), _lib.c_p), _lib.ptr(ws))
    assert h.fsf_train_augment_points(*args, nbytes - 1, _lib.stream_ptr()) == _lib.DEFINES["FSF_ERR_WORKSPACE"] and host.value == -1
    waits = int(h.fsf_get_option(_lib.DEFINES["FSF_OPT_HOST_WAITS"]))
    _lib.check(h.fsf_train_augment_points(*args, nbytes, _lib.stream_ptr()), "fsf_train_augment_points")
    assert host.value == want.shape[0] == int(count) and int(h.fsf_get_option(_lib.DEFINES["FSF_OPT_HOST_WAITS"])) == waits + 1
    assert torch.equal(bits(out[:host.value].cpu()), bits(want))
    ops.train_augment_points(dpts, train_descriptor(aug), RANGE, 17)  # the wrapper passes no host pointer: no wait
    assert int(h.fsf_get_option(_lib.DEFINES["FSF_OPT_HOST_WAITS"])) == waits + 1


def test_two_runs_of_the_batch_call_give_the_same_bits(device):
    aug = DeviceTrainAugment(dict(flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
                             dict(rot_range=[-0.785, 0.785], scale_ratio_range=[0.9, 1.1], translation_std=[0.5, 0.5, 0.5]), RANGE)
    sizes = (5, 0, 40)
    boxes, labels, _, _ = box_batch(sizes, 9, 77)
    clouds = [cloud(n, 8, 200 + n).to(device) for n in (4099, 1, 2048)]
    gt_b = [b.to(device) if k else b for k, b in enumerate(torch.split(boxes, list(sizes)))]  # GT rows on the host and on the device
    gt_l = list(torch.split(labels, list(sizes)))
    metas = [dict(sample_idx=k) for k in range(3)]
    runs = [aug(clouds, gt_b, gt_l, metas, rng=np.random.RandomState(12)) for _ in range(2)]
    for a, b in zip(*runs):
        for x, y in zip(a, b):
            if isinstance(x, dict):
                assert x["shuffle_seed"] == y["shuffle_seed"] and x["pcd_rot_factor"] == y["pcd_rot_factor"] and x["sample_idx"] == y["sample_idx"]
            else:
                assert x.is_cuda and torch.equal(bits(x) if x.dtype == torch.float32 else x, bits(y) if y.dtype == torch.float32 else y)
    pts, out_metas, na_b, na_l, b, l = runs[0]
    assert len({m["shuffle_seed"] for m in out_metas}) == 3 and "pcd_trans" in out_metas[0] and "pcd_rot_factor" not in metas[0]
    # every frame against the specification with the draws its meta records
    for k in range(3):
        a = out_metas[k]
        want, _ = augment_points_host(clouds[k].cpu(), a, RANGE)
        assert torch.equal(bits(pts[k].cpu()), bits(want))
        spec = augment_boxes_host(gt_b[k].cpu(), gt_l[k], gt_b[k].cpu(), gt_l[k], a, RANGE)["in_place"]
        for got, w in zip((b[k], l[k], na_b[k], na_l[k]), spec):
            assert torch.equal(got.cpu(), w) and (w.dtype != torch.float32 or torch.equal(bits(got.cpu()), bits(w)))


def test_forward_train_on_the_device_augmented_frame_equals_the_host_specification_frame(train_graph):  # noqa: F811
    model, inp, gt_boxes, gt_labels, _ = train_graph
    dev = inp["points"][0].device
    flip = dict(flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5)
    rst = dict(rot_range=[-0.785, 0.785], scale_ratio_range=[0.9, 1.1], translation_std=[0.5, 0.5, 0.5])
    seed = 3
    # the range: the model's, with x_max between the two largest augmented box x of this seed's draw — one box drops, and points with it
    probe = DeviceTrainAugment(flip, rst, RANGE).draw(np.random.RandomState(seed))
    xs = torch.sort(augment_boxes_host(gt_boxes[0], gt_labels[0], gt_boxes[0], gt_labels[0], probe, RANGE)["in_place"][0][:, 0]).values
    pc_range = RANGE[:3] + [float((xs[-1] + xs[-2]) / 2)] + RANGE[4:]
    augment = DeviceTrainAugment(flip, rst, pc_range)
    pts, metas, na_b, na_l, b, l = augment(inp["points"], gt_boxes, gt_labels, inp["img_metas"], rng=np.random.RandomState(seed))
    a = metas[0]
    assert a["shuffle_seed"] == probe["shuffle_seed"] and a["pcd_rot_factor"] == probe["pcd_rot_factor"] and b[0].is_cuda and l[0].is_cuda
    n_in, g_in = inp["points"][0].shape[0], gt_labels[0].numel()
    dropped_boxes = int(((l[0] < 0) & (gt_labels[0].to(dev) >= 0)).sum())
    print(f"K40 end to end: {n_in} -> {pts[0].shape[0]} points, {g_in} boxes of which {dropped_boxes} dropped")
    assert dropped_boxes >= 1 and 0 < pts[0].shape[0] < n_in
    host_pts, _ = augment_points_host(inp["points"][0].cpu(), a, pc_range)
    spec = augment_boxes_host(gt_boxes[0], gt_labels[0], gt_boxes[0], gt_labels[0], a, pc_range)
    assert torch.equal(bits(pts[0].cpu()), bits(host_pts)) and torch.equal(bits(b[0].cpu()), bits(spec["in_place"][0]))
    cb, cl, cnb, cnl = spec["compact"]
    assert cb.shape[0] == g_in - dropped_boxes

    def losses(*frame):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        return model.forward_train(*frame, inp["mask_data"], inp["mask_anno"])

    on_device = losses(pts, metas, na_b, na_l, b, l)
    on_host = losses([host_pts.to(dev)], metas, [cnb], [cnl], [cb], [cl])
    assert set(on_device) == set(on_host) and len(on_device) >= 20
    differing = [k for k in sorted(on_host) if not torch.equal(bits(on_device[k].detach().float()), bits(on_host[k].detach().float()))]
    for k in differing:
        print(f"K40 end to end: {k}: device frame {float(on_device[k]):.9g} host frame {float(on_host[k]):.9g}")
    assert differing == []
