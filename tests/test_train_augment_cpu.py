"""Train-time augmentation on the host (K40, docs/kernels/K40_train_augment.md): the draws consume `np.random` in the reference's order,
`DeviceTrainAugment.from_pipeline` reads both reference train pipelines and refuses by name what is not built, the specification
functions the kernels are held to keep points inside their boxes (the sign conventions of points against boxes), are the identity where
they must be, filter objects as MyObjectRangeFilter does, and shuffle by a permutation; the C ABI surface and the static guard-band check
of the new wrapper module."""
import ast
import itertools
import os
import re

import numpy as np
import pytest
import torch

from fullysparsefusion_amd.mmdet3d_plugin.datasets import train_augment as ta
from fullysparsefusion_amd.mmdet3d_plugin.datasets.train_augment import (DeviceTrainAugment, augment_boxes_host, augment_points_host,
                                                                         draw_train_augmentation, shuffle_permutation_host, train_descriptor)
from fullysparsefusion_amd.mmdet3d_plugin.models.decode_heads.segmentation_head import points_in_boxes_first_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("FSF_REFERENCE_ROOT", "/root/reference")

# the two parameter sets of the reference (configs/_base_/datasets/nuscenes_dataloader.py:78-91, AV2_dataloader.py:90-102), literally
NUS_RANGE = [-50, -50, -4.99, 50, 50, 2.99]
NUS_STEPS = [dict(type="SaveNoAugPoints"),
             dict(type="RandomFlip3D", sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
             dict(type="GlobalRotScaleTrans", rot_range=[-0.785, 0.785], scale_ratio_range=[0.9, 1.1], translation_std=[0.5, 0.5, 0.5]),
             dict(type="PointsRangeFilter", point_cloud_range=NUS_RANGE), dict(type="PointShuffle"), dict(type="NormalizePoints"),
             dict(type="MyObjectRangeFilter", point_cloud_range=NUS_RANGE)]
AV2_RANGE = [-204.8, -204.8, -3.2, 204.8, 204.8, 3.2]
AV2_STEPS = [dict(type="SaveNoAugPoints"),
             dict(type="RandomFlip3D", sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
             dict(type="GlobalRotScaleTrans", rot_range=[-0.78539816, 0.78539816], scale_ratio_range=[0.95, 1.05]),
             dict(type="PointsRangeFilter", point_cloud_range=AV2_RANGE), dict(type="MyObjectRangeFilter", point_cloud_range=AV2_RANGE),
             dict(type="PointShuffle")]


def bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32)


def aug_of(flip_h=False, flip_v=False, rot=0.0, scale=1.0, trans=(0.0, 0.0, 0.0), seed=-1):
    return dict(pcd_horizontal_flip=flip_h, pcd_vertical_flip=flip_v, pcd_rot_factor=rot, pcd_scale_factor=scale,
                pcd_trans=np.asarray(trans, dtype=np.float64), shuffle_seed=seed)


# ------------------------------------------------------------------------------------------------ draws
@pytest.mark.parametrize("seed", [0, 7, 12345])
def test_draws_consume_np_random_in_the_reference_order(seed):
    flip, rst = NUS_STEPS[1], NUS_STEPS[2]
    np.random.seed(seed)
    got = draw_train_augmentation(flip, rst)
    np.random.seed(seed)
    h = np.random.rand() < 0.5
    v = np.random.rand() < 0.5
    rot = np.random.uniform(-0.785, 0.785)
    scale = np.random.uniform(0.9, 1.1)
    trans = np.random.normal(scale=np.array([0.5, 0.5, 0.5], dtype=np.float32), size=3).T
    assert got["pcd_horizontal_flip"] is bool(h) and got["pcd_vertical_flip"] is bool(v)
    assert got["pcd_rot_factor"] == rot and got["pcd_scale_factor"] == scale and np.array_equal(got["pcd_trans"], trans)
    assert isinstance(got["shuffle_seed"], int) and 0 <= got["shuffle_seed"] < 2 ** 63
    assert got["shuffle_seed"] == int(np.random.randint(0, np.iinfo(np.int64).max, dtype=np.int64))  # drawn last
    # a RandomState is an `rng` too, and leaves the global stream alone
    state = np.random.get_state()[1].copy()
    again = draw_train_augmentation(flip, rst, np.random.RandomState(seed))
    assert again["pcd_rot_factor"] == rot and again["shuffle_seed"] == got["shuffle_seed"] and np.array_equal(np.random.get_state()[1], state)


def test_zero_flip_ratios_draw_nothing_and_zero_std_still_draws():
    rst = dict(rot_range=[-0.3, 0.3], scale_ratio_range=[0.95, 1.05])
    np.random.seed(3)
    got = draw_train_augmentation(dict(flip_ratio_bev_horizontal=0.0, flip_ratio_bev_vertical=0.0), rst)
    np.random.seed(3)
    rot, scale = np.random.uniform(-0.3, 0.3), np.random.uniform(0.95, 1.05)
    trans = np.random.normal(scale=np.zeros(3, dtype=np.float32), size=3)
    assert got["pcd_horizontal_flip"] is False and got["pcd_vertical_flip"] is False
    assert got["pcd_rot_factor"] == rot and got["pcd_scale_factor"] == scale and np.array_equal(got["pcd_trans"], trans) and not trans.any()
    assert got["shuffle_seed"] == int(np.random.randint(0, np.iinfo(np.int64).max, dtype=np.int64))
    # one ratio of 0: only the other flip draws
    np.random.seed(3)
    one = draw_train_augmentation(dict(flip_ratio_bev_horizontal=0.0, flip_ratio_bev_vertical=0.5), rst)
    np.random.seed(3)
    v = np.random.rand() < 0.5
    assert one["pcd_horizontal_flip"] is False and one["pcd_vertical_flip"] is bool(v) and one["pcd_rot_factor"] == np.random.uniform(-0.3, 0.3)
    # a scalar rot_range / translation_std as GlobalRotScaleTrans takes them
    np.random.seed(5)
    got = draw_train_augmentation({}, dict(rot_range=0.2, scale_ratio_range=[1.0, 1.0], translation_std=0.1))
    np.random.seed(5)
    assert got["pcd_rot_factor"] == np.random.uniform(-0.2, 0.2) and got["pcd_scale_factor"] == np.random.uniform(1.0, 1.0)


def test_descriptor_rounds_to_fp32():
    d = train_descriptor(aug_of(True, False, 0.3, 1.05, (0.1, -0.2, 0.3)))
    c, s = float(torch.cos(torch.tensor(np.float32(0.3)))), float(torch.sin(torch.tensor(np.float32(0.3))))
    assert len(d) == 10 and d[:2] == (c, s) and d[2] == float(np.float32(1.05)) and d[3] == float(np.float32(0.3))
    assert d[4:7] == (1.0, 1.0, 0.0) and d[7:] == tuple(float(np.float32(v)) for v in (0.1, -0.2, 0.3))
    assert train_descriptor(ta.IDENTITY) == (1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------ pipeline parsing
def check_nus(aug):
    assert aug.flip_cfg == dict(flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5)
    assert aug.rst_cfg == dict(rot_range=[-0.785, 0.785], scale_ratio_range=[0.9, 1.1], translation_std=[0.5, 0.5, 0.5])
    assert aug.point_cloud_range == [-50.0, -50.0, -4.99, 50.0, 50.0, 2.99] and aug.shuffle is True


def check_av2(aug):
    assert aug.flip_cfg == dict(flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5)
    assert aug.rst_cfg == dict(rot_range=[-0.78539816, 0.78539816], scale_ratio_range=[0.95, 1.05])
    assert aug.point_cloud_range == [-204.8, -204.8, -3.2, 204.8, 204.8, 3.2] and aug.shuffle is True


def test_from_pipeline_on_the_literal_parameter_sets():
    check_nus(DeviceTrainAugment.from_pipeline(NUS_STEPS))
    check_av2(DeviceTrainAugment.from_pipeline(AV2_STEPS))
    plain = DeviceTrainAugment.from_pipeline([s for s in AV2_STEPS if s["type"] not in ("PointShuffle", "GlobalRotScaleTrans")])
    assert plain.shuffle is False and plain.draw(np.random.RandomState(0))["shuffle_seed"] == -1
    assert plain.rst_cfg == dict(rot_range=[0.0, 0.0], scale_ratio_range=[1.0, 1.0], translation_std=[0, 0, 0])


@pytest.mark.parametrize("name,check", [("nuscenes_dataloader.py", check_nus), ("AV2_dataloader.py", check_av2)])
def test_from_pipeline_on_the_reference_dataloader_configs(name, check):
    path = os.path.join(REFERENCE, "projects", "configs", "_base_", "datasets", name)
    if not os.path.exists(path):
        pytest.skip("the reference tree is not on this machine")
    from fullysparsefusion_amd.compat import Config

    cfg = Config.fromfile(path)
    steps = [dict(s) for s in cfg.train_pipeline]
    assert [s["type"] for s in steps].count("SaveNoAugPoints") == 1
    check(DeviceTrainAugment.from_pipeline(steps))


def replaced(steps, typ, **kw):
    return [dict(s, **kw) if s["type"] == typ else s for s in steps]


@pytest.mark.parametrize("steps,word", [
    (replaced(NUS_STEPS, "RandomFlip3D", sync_2d=True), "sync_2d"),
    ([dict(type="MyRandomFlip3D", flip_ratio_bev_horizontal=0.5)] + NUS_STEPS[2:], "sync_2d"),  # (mmdet3d's default is True)
    (replaced(NUS_STEPS, "GlobalRotScaleTrans", shift_height=True), "shift_height"),
    (NUS_STEPS[:1] + [dict(type="ObjectSample", db_sampler=dict())] + NUS_STEPS[1:], "ObjectSample"),
    (NUS_STEPS[:1] + [dict(type="MyObjectSample", db_sampler=dict())] + NUS_STEPS[1:], "MyObjectSample"),
    (NUS_STEPS + [dict(type="ObjectNoise")], "ObjectNoise"),
    (replaced(NUS_STEPS, "MyObjectRangeFilter", point_cloud_range=[-40, -40, -4.99, 40, 40, 2.99]), r"MyObjectRangeFilter point_cloud_range=\[-40"),
    (replaced(NUS_STEPS, "MyObjectRangeFilter", point_cloud_range=[-40, -40, -4.99, 40, 40, 2.99]), r"PointsRangeFilter point_cloud_range=\[-50"),
    ([s for s in NUS_STEPS if s["type"] != "MyObjectRangeFilter"], "MyObjectRangeFilter"),
])
def test_from_pipeline_refuses_by_name_what_is_not_built(steps, word):
    with pytest.raises(NotImplementedError, match=word):
        DeviceTrainAugment.from_pipeline(steps)


def test_sync_2d_without_a_ratio_is_no_flip():
    aug = DeviceTrainAugment.from_pipeline(replaced(NUS_STEPS, "RandomFlip3D", sync_2d=True, flip_ratio_bev_horizontal=0.0, flip_ratio_bev_vertical=0.0))
    assert aug.flip_cfg == dict(flip_ratio_bev_horizontal=0.0, flip_ratio_bev_vertical=0.0)


# ------------------------------------------------------------------------------------------------ points against boxes
def boxes_with_points(seed=0, n_boxes=40, per_box=50):
    """Boxes far apart (no point lies in two) with random yaw and velocity, and points strictly inside each (the local frame of
    `points_in_boxes_first_host`: lx = sx cos a - sy sin a along l, ly = sx sin a + sy cos a along w, a = -yaw) at <= 0.8 of the half
    extents: fp32 rounding cannot move them across a face."""
    g = torch.Generator().manual_seed(seed)
    grid = torch.arange(n_boxes, dtype=torch.float32)
    boxes = torch.zeros(n_boxes, 9)
    boxes[:, 0] = (grid % 8 - 3.5) * 9.0 + torch.rand(n_boxes, generator=g)
    boxes[:, 1] = (torch.div(grid, 8, rounding_mode="floor") - 2.0) * 9.0 + torch.rand(n_boxes, generator=g)
    boxes[:, 2] = torch.rand(n_boxes, generator=g) * 2 - 2.0
    boxes[:, 3:6] = torch.rand(n_boxes, 3, generator=g) * 2.5 + 0.5
    boxes[:, 6] = (torch.rand(n_boxes, generator=g) * 2 - 1) * 3.1
    boxes[:, 7:] = torch.randn(n_boxes, 2, generator=g)
    local = (torch.rand(n_boxes, per_box, 3, generator=g) * 2 - 1) * 0.8
    lx, ly = local[..., 0] * (boxes[:, 4:5] * 0.5), local[..., 1] * (boxes[:, 3:4] * 0.5)
    a = -boxes[:, 6:7]
    sx, sy = lx * torch.cos(a) + ly * torch.sin(a), -lx * torch.sin(a) + ly * torch.cos(a)  # the local frame inverted
    z = boxes[:, 2:3] + boxes[:, 5:6] * 0.5 + local[..., 2] * (boxes[:, 5:6] * 0.5)
    pts = torch.stack([boxes[:, 0:1] + sx, boxes[:, 1:2] + sy, z], -1).reshape(-1, 3)
    owner = torch.arange(n_boxes).repeat_interleave(per_box)
    return boxes, pts, owner


DESCRIPTORS = list(itertools.product((False, True), (False, True), (0.0, 0.3, -0.785), (0.9, 1.0, 1.1), ((0.0, 0.0, 0.0), (0.5, -0.3, 0.2))))


def test_points_in_boxes_first_host_names_the_same_box_through_every_descriptor():
    """Every flip pair x rotation x scale x translation keeps each of the 2000 points in its box under `points_in_boxes_first_host`, the
    containment test every GT consumer of `FSF.forward_train` applies (csrc/box_contain.h): the sign conventions of the points' and the
    boxes' specification agree.  That frame turns counter-clockwise with yaw, so a counter-clockwise scene rotation by theta takes a GT
    box's yaw to yaw + theta (with yaw - theta, K33's rule for the RoI pooling frame, theta = 0.3 misnamed 10.9 - 11.3 % of the points
    and theta = -0.785 20.9 %)."""
    boxes, pts, owner = boxes_with_points()
    assert torch.equal(points_in_boxes_first_host(pts, boxes[:, :7]), owner)
    labels = torch.arange(boxes.shape[0])
    wide = [-1e4, -1e4, -1e4, 1e4, 1e4, 1e4]
    cloud = torch.cat([pts, torch.rand(pts.shape[0], 2), pts], 1)  # xyz | features | the no-aug xyz
    assert len(DESCRIPTORS) == 72
    for fh, fv, rot, scale, t in DESCRIPTORS:
        aug = aug_of(fh, fv, rot, scale, t)
        p, order = augment_points_host(cloud, aug, wide)
        b = augment_boxes_host(boxes, labels, boxes, labels, aug, wide)["in_place"][0]
        assert torch.equal(order, torch.arange(pts.shape[0])) and torch.equal(bits(p[:, 3:]), bits(cloud[:, 3:]))
        named = points_in_boxes_first_host(p[:, :3], b[:, :7])
        assert torch.equal(named, owner), ((fh, fv, rot, scale, t), float((named != owner).float().mean()))


def test_identity_and_double_flips_return_the_input_bits():
    boxes, pts, _ = boxes_with_points(seed=1, n_boxes=16, per_box=8)
    boxes[:, 6] = boxes[:, 6].clamp(-3.0, 3.0)  # inside [-pi, pi): the wrap leaves it alone
    labels = torch.arange(16)
    wide = [-1e4, -1e4, -1e4, 1e4, 1e4, 1e4]
    cloud = torch.cat([pts, torch.rand(pts.shape[0], 5)], 1)
    p, _ = augment_points_host(cloud, ta.IDENTITY, wide)
    assert torch.equal(bits(p), bits(cloud))
    out = augment_boxes_host(boxes, labels, boxes, labels, ta.IDENTITY, wide)
    for got, want in zip(out["in_place"], (boxes, labels, boxes, labels)):
        assert torch.equal(got, want) and (got.dtype != torch.float32 or torch.equal(bits(got), bits(want)))
    for fh, fv in ((True, False), (False, True), (True, True)):
        aug = aug_of(fh, fv)
        twice, _ = augment_points_host(augment_points_host(cloud, aug, wide)[0], aug, wide)
        assert torch.equal(bits(twice), bits(cloud)), (fh, fv)
    # boxes: x, y, velocity return exactly; yaw returns through -(-yaw + pi) + pi and two wraps.  Per application at most two roundings
    # of values below 2 pi (the sum with pi, the wrap's difference; k * period is exact for |k| <= 1), each <= half an ulp of [4, 8) =
    # 2.4e-7, and each wrap by fp32(2 pi) is off the true period by 1.75e-7: 4 * 2.4e-7 + 2 * 1.75e-7 = 1.31e-6
    for fh, fv in ((True, False), (False, True), (True, True)):
        aug = aug_of(fh, fv)
        once = augment_boxes_host(boxes, labels, boxes, labels, aug, wide)["in_place"][0]
        twice = augment_boxes_host(once, labels, boxes, labels, aug, wide)["in_place"][0]
        keep = [0, 1, 2, 3, 4, 5, 7, 8]
        assert torch.equal(bits(twice[:, keep]), bits(boxes[:, keep])), (fh, fv)
        d = (twice[:, 6] - boxes[:, 6]).abs()
        assert float(torch.minimum(d, (d - 2 * np.pi).abs()).max()) <= 1.31e-6, (fh, fv)


# ------------------------------------------------------------------------------------------------ object filter
def test_object_filter_is_strict_masks_the_no_aug_lists_and_wraps_yaw():
    rng = [-50, -50, -5, 50, 50, 3]
    boxes = torch.tensor([[10.0, 5.0, -1.0, 2.0, 4.0, 1.5, 0.3, 1.0, 0.0],
                          [49.5, 0.0, -1.0, 2.0, 4.0, 1.5, 4.0, 0.0, 1.0],      # x + 0.5 == 50 exactly: dropped (strict)
                          [49.4999, 0.0, -1.0, 2.0, 4.0, 1.5, -4.0, 0.0, 1.0],  # just inside
                          [0.0, -50.5, -1.0, 2.0, 4.0, 1.5, 9.0, 0.0, 0.0],     # y + 0.5 == -50 exactly: dropped
                          [0.0, 60.0, 100.0, 2.0, 4.0, 1.5, 0.0, 0.0, 0.0],     # far out in y
                          [3.0, 3.0, 100.0, 2.0, 4.0, 1.5, -3.2, 0.0, 0.0]])    # z is not tested (BEV)
    labels = torch.tensor([3, 1, 4, 1, 5, -1])
    no_aug = boxes + 0.25
    no_aug[:, 6] = torch.tensor([7.0, -7.0, 3.5, 0.1, -0.1, 12.0])
    aug = aug_of(trans=(0.5, 0.5, 0.0))
    assert float(np.float32(49.5) + np.float32(0.5)) == 50.0 and float(np.float32(-50.5) + np.float32(0.5)) == -50.0
    out = augment_boxes_host(boxes, labels, no_aug, labels, aug, rng)
    assert out["keep"].tolist() == [True, False, True, False, False, True]
    b, l, nb, nl = out["in_place"]
    assert l.tolist() == [3, -1, 4, -1, -1, -1] and nl.tolist() == [3, -1, 4, -1, -1, -1]  # (the last: an input label < 0 stays)
    cb, cl, cnb, cnl = out["compact"]
    keep = out["keep"]
    assert cl.tolist() == [3, 4, -1] and cnl.tolist() == [3, 4, -1]
    for compact, full in ((cb, b), (cnb, nb)):  # the compacted form and the -1 form agree row for row
        assert torch.equal(bits(compact), bits(full[keep]))
    for yaw in (b[:, 6], nb[:, 6]):
        assert bool(((yaw >= -np.pi - 1e-6) & (yaw < np.pi)).all()), yaw
    assert torch.equal(b[:, 6][[0]], boxes[:, 6][[0]])  # inside the period: untouched
    want = torch.tensor([4.0 - 2 * np.pi, -4.0 + 2 * np.pi, 9.0 - 2 * np.pi, -3.2 + 2 * np.pi], dtype=torch.float64)
    assert torch.allclose(b[[1, 2, 3, 5], 6].double(), want, atol=2e-6, rtol=0)
    assert torch.allclose(nb[:, 6].double(), torch.tensor([7 - 2 * np.pi, -7 + 2 * np.pi, 3.5 - 2 * np.pi, 0.1, -0.1, 12 - 4 * np.pi],
                                                              dtype=torch.float64), atol=2e-6, rtol=0)
    # everything else of the no-aug rows is untouched
    cols = [0, 1, 2, 3, 4, 5, 7, 8]
    assert torch.equal(bits(nb[:, cols]), bits(no_aug[:, cols]))
    # no boxes at all
    empty = augment_boxes_host(torch.zeros(0, 7), torch.zeros(0, dtype=torch.long), torch.zeros(0, 7), torch.zeros(0, dtype=torch.long), aug, rng)
    assert empty["compact"][0].shape == (0, 7) and empty["in_place"][1].shape == (0,)


def test_points_filter_is_strict_and_drops_nan():
    rng = [-50, -50, -5, 50, 50, 3]
    pts = torch.tensor([[49.5, 0.0, 0.0, 1.0], [49.4999, 0.0, 0.0, 2.0], [0.0, 0.0, 2.5, 3.0], [0.0, 0.0, 2.4999, 4.0],
                        [float("nan"), 0.0, 0.0, 5.0], [0.0, 0.0, float("nan"), 6.0], [-50.5, 0.0, 0.0, 7.0], [1.0, 1.0, 1.0, 8.0]])
    out, order = augment_points_host(pts, aug_of(trans=(0.5, 0.0, 0.5)), rng)
    assert order.tolist() == [1, 3, 7] and out[:, 3].tolist() == [2.0, 4.0, 8.0]


# ------------------------------------------------------------------------------------------------ shuffle
@pytest.mark.parametrize("n", [0, 1, 2, 2047, 2048, 2049, 10245])
def test_shuffle_is_a_permutation_keyed_by_the_seed(n):
    perm = shuffle_permutation_host(n, 1234567)
    assert perm.dtype == np.int64 and perm.shape == (n,) and np.array_equal(np.sort(perm), np.arange(n))
    assert np.array_equal(perm, shuffle_permutation_host(n, 1234567))
    if n >= 2047:
        assert not np.array_equal(perm, shuffle_permutation_host(n, 1234568))
        assert not np.array_equal(perm, shuffle_permutation_host(n, 1234567 + (1 << 32)))  # the seed's high half counts
        keys = ta.shuffle_keys_host(n, 1234567)
        assert keys.min() >= 0 and keys.max() < 2 ** 31 and np.all(np.diff(keys[perm]) >= 0)


def test_shuffle_moves_nearly_every_row():
    for seed in range(8):
        perm = shuffle_permutation_host(4096, seed)
        fixed = int((perm == np.arange(4096)).sum())
        print(f"seed {seed}: {fixed} fixed points of 4096")
        assert fixed <= 8, (seed, fixed)


def test_shuffled_survivors_are_the_permutation_restricted_to_them():
    g = torch.Generator().manual_seed(2)
    pts = torch.cat([(torch.rand(3000, 3, generator=g) * 2 - 1) * 60, torch.rand(3000, 2, generator=g)], 1)
    rng = [-50, -50, -50, 50, 50, 50]
    plain, src = augment_points_host(pts, aug_of(rot=0.3, scale=0.95), rng)
    shuffled, order = augment_points_host(pts, aug_of(rot=0.3, scale=0.95, seed=99), rng)
    assert 0 < src.numel() < 3000 and torch.equal(src, torch.sort(src).values)
    perm = torch.from_numpy(shuffle_permutation_host(3000, 99))
    keep = torch.zeros(3000, dtype=torch.bool)
    keep[src] = True
    assert torch.equal(order, perm[keep[perm]]) and torch.equal(torch.sort(order).values, src)
    back = torch.argsort(order)
    assert torch.equal(bits(shuffled[back]), bits(plain))


# ------------------------------------------------------------------------------------------------ C ABI surface and guard-band cover
def test_entry_points_are_declared_documented_and_the_abi_version_stays():
    from fullysparsefusion_amd import _lib

    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for name in ("fsf_train_augment_points", "fsf_train_augment_points_workspace_bytes", "fsf_train_augment_boxes"):
        assert name in _lib.SIGNATURES and name in doc, name
    assert _lib.DEFINES["FSF_ABI_VERSION"] == 23
    assert _lib.DEFINES["FSF_TRAIN_AUGMENT_DESC_WORDS"] == 10 == len(train_descriptor(ta.IDENTITY)) and _lib.DEFINES["FSF_TRAIN_AUGMENT_MAX_BATCH"] == 32
    P, I32, I64 = _lib.c_p, _lib.c_i32, _lib.c_i64
    assert _lib.SIGNATURES["fsf_train_augment_points_workspace_bytes"] == ([I64], I64)
    assert _lib.SIGNATURES["fsf_train_augment_points"] == ([P, I64, I32, P, P, I64, P, P, P, P, I64, P], I32)  # the seed by value, as i64
    assert _lib.SIGNATURES["fsf_train_augment_boxes"] == ([P, I64, I32, P, P, I64, P, P, I32, P, P, P, P, P, P, P], I32)


_ALLOCATES = re.compile(r"torch\.empty|empty_like|torch\.zeros|torch\.full|_lib\.workspace\(|_workspace_bytes|_arena_bytes")
_SCRATCH = re.compile(r"_lib\.workspace\(|_workspace_bytes|_arena_bytes")


def test_every_allocating_wrapper_of_the_new_module_has_guard_band_cases():
    import test_guard_bands_augment_gpu as gb
    from fullysparsefusion_amd import hip_ops_augment

    with open(os.path.join(ROOT, "fullysparsefusion_amd", "hip_ops_augment.py")) as f:
        src = f.read()
    alloc, scratch = set(), set()
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef):
            body = ast.get_source_segment(src, node)
            if _ALLOCATES.search(body):
                alloc.add(node.name)
                if _SCRATCH.search(body):
                    scratch.add(node.name)
    assert alloc == {"train_augment_points", "train_augment_boxes"} and scratch == {"train_augment_points"}
    assert sorted(alloc - set(gb.CASES)) == []
    for name, cases in gb.CASES.items():
        assert hasattr(hip_ops_augment, name)
        kinds = [k for k, _ in cases]
        assert "ragged" in kinds and "minimal" in kinds and "empty" in kinds, name
    assert not re.search(r"torch\.zeros|torch\.full|empty_like|torch\.ones|new_zeros|new_empty|new_full", src)


def test_host_pipeline_classes_and_placeholders_are_left_refusing():
    from fullysparsefusion_amd.mmdet3d_plugin.registry import PIPELINES

    for typ in ("PointShuffle", "ObjectSample"):
        with pytest.raises(NotImplementedError):
            PIPELINES.build(dict(type=typ))(dict())
    assert "DeviceTrainAugment" not in PIPELINES.module_dict
