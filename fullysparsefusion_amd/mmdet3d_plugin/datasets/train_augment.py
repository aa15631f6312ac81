"""Train-time augmentation of the uploaded cloud and the GT boxes (K40, docs/kernels/K40_train_augment.md): what both reference train
pipelines run after SaveNoAugPoints (configs/_base_/datasets/nuscenes_dataloader.py:53-95, AV2_dataloader.py:73-105) —

    RandomFlip3D(sync_2d=False)       a random BEV flip                         [UNVENDORED mmdet3d]
    GlobalRotScaleTrans               a random global rotation, scale and translation (transforms_3d.py:59-170)
    PointsRangeFilter                 the strict range test on the augmented xyz
    PointShuffle                      a random order of the survivors           [UNVENDORED mmdet3d]
    MyObjectRangeFilter               GT boxes outside the BEV range dropped, yaw wrapped, the same mask on the no-aug lists
                                      (loading.py:367-408)

as three parts: the DRAWS, on the host, in the reference's order (`draw_train_augmentation`); the SPECIFICATION, plain torch / numpy with
every operation a separately rounded fp32 step (`augment_points_host`, `shuffle_permutation_host`, `augment_boxes_host`); and
`DeviceTrainAugment`, which runs the kernels of csrc/train_augment.hip on the whole batch and matches the specification bit for bit.
The host pipeline classes of pipelines.py and the placeholders of models/placeholders.py keep refusing the random forms: this module
stands beside the registry, not in it.
"""
import numpy as np
import torch

from .pipelines import augmentation_descriptor

TWO_PI = float(np.float32(2 * np.pi))  # limit_yaw's period as the fp32 operand it becomes
IDENTITY = dict(pcd_horizontal_flip=False, pcd_vertical_flip=False, pcd_rot_factor=0.0, pcd_scale_factor=1.0,
                pcd_trans=np.zeros(3), shuffle_seed=-1)


# ------------------------------------------------------------------------------------------------ draws
def draw_train_augmentation(flip_cfg, rst_cfg, rng=np.random):
    """One frame's draws in the reference's order, so that a seeded run consumes `np.random` as upstream does:
    rand() < flip_ratio_bev_horizontal, rand() < flip_ratio_bev_vertical (mmdet3d's RandomFlip3D with sync_2d=False, un-vendored; a ratio
    of 0 draws nothing), uniform(rot_range) (transforms_3d.py:90-92), uniform(scale_ratio_range) (:142-143), normal(scale=translation_std,
    size=3) (:70-71; drawn even when the std is 0, as upstream does), then — not upstream's — the shuffle's int64 seed with `randint`.
    Returns the keys the host classes record plus `shuffle_seed`."""
    ratio_h = float(flip_cfg.get("flip_ratio_bev_horizontal", 0.0))
    ratio_v = float(flip_cfg.get("flip_ratio_bev_vertical", 0.0))
    flip_h = bool(rng.rand() < ratio_h) if ratio_h else False
    flip_v = bool(rng.rand() < ratio_v) if ratio_v else False
    rot_range = rst_cfg.get("rot_range", [-0.78539816, 0.78539816])
    if not isinstance(rot_range, (list, tuple, np.ndarray)):
        rot_range = [-rot_range, rot_range]
    scale_range = rst_cfg.get("scale_ratio_range", [0.95, 1.05])
    std = rst_cfg.get("translation_std", [0, 0, 0])
    if not isinstance(std, (list, tuple, np.ndarray)):
        std = [std, std, std]
    rot = rng.uniform(rot_range[0], rot_range[1])
    scale = rng.uniform(scale_range[0], scale_range[1])
    trans = rng.normal(scale=np.array(std, dtype=np.float32), size=3).T
    seed = int(rng.randint(0, np.iinfo(np.int64).max, dtype=np.int64))
    return dict(pcd_horizontal_flip=flip_h, pcd_vertical_flip=flip_v, pcd_rot_factor=float(rot), pcd_scale_factor=float(scale),
                pcd_trans=trans, shuffle_seed=seed)


def train_descriptor(aug):
    """The 10 floats K40 takes per frame: `augmentation_descriptor`'s seven (cos, sin, scale = fp32(s), angle, rotate, flip_h, flip_v;
    cos / sin from `rotation_cos_sin`) and tx, ty, tz, each rounded to fp32 (`points.translate` adds an fp32 tensor)."""
    t = np.asarray(aug.get("pcd_trans", np.zeros(3)), dtype=np.float64).reshape(3)
    return augmentation_descriptor(aug.get("pcd_rot_factor", 0.0), aug.get("pcd_scale_factor", 1.0), aug.get("pcd_horizontal_flip", False),
                                   aug.get("pcd_vertical_flip", False)) + tuple(float(np.float32(v)) for v in t)


# ------------------------------------------------------------------------------------------------ specification
def _f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def _rotate(x, y, c, s):
    """`rotate_xyz_`'s arithmetic: two rounded products and one rounded sum per coordinate."""
    return (x * _f32(c)) - (y * _f32(s)), (x * _f32(s)) + (y * _f32(c))


def shuffle_keys_host(n, seed):
    """key_i = mix31(i, seed), the integer arithmetic of csrc/train_augment.hip::ta_mix31: murmur3's 32-bit finaliser over
    h = (i ^ seed_lo) + seed_hi * 0x9E3779B9 (mod 2^32), shifted right once to 31 bits."""
    seed = int(seed)
    assert seed >= 0
    m = np.uint64(0xFFFFFFFF)
    h = (np.arange(n, dtype=np.uint64) ^ np.uint64(seed & 0xFFFFFFFF)) + np.uint64(((seed >> 32) * 0x9E3779B9) & 0xFFFFFFFF)
    h &= m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return (h >> np.uint64(1)).astype(np.int64)


def shuffle_permutation_host(n, seed):
    """The shuffle's definition: the stable ascending sort of `shuffle_keys_host(n, seed)` (ties keep source order), i64 [n].  Output
    position j holds source row perm[j].  A deterministic, seed-keyed stand-in for PointShuffle's `torch.randperm`."""
    return np.argsort(shuffle_keys_host(n, seed), kind="stable").astype(np.int64)


def augment_points_host(points, aug, pc_range=None):
    """One frame's cloud f32 [n, C] -> the augmented, range-filtered, shuffled cloud, per row in the train pipeline's order: H flip
    y -> -y, V flip x -> -x, rotation x' = x c - y s, y' = x s + y c (not evaluated for an angle of exactly 0), xyz *= fp32(scale),
    xyz += fp32(t), the strict in-range test on the result (a NaN coordinate fails it).  Columns 3 and up are copied unchanged.  The
    order: with aug['shuffle_seed'] >= 0 the rows of `shuffle_permutation_host(n, seed)` that survive, else the survivors in source
    order.  Returns (rows f32 [count, C], their source row indices i64 [count])."""
    c, s, scale, _, rot, flip_h, flip_v, tx, ty, tz = train_descriptor(aug)
    p = torch.as_tensor(points, dtype=torch.float32).clone()
    x, y, z = p[:, 0].clone(), p[:, 1].clone(), p[:, 2].clone()
    if flip_h:
        y = -y
    if flip_v:
        x = -x
    if rot:
        x, y = _rotate(x, y, c, s)
    x, y, z = x * _f32(scale) + _f32(tx), y * _f32(scale) + _f32(ty), z * _f32(scale) + _f32(tz)
    p[:, 0], p[:, 1], p[:, 2] = x, y, z
    keep = torch.ones(p.shape[0], dtype=torch.bool)
    if pc_range is not None:
        r = [_f32(v) for v in pc_range]
        keep = (x > r[0]) & (y > r[1]) & (z > r[2]) & (x < r[3]) & (y < r[4]) & (z < r[5])
    seed = int(aug.get("shuffle_seed", -1))
    order = torch.from_numpy(shuffle_permutation_host(p.shape[0], seed)) if seed >= 0 else torch.arange(p.shape[0])
    order = order[keep[order]]
    return p[order], order


def limit_yaw_host(yaw):
    """mmdet3d's `limit_yaw(offset=0.5, period=2 * np.pi)` = `limit_period` (un-vendored), v - floor(v / period + 0.5) * period, with each
    step pinned as an fp32 operation: the quotient by fp32(2 pi) (a true division), the sum with 0.5, the floor, the product with
    fp32(2 pi), the difference."""
    period = _f32(TWO_PI)
    return yaw - (torch.floor((yaw / period) + _f32(0.5)) * period)


def augment_boxes_host(boxes, labels, no_aug_boxes, no_aug_labels, aug, pc_range):
    """One sample's GT rows f32 [G, 7 | 9] (x, y, z_bottom, w, l, h, yaw[, vx, vy]) through the flips (H: y, vy negated, yaw -> -yaw + pi;
    V: x, vx negated, yaw -> -yaw: mmdet3d's `tensor[:, 1::7]` / `[:, 0::7]` rule), the rotation of (x, y) and (vx, vy) by the points'
    formula with yaw -> yaw + angle (the frame of `points_in_boxes_first_host`, which every GT consumer of `forward_train` tests: the
    augmented points stay in the augmented boxes), the scale of every column but yaw, the translation of xyz, and
    MyObjectRangeFilter (loading.py:367-408): a box stays when its augmented (x, y) is strictly inside pc_range[[0, 1, 3, 4]], yaw is
    wrapped by `limit_yaw_host`, and the same mask and wrap land on the otherwise untouched no-aug lists.
    Returns dict(compact=(boxes, labels, no_aug_boxes, no_aug_labels) as the reference produces them, in_place=the same four with all G
    rows kept and the label of a dropped row set to -1 (labels already < 0 stay), keep=bool [G])."""
    c, s, scale, angle, rot, flip_h, flip_v, tx, ty, tz = train_descriptor(aug)
    b = torch.as_tensor(boxes, dtype=torch.float32).clone().reshape(-1, torch.as_tensor(boxes).shape[-1])
    na = torch.as_tensor(no_aug_boxes, dtype=torch.float32).clone().reshape(b.shape)
    lab, na_lab = torch.as_tensor(labels).long().reshape(-1).clone(), torch.as_tensor(no_aug_labels).long().reshape(-1).clone()
    vel = b.shape[1] >= 9
    if flip_h:
        b[:, 1] = -b[:, 1]
        if vel:
            b[:, 8] = -b[:, 8]
        b[:, 6] = -b[:, 6] + _f32(np.pi)
    if flip_v:
        b[:, 0] = -b[:, 0]
        if vel:
            b[:, 7] = -b[:, 7]
        b[:, 6] = -b[:, 6]
    if rot:
        b[:, 0], b[:, 1] = _rotate(b[:, 0].clone(), b[:, 1].clone(), c, s)
        if vel:
            b[:, 7], b[:, 8] = _rotate(b[:, 7].clone(), b[:, 8].clone(), c, s)
        b[:, 6] = b[:, 6] + _f32(angle)
    b[:, :6] = b[:, :6] * _f32(scale)
    b[:, 7:] = b[:, 7:] * _f32(scale)
    b[:, 0], b[:, 1], b[:, 2] = b[:, 0] + _f32(tx), b[:, 1] + _f32(ty), b[:, 2] + _f32(tz)
    r = [_f32(v) for v in pc_range]
    keep = (b[:, 0] > r[0]) & (b[:, 1] > r[1]) & (b[:, 0] < r[3]) & (b[:, 1] < r[4])
    b[:, 6] = limit_yaw_host(b[:, 6].clone())
    na[:, 6] = limit_yaw_host(na[:, 6].clone())
    minus = torch.full_like(lab, -1)
    in_place = (b, torch.where(keep | (lab < 0), lab, minus), na, torch.where(keep | (na_lab < 0), na_lab, minus))
    return dict(compact=(b[keep], lab[keep], na[keep], na_lab[keep]), in_place=in_place, keep=keep)


# ------------------------------------------------------------------------------------------------ the device path
_FLIP, _RST = ("RandomFlip3D", "MyRandomFlip3D"), ("GlobalRotScaleTrans", "MyGlobalRotScaleTrans")
_POINT_RANGE, _OBJECT_RANGE = ("PointsRangeFilter", "MyPointsRangeFilter"), ("ObjectRangeFilter", "MyObjectRangeFilter")
_REFUSED = ("ObjectSample", "MyObjectSample", "ObjectNoise")


class DeviceTrainAugment:
    """The train pipeline's augmentation steps on the device, for a whole batch.

    `points`: per-frame device clouds NOT yet range-filtered — a `DevicePointAssembler` whose output feeds this class must be constructed
    with `point_cloud_range=None`: the range test belongs on the augmented xyz (its own `augmentations=` branch notes the same);
    `NormalizePoints` touches no xyz column and commutes.  `gt_bboxes_3d` / `gt_labels_3d`: per-frame GT rows (LiDARInstance3DBoxes or
    [G, 7 | 9] tensors) and labels, on the host or the device.  One host wait per batch — the read of every frame's point count in one
    copy — and none for the boxes: a dropped box keeps its row and gets label -1, which every consumer of `FSF.forward_train` skips."""

    def __init__(self, flip_cfg=None, rst_cfg=None, point_cloud_range=None, shuffle=True):
        self.flip_cfg, self.rst_cfg = dict(flip_cfg or {}), dict(rst_cfg or {})
        if point_cloud_range is None:
            raise ValueError("DeviceTrainAugment needs point_cloud_range (PointsRangeFilter / MyObjectRangeFilter)")
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.shuffle = bool(shuffle)

    @classmethod
    def from_pipeline(cls, pipeline_dicts):
        """Reads the `type=` dicts of a reference train pipeline without building them: the flip ratios and `sync_2d` of RandomFlip3D /
        MyRandomFlip3D, the ranges of GlobalRotScaleTrans / MyGlobalRotScaleTrans, `point_cloud_range` of PointsRangeFilter and
        MyObjectRangeFilter, the presence of PointShuffle.  What is not built is refused by name."""
        flip, rst, prange, orange, shuffle = {}, None, None, None, False
        for step in pipeline_dicts:
            typ = step.get("type")
            if typ in _REFUSED:
                raise NotImplementedError(f"DeviceTrainAugment: {typ} is not built (GT paste / per-object noise are outside the device path)")
            if typ in _FLIP:
                ratios = (step.get("flip_ratio_bev_horizontal", 0.0), step.get("flip_ratio_bev_vertical", 0.0))
                if step.get("sync_2d", True) and any(ratios):
                    raise NotImplementedError(f"DeviceTrainAugment: {typ}(sync_2d=True) with a flip ratio is not built (the images are "
                                              "not augmented); the reference pipelines set sync_2d=False")
                flip = dict(flip_ratio_bev_horizontal=float(ratios[0]), flip_ratio_bev_vertical=float(ratios[1]))
            elif typ in _RST:
                if step.get("shift_height", False):
                    raise NotImplementedError(f"DeviceTrainAugment: {typ}(shift_height=True) is not built")
                rst = {k: step[k] for k in ("rot_range", "scale_ratio_range", "translation_std") if k in step}
            elif typ in _POINT_RANGE:
                prange = [float(v) for v in step["point_cloud_range"]]
            elif typ in _OBJECT_RANGE:
                orange = [float(v) for v in step["point_cloud_range"]]
            elif typ == "PointShuffle":
                shuffle = True
        if prange is None or orange is None:
            missing = "PointsRangeFilter" if prange is None else "MyObjectRangeFilter"
            raise NotImplementedError(f"DeviceTrainAugment: the pipeline has no {missing}; both range filters are part of the built path")
        if prange != orange:
            raise NotImplementedError(f"DeviceTrainAugment: differing ranges are not built: PointsRangeFilter point_cloud_range={prange}, "
                                      f"MyObjectRangeFilter point_cloud_range={orange}")
        if rst is None:
            rst = dict(rot_range=[0.0, 0.0], scale_ratio_range=[1.0, 1.0], translation_std=[0, 0, 0])
        return cls(flip, rst, prange, shuffle)

    def draw(self, rng=np.random):
        aug = draw_train_augmentation(self.flip_cfg, self.rst_cfg, rng)
        if not self.shuffle:
            aug["shuffle_seed"] = -1
        return aug

    def __call__(self, points, gt_bboxes_3d, gt_labels_3d, img_metas, rng=np.random):
        """-> (points, img_metas, no_aug_gt_bboxes_3d, no_aug_gt_labels_3d, gt_bboxes_3d, gt_labels_3d), the leading arguments of
        `FSF.forward_train`; each meta (a copy) records pcd_horizontal_flip, pcd_vertical_flip, pcd_rot_factor, pcd_scale_factor,
        pcd_trans and shuffle_seed.  The no-aug lists are the clone of the inputs (SaveNoAugPoints' rule) through the object filter."""
        from ... import hip_ops_augment
        from ..models.decode_heads.segmentation_head import gt_box_rows

        nb = len(points)
        assert len(gt_bboxes_3d) == nb and len(gt_labels_3d) == nb and len(img_metas) == nb and nb >= 1
        augs = [self.draw(rng) for _ in range(nb)]
        descs = [train_descriptor(a) for a in augs]
        dev = points[0].device
        counts = torch.empty((nb,), dtype=torch.int64, device=dev)
        clouds = [hip_ops_augment.train_augment_points(p, d, self.point_cloud_range, a.get("shuffle_seed", -1), counts[k:k + 1])[0]
                  for k, (p, d, a) in enumerate(zip(points, descs, augs))]
        rows = [gt_box_rows(b).to(dev, torch.float32, non_blocking=True) for b in gt_bboxes_3d]
        labels = [torch.as_tensor(l).reshape(-1).to(dev, torch.int64, non_blocking=True) for l in gt_labels_3d]
        sizes = [r.shape[0] for r in rows]
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64).tolist()
        boxes, labs = torch.cat(rows), torch.cat(labels)
        b_out, l_out, na_out, nal_out = hip_ops_augment.train_augment_boxes(boxes, labs, boxes, labs, offsets, descs, self.point_cloud_range)
        kept = counts.cpu().tolist()  # the batch's one host wait
        metas = []
        for meta, a in zip(img_metas, augs):
            meta = dict(meta)
            meta.update({k: a[k] for k in ("pcd_horizontal_flip", "pcd_vertical_flip", "pcd_rot_factor", "pcd_scale_factor", "pcd_trans",
                                           "shuffle_seed")})
            metas.append(meta)
        split = lambda t: list(torch.split(t, sizes))  # noqa: E731
        return [c[:k] for c, k in zip(clouds, kept)], metas, split(na_out), split(nal_out), split(b_out), split(l_out)
