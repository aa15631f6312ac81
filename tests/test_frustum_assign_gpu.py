"""K38 on the device: `fsf_frustum_assign` (labels, targets, weights, assignment, source, stats) against the host restatement
`frustum_targets_host` bit for bit; `class_max_dist = NULL` against `fsf_hybrid_assign` bit for bit; the fused losses through it against
float64 autograd under K36's bounds (losses relative 1e-6, gradients 1e-7 absolute + 1e-5 of the largest float64 gradient); run-to-run
identity; no host synchronisation; and the whole detector with `refine_head_losses=True` and `forward_train` (K36's model tolerances:
1e-6 against float64, 1e-5 against the unfused path, gradients rtol 1e-3)."""
import ctypes

import numpy as np
import pytest
import torch

from fullysparsefusion_amd.mmdet3d_plugin.core.assigners import DistAssigner
from fullysparsefusion_amd.mmdet3d_plugin.models.dense_heads.cluster_heads import frustum_targets_host
from test_cluster_losses_cpu import NUS_CLASSES, reference_losses_f64
from test_frustum_assign_cpu import (C, FRUSTUM_CFG, RADII, dist_cfg, frustum_frame_case, frustum_targeted_cases, host_targets,
                                     make_frustum_assigner, make_refine_head, refine_head_loss, refine_loss_case, regroup_keep, source_of)
from test_hybrid_assign_cpu import ASSIGNER_CFG, LOSS_NAMES, targeted_cases

pytestmark = pytest.mark.gpu
SUFFIX = f"{NUS_CLASSES}"


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def counts_of(source):
    return np.bincount(np.asarray(source, np.int64), minlength=4).tolist()


def as_case(seed, box_dim=9):
    boxes, labels, aug, l2i, preds, centres, old = frustum_frame_case(seed, box_dim)
    return dict(centres=centres, bidx=np.zeros(len(centres), np.int64), preds=preds, old=old, na=[(boxes[:, :9], labels)], aug=[(aug, labels)],
                l2i=l2i[None], assigner={})


def want_of(c, code=10, **assigner):
    out = host_targets(make_frustum_assigner(**dict(c["assigner"], **assigner)), c["centres"], c["bidx"], c["preds"], c["na"], c["aug"], c["l2i"],
                       c["old"], code=code, parts=True)
    return out[:6], source_of(out[6], c["bidx"])


# ------------------------------------------------------------------------------------------------ through the head's get_targets
def device_targets(head, c, device, gt_on_device, strided):
    """modify_gt_for_single_task (both lists) + get_targets (K37a + K38) on device queries; the GT on the host (pinned uploads) or on
    the device (rows of label < 0 stay, last); the batch index as a column of the [n, 3] query table or on its own."""
    put = (lambda t: t.to(device)) if gt_on_device else (lambda t: t)
    lists = [[put(torch.from_numpy(np.asarray(b, np.float32))) for b, _ in c[key]] for key in ("na", "aug")]
    labs = [[put(torch.from_numpy(np.asarray(l, np.int64))) for _, l in c[key]] for key in ("na", "aug")]
    na = head.modify_gt_for_single_task(lists[0], labs[0], 0)
    au = head.modify_gt_for_single_task(lists[1], labs[1], 0)
    n = len(c["centres"])
    inds = torch.zeros((n, 3), dtype=torch.long)
    inds[:, 0] = torch.from_numpy(c["bidx"])
    inds = inds.to(device)
    metas = [dict(lidar2img=[m for m in l]) for l in c["l2i"]]
    head.task_info = {}
    out = head.get_targets(C, na[0], na[1], au[0], au[1], torch.from_numpy(c["preds"]).to(device), torch.from_numpy(c["centres"]).to(device),
                           inds if strided else inds[:, 0].contiguous(), task_id=0, img_metas_list=metas,
                           old_cls_logits=torch.from_numpy(c["old"]).to(device))
    info = head.task_info["0"]
    stats = [float(info[k]) for k in ("num_preds", "num_pos_preds", "num_gts", "assigned_gts")]
    last = head._last_assignment
    return list(out[:4]) + [last["assigned"], last["source"]], stats, last["avg_factors"].cpu().tolist(), last["source_counts"].cpu().tolist()


def assert_head_equals_host(c, device, name, code=10, **assigner):
    want, source = want_of(c, code, **assigner)
    cfg = dict(FRUSTUM_CFG, **dict(c["assigner"], **assigner))
    for gt_on_device in (False, True):
        for strided in (True, False):
            got, stats, avg, counts = device_targets(make_refine_head(assigner=cfg), c, device, gt_on_device, strided)
            lab, lw, tgt, wgt, asg, src = (t.cpu() for t in got)
            assert lab.dtype == torch.int64 and torch.equal(lab, want[0])
            assert torch.equal(lw, want[1])
            assert torch.equal(bits(tgt), bits(want[2])) and torch.equal(bits(wgt), bits(want[3]))  # bit for bit
            assert torch.equal(asg.long(), want[4])
            assert src.dtype == torch.int32 and src.tolist() == source.tolist()
            assert stats == want[5][:4].tolist() and avg == want[5][4:].tolist() and counts == counts_of(source)
    print(f"K38 {name}: n = {len(source)}, none / 3-D / 2-D / distance {counts_of(source)}")
    return want, source


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_targets_on_a_frame_equal_the_host_bit_for_bit(device, seed):
    want, source = assert_head_equals_host(as_case(seed), device, f"frame seed {seed}")
    assert min(counts_of(source)[1:]) >= 1 and counts_of(source)[3] >= 5


def test_targets_with_the_copy_paste_flag_equal_the_host(device):
    c = as_case(4, box_dim=10)
    assert c["aug"][0][0].shape[1] == 10
    want, source = assert_head_equals_host(c, device, "frame seed 4, copy-paste flags")
    by_dist = torch.from_numpy(source == 3)
    assert bool((want[3][by_dist][:, 8] == 0).any()) and bool((want[3][by_dist][:, 8] == 1).any())


@pytest.mark.parametrize("name", sorted(frustum_targeted_cases()))
def test_targeted_case_equals_the_host_bit_for_bit(device, name):
    c = frustum_targeted_cases()[name]
    want, source = assert_head_equals_host(c, device, name)
    assert want[4].tolist() == list(c["expect"]) and source.tolist() == list(c["source"])


def test_extra_height_grows_the_box_in_z_only_and_distance_takes_the_rest(device):
    e = 0.4
    box = np.array([[12.0, 3.0, -1.0, 2.0, 4.0, 1.6, 0.3, 0.5, -0.5]], np.float32)
    centres = [[12.0, 3.0, 0.6 + e - 0.01], [12.0, 3.0, 0.6 + e + 0.01], [12.0, 3.0, -1.0 - e + 0.01], [12.0, 3.0, -1.0 - e - 0.01],
               [12.0, 4.5, 0.6 + e + 0.01]]
    n = len(centres)
    preds = np.zeros((n, 9), np.float32)
    preds[:, :4] = [1500.0, 800.0, 1510.0, 810.0]
    old = np.full((n, C), -1.0, np.float32)
    old[:, 0] = 1.0
    c = dict(centres=np.array(centres, np.float32), bidx=np.zeros(n, np.int64), preds=preds, old=old, na=[(box, np.array([0]))],
             aug=[(box, np.array([0]))], l2i=targeted_cases()["no_gt"]["l2i"], assigner={})
    want, source = assert_head_equals_host(c, device, "extra_height 0.4", assigner_3d=dict(type="PointInBoxAssigner", extra_height=e))
    assert want[4].tolist() == [0, 0, 0, 0, -1] and source.tolist() == [1, 3, 1, 3, 0]
    plain, source = assert_head_equals_host(c, device, "extra_height 0")
    assert source.tolist() == [3, 3, 3, 3, 0]


def test_batch_of_two_frames_interleaved_plus_an_empty_sample(device):
    a, b = as_case(3), as_case(5)
    empty = (np.zeros((0, 9), np.float32), np.zeros(0, np.int64))
    c = dict(centres=np.concatenate([a["centres"], b["centres"]]), preds=np.concatenate([a["preds"], b["preds"]]),
             old=np.concatenate([a["old"], b["old"]]),
             bidx=np.concatenate([np.zeros(len(a["centres"]), np.int64), np.ones(len(b["centres"]), np.int64)]),
             na=a["na"] + b["na"] + [empty], aug=a["aug"] + b["aug"] + [empty], l2i=np.concatenate([a["l2i"], b["l2i"], a["l2i"]]), assigner={})
    perm = np.random.default_rng(0).permutation(len(c["bidx"]))  # the samples' queries interleaved
    for k in ("centres", "preds", "bidx", "old"):
        c[k] = np.ascontiguousarray(c[k][perm])
    c["bidx"][:7] = 2  # and a few queries of the sample without GT
    want, source = assert_head_equals_host(c, device, "batch of 2 + empty sample")
    assert min(counts_of(source)[1:]) >= 1 and (source[:7] == 0).all()


# ------------------------------------------------------------------------------------------------ the wrapper, called directly
def pack(lists, device):
    ptr = np.concatenate([[0], np.cumsum([len(l) for _, l in lists])])
    width = max([b.shape[1] for b, _ in lists if len(b)] or [9])
    rows = np.concatenate([np.asarray(b, np.float32).reshape(-1, width) for b, _ in lists])
    labels = np.concatenate([np.asarray(l, np.int64) for _, l in lists])
    return torch.tensor(ptr, dtype=torch.int32, device=device), torch.from_numpy(rows).to(device), torch.from_numpy(labels).int().to(device)


def direct(c, device, num_classes=C, code=10, radii=None, bidx="i64", wide_logits=False, extra_height=0.0, hybrid=False,
           regroup=regroup_keep):
    """`hip_ops_frustum.frustum_assign` (or `hip_ops_assign.hybrid_assign`) on the case's regrouped GT, packed here."""
    from fullysparsefusion_amd import hip_ops_assign, hip_ops_frustum

    na_ptr, na_rows, na_labels = pack([regroup(b, l) for b, l in c["na"]], device)
    ptr, rows, labels = pack([regroup(b, l) for b, l in c["aug"]], device)
    boxes_2d, keep = hip_ops_assign.gt_boxes_2d(na_rows[:, :7].contiguous(), na_labels, na_ptr, torch.from_numpy(np.asarray(c["l2i"])).float().to(device))
    n = len(c["centres"])
    xyz, preds = torch.from_numpy(c["centres"]).to(device), torch.from_numpy(c["preds"]).to(device)
    table = torch.zeros((n, 3), dtype=torch.int32 if bidx.startswith("i32") else torch.int64)
    table[:, 1] = torch.from_numpy(c["bidx"])
    table = table.to(device)
    batch = table[:, 1] if bidx.endswith("strided") else table[:, 1].contiguous()
    old = torch.from_numpy(c["old"]).to(device)
    if wide_logits:
        buf = torch.full((n, num_classes + 7), float("nan"), device=device)
        buf[:, 3:3 + num_classes] = old
        old = buf[:, 3:3 + num_classes]
    args = (xyz, batch, preds, na_ptr, boxes_2d, keep, ptr, rows, labels, num_classes, code, extra_height, 0.7, 0.3)
    if hybrid:
        return hip_ops_assign.hybrid_assign(*args)
    return hip_ops_frustum.frustum_assign(*args, old, None if radii is None else radii.to(device))


def assert_direct_equals_host(c, device, name, **kw):
    want, source = want_of(c)
    table = DistAssigner(**{k: v for k, v in dist_cfg().items() if k != "type"}).class_table(C)
    lab, tgt, wgt, asg, src, stats = (t.cpu() for t in direct(c, device, radii=table, **kw))
    assert torch.equal(lab, want[0]) and torch.equal(bits(tgt), bits(want[2])) and torch.equal(bits(wgt), bits(want[3]))
    assert torch.equal(asg.long(), want[4]) and src.tolist() == source.tolist() and torch.equal(bits(stats), bits(want[5]))
    print(f"K38 {name}: n = {len(source)}, none / 3-D / 2-D / distance {counts_of(source)}")
    return source


@pytest.mark.parametrize("bidx", ["i64", "i64_strided", "i32", "i32_strided"])
def test_batch_index_forms_and_logits_as_a_column_view(device, bidx):
    source = assert_direct_equals_host(as_case(4), device, f"frame seed 4, batch index {bidx}, logits a column view", bidx=bidx, wide_logits=True)
    assert min(counts_of(source)[1:]) >= 1


def big_case(n):
    """Frame 3's queries repeated with a jitter up to n rows: several workgroups with a partial last one."""
    c = as_case(3)
    m = len(c["centres"])
    idx = np.arange(n) % m
    rng = np.random.default_rng(77)
    out = dict(c, centres=(c["centres"][idx] + rng.normal(0, 0.05, (n, 3)).astype(np.float32) * (np.arange(n) >= m)[:, None]).astype(np.float32),
               preds=c["preds"][idx].copy(), old=c["old"][idx].copy(), bidx=np.zeros(n, np.int64))
    return out


@pytest.mark.parametrize("n", [1009, 1, 0])
def test_query_counts_across_and_below_a_workgroup(device, n):
    source = assert_direct_equals_host(big_case(n), device, f"n = {n}")
    if n == 1009:
        assert min(counts_of(source)[1:]) >= 20


def test_no_gt_at_all(device):
    c = as_case(5)
    empty = (np.zeros((0, 9), np.float32), np.zeros(0, np.int64))
    c.update(na=[empty], aug=[empty])
    source = assert_direct_equals_host(c, device, "no GT")
    assert counts_of(source)[0] == len(source)
    assert_head_equals_host(c, device, "no GT, through the head")


def test_code_8_with_26_classes(device):
    """The Argoverse 2 form: 7-column boxes, code size 8, 26 classes, each with its own radius."""
    from fullysparsefusion_amd.mmdet3d_plugin.core.assigners import FrustumAssigner

    names = [f"class_{k}" for k in range(26)]
    radii = {n: 0.25 * (k % 5) for k, n in enumerate(names)}
    c = as_case(3)
    rng = np.random.default_rng(5)
    spread = rng.integers(0, 3, len(c["aug"][0][1]))  # labels 0..9 -> 0..25, the same for both lists
    base = c["aug"][0][1]
    labels = np.where((base >= 0) & (base < 6), base + 10 * spread, base)

    def regroup26(b, l):
        order = np.argsort(np.where(l < 0, 26, l), kind="stable")
        return b[order], l[order]

    old = rng.normal(0, 1, (len(c["centres"]), 26)).astype(np.float32)
    near = np.flatnonzero(c["old"].max(1) == 6.0)  # the queries the frame moved next to a GT centre: they name the nearest row's class
    valid = labels >= 0
    d = np.linalg.norm(c["centres"][near, None, :2] - c["aug"][0][0][valid][None, :, :2], axis=2)
    old[near, labels[valid][d.argmin(1)]] = 9.0
    c.update(na=[(c["na"][0][0][:, :7], labels)], aug=[(c["aug"][0][0][:, :7], labels)], old=old)
    cfg = {k: v for k, v in ASSIGNER_CFG.items() if k != "type"}
    cfg.update(class_names=names, tasks=[dict(class_names=names)], assigner_dist=dict(
        type="DistAssigner", assign_tasks=[dict(class_names=[n]) for n in names], max_dist=[[radii[n]] for n in names], class_names=names))
    assigner = FrustumAssigner(**cfg)

    na, au = regroup26(*c["na"][0]), regroup26(*c["aug"][0])
    want = frustum_targets_host(assigner, torch.from_numpy(c["centres"]), torch.from_numpy(c["bidx"]), torch.from_numpy(c["preds"]),
                                [torch.from_numpy(na[0])], [torch.from_numpy(na[1])], [torch.from_numpy(au[0])], [torch.from_numpy(au[1])],
                                torch.from_numpy(c["l2i"]).float(), 26, 8, old_cls_logits=torch.from_numpy(old), return_parts=True)
    source = want[6][0]["source"].numpy()
    lab, tgt, wgt, asg, src, stats = (t.cpu() for t in direct(c, device, num_classes=26, code=8, radii=assigner.assigner_dist.class_table(26),
                                                              regroup=regroup26))
    print(f"K38 code 8 / 26 classes: n = {len(source)}, none / 3-D / 2-D / distance {counts_of(source)}")
    assert tgt.shape[1] == 8 and torch.equal(lab, want[0]) and torch.equal(bits(tgt), bits(want[2])) and torch.equal(bits(wgt), bits(want[3]))
    assert torch.equal(asg.long(), want[4]) and src.tolist() == source.tolist() and torch.equal(bits(stats), bits(want[5]))
    assert min(counts_of(source)[1:]) >= 1 and int(lab[lab < 26].max()) >= 10


def test_null_table_equals_hybrid_assign_bit_for_bit(device):
    for c in (as_case(3), big_case(1009), big_case(0)):
        got = direct(c, device, radii=None)
        want = direct(c, device, hybrid=True)
        for a, b in zip(got[:4] + (got[5],), want):
            assert a.dtype == b.dtype and torch.equal(bits(a), bits(b))
        src = got[4].cpu().numpy()
        assert counts_of(src)[3] == 0 and np.array_equal(src > 0, want[3].cpu().numpy() >= 0)


def test_bad_query_data_leaves_every_index_in_range(device):
    """Batch indices outside [0, B) and rows of NaN logits: such queries stay background / take class 0, nothing is read out of range."""
    c = as_case(5)
    n = len(c["centres"])
    c["bidx"][::7] = 3
    c["bidx"][3::11] = -2
    c["old"][::5] = np.nan
    source = assert_direct_equals_host(c, device, "bad batch indices and NaN logits")
    bad = (c["bidx"] < 0) | (c["bidx"] > 0)
    assert (source[bad] == 0).all() and counts_of(source)[3] >= 1
    lab, tgt, wgt, asg, src, stats = direct(c, device, radii=torch.tensor([RADII[k] for k in NUS_CLASSES]))
    assert int(lab.min()) >= 0 and int(lab.max()) <= C and int(asg.min()) >= -1 and int(asg.max()) < 41 and n == lab.numel()


def test_invalid_arguments_are_refused(device):
    """A table without logits, or with a logits stride below the class count, is FSF_ERR_INVALID_ARG; nothing is launched."""
    from fullysparsefusion_amd import _lib

    h = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    null = ctypes.c_void_p(None)
    n = 4
    f = lambda *s: torch.zeros(s, device=device)  # noqa: E731
    i = lambda *s: torch.zeros(s, dtype=torch.int32, device=device)  # noqa: E731
    xyz, bidx, preds, ptr, table, old = f(n, 3), i(n), f(n, 7), i(2), f(C), f(n, C)
    labels, tgt, wgt, asg, stats = torch.zeros(n, dtype=torch.int64, device=device), f(n, 10), f(n, 10), i(n), f(6)
    ws = torch.zeros(int(h.fsf_frustum_assign_workspace_bytes(0, 0, 6, n)), dtype=torch.uint8, device=device)

    def call(logits, stride, radii):
        return h.fsf_frustum_assign(p(xyz), n, 3, p(bidx), 4, 1, p(preds), 7, p(ptr), null, null, 0, 6, p(ptr), 1, null, 0, 9, 9, null, C, 10, 0.0,
                                    0.7, 0.3, logits, stride, radii, p(ws), ws.numel(), p(labels), p(tgt), p(wgt), p(asg), null, p(stats),
                                    _lib.stream_ptr())

    invalid = _lib.DEFINES["FSF_ERR_INVALID_ARG"]
    assert call(null, C, p(table)) == invalid
    assert call(p(old), C - 1, p(table)) == invalid
    assert call(p(old), C, p(table)) == 0 and call(null, 0, null) == 0
    torch.cuda.synchronize()
    assert labels.tolist() == [C] * n and asg.tolist() == [-1] * n


# ------------------------------------------------------------------------------------------------ losses
def test_fused_losses_match_float64_autograd(device):
    c = refine_loss_case()
    head = make_refine_head().to(device)
    n = len(c["z"])
    buf = torch.zeros((n, 23))
    buf[:, 1:11], buf[:, 12:22] = c["z"], c["r"]
    buf = buf.to(device).requires_grad_()
    z, r = buf[:, 1:11], buf[:, 12:22]  # column views of one buffer: their own row strides
    out = refine_head_loss(head, c, z, r, fused=True, dev=device)
    counts = head._last_assignment["source_counts"].tolist()
    boxes, labels, aug, l2i, preds, centres, old = c["raw"]
    lab, _, tgt, wgt, _, stats = host_targets(make_frustum_assigner(), centres, np.zeros(n, np.int64), preds, [(boxes, labels)], [(aug, labels)],
                                              l2i[None], old)
    grads = [1.0, 0.7, 1.3, 0.9, 1.1]
    want, gz, gr = reference_losses_f64(c["z"], c["r"], lab, tgt, wgt, 4.0, 0.25, [1.0, 0.5, 0.5, 0.2, 0.2], True, grads)
    g = torch.autograd.grad(sum(k * out[name + SUFFIX] for k, name in zip(grads, LOSS_NAMES)), buf)[0].cpu()
    figures = {name: abs(float(out[name + SUFFIX].detach()) - float(w)) / abs(float(w)) for name, w in zip(LOSS_NAMES, want)}
    e_cls, e_reg = float((g[:, 1:11].double() - gz).abs().max()), float((g[:, 12:22].double() - gr).abs().max())
    print(f"K38 fused n={n} positives={int(stats[1])} none / 3-D / 2-D / distance {counts}: relative loss errors "
          + ", ".join(f"{k}={v:.3e}" for k, v in figures.items())
          + f"; grad errors cls {e_cls:.3e} (max |g| {float(gz.abs().max()):.3e}), reg {e_reg:.3e} (max |g| {float(gr.abs().max()):.3e})")
    assert counts[3] >= 5 and [float(out[k + SUFFIX]) for k in ("num_preds", "num_pos_preds", "num_gts", "assigned_gts")] == stats[:4].tolist()
    for name in LOSS_NAMES:
        assert figures[name] <= 1e-6, (name, figures[name])
    assert e_cls <= 1e-7 + 1e-5 * float(gz.abs().max()) and e_reg <= 1e-7 + 1e-5 * float(gr.abs().max())
    assert not g[:, 0].any() and not g[:, 11].any() and not g[:, 22].any()
    unfused = refine_head_loss(head, c, z, r, fused=False, dev=device)
    for name in LOSS_NAMES:
        a, b = float(out[name + SUFFIX].detach()), float(unfused[name + SUFFIX].detach())
        assert abs(a - b) <= 1e-5 * abs(b), name
    with pytest.raises(ValueError, match="old_cls_logits"):
        head.loss([z], [r], c["xyz"].to(device), c["inds"].to(device), c["na_b"], c["na_l"], c["gt_b"], c["gt_l"], c["preds"].to(device), c["metas"])


def test_fused_path_is_bit_identical_from_run_to_run_and_with_a_shared_pack(device):
    c = refine_loss_case(4)
    head = make_refine_head().to(device)
    z, r = c["z"].to(device).requires_grad_(), c["r"].to(device).requires_grad_()
    l2i = head._lidar2img_batch(c["metas"], device)
    packs = {0: head.gt_boxes_2d_pack(0, c["na_b"], c["na_l"], l2i, device)}
    runs = []
    for extra in ({}, {}, dict(boxes_2d_packs=packs)):
        out = refine_head_loss(head, c, z, r, fused=True, dev=device, **extra)
        vals = [out[k + SUFFIX] for k in LOSS_NAMES]
        gz, gr = torch.autograd.grad(sum(vals), (z, r))
        runs.append([v.detach().clone() for v in vals] + [gz, gr] + [out[k + SUFFIX].clone() for k in ("num_pos_preds", "assigned_gts")]
                    + [head._last_assignment["assigned"].clone(), head._last_assignment["source"].clone()])
    assert float(runs[0][-4]) >= 40
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(bits(a), bits(b))


def test_device_path_never_synchronises(device):
    c = refine_loss_case(5)
    head = make_refine_head().to(device)
    z, r = c["z"].to(device).requires_grad_(), c["r"].to(device).requires_grad_()
    xyz, inds, preds, old = c["xyz"].to(device), c["inds"].to(device), c["preds"].to(device), c["old"].to(device)
    host_gt = (c["na_b"], c["na_l"], c["gt_b"], c["gt_l"])
    dev_gt = tuple([t.to(device) for t in lst] for lst in host_gt)
    dev_metas = [dict(lidar2img=torch.from_numpy(np.stack(c["metas"][0]["lidar2img"])).to(device))]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # (from the head's first call on: the per-head tables are pinned, non-blocking uploads)
    try:
        for gts, metas in ((host_gt, c["metas"]), (dev_gt, dev_metas)):  # host GT + host matrices (pinned uploads), and all on the device
            out = head.loss([z], [r], xyz, inds, *gts, preds, metas, None, [old], None)
            sum(out[k + SUFFIX] for k in LOSS_NAMES).backward()
            counts = head._last_assignment["source_counts"]
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(z.grad).all() and torch.isfinite(r.grad).all() and int(counts[3]) >= 5


# ------------------------------------------------------------------------------------------------ through the model
@pytest.fixture(scope="module")
def train_graph(device):
    import bench

    torch.manual_seed(0)
    model = bench.build_model(device).train()
    _, inp = bench.make_inputs(1, 3, device, frames=1)
    torch.manual_seed(11)
    with torch.no_grad():
        out = model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"])
    centres = out["stage_centers"][0].detach().cpu()
    old = torch.cat([out["frustum_obj_result"]["cls_logits"][0], out["fsd_obj_result"]["cls_logits"][0]]).detach().cpu()
    names = model.frustum_refined_head[0].class_names
    radius = torch.tensor([RADII[n] for n in names])
    pred = old.argmax(1)
    usable = torch.nonzero(torch.isfinite(centres).all(1) & (radius[pred] > 0)).reshape(-1)
    assert usable.numel() >= 12, usable.numel()
    rows, labels = [], []
    for j, i in enumerate(usable[:: max(1, usable.numel() // 12)][:12].tolist()):
        x, y, z = centres[i].tolist()
        if j % 3 == 0:  # a box around the stage centre: 3-D containment
            rows.append([x, y, z - 0.75, 1.2, 1.8, 1.5, 0.3 * j, 0.1 * j, -0.05 * j])
            labels.append(j % 10)
        else:  # a box of the class the previous stage predicts, a fraction of its radius away and BELOW the centre: the distance step
            rows.append([x + 0.3 * float(radius[pred[i]]), y, z - 4.0, 1.0, 1.4, 1.5, 0.2 * j, 0.1, -0.2])
            labels.append(int(pred[i]))
    return model, inp, [torch.tensor(rows, dtype=torch.float32)], [torch.tensor(labels)], old


def graph(model, inp, gt_boxes, gt_labels, **flags):
    torch.manual_seed(11)
    return model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"], gt_bboxes_3d=gt_boxes,
                                     gt_labels_3d=gt_labels, no_aug_gt_bboxes_3d=gt_boxes, no_aug_gt_labels_3d=gt_labels, **flags)


def test_forward_train_graph_refine_head_losses_match_the_unfused_path(train_graph):
    model, inp, gt_boxes, gt_labels, old = train_graph
    model.zero_grad(set_to_none=True)
    out = graph(model, inp, gt_boxes, gt_labels, refine_head_losses=True)
    names = LOSS_NAMES + ["num_preds", "num_pos_preds", "num_gts", "assigned_gts"]
    head = model.frustum_refined_head[0]
    suffix = f"{head.tasks[0]['class_names']}"
    assert set(out["losses"]) == {"loss_sem_seg", "loss_vote"} | {"stage_0_" + k + suffix for k in names}
    counts = head._last_assignment["source_counts"].tolist()
    res = out["stage_results"][0]
    # (the previous stage's logits of THIS run: the fixture's came from a no-grad forward, whose heads take other kernels)
    old_dev = [torch.cat([out["frustum_obj_result"]["cls_logits"][0], out["fsd_obj_result"]["cls_logits"][0]]).detach()]
    old = old_dev[0].cpu()
    args = (out["stage_centers"][0], out["obj_coors"], gt_boxes, gt_labels, gt_boxes, gt_labels, out["preds_2d"], inp["img_metas"], None, old_dev, None)
    host = head.loss(res["cls_logits"], res["reg_preds"], *args, fused=False)
    host_counts = head._last_assignment["source_counts"].tolist()
    print(f"K38 model: queries {sum(counts)}, none / 3-D / 2-D / distance fused {counts} unfused {host_counts}")
    assert counts == host_counts and counts[3] >= 1
    for k in names[5:]:
        assert float(out["losses"]["stage_0_" + k + suffix]) == float(host[k + suffix]), k
    na = head.modify_gt_for_single_task(gt_boxes, gt_labels, 0)
    lab, _, tgt, wgt, _, _ = frustum_targets_host(head.assigner, out["stage_centers"][0].detach().cpu(), out["obj_coors"][:, 0].cpu(),
                                                  out["preds_2d"].cpu(), na[0], na[1], na[0], na[1],
                                                  inp["img_metas"][0]["lidar2img"].cpu()[None], 10, 10, old_cls_logits=old)
    want, _, _ = reference_losses_f64(res["cls_logits"][0].cpu(), res["reg_preds"][0].cpu(), lab, tgt, wgt, 4.0, 0.25, [2.0, 0.5, 0.5, 0.2, 0.2], True)
    for k, w in zip(LOSS_NAMES, want):
        a, b = float(out["losses"]["stage_0_" + k + suffix].detach()), float(host[k + suffix].detach())
        print(f"K38 model {k}: fused {a:.9g} unfused {b:.9g} float64 {float(w):.12g}")
        assert abs(a - float(w)) <= 1e-6 * abs(float(w)), k
        assert abs(a - b) <= 1e-5 * abs(b), k
    params = [(n, p) for n, p in model.named_parameters() if p.requires_grad and n.startswith("frustum_refined_head.")]
    assert any(".task_heads.0.vel" in n for n, _ in params) and any("shared_mlp" in n for n, _ in params)
    fused = torch.autograd.grad(sum(out["losses"]["stage_0_" + k + suffix] for k in LOSS_NAMES), [p for _, p in params], retain_graph=True,
                                allow_unused=True)
    ref = torch.autograd.grad(sum(host[k + suffix] for k in LOSS_NAMES), [p for _, p in params], allow_unused=True)
    missing = [n for (n, _), g in zip(params, fused) if g is None]
    assert missing == [], missing[:10]
    for (n, _), g, r in zip(params, fused, ref):
        assert torch.isfinite(g).all(), n
        assert torch.allclose(g, r, rtol=1e-3, atol=1e-6 * float(r.abs().max()) + 1e-9), (n, float((g - r).abs().max()))
    # the head's own part never waits for the device
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = head.loss([t.detach() for t in res["cls_logits"]], [t.detach() for t in res["reg_preds"]], *args)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    for k in LOSS_NAMES:
        assert torch.equal(again[k + suffix], out["losses"]["stage_0_" + k + suffix].detach()), k


def test_forward_train_returns_every_heads_losses_and_two_runs_agree(train_graph):
    model, inp, gt_boxes, gt_labels, _ = train_graph
    names = LOSS_NAMES + ["num_preds", "num_pos_preds", "num_gts", "assigned_gts"]
    suffix = f"{model.frustum_refined_head[0].tasks[0]['class_names']}"
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        losses = model.forward_train(inp["points"], inp["img_metas"], gt_boxes, gt_labels, gt_boxes, gt_labels, inp["mask_data"], inp["mask_anno"])
        assert set(losses) == {"loss_sem_seg", "loss_vote"} | {p + k + suffix for p in ("frustum_", "fsd_", "stage_0_") for k in names}
        sum(v for k, v in losses.items() if "loss" in k).backward()
        grads = [p.grad.clone() for n, p in model.named_parameters() if n.startswith("frustum_refined_head.") and p.grad is not None]
        runs.append(([losses[k].detach().clone() for k in sorted(losses)], grads))
    assert len(runs[0][1]) >= 10 and all(torch.isfinite(g).all() for g in runs[0][1])
    worst = max(float((a.double() - b.double()).abs().max()) for a, b in zip(runs[0][0], runs[1][0]))
    print(f"K38 forward_train: {len(runs[0][0])} entries, largest difference between two runs {worst:.3e}")
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(bits(a), bits(b))
    # host labels with a row of label -1, the boxes already on the device: the row is dropped by index, the losses are the same bits
    dev = runs[0][0][0].device
    more_boxes = [torch.cat([b, b[:1] + 1.0]).to(dev) for b in gt_boxes]
    more_labels = [torch.cat([l, l.new_tensor([-1])]) for l in gt_labels]
    torch.manual_seed(11)
    dropped = model.forward_train(inp["points"], inp["img_metas"], more_boxes, more_labels, more_boxes, more_labels, inp["mask_data"],
                                  inp["mask_anno"])
    for k, v in zip(sorted(dropped), runs[0][0]):
        assert torch.equal(bits(dropped[k].detach()), bits(v)), k
    all_flags = graph(model, inp, gt_boxes, gt_labels, lidar_head_losses=True, camera_head_losses=True, refine_head_losses=True)
    for k, v in zip(sorted(all_flags["losses"]), runs[0][0]):
        assert torch.equal(bits(all_flags["losses"][k].detach()), bits(v)), k


def test_forward_train_graph_without_the_flag_is_todays_output(train_graph):
    model, inp, gt_boxes, gt_labels, _ = train_graph
    plain = graph(model, inp, gt_boxes, gt_labels)
    assert set(plain["losses"]) == {"loss_sem_seg", "loss_vote"}
    flagged = graph(model, inp, gt_boxes, gt_labels, refine_head_losses=True)
    assert set(plain) == set(flagged) and len(flagged["losses"]) == 2 + 9
    for key in ("cls_logits", "reg_preds"):
        for a, b in zip(plain["stage_results"][0][key], flagged["stage_results"][0][key]):
            assert torch.equal(bits(a.detach()), bits(b.detach())), key
    assert torch.equal(bits(plain["stage_centers"][0].detach()), bits(flagged["stage_centers"][0].detach()))
    torch.manual_seed(11)
    bare = model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"])
    assert "losses" not in bare and set(bare) == set(plain) - {"losses"}
    with pytest.raises(ValueError, match="no_aug_gt_bboxes_3d"):
        model.forward_train_graph(inp["points"], inp["img_metas"], inp["mask_data"], inp["mask_anno"], gt_bboxes_3d=gt_boxes,
                                  gt_labels_3d=gt_labels, refine_head_losses=True)
