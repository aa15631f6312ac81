"""GPU: the rotated BEV NMS (K20) on the box pairs where a polygon clip goes wrong — coincident, flipped, nested, edge- and
corner-sharing, crossed, axis-exact, tiny-in-huge, non-finite — through the all-pairs mask kernel (n < 1024), the cell-grid path
(n >= 1024) and its big list (radius > 4 m), with both boxes of a pair first.  Layouts, float64 reference and the derived tolerance:
tests/nms_degenerate_cases.py (checked on their own in tests/test_nms_degenerate_cpu.py)."""
import numpy as np
import pytest
import torch

import nms_degenerate_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(device):
    from fullysparsefusion_amd import hip_ops

    return hip_ops


def _kept_mask(ops, boxes, thresh):
    keep = ops.nms_bev(boxes, float(thresh), True)
    assert bool((keep[1:] > keep[:-1]).all())
    m = torch.zeros(boxes.size(0), dtype=torch.bool, device=boxes.device)
    m[keep] = True
    return m


@pytest.mark.parametrize("size", list(C.SIZES))
@pytest.mark.parametrize("family", C.FAMILIES)
def test_pair_probe_decisions_match_float64(ops, device, family, size):
    """Twenty thresholds x both orders: the first box of every pair and every pad is kept; the second box is kept where the float64
    IoU is below thresh - tol and dropped where it is above thresh + tol (in between it may go either way)."""
    lay = C.layout(family, size)
    k = lay["a"].shape[0]
    n = 2 * k + lay["pads"].shape[0]
    assert (n < 1024) == (size == "small")
    undecided = 0
    for order in ("ab", "ba"):
        boxes = torch.from_numpy(C.boxes_in_order(lay, order)).to(device)
        kept = torch.stack([_kept_mask(ops, boxes, t) for t in C.THRESHOLDS]).cpu().numpy()
        for row, t in zip(kept, C.THRESHOLDS):
            must_keep, must_drop, either = C.expected(lay, t)
            assert row[:k].all() and row[2 * k:].all(), (family, size, order, t)
            second = row[k:2 * k]
            wrong = (must_keep & ~second) | (must_drop & second)
            assert not wrong.any(), (family, size, order, t, np.nonzero(wrong)[0][:5], lay["iou"][wrong][:5], lay["tol"])
            undecided += int(either.sum())
    assert undecided <= C.MAX_UNDECIDED * 2 * k * len(C.THRESHOLDS)


@pytest.mark.parametrize("seed", range(8))
def test_identical_copies_suppress_their_copy(ops, device, seed):
    """4096 boxes and their exact copies (over the eight seeds 32 768 pairs: by the host count about ten of them clip to a polygon of
    more than eight vertices): the copy goes at every threshold, through the cell-grid path (n = 8192) and, in slices of 511 pairs,
    through the all-pairs mask kernel (n = 1022)."""
    a, tol = C.identical_layout(seed)
    assert tol < 1.0 - 0.999
    both = torch.from_numpy(np.concatenate([a, a])).to(device)
    for t in (0.05, 0.5, 0.999):
        assert torch.equal(ops.nms_bev(both, t, True).cpu(), torch.arange(4096))
    at = torch.from_numpy(a).to(device)
    for s in range(0, 4096, 511):
        part = at[s:s + 511]
        keep = ops.nms_bev(torch.cat([part, part]), 0.999, True)
        assert torch.equal(keep.cpu(), torch.arange(part.size(0))), (seed, s)


def _poison(box, kind):
    box = box.copy()
    if kind == "nan_yaw":
        box[4] = np.nan
    elif kind == "nan_coord":
        box[1] = np.nan
    elif kind == "inf_hi":
        box[2] = np.inf
    elif kind == "inf_lo":
        box[0] = -np.inf
    elif kind == "zero_width":
        box[2] = box[0]
    elif kind == "negative_width":
        box[0], box[2] = box[2], box[0]
    else:
        raise KeyError(kind)
    return box


@pytest.mark.parametrize("size", ["small", "grid"])
@pytest.mark.parametrize("kind", ["nan_yaw", "nan_coord", "inf_hi", "inf_lo", "zero_width", "negative_width"])
def test_non_finite_and_non_positive_boxes_neither_suppress_nor_are_suppressed(ops, device, kind, size):
    """Such a box is kept, no longer suppresses its partner, leaves every other pair's decision alone, and two calls agree."""
    lay = C.layout("slid", size)
    k = lay["a"].shape[0]
    boxes = C.boxes_in_order(lay, "ab").copy()
    bad_first, bad_second = np.arange(3, k, 7), np.arange(5, k, 7)  # A_p of some pairs, B_q of others
    for i in np.concatenate([bad_first, k + bad_second]):
        boxes[i] = _poison(boxes[i], kind)
    iou = lay["iou"].copy()
    iou[bad_first] = 0.0
    iou[bad_second] = 0.0
    t = 0.5
    assert (lay["iou"][bad_first] > t + lay["tol"]).any() and (lay["iou"][bad_second] > t + lay["tol"]).any()  # some did suppress before
    dev = torch.from_numpy(boxes).to(device)
    first = ops.nms_bev(dev, t, True)
    again = ops.nms_bev(dev, t, True)
    assert torch.equal(first, again)
    kept = np.zeros(2 * k, bool)
    kept[first.cpu().numpy()] = True
    assert kept[:k].all()
    second = kept[k:]
    wrong = ((iou < t - lay["tol"]) & ~second) | ((iou > t + lay["tol"]) & second)
    assert not wrong.any(), (kind, size, np.nonzero(wrong)[0][:5])


@pytest.mark.parametrize("m", [300, 400])
def test_multiclass_on_exact_duplicates_equals_per_class_calls(ops, device, m):
    """Three exact copies of m rotated boxes, three classes with their own score orders (n = 900: all-pairs mask; 1200: cell grid):
    the batched call equals the per-class calls and every class keeps exactly one copy of every box."""
    rng = np.random.default_rng(m)
    base = C.identical_layout(0)[0][rng.permutation(4096)[:m]]
    n, c = 3 * m, 3
    boxes = torch.from_numpy(np.tile(base, (3, 1))).to(device)
    scores = torch.from_numpy(rng.random((c, n)).astype(np.float32) + 0.01).to(device)
    order = scores.sort(dim=1, descending=True, stable=True)[1]
    count = torch.full((c,), n, dtype=torch.int32, device=device)
    pos = torch.arange(n, device=device, dtype=torch.int32).expand(c, n)
    rank = torch.empty_like(pos).scatter_(1, order, pos)
    keep, num = ops.nms_bev_multiclass(boxes, rank, count, 0.5, True)
    for cls in range(c):
        want = ops.nms_bev(boxes[order[cls]], 0.5, True)
        assert int(num[cls]) == want.numel() == m
        assert torch.equal(keep[cls, :m], want)
        originals = order[cls][keep[cls, :m]] % m
        assert torch.equal(originals.sort()[0].cpu(), torch.arange(m))
        # the copy kept is the best-scoring of the three
        best = scores[cls].view(3, m).argmax(0) * m + torch.arange(m, device=device)
        assert torch.equal(order[cls][keep[cls, :m]].sort()[0], best.sort()[0])
