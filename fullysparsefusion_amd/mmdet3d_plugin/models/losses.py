"""`CrossEntropyLoss`, `L1Loss` and `FocalLoss` (LOSSES) in the semantics of the mmdet 2.14 pin (mmdet/models/losses/
cross_entropy_loss.py, smooth_l1_loss.py, focal_loss.py, utils.py::weight_reduce_loss).  Plain torch: the fused device paths (K35,
VoteSegHead.losses; K36, SparseClusterHeadV2.loss) read `class_weight` / `gamma` / `alpha` / `loss_weight` from these modules and never
call them.  They hold no parameters or buffers (`class_weight` is a plain attribute), so building them changes no state_dict."""
import torch
import torch.nn.functional as F
from torch import nn

from ..registry import LOSSES


def reduce_loss(loss, reduction):
    if reduction == "none":
        return loss
    if reduction == "mean":
        return loss.mean()
    if reduction == "sum":
        return loss.sum()
    raise ValueError(f"unknown reduction {reduction!r}")


def weight_reduce_loss(loss, weight=None, reduction="mean", avg_factor=None):
    if weight is not None:
        loss = loss * weight
    if avg_factor is None:
        return reduce_loss(loss, reduction)
    if reduction == "mean":
        return loss.sum() / avg_factor
    if reduction != "none":
        raise ValueError('avg_factor can not be used with reduction="sum"')
    return loss


def cross_entropy(pred, label, weight=None, reduction="mean", avg_factor=None, class_weight=None):
    loss = F.cross_entropy(pred, label, weight=class_weight, reduction="none")
    if weight is not None:
        weight = weight.float()
    return weight_reduce_loss(loss, weight=weight, reduction=reduction, avg_factor=avg_factor)


def _expand_onehot_labels(labels, label_weights, label_channels):
    bin_labels = labels.new_full((labels.size(0), label_channels), 0)
    inds = torch.nonzero((labels >= 0) & (labels < label_channels), as_tuple=False).squeeze()
    if inds.numel() > 0:
        bin_labels[inds, labels[inds]] = 1
    if label_weights is None:
        bin_label_weights = None
    else:
        bin_label_weights = label_weights.view(-1, 1).expand(label_weights.size(0), label_channels)
    return bin_labels, bin_label_weights


def binary_cross_entropy(pred, label, weight=None, reduction="mean", avg_factor=None, class_weight=None):
    if pred.dim() != label.dim():
        label, weight = _expand_onehot_labels(label, weight, pred.size(-1))
    if weight is not None:
        weight = weight.float()
    loss = F.binary_cross_entropy_with_logits(pred, label.float(), pos_weight=class_weight, reduction="none")
    return weight_reduce_loss(loss, weight, reduction=reduction, avg_factor=avg_factor)


@LOSSES.register_module()
class CrossEntropyLoss(nn.Module):
    def __init__(self, use_sigmoid=False, use_mask=False, reduction="mean", class_weight=None, loss_weight=1.0):
        super().__init__()
        assert (use_sigmoid is False) or (use_mask is False)
        if use_mask:
            raise NotImplementedError("CrossEntropyLoss(use_mask=True) is not used by the FSF configs")
        self.use_sigmoid, self.use_mask = use_sigmoid, use_mask
        self.reduction = reduction
        self.loss_weight = loss_weight
        self.class_weight = class_weight
        self.cls_criterion = binary_cross_entropy if use_sigmoid else cross_entropy

    def forward(self, cls_score, label, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        class_weight = cls_score.new_tensor(self.class_weight) if self.class_weight is not None else None
        return self.loss_weight * self.cls_criterion(cls_score, label, weight, class_weight=class_weight, reduction=reduction,
                                                     avg_factor=avg_factor, **kwargs)


def l1_loss(pred, target, weight=None, reduction="mean", avg_factor=None):
    if target.numel() == 0:
        return pred.sum() * 0
    assert pred.size() == target.size() and target.numel() > 0
    loss = torch.abs(pred - target)
    return weight_reduce_loss(loss, weight, reduction, avg_factor)


@LOSSES.register_module()
class L1Loss(nn.Module):
    def __init__(self, reduction="mean", loss_weight=1.0):
        super().__init__()
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        return self.loss_weight * l1_loss(pred, target, weight, reduction=reduction, avg_factor=avg_factor)


def sigmoid_focal_loss(pred, target, weight=None, gamma=2.0, alpha=0.25, reduction="mean", avg_factor=None):
    """mmdet 2.14 `py_sigmoid_focal_loss` on integer labels: pred [N, C] logits, target i64 [N] with C = background (its one-hot row
    is all zero).  FL = -alpha t (1 - p)^gamma log p - (1 - alpha)(1 - t) p^gamma log(1 - p), p = sigmoid(pred); the log terms come
    from binary_cross_entropy_with_logits, so large |pred| gives neither inf nor log 0.  `weight` [N] applies to every class of a row."""
    num_classes = pred.size(1)
    target = F.one_hot(target, num_classes=num_classes + 1)[:, :num_classes].type_as(pred)
    pred_sigmoid = pred.sigmoid()
    pt = (1 - pred_sigmoid) * target + pred_sigmoid * (1 - target)
    focal_weight = (alpha * target + (1 - alpha) * (1 - target)) * pt.pow(gamma)
    loss = F.binary_cross_entropy_with_logits(pred, target, reduction="none") * focal_weight
    if weight is not None:
        if weight.shape != loss.shape:
            if weight.size(0) == loss.size(0):
                weight = weight.view(-1, 1)
            else:
                assert weight.numel() == loss.numel()
                weight = weight.view(loss.size(0), -1)
        assert weight.ndim == loss.ndim
    return weight_reduce_loss(loss, weight, reduction, avg_factor)


@LOSSES.register_module()
class FocalLoss(nn.Module):
    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.25, reduction="mean", loss_weight=1.0):
        super().__init__()
        assert use_sigmoid is True, "Only sigmoid focal loss supported now."
        self.use_sigmoid = use_sigmoid
        self.gamma, self.alpha = gamma, alpha
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        return self.loss_weight * sigmoid_focal_loss(pred, target, weight, gamma=self.gamma, alpha=self.alpha, reduction=reduction,
                                                     avg_factor=avg_factor)
