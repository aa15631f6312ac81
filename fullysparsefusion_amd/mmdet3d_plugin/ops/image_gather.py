"""`point_image_gather`: the per-point bilinear image-feature gather as a differentiable op.

    out = point_image_gather(xyz, lidar2img, feat, img_hw, channels_last=False, reduce_cams=False, return_count=False)

* `xyz` f32 [n, >= 3] LiDAR points of ONE sample, `lidar2img` f32 [ncam, 4, 4], `feat` f32 [ncam, C, Hf, Wf] (or [ncam, Hf, Wf, C] with
  `channels_last`), `img_hw` the image size the projection normalises by;
* `out` f32 [n, ncam, C], or [n, C] summed over the cameras that see the point (`reduce_cams`); with `return_count` also the number of
  cameras that see each point, u8 [n], non-differentiable;
* the projection is FSF.prj_points_2d (FSF.py:169-200), the sampling F.grid_sample(bilinear, align_corners=False, zeros).

The forward is `fsf_project_gather_bilinear` (K13b, csrc/project.hip), the backward `fsf_project_gather_bilinear_backward` (K13c,
csrc/project_bwd.hip): the gradient reaches `feat` only, summed in a fixed order without float atomics, so a training step through the
image backbone is reproducible bit for bit.  The points and the matrices are inputs, not learned: asking for their gradient is refused.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ... import hip_ops, hip_ops_project


class PointImageGatherFunction(Function):
    @staticmethod
    def forward(ctx, xyz, lidar2img, feat, img_hw, channels_last, reduce_cams):
        out, count = hip_ops.project_gather_bilinear(xyz, lidar2img, feat, img_hw, channels_last=channels_last, reduce_cams=reduce_cams,
                                                     return_count=True)
        ctx.save_for_backward(xyz, lidar2img)
        ctx.feat_hw = tuple(feat.shape[1:3]) if channels_last else tuple(feat.shape[2:4])
        ctx.img_hw, ctx.channels_last, ctx.reduce_cams = (int(img_hw[0]), int(img_hw[1])), bool(channels_last), bool(reduce_cams)
        ctx.mark_non_differentiable(count)
        return out, count

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_count):
        xyz, lidar2img = ctx.saved_tensors
        grad_feat = None
        if ctx.needs_input_grad[2]:
            grad_feat = hip_ops_project.project_gather_bilinear_backward(xyz, lidar2img, grad_out.contiguous(), ctx.feat_hw, ctx.img_hw,
                                                                         channels_last=ctx.channels_last, reduce_cams=ctx.reduce_cams)
        return None, None, grad_feat, None, None, None


def point_image_gather(xyz, lidar2img, feat, img_hw, channels_last=False, reduce_cams=False, return_count=False):
    for name, t in (("xyz", xyz), ("lidar2img", lidar2img)):  # (before any device check: the refusal does not need a GPU)
        if t.requires_grad:
            raise NotImplementedError(f"point_image_gather: no gradient for `{name}` (the points and the camera matrices are inputs, "
                                      "not learned; only `feat` receives one)")
    out, count = PointImageGatherFunction.apply(xyz, lidar2img, feat, img_hw, bool(channels_last), bool(reduce_cams))
    return (out, count) if return_count else out


class PointImageFeatureGather(nn.Module):
    """Image features for the points of a batch: `points` a list of B per-sample point tensors f32 [n_b, >= 3] (columns 0:3 = xyz),
    `lidar2img` f32 [B, ncam, 4, 4], `feat` f32 [B, ncam, C, Hf, Wf] -> the list of B per-sample features f32 [n_b, C] (`reduce_cams`)
    or [n_b, ncam, C].  One `point_image_gather` call per sample; the gradient reaches `feat`."""

    def __init__(self, img_hw, reduce_cams=True):
        super().__init__()
        self.img_hw = (int(img_hw[0]), int(img_hw[1]))
        self.reduce_cams = bool(reduce_cams)

    def forward(self, points, lidar2img, feat):
        assert len(points) == lidar2img.size(0) == feat.size(0) and feat.dim() == 5
        return [point_image_gather(p[:, :3], lidar2img[b], feat[b], self.img_hw, reduce_cams=self.reduce_cams)
                for b, p in enumerate(points)]
