"""Thin torch-tensor wrapper of the bilinear image-feature gather's backward in libfsf_hip.so (K13c: include/fsf_hip.h,
docs/kernels/K13c_bilinear_backward.md).  `mmdet3d_plugin.ops.point_image_gather` is the public interface; the forward is
`hip_ops.project_gather_bilinear`.

Same rules as hip_ops.py / hip_ops_augment.py: the function only marshals pointers / sizes and allocates the caller-owned output
(`torch.empty`) and scratch (`_lib.workspace`); all arithmetic happens in the HIP kernels; nothing here waits for the device.  It has
ragged / minimal / empty guard-band cases in tests/test_guard_bands_project_gpu.py (tests/test_bilinear_backward_cpu.py holds it to that).
"""
import torch

from . import _lib
from ._lib import c_p, check, ptr, require_cuda, stream_ptr
from .hip_ops import _L, _rows_view

CHUNK = _lib.DEFINES["FSF_BILINEAR_BWD_CHUNK"]


def project_gather_bilinear_backward(xyz: torch.Tensor, lidar2img: torch.Tensor, grad_out: torch.Tensor, feat_hw, img_hw,
                                     channels_last=False, reduce_cams=False):
    """fsf_project_gather_bilinear_backward (K13c) for ONE sample: xyz f32 [n, >= 3] (a row-strided view is taken as it is), lidar2img
    f32 [ncam, 4, 4], grad_out f32 [n, ncam, C] (or [n, C] with reduce_cams) -> grad_feat f32 [ncam, C, Hf, Wf] (or [ncam, Hf, Wf, C]
    with channels_last), every element written: the exact transpose of `hip_ops.project_gather_bilinear` on the same taps, summed in
    a fixed order without float atomics.  No sync."""
    require_cuda(xyz, lidar2img, grad_out)
    assert xyz.dtype == torch.float32 and lidar2img.dtype == torch.float32 and grad_out.dtype == torch.float32
    assert xyz.dim() == 2 and xyz.size(1) >= 3 and lidar2img.dim() == 3 and lidar2img.shape[1:] == (4, 4)
    xyz, stride = _rows_view(xyz)
    lidar2img, grad_out = lidar2img.contiguous(), grad_out.contiguous()
    n = xyz.size(0)
    ncam = lidar2img.size(0)
    hf, wf = int(feat_hw[0]), int(feat_hw[1])
    assert grad_out.dim() == (2 if reduce_cams else 3) and grad_out.size(0) == n and (reduce_cams or grad_out.size(1) == ncam)
    c = grad_out.size(-1)
    grad_feat = torch.empty((ncam, hf, wf, c) if channels_last else (ncam, c, hf, wf), dtype=torch.float32, device=xyz.device)
    h = _L()
    ws = _lib.workspace(h.fsf_project_gather_bilinear_backward_workspace_bytes(n, ncam, hf, wf, c), xyz.device)
    check(h.fsf_project_gather_bilinear_backward(c_p(xyz.data_ptr()) if n else c_p(None), n, stride, ptr(lidar2img), ncam,
                                                 ptr(grad_out) if n else c_p(None), c, hf, wf, int(bool(channels_last)), int(img_hw[0]),
                                                 int(img_hw[1]), int(bool(reduce_cams)), ptr(grad_feat), ptr(ws), ws.numel(), stream_ptr()),
          "fsf_project_gather_bilinear_backward")
    return grad_feat
