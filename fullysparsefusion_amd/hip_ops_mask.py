"""Thin torch-tensor wrapper of the RoI-map painter in libfsf_hip.so (K34c: include/fsf_hip.h, docs/kernels/K34_mask_paint.md).
`mmdet3d_plugin.datasets.mask_paint.PaintMasksFromDetections` is the public interface (the `mask_rois` form of its detections);
the other K34 wrappers are `hip_ops.mask_extents` / `hip_ops.paint_instance_masks`.

Same rules as hip_ops.py / hip_ops_project.py: the function only marshals pointers / sizes and allocates the caller-owned output
(`torch.empty`); all arithmetic happens in the HIP kernel; nothing here waits for the device.  It has ragged / minimal / empty
guard-band cases in tests/test_guard_bands_mask_gpu.py.
"""
import torch

from ._lib import check, ptr, require_cuda, stream_ptr
from .hip_ops import _L

ROI_MAX = 64


def paint_roi_masks(table: torch.Tensor, boxes: torch.Tensor, roi_off: torch.Tensor, plane_ptr: torch.Tensor, plane_src_hw: torch.Tensor,
                    plane_scale: torch.Tensor, dst_hw, out_dtype, rois: torch.Tensor, roi_size: int, thr: float = 0.5):
    """fsf_paint_roi_masks (K34c): object table i32 [R, 8] (plane, y0, x0, h, w, -, -, id) in paint order, grouped per plane by
    plane_ptr i32 [P + 1], (y0, x0, h, w) the row's candidate rectangle; boxes f32 [R, 4] (x0, y0, x1, y1); roi_off i64 [R]: element
    offset of the row's map in `rois`, an f32 / f16 tensor of roi_size x roi_size maps (any shape, read only at those offsets; may be
    None or empty when R == 0); per-plane source size plane_src_hw i32 [P, 2] and f32 scale [P, 2] -> out_dtype (u8 | i32)
    [P, dst_h, dst_w], every element written once.  The caller guarantees every offset lies inside `rois`
    (mmdet3d_plugin/datasets/mask_paint.py builds the table).  No sync."""
    require_cuda(table, boxes, roi_off, plane_ptr, plane_src_hw, plane_scale, rois)
    assert table.dtype == torch.int32 and table.dim() == 2 and table.size(1) == 8
    n_rows = table.size(0)
    assert boxes.dtype == torch.float32 and boxes.numel() == 4 * n_rows
    assert roi_off.dtype == torch.int64 and roi_off.numel() == n_rows
    assert plane_ptr.dtype == torch.int32 and plane_src_hw.dtype == torch.int32 and plane_scale.dtype == torch.float32
    num_planes = plane_ptr.numel() - 1
    assert num_planes >= 0 and plane_src_hw.numel() == 2 * num_planes and plane_scale.numel() == 2 * num_planes
    assert out_dtype in (torch.uint8, torch.int32)
    roi_size = int(roi_size)
    assert 1 <= roi_size <= ROI_MAX and float(thr) > 0.0
    elem = 4
    if rois is not None:
        assert rois.dtype in (torch.float32, torch.float16), "rois must be f32 / f16"
        assert n_rows == 0 or rois.numel() >= roi_size * roi_size
        rois = rois.contiguous()
        elem = rois.element_size()
    else:
        assert n_rows == 0, "rows without RoI maps"
    dh, dw = int(dst_hw[0]), int(dst_hw[1])
    out = torch.empty((num_planes, dh, dw), dtype=out_dtype, device=table.device)
    check(_L().fsf_paint_roi_masks(ptr(table.contiguous()), ptr(boxes.contiguous()), ptr(roi_off.contiguous()), n_rows,
                                   ptr(plane_ptr.contiguous()), ptr(plane_src_hw.contiguous()), ptr(plane_scale.contiguous()), num_planes,
                                   ptr(rois) if rois is not None and rois.numel() else ptr(None), roi_size, elem, float(thr), dh, dw,
                                   out.element_size(), ptr(out), stream_ptr()), "fsf_paint_roi_masks")
    return out
