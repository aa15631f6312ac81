"""Thin torch-tensor wrapper of the optimizer step in libfsf_hip.so (K39, gradient clip + AdamW + gradient clear on the gradient
buckets: include/fsf_hip.h, docs/kernels/K39_optimizer_step.md).  `fullysparsefusion_amd.optim.FusedAdamW` is the public interface.

Same rules as hip_ops.py / hip_ops_assign.py / hip_ops_frustum.py: the functions only marshal pointers / sizes and allocate
caller-owned outputs (`torch.empty`) and scratch (`_lib.workspace`); all arithmetic happens in the HIP kernels; nothing here waits for
the device.  Every allocating function has ragged / minimal / empty guard-band cases in tests/test_guard_bands_optim_gpu.py
(tests/test_optim_cpu.py holds it to that).
"""
import torch

from . import _lib
from ._lib import c_p, check, f32_array, ptr, require_cuda, stream_ptr
from .hip_ops import _L

CHUNK = _lib.DEFINES["FSF_OPTIM_CHUNK"]
MAX_GROUPS = _lib.DEFINES["FSF_OPTIM_MAX_GROUPS"]
MAX_PARTIALS = _lib.DEFINES["FSF_OPTIM_MAX_PARTIALS"]
TABLE_WORDS = _lib.DEFINES["FSF_OPTIM_TABLE_WORDS"]


def chunk_table(rows: torch.Tensor, device):
    """The chunk table on the device: `rows` i64 [n, FSF_OPTIM_TABLE_WORDS] on the host (`optim.chunk_rows` builds them) -> the same
    on `device`, fsf_optim_table_bytes(n) bytes.  Built once per optimizer."""
    assert rows.dtype == torch.int64 and rows.dim() == 2 and rows.size(1) == TABLE_WORDS and not rows.is_cuda
    n = rows.size(0)
    nbytes = int(_L().fsf_optim_table_bytes(n))
    assert nbytes == n * TABLE_WORDS * 8
    table = torch.empty((n, TABLE_WORDS), dtype=torch.int64, device=device)
    require_cuda(table)
    if n:
        table.copy_(rows)
    return table


def adamw_step(table: torch.Tensor, decay_factor, step_size, one_minus_beta1: float, beta2: float, one_minus_beta2: float,
               bc2_sqrt: float, eps: float, max_norm, zero_grads: bool, grad_norm: torch.Tensor):
    """fsf_optim_grad_sumsq + fsf_optim_adamw_step (K39a, K39b) over every row of `table`: the parameters, both moments and (with
    `zero_grads`) the gradients the table points at are updated in place.  `decay_factor` / `step_size`: one float per group;
    `max_norm=None`: no clipping, ONE launch, `grad_norm` (f32 [1], device) is left as it is; else two launches and `grad_norm[0]`
    becomes the gradient's global 2-norm.  The scalars are taken as given (the caller rounds them to f32).  No sync."""
    require_cuda(table, grad_norm)
    assert table.dtype == torch.int64 and table.dim() == 2 and table.size(1) == TABLE_WORDS and table.is_contiguous()
    assert grad_norm.dtype == torch.float32 and grad_norm.numel() == 1
    assert len(decay_factor) == len(step_size)
    n, groups, h = table.size(0), len(decay_factor), _L()
    clip = max_norm is not None
    ws, ws_bytes = None, 0
    if clip:
        ws = _lib.workspace(h.fsf_optim_workspace_bytes(n), table.device)
        ws_bytes = ws.numel()
        check(h.fsf_optim_grad_sumsq(ptr(table) if n else c_p(None), n, ptr(ws), ws_bytes, stream_ptr()), "fsf_optim_grad_sumsq")
    check(h.fsf_optim_adamw_step(ptr(table) if n else c_p(None), n, groups, f32_array(decay_factor), f32_array(step_size),
                                 float(one_minus_beta1), float(beta2), float(one_minus_beta2), float(bc2_sqrt), float(eps),
                                 float(max_norm) if clip else 0.0, int(clip), int(bool(zero_grads)), ptr(ws), ws_bytes, ptr(grad_norm),
                                 stream_ptr()), "fsf_optim_adamw_step")
    return grad_norm
