"""Gaussian-kernel maximum mean discrepancy, the InfoVAE regulariser (``coco/model.py:385-402``, the same functions in
``mnist/train_infovae.py:45-76``), on one fused HIP op (csrc/mmd.hip)::

    k(a, b)   = exp(-mean_k (a_k - b_k)^2 / D)
    MMD(x, y) = mean_ij k(x_i, x_j) + mean_ij k(y_i, y_j) - 2 mean_ij k(x_i, y_j)

``compute_mmd`` is differentiable in both arguments: ONE call of ``mmvae_mmd`` computes the value and both gradients (they share
every k_ij), the backward is a multiply by the upstream scalar.  The ``(n, n, D)`` tensors of the reference formulation never
exist, so the aggregate posterior of a whole test set against the prior (10,000 x 10,000) is one call.  fp32 device tensors only;
there is no CPU fallback.  All three functions run on the caller's current stream; the workspace is cached per (device, stream,
shape).  Results depend on the shape alone: two calls give identical bits.
"""
from __future__ import annotations

from typing import Tuple

import torch

from ._lib import MMVAEError, call, ptr
from ._ops import WorkspaceCache, geometry, stream

_WS = WorkspaceCache(8)          # cached workspaces (the oldest goes first)


def mmd_geometry() -> Tuple[int, int, int]:
    """(rows per workgroup, rows per column tile, largest D) of the kernels; include/mmvae_hip.h states the split rule."""
    return geometry("mmvae_mmd_geometry", 3)


def _pair(x: torch.Tensor, y: torch.Tensor, what: str):
    if not (torch.is_tensor(x) and torch.is_tensor(y)) or x.dim() != 2 or y.dim() != 2 or x.shape[1] != y.shape[1]:
        raise MMVAEError("%s: x (n_x, D) and y (n_y, D) expected" % what)
    if x.device.type != "cuda" or y.device != x.device:
        raise MMVAEError("%s runs on a gfx950 GPU only (got %s, %s): move both tensors to the device.  There is no CPU fallback."
                         % (what, x.device, y.device))
    if x.dtype != torch.float32 or y.dtype != torch.float32:
        raise MMVAEError("%s: float32 tensors expected (got %s, %s)" % (what, x.dtype, y.dtype))
    same = y is x
    x = x.detach().contiguous()
    y = x if same else y.detach().contiguous()
    return x, y, x.shape[0], y.shape[0], x.shape[1]


def _workspace(dev: torch.device, n_x: int, n_y: int, dim: int) -> Tuple[torch.Tensor, int]:
    need = call("mmvae_mmd_workspace_bytes", n_x, n_y, dim)
    if need <= 0:
        _, _, md = mmd_geometry()
        raise MMVAEError("mmd: n_x = %d, n_y = %d, D = %d: need 1..65536 rows and 1..%d columns" % (n_x, n_y, dim, md))
    return _WS.get(dev, need, n_x, n_y, dim), need


def _run(x: torch.Tensor, y: torch.Tensor, grad: bool):
    x, y, n_x, n_y, dim = _pair(x, y, "compute_mmd")
    with torch.cuda.device(x.device):
        ws, need = _workspace(x.device, n_x, n_y, dim)
        out = torch.empty(4, dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x) if grad else None
        dy = torch.empty_like(y) if grad else None
        call("mmvae_mmd", ptr(x), n_x, ptr(y), n_y, dim, ptr(ws), need, ptr(out), ptr(dx), ptr(dy), stream())
    return out, dx, dy


class _MMDFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        out, dx, dy = _run(x, y, grad)
        if grad:
            ctx.save_for_backward(dx, dy)
        return out[3].clone()

    @staticmethod
    def backward(ctx, g):
        dx, dy = ctx.saved_tensors
        return (dx * g if ctx.needs_input_grad[0] else None), (dy * g if ctx.needs_input_grad[1] else None)


def compute_mmd(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """coco/model.py:397-402 -> 0-d tensor, with autograd into both inputs."""
    return _MMDFn.apply(x, y)


@torch.no_grad()
def mmd_terms(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """-> device tensor of 4: (mean k(x, x), mean k(y, y), mean k(x, y), MMD).  No autograd."""
    return _run(x, y, False)[0]


@torch.no_grad()
def compute_kernel(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """coco/model.py:385-394 -> the (n_x, n_y) kernel matrix, with the per-pair arithmetic of ``compute_mmd``.  NO autograd: the
    differentiable quantity is ``compute_mmd``, which never forms this matrix."""
    x, y, n_x, n_y, dim = _pair(x, y, "compute_kernel")
    k = torch.empty(n_x, n_y, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        call("mmvae_mmd_kernel_matrix", ptr(x), n_x, ptr(y), n_y, dim, ptr(k), stream())
    return k
