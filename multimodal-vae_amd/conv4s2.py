"""The 4 x 4, stride 2, pad 1 convolution and its transpose, bias-free, with a fused activation (csrc/conv4s2.hip): the down- and
up-sampling block of a small convolutional autoencoder, here the MNIST ``InfoVAE`` (``mnist/model.py:238-279``).

With ``Cs`` the channels on the high-resolution side (2H x 2W) and ``Cl`` those on the low-resolution side (H x W), an
``nn.Conv2d(Cs, Cl, 4, 2, 1)`` weight and an ``nn.ConvTranspose2d(Cl, Cs, 4, 2, 1)`` weight are both ``(Cl, Cs, 4, 4)``: ``down4s2``
takes the first, ``up4s2`` the second, and three kernels (down, up, weight gradient) serve both in both directions.  Device-only:
there is no CPU fallback.
"""
from __future__ import annotations

from typing import Tuple

import torch

from ._lib import MMVAEError, call, ptr
from ._ops import CONV_WS, empty_nhwc, geometry, nhwc, stream

ACTS = ("none", "relu", "leaky", "sigmoid")


def conv4s2_geometry() -> Tuple[int, int, int, int, int, int]:
    """(L positions per workgroup, output channels per workgroup, least L positions per weight-gradient chunk, most chunks, largest
    channel count, largest side of the high-resolution image)"""
    return geometry("mmvae_conv4s2_geometry", 6)


def conv4s2_workspace_bytes(B, Cs, Cl, Hs, Ws) -> int:
    """device scratch one call needs; 0 when the shape is outside the op's limits (a host function: needs no GPU)"""
    return int(call("mmvae_conv4s2_workspace_bytes", int(B), int(Cs), int(Cl), int(Hs), int(Ws)))


def _check(what, x, weight, act, x_channels):
    """validates everything before anything is launched -> (act code, (B, Cs, Cl, Hs, Ws))"""
    if act not in ACTS:
        raise MMVAEError("%s: act %r, need one of %s" % (what, act, ACTS))
    for name, t in (("x", x), ("weight", weight)):
        if not torch.is_tensor(t) or t.device.type != "cuda" or t.dtype != torch.float32:
            raise MMVAEError("%s: %s must be a float32 tensor on a gfx950 GPU (got %s): there is no CPU fallback"
                             % (what, name, "%s, %s" % (t.device, t.dtype) if torch.is_tensor(t) else type(t).__name__))
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[2:]) != (4, 4) or weight.shape[x_channels] != x.shape[1] or weight.device != x.device:
        raise MMVAEError("%s: x %s and weight %s do not fit: (B, %s, H, W) and (Cl, Cs, 4, 4) on one device expected"
                         % (what, tuple(x.shape), tuple(weight.shape), "Cs" if x_channels == 1 else "Cl"))
    B, Cl, Cs = int(x.shape[0]), int(weight.shape[0]), int(weight.shape[1])
    Hs, Ws = (int(x.shape[2]), int(x.shape[3])) if x_channels == 1 else (2 * int(x.shape[2]), 2 * int(x.shape[3]))
    dims = (B, Cs, Cl, Hs, Ws)
    if conv4s2_workspace_bytes(*dims) <= 0:
        _, _, _, _, max_ch, max_side = conv4s2_geometry()
        raise MMVAEError("%s: B = %d, Cs = %d, Cl = %d, high-resolution side %d x %d is outside what the kernels are built for (B >= 1, "
                         "channels 1..%d, even sides 2..%d)" % ((what,) + dims + (max_ch, max_side)))
    return ACTS.index(act), dims


def _tail(dims, dev):
    ws = CONV_WS.get(dev, conv4s2_workspace_bytes(*dims))
    return dims + (ptr(ws), ws.numel(), stream())


class _Down(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, act, slope):
        code, dims = _check("down4s2", x, weight, act, 1)
        B, Cs, Cl, Hs, Ws = dims
        x, w = nhwc(x.detach()), weight.detach().contiguous()
        with torch.cuda.device(x.device):
            y = empty_nhwc(B, Cl, Hs // 2, Ws // 2, x.device)
            call("mmvae_conv4s2_down", ptr(x), None, ptr(w), ptr(y), 0, code, float(slope), *_tail(dims, x.device))
        ctx.save_for_backward(x, w, y)
        ctx.code, ctx.slope, ctx.dims = code, float(slope), dims
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, w, y = ctx.saved_tensors
        B, Cs, Cl, Hs, Ws = ctx.dims
        g = nhwc(g)
        yp = ptr(y) if ctx.code else None                  # (no activation: the gradient operand is g itself)
        dx = dw = None
        with torch.cuda.device(x.device):
            if ctx.needs_input_grad[0]:
                dx = empty_nhwc(B, Cs, Hs, Ws, x.device)
                call("mmvae_conv4s2_up", ptr(g), yp, ptr(w), ptr(dx), ctx.code, 0, ctx.slope, *_tail(ctx.dims, x.device))
            if ctx.needs_input_grad[1]:
                dw = torch.empty_like(w)
                call("mmvae_conv4s2_wgrad", ptr(x), ptr(g), None, yp, ctx.code, ctx.slope, ptr(dw), *_tail(ctx.dims, x.device))
        return dx, dw, None, None


class _Up(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, act, slope):
        code, dims = _check("up4s2", x, weight, act, 0)
        B, Cs, Cl, Hs, Ws = dims
        x, w = nhwc(x.detach()), weight.detach().contiguous()
        with torch.cuda.device(x.device):
            y = empty_nhwc(B, Cs, Hs, Ws, x.device)
            call("mmvae_conv4s2_up", ptr(x), None, ptr(w), ptr(y), 0, code, float(slope), *_tail(dims, x.device))
        ctx.save_for_backward(x, w, y)
        ctx.code, ctx.slope, ctx.dims = code, float(slope), dims
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, w, y = ctx.saved_tensors
        B, Cs, Cl, Hs, Ws = ctx.dims
        g = nhwc(g)
        yp = ptr(y) if ctx.code else None
        dx = dw = None
        with torch.cuda.device(x.device):
            if ctx.needs_input_grad[0]:
                dx = empty_nhwc(B, Cl, Hs // 2, Ws // 2, x.device)
                call("mmvae_conv4s2_down", ptr(g), yp, ptr(w), ptr(dx), ctx.code, 0, ctx.slope, *_tail(ctx.dims, x.device))
            if ctx.needs_input_grad[1]:
                dw = torch.empty_like(w)
                call("mmvae_conv4s2_wgrad", ptr(g), ptr(x), yp, None, ctx.code, ctx.slope, ptr(dw), *_tail(ctx.dims, x.device))
        return dx, dw, None, None


def down4s2(x, weight, act="none", slope=0.1):
    """``act(F.conv2d(x, weight, stride=2, padding=1))`` as one device op: ``x`` (B, Cs, Hs, Ws) float32 (consumed channels-last),
    ``weight`` (Cl, Cs, 4, 4) -> (B, Cl, Hs/2, Ws/2) float32, channels-last.  ``act`` is one of ``ACTS``; ``slope`` is the leaky
    slope.  With bf16(.) round-to-nearest-even and fp32 accumulation, a position outside the image contributing nothing::

        pre[b,l,oy,ox] = sum_{s,ky,kx} bf16(x[b,s,2oy-1+ky,2ox-1+kx]) bf16(w[l,s,ky,kx])
        y = act(pre):  leaky: pre > 0 ? pre : slope pre;  sigmoid: 1 / (1 + exp(-pre))

    The backward works from the saved output ``y`` (the pre-activation is never stored): ``gp = g`` (none), ``y > 0 ? g : 0`` (relu),
    ``y > 0 ? g : slope g`` (leaky), ``(g y) (1 - y)`` (sigmoid), formed in fp32 while the gradient operand is loaded and then rounded to
    bf16; ``dx = up(gp, w)``, ``dw[l,s,ky,kx] = sum_{b,oy,ox} bf16(gp[b,l,oy,ox]) bf16(x[b,s,2oy-1+ky,2ox-1+kx])``.

    Once differentiable; gradients nobody asked for are not computed; no atomics, two calls give identical bits.  Limits: Cs, Cl
    1..128, Hs, Ws even in 2..64 (``conv4s2_geometry``).  Device-only: a CPU tensor raises ``MMVAEError``."""
    return _Down.apply(x, weight, act, slope)


def up4s2(x, weight, act="none", slope=0.1):
    """``act(F.conv_transpose2d(x, weight, stride=2, padding=1))`` as one device op: ``x`` (B, Cl, H, W) float32 (consumed
    channels-last), ``weight`` (Cl, Cs, 4, 4) -> (B, Cs, 2H, 2W) float32, channels-last::

        pre[b,s,iy,ix] = sum_{l,ky,kx : iy+1-ky, ix+1-kx even and inside} bf16(x[b,l,(iy+1-ky)/2,(ix+1-kx)/2]) bf16(w[l,s,ky,kx])

    An output pixel's row and column parity selects 2 x 2 of the 16 cells: four dense sub-problems, not a scatter.  Activation,
    backward (``dx = down(gp, w)``, ``dw[l,s,ky,kx] = sum bf16(x[b,l,oy,ox]) bf16(gp[b,s,2oy-1+ky,2ox-1+kx])``), limits and errors as
    in ``down4s2``."""
    return _Up.apply(x, weight, act, slope)
