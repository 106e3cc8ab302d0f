"""PixelCNN / GatedPixelCNN (``coco/model.py:405-585``, the same family in ``mnist/model.py``) and a one-launch incremental
sampler for them (csrc/pixelcnn.hip).

The modules are plain torch: constructor signatures, attribute names and ``state_dict`` keys are those of ``coco/model.py``, so a
reference checkpoint loads; they run wherever torch runs and train through autograd.  ``nll(model, x)`` is the per-element negative log-likelihood
(``bits_per_dim`` per image); with ``head="hip"`` the output head ``conv4`` and the cross entropy run as one fused device op,
``head_nll`` (csrc/head_nll.hip), that never writes the logits to memory.  ``set_conv_backend(model, "hip")`` routes every
convolution of a model through ``causal_conv2d`` (csrc/causal_conv.hip: bf16 operands, fp32 accumulation, only the taps that exist)
for training on the device; the default backend stays torch.  The forward returns
``(B, out_dims, data_channels, H, W)``, output channel ``v * data_channels + c`` being level ``v`` of channel ``c``.

``generate`` replaces the reference's sampling loop (one full forward per pixel and channel, ``coco/train_pixelcnn.py:185-197``).
These classes use ``MaskedConv2d`` (not ``MaskedConv2dRGB``), so the logits at (i, j) depend on raster-earlier pixels only and all
channels of a pixel are drawn from one evaluation; the kernel computes, per pixel, each layer's activation at that pixel alone from
cached rows.  Device-only: there is no CPU fallback.

Left out: ``MaskedConv2dRGB`` (references an undefined ``mask``, never instantiated) and ``mnist/model.py``'s ``PixelCNNv2``
(broken).
"""
from __future__ import annotations

import ctypes
import os
import shutil
from collections import namedtuple
from typing import Dict, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ._lib import MMVAEError, call, ptr
from ._ops import CONV_WS, WorkspaceCache, empty_nhwc, geometry, nhwc, stream

PixelSample = namedtuple("PixelSample", ["image", "levels", "logits"])


class MaskedConv2d(nn.Conv2d):
    """A convolution that sees raster-earlier taps only: of a kh x kw window (both > 1) mask A keeps the taps in front of the
    centre, mask B those up to and including it.  A 1 x 1 (or one-row, one-column) kernel keeps everything.  ``mask`` is a buffer
    and so part of the ``state_dict``; a forward zeroes the masked entries of ``weight`` in place, as the reference's does."""

    def __init__(self, mask_type, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if mask_type not in ("A", "B"):
            raise ValueError("mask_type must be 'A' or 'B' (got %r)" % (mask_type,))
        kh, kw = self.kernel_size
        keep = torch.ones(kh, kw)
        if min(kh, kw) > 1:
            raster = torch.arange(kh * kw).view(kh, kw)
            centre = (kh // 2) * kw + kw // 2
            keep = (raster <= centre if mask_type == "B" else raster < centre).float()
        self.register_buffer("mask", torch.ones_like(self.weight.data) * keep)
        self.mask_type = mask_type

    def forward(self, x):
        self.weight.data.mul_(self.mask)
        if getattr(self, "conv_backend", "torch") == "hip":
            return causal_conv2d(x, self.weight, self.bias, taps_of(self))
        return self._conv_forward(x, self.weight, self.bias)


class CroppedConv2d(nn.Conv2d):
    """A side padded by the whole kernel size loses its last kernel size + 1 outputs: what is left sees strictly earlier rows
    (columns) of the input."""

    def forward(self, x):
        if getattr(self, "conv_backend", "torch") == "hip":
            return causal_conv2d(x, self.weight, self.bias, taps_of(self))      # (the cropped rows and columns are never computed)
        y = self._conv_forward(x, self.weight, self.bias)
        rows, cols = y.shape[2:]
        if self.padding[0] == self.kernel_size[0]:
            rows -= self.kernel_size[0] + 1
        if self.padding[1] == self.kernel_size[1]:
            cols -= self.kernel_size[1] + 1
        return y[:, :, :rows, :cols]


def _conv1x1(m, x):
    """a plain 1 x 1 ``nn.Conv2d`` under the backend ``set_conv_backend`` chose for it"""
    if getattr(m, "conv_backend", "torch") == "hip":
        return causal_conv2d(x, m.weight, m.bias, taps_of(m))
    return m(x)


def _gate(t):
    """tanh of the first half of the channels x sigmoid of the second"""
    a, b = t.chunk(2, dim=1)
    return torch.tanh(a) * torch.sigmoid(b)


class GatedResidualBlock(nn.Module):
    """A vertical stack (the rows above) and a horizontal stack (the pixels to the left, fed by the vertical one through
    ``x_to_h_conv``), each gated.  -> (vertical output, horizontal output before the residual)"""

    def __init__(self, mask_type, in_channels, out_channels, kernel_size):
        super().__init__()
        reach, wide = kernel_size // 2 + 1, 2 * out_channels
        self.vertical_conv = CroppedConv2d(in_channels, wide, kernel_size=(reach, kernel_size), padding=(reach, kernel_size // 2))
        self.x_to_h_conv = MaskedConv2d(mask_type, wide, wide, 1)
        self.vertical_gate_conv = nn.Conv2d(wide, wide, 1)
        self.horizontal_conv = CroppedConv2d(in_channels, wide, kernel_size=(1, reach), padding=(0, reach))
        self.horizontal_gate_conv = nn.Conv2d(wide, wide, 1)
        self.horizontal_output = MaskedConv2d(mask_type, out_channels, out_channels, 1)
        self.in_channels = in_channels
        self.out_channels = out_channels

    def forward(self, x, h):
        above = self.vertical_conv(x)
        left = self.horizontal_conv(h) + self.x_to_h_conv(above)
        return _gate(_conv1x1(self.vertical_gate_conv, above)), self.horizontal_output(_gate(_conv1x1(self.horizontal_gate_conv, left)))


class GatedResidualBlockList(nn.Module):
    def __init__(self, block_num, *args, **kwargs):
        super().__init__()
        self.blocks = nn.Sequential(*[GatedResidualBlock(*args, **kwargs) for _ in range(block_num)])

    def forward(self, x, h):
        for block in self.blocks:
            x_, h_ = block(x, h)
            x, h = x_, h + h_
        return x, h


class PixelCNN(nn.Module):
    """The masked-convolution PixelCNN of van den Oord et al."""

    def __init__(self, n_blocks=15, data_channels=1, hid_dims=128, out_dims=256):
        super().__init__()
        self.conv1 = MaskedConv2d("A", data_channels, hid_dims, 7, 1, 3)
        blocks = []
        for _ in range(n_blocks):
            blocks += [MaskedConv2d("B", hid_dims, hid_dims, 3, 1, 1), nn.ReLU(True)]
        self.blocks = nn.Sequential(*blocks)
        self.conv2 = MaskedConv2d("B", hid_dims, hid_dims, 1)
        self.conv4 = MaskedConv2d("B", hid_dims, out_dims * data_channels, 1)
        self.data_channels = data_channels
        self.hid_dims = hid_dims
        self.out_dims = out_dims
        self.n_blocks = n_blocks

    def features(self, x):
        """the activation ``conv4`` consumes (its ReLU included): (B, hid_dims, H, W)"""
        x = self.conv1(x)
        x = self.blocks(x)
        return F.relu(self.conv2(x))

    def forward(self, x):
        x = self.conv4(self.features(x))
        batch_size, _, height, width = x.size()
        return x.view(batch_size, self.out_dims, self.data_channels, height, width)


class GatedPixelCNN(nn.Module):
    """PixelCNN with a vertical and a horizontal stack (no blind spot) and gated blocks."""

    def __init__(self, n_blocks=15, data_channels=1, hid_dims=128, out_dims=256):
        super().__init__()
        self.conv1 = GatedResidualBlock("A", data_channels, hid_dims, 7)
        self.blocks = GatedResidualBlockList(n_blocks, "B", hid_dims, hid_dims, 3)
        self.conv2 = MaskedConv2d("B", hid_dims, hid_dims, 1)
        self.conv4 = MaskedConv2d("B", hid_dims, out_dims * data_channels, 1)
        self.data_channels = data_channels
        self.hid_dims = hid_dims          # (the reference leaves this one out; the sampler and the checkpoint need it)
        self.out_dims = out_dims
        self.n_blocks = n_blocks

    def features(self, x):
        """the activation ``conv4`` consumes (its ReLU included): (B, hid_dims, H, W)"""
        x, h = self.conv1(x, x)
        _, h = self.blocks(x, h)
        return F.relu(self.conv2(F.relu(h)))

    def forward(self, x):
        h = self.conv4(self.features(x))
        batch_size, _, height, width = h.size()
        return h.view(batch_size, self.out_dims, self.data_channels, height, width)


def log_softmax_by_dim(input, dim=1):
    return F.log_softmax(input, dim=dim)


def cross_entropy_by_dim(input, output, dim=1):
    """input (B, V, C, H, W) logits, output (B, C, H, W) integer levels -> mean cross entropy over every (sample, channel, pixel)."""
    trans = input.permute(0, 2, 3, 4, 1)
    return F.cross_entropy(trans.contiguous().view(-1, trans.size(-1)), output.contiguous().view(-1))


def quantisize(images, levels):
    """values in [0, 1] -> integer levels 0..levels - 1 (numpy in, numpy out)"""
    return (np.digitize(images, np.arange(levels) / levels) - 1).astype("i")


# ------------------------------------------------------------------------------------------------------ checkpoints
def save_checkpoint(state, is_best, folder="./", filename="checkpoint.pth.tar"):
    torch.save(state, os.path.join(folder, filename))
    if is_best:
        shutil.copyfile(os.path.join(folder, filename), os.path.join(folder, "model_best.pth.tar"))


def infer_config(state_dict) -> dict:
    """(gated, n_blocks, data_channels, hid_dims, out_dims) from the tensor shapes: what a checkpoint without these keys lacks"""
    gated = "conv1.vertical_conv.weight" in state_dict
    w1 = state_dict["conv1.vertical_conv.weight" if gated else "conv1.weight"]
    channels = int(w1.shape[1])
    hid = int(state_dict["conv2.weight"].shape[0])
    if gated:
        n_blocks = len({k.split(".")[2] for k in state_dict if k.startswith("blocks.blocks.")})
    else:
        n_blocks = len({k.split(".")[1] for k in state_dict if k.startswith("blocks.")})
    return {"gated": gated, "n_blocks": n_blocks, "data_channels": channels, "hid_dims": hid,
            "out_dims": int(state_dict["conv4.weight"].shape[0]) // channels}


def load_checkpoint(file_path, use_cuda=False):
    ckpt = torch.load(file_path, map_location=None if use_cuda else "cpu", weights_only=False)
    cfg = infer_config(ckpt["state_dict"])
    for k in cfg:
        if k in ckpt:
            cfg[k] = ckpt[k]
    cls = GatedPixelCNN if cfg.pop("gated") else PixelCNN
    model = cls(**cfg)
    model.load_state_dict(ckpt["state_dict"])
    model.height, model.width = ckpt.get("height"), ckpt.get("width")
    if use_cuda:
        model.cuda()
    return model


# ------------------------------------------------------------------------------------------------------ the sampler
_WS = WorkspaceCache(4)          # cached workspaces (the oldest goes first)


def pixelcnn_geometry() -> Tuple[int, int, int]:
    """(samples per workgroup, largest hid_dims, largest side) of the kernel"""
    return geometry("mmvae_pixelcnn_geometry", 3)


def _config(model, what="generate") -> Tuple[int, int, int, int, int]:
    if isinstance(model, GatedPixelCNN):
        gated, hid = 1, model.conv2.weight.shape[0]
    elif isinstance(model, PixelCNN):
        gated, hid = 0, model.hid_dims
    else:
        raise MMVAEError("%s: a PixelCNN or GatedPixelCNN expected (got %s)" % (what, type(model).__name__))
    return gated, int(model.n_blocks), int(model.data_channels), int(hid), int(model.out_dims)


def _layers(model):
    """the convolutions in the order of the kernel's operation table (include/mmvae_hip.h)"""
    if isinstance(model, GatedPixelCNN):
        out = []
        for blk in [model.conv1] + list(model.blocks.blocks):
            out += [blk.vertical_conv, blk.x_to_h_conv, blk.vertical_gate_conv, blk.horizontal_conv, blk.horizontal_gate_conv,
                    blk.horizontal_output]
        return out + [model.conv2, model.conv4]
    return [model.conv1] + [m for m in model.blocks if isinstance(m, nn.Conv2d)] + [model.conv2, model.conv4]


def _check_model(model):
    """-> (cfg, device); raises before anything is launched"""
    cfg = _config(model)
    if call("mmvae_pixelcnn_packed_elems", *cfg) <= 0:
        raise MMVAEError("pixelcnn: n_blocks = %d, data_channels = %d, hid_dims = %d, out_dims = %d is outside what the kernel is built "
                         "for (n_blocks 0..15, data_channels 1 or 3, hid_dims a multiple of 16 up to 128, out_dims 2..256)" % cfg[1:])
    w = model.conv4.weight
    if w.device.type != "cuda" or any(m.weight.dtype != torch.float32 or m.weight.device != w.device for m in _layers(model)):
        raise MMVAEError("pixelcnn: the sampler runs on a gfx950 GPU only, on float32 weights (got %s, %s): move the model to the device."
                         "  There is no CPU fallback." % (w.device, w.dtype))
    return cfg, w.device


def pack_weights(model) -> torch.Tensor:
    """-> the packed fp32 device vector the kernel reads: tap-major per layer, masks applied."""
    cfg, dev = _check_model(model)
    parts = []
    for m in _layers(model):
        parts += [m.weight.detach().reshape(-1), m.bias.detach().reshape(-1)]
    flat = torch.cat(parts).contiguous()
    packed = torch.empty(call("mmvae_pixelcnn_packed_elems", *cfg), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        call("mmvae_pixelcnn_pack_weights", *cfg, ptr(flat), flat.numel(), ptr(packed), stream())
    return packed


def _workspace(dev, cfg, B, H, W):
    need = call("mmvae_pixelcnn_workspace_bytes", *cfg, B, H, W)
    return _WS.get(dev, need, cfg, B, H, W), need


@torch.no_grad()
def generate(model, n_samples=64, height=28, width=28, *, uniforms=None, seed=0, given=None, n_given=0, return_logits=False):
    """Draws ``n_samples`` images pixel by pixel in ONE kernel launch -> ``PixelSample(image, levels, logits)``.

    ``uniforms`` (B, C, H, W) float32 on the model's device decides every draw (the smallest level v with u < CDF_v); when None it
    comes from ``torch.rand`` under a generator seeded with ``seed``.  The first ``n_given`` pixels in raster order are taken from
    ``given`` (B, C, H, W), integer levels, instead of being drawn: ``n_given = H * W`` evaluates a whole image teacher-forced,
    ``n_given = r * W`` completes an image from row r.  ``image`` is ``levels / (out_dims - 1)`` float32, ``levels`` int64, ``logits``
    (B, out_dims, C, H, W) the logits each pixel was drawn from (None unless ``return_logits``)."""
    cfg, dev = _check_model(model)
    B, H, W, C, V = int(n_samples), int(height), int(width), cfg[2], cfg[4]
    if call("mmvae_pixelcnn_workspace_bytes", *cfg, B, H, W) <= 0:
        _, _, side = pixelcnn_geometry()
        raise MMVAEError("generate: n_samples = %d, height = %d, width = %d: need n_samples >= 1 and sides 1..%d" % (B, H, W, side))
    if n_given < 0 or n_given > H * W:
        raise MMVAEError("generate: n_given = %d, need 0..%d" % (n_given, H * W))
    if uniforms is None:
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        uniforms = torch.rand(B, C, H, W, generator=gen, device=dev, dtype=torch.float32)
    if not torch.is_tensor(uniforms) or tuple(uniforms.shape) != (B, C, H, W) or uniforms.dtype != torch.float32 or uniforms.device != dev:
        raise MMVAEError("generate: uniforms must be a float32 tensor of shape %s on %s" % ((B, C, H, W), dev))
    g32 = None
    if n_given > 0:
        if (not torch.is_tensor(given) or tuple(given.shape) != (B, C, H, W) or given.is_floating_point() or given.is_complex()
                or given.dtype == torch.bool or given.device != dev):
            raise MMVAEError("generate: given must be an integer tensor of levels, shape %s on %s" % ((B, C, H, W), dev))
        g32 = given.to(torch.int32).contiguous()
    uniforms = uniforms.contiguous()
    packed = pack_weights(model)
    with torch.cuda.device(dev):
        ws, need = _workspace(dev, cfg, B, H, W)
        levels = torch.empty(B, C, H, W, dtype=torch.int32, device=dev)
        image = torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
        logits = torch.empty(B, V, C, H, W, dtype=torch.float32, device=dev) if return_logits else None
        call("mmvae_pixelcnn_sample", *cfg, ptr(packed), ptr(ws), need, B, H, W, ptr(uniforms), ptr(g32), int(n_given), ptr(levels),
             ptr(image), ptr(logits), stream())
    return PixelSample(image, levels.long(), logits)


# ------------------------------------------------------------------------------------------------------ the training convolution
_conv_ws, _CONV_WS = CONV_WS.get, CONV_WS.buffers          # the shared scratch (_ops.py); the tests poison _CONV_WS between two runs
_TAPS_C: Dict[Tuple, ctypes.Array] = {}
CONV_BACKENDS = ("torch", "hip")


def causal_conv_geometry() -> Tuple[int, int, int, int, int, int]:
    """(positions per tile, channels per tile, positions per weight-gradient chunk, most taps, largest |offset|, most channels)"""
    return geometry("mmvae_causal_conv_geometry", 6)


def taps_of(module) -> Tuple[Tuple[int, int, int, int], ...]:
    """The tap list ``((r, c, dy, dx), ...)`` of a ``MaskedConv2d``, a ``CroppedConv2d`` or a plain 1 x 1 ``nn.Conv2d``: kernel cell
    (r, c) is applied at offset (dy, dx) = (r - padding[0], c - padding[1]).  A masked kh x kw window keeps its first n cells in raster
    order (mask A 24 of 49, mask B 5 of 9); the vertical cropped convolution, padded by its whole height, reaches rows -reach .. -1,
    the horizontal one columns -reach .. -1."""
    if not isinstance(module, nn.Conv2d):
        raise MMVAEError("taps_of: a convolution module expected (got %s)" % type(module).__name__)
    (kh, kw), (ph, pw) = module.kernel_size, module.padding
    if module.stride != (1, 1) or module.dilation != (1, 1) or module.groups != 1 or isinstance(ph, str) or module.padding_mode != "zeros":
        raise MMVAEError("taps_of: stride 1, dilation 1, groups 1 and zero padding expected")
    n = kh * kw
    if isinstance(module, MaskedConv2d):
        if (ph, pw) != (kh // 2, kw // 2) or kh % 2 == 0 or kw % 2 == 0:
            raise MMVAEError("taps_of: a MaskedConv2d needs an odd kernel with centre padding (kernel %s, padding %s)" % ((kh, kw), (ph, pw)))
        if min(kh, kw) > 1:
            n = (kh // 2) * kw + kw // 2 + (1 if module.mask_type == "B" else 0)
    elif isinstance(module, CroppedConv2d):
        if not ((ph == kh or (ph == kh // 2 and kh % 2 == 1)) and (pw == kw or (pw == kw // 2 and kw % 2 == 1))):
            raise MMVAEError("taps_of: a CroppedConv2d pads a side by the whole kernel size or by half an odd one (kernel %s, padding %s)"
                             % ((kh, kw), (ph, pw)))
    elif (kh, kw) != (1, 1) or (ph, pw) != (0, 0):
        raise MMVAEError("taps_of: a plain nn.Conv2d must be 1 x 1 without padding (kernel %s, padding %s)" % ((kh, kw), (ph, pw)))
    return tuple((t // kw, t % kw, t // kw - ph, t % kw - pw) for t in range(n))


def _taps_c(taps):
    arr = _TAPS_C.get(taps)
    if arr is None:
        flat = [int(v) for tap in taps for v in tap]
        arr = _TAPS_C[taps] = (ctypes.c_int * max(1, len(flat)))(*flat)
    return arr


class _CausalConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, taps):
        for name, t in (("x", x), ("weight", weight), ("bias", bias)):
            if t is None and name == "bias":
                continue
            if not torch.is_tensor(t) or t.device.type != "cuda" or t.dtype != torch.float32:
                raise MMVAEError("causal_conv2d: %s must be a float32 tensor on a gfx950 GPU (got %s): there is no CPU fallback"
                                 % (name, "%s, %s" % (t.device, t.dtype) if torch.is_tensor(t) else type(t).__name__))
        if x.dim() != 4 or weight.dim() != 4 or weight.shape[1] != x.shape[1] or weight.device != x.device:
            raise MMVAEError("causal_conv2d: x %s and weight %s do not fit: (B, Cin, H, W) and (Cout, Cin, kh, kw) on one device expected"
                             % (tuple(x.shape), tuple(weight.shape)))
        if bias is not None and (tuple(bias.shape) != (weight.shape[0],) or bias.device != x.device):
            raise MMVAEError("causal_conv2d: bias %s, need (%d,) on %s" % (tuple(bias.shape), weight.shape[0], x.device))
        taps = tuple(tuple(int(v) for v in tap) for tap in taps)
        if any(len(tap) != 4 for tap in taps):
            raise MMVAEError("causal_conv2d: a tap is (r, c, dy, dx)")
        (B, Cin, H, W), (Cout, _, kh, kw) = x.shape, weight.shape
        dims = (B, H, W, Cin, Cout, kh, kw)
        x, w = nhwc(x.detach()), weight.detach().contiguous()
        b = None if bias is None else bias.detach().contiguous()
        need = call("mmvae_causal_conv_workspace_bytes", *dims, len(taps))
        with torch.cuda.device(x.device):
            ws = _conv_ws(x.device, need)
            y = empty_nhwc(B, Cout, H, W, x.device)
            call("mmvae_causal_conv_forward", ptr(x), ptr(w), ptr(b), ptr(y), _taps_c(taps), len(taps), *dims, ptr(ws), ws.numel(), stream())
        ctx.save_for_backward(x, w)
        ctx.taps, ctx.dims, ctx.has_bias = taps, dims, bias is not None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        taps, dims = ctx.taps, ctx.dims
        B, H, W, Cin, Cout, kh, kw = dims
        g = nhwc(g)
        dx = dw = db = None
        with torch.cuda.device(x.device):
            ws = _conv_ws(x.device, call("mmvae_causal_conv_workspace_bytes", *dims, len(taps)))
            tail = (_taps_c(taps), len(taps)) + dims + (ptr(ws), ws.numel(), stream())
            if ctx.needs_input_grad[0]:
                dx = empty_nhwc(B, Cin, H, W, x.device)
                call("mmvae_causal_conv_backward_data", ptr(g), ptr(w), ptr(dx), *tail)
            want_w, want_b = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
            if want_w or want_b:
                dw = torch.empty_like(w) if want_w else None
                db = torch.empty(Cout, dtype=torch.float32, device=x.device) if want_b else None
                call("mmvae_causal_conv_backward_weight", ptr(g), ptr(x), ptr(dw), ptr(db), *tail)
        return dx, dw, db, None


def causal_conv2d(x, weight, bias, taps):
    """The convolution every layer of both models is, as a device op with HIP forward, data gradient and weight gradient.

    ``x`` (B, Cin, H, W) float32 (consumed channels-last), ``weight`` (Cout, Cin, kh, kw), ``bias`` (Cout,) or None, ``taps`` a tuple
    of ``(r, c, dy, dx)``: kernel cell (r, c) applied at offset (dy, dx) -> (B, Cout, H, W) float32, channels-last.  With bf16(.)
    round-to-nearest-even and fp32 accumulation, a position outside the image contributing nothing::

        y[b,co,i,j]       = bias[co] + sum_t sum_ci bf16(x[b,ci,i+dy_t,j+dx_t]) bf16(w[co,ci,r_t,c_t])
        dx[b,ci,i,j]      = sum_t sum_co bf16(g[b,co,i-dy_t,j-dx_t]) bf16(w[co,ci,r_t,c_t])
        dw[co,ci,r_t,c_t] = sum_{b,i,j} bf16(g[b,co,i,j]) bf16(x[b,ci,i+dy_t,j+dx_t]);   cells in no tap: exactly 0
        db[co]            = sum_{b,i,j} g[b,co,i,j]

    Once differentiable; gradients nobody asked for are not computed; two calls give identical bits.  Device-only: a CPU tensor
    raises ``MMVAEError``.  One deliberate difference to the torch path: there autograd gives masked weight cells a non-zero gradient
    (the next forward zeroes the cells again, but ``clip_grad_norm_`` counts it); here it is exactly 0, so a clipped norm is taken
    over the taps that exist."""
    return _CausalConv.apply(x, weight, bias, taps)


def set_conv_backend(model, backend):
    """Chooses what the convolutions of a ``PixelCNN`` / ``GatedPixelCNN`` run on: ``"torch"`` (the default) or ``"hip"``
    (``causal_conv2d``; the model has to be on the device by the time of its forward).  A plain attribute on the modules: no buffer,
    no parameter, the ``state_dict`` does not change.  Gates, ReLUs, residual adds and the loss stay torch ops.  -> model"""
    if backend not in CONV_BACKENDS:
        raise MMVAEError("set_conv_backend: %r, need one of %s" % (backend, CONV_BACKENDS))
    _config(model, "set_conv_backend")
    for m in _layers(model):
        m.conv_backend = backend
    return model


# ------------------------------------------------------------------------------------------------------ the fused head
HEADS = ("torch", "hip")


def head_nll_geometry() -> Tuple[int, int, int, int, int, int]:
    """(positions per workgroup, levels per tile, positions per dw / db chunk, largest hid, most levels, most positions)"""
    return geometry("mmvae_head_nll_geometry", 6)


def head_nll_workspace_bytes(B, C, H, W, hid, V) -> int:
    """device scratch one ``head_nll`` call needs; 0 when the shape is outside the op's limits (a host function: needs no GPU)"""
    return int(call("mmvae_head_nll_workspace_bytes", int(B), int(C), int(H), int(W), int(hid), int(V)))


def _head_dims(what, h, weight, bias, target, data_channels):
    """validates everything before anything is launched -> (B, C, H, W, hid, V)"""
    for name, t in (("h", h), ("weight", weight), ("bias", bias)):
        if not torch.is_tensor(t) or t.device.type != "cuda" or t.dtype != torch.float32:
            raise MMVAEError("%s: %s must be a float32 tensor on a gfx950 GPU (got %s): there is no CPU fallback"
                             % (what, name, "%s, %s" % (t.device, t.dtype) if torch.is_tensor(t) else type(t).__name__))
    if not torch.is_tensor(target) or target.dtype != torch.int64 or target.device != h.device:
        raise MMVAEError("%s: target must be an int64 tensor of levels on %s" % (what, h.device))
    C = int(data_channels)
    if h.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[1:]) != (h.shape[1], 1, 1) or C < 1 or weight.shape[0] % C != 0:
        raise MMVAEError("%s: h %s, weight %s, data_channels %d do not fit: (B, hid, H, W) and (V * C, hid, 1, 1) expected"
                         % (what, tuple(h.shape), tuple(weight.shape), C))
    (B, hid, H, W), V = h.shape, weight.shape[0] // C
    if tuple(bias.shape) != (V * C,) or tuple(target.shape) != (B, C, H, W) or weight.device != h.device or bias.device != h.device:
        raise MMVAEError("%s: bias %s, target %s: need (%d,) and %s on %s" % (what, tuple(bias.shape), tuple(target.shape), V * C,
                                                                             (B, C, H, W), h.device))
    if head_nll_workspace_bytes(B, C, H, W, hid, V) <= 0:
        _, _, _, max_hid, max_v, max_pos = head_nll_geometry()
        raise MMVAEError("%s: B = %d, C = %d, H = %d, W = %d, hid = %d, V = %d is outside what the kernels are built for (C 1 or 3, hid a "
                         "multiple of 8 up to %d, V 2..%d, B * H * W <= %d)" % (what, B, C, H, W, hid, V, max_hid, max_v, max_pos))
    return int(B), C, int(H), int(W), int(hid), int(V)


class _HeadNLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, weight, bias, target, data_channels):
        dims = _head_dims("head_nll", h, weight, bias, target, data_channels)
        B, C, H, W, hid, V = dims
        h, w, b, t = nhwc(h.detach()), weight.detach().contiguous(), bias.detach().contiguous(), target.contiguous()
        keep = any(ctx.needs_input_grad[:3])
        with torch.cuda.device(h.device):
            ws = _conv_ws(h.device, head_nll_workspace_bytes(*dims))
            nll = torch.empty(B, C, H, W, dtype=torch.float32, device=h.device)
            lse = torch.empty(B, C, H, W, dtype=torch.float32, device=h.device) if keep else None
            call("mmvae_head_nll_forward", ptr(h), ptr(w), ptr(b), ptr(t), ptr(nll), ptr(lse), *dims, ptr(ws), ws.numel(), stream())
        if keep:
            ctx.save_for_backward(h, w, b, t, lse)
        ctx.dims = dims
        return nll

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        h, w, b, t, lse = ctx.saved_tensors
        dims = ctx.dims
        B, C, H, W, hid, V = dims
        g = g.contiguous()
        want_h, want_w, want_b = ctx.needs_input_grad[:3]
        with torch.cuda.device(h.device):
            ws = _conv_ws(h.device, head_nll_workspace_bytes(*dims))
            dh = empty_nhwc(B, hid, H, W, h.device) if want_h else None
            dw = torch.empty_like(w) if want_w else None
            db = torch.empty_like(b) if want_b else None
            call("mmvae_head_nll_backward", ptr(h), ptr(w), ptr(b), ptr(t), ptr(lse), ptr(g), ptr(dh), ptr(dw), ptr(db), *dims, ptr(ws),
                 ws.numel(), stream())
        return dh, dw, db, None, None


def head_nll(h, weight, bias, target, data_channels):
    """The output head ``conv4`` and the cross entropy as one device op: the logits never exist in memory.

    ``h`` (B, hid, H, W) float32 (consumed channels-last), ``weight`` (V * C, hid, 1, 1) with output channel ``v * C + c`` = level v of
    data channel c, ``bias`` (V * C,), ``target`` (B, C, H, W) int64 levels -> ``nll`` (B, C, H, W) float32 in nats.  With bf16(.)
    round-to-nearest-even and fp32 accumulation, p = (b, i, j)::

        l[p,v,c]   = bias[vC+c] + sum_k bf16(h[p,k]) bf16(w[vC+c,k])
        lse[p,c]   = log sum_v exp(l[p,v,c])                                 (online, the running maximum subtracted)
        nll[p,c]   = lse[p,c] - l[p,target[p,c],c]                           (a target outside 0..V-1: NaN for that element)
        d[p,v,c]   = g[p,c] (exp(l[p,v,c] - lse[p,c]) - [v == target[p,c]])
        dh[p,k]    = sum_{v,c} bf16(d[p,v,c]) bf16(w[vC+c,k])
        dw[vC+c,k] = sum_p bf16(d[p,v,c]) bf16(h[p,k]);    db[vC+c] = sum_p d[p,v,c]

    Once differentiable; the backward recomputes the logits from ``h``, the weights and the saved ``lse``; gradients nobody asked for
    are not computed; no atomics, two calls give identical bits.  Limits: C 1 or 3, hid a multiple of 8 up to 256, V 2..256
    (``head_nll_geometry``).  Device-only: a CPU tensor raises ``MMVAEError``."""
    return _HeadNLL.apply(h, weight, bias, target, data_channels)


def check_head(model, head, what="nll"):
    """raises ``MMVAEError`` unless ``head`` can run on ``model`` (hip: the model within the op's limits)"""
    if head not in HEADS:
        raise MMVAEError("%s: head %r, need one of %s" % (what, head, HEADS))
    _, _, C, hid, V = _config(model, what)
    if head == "hip" and head_nll_workspace_bytes(1, C, 1, 1, hid, V) <= 0:
        _, _, _, max_hid, max_v, _ = head_nll_geometry()
        raise MMVAEError("%s: head 'hip' needs data_channels 1 or 3, hid_dims a multiple of 8 up to %d and out_dims 2..%d (got %d, %d, %d)"
                         % (what, max_hid, max_v, C, hid, V))


def nll(model, x, target=None, head="torch"):
    """Per-element negative log-likelihood of ``target`` (default ``(x * (out_dims - 1)).long()``) under ``model`` given ``x``:
    (B, C, H, W) in nats, differentiable.  ``head="torch"`` is ``log_softmax`` + gather on ``model(x)`` and runs anywhere;
    ``head="hip"`` is ``head_nll`` on ``model.features(x)`` (device-only), independent of ``set_conv_backend``."""
    check_head(model, head)
    if target is None:
        target = (x * (model.out_dims - 1)).long()
    if head == "hip":
        model.conv4.weight.data.mul_(model.conv4.mask)          # what a MaskedConv2d forward does
        return head_nll(model.features(x), model.conv4.weight, model.conv4.bias, target, model.data_channels)
    logp = F.log_softmax(model(x), dim=1)
    return -logp.gather(1, target.unsqueeze(1)).squeeze(1)


def bits_per_dim(nll):
    """(B, C, H, W) nats -> (B,) bits per dimension: the mean over C * H * W divided by ln 2"""
    return nll.flatten(1).mean(dim=1) / float(np.log(2.0))
