"""PixelCNN / GatedPixelCNN (``coco/model.py:405-585``, the same family in ``mnist/model.py``) and a one-launch incremental
sampler for them (csrc/pixelcnn.hip).

The modules are plain torch: constructor signatures, attribute names and ``state_dict`` keys are those of ``coco/model.py``, so a
reference checkpoint loads; they run wherever torch runs and train through autograd.  The forward returns
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
        return self._conv_forward(x, self.weight, self.bias)


class CroppedConv2d(nn.Conv2d):
    """A side padded by the whole kernel size loses its last kernel size + 1 outputs: what is left sees strictly earlier rows
    (columns) of the input."""

    def forward(self, x):
        y = self._conv_forward(x, self.weight, self.bias)
        rows, cols = y.shape[2:]
        if self.padding[0] == self.kernel_size[0]:
            rows -= self.kernel_size[0] + 1
        if self.padding[1] == self.kernel_size[1]:
            cols -= self.kernel_size[1] + 1
        return y[:, :, :rows, :cols]


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
        return _gate(self.vertical_gate_conv(above)), self.horizontal_output(_gate(self.horizontal_gate_conv(left)))


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

    def forward(self, x):
        x = self.conv1(x)
        x = self.blocks(x)
        x = F.relu(self.conv2(x))
        x = self.conv4(x)
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

    def forward(self, x):
        x, h = self.conv1(x, x)
        _, h = self.blocks(x, h)
        h = self.conv2(F.relu(h))
        h = self.conv4(F.relu(h))
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
_WS: Dict[Tuple, torch.Tensor] = {}
_WS_MAX = 4          # cached workspaces (the oldest goes first)


def pixelcnn_geometry() -> Tuple[int, int, int]:
    """(samples per workgroup, largest hid_dims, largest side) of the kernel"""
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    call("mmvae_pixelcnn_geometry", ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return a.value, b.value, c.value


def _config(model) -> Tuple[int, int, int, int, int]:
    if isinstance(model, GatedPixelCNN):
        gated, hid = 1, model.conv2.weight.shape[0]
    elif isinstance(model, PixelCNN):
        gated, hid = 0, model.hid_dims
    else:
        raise MMVAEError("generate: a PixelCNN or GatedPixelCNN expected (got %s)" % type(model).__name__)
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
        call("mmvae_pixelcnn_pack_weights", *cfg, ptr(flat), flat.numel(), ptr(packed), _stream())
    return packed


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _workspace(dev, cfg, B, H, W):
    need = call("mmvae_pixelcnn_workspace_bytes", *cfg, B, H, W)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream, cfg, B, H, W)
    ws = _WS.get(key)
    if ws is None:
        while len(_WS) >= _WS_MAX:
            _WS.pop(next(iter(_WS)))
        ws = _WS[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    return ws, need


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
             ptr(image), ptr(logits), _stream())
    return PixelSample(image, levels.long(), logits)
