"""``transforms.Scale(size)`` + ``CenterCrop(size)`` + ``ToTensor()`` of the reference's image pipelines (``celeba/train.py:102-104``,
``coco/train.py:107-112``) on the device (csrc/imgprep.hip): a ragged batch of decoded RGB images in, ``(n, 3, size, size)`` out, in
one launch.

The result is bit for bit what torchvision's transforms of that era give over Pillow's 8-bit BILINEAR resample
(``csrc/imgprep_core.h`` states the arithmetic): the image is scaled so that its SHORTER side becomes ``size`` (``scaled_size``), with
Pillow's widened support when that shrinks it, and the centre ``size`` x ``size`` window is cut out (``crop_offset``).  Only that
window is computed.  torchvision is not needed and Pillow only decodes files; neither is imported here.  Device-only: there is no CPU
fallback.
"""
from __future__ import annotations

import ctypes
from typing import List, Sequence, Tuple

import numpy as np
import torch

from ._lib import MMVAEError, call, ptr
from ._ops import geometry, stream


def imgprep_geometry() -> Tuple[int, int, int]:
    """(largest input side, largest output side, fixed-point bits of a coefficient)"""
    return geometry("mmvae_imgprep_geometry", 3)


def scaled_size(w: int, h: int, size: int) -> Tuple[int, int]:
    """``Scale(size)`` -> (ow, oh): the shorter side becomes ``size``, the other ``int(size * long / short)``"""
    w, h, size = int(w), int(h), int(size)
    if w < 1 or h < 1 or size < 1:
        raise MMVAEError("imgprep.scaled_size: w = %d, h = %d, size = %d" % (w, h, size))
    if w <= h:
        return size, size * h // w          # (the truncated float quotient is the integer quotient: csrc/imgprep_core.h)
    return size * w // h, size


def crop_offset(d: int) -> int:
    """``CenterCrop``'s ``int(round(d / 2.))`` of that era (Python 2: halves round away from zero) for a difference d >= 0"""
    d = int(d)
    if d < 0:
        raise MMVAEError("imgprep.crop_offset: d = %d" % d)
    return (d + 1) // 2


def coefficients(n_in: int, n_out: int, first: int = 0, count: int = None):
    """The host build of the kernel's own coefficient functions (needs no GPU) -> (xmin int32 (count,), taps int32 (count,), coefs
    int32 (count, most taps)) for the output indices ``first .. first + count - 1`` of an axis ``n_in -> n_out``."""
    count = int(n_out) - int(first) if count is None else int(count)
    stride = min(int(n_in), 2 * (max(int(n_in), int(n_out)) // max(int(n_out), 1)) + 4)
    xmin, taps = np.zeros(count, dtype=np.int32), np.zeros(count, dtype=np.int32)
    coefs = np.zeros((count, stride), dtype=np.int32)
    call("mmvae_imgprep_coeffs", int(n_in), int(n_out), int(first), count, stride, ctypes.c_void_p(xmin.ctypes.data),
         ctypes.c_void_p(taps.ctypes.data), ctypes.c_void_p(coefs.ctypes.data))
    return xmin, taps, coefs[:, :max(int(taps.max()), 1) if count else 1]


def pack_images(arrays: Sequence) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """A list of (h, w, 3) uint8 arrays (``numpy.asarray`` of a PIL RGB image) or tensors -> pinned host tensors ``(pixels uint8 (bytes,),
    offsets int64 (n,), heights int32 (n,), widths int32 (n,))``: the images back to back, each from a 16-byte aligned offset."""
    hs, ws, offs, total = [], [], [], 0
    arrs = []
    for i, a in enumerate(arrays):
        a = a.numpy() if torch.is_tensor(a) else np.asarray(a)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
            raise MMVAEError("imgprep.pack_images: image %d is %s %s, need uint8 (h, w, 3)" % (i, a.dtype, a.shape))
        arrs.append(a)
        hs.append(a.shape[0])
        ws.append(a.shape[1])
        offs.append(total)
        total += (a.size + 15) // 16 * 16
    pin = torch.cuda.is_available()
    pixels = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=pin)
    flat = pixels.numpy()
    for a, o in zip(arrs, offs):
        flat[o:o + a.size] = a.reshape(-1)

    def small(v, dt):
        t = torch.tensor(v, dtype=dt)
        return t.pin_memory() if pin else t
    return pixels, small(offs, torch.int64), small(hs, torch.int32), small(ws, torch.int32)


def check_descriptors(pixels_bytes: int, offsets, heights, widths, where="imgprep") -> None:
    """what the kernel refuses, checked on the host (which has the sizes anyway): raises ``MMVAEError`` naming the first image"""
    max_side = imgprep_geometry()[0]
    o, h, w = (np.asarray(t.cpu() if torch.is_tensor(t) else t, dtype=np.int64) for t in (offsets, heights, widths))
    if not (o.shape == h.shape == w.shape and o.ndim == 1):
        raise MMVAEError("%s: offsets, heights and widths must be 1-D and of one length" % where)
    bad = (h < 1) | (h > max_side) | (w < 1) | (w > max_side) | (o < 0) | (o + 3 * h * w > int(pixels_bytes))
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise MMVAEError("%s: image %d (h = %d, w = %d, offset %d) is unusable: sides must be 1..%d and offset + 3 h w <= %d bytes"
                         % (where, i, h[i], w[i], o[i], max_side, int(pixels_bytes)))


def scale_center_crop(images_or_packed, size: int, out: str = "u8", device=None) -> torch.Tensor:
    """``images_or_packed``: a list of (h, w, 3) uint8 images, or the 4-tuple of ``pack_images`` (host or device tensors) ->
    uint8 (n, 3, size, size) (``out="u8"``) or float32 = u8 / 255 (``out="f32"``, what ``ToTensor`` gives) on the device.

    One launch for the whole batch; a batch does not change an image's result.  The descriptors are checked here on the host and once
    more by the kernel, which refuses an unusable image (zeros, status -1) without reading it; any non-zero status raises
    ``MMVAEError`` naming the image.  Device-only: there is no CPU fallback."""
    if out not in ("u8", "f32"):
        raise MMVAEError("imgprep.scale_center_crop: out %r, need 'u8' or 'f32'" % (out,))
    max_side, max_out, _ = imgprep_geometry()
    size = int(size)
    if not 1 <= size <= max_out:
        raise MMVAEError("imgprep.scale_center_crop: size = %d, need 1..%d" % (size, max_out))
    if not torch.cuda.is_available():
        raise MMVAEError("imgprep.scale_center_crop runs on a gfx950 GPU only: there is no CPU fallback")
    packed = images_or_packed if (isinstance(images_or_packed, tuple) and len(images_or_packed) == 4
                                  and all(torch.is_tensor(t) for t in images_or_packed)) else pack_images(list(images_or_packed))
    pixels, offsets, heights, widths = packed
    if pixels.dtype != torch.uint8 or offsets.dtype != torch.int64 or heights.dtype != torch.int32 or widths.dtype != torch.int32:
        raise MMVAEError("imgprep.scale_center_crop: packed = (uint8 pixels, int64 offsets, int32 heights, int32 widths)")
    n = len(offsets)
    check_descriptors(pixels.numel(), offsets, heights, widths, "imgprep.scale_center_crop")
    dev = torch.device(device) if device is not None else (pixels.device if pixels.device.type == "cuda"
                                                            else torch.device("cuda", torch.cuda.current_device()))
    result = torch.empty((n, 3, size, size), dtype=torch.uint8 if out == "u8" else torch.float32, device=dev)
    if n == 0:
        return result
    with torch.cuda.device(dev):
        d_pix, d_off, d_h, d_w = (t.contiguous().to(dev, non_blocking=True) for t in (pixels.view(-1), offsets, heights, widths))
        status = torch.empty(n, dtype=torch.int32, device=dev)
        call("mmvae_imgprep_scale_crop", ptr(d_pix), d_pix.numel(), ptr(d_off), ptr(d_h), ptr(d_w), n, size,
             ptr(result) if out == "u8" else None, ptr(result) if out == "f32" else None, ptr(status), stream())
        bad = status.cpu().nonzero()
    if len(bad):
        i = int(bad[0])
        raise MMVAEError("imgprep.scale_center_crop: the kernel refused image %d (h = %d, w = %d, offset %d): status %d"
                         % (i, int(heights[i]), int(widths[i]), int(offsets[i]), int(status[i])))
    return result


__all__ = ["scaled_size", "crop_offset", "pack_images", "scale_center_crop", "check_descriptors", "coefficients", "imgprep_geometry"]
