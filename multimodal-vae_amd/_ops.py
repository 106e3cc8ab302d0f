"""What the wrappers of the stand-alone device ops share: the caller's stream, the geometry call, the workspace caches and the
channels-last helpers.  No wrapper imports a private name from another wrapper or from a model file; they meet here."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import torch

from ._lib import call


def stream():
    """the caller's current stream as the ``void*`` every entry point takes last"""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def geometry(name: str, n: int) -> Tuple[int, ...]:
    """calls ``name(int* x n)`` -> the n values"""
    v = [ctypes.c_int() for _ in range(n)]
    call(name, *[ctypes.byref(a) for a in v])
    return tuple(a.value for a in v)


class WorkspaceCache:
    """uint8 device buffers keyed by (device index, current stream handle, *key).

    ``max_entries`` = n: a buffer of exactly ``need`` bytes per key, n keys at most, the oldest inserted evicted first.
    ``max_entries`` = None: grow-only scratch, one buffer per key, at least 1 MiB, rounded up to 16 bytes, reallocated only when too
    small."""

    def __init__(self, max_entries: Optional[int]):
        self.max_entries = max_entries
        self.buffers: Dict[Tuple, torch.Tensor] = {}

    def get(self, dev: torch.device, need: int, *key) -> torch.Tensor:
        key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream) + key
        ws = self.buffers.get(key)
        if self.max_entries is None:
            if ws is None or ws.numel() < need:
                ws = self.buffers[key] = torch.empty((max(need, 1 << 20) + 15) // 16 * 16, dtype=torch.uint8, device=dev)
        elif ws is None:
            while len(self.buffers) >= self.max_entries:
                self.buffers.pop(next(iter(self.buffers)))
            ws = self.buffers[key] = torch.empty(need, dtype=torch.uint8, device=dev)
        return ws


# the scratch of the convolution ops and the fused head (causal_conv2d, head_nll, down4s2 / up4s2): ``CONV_WS.get(dev, need)``
CONV_WS = WorkspaceCache(None)


def nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def empty_nhwc(B, C, H, W, dev):
    # (not a permuted view: an in-place ReLU on the op's output has to stay legal)
    return torch.empty((B, C, H, W), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
