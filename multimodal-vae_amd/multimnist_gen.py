"""MultiMNIST made on the device (csrc/multimnist_gen.hip; the reference's ``multimnist/datasets.py``): the dataset files in one call
and a stream of fresh, never-repeating batches for training.

The input is MNIST as the ``.pt`` pair the MNIST family already reads, ``(uint8 (N,28,28), int64 (N,))`` -- torchvision's
``MNIST/processed/{training,test}.pt``.  Per canvas the reference draws 0 .. ``max_digits`` digits, resizes each with
``scipy.misc.imresize(digit, 1 / scale)``, scale ~ N(1.3, 0.1) (Pillow's 8-bit bilinear resample; SciPy removed the function), places it
at a random position of a 50 x 50 canvas and draws the whole canvas again when the sum passes 255.  The kernel does the same in integer
arithmetic, bit for bit the resize of Pillow, with counter-based draws (``csrc/mmgen_core.h`` states them): canvas ``first + i`` of a
seed is the same whatever the call that makes it.  The numpy MT19937 stream of the reference's fixed seed is NOT reproduced: the
canvases have the reference's distribution, not its images.  Device-only: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Iterator, List, Tuple

import torch

from ._lib import MMVAEError, call, ptr
from ._ops import geometry, stream
from .utils import FILL

F_FIXED, F_NO_RESIZE, F_NO_TRANSLATE, F_REVERSE, F_SCRAMBLE, F_NO_REPEAT = 1, 2, 4, 8, 16, 32
MODE_KEYS = ("fixed", "resize", "translate", "min_digits", "max_digits", "reverse", "scramble", "no_repeat")

_TABLES: Dict[int, torch.Tensor] = {}


def mmgen_geometry() -> Tuple[int, int, int, int, int, int]:
    """(smallest side, largest side, most taps of a resize coefficient row, attempts per canvas, redraws per ``no_repeat`` slot, canvas
    size)"""
    return geometry("mmvae_mmgen_geometry", 6)


def build_tables() -> torch.Tensor:
    """the resize coefficients and side thresholds as the int32 host tensor the kernels read (a host function: needs no GPU)"""
    buf = torch.zeros(int(call("mmvae_mmgen_table_bytes")) // 4, dtype=torch.int32)
    call("mmvae_mmgen_build_tables", ctypes.c_void_p(buf.data_ptr()))
    return buf


def _tables(dev: torch.device) -> torch.Tensor:
    """built once on the host, cached per device"""
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    t = _TABLES.get(idx)
    if t is None:
        t = _TABLES[idx] = build_tables().to(torch.device("cuda", idx))
    return t


def mode_flags(*, fixed=False, resize=True, translate=True, min_digits=0, max_digits=2, reverse=False, scramble=False,
               no_repeat=False) -> Tuple[int, int, int]:
    """-> (flags, min_digits, max_digits) of the C-ABI.  Refuses what the reference's command line refuses: ``no_repeat``, ``scramble``
    and ``reverse`` need ``fixed``; with both, ``scramble`` overrides ``reverse`` (datasets.py:302-313)."""
    for name, on in (("no_repeat", no_repeat), ("scramble", scramble), ("reverse", reverse)):
        if on and not fixed:
            raise MMVAEError("multimnist_gen: %s needs fixed=True (as the reference's --%s needs --fixed)" % (name, name))
    min_digits, max_digits = int(min_digits), int(max_digits)
    if not 0 <= min_digits <= max_digits <= 4:
        raise MMVAEError("multimnist_gen: min_digits = %d, max_digits = %d, need 0 <= min <= max <= 4" % (min_digits, max_digits))
    if reverse and scramble:
        reverse = False
    flags = (F_FIXED if fixed else 0) | (0 if resize else F_NO_RESIZE) | (0 if translate else F_NO_TRANSLATE) \
        | (F_REVERSE if reverse else 0) | (F_SCRAMBLE if scramble else 0) | (F_NO_REPEAT if no_repeat else 0)
    return flags, min_digits, max_digits


def _check_digits(what: str, digits_u8, labels=None) -> torch.device:
    named = (("digits_u8", digits_u8, torch.uint8),) + ((("labels", labels, torch.int64),) if labels is not None else ())
    for name, t, dt in named:
        if not torch.is_tensor(t) or t.device.type != "cuda" or t.dtype != dt:
            raise MMVAEError("%s: %s must be a %s tensor on a gfx950 GPU (got %s): there is no CPU fallback"
                             % (what, name, str(dt).replace("torch.", ""), "%s, %s" % (t.device, t.dtype) if torch.is_tensor(t) else type(t).__name__))
    if digits_u8.dim() != 3 or tuple(digits_u8.shape[1:]) != (28, 28) or len(digits_u8) < 1 or not digits_u8.is_contiguous():
        raise MMVAEError("%s: digits_u8 %s, need a contiguous (M >= 1, 28, 28)" % (what, tuple(digits_u8.shape)))
    if labels is not None and (labels.dim() != 1 or len(labels) != len(digits_u8) or labels.device != digits_u8.device or not labels.is_contiguous()):
        raise MMVAEError("%s: labels %s do not fit digits_u8 %s" % (what, tuple(labels.shape), tuple(digits_u8.shape)))
    return digits_u8.device


def _launch(digits_u8, labels, n, flags, lo, hi, seed, first, out, params, attempts, fail):
    """one mmvae_mmgen_generate on the caller's stream -> (images, text); nothing is read back"""
    dev = digits_u8.device
    with torch.cuda.device(dev):
        u8 = torch.empty((n, 50, 50), dtype=torch.uint8, device=dev) if out == "u8" else None
        f32 = torch.empty((n, 1, 50, 50), dtype=torch.float32, device=dev) if out == "f32" else None
        text = torch.empty((n, 4), dtype=torch.int64, device=dev)
        call("mmvae_mmgen_generate", ptr(digits_u8), ptr(labels), len(digits_u8), ptr(_tables(dev)), flags, lo, hi,
             ctypes.c_ulonglong(int(seed) & (2 ** 64 - 1)), ctypes.c_ulonglong(int(first) & (2 ** 64 - 1)), n, ptr(u8), ptr(f32), ptr(text),
             ptr(params), ptr(attempts), ptr(fail), stream())
    return (u8 if out == "u8" else f32), text


def generate(digits_u8, labels, n, *, seed=0, first=0, fixed=False, resize=True, translate=True, min_digits=0, max_digits=2, reverse=False,
             scramble=False, no_repeat=False, out="u8", return_params=False):
    """``n`` canvases, the global canvases ``first .. first + n - 1`` of ``seed``, from the MNIST digits ``digits_u8`` (M,28,28) uint8 and
    ``labels`` (M,) int64 in 0..9, both on the device -> ``(images, text)``: images uint8 (n,50,50) (``out="u8"``, the dataset file's
    layout) or float32 (n,1,50,50) = u8 / 255 (``out="f32"``, what ``ToTensor`` gives); text int64 (n,4), ``FILL`` past the digits.
    With ``return_params`` also ``params`` int32 (n,4,4) = (digit index or -1, side, top, left) per slot, the argument of ``render``, and
    ``attempts`` int32 (n,), the 1-based number of the accepted attempt.

    The mode arguments are the reference's: random mode (``resize``, ``translate``: ``--no_resize`` gives side 28, ``--no_translate`` the
    centre) or ``fixed`` (side 21 at four fixed places, with ``reverse``, ``scramble``, ``no_repeat``).

    A canvas that is still rejected after ``mmgen_geometry()[3]`` attempts is zeros with FILL text and ``attempts`` 0 (the reference
    would recurse for ever); the call then raises ``MMVAEError`` naming how many failed, so it reads one int back: use
    ``MultiMNISTStream`` where no host synchronisation per batch is wanted.  Device-only: a CPU tensor raises ``MMVAEError``."""
    flags, lo, hi = mode_flags(fixed=fixed, resize=resize, translate=translate, min_digits=min_digits, max_digits=max_digits,
                               reverse=reverse, scramble=scramble, no_repeat=no_repeat)
    if out not in ("u8", "f32"):
        raise MMVAEError("multimnist_gen.generate: out %r, need 'u8' or 'f32'" % (out,))
    dev = _check_digits("multimnist_gen.generate", digits_u8, labels)
    n = int(n)
    if n < 0 or int(first) < 0:
        raise MMVAEError("multimnist_gen.generate: n = %d, first = %d" % (n, int(first)))
    params = torch.empty((n, 4, 4), dtype=torch.int32, device=dev) if return_params else None
    attempts = torch.empty((n,), dtype=torch.int32, device=dev) if return_params else None
    fail = torch.zeros(1, dtype=torch.int32, device=dev)
    images, text = _launch(digits_u8, labels, n, flags, lo, hi, seed, first, out, params, attempts, fail)
    failed = int(fail.item())
    if failed:
        err = MMVAEError("multimnist_gen.generate: %d of %d canvases were still rejected after %d attempts (overlapping digits pass 255 "
                         "every time): they are zeros with FILL text" % (failed, n, mmgen_geometry()[3]))
        err.failed, err.result = failed, (images, text, params, attempts)
        raise err
    return (images, text, params, attempts) if return_params else (images, text)


def render(digits_u8, params, out="u8"):
    """The canvases of an explicit table: ``params`` int32 (n,4,4) = (digit index or -1 for an absent slot, side, top, left) ->
    ``(images, overflow)``: the digits resized and summed exactly as ``generate`` does, without draws and without rejection; the sum is
    clamped to 255 and ``overflow`` int32 (n,) is 1 where that happened.  Limits (``mmgen_geometry``): side 14..41, top + side <= 50,
    left + side <= 50, index < M; checked here before the launch (one read-back of ``params``)."""
    dev = _check_digits("multimnist_gen.render", digits_u8)
    if out not in ("u8", "f32"):
        raise MMVAEError("multimnist_gen.render: out %r, need 'u8' or 'f32'" % (out,))
    if not torch.is_tensor(params) or params.device != dev or params.dtype != torch.int32 or params.dim() != 3 or tuple(params.shape[1:]) != (4, 4):
        raise MMVAEError("multimnist_gen.render: params must be an int32 (n,4,4) tensor on the digits' device: there is no CPU fallback")
    params = params.contiguous()
    lo, hi = mmgen_geometry()[:2]
    p = params.cpu()
    idx, side, top, left = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    bad = (idx >= 0) & ((idx >= len(digits_u8)) | (side < lo) | (side > hi) | (top < 0) | (left < 0) | (top + side > 50) | (left + side > 50))
    if bool(bad.any()):
        i, j = (int(v) for v in bad.nonzero()[0])
        raise MMVAEError("multimnist_gen.render: canvas %d slot %d = %s is out of range: index < %d, side %d..%d, top, left >= 0, top + side "
                         "<= 50, left + side <= 50" % (i, j, p[i, j].tolist(), len(digits_u8), lo, hi))
    n = len(params)
    with torch.cuda.device(dev):
        u8 = torch.empty((n, 50, 50), dtype=torch.uint8, device=dev) if out == "u8" else None
        f32 = torch.empty((n, 1, 50, 50), dtype=torch.float32, device=dev) if out == "f32" else None
        overflow = torch.empty((n,), dtype=torch.int32, device=dev)
        call("mmvae_mmgen_render", ptr(digits_u8), len(digits_u8), ptr(_tables(dev)), ptr(params), n, ptr(u8), ptr(f32), ptr(overflow), stream())
    return (u8 if out == "u8" else f32), overflow


def label_lists(text: torch.Tensor) -> List[List[int]]:
    """(n,4) FILL-padded text -> the reference's label lists (``data.save_multimnist``)"""
    return [[v for v in row if v != FILL] for row in text.cpu().tolist()]


def make_dataset(root, mnist_train, mnist_test, *, n_train=60000, n_test=10000, seed=0, device=None, **mode) -> Tuple[str, str]:
    """Writes ``<root>/processed/{training,test}.pt`` in the reference's format (``data.save_multimnist``): ``n_train`` canvases from the
    MNIST training digits and ``n_test`` from the test digits (60,000 + 10,000 as ``datasets.py:175-178``), one call each.
    ``mnist_train`` / ``mnist_test``: ``(uint8 (N,28,28), int64 (N,))`` pairs, on the host or the device.  The test canvases continue
    the training split's canvas numbering, so the two never share a draw.  -> the two paths."""
    from . import data as D
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    paths = []
    for train, (digits, labels), n, first in ((True, mnist_train, int(n_train), 0), (False, mnist_test, int(n_test), int(n_train))):
        digits, labels = digits.to(dev).contiguous(), labels.to(dev, torch.int64).contiguous()
        images, text = generate(digits, labels, n, seed=seed, first=first, **mode)
        paths.append(D.save_multimnist(root, train, images.cpu(), label_lists(text)))
    return paths[0], paths[1]


class MultiMNISTStream:
    """Iterates fresh ``(image float32 (B,1,50,50), text int64 (B,4))`` device batches: batch ``b`` of epoch ``e`` (``e`` counts the
    iterations of this object) is ``generate(first=(e * len + b) * B, n=B, out="f32")``, so no canvas is ever repeated and a second
    stream with the same seed repeats the first.

    A batch is ONE kernel on the caller's current stream, in front of the step that reads it: no copy stream, no event, no edge between
    streams (``data.DeviceBatcher`` says what those cost), no host synchronisation per step.  The batch tensors are the caller's own.
    Failed canvases (``generate``) are counted on the device; ``check()`` reads the counter once and raises ``MMVAEError`` if it is not
    zero; it is called at the end of every epoch."""

    def __init__(self, digits_u8, labels, batch_size, device, epoch_size=60000, seed=0, **mode):
        self.flags, self.lo, self.hi = mode_flags(**mode)
        self.device = torch.device(device)
        self.digits, self.labels = digits_u8.to(self.device).contiguous(), labels.to(self.device, torch.int64).contiguous()
        _check_digits("MultiMNISTStream", self.digits, self.labels)
        if int(self.labels.min()) < 0 or int(self.labels.max()) > 9:
            raise MMVAEError("MultiMNISTStream: labels must be digits 0..9")
        self.B, self.n_batches, self.seed, self.epoch = int(batch_size), int(epoch_size) // int(batch_size), int(seed), 0
        if self.B < 1:
            raise MMVAEError("MultiMNISTStream: batch_size = %d" % self.B)
        self.fail = torch.zeros(1, dtype=torch.int32, device=self.device)
        _tables(self.device)

    def __len__(self) -> int:
        return self.n_batches

    def batch(self, index: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """global batch ``index`` = canvases ``index * B ..``, on the caller's stream"""
        return _launch(self.digits, self.labels, self.B, self.flags, self.lo, self.hi, self.seed, index * self.B, "f32", None, None, self.fail)

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        e = self.epoch
        self.epoch += 1
        for b in range(self.n_batches):
            yield self.batch(e * self.n_batches + b)
        self.check()

    def check(self) -> None:
        failed = int(self.fail.item())
        if failed:
            self.fail.zero_()
            raise MMVAEError("MultiMNISTStream: %d canvases were still rejected after %d attempts and were emitted as zeros"
                             % (failed, mmgen_geometry()[3]))


__all__ = ["generate", "render", "make_dataset", "MultiMNISTStream", "mmgen_geometry", "build_tables", "mode_flags", "label_lists"]
