"""Yardsticks for the causal tap-list convolution (``pixelcnn.causal_conv2d``), independent of the package's op and of ``taps_of``.

``taps_ref``      the tap list of a masked / vertical / horizontal / 1 x 1 convolution, written from ``pixelcnn_ref.mask`` and from the
                  one-sided padding of ``pixelcnn_ref._gated_block``
``tapconv``       the convolution by padding and shifting, in any dtype, differentiable by autograd
``tapconv_dx``,
``tapconv_dw``    its two gradients written out; ``fault`` injects what an implementation can get wrong (FAULTS)
``reference``     forward and the four gradients in float64 on bf16-rounded operands, the same in float32 (the yardstick), the gates
``QConv``         float64 convolution that rounds x, w and, in backward, g to bf16 as the op does; ``emulated_forward`` runs
                  ``pixelcnn_ref.forward`` on it
"""
import contextlib

import torch
import torch.nn.functional as F

import pixelcnn_ref as R

GATE_FACTOR = R.GATE_FACTOR
FAULTS = ("drop_tap", "col_off", "row_off", "no_round", "swap_dgrad", "masked_grad", "border_bias", "last_chunk")
KINDS = ("A", "B", "vertical", "horizontal", "one")


def round_bf16(t):
    """round to nearest even to bf16, back in the dtype it came in (exact for what float32 holds)"""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def taps_ref(kind, kh, kw):
    """(r, c, dy, dx) per kept cell.  A / B: the cells ``pixelcnn_ref.mask`` keeps, centre padding.  vertical: a (kh, kw) kernel over
    an input padded by kh rows on top only (row i sees rows i - kh .. i - 1) and kw // 2 columns on both sides.  horizontal: a
    (1, kw) kernel over an input padded by kw columns on the left only (column j sees j - kw .. j - 1).  one: a 1 x 1 kernel."""
    if kind in ("A", "B"):
        m = R.mask(kind, kh, kw)
        return tuple((r, c, r - kh // 2, c - kw // 2) for r in range(kh) for c in range(kw) if m[r, c] != 0)
    if kind == "vertical":
        return tuple((r, c, r - kh, c - kw // 2) for r in range(kh) for c in range(kw))
    if kind == "horizontal":
        assert kh == 1
        return tuple((0, c, 0, c - kw) for c in range(kw))
    assert kind == "one" and (kh, kw) == (1, 1)
    return ((0, 0, 0, 0),)


def shift(x, dy, dx):
    """s[..., i, j] = x[..., i + dy, j + dx], 0 outside"""
    H, W = x.shape[-2:]
    m = max(abs(dy), abs(dx), 1)
    return F.pad(x, (m, m, m, m))[..., m + dy:m + dy + H, m + dx:m + dx + W]


def _faulty_taps(taps, fault):
    taps = list(taps)
    if fault == "drop_tap":
        taps = taps[:-1]
    elif fault == "col_off":
        taps[-1] = taps[-1][:3] + (taps[-1][3] - 1,)
    elif fault == "row_off":
        taps[-1] = taps[-1][:2] + (taps[-1][2] - 1, taps[-1][3])
    return taps


def tapconv(x, w, b, taps, fault=None):
    y = torch.zeros(x.shape[0], w.shape[0], x.shape[2], x.shape[3], dtype=x.dtype)
    outside = torch.zeros(x.shape[2], x.shape[3], dtype=torch.bool)
    for r, c, dy, dx in _faulty_taps(taps, fault):
        y = y + torch.einsum("bchw,oc->bohw", shift(x, dy, dx), w[:, :, r, c])
        outside |= shift(torch.ones(x.shape[2], x.shape[3]), dy, dx) == 0
    bias = b.view(1, -1, 1, 1).expand_as(y)
    if fault == "border_bias":
        bias = bias * (~outside).to(x.dtype)
    return y + bias


def tapconv_dx(g, w, taps, fault=None):
    dx = torch.zeros(g.shape[0], w.shape[1], g.shape[2], g.shape[3], dtype=g.dtype)
    for r, c, dy, dx_ in _faulty_taps(taps, fault):
        wt = w[:, :, r, c]
        if fault == "swap_dgrad":
            assert wt.shape[0] == wt.shape[1]
            wt = wt.t()
        dx = dx + torch.einsum("bohw,oc->bchw", shift(g, -dy, -dx_), wt)
    return dx


def tapconv_dw(g, x, wshape, taps, fault=None, chunk=None):
    """``last_chunk``: the positions of the last chunk of ``chunk`` (raster order over b, i, j) are left out"""
    dw = torch.zeros(wshape, dtype=g.dtype)
    if fault == "last_chunk":
        P = g.shape[0] * g.shape[2] * g.shape[3]
        keep = (torch.arange(P) < ((P - 1) // chunk) * chunk).view(g.shape[0], 1, g.shape[2], g.shape[3]).to(g.dtype)
        g = g * keep
    for r, c, dy, dx in _faulty_taps(taps, fault):
        dw[:, :, r, c] = torch.einsum("bohw,bchw->oc", g, shift(x, dy, dx))
    if fault == "masked_grad":
        kh, kw = wshape[2:]
        free = [(r, c) for r in range(kh) for c in range(kw) if (r, c) not in {(t[0], t[1]) for t in taps}]
        if free:
            r, c = free[0]
            dw[:, :, r, c] = torch.einsum("bohw,bchw->oc", g, shift(x, r - kh // 2, c - kw // 2))
    return dw


def all_four(x, w, b, g, taps, dtype, fault=None, chunk=None):
    """(y, dx, dw, db) in ``dtype`` from float32 operands, rounded to bf16 as the op rounds them (db from the unrounded g)"""
    rnd = (lambda t: t) if fault == "no_round" else round_bf16
    xq, wq, gq = rnd(x).to(dtype), rnd(w).to(dtype), rnd(g).to(dtype)
    return {"y": tapconv(xq, wq, b.to(dtype), taps, fault), "dx": tapconv_dx(gq, wq, taps, fault),
            "dw": tapconv_dw(gq, xq, w.shape, taps, fault, chunk), "db": g.to(dtype).sum(dim=(0, 2, 3))}


def reference(x, w, b, g, taps):
    """-> (float64 results, gates): gate = GATE_FACTOR x max(yardstick, 2^-23 max |reference|), the yardstick being the error of the
    same computation in float32 on the CPU, the floor half an ulp of the stored fp32 result"""
    ref = all_four(x, w, b, g, taps, torch.float64)
    f32 = all_four(x, w, b, g, taps, torch.float32)
    yard = {k: float((f32[k].double() - ref[k]).abs().max()) for k in ref}
    gates = {k: GATE_FACTOR * max(yard[k], 2.0 ** -23 * float(ref[k].abs().max())) for k in ref}
    return ref, yard, gates


def operands(B, Cin, Cout, H, W, kh, kw, seed=0):
    """float32 x, w, b and an upstream gradient g, seeded"""
    gen = torch.Generator().manual_seed(4242 + seed)
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, kh, kw, generator=gen) / (Cin * kh * kw) ** 0.5
    b = torch.rand(Cout, generator=gen) - 0.5
    g = torch.randn(B, Cout, H, W, generator=gen)
    return x, w, b, g


# ------------------------------------------------------------------------------------------------------ the emulated model
class QConv(torch.autograd.Function):
    """``F.conv2d(x, w) + b`` in float64 on operands rounded to bf16 (x, w; in backward g too), as the op computes it.  The bias
    gradient comes from the unrounded g."""

    @staticmethod
    def forward(ctx, x, w, b):
        xq, wq = round_bf16(x), round_bf16(w)
        ctx.save_for_backward(xq, wq)
        return F.conv2d(xq, wq) + b.view(1, -1, 1, 1)

    @staticmethod
    def backward(ctx, g):
        xq, wq = ctx.saved_tensors
        gq = round_bf16(g)
        return (torch.nn.grad.conv2d_input(xq.shape, wq, gq), torch.nn.grad.conv2d_weight(xq, wq.shape, gq), g.sum(dim=(0, 2, 3)))


def _qconv(sd, name, x, kind=None, pad=(0, 0, 0, 0)):
    w = sd[name + ".weight"].to(x.dtype)
    if kind is not None:
        w = w * R.mask(kind, w.shape[2], w.shape[3], x.dtype)
    return QConv.apply(F.pad(x, pad), w, sd[name + ".bias"].to(x.dtype))


@contextlib.contextmanager
def _emulating():
    keep = R._conv
    R._conv = _qconv
    try:
        yield
    finally:
        R._conv = keep


def emulated_forward(sd, cfg, x):
    """``pixelcnn_ref.forward`` with every convolution a ``QConv``"""
    with _emulating():
        return R.forward(sd, cfg, x)
