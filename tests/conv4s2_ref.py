"""Yardsticks for the 4 x 4 stride-2 convolution / transposed convolution op (``conv4s2.down4s2`` / ``up4s2``), independent of the package.

``down`` / ``up`` / ``dw``  the three products written out by padding and strided slicing, in any dtype; ``fault`` injects what an
                           implementation can get wrong (FAULTS)
``act`` / ``gp``           the activation and the gradient in front of it from the upstream gradient g and the SAVED OUTPUT y
``all_``                   forward, dx and dw of one direction in a dtype, on operands rounded to bf16 as the op rounds them
``reference``              the same in float64, in float32 (the yardstick), and the gates
``qdown`` / ``qup``        float64 convolutions that round x, w and, in backward, the gradient operand to bf16 as the op does;
                           ``infovae_forward`` runs the model on them; the ``formula_*`` helpers rebuild the fixture's weights and inputs

Cs = channels on the high-resolution side S (Hs x Ws), Cl = channels on the low-resolution side L (Hs/2 x Ws/2); w is (Cl, Cs, 4, 4).
"""
import torch
import torch.nn.functional as F

import pixelcnn_ref as R

GATE_FACTOR = R.GATE_FACTOR              # the project's margin for another summation order
ACTS = ("none", "relu", "leaky", "sigmoid")
FAULTS = ("parity", "drop_cell", "row_off", "col_off", "no_round", "transpose_up", "no_slope", "gp_sign_g", "border", "last_chunk")
CELL = (2, 1)                            # the cell the single-cell faults hit: inside the image at every shape, a 2 x 2 image included
CHUNK = 512                              # L positions per weight-gradient partial (checked against conv4s2_geometry on the GPU)

# (B, Cs, Cl, Hs, Ws)
SHAPES = [(1, 1, 1, 2, 2),               # one output position, every cell at a border
          (2, 1, 64, 28, 28),            # the model's outer pair
          (3, 64, 128, 14, 14),          # the model's inner pair
          (2, 3, 5, 4, 10),              # odd channel counts, not square
          (5, 8, 16, 6, 2),              # one output column
          (1, 128, 128, 4, 4),           # the channel limit
          (17, 16, 8, 2, 6),             # B across a tile boundary, Cl < Cs
          (4, 72, 40, 8, 8),             # channels that are no multiple of 16 or 32
          (3, 1, 5, 6, 4),               # the one-channel path with a channel count that is no multiple of 4
          (2, 1, 128, 4, 4)]             # the one-channel path at the channel limit


def chunk_shape(chunk=CHUNK, cs=8):
    """a shape whose B * Hs/2 * Ws/2 is one more than a weight-gradient chunk: the largest image of sides <= 32 that divides it"""
    best = max((h * w, h, w) for h in range(1, 33) for w in range(1, 33) if (chunk + 1) % (h * w) == 0)
    return ((chunk + 1) // best[0], cs, 16, 2 * best[1], 2 * best[2])


def slope32(slope):
    """the leaky slope as the float32 the op receives"""
    return float(torch.tensor(slope, dtype=torch.float32))


def round_bf16(t):
    """round to nearest even to bf16, back in the dtype it came in (exact for what float32 holds)"""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def _pad(t, n, fault):
    """n zeros around the image; the ``border`` fault lets the first ring repeat the edge instead"""
    if fault == "border":
        t = F.pad(t, (1, 1, 1, 1), mode="replicate")
        n -= 1
    return F.pad(t, (n, n, n, n))


def _cells(fault):
    for ky in range(4):
        for kx in range(4):
            if fault == "drop_cell" and (ky, kx) == CELL:
                continue
            hit = (ky, kx) == CELL
            yield ky, kx, (1 if fault == "row_off" and hit else 0), (1 if fault == "col_off" and hit else 0)


def _window(sp, ky, kx, dy, dx, H, W):
    """S padded by 2 -> the (H, W) source positions (2 oy - 1 + ky + dy, 2 ox - 1 + kx + dx) of cell (ky, kx)"""
    return sp[:, :, 1 + ky + dy:1 + ky + dy + 2 * H:2, 1 + kx + dx:1 + kx + dx + 2 * W:2]


def down(x, w, fault=None):
    """pre[b,l,oy,ox] = sum_{s,ky,kx} x[b,s,2oy-1+ky,2ox-1+kx] w[l,s,ky,kx];  x (B, Cs, Hs, Ws) -> (B, Cl, Hs/2, Ws/2)"""
    H, W = x.shape[2] // 2, x.shape[3] // 2
    xp = _pad(x, 2, fault)
    out = torch.zeros(x.shape[0], w.shape[0], H, W, dtype=x.dtype)
    for ky, kx, dy, dx in _cells(fault):
        out = out + torch.einsum("bshw,ls->blhw", _window(xp, ky, kx, dy, dx, H, W), w[:, :, ky, kx])
    return out


def up(x, w, fault=None):
    """pre[b,s,iy,ix] = sum over the (l, ky, kx) with iy = 2oy-1+ky, ix = 2ox-1+kx of x[b,l,oy,ox] w[l,s,ky,kx];
    x (B, Cl, H, W) -> (B, Cs, 2H, 2W).  Written as the scatter it is; ``border``: the positions one step outside L repeat the edge."""
    if fault == "transpose_up":
        w = w.permute(1, 0, 2, 3).contiguous().view(w.shape)       # (the transposition itself when Cl == Cs)
    ring = 1 if fault == "border" else 0
    if ring:
        x = F.pad(x, (1, 1, 1, 1), mode="replicate")               # an L shift of one is an S shift of two
    H, W = x.shape[2:]
    out = torch.zeros(x.shape[0], w.shape[1], 2 * H + 4, 2 * W + 4, dtype=x.dtype)
    for ky, kx, dy, dx in _cells(fault):
        wk = w[:, :, ky ^ 1, kx] if fault == "parity" else w[:, :, ky, kx]
        out[:, :, 1 + ky + dy:1 + ky + dy + 2 * H:2, 1 + kx + dx:1 + kx + dx + 2 * W:2] += torch.einsum("blhw,ls->bshw", x, wk)
    c = 2 + 2 * ring
    return out[:, :, c:out.shape[2] - c, c:out.shape[3] - c]


def dw(l_side, s_side, fault=None, chunk=None):
    """dw[l,s,ky,kx] = sum_{b,oy,ox} L[b,l,oy,ox] S[b,s,2oy-1+ky,2ox-1+kx].  ``last_chunk``: the L positions of the last chunk of
    ``chunk`` (raster order over b, oy, ox) are left out"""
    B, Cl, H, W = l_side.shape
    if fault == "last_chunk":
        P = B * H * W
        keep = (torch.arange(P) < ((P - 1) // chunk) * chunk).view(B, 1, H, W).to(l_side.dtype)
        l_side = l_side * keep
    sp = _pad(s_side, 2, fault)
    out = torch.zeros(Cl, s_side.shape[1], 4, 4, dtype=l_side.dtype)
    for ky, kx, dy, dx in _cells(fault):
        out[:, :, ky, kx] = torch.einsum("blhw,bshw->ls", l_side, _window(sp, ky, kx, dy, dx, H, W))
    return out


def act(pre, kind, slope, fault=None):
    if kind == "relu":
        return torch.where(pre > 0, pre, torch.zeros_like(pre))
    if kind == "leaky":
        return torch.where(pre > 0, pre, (0.0 if fault == "no_slope" else slope) * pre)
    if kind == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-pre))
    return pre


def gp(g, y, kind, slope, fault=None):
    """the gradient in front of the activation, from the saved output y: float32 in, float32 out, each operation rounded"""
    g, y = g.float(), y.float()
    on = (g if fault == "gp_sign_g" else y) > 0
    if kind == "relu":
        return torch.where(on, g, torch.zeros_like(g))
    if kind == "leaky":
        return torch.where(on, g, torch.tensor(0.0 if fault == "no_slope" else slope, dtype=torch.float32) * g)   # y == 0: the slope branch
    if kind == "sigmoid":
        return (g * y) * (1.0 - y)
    return g


def all_(direction, x, w, g, kind, slope, dtype, fault=None, chunk=CHUNK, y=None):
    """{"y", "dx", "dw"} of ``direction`` ("down": x on S; "up": x on L) in ``dtype`` from float32 operands rounded to bf16 as the op
    rounds them.  The backward uses ``y`` (float32, the saved output) when given, else this forward's own output rounded to float32."""
    rnd = (lambda t: t) if fault == "no_round" else round_bf16
    slope = slope32(slope)
    xq, wq = rnd(x).to(dtype), rnd(w).to(dtype)
    fwd, bwd = (down, up) if direction == "down" else (up, down)
    out = act(fwd(xq, wq, fault), kind, slope, fault)
    gq = rnd(gp(g, out if y is None else y, kind, slope, fault)).to(dtype)
    return {"y": out, "dx": bwd(gq, wq, fault), "dw": dw(gq, xq, fault, chunk) if direction == "down" else dw(xq, gq, fault, chunk)}


def reference(direction, x, w, g, kind, slope, y=None):
    """-> (float64 results, yardsticks, gates): gate = GATE_FACTOR x max(yardstick, 2^-23 max |reference|), the yardstick being the
    error of the same computation in float32 on the CPU, the floor half an ulp of the stored fp32 result.  Both backwards work from
    the same saved output: ``y`` (the op's own, float32) when given, else the float64 forward rounded to float32."""
    fwd = all_(direction, x, w, g, kind, slope, torch.float64)
    saved = fwd["y"].float() if y is None else y.float()
    ref = all_(direction, x, w, g, kind, slope, torch.float64, y=saved)
    f32 = all_(direction, x, w, g, kind, slope, torch.float32, y=saved)
    yard = {k: float((f32[k].double() - ref[k]).abs().max()) for k in ref}
    gates = {k: GATE_FACTOR * max(yard[k], 2.0 ** -23 * float(ref[k].abs().max())) for k in ref}
    return ref, yard, gates


def operands(direction, shape, seed=0):
    """float32 x, w and an upstream gradient g, seeded; pre-activations of about unit scale"""
    B, Cs, Cl, Hs, Ws = shape
    gen = torch.Generator().manual_seed(1717 + seed)
    s_shape, l_shape = (B, Cs, Hs, Ws), (B, Cl, Hs // 2, Ws // 2)
    x = torch.randn(s_shape if direction == "down" else l_shape, generator=gen)
    w = torch.randn(Cl, Cs, 4, 4, generator=gen) / (16 * Cs if direction == "down" else 4 * Cl) ** 0.5
    g = torch.randn(l_shape if direction == "down" else s_shape, generator=gen)
    return x, w, g


# ------------------------------------------------------------------------------------------------------ the emulated model
class _Q(torch.autograd.Function):
    """conv / transposed conv + activation in float64 on operands rounded to bf16 (x, w; in backward the gradient in front of the
    activation too), as the op computes it"""

    @staticmethod
    def forward(ctx, x, w, direction, kind, slope):
        xq, wq, slope = round_bf16(x), round_bf16(w), slope32(slope)
        pre = F.conv2d(xq, wq, stride=2, padding=1) if direction == "down" else F.conv_transpose2d(xq, wq, stride=2, padding=1)
        y = act(pre, kind, slope)
        ctx.save_for_backward(xq, wq, y)
        ctx.cfg = (direction, kind, slope)
        return y.clone()

    @staticmethod
    def backward(ctx, g):
        xq, wq, y = ctx.saved_tensors
        direction, kind, slope = ctx.cfg
        if kind == "sigmoid":
            gq = (g * y) * (1.0 - y)
        elif kind == "none":
            gq = g
        else:
            gq = torch.where(y > 0, g, (slope if kind == "leaky" else 0.0) * g)
        gq = round_bf16(gq)
        if direction == "down":
            return up(gq, wq), dw(gq, xq), None, None, None
        return down(gq, wq), dw(xq, gq), None, None, None


def qdown(x, w, kind, slope=0.1):
    return _Q.apply(x, w, "down", kind, slope)


def qup(x, w, kind, slope=0.1):
    return _Q.apply(x, w, "up", kind, slope)


def infovae_forward(sd, x, emulate=False):
    """mnist/model.py:265-279 as a function of a ``state_dict``, in x's dtype -> (recon, z).  ``emulate``: the four convolutions on
    bf16-rounded operands (``qdown`` / ``qup``), everything else unchanged"""
    w = {k: v.to(x.dtype) if not v.requires_grad else v for k, v in sd.items()}
    if emulate:
        h = qdown(qdown(x, w["encoder_conv.0.weight"], "leaky", 0.1), w["encoder_conv.2.weight"], "leaky", 0.1)
    else:
        h = F.leaky_relu(F.conv2d(x, w["encoder_conv.0.weight"], stride=2, padding=1), 0.1)
        h = F.leaky_relu(F.conv2d(h, w["encoder_conv.2.weight"], stride=2, padding=1), 0.1)
    h = F.leaky_relu(F.linear(h.reshape(h.shape[0], -1), w["encoder_fc.0.weight"], w["encoder_fc.0.bias"]), 0.1)
    z = F.linear(h, w["encoder_fc.2.weight"], w["encoder_fc.2.bias"])
    h = torch.relu(F.linear(z, w["decoder_fc.0.weight"], w["decoder_fc.0.bias"]))
    h = torch.relu(F.linear(h, w["decoder_fc.2.weight"], w["decoder_fc.2.bias"])).view(-1, 128, 7, 7)
    if emulate:
        return qup(qup(h, w["decoder_conv.0.weight"], "relu"), w["decoder_conv.2.weight"], "sigmoid"), z
    h = torch.relu(F.conv_transpose2d(h, w["decoder_conv.0.weight"], stride=2, padding=1))
    return torch.sigmoid(F.conv_transpose2d(h, w["decoder_conv.2.weight"], stride=2, padding=1)), z


def formula_tensor(shape, n, fan):
    """sin(0.37 i + n) / sqrt(fan) over the flat index i"""
    i = torch.arange(int(torch.tensor(shape).prod()), dtype=torch.float64)
    return (torch.sin(0.37 * i + n) / fan ** 0.5).view(shape)


def formula_state_dict(names, shapes, scale=1.0):
    """tensor n of the state_dict, in order: sin(0.37 i + n) / sqrt(fan), fan = v[0].numel(), times ``scale`` -> float64"""
    out = {}
    for n, (k, shp) in enumerate(zip(names, shapes)):
        fan = 1
        for d in shp[1:]:
            fan *= int(d)
        out[k] = scale * formula_tensor(tuple(int(d) for d in shp), n, fan)
    return out


def formula_input(B=4):
    """0.5 + 0.5 sin(0.11 i) as (B, 1, 28, 28), float64"""
    i = torch.arange(B * 784, dtype=torch.float64)
    return (0.5 + 0.5 * torch.sin(0.11 * i)).view(B, 1, 28, 28)


def formula_latent_grid(B=4):
    """the decoder_conv input of the fixture: 0.5 + 0.5 sin(0.07 i) as (B, 128, 7, 7), float64"""
    i = torch.arange(B * 128 * 49, dtype=torch.float64)
    return (0.5 + 0.5 * torch.sin(0.07 * i)).view(B, 128, 7, 7)
