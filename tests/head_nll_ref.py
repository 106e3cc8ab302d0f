"""Yardsticks for the fused PixelCNN head (``pixelcnn.head_nll``), independent of the package's op.

``head``          the op's formulas in any dtype: logits of the 1 x 1 convolution with output channel ``v * C + c``, log-sum-exp, NLL,
                  and the three gradients for an upstream gradient ``g``.  ``rounded=True`` rounds h, w and, in backward, d to bf16 as
                  the op does (float64 arithmetic on those values is "the emulation"); ``rounded=False`` is the pure computation.
                  ``fault`` injects what an implementation can get wrong (FAULTS).
``reference``     the emulation in float64, the same in float32 (the yardstick), and the tight gates
``tight_ratio``   error / max(yardstick, 2^-23 max |reference|): a tight comparison passes when this is <= GATE_FACTOR
``loose_ratio``   (error against pure float64) / (the emulation's own error against pure float64): passes when <= LOOSE_FACTOR
``operands``, ``separated``, ``single_position_g``, ``large_logits``   the inputs of the GPU tests
``check_*``       the gates of the GPU tests as functions of an implementation ``run(h, w, b, target, g, C) -> dict``: each returns
                  ratios that must stay <= its factor (tests/test_cpu_head_nll.py runs them on the injected faults)
``HeadFn``, ``model_nll``   the head as an autograd function on float64 leaves, for whole-model references
"""
import functools
import math

import torch

import pixelcnn_ref as R

GATE_FACTOR = R.GATE_FACTOR      # 8, the project's
LOOSE_FACTOR = 2.0
FAULTS = ("channel_order", "pad_columns", "no_max", "no_onehot", "uniform_g", "no_bias", "last_chunk", "last_kblock", "no_round")

# (B, C, hid, V, H, W)
CASES = [(1, 1, 8, 2, 1, 1), (2, 3, 16, 256, 3, 5), (1, 3, 48, 8, 6, 9), (3, 1, 128, 8, 4, 4), (1, 3, 40, 5, 7, 9), (1, 3, 16, 100, 3, 3),
         (1, 1, 256, 4, 5, 5), (1, 1, 16, 4, 300, 7)]


def tile_cases(tile):
    """B * H * W = tile - 1, tile, tile + 1"""
    return [(1, 1, 16, 4, 1, tile - 1), (1, 1, 16, 4, 1, tile), (1, 1, 16, 4, 1, tile + 1)]


def case_id(c):
    return "B%d-C%d-h%d-V%d-%dx%d" % tuple(c)


def round_bf16(t):
    """round to nearest even to bf16, back in the dtype it came in"""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def head(h, w, b, target, g, C, dtype=torch.float64, rounded=True, fault=None, chunk=1024, tile=64):
    """h (B, hid, H, W), w (V * C, hid, 1, 1), b (V * C,), target (B, C, H, W) int64, g (B, C, H, W) or None
    -> {"nll", "lse" (B, C, H, W), "dh" (B, hid, H, W), "dw" like w, "db" like b}, all in ``dtype``"""
    rnd = round_bf16 if (rounded and fault != "no_round") else (lambda t: t)
    B, hid, H, W = h.shape
    V, P = w.shape[0] // C, B * H * W
    hp = rnd(h).to(dtype).permute(0, 2, 3, 1).reshape(P, hid)
    wq = rnd(w.reshape(V * C, hid)).to(dtype)
    bq = b.to(dtype)
    if fault == "channel_order":                                   # c * V + v instead of v * C + c
        wl, bl = wq.view(C, V, hid).permute(1, 0, 2), bq.view(C, V).t()
    else:
        wl, bl = wq.view(V, C, hid), bq.view(V, C)
    hl = hp
    if fault == "last_kblock" and hid > 128:
        hl = hp.clone()
        hl[:, 128:] = 0
    l = torch.einsum("pk,vck->pvc", hl, wl)
    if fault != "no_bias":
        l = l + bl
    t = target.permute(0, 2, 3, 1).reshape(P, C)
    if fault == "no_max":                                           # fp32 exponentials of the logits as they are
        lse = torch.log(torch.exp(l.float()).sum(dim=1)).to(dtype)
    elif fault == "pad_columns":                                    # the zero rows V .. Vp - 1 of the packed weights counted
        lse = torch.logsumexp(torch.cat([l, torch.zeros(P, (-V) % tile, C, dtype=dtype)], dim=1), dim=1)
    else:
        lse = torch.logsumexp(l, dim=1)
    bad = (t < 0) | (t >= V)
    tc = t.clamp(0, V - 1)
    nll = lse - l.gather(1, tc.unsqueeze(1)).squeeze(1)
    nll = torch.where(bad, torch.full_like(nll, float("nan")), nll)

    def back(x):
        return x.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()

    out = {"nll": back(nll), "lse": back(lse)}
    if g is None:
        return out
    gp = g.to(dtype).permute(0, 2, 3, 1).reshape(P, C)
    if fault == "uniform_g":
        gp = torch.ones_like(gp)
    onehot = torch.zeros_like(l)
    if fault != "no_onehot":
        onehot.scatter_(1, tc.unsqueeze(1), (~bad).to(dtype).unsqueeze(1))
    d = gp.unsqueeze(1) * (torch.exp(l - lse.unsqueeze(1)) - onehot)
    dq = rnd(d)
    dh = torch.einsum("pvc,vck->pk", dq, wl)
    dq_w, d_b = dq, d
    if fault == "last_chunk":
        keep = (torch.arange(P) < ((P - 1) // chunk) * chunk).to(dtype).view(P, 1, 1)
        dq_w, d_b = dq * keep, d * keep
    dw, db = torch.einsum("pvc,pk->vck", dq_w, hp), d_b.sum(dim=0)
    if fault == "channel_order":
        dw, db = dw.permute(1, 0, 2), db.t()
    out.update({"dh": back(dh), "dw": dw.reshape(V * C, hid, 1, 1).contiguous(), "db": db.reshape(V * C).contiguous(), "d": d})
    return out


def _absmax(t):
    t = t[~torch.isnan(t)]
    return float(t.abs().max()) if t.numel() else 0.0


def error(got, ref):
    """max |got - ref| over the elements where ref is a number; inf when got is NaN there or the NaN patterns differ"""
    got, ref = got.double(), ref.double()
    if not torch.equal(torch.isnan(got), torch.isnan(ref)):
        return float("inf")
    return _absmax(got - ref)


def reference(h, w, b, target, g, C, keys=("nll", "lse", "dh", "dw", "db")):
    """-> (emulation in float64, yardstick per tensor): the yardstick is max(error of the same computation in float32 on the CPU,
    2^-23 max |reference|), the floor being half an ulp of the stored fp32 result"""
    ref = head(h, w, b, target, g, C, torch.float64)
    f32 = head(h, w, b, target, g, C, torch.float32)
    yard = {k: max(error(f32[k], ref[k]), 2.0 ** -23 * _absmax(ref[k])) for k in keys if k in ref}
    return ref, yard


def tight_ratio(got, ref, yard):
    e = error(got, ref)
    return e / yard if yard > 0 else (0.0 if e == 0 else float("inf"))


def loose_yardsticks(h, w, b, target, g, C, keys=("dh", "dw", "db")):
    """-> (pure float64 results, the emulation's own error against them per tensor)"""
    pure = head(h, w, b, target, g, C, torch.float64, rounded=False)
    emu = head(h, w, b, target, g, C, torch.float64)
    return pure, {k: error(emu[k], pure[k]) for k in keys}


def loose_ratio(got, pure, yard):
    e = error(got, pure)
    return e / yard if yard > 0 else (0.0 if e == 0 else float("inf"))


# ------------------------------------------------------------------------------------------------------ inputs
def operands(case, seed=0):
    """float32 h, w, b, int64 target and an upstream gradient g with zeros and negative entries, seeded"""
    B, C, hid, V, H, W = case
    gen = torch.Generator().manual_seed(9090 + seed)
    h = torch.randn(B, hid, H, W, generator=gen)
    w = torch.randn(V * C, hid, 1, 1, generator=gen) * (2.0 / hid ** 0.5)
    b = torch.rand(V * C, generator=gen) - 0.5
    target = torch.randint(0, V, (B, C, H, W), generator=gen)
    g = torch.randn(B, C, H, W, generator=gen)
    g = g * (torch.rand(B, C, H, W, generator=gen) >= 0.25).float()
    g.view(-1)[0] = -0.75
    if g.numel() > C:                                               # one position with g = 0 in every channel
        g[-1, :, -1, -1] = 0.0
    return h, w, b, target, g


def single_position_g(g):
    """g non-zero at one position only (the middle one): db is then d at that position, a single summand"""
    B, C, H, W = g.shape
    out = torch.zeros_like(g)
    p = (B * H * W) // 2
    bi, rem = divmod(p, H * W)
    out[bi, :, rem // W, rem % W] = torch.tensor([1.5, -0.625, 0.875])[:C]
    return out


def large_logits(case, seed=0):
    """weights x 30 (logits of magnitude 100 and more); level 0 of channel 0 gets a bias of -200 and is the target at one position"""
    h, w, b, target, g = operands(case, seed)
    w, b, target = w * 30.0, b.clone(), target.clone()
    b[0] = -200.0
    target[0, 0, 0, 0] = 0
    return h, w, b, target, g


def separated(case, h_first=True, seed=0):
    """h non-zero in one half of the channels only and w in the other, the bias constant per data channel, g signed powers of two:
    the logits are flat, d = g (1 / V - [v == target]) is exact in bf16 when V is a power of two, and no rounding boundary is near"""
    B, C, hid, V, H, W = case
    h, w, b, target, _ = operands(case, seed)
    half = hid // 2
    h, w = h.clone(), w.clone()
    if h_first:
        h[:, half:] = 0
        w[:, :half] = 0
    else:
        h[:, :half] = 0
        w[:, half:] = 0
    b = torch.tensor([0.25, -0.5, 0.125])[:C].repeat(V)             # b[v * C + c] = beta_c
    gen = torch.Generator().manual_seed(17 + seed)
    e = torch.randint(-3, 3, (B, C, H, W), generator=gen).float()
    s = torch.randint(0, 2, (B, C, H, W), generator=gen).float() * 2 - 1
    return h, w, b, target, s * torch.pow(2.0, e)


# ------------------------------------------------------------------------------------------------------ the gates
SEPARATED_SHAPES = [(1, 1, 16, None, 300, 7), (1, 3, 256, None, 5, 5)]      # multi-chunk; two K blocks.  V in SEPARATED_LEVELS
SEPARATED_LEVELS = (2, 8, 256)
DB1_CASES = [CASES[2], CASES[4], CASES[6], CASES[7]]


@functools.lru_cache(maxsize=None)
def _tight(kind, case, flag=True):
    """inputs, emulation and yardsticks of one tight comparison, computed once and shared (do not modify)"""
    if kind == "large":
        ops = large_logits(case)
    elif kind == "db1":
        ops = operands(case)
        ops = ops[:4] + (single_position_g(ops[4]),)
    elif kind == "separated":
        ops = separated(case, flag)
    else:
        ops = operands(case)
    return ops, reference(*ops, case[1])


@functools.lru_cache(maxsize=None)
def _loose(case):
    ops = operands(case)
    return ops, loose_yardsticks(*ops, case[1])


def check_forward(run, case, kind="general"):
    """nll and lse against the emulation; tight (<= GATE_FACTOR).  Any non-finite value where the reference is finite: inf"""
    ops, (ref, yard) = _tight(kind, case)
    got = run(*ops, case[1])
    return {k: tight_ratio(got[k], ref[k], yard[k]) for k in ("nll", "lse") if got.get(k) is not None}


def check_db1(run, case):
    """db with g non-zero at a single position: one summand, no bf16 rounding of d involved; tight"""
    ops, (ref, yard) = _tight("db1", case)
    return {"db": tight_ratio(run(*ops, case[1])["db"], ref["db"], yard["db"])}


def check_separated(run, case, h_first):
    """dh and dw on separated supports: the non-zero halves tight, the other halves exactly 0 (else inf)"""
    ops, (ref, yard) = _tight("separated", case, h_first)
    got = run(*ops, case[1])
    half = case[2] // 2
    zh, zw = (slice(0, half), slice(half, None)) if h_first else (slice(half, None), slice(0, half))   # where dh / dw must be 0
    out = {k: tight_ratio(got[k], ref[k], yard[k]) for k in ("dh", "dw")}
    if bool((got["dh"][:, zh] != 0).any()) or bool((ref["dh"][:, zh] != 0).any()):
        out["dh"] = float("inf")
    if bool((got["dw"][:, zw] != 0).any()) or bool((ref["dw"][:, zw] != 0).any()):
        out["dw"] = float("inf")
    return out


def check_loose(run, case):
    """dh, dw, db against pure float64, in units of the emulation's own error; <= LOOSE_FACTOR"""
    ops, (pure, yard) = _loose(case)
    got = run(*ops, case[1])
    return {k: loose_ratio(got[k], pure[k], yard[k]) for k in ("dh", "dw", "db")}


# ------------------------------------------------------------------------------------------------------ whole-model references
class HeadFn(torch.autograd.Function):
    """``head`` on float64 leaves: nll from (features, conv4.weight, conv4.bias); ``rounded`` as in ``head``"""

    @staticmethod
    def forward(ctx, h, w, b, target, C, rounded):
        ctx.save_for_backward(h, w, b, target)
        ctx.C, ctx.rounded = C, rounded
        return head(h, w, b, target, None, C, torch.float64, rounded)["nll"]

    @staticmethod
    def backward(ctx, g):
        h, w, b, target = ctx.saved_tensors
        r = head(h, w, b, target, g, ctx.C, torch.float64, ctx.rounded)
        return r["dh"], r["dw"], r["db"], None, None, None


def features(sd, cfg, x):
    """``pixelcnn_ref.forward`` up to the activation conv4 consumes (its ReLU included)"""
    hid = cfg["hid_dims"]
    if cfg["gated"]:
        xv, h = R._gated_block(sd, "conv1.", x, x, 7, hid)
        for k in range(cfg["n_blocks"]):
            xv, h_ = R._gated_block(sd, "blocks.blocks.%d." % k, xv, h, 3, hid)
            h = h + h_
        return torch.relu(R._conv(sd, "conv2", torch.relu(h)))
    h = R._conv(sd, "conv1", x, "A", (3, 3, 3, 3))
    for k in range(cfg["n_blocks"]):
        h = torch.relu(R._conv(sd, "blocks.%d" % (2 * k), h, "B", (1, 1, 1, 1)))
    return torch.relu(R._conv(sd, "conv2", h))


def model_nll(sd, cfg, x, target, emulated):
    """per-element NLL of the whole model in float64: pure, or with every convolution and the head emulated (bf16-rounded operands)"""
    if emulated:
        import causal_conv_ref as CC
        with CC._emulating():
            f = features(sd, cfg, x)
    else:
        f = features(sd, cfg, x)
    return HeadFn.apply(f, sd["conv4.weight"], sd["conv4.bias"], target, cfg["data_channels"], emulated)


LN2 = math.log(2.0)
