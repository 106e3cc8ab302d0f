"""float64 references, float32 baselines, stand-in faults and gates of the streaming kernels every step runs (csrc/elementwise.hip: the
3-pass latent block, sigmoid + BCE, log-softmax + NLL, the BatchNorm triple, embedding gather / scatter, column sums) and of the
stand-alone latent / loss ops.  Nothing here needs a GPU.

Every reference is ONE plain torch function of a ``dtype``: at float64 it is the reference, at float32 on the CPU it is the reference
project's own arithmetic -- the only baseline a gate uses.  It is built from the oracle's pieces (``product_of_experts``,
``reparametrize``, ``kl_sum`` of oracle/mmvae_ref.py) where they exist.  Next to each value it returns the value's MAGNITUDE: the sum of
the absolute values of the terms added to form it (at least 1 for a logarithm), so that a cancelling sum (d_im0 + d_im1, dz + kl_coef mu)
is not measured against its own small result.  The backward formulas are checked against float64 autograd in
tests/test_cpu_elementwise_ref.py.

Gates (``Rec`` records, ``violations``):
  fp32 element   err = max |got - ref64| / magnitude <= max(4 err32, 2^-22), err32 the same figure of the float32 CPU evaluation
  bf16 element   |got - ref64| / magnitude <= 2^-8; pads exact
  atomic sums    |got - ref64| <= 2 N 2^-24 sum|terms|, N = the number of scalar terms added into the output (4 per element for a KL sum,
                 2 per element for a BCE sum, 1 per row for a bias, NLL or column sum, plus 1 for a non-zero start value; a one-row
                 bias "sum" is floored by the fp32 element gate).  The BCE term (1 - t) log(1 - p) counts with max(|log(1 - p)|, (1 + p) / (1 - p)): the
                 cancellation of 1 - p inside the logarithm, which the reference's own float32 arithmetic carries too
  BatchNorm      mean / running mean: fp32 element gate; rstd: relative error <= 2^-22 (1 + mean^2 / var) (var = 0: 2^-22, i.e. the
                 clamped variance must be exactly 0); running variance, per channel: relative error <= max(2^-22 (1 + max_g mean^2 / var), 4 err32 of that channel) -- the second
                 term for the roundings of the momentum updates (measured figure in gate_bn_tables).

``FAULTS`` names wrong variants; ``emulate_*`` evaluates an operation in float32 with one of them (the stand-in for a subtly wrong
kernel).  The CPU test runs every fault through the gate functions below -- the ones the GPU test calls -- on the GPU test's inputs.
"""
import collections
import math

import torch
import torch.nn.functional as F

from oracle import mmvae_ref as R

F64, F32 = torch.float64, torch.float32
U24, U22, BF16_GATE = 2.0 ** -24, 2.0 ** -22, 2.0 ** -8
STAT_SLOTS, LOSS_SLOTS = 16, 32
BN_EPS, BN_MOM = 1e-5, 0.1

FAULTS = ("no_1e8", "precision_mean", "pass1_variant0", "kl_coef_ignored", "no_eps_dlogvar", "biased_running_var", "skip_mask_ignored",
          "updates_once", "pad_nonzero", "no_bce_clamp", "target_not_wrapped")
# which operation shows which fault
FAULTS_OF = dict(
    latent3_fwd=("no_1e8", "precision_mean", "pass1_variant0", "pad_nonzero"),
    latent3_bwd=("no_1e8", "precision_mean", "pass1_variant0", "kl_coef_ignored", "no_eps_dlogvar", "pad_nonzero"),
    bn=("biased_running_var", "skip_mask_ignored", "updates_once", "pad_nonzero"),
    bce=("no_bce_clamp",),
    nll=("target_not_wrapped", "pad_nonzero"),
)

Rec = collections.namedtuple("Rec", "name err gate")


def violations(recs):
    """the records that miss their gate (a NaN misses); empty: pass"""
    return ["%s: %.3e > gate %.3e" % r for r in recs if not r.err <= r.gate]


def describe(recs):
    worst = {}
    for r in recs:
        if r.name not in worst or r.err / max(r.gate, 1e-300) > worst[r.name].err / max(worst[r.name].gate, 1e-300):
            worst[r.name] = r
    return "; ".join("%s %.2e (gate %.2e)" % r for r in worst.values())


def _err(got, ref, mag):
    got, ref, mag = got.detach().double().cpu(), ref.detach().double(), mag.detach().double()
    if got.numel() == 0:
        return 0.0
    d = (got - ref).abs()
    e = torch.where(d == 0, torch.zeros_like(d), d / mag.clamp_min(1e-300))      # equal values: no error, whatever the magnitude
    e = torch.where(torch.isfinite(got), e, torch.full_like(e, float("inf")))
    return float(e.max())


def rec_f32(name, got, ref64, mag, ref32):
    return Rec(name, _err(got, ref64, mag), max(4.0 * _err(ref32, ref64, mag), U22))


def rec_bf16(name, got, ref64, mag):
    return Rec(name, _err(got, ref64, mag), BF16_GATE)


def rec_sum(name, got, ref64, sum_abs, nterms):
    return Rec(name, _err(got, ref64, sum_abs), 2.0 * nterms * U24)


def rec_exact(name, got, want):
    got, want = got.detach().cpu(), want.detach().cpu()
    same = got.shape == want.shape and bool(((got == want) | (torch.isnan(got) & torch.isnan(want))).all())
    return Rec(name + " exact", 0.0 if same else float("inf"), 0.0)


def bf16_round(x):
    return x.to(torch.bfloat16)


# ====================================================================================================== product of experts, reparam, KL
def poe(mu, lv, dtype=F64, fault=None):
    """R.product_of_experts on experts stacked along dim 0 -> (mu, logvar, magnitude of mu, magnitude of logvar)"""
    mu, lv = mu.to(dtype), lv.to(dtype)
    e8 = 0.0 if fault == "no_1e8" else 1e-8
    if fault == "precision_mean":
        var = torch.exp(lv) + e8
        pm, plv = torch.sum(mu / var, 0) / torch.sum(1 / var, 0), torch.log(1 / torch.sum(1 / var, 0))
    else:
        pm, plv = R.product_of_experts(mu, lv, e8)
    var = torch.exp(lv) + e8
    return pm, plv, torch.sum(mu.abs() * var, 0) / torch.sum(var, 0), plv.abs().clamp_min(1.0)


def poe_bwd(mu, lv, gmu, glv, dtype=F64, fault=None, gmu_mag=None, glv_mag=None):
    """backward of ``poe``: -> (d_mu, d_logvar, their magnitudes), each [M][...]"""
    mu, lv, gmu, glv = mu.to(dtype), lv.to(dtype), gmu.to(dtype), glv.to(dtype)
    gmu_mag = gmu.abs() if gmu_mag is None else gmu_mag.to(dtype)
    glv_mag = glv.abs() if glv_mag is None else glv_mag.to(dtype)
    e8 = 0.0 if fault == "no_1e8" else 1e-8
    e = torch.exp(lv)
    var = e + e8
    s0, t = var.sum(0), (1 / var).sum(0)
    if fault == "precision_mean":
        pm = torch.sum(mu / var, 0) / t
        dmu = gmu * (1 / var) / t
        dvar = -gmu * (mu - pm) / (var * var * t) + glv / (t * var * var)
        return dmu, dvar * e, gmu_mag / (var * t), (gmu_mag * (mu.abs() + pm.abs()) / (var * var * t) + glv_mag / (t * var * var)) * e
    pm = torch.sum(mu * var, 0) / s0
    pm_mag = torch.sum(mu.abs() * var, 0) / s0
    dmu = gmu * var / s0
    dvar = gmu * (mu - pm) / s0 + glv / (t * var * var)
    return dmu, dvar * e, gmu_mag * var / s0, (gmu_mag * (mu.abs() + pm_mag) / s0 + glv_mag / (t * var * var)) * e


def reparam(mu, lv, eps, dtype=F64):
    mu, lv, eps = mu.to(dtype), lv.to(dtype), eps.to(dtype)
    return R.reparametrize(mu, lv, True, eps), (eps * torch.exp(0.5 * lv)).abs() + mu.abs()


def reparam_bwd(lv, eps, dz, dtype=F64):
    """-> (d_mu, d_logvar, magnitudes)"""
    lv, eps, dz = lv.to(dtype), eps.to(dtype), dz.to(dtype)
    dlv = dz * eps * 0.5 * torch.exp(0.5 * lv)
    return dz, dlv, dz.abs(), dlv.abs()


def kl_terms(mu, lv, dtype=F64):
    """-> (R.kl_sum, sum of the absolute terms, number of terms)"""
    mu, lv = mu.to(dtype), lv.to(dtype)
    return R.kl_sum(mu, lv), 0.5 * (1 + lv.abs() + mu * mu + torch.exp(lv)).sum(), 4 * mu.numel()


def kl_bwd(mu, lv, coef, dtype=F64):
    mu, lv = mu.to(dtype), lv.to(dtype)
    return coef * mu, -0.5 * coef * (1 - torch.exp(lv)), (coef * mu).abs(), 0.5 * abs(coef) * (1 + torch.exp(lv))


# ====================================================================================================== 3-pass latent block
def latent3_inputs(B, D, seed=None):
    """seeded operands: image variants that differ, logvars spread over [-20, 2] with -20 exactly in every tensor"""
    g = torch.Generator().manual_seed(4000 + 131 * B + D if seed is None else seed)

    def enc():
        mu = torch.randn(B, D, generator=g)
        lv = torch.linspace(-20.0, 2.0, B * D) if B * D > 1 else torch.full((1,), -20.0)
        lv = lv[torch.randperm(B * D, generator=g)].view(B, D)
        return torch.cat((mu, lv), 1).contiguous()
    img0, img1, txt = enc(), enc(), enc()
    assert B * D == 1 or not torch.equal(img0, img1)
    if B * D == 1:
        img1[0, 0] = -0.75                 # the variants differ where the logvar is pinned at -20
        txt[0, 1] = 1.0                    # and the two experts of pass 0 differ in variance (else every weighting of the mean agrees)
    return dict(img0=img0, img1=img1, txt=txt, eps=torch.randn(3, B, D, generator=g), dz_a=torch.randn(3, B, D, generator=g),
                dz_b=0.3 * torch.randn(3, B, D, generator=g))


def _experts(inp, dtype, fault):
    D = inp["txt"].shape[1] // 2
    i0, i1, tx = inp["img0"].to(dtype), inp["img1"].to(dtype), inp["txt"].to(dtype)
    if fault == "pass1_variant0":
        i1 = i0
    sp = lambda x: (x[:, :D], x[:, D:])
    (m0, l0), (m1, l1), (mt, lt) = sp(i0), sp(i1), sp(tx)
    return [(torch.stack((m0, mt)), torch.stack((l0, lt))), (m1[None], l1[None]), (mt[None], lt[None])]


def latent3_fwd(inp, training=True, dtype=F64, fault=None):
    """-> dict(mu, logvar, z [3][B][D], kl [3]) and *_mag, kl_abs, kl_n.  Pass 0: PoE{image 0, text}; 1: PoE{image 1}; 2: PoE{text}."""
    pf = fault if fault in ("no_1e8", "precision_mean") else None
    out = collections.defaultdict(list)
    for k, (m, l) in enumerate(_experts(inp, dtype, fault)):
        pm, plv, mm, lm = poe(m, l, dtype, pf)
        if training:
            z, zm = reparam(pm, plv, inp["eps"][k], dtype)
            zm = zm - pm.abs() + mm
        else:
            z, zm = pm, mm
        kl, kla, kln = kl_terms(pm, plv, dtype)
        for n, v in (("mu", pm), ("logvar", plv), ("z", z), ("kl", kl), ("mu_mag", mm), ("logvar_mag", lm), ("z_mag", zm), ("kl_abs", kla)):
            out[n].append(v)
    res = {n: torch.stack(v) for n, v in out.items()}
    res["kl_n"] = kln
    return res


def latent3_bwd(inp, mu, lv, kl_coef, training=True, use_a=True, use_b=True, dtype=F64, fault=None):
    """Gradient of sum_k <dz_a + dz_b, z_k> + kl_coef[k] KL_k wrt the encoder outputs, from the forward's mu / logvar [3][B][D].
    -> dict(d_im0, d_im1, d_txt [B][2D]) and *_mag"""
    pf = fault if fault in ("no_1e8", "precision_mean") else None
    mu, lv = mu.to(dtype), lv.to(dtype)
    res = {}
    dt, dtm = 0.0, 0.0
    for k, (m, l) in enumerate(_experts(inp, dtype, fault)):
        dz = torch.zeros_like(mu[k])
        dzm = torch.zeros_like(mu[k])
        for use, key in ((use_a, "dz_a"), (use_b, "dz_b")):
            if use:
                dz, dzm = dz + inp[key][k].to(dtype), dzm + inp[key][k].to(dtype).abs()
        kc = 0.0 if (fault == "kl_coef_ignored" and k == 1) else kl_coef[k]
        k_mu, k_lv, k_mum, k_lvm = kl_bwd(mu[k], lv[k], kc, dtype)
        gmu, gmum, glv, glvm = dz + k_mu, dzm + k_mum, k_lv, k_lvm
        if training and fault != "no_eps_dlogvar":
            _, r_lv, _, r_lvm = reparam_bwd(lv[k], inp["eps"][k], dz, dtype)
            glv, glvm = glv + r_lv, glvm + dzm * (inp["eps"][k].to(dtype) * 0.5 * torch.exp(0.5 * lv[k])).abs()
        dm, dl, dmm, dlm = poe_bwd(m, l, gmu, glv, dtype, pf, gmum, glvm)
        cat = lambda a, b, i: torch.cat((a[i], b[i]), 1)
        if k == 0:
            res["d_im0"], res["d_im0_mag"] = cat(dm, dl, 0), cat(dmm, dlm, 0)
            dt, dtm = cat(dm, dl, 1), cat(dmm, dlm, 1)
        elif k == 1:
            res["d_im1"], res["d_im1_mag"] = cat(dm, dl, 0), cat(dmm, dlm, 0)
        else:
            res["d_txt"], res["d_txt_mag"] = dt + cat(dm, dl, 0), dtm + cat(dmm, dlm, 0)
    return res


def latent3_loss64(inp, kl_coef, training=True, use_a=True, use_b=True):
    """the scalar whose float64 autograd gradient ``latent3_bwd`` must equal; -> (loss, img0, img1, txt leaves)"""
    leaves = {k: inp[k].double().clone().requires_grad_(True) for k in ("img0", "img1", "txt")}
    f = latent3_fwd(dict(inp, **leaves), training, F64)
    dz = sum(inp[k].double() for k, u in (("dz_a", use_a), ("dz_b", use_b)) if u) if (use_a or use_b) else torch.zeros_like(f["z"])
    loss = (dz * f["z"]).sum() + sum(kl_coef[k] * f["kl"][k] for k in range(3))
    return loss, leaves, f


def emulate_latent3_fwd(inp, ldz, training=True, fault=None):
    """what a float32 kernel (with one fault) would leave in the output buffers"""
    f = latent3_fwd(inp, training, F32, fault)
    _, B, D = f["z"].shape
    zb = torch.zeros(3 * B, ldz, dtype=torch.bfloat16)
    zb[:, :D] = bf16_round(f["z"].reshape(3 * B, D))
    if ldz > D:
        zb[:, D] = 1.0
    if fault == "pad_nonzero" and ldz > D + 1:
        zb[3 * B - 1, ldz - 1] = 2.0 ** -20
    return dict(mu=f["mu"], logvar=f["logvar"], z=f["z"], z_bf=zb, kl=f["kl"])


def gate_latent3_fwd(got, inp, ldz, training=True):
    """got: dict(mu, logvar, z [3][B][D] fp32, z_bf [3B][ldz] bf16, kl [3] = the slot rows folded)"""
    r64, r32 = latent3_fwd(inp, training, F64), latent3_fwd(inp, training, F32)
    _, B, D = r64["z"].shape
    recs = [rec_f32(n, got[n], r64[n], r64[n + "_mag"], r32[n]) for n in ("mu", "logvar", "z")]
    zb = got["z_bf"].cpu()
    recs.append(rec_bf16("z_bf", zb[:, :D].double(), r64["z"].reshape(3 * B, D), r64["z_mag"].reshape(3 * B, D)))
    recs.append(rec_exact("z_bf == bf16(z)", zb[:, :D], bf16_round(got["z"].cpu().reshape(3 * B, D))))
    pads = torch.zeros(3 * B, ldz - D)
    if ldz > D:
        pads[:, 0] = 1.0
    recs.append(rec_exact("z_bf pads", zb[:, D:].float(), pads))
    if not training:
        recs.append(rec_exact("eval z == mu", got["z"], got["mu"]))
    recs += [rec_sum("kl[%d]" % k, got["kl"][k], r64["kl"][k], r64["kl_abs"][k], r64["kl_n"]) for k in range(3)]
    return recs


IMG_FORMS = ("f32_sum", "bf16_sum", "bf16_two_padded", "bf16_two")


def img_form_ld(form, D):
    return {"f32_sum": 0, "bf16_sum": 0, "bf16_two": 0, "bf16_two_padded": (2 * D + 7) // 8 * 8 + 8}[form]


def emulate_latent3_bwd(inp, mu, lv, kl_coef, form, training=True, use_a=True, use_b=True, fault=None):
    r = latent3_bwd(inp, mu, lv, kl_coef, training, use_a, use_b, F32, fault)
    B, D2 = r["d_txt"].shape
    out = dict(d_txt=r["d_txt"], d_txt_bf=bf16_round(r["d_txt"]), d_img_bias=(r["d_im0"] + r["d_im1"]).sum(0), d_txt_bias=r["d_txt"].sum(0))
    if form == "f32_sum":
        out["d_img_f32"] = r["d_im0"] + r["d_im1"]
    elif form == "bf16_sum":
        out["d_img_bf"] = bf16_round(r["d_im0"] + r["d_im1"])
    else:
        ld = img_form_ld(form, D2 // 2) or D2
        o = torch.zeros(2 * B, ld, dtype=torch.bfloat16)
        o[:B, :D2], o[B:, :D2] = bf16_round(r["d_im0"]), bf16_round(r["d_im1"])
        if fault == "pad_nonzero" and ld > D2:
            o[B, ld - 1] = 2.0 ** -20
        out["d_img_bf"] = o
    return out


def gate_latent3_bwd(got, inp, mu, lv, kl_coef, form, training=True, use_a=True, use_b=True, bias_start=0.0):
    """got: any of d_img_f32 [B][2D], d_img_bf (form's layout), d_txt, d_txt_bf, d_img_bias, d_txt_bias [2D] (started at bias_start)"""
    r64 = latent3_bwd(inp, mu, lv, kl_coef, training, use_a, use_b, F64)
    r32 = latent3_bwd(inp, mu, lv, kl_coef, training, use_a, use_b, F32)
    B, D2 = r64["d_txt"].shape
    s64, sm, s32 = r64["d_im0"] + r64["d_im1"], r64["d_im0_mag"] + r64["d_im1_mag"], r32["d_im0"] + r32["d_im1"]
    recs = []
    if form == "f32_sum":
        recs.append(rec_f32("d_img_f32", got["d_img_f32"], s64, sm, s32))
    elif form == "bf16_sum":
        recs.append(rec_bf16("d_img_bf sum", got["d_img_bf"].double(), s64, sm))
    else:
        o = got["d_img_bf"].cpu()
        recs.append(rec_bf16("d_img_bf variant 0", o[:B, :D2].double(), r64["d_im0"], r64["d_im0_mag"]))
        recs.append(rec_bf16("d_img_bf variant 1", o[B:, :D2].double(), r64["d_im1"], r64["d_im1_mag"]))
        recs.append(rec_exact("d_img_bf pads", o[:, D2:].float(), torch.zeros(2 * B, o.shape[1] - D2)))
    if "d_txt" in got:
        recs.append(rec_f32("d_txt", got["d_txt"], r64["d_txt"], r64["d_txt_mag"], r32["d_txt"]))
    if "d_txt_bf" in got:
        recs.append(rec_bf16("d_txt_bf", got["d_txt_bf"].double(), r64["d_txt"], r64["d_txt_mag"]))
    # N = B rows per column sum, as test_latent1_alone.  A one-row "sum" is the element itself and carries the element's own rounding,
    # which the summation bound does not cover: at B = 1 the fp32 element gate max(4 err32, 2^-22) is the floor (the float32 CPU
    # evaluation measures 1.9e-7 of sum|terms| there, against 2 B 2^-24 = 1.19e-7; 0.9e-7 .. 1.1e-7 at B = 3 .. 9, inside the plain bound).
    nb = B + (1 if bias_start else 0)
    for name, v64, vm, v32 in (("d_img_bias", s64, sm, s32), ("d_txt_bias", r64["d_txt"], r64["d_txt_mag"], r32["d_txt"])):
        if name in got:
            r = rec_sum(name, got[name], v64.sum(0) + bias_start, vm.sum(0) + abs(bias_start), nb)
            if B == 1:
                r = Rec(r.name, r.err, max(r.gate, rec_f32(name, got[name], v64.sum(0) + bias_start, vm.sum(0) + abs(bias_start),
                                                           v32.sum(0) + bias_start).gate))
            recs.append(r)
    return recs


# ====================================================================================================== sigmoid + BCE
SATURATED = (20.0, -20.0, 40.0, -40.0, 100.0, -100.0)


def bce_inputs(G, B, C, H, W, ldl, seed=None):
    """logits NHWC [G*B][H][W][ldl] in an ordinary range (|l| <= 8) with +-20, +-40, +-100 among them; targets NCHW in [0, 1] with exact
    0 and 1.  A single element is an ordinary logit."""
    g = torch.Generator().manual_seed(5000 + 7 * G + B * C * H * W if seed is None else seed)
    logits = (6.0 * torch.rand(G * B, H, W, ldl, generator=g) - 3.0)
    target = torch.rand(B, C, H, W, generator=g)
    n = B * C * H * W
    if n >= 32:
        tf = target.view(-1)
        tf[30::7], tf[33::7] = 0.0, 1.0
        lv = logits[..., :C].permute(0, 3, 1, 2).reshape(G, n).clone()          # NCHW order, per group
        for j, s in enumerate(SATURATED):              # a run of five per saturated logit: targets 0, 1 exactly and three in between
            for q in range(5):
                lv[:, 5 * j + q] = s
            tf[5 * j], tf[5 * j + 1] = 0.0, 1.0
        logits[..., :C] = lv.view(G * B, C, H, W).permute(0, 2, 3, 1)
    return logits.contiguous(), target.contiguous()


def _nchw(logits, C):
    return logits[..., :C].permute(0, 3, 1, 2).contiguous()


def bce(logits, target, G, C, coef, dtype=F64, fault=None):
    """F.binary_cross_entropy(F.sigmoid(logits), target, reduction='sum') per group and its gradient, written out (clamps included)
    -> dict(recon, dlogit [G*B][C][H][W], loss [G]) + magnitudes"""
    l = _nchw(logits, C).to(dtype)
    GB = l.shape[0]
    t = target.to(dtype).repeat(G, 1, 1, 1)
    p = torch.sigmoid(l)
    lp, lq = torch.log(p), torch.log(1 - p)
    if fault != "no_bce_clamp":
        lp, lq = lp.clamp_min(-100.0), lq.clamp_min(-100.0)
    a, b = t * lp, (1 - t) * lq
    cg = torch.tensor(coef[:G], dtype=dtype).repeat_interleave(GB // G).view(GB, 1, 1, 1)
    pq = p * (1 - p)
    dl = cg * (p - t) / pq.clamp_min(1e-12) * pq
    # log(1 - p) is the logarithm of a cancelling difference: an error of one rounding of p moves it by (1 + p) / (1 - p) roundings, so
    # that -- never less than 1 -- is the magnitude of the term next to |log(1 - p)| itself (p = sigmoid(l): (1 + p) / (1 - p) = 2 e^l + 1)
    mag_terms = t * lp.abs().clamp_min(1.0) + (1 - t) * torch.maximum(lq.abs(), (2 * torch.exp(l) + 1).clamp_max(1e30))
    return dict(recon=p, dlogit=dl, loss=-(a + b).view(G, -1).sum(1), recon_mag=torch.ones_like(p), dlogit_mag=cg.abs() * (p + t),
                loss_mag=mag_terms, loss_n=2 * (l.numel() // G))


def bce_torch32(logits, target, G, C, coef):
    """the reference project's own arithmetic: torch.sigmoid -> F.binary_cross_entropy(reduction='sum') in float32, autograd for dlogit"""
    l = _nchw(logits, C).float().requires_grad_(True)
    t = target.float().repeat(G, 1, 1, 1)
    p = torch.sigmoid(l)
    per = F.binary_cross_entropy(p, t, reduction="none").view(G, -1).sum(1)
    (per * torch.tensor(coef[:G])).sum().backward()
    return dict(recon=p.detach(), dlogit=l.grad, loss=per.detach())


def emulate_bce(logits, target, G, C, coef, fault=None):
    r = bce(logits, target, G, C, coef, F32, fault)
    return dict(recon=r["recon"], dlogit=r["dlogit"], loss=r["loss"])


def gate_bce(got, logits, target, G, C, coef, loss_start=0.0):
    """Ordinary logits (|l| <= 10) against float64; saturated ones against torch's float32 BCE, whose clamps a float64 sigmoid never
    reaches.  The loss sum takes float64 terms for the ordinary and float32-torch terms for the saturated elements."""
    r64, r32, t32 = bce(logits, target, G, C, coef, F64), bce(logits, target, G, C, coef, F32), bce_torch32(logits, target, G, C, coef)
    sat = _nchw(logits, C).abs() > 10.0
    recs = []
    for n in ("recon", "dlogit"):
        if n not in got:
            continue
        ref = torch.where(sat, t32[n].double(), r64[n])
        base = torch.where(sat, t32[n].double(), r32[n].double())
        recs.append(rec_f32(n, got[n], ref, r64[n + "_mag"], base))
    l32 = _nchw(logits, C).float()
    t = target.float().repeat(G, 1, 1, 1)
    sat_terms = F.binary_cross_entropy(torch.sigmoid(l32), t, reduction="none").double()
    l64 = _nchw(logits, C).double()
    p = torch.sigmoid(l64)
    ord_terms = -(t.double() * torch.log(p) + (1 - t.double()) * torch.log(1 - p))
    ref_loss = torch.where(sat, sat_terms, ord_terms).view(G, -1).sum(1)
    extra = 1 if loss_start else 0
    sum_abs = torch.where(sat, sat_terms.clamp_min(1.0), r64["loss_mag"]).view(G, -1).sum(1)
    recs.append(rec_sum("loss", got["loss"], ref_loss + loss_start, sum_abs + abs(loss_start), r64["loss_n"] + extra))
    return recs


# ====================================================================================================== log-softmax + NLL
def nll_inputs(G, rows_per_group, classes, seed=None):
    g = torch.Generator().manual_seed(6000 + 97 * rows_per_group + classes if seed is None else seed)
    rows = G * rows_per_group
    logits = 3.0 * torch.randn(rows, classes, generator=g)
    logits[rows // 2] = torch.linspace(-100.0, 100.0, classes) if classes > 1 else torch.full((1,), 100.0)   # a spread of 200
    target = torch.randint(0, classes, (rows_per_group,), generator=g)
    return logits.contiguous(), target


def logsoftmax_nll(logits, target, rows_per_group, coef, dtype=F64, fault=None):
    """-> dict(words [rows][classes], nll [G], dlogits [rows][classes]) + magnitudes; target [target_rows] wraps over the rows"""
    l = logits.to(dtype)
    rows, classes = l.shape
    G = (rows + rows_per_group - 1) // rows_per_group
    words = torch.log_softmax(l, 1)
    res = dict(words=words, words_mag=words.abs().clamp_min(1.0))
    if target is None:
        return res
    r = torch.arange(rows)
    tg = target[r.clamp_max(len(target) - 1)] if fault == "target_not_wrapped" else target[r % len(target)]
    onehot = F.one_hot(tg, classes).to(dtype)
    cg = torch.tensor(coef, dtype=dtype)[r // rows_per_group].view(rows, 1)
    picked = -(words * onehot).sum(1)
    grp = F.one_hot(r // rows_per_group, G).to(dtype)
    res.update(nll=picked @ grp, nll_abs=picked.abs().clamp_min(1.0) @ grp, nll_n=rows_per_group,
               dlogits=cg * (torch.exp(words) - onehot), dlogits_mag=cg.abs() * (torch.exp(words) + onehot))
    return res


def emulate_nll(logits, target, rows_per_group, coef, ld_d, fault=None):
    r = logsoftmax_nll(logits, target, rows_per_group, coef, F32, fault)
    rows, classes = logits.shape
    db = torch.zeros(rows, ld_d, dtype=torch.bfloat16)
    db[:, :classes] = bf16_round(r["dlogits"])
    if fault == "pad_nonzero" and ld_d > classes:
        db[rows - 1, ld_d - 1] = 2.0 ** -20
    return dict(words=r["words"], nll=r["nll"], dlogits_bf=db, dlogits_f32=r["dlogits"])


def gate_nll(got, logits, target, rows_per_group, coef):
    r64, r32 = (logsoftmax_nll(logits, target, rows_per_group, coef, d) for d in (F64, F32))
    classes = logits.shape[1]
    recs = [rec_f32("words", got["words"], r64["words"], r64["words_mag"], r32["words"])]
    if "nll" in got:
        recs.append(rec_sum("nll", got["nll"], r64["nll"], r64["nll_abs"], r64["nll_n"]))
    if "dlogits_f32" in got:
        recs.append(rec_f32("dlogits_f32", got["dlogits_f32"], r64["dlogits"], r64["dlogits_mag"], r32["dlogits"]))
    if "dlogits_bf" in got:
        d = got["dlogits_bf"].cpu()
        recs.append(rec_bf16("dlogits_bf", d[:, :classes].double(), r64["dlogits"], r64["dlogits_mag"]))
        recs.append(rec_exact("dlogits_bf pads", d[:, classes:].float(), torch.zeros(d.shape[0], d.shape[1] - classes)))
    return recs


# ====================================================================================================== BatchNorm
ACTS = (0, 1, 2)          # none, swish, relu: the codes the plans pass


def bn_inputs(C, ld, G, rows_per_group, seed=None):
    """bf16 r / db / db2 [rows][ld] (pads zero), gamma / beta / running buffers.  Channel 0 is constant within each group (variance 0);
    the last channel (C > 1) has |mean| = 8 standard deviations."""
    g = torch.Generator().manual_seed(7000 + 131 * C + 17 * G + rows_per_group + ld if seed is None else seed)
    rows = G * rows_per_group
    x = torch.randn(rows, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)
    if C > 1:
        x[:, C - 1] = 0.25 * torch.randn(rows, generator=g) + 2.0
    x[:, 0] = torch.tensor([1.3125, -0.40625, 2.5])[torch.arange(rows) // rows_per_group % 3]
    r = torch.zeros(rows, ld, dtype=torch.bfloat16)
    r[:, :C] = bf16_round(x)
    db, db2 = torch.zeros_like(r), torch.zeros_like(r)
    db[:, :C], db2[:, :C] = bf16_round(torch.randn(rows, C, generator=g)), bf16_round(0.5 * torch.randn(rows, C, generator=g))
    return dict(r=r, db=db, db2=db2, gamma=(0.5 + torch.rand(C, generator=g)), beta=torch.randn(C, generator=g),
                running_mean=torch.randn(C, generator=g), running_var=0.5 + torch.rand(C, generator=g), C=C, G=G,
                rows_per_group=rows_per_group, slot_of_row=torch.where(torch.arange(rows) % 4 != 0, (3 * torch.arange(rows) ** 2 + torch.arange(rows)) % STAT_SLOTS, torch.tensor(5)))


def _slots(vals, inp):
    """per-row float64 values [rows][C] -> [G][16][C] float32 partial sums: rows spread unevenly over the slots, some slots empty"""
    G, n, C = inp["G"], inp["rows_per_group"], inp["C"]
    out = torch.zeros(G * STAT_SLOTS, C, dtype=F64)
    out.index_add_(0, torch.arange(G * n) // n * STAT_SLOTS + inp["slot_of_row"], vals.double())
    return out.view(G, STAT_SLOTS, C).float()


def bn_stats(inp):
    """the [G][16][C][2] (sum, sum of squares) slot table a GEMM epilogue would have left, from the bf16 r in float64"""
    x = inp["r"][:, :inp["C"]].double()
    s1, s2 = _slots(x, inp), _slots(x * x, inp)
    # Channel 0 is constant: its partial sums are exact in fp32, E[x^2] - mean^2 would be exactly 0 and the clamp at 0 idle.  An epilogue
    # that accumulates in fp32 may round the sum of squares down: the largest slot gives up 4 ulp of the group's total (still exact
    # fp32 values, and every partial sum of the fold stays exact), so E[x^2] lands a few ulp BELOW mean^2 whatever the contraction,
    # and only the clamp makes the variance the exact 0 the two-pass reference has.
    if inp["rows_per_group"] <= 4096:
        for g in range(inp["G"]):
            tot = float(s2[g, :, 0].double().sum())
            s2[g, int(s2[g, :, 0].argmax()), 0] -= 4.0 * 2.0 ** (math.floor(math.log2(tot)) - 23)
    return torch.stack((s1, s2), -1).contiguous()


def bn_tables(inp, stats=None, training=True, updates=1, skip_mask=0, dtype=F64, fault=None):
    """Two-pass batch statistics of the bf16 r (float64 / float32) -> dict(mean, var, rstd [G][C], affine [G][C][2], running_mean,
    running_var [C], nbt increment) + magnitudes.  torch's running update (momentum 0.1, unbiased variance) once per call a group
    stands for."""
    C, G, n = inp["C"], inp["G"], inp["rows_per_group"]
    gamma, beta = inp["gamma"].to(dtype), inp["beta"].to(dtype)
    rm, rv = inp["running_mean"].to(dtype).clone(), inp["running_var"].to(dtype).clone()
    rm_mag, rv_mag = rm.abs(), rv.abs()
    if not training:
        mean, var = rm.expand(G, C), rv.expand(G, C)
        nbt = 0
    else:
        x = inp["r"][:, :C].to(dtype).view(G, n, C)
        mean = x.mean(1)
        var = ((x - mean[:, None]) ** 2).mean(1)
        nbt = 0
        for g in range(G):
            skipped = (skip_mask >> g) & 1 and fault != "skip_mask_ignored"
            for _ in range(0 if skipped else (1 if fault == "updates_once" else updates)):
                v = var[g] if fault == "biased_running_var" else var[g] * n / (n - 1)
                rm, rm_mag = (1 - BN_MOM) * rm + BN_MOM * mean[g], (1 - BN_MOM) * rm_mag + BN_MOM * x[g].abs().mean(0)
                rv, rv_mag = (1 - BN_MOM) * rv + BN_MOM * v, (1 - BN_MOM) * rv_mag + BN_MOM * v
                nbt += 1
    rstd = 1 / torch.sqrt(var + BN_EPS)
    scale = gamma * rstd
    res = dict(mean=mean, var=var, rstd=rstd, affine=torch.stack((scale, beta - mean * scale), -1), running_mean=rm, running_var=rv, nbt=nbt,
               running_mean_mag=rm_mag, running_var_mag=rv_mag)
    res["mean_mag"] = inp["r"][:, :C].to(dtype).view(G, n, C).abs().mean(1) if training else mean.abs()
    return res


def bn_act(inp, act, training=True, dtype=F64):
    """a = act(r * scale + shift) -> (value [rows][C], magnitude)"""
    C, G, n = inp["C"], inp["G"], inp["rows_per_group"]
    t = bn_tables(inp, training=training, dtype=dtype)
    x = inp["r"][:, :C].to(dtype).view(G, n, C)
    sc, sh = t["affine"][..., 0][:, None], t["affine"][..., 1][:, None]
    y = x * sc + sh
    mag = (x * sc).abs() + inp["beta"].to(dtype).abs() + (t["mean"] * t["affine"][..., 0]).abs()[:, None]
    if act == 1:
        y = y * torch.sigmoid(y)          # |sigmoid| <= 1: the magnitude of the pre-activation bounds it
    elif act == 2:
        y = y.clamp_min(0)
    return y.reshape(G * n, C), mag.reshape(G * n, C)


def bn_red(inp, use_db2=False):
    """[G][16][C][2] (sum db, sum db * xhat) slot table in float64 from the bf16 operands (db + db2 where the second one is given)"""
    C, G, n = inp["C"], inp["G"], inp["rows_per_group"]
    t = bn_tables(inp)
    d = inp["db"][:, :C].double() + (inp["db2"][:, :C].double() if use_db2 else 0.0)
    xh = ((inp["r"][:, :C].double().view(G, n, C) - t["mean"][:, None]) * t["rstd"][:, None]).reshape(G * n, C)
    return torch.stack((_slots(d, inp), _slots(d * xh, inp)), -1).contiguous()


def bn_bwd(inp, use_db2=False, dtype=F64):
    """BatchNorm backward from two-pass statistics: -> dict(dr [rows][C], dgamma, dbeta [C]) + magnitudes"""
    C, G, n = inp["C"], inp["G"], inp["rows_per_group"]
    t = bn_tables(inp, dtype=dtype)
    d = (inp["db"][:, :C].to(dtype) + (inp["db2"][:, :C].to(dtype) if use_db2 else 0.0)).view(G, n, C)
    xh = (inp["r"][:, :C].to(dtype).view(G, n, C) - t["mean"][:, None]) * t["rstd"][:, None]
    s1, s2 = d.mean(1, keepdim=True), (d * xh).mean(1, keepdim=True)
    gr = (inp["gamma"].to(dtype) * t["rstd"])[:, None]
    dr = gr * (d - s1 - xh * s2)
    mag = gr.abs() * (d.abs() + d.abs().mean(1, keepdim=True) + xh.abs() * (d * xh).abs().mean(1, keepdim=True))
    return dict(dr=dr.reshape(G * n, C), dr_mag=mag.reshape(G * n, C), dgamma=(d * xh).sum((0, 1)), dbeta=d.sum((0, 1)),
                dgamma_abs=(d * xh).abs().sum((0, 1)), dbeta_abs=d.abs().sum((0, 1)))


def emulate_bn_finalize(inp, training=True, updates=1, skip_mask=0, fault=None):
    """float32 tables and running buffers (two-pass: the stand-in need not share the kernel's single-pass form)"""
    t = bn_tables(inp, None, training, updates, skip_mask, F32, fault)
    G = inp["G"]
    nbt = t["nbt"]
    return dict(meanrstd=torch.stack((t["mean"].expand(G, -1), t["rstd"].expand(G, -1)), -1), affine=t["affine"].expand(G, -1, -1),
                running_mean=t["running_mean"], running_var=t["running_var"], nbt=nbt)


def gate_bn_tables(got, inp, training=True, updates=1, skip_mask=0):
    """got: meanrstd, affine [G][C][2], running_mean, running_var [C], nbt (the increment)"""
    r64 = bn_tables(inp, None, training, updates, skip_mask, F64)
    r32 = bn_tables(inp, None, training, updates, skip_mask, F32)
    G, C = inp["G"], inp["C"]
    mean, rstd = got["meanrstd"][..., 0], got["meanrstd"][..., 1]
    canc = 1.0 + torch.where(r64["var"] > 0, r64["mean"] ** 2 / r64["var"].clamp_min(1e-300), torch.zeros_like(r64["var"]))
    recs = [rec_f32("mean", mean, r64["mean"].expand(G, C), r64["mean_mag"].expand(G, C), r32["mean"].expand(G, C))]
    if training:
        rel = (rstd.double().cpu() - r64["rstd"]).abs() / r64["rstd"] / canc
        recs.append(Rec("rstd / (1 + mean^2 / var)", float(rel.max()), U22))
    else:
        recs.append(rec_f32("rstd (eval)", rstd, r64["rstd"].expand(G, C), r64["rstd"].expand(G, C), r32["rstd"].expand(G, C)))
    # affine = (gamma rstd, beta - mean gamma rstd): the same bound through its factors
    sc64, sh64 = r64["affine"][..., 0].expand(G, C), r64["affine"][..., 1].expand(G, C)
    cg = canc if training else torch.ones_like(canc)
    recs.append(Rec("scale / (1 + mean^2 / var)", float(((got["affine"][..., 0].double().cpu() - sc64).abs() / sc64.abs() / cg).max()), 2 * U22))
    sh_mag = inp["beta"].double().abs() + (r64["mean"] * r64["affine"][..., 0]).abs().expand(G, C)
    recs.append(Rec("shift / (1 + mean^2 / var)", float(((got["affine"][..., 1].double().cpu() - sh64).abs() / sh_mag / cg).max()), 2 * U22))
    recs.append(rec_f32("running_mean", got["running_mean"], r64["running_mean"], r64["running_mean_mag"], r32["running_mean"]))
    # Per channel: the cancellation bound of the worst group, or 4x the error of the float32 two-pass evaluation IN THAT CHANNEL where
    # that is larger.  The second term is for the roundings of the momentum updates (up to 6 of them), which the cancellation bound does
    # not count: the float32 two-pass evaluation itself measures up to 3.0e-7 / (1 + mean^2 / var) (C = 64, G = 3, 2 rows, 2 updates
    # per group) against the bare 2^-22 = 2.38e-7.  The record is the worst ratio error / gate over the channels (gate 1).
    rel = lambda v: (v.double().cpu() - r64["running_var"]).abs() / r64["running_var_mag"]
    rv_gate = torch.maximum(4 * rel(r32["running_var"]), U22 * canc.max(0).values)
    bad = ~torch.isfinite(got["running_var"].double().cpu())
    ratio = torch.where(bad, torch.full_like(rv_gate, float("inf")), rel(got["running_var"]) / rv_gate)
    recs.append(Rec("running_var error / per-channel gate", float(ratio.max()), 1.0 if training else 0.0))
    recs.append(Rec("num_batches_tracked", float(abs(got["nbt"] - r64["nbt"])), 0.0))
    return recs


def gate_bn_act(got_a, inp, act, training=True):
    """got_a: bf16 [rows][ld]; columns [C, 8 ceil(C / 8)) written as zero"""
    C = inp["C"]
    v, m = bn_act(inp, act, training)
    a = got_a.cpu()
    c8 = (C + 7) // 8 * 8
    # the affine table carries the cancellation bound of rstd: far below a bf16 ulp at these shapes
    return [rec_bf16("a", a[:, :C].double(), v, m), rec_exact("a pads", a[:, C:c8].float(), torch.zeros(a.shape[0], c8 - C))]


def gate_bn_bwd(got, inp, use_db2=False, start=0.0):
    """got: dr bf16 [rows][ld], optionally dgamma / dbeta [C] (started at `start`).  The sums are those of the slot table the test built
    (red, fp32-rounded float64 partials): N = the 16 G slot values folded."""
    C, G = inp["C"], inp["G"]
    r = bn_bwd(inp, use_db2)
    dr = got["dr"].cpu()
    c8 = (C + 7) // 8 * 8
    recs = [rec_bf16("dr", dr[:, :C].double(), r["dr"], r["dr_mag"]), rec_exact("dr pads", dr[:, C:c8].float(), torch.zeros(dr.shape[0], c8 - C))]
    extra = 1 if start else 0
    for n in ("dgamma", "dbeta"):
        if n in got:
            recs.append(rec_sum(n, got[n], r[n] + start, r[n + "_abs"] + abs(start), STAT_SLOTS * G + extra))
    return recs


# ====================================================================================================== embedding, column sums
def gate_colsum(name, got, x, start=0.0):
    """got [cols] = start + column sums of x [rows][cols] (any dtype; summed here in float64)"""
    x = x.double()
    return [rec_sum(name, got, x.sum(0) + start, x.abs().sum(0) + abs(start), x.shape[0] + (1 if start else 0))]


def embed_ref(table, idx, rows, idx_rows, rows_per_group, ld):
    """-> (x bf16 [rows][ld] with zero pads, colstats [G][C][2] float64 of the bf16 values, their absolute sums, terms per sum)"""
    C = table.shape[1]
    x = torch.zeros(rows, ld, dtype=torch.bfloat16)
    x[:, :C] = bf16_round(table[idx[torch.arange(rows) % idx_rows]])
    G = (rows + rows_per_group - 1) // rows_per_group
    xd = x[:, :C].double()
    grp = F.one_hot(torch.arange(rows) // rows_per_group, G).double()
    st = torch.stack((grp.t() @ xd, grp.t() @ (xd * xd)), -1)
    ab = torch.stack((grp.t() @ xd.abs(), grp.t() @ (xd * xd)), -1)
    return x, st, ab, rows_per_group


def scatter_ref(d, idx, nrows_table, C):
    """-> (float64 table [nrows_table][C] of sum_r d[r][:C] at idx[r], absolute sums, most terms into one entry)"""
    t, a = torch.zeros(nrows_table, C, dtype=F64), torch.zeros(nrows_table, C, dtype=F64)
    t.index_add_(0, idx, d[:, :C].double())
    a.index_add_(0, idx, d[:, :C].double().abs())
    return t, a, int(torch.bincount(idx).max())


# ====================================================================================================== stand-alone loss ops
def bce_probs(p, t, dtype=F64):
    """F.binary_cross_entropy(p, t, 'sum') on probabilities -> (sum, sum|terms|, n terms, d/dp per unit coef, its magnitude)"""
    p, t = p.to(dtype), t.to(dtype)
    lp, lq = torch.log(p).clamp_min(-100.0), torch.log(1 - p).clamp_min(-100.0)
    s = -(t * lp + (1 - t) * lq).sum()
    sa = (t * lp.abs().clamp_min(1.0) + (1 - t) * lq.abs().clamp_min(1.0)).sum()
    den = ((1 - p) * p).clamp_min(1e-12)
    return s, sa, 2 * p.numel(), (p - t) / den, (p + t) / den


def mse(a, b, dtype=F64):
    a, b = a.to(dtype), b.to(dtype)
    d = a - b
    return (d * d).sum(), (d * d).sum(), a.numel(), 2 * d, 2 * (a.abs() + b.abs())


def nll_picked(lp, tg, dtype=F64):
    lp = lp.to(dtype)
    v = lp.gather(1, tg.view(-1, 1)).view(-1)
    return -v.sum(), v.abs().sum(), lp.shape[0]


# ====================================================================================================== the cases of tests/test_gpu_elementwise.py
L3_FWD_CASES = [(1, 1), (3, 4), (5, 20), (4, 65), (7, 100), (2, 127)]
L3_FWD_BIG = (600, 100)                    # past the forward launcher's cap of 256 blocks of 256 elements of B * ldz
L3_BWD_B, L3_BWD_D = (1, 3, 4, 5, 9), (1, 20, 64, 65, 100)
L3_BWD_CROSS = (5, 65)                     # the smallest (B, D) with a ragged row block (B % 4 != 0) and a second column block (D > 64)
KL_COEF = (1e-3 / 4, 2.5e-3, 5e-4)
BCE_CASES = [(2, 1, 28, 28, 1), (3, 3, 5, 7, 8), (1, 1, 1, 1, 1)]          # B, C, H, W, ldl
BCE_COEF = (0.5, 0.0, 0.25, 1.0)                                         # group 1: a skipped pass
NLL_CLASSES, NLL_ROWS = (1, 10, 33), (5, 37, 64)
NLL_COEF = (0.2, 0.0, 1.5, 1.0)
BN_C, BN_G, BN_ROWS = (1, 8, 10, 50, 64), (1, 3), (2, 5, 37)
BN_UPDATES, BN_SKIP = (1, 2), (0, 0b010, 0b101)
COLSUM_F32, COLSUM_BF16_LD = [(1, 1), (5, 10), (37, 65), (300, 784)], (8, 24, 56, 2048)
STANDALONE_N = (1, 255, 257, 1000)


def ldz_of(D):
    return (D + 1 + 7) // 8 * 8 + 8          # more than one pad column behind the 1.0


def fwd_mu_logvar32(inp, training=True):
    """the operands of the backward tests: the float64 forward's mu / logvar rounded to fp32"""
    f = latent3_fwd(inp, training, F64)
    return f["mu"].float(), f["logvar"].float()
