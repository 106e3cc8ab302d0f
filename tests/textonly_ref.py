"""float64 reference, bf16-operand emulation, stand-in faults and gates of the text-only VAE step (coco/model.py:120-144,
coco/train_textonly.py:106-120).  Nothing here needs a GPU.

Reference (``step64``): ``oracle.mmvae_ref.coco_text_encoder`` -> the two halves of its output as mu / logvar, untouched (NO product
of experts) -> ``reparametrize`` with the injected eps -> ``coco_text_decoder`` with the injected keep masks -> ``coco_loss`` with the
caption term alone, backward by torch.autograd.

Emulation (``emulate``): the same chain with the two modules of tests/coco_text_ref.py, which round to bf16 what the kernels of the
form that runs round (``forms_of`` restates which form runs at a shape and knob setting).  The latent block rounds nothing.

Gates are the project's own for the COCO step (tests/test_gpu_coco.py): loss rel 1e-3, mu / logvar abs 1e-2, every gradient tensor
rel-L2 4.5e-2, total gradient norm rel 1e-2; the caption output is gated at 4x the emulation's own distance from float64 on the
case (``sentence_gate``; floor: the 2e-5 of the fp32 caption kernels).  A gradient tensor whose reference is below 1e-6 of the total
norm (the hidden weights of the encoder's one-step reverse direction; at T = 1 those of the forward direction) must itself stay
below 1e-4 of the total norm (tests/gradcheck.py).

``fault`` turns the emulation into a stand-in engine with one defect:
  "last_dec_step"  the last decoder step takes no part in the loss
  "no_eps_dlogvar" the eps term is dropped from d_logvar (the value of z is unchanged)
  "mse_3b"         the MSE coefficient is divided by 3 B
  "keep_ignored"   the keep mask of the last step is ignored (a defect only where masks are given)
  "no_reverse"     the encoder's reverse direction is dropped
"""
import torch

from oracle import mmvae_ref as R
import coco_text_ref as CT

H, E = R.COCO_HID, R.COCO_EMB
ENC, DEC = CT.ENC, CT.DEC
GATES = dict(loss=1e-3, mu=1e-2, logvar=1e-2, tensor=4.5e-2, total=1e-2)
SENTENCE_FACTOR, SENTENCE_FLOOR = 4.0, CT.FLOOR_ABS
FAULTS = ("last_dec_step", "no_eps_dlogvar", "mse_3b", "keep_ignored", "no_reverse")

# (T, B, D, keep masks) of tests/test_gpu_textonly.py
CASES = [(1, 3, 20, False), (2, 1, 4, False), (7, 17, 100, True), (5, 23, 120, False), (5, 20, 124, False), (102, 4, 100, False)]
# knob settings the (7, 17, 100) case is repeated under
KNOB_RUNS = [dict(coco_cluster=4), dict(coco_cluster=1), dict(coco_enc_streamed=1)]


def case_id(c):
    return "T%d-B%d-D%d%s" % (c[0], c[1], c[2], "-keep" if c[3] else "")


def forms_of(B, D, knobs=None):
    """(encoder form, decoder form) the one-pass step runs at this shape: resident encoder at B % 4 == 0 unless coco_enc_streamed,
    composed decoder at a cluster of 8 (the default up to 128 row blocks' worth of compute units) and 200 + D <= 320."""
    knobs = knobs or {}
    enc = CT.enc_form(B, knobs.get("coco_enc_streamed", 0))
    cluster = CT.dec_dispatch(B, D, knobs.get("coco_cluster", 8))[-1]
    dec = "composed" if cluster == 8 and not knobs.get("coco_no_comb", 0) and H + D <= 320 else "three"
    return enc, dec


def state_dict_keys(D):
    """The keys of ``TextVAE(D).state_dict()``: the caption half of ``R.param_table`` under ``encoder.`` / ``decoder.``."""
    return [n[len("text_"):] for n, _ in R.param_table("coco", D) if n.startswith((ENC, DEC))]


def state_dict_shapes(D):
    return {n[len("text_"):]: tuple(s) for n, s in R.param_table("coco", D) if n.startswith((ENC, DEC))}


def make_inputs(T, B, D, keep, seed=0):
    """float32 / integer inputs of one case: captions of GloVe-like scale, eps, keep masks (or None)"""
    g = torch.Generator().manual_seed(9000 + 131 * D + 17 * B + 1009 * T + seed)
    text = 0.4 * torch.randn(B, T, E, generator=g)
    eps = torch.randn(B, D, generator=g)
    km = (torch.rand(T, B, H, generator=g) >= R.DROP_P).to(torch.uint8)
    return dict(text=text, eps=eps, keep=km if keep else None)


class _DropGrad(torch.autograd.Function):
    """identity forward, no gradient: the operand of a term a faulty backward leaves out"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return torch.zeros_like(g)


def _chain(P, inp, sos, kl_lambda, lambda_y, training, encoder, decoder, fault=None):
    text = inp["text"].double()
    B, T, _ = text.shape
    out = encoder(P, text)
    D = out.shape[1] // 2
    mu, logvar = out[:, :D], out[:, D:]
    if training:
        lv_z = _DropGrad.apply(logvar) if fault == "no_eps_dlogvar" else logvar
        z = inp["eps"].double() * torch.exp(0.5 * lv_z) + mu          # R.reparametrize's expression
    else:
        z = mu
    keep = inp["keep"] if training else None
    km = None if keep is None else [keep[t].double() for t in range(T)]
    if km is not None and fault == "keep_ignored":
        km[T - 1] = torch.ones_like(km[T - 1]) * (1.0 - R.DROP_P)   # dropout() divides by 0.9: a kept-everywhere, unscaled step
    sent = decoder(P, z, sos.double(), T, km, training)
    if fault == "last_dec_step":
        scored, n = sent[:, :T - 1], B * T * E
        mse = ((scored - text[:, :T - 1]) ** 2).sum() / n if T > 1 else sent.sum() * 0.0
        loss = lambda_y * mse + R.kl_sum(mu, logvar) / B * kl_lambda
    else:
        lam = lambda_y / (3.0 * B) if fault == "mse_3b" else lambda_y
        loss = R.coco_loss(mu, logvar, recon_text=sent, text=text, kl_lambda=kl_lambda, lambda_yx=lam)
    return loss, mu, logvar, sent


def _result(P, loss, mu, logvar, sent, backward):
    grads = {}
    if backward:
        loss.backward()
        zero = torch.zeros(())
        grads = {k: (P[k].grad if P[k].grad is not None else zero.expand_as(P[k]).double()) for k in P}
    return dict(loss=float(loss.detach()), mu=mu.detach(), logvar=logvar.detach(), sentence=sent.detach(), grads=grads)


def step64(P32, inp, sos=None, kl_lambda=1e-3, lambda_y=1.0, training=True, backward=True):
    """The float64 step on float32 parameters {text_encoder.* / text_decoder.*: tensor} -> dict(loss, mu, logvar, sentence, grads)."""
    sos = R.formula_sos() if sos is None else sos
    P = CT.f64(P32, requires_grad=True)

    def dec(P, z, sos, T, km, training):
        return R.coco_text_decoder(P, z, training, sos, T, km, drop_p=R.DROP_P if km is not None else 0.0)
    return _result(P, *_chain(P, inp, sos, kl_lambda, lambda_y, training, R.coco_text_encoder, dec), backward)


def emulate(P32, inp, enc_form, dec_form, sos=None, kl_lambda=1e-3, lambda_y=1.0, rounded=True, fault=None):
    """The training step with bf16 operands where the kernels of (enc_form, dec_form) round them, optionally with one fault."""
    sos = R.formula_sos() if sos is None else sos
    P = CT.f64(P32, requires_grad=True)

    def enc(P, text):
        if fault != "no_reverse":
            return CT.text_encoder(P, text, rounded, enc_form)
        Q = dict(P)
        for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):       # sigmoid(0) / tanh(0) from h = 0: hb = 0
            Q[ENC + "gru.%s_l0_reverse" % k] = P[ENC + "gru.%s_l0_reverse" % k] * 0.0
        return CT.text_encoder(Q, text, rounded, enc_form)

    def dec(P, z, sos, T, km, training):
        return CT.text_decoder(P, z, sos, T, km, rounded, dec_form)
    return _result(P, *_chain(P, inp, sos, kl_lambda, lambda_y, True, enc, dec, fault), True)


# ------------------------------------------------------------------------------------------------ comparisons
def measure(got, ref):
    """loss rel, mu / logvar / sentence max abs, each gradient tensor rel-L2 (`tensors`; `small`: norm / total reference norm of the
    tensors whose reference is below 1e-6 of the total), total gradient norm rel."""
    m = dict(loss=abs(got["loss"] - ref["loss"]) / abs(ref["loss"]))
    for k in ("mu", "logvar", "sentence"):
        m[k] = float((got[k].double().cpu() - ref[k]).abs().max())
    tr = sum(float(g.double().pow(2).sum()) for g in ref["grads"].values()) ** 0.5
    tg = sum(float(got["grads"][k].double().pow(2).sum()) for k in ref["grads"]) ** 0.5
    m["total"] = abs(tg - tr) / tr
    m["tensors"], m["small"] = {}, {}
    for k, gr in ref["grads"].items():
        gh, gr = got["grads"][k].double().cpu().reshape(-1), gr.double().reshape(-1)
        if float(gr.norm()) < 1e-6 * tr:
            m["small"][k] = float(gh.norm()) / tr
        else:
            m["tensors"][k] = float((gh - gr).norm()) / float(gr.norm())
    m["tensor"] = max(m["tensors"].values())
    m["tensor_worst"] = max(m["tensors"], key=m["tensors"].get)
    return m


def sentence_gate(yardstick):
    return max(SENTENCE_FACTOR * yardstick, SENTENCE_FLOOR)


def violations(m, sent_gate):
    """the gates `m` (of ``measure``) misses; empty: it passes"""
    bad = ["%s: %.3e > gate %.1e" % (k, m[k], GATES[k]) for k in ("loss", "mu", "logvar", "total") if not m[k] <= GATES[k]]
    if not m["sentence"] <= sent_gate:
        bad.append("sentence: %.3e > gate %.3e" % (m["sentence"], sent_gate))
    bad += ["grad %s: %.3e > gate %.1e" % (k, v, GATES["tensor"]) for k, v in m["tensors"].items() if not v <= GATES["tensor"]]
    bad += ["grad %s: %.3e of the total norm where the reference is zero" % (k, v) for k, v in m["small"].items() if not v <= 1e-4]
    return bad


def describe(m):
    return "loss rel %.2e | mu %.2e logvar %.2e sentence %.2e abs | grad worst tensor %.3e (%s) total %.2e" % (
        m["loss"], m["mu"], m["logvar"], m["sentence"], m["tensor"], m["tensor_worst"], m["total"])


# ---- the one-expert latent block's backward alone (float64 formula of mmvae_latent1_bwd_f32)
def latent1_bwd_f32_terms(mu, lv, eps, dz, kl_coef, training):
    """-> (value (B, 2D), sum of the absolute terms (B, 2D)): d_mu = dz + kc mu; d_logvar = dz eps exp(lv / 2) / 2 - kc / 2 + kc exp(lv) / 2"""
    mu, lv, dz = mu.double(), lv.double(), dz.double()
    t_mu = (dz, kl_coef * mu)
    t_lv = [-0.5 * kl_coef * torch.ones_like(lv), 0.5 * kl_coef * torch.exp(lv)]
    if training:
        t_lv.append(dz * eps.double() * 0.5 * torch.exp(0.5 * lv))
    val = torch.cat((sum(t_mu), sum(t_lv)), dim=1)
    mag = torch.cat((sum(t.abs() for t in t_mu), sum(t.abs() for t in t_lv)), dim=1)
    return val, mag
