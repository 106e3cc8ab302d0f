"""Importance-sampled log p(x), log p(y) of the COCO model: the two scoring kernels through their hooks (mmvae_coco_iw_tail,
mmvae_coco_iw_text_sse), evaluate.iw_estimate / marginal_table on mmvae_coco_iw_score and the loglik_coco command line, against
float64 (oracle.mmvae_ref).  Captions of 3..5 steps and n_latents 8 / 20 keep every case at a few seconds.

Tolerance rules (those of test_gpu_celeba_loglik.py; every allowance comes from CPU evaluations or from the existing unfused modules).
  * fp32 quantities (``_tol``): the test evaluates the same formula twice on the CPU, in float64 (the reference) and in torch's
    float32, and allows the GPU 16 x the float32 evaluation's worst absolute error.
  * DEVIATION in test 3 (the squared-error sums): the rule above, taken per case, would allow 16 x the float32 error of that
    case's own rows; a one-row case can have a float32 error of exactly zero, which would turn the rule into bit-equality with
    float64 by chance of the data.  Instead the worst RELATIVE error of torch's float32 over all rows of all six cases is taken,
    times 16, times the row's own value.  The measured errors (5.2e-8 relative at most, allowance 2.0e-6) are far inside either
    reading.
  * the tail with an activation: the kernel rounds the activated input to bf16 for the matrix cores.  Allowed: 4 x the worst
    error of a CPU evaluation that does that rounding (and nothing else) against float64 without it.  The weights of those tests
    are multiples of 1/8, exact in bf16.
  * log p(x|z) of the bf16 image decoder: 2 x the worst error of the unfused chain (eval-mode ``vae.image_decoder`` on the same z,
    log terms in float64) against float64, plus 1e-6 max|log p(x|z)|.
  * the caption squared error: 2 x the worst error of eval-mode ``vae.text_decoder`` on the same z (squared error in float64)
    plus the fp32 reduction allowance of test 3.  The scoring call runs the launches of that module, whose recurrence is the
    stepwise fp32 form at EVERY row count (the persistent bf16 kernels belong to the fused training step), so the allowance stays
    far below 1 nat at 4 steps and ``steps`` did not have to be shortened further.  It also means that the 6-row and 8-row cases
    (a row count that is no multiple of 4, and one that is) run ONE caption-decoder form, not two: they differ in the plan's row
    count and in the tiles of the image decoder's and the recurrence's GEMMs only.
  * log p^ / log w columns: a log-sum-exp moves by at most the largest change of its arguments: the sum of the allowances of the
    likelihood terms in the column (the caption's divided by 2 sigma^2) plus 16 x the float32 error of log p(z) - log q(z).
    Nothing is added for the constant -(steps 300 / 2) log(2 pi sigma^2) the y / xy columns carry."""
import ctypes as C
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSTS = ("joint", "image", "text")
ACT_NONE, ACT_SWISH = 0, 1
E = 300


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cast(P, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in P.items()}


def _tol(v32, v64):
    return 16.0 * float((v32.double() - v64).abs().max())


def _check(name, got, want, tol, note=""):
    err = float((got.double().cpu() - want).abs().max())
    print("%-52s  GPU worst error %.3e   allowed %.3e %s" % (name, err, tol, note))
    assert np.isfinite(tol) and err <= tol, (name, err, tol)


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: the scoring tail through its hook

def _tail_case(B, K):
    """-> q3 (rows,16,16,64) NHWC integers in [-4, 4], w (64,3,4,4) multiples of 1/8 in [-1, 1], image (B,3,32,32) in [0, 1]."""
    g = torch.Generator().manual_seed(100 * B + K)
    q3 = torch.randint(-4, 5, (B * K, 16, 16, 64), generator=g).float()
    w = torch.randint(-8, 9, (64, 3, 4, 4), generator=g).float() / 8
    image = torch.rand(B, 3, 32, 32, generator=g)                     # differs per example
    return q3, w, image


def _tail_ref(act_in, w, image, K, dtype):
    """logits (rows,3,32,32) and log p(x|z) (rows,) of the activated NCHW input in ``dtype``."""
    l = F.conv_transpose2d(act_in.to(dtype), w.to(dtype), None, 2, 1)
    x = image.to(dtype).repeat_interleave(K, 0)
    return l, (x * l - F.softplus(l)).sum((1, 2, 3))


def _run_tail(q3, affine, act, w, image, B, K):
    from multimodal_vae_amd._lib import call, ptr
    dev = _dev()
    rows = B * K
    q = q3.to(dev).to(torch.bfloat16).contiguous()
    assert torch.equal(q.float().cpu(), q3)                          # the raw input is exact in bf16
    aff, wd, img = affine.to(dev).contiguous(), w.to(dev).contiguous(), image.to(dev).contiguous()
    ll = torch.full((rows + 1,), float("nan"), device=dev)           # one guard element behind the last
    logits = torch.full((rows + 1, 3, 32, 32), float("nan"), device=dev)
    call("mmvae_coco_iw_tail", ptr(q), ptr(aff), act, ptr(wd), ptr(img), B, K, ptr(ll), ptr(logits), _stream())
    ll2 = torch.full((rows,), float("nan"), device=dev)
    call("mmvae_coco_iw_tail", ptr(q), ptr(aff), act, ptr(wd), ptr(img), B, K, ptr(ll2), None, _stream())   # no dump: same sums
    torch.cuda.synchronize()
    assert torch.isnan(ll[rows]) and torch.isnan(logits[rows]).all()
    assert torch.equal(ll[:rows], ll2)
    return logits[:rows], ll[:rows]


@pytest.mark.parametrize("B,K", [(1, 1), (2, 3)])
def test_tail_exact(B, K):
    """Identity activation, affine (1, 0): every product and every sum of the convolution is exact in fp32, so the dumped logits
    equal float64 conv_transpose2d exactly -- a dropped tap, pixel, channel, border row or a wrong row -> example mapping shows."""
    q3, w, image = _tail_case(B, K)
    affine = torch.tensor([1.0, 0.0]).repeat(64, 1)
    x = q3.permute(0, 3, 1, 2).contiguous()
    l64, ll64 = _tail_ref(x, w, image, K, torch.float64)
    l32, ll32 = _tail_ref(x, w, image, K, torch.float32)
    assert torch.equal(l32.double(), l64)                            # (exact on the CPU too)
    logits, ll = _run_tail(q3, affine, ACT_NONE, w, image, B, K)
    assert torch.equal(logits.double().cpu(), l64)
    _check("tail exact B=%d K=%d log p(x|z)" % (B, K), ll, ll64, _tol(ll32, ll64), "(|ll| up to %.0f)" % float(ll64.abs().max()))


def test_tail_swish_and_affine():
    B, K = 2, 3
    q3, w, image = _tail_case(B, K)
    c = torch.arange(64, dtype=torch.float64)
    scale, shift = 0.6 + 0.3 * torch.sin(0.7 * c), 0.4 * torch.sin(1.3 * c + 0.5)
    affine = torch.stack([scale, shift], 1).float()
    pre = q3.permute(0, 3, 1, 2).double() * affine[:, 0].double().view(1, 64, 1, 1) + affine[:, 1].double().view(1, 64, 1, 1)
    a64 = pre * torch.sigmoid(pre)
    l64, ll64 = _tail_ref(a64, w, image, K, torch.float64)
    lr, llr = _tail_ref(a64.float().to(torch.bfloat16).double(), w, image, K, torch.float64)       # the bf16 rounding alone
    tol_l, tol_ll = 4.0 * float((lr - l64).abs().max()), 4.0 * float((llr - ll64).abs().max())
    logits, ll = _run_tail(q3, affine, ACT_SWISH, w, image, B, K)
    _check("tail swish logits", logits, l64, tol_l, "(bf16 rounding alone %.3e)" % (tol_l / 4))
    _check("tail swish log p(x|z)", ll, ll64, tol_ll, "(bf16 rounding alone %.3e)" % (tol_ll / 4))


def test_tail_rows_beyond_the_grid_are_bit_equal_to_small_calls():
    """More rows than the launch has workgroups (the grid is capped at two workgroups per CU): a workgroup then walks several
    rows, prefetching the next one and reusing its LDS tile and its partial sums.  The 1400 rows of one call must be bit-equal to
    the same rows scored 40 at a time (one row per workgroup, no walk), and a few of them are checked against float64."""
    from multimodal_vae_amd._lib import call, ptr
    dev = _dev()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    rows, part = 1400, 40
    assert rows > 2 * cus, "the device has %d CUs: %d rows do not exceed its grid" % (cus, rows)
    g = torch.Generator().manual_seed(77)
    q3 = torch.randint(-4, 5, (rows, 16, 16, 64), generator=g).float()
    w = torch.randint(-8, 9, (64, 3, 4, 4), generator=g).float() / 8
    image = torch.rand(rows, 3, 32, 32, generator=g)                  # K = 1: every row has its own image
    c = torch.arange(64, dtype=torch.float64)
    affine = torch.stack([0.6 + 0.3 * torch.sin(0.7 * c), 0.4 * torch.sin(1.3 * c + 0.5)], 1).float()
    q, aff, wd, img = q3.to(dev).to(torch.bfloat16).contiguous(), affine.to(dev), w.to(dev), image.to(dev)
    ll = torch.full((rows + 1,), float("nan"), device=dev)
    call("mmvae_coco_iw_tail", ptr(q), ptr(aff), ACT_SWISH, ptr(wd), ptr(img), rows, 1, ptr(ll), None, _stream())
    small = torch.full((rows,), float("nan"), device=dev)
    for r0 in range(0, rows, part):
        call("mmvae_coco_iw_tail", ptr(q[r0:]), ptr(aff), ACT_SWISH, ptr(wd), ptr(img[r0:]), part, 1, ptr(small[r0:]), None, _stream())
    again = torch.full((rows,), float("nan"), device=dev)
    call("mmvae_coco_iw_tail", ptr(q), ptr(aff), ACT_SWISH, ptr(wd), ptr(img), rows, 1, ptr(again), None, _stream())
    torch.cuda.synchronize()
    assert torch.isnan(ll[rows]) and torch.isfinite(ll[:rows]).all()
    assert torch.equal(ll[:rows], small) and torch.equal(ll[:rows], again)
    # the first, some middle and the last rows against float64, by the rule of test_tail_swish_and_affine
    pick = torch.tensor([0, 1, 2 * cus - 1, 2 * cus, 2 * cus + 1, rows - 2, rows - 1])
    pre = q3[pick].permute(0, 3, 1, 2).double() * affine[:, 0].double().view(1, 64, 1, 1) + affine[:, 1].double().view(1, 64, 1, 1)
    a64 = pre * torch.sigmoid(pre)
    _, ll64 = _tail_ref(a64, w, image[pick], 1, torch.float64)
    _, llr = _tail_ref(a64.float().to(torch.bfloat16).double(), w, image[pick], 1, torch.float64)
    _check("tail, rows beyond the grid, log p(x|z)", ll[pick.to(dev)], ll64, 4.0 * float((llr - ll64).abs().max()))


# ---------------------------------------------------------------------------------------------------------------------
# 3: the squared-error reduction through its hook
SSE_CASES = [(steps, B, K) for steps in (1, 5) for (B, K) in ((1, 1), (2, 3), (3, 5))]


def _sse_case(steps, B, K):
    g = torch.Generator().manual_seed(1000 * steps + 10 * B + K)
    return torch.randn(B * K, steps, E, generator=g), 0.4 * torch.randn(B, steps, E, generator=g)


def _sse_ref(sentence, text, K, dtype):
    return (sentence.to(dtype) - text.to(dtype).repeat_interleave(K, 0)).pow(2).sum((1, 2))


@functools.lru_cache(maxsize=None)
def _sse_rel_allowance():
    """16 x the worst relative error of torch's float32 squared-error sum over every row of every case of test 3."""
    worst = 0.0
    for steps, B, K in SSE_CASES:
        s, t = _sse_case(steps, B, K)
        v64 = _sse_ref(s, t, K, torch.float64)
        worst = max(worst, float(((_sse_ref(s, t, K, torch.float32).double() - v64).abs() / v64).max()))
    assert worst > 0
    return 16.0 * worst


def _run_sse(sentence, text, B, K, steps):
    from multimodal_vae_amd._lib import call, ptr
    dev = _dev()
    s, t = sentence.to(dev).contiguous(), text.to(dev).contiguous()
    out = torch.full((B * K + 1,), float("nan"), device=dev)
    call("mmvae_coco_iw_text_sse", ptr(s), ptr(t), B, K, steps, ptr(out), _stream())
    torch.cuda.synchronize()
    assert torch.isnan(out[B * K]) and torch.isfinite(out[:B * K]).all()
    return out[:B * K]


@pytest.mark.parametrize("steps,B,K", SSE_CASES)
def test_text_sse(steps, B, K):
    sentence, text = _sse_case(steps, B, K)
    v64 = _sse_ref(sentence, text, K, torch.float64)
    got = _run_sse(sentence, text, B, K, steps)
    rel = _sse_rel_allowance()
    err = ((got.double().cpu() - v64).abs() / v64)
    print("sse steps=%d B=%d K=%d  GPU worst relative error %.3e   allowed %.3e" % (steps, B, K, float(err.max()), rel))
    assert float(err.max()) <= rel
    assert torch.equal(got, _run_sse(sentence, text, B, K, steps))    # a second call: bit-equal
    # the last row again as the only row of another batch (its own example alone): independent of the rows around it
    b = B - 1
    alone = _run_sse(sentence[B * K - 1:], text[b:], 1, 1, steps)
    assert torch.equal(alone, got[B * K - 1:])
    if K > 1:                                                         # ... and as the first of the last example's K rows
        part = _run_sse(sentence[b * K:], text[b:], 1, K, steps)
        assert torch.equal(part, got[b * K:])


# ---------------------------------------------------------------------------------------------------------------------
def _stats(P, prefixes):
    """Running means / variances that matter (the formula model's are (0, 1))."""
    for k in list(P):
        if k.startswith(prefixes):
            n = torch.arange(P[k].numel(), dtype=torch.float32)
            if k.endswith("running_mean"):
                P[k] = 0.3 * torch.sin(0.7 * n)
            elif k.endswith("running_var"):
                P[k] = 1.0 + 0.5 * torch.cos(0.3 * n)
    return P


def _vae(P, D, steps):
    from multimodal_vae_amd import coco as M
    from oracle import mmvae_ref as R
    vae = M.MultimodalVAE(D, sos=R.formula_sos(), steps=steps)
    vae.load_state_dict({k: v.clone() for k, v in P.items()}, strict=True)
    vae.cuda()
    vae.eval()
    return vae


def _inputs(B, steps):
    from oracle import mmvae_ref as R
    image, text = R.formula_inputs("coco", B)
    return image, text[:, :steps].contiguous()


def _image_logits(P, z):
    """coco/model.py:197-216 without the sigmoid (oracle.mmvae_ref.coco_image_decoder restated up to the logit)."""
    from oracle import mmvae_ref as R
    pre = "image_decoder."
    x = R.swish(F.linear(z, P[pre + "upsample.0.weight"], P[pre + "upsample.0.bias"])).view(-1, 512, 2, 2)
    x = R.swish(R.batch_norm(F.conv_transpose2d(x, P[pre + "hallucinate.0.weight"], None, 2, 1), P, pre + "hallucinate.1", False))
    x = R.swish(R.batch_norm(F.conv_transpose2d(x, P[pre + "hallucinate.3.weight"], None, 2, 1), P, pre + "hallucinate.4", False))
    x = R.swish(R.batch_norm(F.conv_transpose2d(x, P[pre + "hallucinate.6.weight"], None, 2, 1), P, pre + "hallucinate.7", False))
    return F.conv_transpose2d(x, P[pre + "hallucinate.9.weight"], None, 2, 1)


# 4: end to end given particles
D4, S4, B4 = 20, 4, 2


@functools.lru_cache(maxsize=None)
def _model4():
    from oracle import mmvae_ref as R
    P = _stats(R.formula_params("coco", D4), ("image_decoder.",))
    return P, _cast(P, torch.float64), _vae(P, D4, S4)


def _score(vae, z, image, text):
    """mmvae_coco_iw_score on z (B,K,D): -> log p(x|z) (B,K), sse (B,K) exactly as the kernels wrote them."""
    from multimodal_vae_amd._lib import call, ptr
    B, K, D = z.shape
    st = vae._core.sync(z.device)
    h = st.plan(B * K)
    wsb = call("mmvae_coco_iw_workspace_bytes", h)
    ws = torch.empty(wsb, dtype=torch.uint8, device=z.device)
    lx, sse = torch.empty(B, K, device=z.device), torch.empty(B, K, device=z.device)
    sos = vae.text_decoder.sos.to(z.device).contiguous()
    call("mmvae_coco_iw_score", h, ptr(ws), wsb, ptr(z.contiguous()), ptr(image.contiguous().float()), ptr(text.contiguous().float()),
         ptr(sos), B, K, ptr(lx), ptr(sse), _stream())
    torch.cuda.synchronize()
    return lx, sse


@functools.lru_cache(maxsize=None)
def _parity(post, K):
    """The float64 reference, the GPU results and the allowances of one posterior at B4 * K rows (computed once, shared)."""
    from multimodal_vae_amd.evaluate import coco_text_constant, iw_estimate
    from oracle import mmvae_ref as R
    dev = _dev()
    P, P64, vae = _model4()
    image, text = _inputs(B4, S4)
    sos = R.formula_sos()
    eps = torch.randn(B4, K, D4, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    const = coco_text_constant(S4, 1.0)
    with torch.no_grad():
        _, _, mu, lv = R.coco_forward(P64, image.double() if post != "text" else None, text.double() if post != "image" else None, False,
                                      sos.double(), steps=S4)

        def ratio(mu, lv, eps):
            z = mu.unsqueeze(1) + lv.mul(0.5).exp().unsqueeze(1) * eps
            return z, (-0.5 * z.pow(2) + 0.5 * eps.pow(2) + 0.5 * lv.unsqueeze(1)).sum(2)      # log p(z) - log q(z)
        z64, lr64 = ratio(mu, lv, eps)
        _, lr32 = ratio(mu.float(), lv.float(), eps.float())
        zf = z64.reshape(B4 * K, D4)
        l64 = _image_logits(P64, zf)
        lx64 = (image.double().repeat_interleave(K, 0) * l64 - F.softplus(l64)).sum((1, 2, 3)).view(B4, K)
        y64 = R.coco_text_decoder(P64, zf, False, sos.double(), S4)
        sse64 = _sse_ref(y64, text.double(), K, torch.float64).view(B4, K)
    ly64 = -0.5 * sse64 + const
    lp64 = torch.stack([torch.logsumexp(lx64 + lr64, 1), torch.logsumexp(ly64 + lr64, 1), torch.logsumexp(lx64 + ly64 + lr64, 1)], 1) - np.log(K)
    img, txt = image.to(dev), text.to(dev)
    r = iw_estimate(vae, img, txt, mu.float().to(dev), lv.float().to(dev), K, eps=eps.float().to(dev), return_log_w=True, return_z=True)
    # the existing unfused modules on the same z: eval-mode decoders, log terms / squared error in float64
    zg = r["z"].reshape(B4 * K, D4)
    with torch.no_grad():
        p = vae.image_decoder(zg).double().cpu()
        yu = vae.text_decoder(zg).double().cpu()
    x = image.double().repeat_interleave(K, 0)
    lx_unf = (x * p.log() + (1 - x) * torch.log1p(-p)).sum((1, 2, 3)).view(B4, K)
    sse_unf = _sse_ref(yu, text.double(), K, torch.float64).view(B4, K)
    unf_x, unf_y = float((lx_unf - lx64).abs().max()), float((sse_unf - sse64).abs().max())
    tol = {"x": 2.0 * unf_x + 1e-6 * float(lx64.abs().max()), "sse": 2.0 * unf_y + _sse_rel_allowance() * float(sse64.max()),
           "r": _tol(lr32, lr64), "unf_x": unf_x, "unf_y": unf_y}
    tol["y"] = 0.5 * tol["sse"]                                       # sigma = 1: log p(y|z) = -sse / 2 + const
    lx_direct, sse_direct = _score(vae, r["z"], img, txt)
    return dict(r=r, lx64=lx64, ly64=ly64, sse64=sse64, lr64=lr64, lp64=lp64, tol=tol, lx_direct=lx_direct, sse_direct=sse_direct)


@pytest.mark.parametrize("K", [3, 4])          # 6 rows and 8 rows: a row count that is no multiple of 4, and one that is
@pytest.mark.parametrize("post", POSTS)
def test_iw_oracle_parity_given_particles(post, K):
    c = _parity(post, K)
    r, tol = c["r"], c["tol"]
    lw = r["log_w"]
    assert lw.shape == (B4, K, 3) and r["log_p"].shape == (B4, 3) and r["sse"].shape == (B4, K)
    tag = "D=%d steps=%d rows=%d %s" % (D4, S4, B4 * K, post)
    assert tol["sse"] < 1.0, tol
    _check(tag + " log p(x|z) [log_w]", lw[..., 2] - lw[..., 1], c["lx64"], tol["x"], "(unfused chain %.3e)" % tol["unf_x"])
    _check(tag + " log p(x|z) [scoring call]", c["lx_direct"], c["lx64"], tol["x"], "(unfused chain %.3e)" % tol["unf_x"])
    _check(tag + " sse [scoring call]", c["sse_direct"], c["sse64"], tol["sse"], "(unfused module %.3e)" % tol["unf_y"])
    _check(tag + " sse [iw_estimate]", r["sse"], c["sse64"], tol["sse"], "(unfused module %.3e)" % tol["unf_y"])
    cols = (("log p^(x)", tol["x"] + tol["r"]), ("log p^(y)", tol["y"] + tol["r"]), ("log p^(x,y)", tol["x"] + tol["y"] + tol["r"]))
    for i, (nm, t) in enumerate(cols):
        want = (c["lx64"], c["ly64"], c["lx64"] + c["ly64"])[i] + c["lr64"]
        _check("%s %s" % (tag, nm), r["log_p"][:, i], c["lp64"][:, i], t)
        _check("%s log_w column %d" % (tag, i), lw[..., i], want, t)
    ess = r["ess"]
    assert torch.isfinite(ess).all() and (ess >= 1 - 1e-4).all() and (ess <= K * (1 + 1e-4)).all(), ess
    # the caption NLL is the mean over the particles of sse / 2 - const
    _check(tag + " caption nll", r["nll"][:, 1], -c["ly64"].mean(1), tol["y"])


# ---------------------------------------------------------------------------------------------------------------------
# 5
def test_iw_exact_when_decoders_ignore_z():
    """With every z path of the two decoders zeroed, p(x|z) p(y|z) is a constant c, and with q = p (mu = 0, logvar = 0) every
    weight is c: log p^ = log c for any K, ESS = K, and the reconstruction NLLs are -log p^."""
    from multimodal_vae_amd.evaluate import iw_estimate
    from oracle import mmvae_ref as R
    dev = _dev()
    D, B, steps = 8, 3, 3
    P = R.formula_params("coco", D)
    P["image_decoder.upsample.0.weight"].zero_()
    P["text_decoder.z2h.weight"].zero_()
    P["text_decoder.gru.weight_ih_l0"][:, E:].zero_()
    P["text_decoder.h2o.weight"][:, 200:].zero_()
    vae = _vae(P, D, steps)
    image, text = _inputs(B, steps)
    image, text = image.to(dev), text.to(dev)
    mu = torch.zeros(B, D, device=dev)
    for K in (1, 7, 64):
        r = iw_estimate(vae, image, text, mu, torch.zeros_like(mu), K, seed=5, return_log_w=True)
        lw = r["log_w"].double().cpu()
        spread = (lw.max(1).values - lw.min(1).values).abs()
        assert (spread <= 1e-6 * lw.abs().max(1).values).all(), (K, spread)
        np.testing.assert_allclose(r["ess"].double().cpu().numpy(), np.full((B, 3), K), rtol=1e-4)
        np.testing.assert_allclose(r["nll"].double().cpu().numpy(), -r["log_p"][:, :2].double().cpu().numpy(), rtol=1e-5)
        sse = r["sse"].double().cpu()
        assert (sse.max(1).values - sse.min(1).values <= 1e-6 * sse.max(1).values).all()


# 6
def test_iw_chunk_and_batch_invariance():
    from multimodal_vae_amd.evaluate import _proposal, iw_estimate
    dev = _dev()
    B, K = 4, 6
    _, _, vae = _model4()
    image, text = _inputs(B, S4)
    image, text = image.to(dev), text.to(dev)
    with torch.no_grad():
        mu, lv = _proposal(vae, image, text, "joint")
    kw = dict(seed=21, return_z=True, return_log_w=True)
    full = iw_estimate(vae, image, text, mu, lv, K, **kw)                               # one call of 24 rows
    for ppc in (1, 3):                                                                  # 6 calls of 4 rows, 2 calls of 12 rows
        part = iw_estimate(vae, image, text, mu, lv, K, particles_per_call=ppc, **kw)
        assert torch.equal(part["z"], full["z"])
        d = (part["log_w"].double() - full["log_w"].double()).abs().amax((0, 1)).cpu().tolist()
        print("log_w, %d particles per call against one call: worst difference %s (bit-equal asked)" % (ppc, d))
        assert torch.equal(part["log_w"], full["log_w"]), (ppc, d)
        assert torch.equal(part["sse"], full["sse"])
    # example 2 alone, first_row = 2: the same particles; 6 rows there (no multiple of 4) against 24 here
    alone = iw_estimate(vae, image[2:3], text[2:3], mu[2:3], lv[2:3], K, first_row=2, **kw)
    assert torch.equal(alone["z"], full["z"][2:3])
    tol = _parity("joint", 3)["tol"]
    allowed = (tol["x"] + tol["r"], tol["y"] + tol["r"], tol["x"] + tol["y"] + tol["r"])
    d = (alone["log_w"].double() - full["log_w"][2:3].double()).abs().amax((0, 1)).cpu()
    print("log_w, an example alone (6 rows) against inside the batch (24 rows): worst difference %s   allowed %s" % (d.tolist(), list(allowed)))
    assert all(float(d[i]) <= allowed[i] for i in range(3)), (d, allowed)
    # ... and with 8 particles both row counts (8, 32) are multiples of 4: bit-equal
    full8 = iw_estimate(vae, image, text, mu, lv, 8, **kw)
    alone8 = iw_estimate(vae, image[2:3], text[2:3], mu[2:3], lv[2:3], 8, first_row=2, **kw)
    assert torch.equal(alone8["z"], full8["z"][2:3])
    d8 = (alone8["log_w"].double() - full8["log_w"][2:3].double()).abs().amax((0, 1)).cpu().tolist()
    print("log_w, an example alone (8 rows) against inside the batch (32 rows): worst difference %s (bit-equal asked)" % d8)
    assert torch.equal(alone8["log_w"], full8["log_w"][2:3]), d8
    other = iw_estimate(vae, image, text, mu, lv, K, seed=22, return_z=True)
    assert not torch.equal(other["z"], full["z"])


# 7
def test_text_sigma_moves_the_caption_columns_as_the_formula_says():
    from multimodal_vae_amd.evaluate import _proposal, coco_text_constant, iw_estimate
    dev = _dev()
    B, K = 2, 4
    _, _, vae = _model4()
    image, text = _inputs(B, S4)
    image, text = image.to(dev), text.to(dev)
    with torch.no_grad():
        mu, lv = _proposal(vae, image, text, "image")
    one = iw_estimate(vae, image, text, mu, lv, K, seed=4, return_log_w=True)
    sse = one["sse"].double().cpu()
    base = one["log_w"][..., 1].double().cpu() + 0.5 * sse - coco_text_constant(S4, 1.0)      # log p(z) - log q(z) as this run had it
    for sigma in (0.5, 2.0):
        r = iw_estimate(vae, image, text, mu, lv, K, seed=4, return_log_w=True, text_sigma=sigma)
        assert torch.equal(r["sse"], one["sse"])
        assert torch.equal(r["log_w"][..., 0], one["log_w"][..., 0]) and torch.equal(r["log_p"][:, 0], one["log_p"][:, 0])
        want = base - sse / (2 * sigma ** 2) + coco_text_constant(S4, sigma)
        # fp32 roundings on the way: sum with the ratio and shift by the constant, in this run and in the sigma = 1 run `base`
        # comes from (the products by -1/2, -2 and -1/8 are exact): at most 4 half-units of the largest magnitude involved
        ulp = 2.0 ** -23 * max(float(want.abs().max()), float(one["log_w"][..., 1].abs().max()), abs(coco_text_constant(S4, sigma)))
        _check("text_sigma=%.1f log_w y column" % sigma, r["log_w"][..., 1], want, 2.0 * ulp)
        d = r["log_w"][..., 2].double().cpu() - r["log_w"][..., 1].double().cpu() - (one["log_w"][..., 2].double().cpu() - one["log_w"][..., 1].double().cpu())
        assert float(d.abs().max()) <= 4.0 * 2.0 ** -23 * float(one["log_w"][..., 2].abs().max())   # xy - y = log p(x|z), sigma-free
    with pytest.raises(ValueError):
        iw_estimate(vae, image, text, mu, lv, K, text_sigma=0.0)
    with pytest.raises(ValueError):
        iw_estimate(vae, image, text[:, :3], mu, lv, K)               # captions of another length than the model's steps


# 8
def test_marginal_table_has_no_side_effects():
    from multimodal_vae_amd.coco import FusedTrainer
    from multimodal_vae_amd.evaluate import marginal_table
    from oracle import mmvae_ref as R
    _dev()
    P = _stats(R.formula_params("coco", D4), ("image_decoder.", "image_encoder."))
    vae, twin = _vae(P, D4, S4), _vae(P, D4, S4)
    image, text = _inputs(7, S4)
    loader = [(image[:4], text[:4]), (image[4:], text[4:])]                      # a partial last batch
    before = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    assert any(k.endswith("num_batches_tracked") for k in before) and any(k.endswith("running_var") for k in before)
    table = marginal_table(vae, loader, n_particles=5, seed=3, text_sigma=1.0)
    torch.cuda.synchronize()
    after = vae.state_dict()
    assert set(after) == set(before)
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    assert set(table) == set(POSTS)
    for post in POSTS:
        t = table[post]
        assert t["n"] == 7 and t["log_p"].shape == (7, 3) and t["ess"].shape == (7, 3)
        assert all(np.isfinite(t[k]) for k in ("log_px", "log_py", "log_pxy", "image_nll", "text_nll"))
        assert t["log_px"] < 0 and t["log_py"] < 0 and t["image_nll"] > 0 and t["text_nll"] > 0
    # a training step after the evaluation gives the loss of the same step on a model that was never evaluated
    dev = next(vae.parameters()).device
    img, txt = image[:4].to(dev).contiguous(), text[:4].to(dev).contiguous()
    vae.train(); twin.train()
    got = FusedTrainer(vae, 4, seed=11)(img, txt).losses().double().cpu()
    want = FusedTrainer(twin, 4, seed=11)(img, txt).losses().double().cpu()
    print("training step after marginal_table: losses %s   without it %s" % (got.tolist(), want.tolist()))
    assert torch.isfinite(want).all()
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-6, atol=0)     # (the loss sums are fp32 atomics: order only)


# 9
def test_loglik_coco_cli(tmp_path):
    from multimodal_vae_amd.train import save_checkpoint
    from oracle import mmvae_ref as R
    _dev()
    D, K = 20, 4
    P = R.formula_params("coco", D)
    save_checkpoint({"state_dict": {k: v.clone() for k, v in P.items()}, "n_latents": D}, False, folder=str(tmp_path))
    out = tmp_path / "bounds.json"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "multimodal_vae_amd.evaluate", "loglik_coco", str(tmp_path / "checkpoint.pth.tar"), "--all",
           "--synthetic", "8", "--n_samples", str(K), "--text_sigma", "2.0", "--json", str(out)]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Test Image NLL: " in p.stdout and "\tTest Text NLL: " in p.stdout, p.stdout
    res = json.loads(out.read_text())
    assert set(res) == {"n_samples", "n_examples", "seed", "text_sigma", "joint", "image", "text"}
    assert res["n_samples"] == K and res["n_examples"] == 8 and res["seed"] == 0 and res["text_sigma"] == 2.0
    for post in POSTS:
        assert set(res[post]) == {"log_px", "log_py", "log_pxy", "image_nll", "text_nll", "mean_ess"}
        assert all(math.isfinite(res[post][k]) for k in ("log_px", "log_py", "log_pxy", "image_nll", "text_nll"))
        assert len(res[post]["mean_ess"]) == 3 and all(1 - 1e-4 <= e <= K * (1 + 1e-4) for e in res[post]["mean_ess"])
        # the constant of sigma = 2 at 102 steps (about -49,330) is in the caption columns
        const = -0.5 * 102 * 300 * math.log(2 * math.pi * 4.0)
        assert abs(res[post]["log_py"] - const) < 0.1 * abs(const) and abs(res[post]["text_nll"] + const) < 0.1 * abs(const)
