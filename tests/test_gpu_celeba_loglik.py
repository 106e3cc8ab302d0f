"""Importance-sampled log p(x), log p(y) of the CelebA model: the two scoring kernels through their hooks
(mmvae_celeba_iw_tail, mmvae_celeba_iw_attrs), evaluate.iw_estimate / log_marginal / marginal_table on mmvae_celeba_iw_score and
the loglik_celeba command line, against float64 (oracle.mmvae_ref).

Tolerance rules.
  * fp32 quantities (``_tol``, the rule of test_gpu_mnist_loglik.py): the test evaluates the same formula twice on the CPU, in
    float64 (the reference) and in torch's float32, and allows the GPU 16 x the float32 evaluation's worst absolute error: the
    kernels sum in another order and use other exp / log implementations.
  * the tail with an activation: the kernel rounds the activated input to bf16 for the matrix cores.  Allowed: 4 x the worst
    error of a CPU evaluation that does that rounding (and nothing else) against float64 without it; the factor covers roundings
    that flip because the GPU's Swish differs from the CPU's in the last fp32 bit.  The weights of those tests are multiples of
    1/8, exact in bf16, so that the kernel's rounding of the weights contributes nothing.
  * log p(x|z) of the bf16 image decoder: 2 x the worst error of the existing unfused chain (eval-mode ``vae.image_decoder`` on the
    same z, log terms in float64) against the same float64 values, plus 1e-6 max|log p(x|z)|: the scorer runs the same bf16 body,
    the factor covers a plan of another row count picking another kernel instantiation.
  * log p^ columns: a log-sum-exp moves by at most the largest change of its arguments, so the allowance is the sum of those of
    the likelihood terms in the column plus 16 x the float32 error of log p(z) - log q(z).
Every row is compared: CelebA has no greedy feedback, so there are no ties to leave out."""
import ctypes as C
import functools
import json
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
NA = 18


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
    print("%-44s  GPU worst error %.3e   allowed %.3e %s" % (name, err, tol, note))
    assert np.isfinite(tol) and err <= tol, (name, err, tol)


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: the scoring tail through its hook

def _tail_case(B, K):
    """-> q3 (rows,32,32,32) NHWC integers in [-4, 4], w (32,3,4,4) multiples of 1/8 in [-1, 1], image (B,3,64,64) in [0, 1]."""
    g = torch.Generator().manual_seed(100 * B + K)
    q3 = torch.randint(-4, 5, (B * K, 32, 32, 32), generator=g).float()
    w = torch.randint(-8, 9, (32, 3, 4, 4), generator=g).float() / 8
    image = torch.rand(B, 3, 64, 64, generator=g)                     # differs per example
    return q3, w, image


def _tail_ref(act_in, w, image, K, dtype):
    """logits (rows,3,64,64) and log p(x|z) (rows,) of the activated NCHW input in ``dtype``."""
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
    ll = torch.full((rows,), float("nan"), device=dev)
    logits = torch.full((rows, 3, 64, 64), float("nan"), device=dev)
    call("mmvae_celeba_iw_tail", ptr(q), ptr(aff), act, ptr(wd), ptr(img), B, K, ptr(ll), ptr(logits), _stream())
    ll2 = torch.full((rows,), float("nan"), device=dev)
    call("mmvae_celeba_iw_tail", ptr(q), ptr(aff), act, ptr(wd), ptr(img), B, K, ptr(ll2), None, _stream())   # no dump: same sums
    torch.cuda.synchronize()
    assert torch.equal(ll, ll2)
    return logits, ll


@pytest.mark.parametrize("B,K", [(1, 1), (2, 3)])
def test_tail_exact(B, K):
    """Identity activation, affine (1, 0): every product and every sum of the convolution is exact in fp32, so the dumped logits
    equal float64 conv_transpose2d exactly -- a dropped tap, pixel, channel, border row or a wrong row -> example mapping shows."""
    q3, w, image = _tail_case(B, K)
    affine = torch.tensor([1.0, 0.0]).repeat(32, 1)
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
    c = torch.arange(32, dtype=torch.float64)
    scale, shift = 0.6 + 0.3 * torch.sin(0.7 * c), 0.4 * torch.sin(1.3 * c + 0.5)
    affine = torch.stack([scale, shift], 1).float()
    pre = q3.permute(0, 3, 1, 2).double() * affine[:, 0].double().view(1, 32, 1, 1) + affine[:, 1].double().view(1, 32, 1, 1)
    a64 = pre * torch.sigmoid(pre)
    l64, ll64 = _tail_ref(a64, w, image, K, torch.float64)
    lr, llr = _tail_ref(a64.float().to(torch.bfloat16).double(), w, image, K, torch.float64)       # the bf16 rounding alone
    tol_l, tol_ll = 4.0 * float((lr - l64).abs().max()), 4.0 * float((llr - ll64).abs().max())
    logits, ll = _run_tail(q3, affine, ACT_SWISH, w, image, B, K)
    _check("tail swish logits", logits, l64, tol_l, "(bf16 rounding alone %.3e)" % (tol_l / 4))
    _check("tail swish log p(x|z)", ll, ll64, tol_ll, "(bf16 rounding alone %.3e)" % (tol_ll / 4))


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


def _vae(P, D):
    from multimodal_vae_amd import celeba as M
    vae = M.MultimodalVAE(D)
    vae.load_state_dict({k: v.clone() for k, v in P.items()}, strict=True)
    vae.cuda()
    vae.eval()
    return vae


def _attr_logits(P, z):
    """celeba/model.py:181-196 without the sigmoid, from the oracle's helpers, in the dtype of P / z."""
    from oracle import mmvae_ref as R
    x = F.linear(z, P["attrs_decoder.net.0.weight"], P["attrs_decoder.net.0.bias"])
    x = R.swish(R.batch_norm(x, P, "attrs_decoder.net.1", False))
    return F.linear(x, P["attrs_decoder.net.3.weight"], P["attrs_decoder.net.3.bias"])


def _image_logits(P, z):
    """celeba/model.py:131-161 without the sigmoid (oracle.mmvae_ref.celeba_image_decoder restated up to the logit)."""
    from oracle import mmvae_ref as R
    pre = "image_decoder."
    x = R.swish(F.linear(z, P[pre + "upsample.0.weight"], P[pre + "upsample.0.bias"])).view(-1, 256, 5, 5)
    x = R.swish(R.batch_norm(F.conv_transpose2d(x, P[pre + "hallucinate.0.weight"], None, 1, 0), P, pre + "hallucinate.1", False))
    x = R.swish(R.batch_norm(F.conv_transpose2d(x, P[pre + "hallucinate.3.weight"], None, 2, 1), P, pre + "hallucinate.4", False))
    x = R.swish(R.batch_norm(F.conv_transpose2d(x, P[pre + "hallucinate.6.weight"], None, 2, 1), P, pre + "hallucinate.7", False))
    return F.conv_transpose2d(x, P[pre + "hallucinate.9.weight"], None, 2, 1)


def _words(a):
    return torch.stack([-F.softplus(a), a - F.softplus(a)], -1)


@pytest.mark.parametrize("D", [20, 100])
@pytest.mark.parametrize("rows", [15, 133])
def test_attribute_scorer(D, rows):
    """Row counts below one 64-row tile and over two tiles with a partial third; BatchNorm statistics that matter."""
    from multimodal_vae_amd._lib import call, ptr
    from oracle import mmvae_ref as R
    dev = _dev()
    P = _stats(R.formula_params("celeba", D), ("attrs_decoder.",))
    vae = _vae(P, D)
    st = vae._core.sync(dev)
    z = 1.5 * torch.randn(rows, D, generator=torch.Generator().manual_seed(rows + D))
    with torch.no_grad():
        a64 = _attr_logits(_cast(P, torch.float64), z.double())
        a32 = _attr_logits(P, z)
    zd = z.to(dev).contiguous()
    words = torch.full((rows + 1, NA, 2), float("nan"), device=dev)          # one guard row behind the last
    call("mmvae_celeba_iw_attrs", st.plan(1), ptr(zd), rows, ptr(words), _stream())
    torch.cuda.synchronize()
    assert torch.isnan(words[rows]).all() and torch.isfinite(words[:rows]).all()
    words = words[:rows]
    tag = "attrs D=%d rows=%d" % (D, rows)
    _check(tag + " words", words, _words(a64), _tol(_words(a32), _words(a64)))
    one = float((words.double().exp().sum(-1) - 1).abs().max())
    print("%-44s  |p + (1 - p) - 1| worst %.3e   allowed 1e-06" % (tag, one))
    assert one <= 1e-6
    w32 = _words(a32)
    _check(tag + " log p - log(1 - p) = logit", words[..., 1] - words[..., 0], a64, _tol(w32[..., 1] - w32[..., 0], a64))


# ---------------------------------------------------------------------------------------------------------------------
# 4: end to end given particles
D4, B4, K4 = 100, 13, 8


@functools.lru_cache(maxsize=None)
def _model4():
    from oracle import mmvae_ref as R
    P = _stats(R.formula_params("celeba", D4), ("image_decoder.", "attrs_decoder."))
    return P, _cast(P, torch.float64), _vae(P, D4)


def _score(vae, z, image):
    """mmvae_celeba_iw_score on z (B,K,D): -> log p(x|z) (B,K), words (B,K,18,2) exactly as the kernels wrote them."""
    from multimodal_vae_amd._lib import call, ptr
    B, K, D = z.shape
    st = vae._core.sync(z.device)
    h = st.plan(B * K)
    wsb = call("mmvae_celeba_iw_workspace_bytes", h)
    ws = torch.empty(wsb, dtype=torch.uint8, device=z.device)
    lx = torch.empty(B, K, device=z.device)
    words = torch.empty(B, K, NA, 2, device=z.device)
    call("mmvae_celeba_iw_score", h, ptr(ws), wsb, ptr(z.contiguous()), ptr(image.contiguous().float()), B, K, ptr(lx), ptr(words), _stream())
    torch.cuda.synchronize()
    return lx, words


@functools.lru_cache(maxsize=None)
def _parity(post):
    """The float64 reference, the GPU results and the allowances of one posterior (computed once, shared by the tests)."""
    from multimodal_vae_amd.evaluate import iw_estimate
    from oracle import mmvae_ref as R
    dev = _dev()
    P, P64, vae = _model4()
    image, attrs = R.formula_inputs("celeba", B4)
    eps = torch.randn(B4, K4, D4, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    with torch.no_grad():
        _, _, mu, lv = R.celeba_forward(P64, image.double() if post != "text" else None, attrs.double() if post != "image" else None, False)

        def terms(Pd, mu, lv, eps):
            z = mu.unsqueeze(1) + lv.mul(0.5).exp().unsqueeze(1) * eps
            a = _attr_logits(Pd, z.reshape(B4 * K4, D4)).view(B4, K4, NA)
            y = attrs.to(z.dtype).unsqueeze(1)
            ly = (y * a - F.softplus(a)).sum(2)
            lr = (-0.5 * z.pow(2) + 0.5 * eps.pow(2) + 0.5 * lv.unsqueeze(1)).sum(2)          # log p(z) - log q(z)
            return z, ly, lr
        z64, ly64, lr64 = terms(P64, mu, lv, eps)
        _, ly32, lr32 = terms(P, mu.float(), lv.float(), eps.float())
        l64 = _image_logits(P64, z64.reshape(B4 * K4, D4))
        lx64 = (image.double().repeat_interleave(K4, 0) * l64 - F.softplus(l64)).sum((1, 2, 3)).view(B4, K4)
    lp64 = torch.stack([torch.logsumexp(lx64 + lr64, 1), torch.logsumexp(ly64 + lr64, 1), torch.logsumexp(lx64 + ly64 + lr64, 1)], 1) - np.log(K4)
    img, att = image.to(dev), attrs.to(dev)
    r = iw_estimate(vae, img, att, mu.float().to(dev), lv.float().to(dev), K4, eps=eps.float().to(dev), return_log_w=True, return_z=True)
    # the existing unfused chain on the same z: eval-mode image decoder, log terms in float64
    with torch.no_grad():
        p = vae.image_decoder(r["z"].reshape(B4 * K4, D4)).double().cpu()
    x = image.double().repeat_interleave(K4, 0)
    lx_unf = (x * p.log() + (1 - x) * torch.log1p(-p)).sum((1, 2, 3)).view(B4, K4)
    unf = float((lx_unf - lx64).abs().max())
    tol = {"x": 2.0 * unf + 1e-6 * float(lx64.abs().max()), "y": _tol(ly32, ly64), "r": _tol(lr32, lr64), "unfused": unf}
    lx_direct, words = _score(vae, r["z"], img)
    return dict(r=r, lx64=lx64, ly64=ly64, lr64=lr64, lp64=lp64, tol=tol, lx_direct=lx_direct, words=words, attrs=attrs)


@pytest.mark.parametrize("post", POSTS)
def test_iw_oracle_parity_given_particles(post):
    c = _parity(post)
    r, tol = c["r"], c["tol"]
    lw = r["log_w"]
    assert lw.shape == (B4, K4, 3) and r["log_p"].shape == (B4, 3)
    tag = "D=%d B=%d K=%d %s" % (D4, B4, K4, post)
    note = "(unfused chain %.3e)" % tol["unfused"]
    _check(tag + " log p(x|z) [log_w]", lw[..., 2] - lw[..., 1], c["lx64"], tol["x"], note)
    _check(tag + " log p(x|z) [scoring call]", c["lx_direct"], c["lx64"], tol["x"], note)
    # log p(y|z) sits in log_w only next to log p(z) - log q(z) (or log p(x|z)), whose fp32 rounding unit exceeds this
    # allowance: it is read from the words the scoring call wrote for the same z, selected by the targets like accumulate does
    sel = c["attrs"].long().to(c["words"].device).view(B4, 1, NA, 1).expand(B4, K4, NA, 1)
    ly = c["words"].double().gather(3, sel).squeeze(3).sum(2)
    _check(tag + " log p(y|z) [scoring call]", ly, c["ly64"], tol["y"])
    cols = (("log p^(x)", tol["x"] + tol["r"]), ("log p^(y)", tol["y"] + tol["r"]), ("log p^(x,y)", tol["x"] + tol["y"] + tol["r"]))
    for i, (nm, t) in enumerate(cols):
        _check("%s %s" % (tag, nm), r["log_p"][:, i], c["lp64"][:, i], t)
        _check("%s log_w column %d" % (tag, i), lw[..., i], (c["lx64"], c["ly64"], c["lx64"] + c["ly64"])[i] + c["lr64"], t)
    ess = r["ess"]
    assert torch.isfinite(ess).all() and (ess >= 1 - 1e-4).all() and (ess <= K4 * (1 + 1e-4)).all(), ess


# ---------------------------------------------------------------------------------------------------------------------
def test_iw_exact_when_decoders_ignore_z():
    from multimodal_vae_amd.evaluate import iw_estimate
    from oracle import mmvae_ref as R
    dev = _dev()
    D, B = 100, 5
    P = R.formula_params("celeba", D)
    P["image_decoder.upsample.0.weight"].zero_()
    P["attrs_decoder.net.0.weight"].zero_()
    vae = _vae(P, D)
    image, attrs = R.formula_inputs("celeba", B)
    image, attrs = image.to(dev), attrs.to(dev)
    mu = torch.zeros(B, D, device=dev)
    for K in (1, 7, 64):
        r = iw_estimate(vae, image, attrs, mu, torch.zeros_like(mu), K, seed=5, return_log_w=True)
        lw = r["log_w"].double().cpu()
        spread = (lw.max(1).values - lw.min(1).values).abs()
        assert (spread <= 1e-6 * lw.abs().max(1).values).all(), (K, spread)
        np.testing.assert_allclose(r["ess"].double().cpu().numpy(), np.full((B, 3), K), rtol=1e-4)
        np.testing.assert_allclose(r["nll"].double().cpu().numpy(), -r["log_p"][:, :2].double().cpu().numpy(), rtol=1e-5)


def test_iw_chunk_and_batch_invariance():
    from multimodal_vae_amd.evaluate import _proposal, iw_estimate
    from oracle import mmvae_ref as R
    dev = _dev()
    B, K = 16, 64
    _, _, vae = _model4()
    tol = _parity("joint")["tol"]                                      # the allowances of test_iw_oracle_parity_given_particles
    image, attrs = R.formula_inputs("celeba", B)
    image, attrs = image.to(dev), attrs.to(dev)
    with torch.no_grad():
        mu, lv = _proposal(vae, image, attrs.long(), "joint")
    one = iw_estimate(vae, image, attrs, mu, lv, K, seed=21, particles_per_call=64, return_z=True, return_log_w=True)
    four = iw_estimate(vae, image, attrs, mu, lv, K, seed=21, particles_per_call=16, return_z=True, return_log_w=True)
    assert torch.equal(one["z"], four["z"])
    d = (one["log_w"].double() - four["log_w"].double()).abs().amax((0, 1)).cpu()
    allowed = (tol["x"] + tol["r"], tol["y"] + tol["r"], tol["x"] + tol["y"] + tol["r"])
    print("log_w, 64 against 16 particles per call: worst difference %s   allowed %s" % (d.tolist(), list(allowed)))
    assert all(float(d[i]) <= allowed[i] for i in range(3)), (d, allowed)
    part = iw_estimate(vae, image[8:], attrs[8:], mu[8:], lv[8:], K, seed=21, first_row=8, return_z=True)
    assert torch.equal(part["z"], one["z"][8:])
    other = iw_estimate(vae, image, attrs, mu, lv, K, seed=22, return_z=True)
    assert not torch.equal(other["z"], one["z"])


def test_attrs_posterior_is_the_text_posterior():
    from multimodal_vae_amd.evaluate import _proposal
    from oracle import mmvae_ref as R
    dev = _dev()
    _, _, vae = _model4()
    image, attrs = R.formula_inputs("celeba", 4)
    with torch.no_grad():
        a = _proposal(vae, image.to(dev), attrs.to(dev), "attrs")
        b = _proposal(vae, image.to(dev), attrs.to(dev).long(), "text")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_marginal_table_has_no_side_effects():
    from multimodal_vae_amd.evaluate import marginal_table
    from oracle import mmvae_ref as R
    _dev()
    _, _, vae = _model4()
    image, attrs = R.formula_inputs("celeba", 21)
    loader = [(image[:13], attrs[:13]), (image[13:], attrs[13:])]                # a partial last batch
    before = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    assert any(k.endswith("num_batches_tracked") for k in before) and any(k.endswith("running_var") for k in before)
    table = marginal_table(vae, loader, n_particles=5, seed=3)
    torch.cuda.synchronize()
    after = vae.state_dict()
    assert set(after) == set(before)
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    assert set(table) == set(POSTS)
    for post in POSTS:
        t = table[post]
        assert t["n"] == 21 and t["log_p"].shape == (21, 3) and t["ess"].shape == (21, 3)
        assert all(np.isfinite(t[k]) for k in ("log_px", "log_py", "log_pxy", "image_nll", "text_nll"))
        assert t["log_px"] < 0 and t["log_py"] < 0 and t["image_nll"] > 0 and t["text_nll"] > 0


def test_loglik_celeba_cli(tmp_path):
    from multimodal_vae_amd.train import save_checkpoint
    from oracle import mmvae_ref as R
    _dev()
    D = 100
    P = R.formula_params("celeba", D)
    save_checkpoint({"state_dict": {k: v.clone() for k, v in P.items()}, "n_latents": D}, False, folder=str(tmp_path))
    out = tmp_path / "bounds.json"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "multimodal_vae_amd.evaluate", "loglik_celeba", str(tmp_path / "checkpoint.pth.tar"), "--all",
           "--synthetic", "32", "--n_samples", "4", "--json", str(out)]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Test Image NLL: " in p.stdout and "\tTest Attrs NLL: " in p.stdout, p.stdout
    res = json.loads(out.read_text())
    assert res["n_samples"] == 4 and res["n_examples"] == 32
    six = [res[post][k] for post in POSTS for k in ("log_px", "log_py")]
    assert len(six) == 6 and all(np.isfinite(v) for v in six)
