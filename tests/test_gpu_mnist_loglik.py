"""Importance-sampled log p(x), log p(y) of the MNIST model (evaluate.iw_estimate / log_marginal / marginal_table on the fused
fp32 scorer mmvae_mnist_iw_score, compute_nll_mnist / test_mnist, the loglik command line with --dataset mnist) against the
float64 oracle.

Tolerance rule (``_tol``): the test evaluates the same formulas twice on the CPU, in float64 (the reference value) and in
torch's own float32, and allows the GPU 16 x the float32 evaluation's worst absolute error per quantity: the kernel sums the 784
pixel terms and the MFMA k-chunks in another order and uses the hardware exp / log where torch uses libm.  Every row is
compared: the MNIST text decoder has no greedy feedback, so there are no ties to leave out."""
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


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _vae(P, D, precision="fp32"):
    from multimodal_vae_amd import mnist as M
    vae = M.MultimodalVAE(D, precision=precision)
    vae.load_state_dict({k: v.clone() for k, v in P.items()}, strict=True)
    vae.cuda()
    vae.eval()
    return vae


def _cast(P, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in P.items()}


def _ll(P, z, image, label):
    """log p(x|z), log p(y|z) per row of z in the dtype of P / z (image, label given per row)."""
    from oracle import mmvae_ref as R
    with torch.no_grad():
        l = R._mlp_bn_relu(P, z, "image_decoder.", (0, 3, 6), False)
        lx = (image.to(z.dtype) * l - F.softplus(l)).sum(1)
        words = F.log_softmax(R._mlp_bn_relu(P, z, "text_decoder.", (0, 3), False), dim=1)
        ly = words.gather(1, label.unsqueeze(1)).squeeze(1)
    return lx, ly


def _estimate(P, mu, lv, eps, image, label):
    """The estimator restated on the CPU in the dtype of its inputs: -> (log p(x|z) (B,K), log p(y|z) (B,K), log p^ (B,3))."""
    B, K, D = eps.shape
    z = mu.unsqueeze(1) + lv.mul(0.5).exp().unsqueeze(1) * eps
    lx, ly = _ll(P, z.reshape(B * K, D), image.repeat_interleave(K, 0), label.repeat_interleave(K, 0))
    lr = (-0.5 * z.pow(2) + 0.5 * eps.pow(2) + 0.5 * lv.unsqueeze(1)).sum(2)          # log p(z) - log q(z)
    lx, ly = lx.view(B, K), ly.view(B, K)
    lp = torch.stack([torch.logsumexp(lx + lr, 1), torch.logsumexp(ly + lr, 1), torch.logsumexp(lx + ly + lr, 1)], 1) - np.log(K)
    return lx, ly, lp


def _tol(v32, v64):
    return 16.0 * float((v32.double() - v64).abs().max())


def _check(name, got, want, tol):
    err = float((got.double().cpu() - want).abs().max())
    print("%-40s  GPU worst error %.3e   allowed %.3e (err32 %.3e)" % (name, err, tol, tol / 16.0))
    assert err <= tol, (name, err, tol)


def _proposal64(P64, image, label, post):
    from oracle import mmvae_ref as R
    with torch.no_grad():
        _, _, mu, lv = R.mnist_forward(P64, image.double() if post != "text" else None, label if post != "image" else None, False)
    return mu, lv


def _parity(P, D, B, K, posts, tag, seed=3):
    """iw_estimate with injected particles against the float64 restatement, all of ``posts``."""
    from multimodal_vae_amd.evaluate import iw_estimate
    from oracle import mmvae_ref as R
    dev = _dev()
    P64 = _cast(P, torch.float64)
    vae = _vae(P, D)
    image, label = R.formula_inputs("mnist", B)
    eps = torch.randn(B, K, D, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    for post in posts:
        mu, lv = _proposal64(P64, image, label, post)
        lx64, ly64, lp64 = _estimate(P64, mu, lv, eps, image, label)
        lx32, ly32, lp32 = _estimate(P, mu.float(), lv.float(), eps.float(), image, label)
        r = iw_estimate(vae, image.to(dev), label.to(dev), mu.float().to(dev), lv.float().to(dev), K, eps=eps.float().to(dev),
                        return_log_w=True)
        lw = r["log_w"]
        assert lw.shape == (B, K, 3) and r["log_p"].shape == (B, 3)
        _check("%s %s log p(x|z)" % (tag, post), lw[..., 2] - lw[..., 1], lx64, _tol(lx32, lx64))
        for c, nm in enumerate(("log p^(x)", "log p^(y)", "log p^(x,y)")):
            _check("%s %s %s" % (tag, post, nm), r["log_p"][:, c], lp64[:, c], _tol(lp32[:, c], lp64[:, c]))
        ess = r["ess"]
        assert torch.isfinite(ess).all() and (ess >= 1 - 1e-4).all() and (ess <= K * (1 + 1e-4)).all(), ess


@pytest.mark.parametrize("D", [20, 64])
def test_iw_oracle_parity_given_particles(D):
    from oracle import mmvae_ref as R
    _parity(R.formula_params("mnist", D), D, 13, 8, POSTS, "D=%d B=13 K=8" % D)


def test_iw_uses_the_running_statistics():
    """The formula model's BatchNorm buffers are (0, 1): the same parity with running means / variances that matter."""
    from oracle import mmvae_ref as R
    D = 20
    P = R.formula_params("mnist", D)
    for k in list(P):
        if k.endswith("running_mean"):
            P[k] = 0.3 * torch.sin(0.7 * torch.arange(P[k].numel(), dtype=torch.float32))
        elif k.endswith("running_var"):
            P[k] = 1.0 + 0.5 * torch.cos(0.3 * torch.arange(P[k].numel(), dtype=torch.float32))
    _parity(P, D, 13, 8, ("joint",), "running stats")


def test_iw_same_result_from_fp32_and_bf16_plans():
    from multimodal_vae_amd.evaluate import iw_estimate
    from oracle import mmvae_ref as R
    dev = _dev()
    D, B, K = 20, 13, 8
    P = R.formula_params("mnist", D)
    image, label = R.formula_inputs("mnist", B)
    mu, lv = _proposal64(_cast(P, torch.float64), image, label, "joint")
    eps = torch.randn(B, K, D, generator=torch.Generator().manual_seed(3))
    out = []
    for precision in ("fp32", "bf16"):
        vae = _vae(P, D, precision)
        assert vae.precision == precision
        out.append(iw_estimate(vae, image.to(dev), label.to(dev), mu.float().to(dev), lv.float().to(dev), K, eps=eps.to(dev)))
    assert torch.equal(out[0]["log_p"], out[1]["log_p"])             # the scorer reads the fp32 masters


def _const_model(D=20):
    """Both decoders independent of z."""
    from oracle import mmvae_ref as R
    P = R.formula_params("mnist", D)
    P["image_decoder.net.0.weight"].zero_()
    P["text_decoder.net.0.weight"].zero_()
    return P, _vae(P, D)


def test_iw_exact_when_decoders_ignore_z():
    from multimodal_vae_amd.evaluate import iw_estimate
    from oracle import mmvae_ref as R
    dev = _dev()
    D, B = 20, 5
    P, vae = _const_model(D)
    image, label = R.formula_inputs("mnist", B)
    z0 = torch.zeros(B, D)
    lx64, ly64 = _ll(_cast(P, torch.float64), z0.double(), image, label)
    lx32, ly32 = _ll(P, z0, image, label)
    want = torch.stack([lx64, ly64, lx64 + ly64], 1)
    have32 = torch.stack([lx32, ly32, lx32 + ly32], 1)
    mu = torch.zeros(B, D, device=dev)
    for K in (1, 7, 64):
        r = iw_estimate(vae, image.to(dev), label.to(dev), mu, torch.zeros_like(mu), K, seed=5, return_log_w=True)
        lw = r["log_w"].double().cpu()
        spread = (lw.max(1).values - lw.min(1).values).abs()
        assert (spread <= 1e-6 * lw.abs().max(1).values).all(), (K, spread)
        np.testing.assert_allclose(r["ess"].double().cpu().numpy(), np.full((B, 3), K), rtol=1e-4)
        for c, nm in enumerate(("log p(x)", "log p(y)", "log p(x) + log p(y)")):
            _check("const K=%d %s" % (K, nm), r["log_p"][:, c], want[:, c], _tol(have32[:, c], want[:, c]))
        np.testing.assert_allclose(r["nll"].double().cpu().numpy(), -r["log_p"][:, :2].double().cpu().numpy(), rtol=1e-5)


def test_iw_unbiased_with_wide_proposal():
    from multimodal_vae_amd.evaluate import iw_estimate
    from oracle import mmvae_ref as R
    dev = _dev()
    D, B = 20, 256
    P, vae = _const_model(D)
    image, label = R.formula_inputs("mnist", B)
    image, label = image.to(dev), label.to(dev)
    mu = torch.zeros(B, D, device=dev)
    exact = iw_estimate(vae, image, label, mu, torch.zeros_like(mu), 1)["log_p"].double()        # p(x|z) = p(x): log p
    lv = torch.full_like(mu, 0.1)
    means = {}
    for K in (1, 64):
        lp = iw_estimate(vae, image, label, mu, lv, K, seed=9)["log_p"].double()
        means[K] = lp.mean(0).cpu()
        if K == 64:
            ratio = (lp - exact).exp().cpu()                  # p^ / p per row
            for c in range(3):
                m, se = ratio[:, c].mean().item(), ratio[:, c].std().item() / np.sqrt(B)
                assert abs(m - 1.0) <= 4 * se, (c, m, se)
    assert (means[64] >= means[1]).all(), means


def test_iw_chunk_and_batch_invariance():
    from multimodal_vae_amd.evaluate import iw_estimate
    from oracle import mmvae_ref as R
    dev = _dev()
    D, B, K = 20, 16, 64
    P = R.formula_params("mnist", D)
    vae = _vae(P, D)
    image, label = R.formula_inputs("mnist", B)
    mu, lv = _proposal64(_cast(P, torch.float64), image, label, "joint")
    image, label, mu, lv = image.to(dev), label.to(dev), mu.float().to(dev), lv.float().to(dev)
    one = iw_estimate(vae, image, label, mu, lv, K, seed=21, particles_per_call=64, return_z=True)
    four = iw_estimate(vae, image, label, mu, lv, K, seed=21, particles_per_call=16, return_z=True)
    assert torch.equal(one["z"], four["z"])
    np.testing.assert_allclose(four["log_p"].cpu().numpy(), one["log_p"].cpu().numpy(), rtol=1e-5)
    part = iw_estimate(vae, image[8:], label[8:], mu[8:], lv[8:], K, seed=21, first_row=8, return_z=True)
    assert torch.equal(part["z"], one["z"][8:])
    other = iw_estimate(vae, image, label, mu, lv, K, seed=22, return_z=True)
    assert not torch.equal(other["z"], one["z"])
    # (B, 1, 28, 28) images are the same examples
    img4 = iw_estimate(vae, image.view(B, 1, 28, 28), label, mu, lv, K, seed=21, particles_per_call=64)
    assert torch.equal(img4["log_p"], one["log_p"])


@pytest.mark.parametrize("B,K", [(1, 1), (3, 5), (5, 37), (64, 64)])
def test_iw_tile_edges(B, K):
    """Row counts that are no multiple of the kernel's row tile, one example, one particle."""
    from oracle import mmvae_ref as R
    _parity(R.formula_params("mnist", 20), 20, B, K, ("joint",), "B=%d K=%d" % (B, K), seed=4)


@pytest.mark.parametrize("D", [4, 124])
def test_iw_smallest_and_largest_latent_size(D):
    """n_latents below one 16-deep MFMA step and at the plan's upper limit (no multiple of 16 either)."""
    from oracle import mmvae_ref as R
    _parity(R.formula_params("mnist", D), D, 3, 5, ("joint",), "D=%d B=3 K=5" % D, seed=4)


def test_marginal_table_has_no_side_effects():
    from multimodal_vae_amd.evaluate import marginal_table
    from oracle import mmvae_ref as R
    _dev()
    D = 20
    vae = _vae(R.formula_params("mnist", D), D)
    image, label = R.formula_inputs("mnist", 21)
    loader = [(image[:13], label[:13]), (image[13:], label[13:])]                # a partial last batch
    before = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    assert any(k.endswith("num_batches_tracked") for k in before) and any(k.endswith("running_var") for k in before)
    table = marginal_table(vae, loader, n_particles=5, seed=3)
    torch.cuda.synchronize()
    after = vae.state_dict()
    assert set(after) == set(before)
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    for post in POSTS:
        t = table[post]
        assert t["n"] == 21 and t["log_p"].shape == (21, 3) and t["ess"].shape == (21, 3)
        assert all(np.isfinite(t[k]) for k in ("log_px", "log_py", "log_pxy", "image_nll", "text_nll"))
        assert t["log_px"] < 0 and t["log_py"] < 0 and t["image_nll"] > 0 and t["text_nll"] > 0


@pytest.mark.parametrize("D", [20, 64])
def test_consumers_against_the_oracle(D):
    from multimodal_vae_amd.evaluate import compute_nll_mnist, test_mnist
    from oracle import mmvae_ref as R
    dev = _dev()
    N, Bb, K = 32, 16, 3
    P = R.formula_params("mnist", D)
    P64 = _cast(P, torch.float64)
    vae = _vae(P, D)
    image, label = R.formula_inputs("mnist", N)
    loader = [(image[i:i + Bb], label[i:i + Bb]) for i in range(0, N, Bb)]

    def restate(Pd, dtype, kw):
        """mnist/loglikelihood.py:15-65 on the CPU: -> per (example, particle) NLL terms (N*K,) image and label."""
        ti, tt = [], []
        with torch.no_grad():
            for im, lb in loader:
                _, _, mu, lv = R.mnist_forward(Pd, im.to(dtype) if kw != "text" else None, lb if kw != "image" else None, False)
                sample = torch.randn(K, D).to(dtype)
                z = sample.unsqueeze(0) * lv.mul(0.5).exp().unsqueeze(1) + mu.unsqueeze(1)
                for i in range(K):
                    p = torch.sigmoid(R._mlp_bn_relu(Pd, z[:, i], "image_decoder.", (0, 3, 6), False))
                    w = F.log_softmax(R._mlp_bn_relu(Pd, z[:, i], "text_decoder.", (0, 3), False), dim=1)
                    ti.append(F.binary_cross_entropy(p, im.to(dtype), reduction="none").sum(1))
                    tt.append(F.nll_loss(w, lb, reduction="none"))
        return torch.cat(ti), torch.cat(tt)

    for kw in POSTS:
        torch.manual_seed(11)
        i64, t64 = restate(P64, torch.float64, kw)
        torch.manual_seed(11)
        i32, t32 = restate(P, torch.float32, kw)
        torch.manual_seed(11)
        got_i, got_t = compute_nll_mnist(vae, loader, image_only=kw == "image", text_only=kw == "text", n_samples=K, use_cuda=True)
        # the result is the sum of the N*K terms over K*N: the allowed error of a term, times the terms summed, over K*N
        n_terms = N * K
        for nm, got, w64, w32 in (("image", got_i, i64, i32), ("label", got_t, t64, t32)):
            want = float(w64.sum() / (K * N))
            tol = _tol(w32, w64) * n_terms / (K * N)
            print("D=%d compute_nll_mnist [%s] %s NLL  GPU %.6f  oracle %.6f  error %.3e  allowed %.3e" %
                  (D, kw, nm, got, want, abs(got - want), tol))
            assert abs(got - want) <= tol, (kw, nm, got, want, tol)

    with torch.no_grad():
        _, words64, _, _ = R.mnist_forward(P64, image.double(), None, False)
    top = words64.topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) > 1e-3            # the oracle's own decisions are decisive (0.043 measured)
    pred64 = words64.argmax(1)
    with torch.no_grad():
        _, recon_text, _, _ = vae(image=image.to(dev))
    assert torch.equal(recon_text.argmax(1).cpu(), pred64)            # all 32, no example excused
    acc = test_mnist(vae, loader, use_cuda=True, verbose=False)
    assert acc == float((pred64 == label).sum()) / N


def _cli(tmp_path, extra):
    from multimodal_vae_amd.train import save_checkpoint
    from oracle import mmvae_ref as R
    _dev()
    fam = "mnist" if "mnist" in extra else "multimnist"
    D = 20 if fam == "mnist" else 100
    P = R.formula_params(fam, D)
    save_checkpoint({"state_dict": {k: v.clone() for k, v in P.items()}, "n_latents": D}, False, folder=str(tmp_path))
    out = tmp_path / "bounds.json"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "multimodal_vae_amd.evaluate", "loglik", str(tmp_path / "checkpoint.pth.tar"), "--all",
           "--synthetic", "64", "--n_samples", "8", "--json", str(out)] + extra
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Test Image NLL: " in p.stdout and "\tTest Text NLL: " in p.stdout, p.stdout
    res = json.loads(out.read_text())
    assert res["n_samples"] == 8 and res["n_examples"] == 64
    six = [res[post][k] for post in POSTS for k in ("log_px", "log_py")]
    assert len(six) == 6 and all(np.isfinite(v) for v in six)
    return res


def test_loglik_cli_on_an_mnist_checkpoint(tmp_path):
    _cli(tmp_path, ["--dataset", "mnist"])


def test_loglik_cli_explicit_multimnist_is_the_default(tmp_path):
    a = _cli(tmp_path / "a", ["--dataset", "multimnist"])
    b = _cli(tmp_path / "b", [])
    assert a.keys() == b.keys()
    for post in POSTS:
        for k, v in a[post].items():
            np.testing.assert_allclose(v, b[post][k], rtol=1e-5, err_msg="%s %s" % (post, k))
