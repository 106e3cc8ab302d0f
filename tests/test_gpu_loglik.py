"""Importance-sampled marginal log-likelihood (evaluate.iw_estimate / log_marginal / marginal_table, the loglik CLI)
against the float64 oracle and against what an importance-sampling estimate must satisfy."""
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
D = 100


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _vae(P, dev, n_latents=D):
    from multimodal_vae_amd import multimnist as M
    vae = M.MultimodalVAE(n_latents, use_cuda=True)
    vae.load_state_dict({k: v.clone() for k, v in P.items()}, strict=True)
    vae.cuda()
    vae.eval()
    return vae


def _f64(P):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}


def _oracle_ll(P64, z, image, text):
    """float64 log p(x|z), log p(y|z) per row of z (rows of image / text given per row) and the near-tie flag of the
    text decoder's greedy pass (two largest log-probabilities within 1e-2 at some step)."""
    from oracle import mmvae_ref as R
    with torch.no_grad():
        l = R.multimnist_image_decoder_logits(P64, z, False).reshape(z.shape[0], -1)
        lx = (image.reshape(z.shape[0], -1).double() * l - F.softplus(l)).sum(1)
        words, _ = R.multimnist_text_decoder(P64, z, False)
        ly = words.gather(2, text.unsqueeze(2)).squeeze(2).sum(1)
        top = words.topk(2, dim=2).values
        tie = ((top[..., 0] - top[..., 1]) < 1e-2).any(1)
    return lx, ly, tie


def _zero_z_paths(P):
    """Both decoders independent of z."""
    Q = {k: v.clone() for k, v in P.items()}
    Q["image_decoder.upsample.0.weight"].zero_()
    Q["text_decoder.z2h.weight"].zero_()
    Q["text_decoder.gru.weight_ih_l0"][:, 100:] = 0
    Q["text_decoder.h2o.weight"][:, 100:] = 0
    return Q


@pytest.mark.parametrize("D", [100, 20, 127])
def test_iw_oracle_parity_given_particles(D):
    """D = 100 scores the text through the weights-resident decoder kernel (csrc/text.hip: 97 <= D <= 100), 20 and 127 through
    the streamed one (kz = 32 / kx = 128 both padded; kz = 128 / kx = 256, the upper limit of mmvae_mm_create)."""
    from multimodal_vae_amd.evaluate import iw_estimate
    from oracle import mmvae_ref as R
    dev = _dev()
    B, K = 13, 8
    P = R.formula_params("multimnist", D)
    # The formula initialisation's text decoder is untrained and nearly uniform: 10 of 13 rows hold a near-tie among their
    # 32 greedy decisions.  A FILL bias of +4 makes the decisions decisive; the z-dependent part of the logits is unchanged.
    P["text_decoder.h2o.bias"][11] += 4.0
    P64 = _f64(P)
    vae = _vae(P, dev, D)
    image, text = R.formula_inputs("multimnist", B)
    g = torch.Generator().manual_seed(3)
    eps = torch.randn(B, K, D, generator=g, dtype=torch.float64)
    for post in ("joint", "image", "text"):
        with torch.no_grad():
            _, _, mu, lv, _ = R.multimnist_forward(P64, image.double() if post != "text" else None,
                                                    text if post != "image" else None, False)
        z = mu.unsqueeze(1) + lv.mul(0.5).exp().unsqueeze(1) * eps                      # (B, K, D) float64
        lx, ly, tie = _oracle_ll(P64, z.reshape(B * K, D), image.repeat_interleave(K, 0), text.repeat_interleave(K, 0))
        lr = (-0.5 * z.pow(2) + 0.5 * eps.pow(2) + 0.5 * lv.unsqueeze(1)).sum(2)      # log p(z) - log q(z)
        lx, ly = lx.view(B, K), ly.view(B, K)
        want = torch.stack([torch.logsumexp(lx + lr, 1), torch.logsumexp(ly + lr, 1), torch.logsumexp(lx + ly + lr, 1)], 1)
        want = want - np.log(K)
        r = iw_estimate(vae, image.to(dev), text.to(dev), mu.float().to(dev), lv.float().to(dev), K, eps=eps.float().to(dev),
                        return_log_w=True)
        lw = r["log_w"].double().cpu()
        got_lx = lw[..., 2] - lw[..., 1]
        np.testing.assert_allclose(got_lx.numpy(), lx.numpy(), rtol=1e-2, err_msg=post)
        got = r["log_p"].double().cpu()
        np.testing.assert_allclose(got[:, 0].numpy(), want[:, 0].numpy(), rtol=1e-2, err_msg=post)
        # With the +4 bias the oracle's smallest top-two gap is at least 1.4 nats at every D used here, for all three
        # posteriors: no row is a near-tie, so no row is excused at the new sizes (D = 100 keeps its earlier allowance of 2).
        excl = tie.view(B, K).any(1)
        assert int(excl.sum()) <= (2 if D == 100 else 0), (post, D, int(excl.sum()))
        keep = ~excl
        np.testing.assert_allclose(got[keep, 1:].numpy(), want[keep, 1:].numpy(), rtol=1e-2, err_msg=post)
        assert torch.isfinite(r["ess"]).all() and (r["ess"] >= 1 - 1e-4).all() and (r["ess"] <= K * (1 + 1e-4)).all()


def _const_model():
    from oracle import mmvae_ref as R
    P = _zero_z_paths(R.formula_params("multimnist", D))
    return P, _vae(P, _dev())


def test_iw_exact_when_decoders_ignore_z():
    from multimodal_vae_amd.evaluate import iw_estimate
    from oracle import mmvae_ref as R
    dev = _dev()
    P, vae = _const_model()
    B = 5
    image, text = R.formula_inputs("multimnist", B)
    lx, ly, _ = _oracle_ll(_f64(P), torch.zeros(B, D, dtype=torch.float64), image, text)
    mu = torch.zeros(B, D, device=dev)
    for K in (1, 7, 64):
        r = iw_estimate(vae, image.to(dev), text.to(dev), mu, torch.zeros_like(mu), K, seed=5, return_log_w=True)
        lw = r["log_w"].double().cpu()
        spread = (lw.max(1).values - lw.min(1).values).abs()
        assert (spread <= 1e-6 * lw.abs().max(1).values + 1e-6).all(), (K, spread)
        lp = r["log_p"].double().cpu()
        np.testing.assert_allclose(lp.numpy(), lw[:, 0].numpy(), rtol=1e-5)
        np.testing.assert_allclose(r["ess"].double().cpu().numpy(), np.full((B, 3), K), rtol=1e-4)
        np.testing.assert_allclose(lp[:, 0].numpy(), lx.numpy(), rtol=1e-2)
        np.testing.assert_allclose(lp[:, 1].numpy(), ly.numpy(), rtol=1e-2)
        np.testing.assert_allclose(lp[:, 2].numpy(), (lx + ly).numpy(), rtol=1e-2)
        np.testing.assert_allclose(r["nll"].double().cpu().numpy(), -lp[:, :2].numpy(), rtol=1e-5)


def test_iw_unbiased_with_wide_proposal():
    from multimodal_vae_amd.evaluate import iw_estimate
    from oracle import mmvae_ref as R
    dev = _dev()
    P, vae = _const_model()
    B = 256
    image, text = R.formula_inputs("multimnist", B)
    image, text = image.to(dev), text.to(dev)
    mu = torch.zeros(B, D, device=dev)
    exact = iw_estimate(vae, image, text, mu, torch.zeros_like(mu), 1)["log_p"].double()       # p(x|z) = p(x): log p
    lv = torch.full_like(mu, 0.1)
    means = {}
    for K in (1, 64):
        lp = iw_estimate(vae, image, text, mu, lv, K, seed=9)["log_p"].double()
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
    P = R.formula_params("multimnist", D)
    vae = _vae(P, dev)
    B, K = 16, 64
    image, text = R.formula_inputs("multimnist", B)
    image, text = image.to(dev), text.to(dev)
    with torch.no_grad():
        _, _, mu, lv, _ = R.multimnist_forward(P, image.cpu(), text.cpu(), False)
    mu, lv = mu.to(dev), lv.to(dev)
    one = iw_estimate(vae, image, text, mu, lv, K, seed=21, particles_per_call=64, return_z=True)
    four = iw_estimate(vae, image, text, mu, lv, K, seed=21, particles_per_call=16, return_z=True)
    assert torch.equal(one["z"], four["z"])
    np.testing.assert_allclose(four["log_p"].cpu().numpy(), one["log_p"].cpu().numpy(), rtol=1e-5)
    part = iw_estimate(vae, image[8:], text[8:], mu[8:], lv[8:], K, seed=21, first_row=8, return_z=True)
    assert torch.equal(part["z"], one["z"][8:])
    other = iw_estimate(vae, image, text, mu, lv, K, seed=22, return_z=True)
    assert not torch.equal(other["z"], one["z"])


def test_iw_device_rng_is_standard_normal():
    from multimodal_vae_amd.evaluate import iw_estimate
    from oracle import mmvae_ref as R
    dev = _dev()
    vae = _vae(R.formula_params("multimnist", D), dev)
    B, K = 16, 256
    image, text = R.formula_inputs("multimnist", B)
    g = torch.Generator().manual_seed(1)
    mu = (torch.rand(B, D, generator=g) - 0.5).to(dev)
    lv = (torch.rand(B, D, generator=g) - 0.5).to(dev)
    r = iw_estimate(vae, image.to(dev), text.to(dev), mu, lv, K, seed=77, return_z=True)
    e = ((r["z"] - mu.unsqueeze(1)) / lv.mul(0.5).exp().unsqueeze(1)).double().reshape(-1)
    n = e.numel()
    assert n == 16 * 256 * 100
    m, v = e.mean().item(), e.var().item()
    assert abs(m) <= 4 / np.sqrt(n), m
    assert abs(v - 1.0) <= 4 * np.sqrt(2.0 / n), v


def test_marginal_table_has_no_side_effects():
    from multimodal_vae_amd.evaluate import marginal_table
    from oracle import mmvae_ref as R
    dev = _dev()
    vae = _vae(R.formula_params("multimnist", D), dev)
    image, text = R.formula_inputs("multimnist", 21)
    loader = [(image[:13], text[:13]), (image[13:], text[13:])]                  # a partial last batch
    before = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    table = marginal_table(vae, loader, n_particles=5, seed=3)
    torch.cuda.synchronize()
    after = vae.state_dict()
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    for post in ("joint", "image", "text"):
        t = table[post]
        assert t["n"] == 21 and t["log_p"].shape == (21, 3) and t["ess"].shape == (21, 3)
        assert all(np.isfinite(t[k]) for k in ("log_px", "log_py", "log_pxy", "image_nll", "text_nll"))
        assert t["log_px"] < 0 and t["image_nll"] > 0


def test_loglik_cli_on_a_checkpoint(tmp_path):
    from multimodal_vae_amd.train import save_checkpoint
    from oracle import mmvae_ref as R
    _dev()
    P = R.formula_params("multimnist", D)
    save_checkpoint({"state_dict": {k: v.clone() for k, v in P.items()}, "n_latents": D}, False, folder=str(tmp_path))
    out = tmp_path / "bounds.json"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "multimodal_vae_amd.evaluate", "loglik", str(tmp_path / "checkpoint.pth.tar"), "--all",
           "--synthetic", "64", "--n_samples", "8", "--json", str(out)]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Test Image NLL: " in p.stdout and "\tTest Text NLL: " in p.stdout, p.stdout
    res = json.loads(out.read_text())
    assert res["n_samples"] == 8 and res["n_examples"] == 64
    six = [res[post][k] for post in ("joint", "image", "text") for k in ("log_px", "log_py")]
    assert len(six) == 6 and all(np.isfinite(v) for v in six)
