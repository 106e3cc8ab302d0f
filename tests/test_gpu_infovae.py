"""GPU tests of the InfoVAE surface (coco/model.py:358-402, coco/train_infovae.py): coco.InfoVAE + coco.infovae_loss against the CPU
oracle's image modules with the MMD term in torch autograd (tests/mmd_ref.py), the checkpoint round trip, training on one batch and
the two command lines.  Gates of the oracle comparison: those of tests/test_gpu_coco.py::test_image_modules_match_oracle for these
modules (bf16 MFMA inputs, BatchNorm over a small batch): outputs abs 2e-2, every parameter gradient 5e-2 of its norm."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mmd_ref as MR  # noqa: E402
from oracle import mmvae_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

D = 20


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _renamed(P):
    """the oracle's image parameters and buffers under InfoVAE's prefixes"""
    out = {}
    for k, v in P.items():
        if k.startswith("image_encoder."):
            out["encoder." + k[len("image_encoder."):]] = v.detach().clone()
        elif k.startswith("image_decoder."):
            out["decoder." + k[len("image_decoder."):]] = v.detach().clone()
    return out


def _oracle_name(k):
    return ("image_encoder." + k[len("encoder."):]) if k.startswith("encoder.") else ("image_decoder." + k[len("decoder."):])


def _batch(B, seed=5):
    """B images in [0, 1] with structure a decoder can learn: one smooth pattern, dimmed per example"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(32.0), torch.arange(32.0), indexing="ij")
    base = torch.stack([0.5 + 0.5 * torch.sin(0.3 * xx + c) * torch.cos(0.2 * yy - c) for c in range(3)])
    level = 0.15 + 0.5 * torch.rand(B, 1, 1, 1, generator=g)
    return (base[None] * level + 0.03 * torch.rand(B, 3, 32, 32, generator=g)).clamp(0, 1).contiguous()


@pytest.mark.parametrize("training", [True, False])
def test_infovae_matches_oracle(training):
    from multimodal_vae_amd import coco as M
    dev = _dev()
    B = 8
    P = R.formula_params("coco", D, requires_grad=True)
    vae = M.InfoVAE(n_latents=D)
    vae.load_state_dict(_renamed(P), strict=True)
    vae = vae.cuda().train(training)
    image, _ = R.formula_inputs("coco", B)
    eps = R.formula_eps(B, D, 0)
    true_samples = R.formula_eps(B, D, 4)
    g = torch.Generator().manual_seed(3)
    masks = ((torch.rand(B, 1024, generator=g) >= 0.1), (torch.rand(B, 256, generator=g) >= 0.1))

    imd = image.to(dev)
    with torch.set_grad_enabled(training):
        recon, z = vae(imd, eps=eps.to(dev), enc_masks=tuple(m.to(dev) for m in masks))
        loss = M.infovae_loss(recon, imd, z, true_samples=true_samples.to(dev))
    assert recon.shape == (B, 3, 32, 32) and z.shape == (B, D) and loss.dim() == 0
    assert recon.is_cuda and z.is_cuda and loss.is_cuda           # no CPU fallback: every output is on the device

    with torch.set_grad_enabled(training):
        o = R.coco_image_encoder(P, image, training, [m.float() for m in masks], drop_p=0.1)
        mu, logvar = o[:, :D], o[:, D:]
        zo = mu + eps * torch.exp(0.5 * logvar) if training else mu
        ro = R.coco_image_decoder(P, zo, training)
        lo = torch.nn.functional.binary_cross_entropy(ro, image) + MR.formulation_mmd(true_samples, zo)
    np.testing.assert_allclose(z.detach().cpu().numpy(), zo.detach().numpy(), atol=2e-2)
    np.testing.assert_allclose(recon.detach().cpu().numpy(), ro.detach().numpy(), atol=2e-2)
    np.testing.assert_allclose(loss.item(), lo.item(), atol=2e-2)
    if not training:
        mu_d, _ = vae.encode(imd)
        assert torch.equal(z, mu_d)                                # eval mode returns the mean
        return
    loss.backward()
    lo.backward()
    for n, p in vae.named_parameters():
        gr, gh = P[_oracle_name(n)].grad, p.grad.cpu()
        slack = 1e-4 if n.startswith("encoder.") else 1e-6         # as test_image_modules_match_oracle
        assert (gh - gr).norm().item() <= 5e-2 * gr.norm().item() + slack, (n, (gh - gr).norm().item(), gr.norm().item())


def test_infovae_loss_draws_its_own_prior_samples():
    from multimodal_vae_amd import coco as M
    dev = _dev()
    torch.manual_seed(0)
    vae = M.InfoVAE(n_latents=D).cuda().train()
    img = _batch(16).to(dev)
    recon, z = vae(img)
    torch.manual_seed(11)
    a = M.infovae_loss(recon, img, z)
    torch.manual_seed(11)
    b = M.infovae_loss(recon, img, z)
    c = M.infovae_loss(recon, img, z)
    # the same seed draws the same prior samples (the BCE sum uses float atomics: the last bits of the loss are not reproducible)
    assert a.is_cuda and bool(torch.isfinite(a)) and abs(a.item() - b.item()) < 2e-6 and abs(a.item() - c.item()) > 2e-5
    bce = torch.nn.functional.binary_cross_entropy(recon.detach(), img)
    assert -1e-6 <= a.item() - bce.item() <= 2.0                   # + an MMD term, which lies in [0, 2]
    assert float(M.compute_kernel(z.detach(), z.detach()).diagonal().min()) == 1.0


def test_checkpoint_round_trip(tmp_path):
    from multimodal_vae_amd import coco as M, train_infovae as T
    from multimodal_vae_amd.train import save_checkpoint
    dev = _dev()
    torch.manual_seed(1)
    vae = M.InfoVAE(n_latents=D).cuda()
    opt = torch.optim.Adam(vae.parameters(), lr=1e-3)
    img = _batch(8).to(dev)
    vae.train()
    recon, z = vae(img)
    M.infovae_loss(recon, img, z).backward()
    opt.step()                                                     # moved parameters, BatchNorm statistics of one batch
    save_checkpoint({'state_dict': vae.state_dict(), 'best_loss': 1.0, 'n_latents': D, 'optimizer': opt.state_dict()}, True,
                    folder=str(tmp_path))
    back = T.load_checkpoint(os.path.join(str(tmp_path), 'model_best.pth.tar'), use_cuda=True)
    assert isinstance(back, M.InfoVAE) and back.n_latents == D
    sd, sb = vae.state_dict(), back.state_dict()
    assert list(sd) == list(sb) and all(torch.equal(sd[k].cpu(), sb[k].cpu()) for k in sd)
    assert int(sd["encoder.features.3.num_batches_tracked"]) == 1
    vae.eval(); back.eval()
    with torch.no_grad():
        r1, z1 = vae(img)
        r2, z2 = back(img)
    assert torch.equal(z1, z2) and torch.equal(r1, r2)


def test_training_reduces_the_loss():
    from multimodal_vae_amd import coco as M
    dev = _dev()
    torch.manual_seed(0)
    vae = M.InfoVAE(n_latents=D).cuda().train()
    opt = torch.optim.Adam(vae.parameters(), lr=1e-3)
    img = _batch(32).to(dev)
    losses = []
    for _ in range(31):                                            # the first loss, then 30 Adam steps
        opt.zero_grad()
        recon, z = vae(img)
        loss = M.infovae_loss(recon, img, z)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu().tolist()
    first, last = losses[0], losses[-1]
    assert np.isfinite(last) and last < 0.95 * first, (first, last)


def test_command_lines(tmp_path, capsys):
    from multimodal_vae_amd import evaluate as E, train_infovae as T
    _dev()
    out, results = str(tmp_path / "models"), str(tmp_path / "results")
    hist = T.main(["--synthetic", "256", "--epochs", "2", "--batch_size", "32", "--n_latents", "20", "--cuda", "--out", out,
                   "--results", results, "--log_interval", "4", "--seed", "3"])
    printed = capsys.readouterr().out
    assert "Train Epoch: 1 [0/256 (0%)]\tLoss: " in printed and "====> Epoch: 2 Average loss: " in printed
    assert "====> Test set loss: " in printed
    assert len(hist["train"]) == 2 and len(hist["test"]) == 2 and all(np.isfinite(v) for v in hist["train"] + hist["test"])
    ckpt = os.path.join(out, "infovae", "checkpoint.pth.tar")
    assert hist["checkpoint"] == ckpt and os.path.exists(os.path.join(out, "infovae", "model_best.pth.tar"))
    state = torch.load(ckpt, weights_only=False)
    assert sorted(state) == ["best_loss", "n_latents", "optimizer", "state_dict"] and state["n_latents"] == 20
    assert state["best_loss"] == min(hist["test"])
    vae = T.load_checkpoint(ckpt, use_cuda=True)
    assert next(vae.parameters()).is_cuda
    assert tuple(torch.load(os.path.join(results, "sample_epoch2.pt")).shape) == (64, 3, 32, 32)

    jf = str(tmp_path / "mmd.json")
    r = E._main(["latent_mmd", ckpt, "--synthetic", "512", "--json", jf])
    printed = capsys.readouterr().out
    assert "Latent MMD over 512 examples" in printed
    terms = [r["k_prior"], r["k_posterior"], r["k_cross"], r["mmd"]]
    assert r["n"] == 512 and all(np.isfinite(t) for t in terms) and all(0.0 < t <= 1.0 for t in terms[:3])
    assert abs(terms[3] - (terms[0] + terms[1] - 2 * terms[2])) < 1e-5
    with open(jf) as fp:
        assert json.load(fp) == r


def test_no_cpu_fallback():
    from multimodal_vae_amd import coco as M, MMVAEError
    vae = M.InfoVAE(n_latents=D)
    with pytest.raises(MMVAEError):
        vae(torch.zeros(2, 3, 32, 32))
    with pytest.raises(MMVAEError):
        M.compute_mmd(torch.zeros(2, D), torch.zeros(2, D))
