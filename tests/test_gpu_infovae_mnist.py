"""GPU tests of ``mnist.InfoVAE`` under ``set_infovae_backend(vae, "hip")``: the whole model against pure float64 and a short
training run.

Whole model, formula weights (tests/golden/mnist_infovae_reference.npz records what the reference's own class computes from them):
E_hip = max |hip backend - float64 model|, E_emu = max |float64 model with bf16-rounded convolution operands - float64 model|
(``conv4s2_ref.infovae_forward(..., emulate=True)``); required is E_hip <= 2 E_emu + 8 x 2^-23 max |float64 model| for recon, z and
the gradient of the loss with respect to each of the four convolution weights and to ``encoder_fc.0.weight``.  The factor 2 is the
one tests/test_gpu_pixelcnn_train.py holds whole models to (rounding boundaries flip between two correct realisations); the second
term is the fp32 floor of the op-level gate, for the tensors the convolutions hardly reach (z is dominated by the biases of the
linear layers under these weights).

Training: 20 ``train_step``s at B = 32 on synthetic data under the hip backend; the step-0 loss against the torch backend's from
equal weights and equal ``true_samples``, under the same bound with E_emu the loss's own emulation error.

`pytest -s` prints the figures; MEASURED ones are in profiles/infovae_mnist_bench.txt.
"""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv4s2_ref as C  # noqa: E402

pytestmark = pytest.mark.gpu

GRADS = ("encoder_conv.0.weight", "encoder_conv.2.weight", "decoder_conv.0.weight", "decoder_conv.2.weight", "encoder_fc.0.weight")
FLOOR = 8 * 2.0 ** -23


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _formula_model():
    import multimodal_vae_amd.mnist as M
    vae = M.InfoVAE(n_latents=20)
    sd = vae.state_dict()
    vae.load_state_dict({k: v.float() for k, v in C.formula_state_dict(list(sd), [tuple(v.shape) for v in sd.values()]).items()})
    return vae


def _mmd64(x, y):
    def k(a, b):
        return torch.exp(-(a.unsqueeze(1) - b.unsqueeze(0)).pow(2).mean(dim=2) / a.shape[1])
    return k(x, x).mean() + k(y, y).mean() - 2 * k(x, y).mean()


def _loss_and_grads(sd32, x, true_samples, emulate):
    """float64 model on the float32 weights -> recon, z, loss, {name: gradient}"""
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in sd32.items()}
    recon, z = C.infovae_forward(leaves, x.double(), emulate)
    loss = torch.nn.functional.mse_loss(recon, x.double()) + _mmd64(true_samples.double(), z)
    grads = torch.autograd.grad(loss, [leaves[k] for k in GRADS])
    return recon.detach(), z.detach(), float(loss.detach()), dict(zip(GRADS, grads))


@pytest.mark.parametrize("B", [4, 9])
def test_whole_model(B):
    import multimodal_vae_amd.mnist as M
    dev = _dev()
    vae = _formula_model()
    sd = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    x = C.formula_input(B).float()
    ts = torch.randn(B, 20, generator=torch.Generator().manual_seed(5))
    r64, z64, l64, g64 = _loss_and_grads(sd, x, ts, False)
    rem, zem, lem, gem = _loss_and_grads(sd, x, ts, True)

    vae = M.set_infovae_backend(vae, "hip").to(dev)
    recon, z = vae(x.to(dev))
    assert recon.shape == (B, 1, 28, 28) and z.shape == (B, 20)
    loss = M.infovae_loss(recon, x.to(dev), z, ts.to(dev))
    loss.backward()
    got = dict(vae.named_parameters())
    rows = [("recon", recon.detach().cpu().double(), rem, r64), ("z", z.detach().cpu().double(), zem, z64)]
    rows += [(k, got[k].grad.cpu().double(), gem[k], g64[k]) for k in GRADS]
    for name, hip, emu, ref in rows:
        e_hip, e_emu, top = float((hip - ref).abs().max()), float((emu - ref).abs().max()), float(ref.abs().max())
        bound = 2 * e_emu + FLOOR * top
        print("B=%d %-24s E_hip %.3e  E_emu %.3e  max|ref| %.3e  E_hip / bound %.2f" % (B, name, e_hip, e_emu, top, e_hip / bound))
        assert e_hip <= bound, (name, e_hip, e_emu, top)
    print("B=%d loss hip %.8f  float64 %.8f  emulated %.8f" % (B, float(loss.detach()), l64, lem))


def test_training_and_checkpoint(tmp_path):
    import multimodal_vae_amd.data as D
    import multimodal_vae_amd.evaluate as E
    import multimodal_vae_amd.mnist as M
    import multimodal_vae_amd.train_infovae_mnist as T
    dev = _dev()
    B = 32
    images = D.synthetic_mnist(B, seed=3)[0]
    data = images.float().div(255.0).unsqueeze(1)
    torch.manual_seed(21)
    vae = M.InfoVAE(n_latents=20)
    sd = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    ts = torch.randn(B, 20, generator=torch.Generator().manual_seed(6))
    _, _, l64, _ = _loss_and_grads(sd, data, ts, False)
    _, _, lem, _ = _loss_and_grads(sd, data, ts, True)
    with torch.no_grad():
        r_torch, z_torch = copy.deepcopy(vae).to(dev)(data.to(dev))
        loss_torch = float(M.infovae_loss(r_torch, data.to(dev), z_torch, ts.to(dev)))
    vae = M.set_infovae_backend(vae, "hip").to(dev)
    opt = torch.optim.Adam(vae.parameters(), lr=1e-3)
    xd = data.to(dev)
    losses = [float(T.train_step(vae, opt, xd, ts.to(dev) if k == 0 else None)) for k in range(20)]
    bound = 2 * abs(lem - l64) + FLOOR * abs(l64)
    print("step 0 %.8f (torch backend %.8f, |difference| %.3e; float64 %.8f, emulated %.8f, bound %.3e), last five %.6f, first five %.6f"
          % (losses[0], loss_torch, abs(losses[0] - loss_torch), l64, lem, bound, sum(losses[-5:]) / 5, sum(losses[:5]) / 5))
    assert all(torch.isfinite(torch.tensor(losses)))
    assert sum(losses[-5:]) / 5 < sum(losses[:5]) / 5
    assert abs(losses[0] - loss_torch) <= bound
    # the trained weights load into a CPU torch-backend model, and the checkpoint evaluates
    T.save_checkpoint({"state_dict": vae.state_dict(), "best_loss": losses[-1], "n_latents": 20, "optimizer": opt.state_dict()}, False,
                      folder=str(tmp_path))
    path = os.path.join(str(tmp_path), "checkpoint.pth.tar")
    cpu = M.load_infovae_checkpoint(path)
    assert cpu.conv_backend == "torch" and next(cpu.parameters()).device.type == "cpu"
    with torch.no_grad():
        vae.eval()
        r_hip, z_hip = vae(xd[:4])
        r_cpu, z_cpu = cpu.eval()(data[:4])
    assert float((r_hip.cpu() - r_cpu).abs().max()) < 5e-2 and torch.isfinite(z_cpu).all()
    torch.save((images, torch.zeros(B, dtype=torch.int64)), os.path.join(str(tmp_path), "images.pt"))
    for backend in ("torch", "hip"):
        out = E.main(["latent_mmd", path, "--dataset", "mnist", "--data", os.path.join(str(tmp_path), "images.pt"), "--conv_backend", backend])
        assert set(out) == {"n", "k_prior", "k_posterior", "k_cross", "mmd"} and out["n"] == B
        assert all(torch.isfinite(torch.tensor([float(v) for v in out.values()])))
