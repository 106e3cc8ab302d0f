"""float64 reference of the fused COCO InfoVAE step (coco/model.py:358-402, coco/train_infovae.py:44-55):

    loss = lambda_x * BCE(recon, image) + lambda_mmd * MMD(true_samples, z) + kl_lambda * KL / B

``imageonly_ref.forward`` for the pass (no product of experts), ``torch.nn.functional.binary_cross_entropy`` (mean over B * 3072) and
``mmd_ref.formulation_mmd(true_samples, z)`` with autograd, at the dtype of the parameters (float64: the oracle; float32: the size of
an honest deviation, tests/test_cpu_infovae_step.py).

Faults (``fault=``), each one thing a fused step can get wrong without any value looking odd:
  "no_mmd_grad"       the MMD value is there, its gradient never reaches z
  "grad_for_samples"  z receives dMMD/d(true_samples) -- the x class of the sweep -- instead of dMMD/dz
  "lambda_ignored"    lambda_mmd taken as 1
  "cross_sign"        mean Kxx + mean Kyy + 2 mean Kxy
"""
import torch

from oracle import mmvae_ref as R
import imageonly_ref as IR
import mmd_ref as MR

FAULTS = ("no_mmd_grad", "grad_for_samples", "lambda_ignored", "cross_sign")
STEP_SHAPES = [(4, 100), (6, 20), (4, 124), (5, 4), (65, 100)]       # (B, D) of the GPU test of the step
MMD_ONLY_SHAPES = [(6, 20), (65, 100)]                               # (B, D) of the GPU test with lambda_x = 0


def params(D, dtype=torch.float64, requires_grad=False):
    """``R.formula_params('coco', D)`` at ``dtype``"""
    p = {}
    for k, v in R.formula_params("coco", D).items():
        if not v.is_floating_point():
            p[k] = v.clone()
        else:
            p[k] = v.detach().to(dtype).requires_grad_(requires_grad and "running_" not in k)
    return p


def inputs(B, D):
    """image, eps, true_samples of a case: the oracle's formula inputs"""
    return R.formula_inputs("coco", B)[0], R.formula_eps(B, D, 1), R.formula_eps(B, D, 4)


def masks_of(B, D):
    g = torch.Generator().manual_seed(7 * B + D)
    return tuple((torch.rand(B, w, generator=g) >= 0.1).to(torch.uint8) for w in IR.MASK_WIDTHS["coco"])


def _forward(p, image, training, eps, masks, drop_p, dtype):
    """imageonly_ref.forward at ``dtype`` (that function casts to float64 itself), also returning z"""
    image = image.to(dtype)
    o = R.coco_image_encoder(p, image, training, None if masks is None else tuple(m.to(dtype) for m in masks), drop_p=drop_p)
    D = o.shape[1] // 2
    mu, logvar = o[:, :D], o[:, D:]
    z = R.reparametrize(mu, logvar, training, None if eps is None else eps.to(dtype))
    return R.coco_image_decoder(p, z, training), mu, logvar, z


def mmd_term(true_samples, z, fault=None):
    """MMD(true_samples, z) as the loss sees it"""
    x = true_samples
    if fault == "cross_sign":
        return torch.mean(MR.formulation_kernel(x, x)) + torch.mean(MR.formulation_kernel(z, z)) + 2 * torch.mean(MR.formulation_kernel(x, z))
    if fault == "no_mmd_grad":
        return MR.formulation_mmd(x, z.detach())
    if fault == "grad_for_samples":
        xs = x.detach().clone().requires_grad_(True)
        v = MR.formulation_mmd(xs, z.detach())
        g, = torch.autograd.grad(v, xs)
        carrier = (g * z).sum()
        return v.detach() + carrier - carrier.detach()          # the value, with dMMD/dx as the gradient of z
    return MR.formulation_mmd(x, z)


def step_loss(p, image, training, eps, true_samples, masks=None, drop_p=0.0, lambda_x=1.0, lambda_mmd=1.0, kl_lambda=0.0, fault=None):
    """-> (loss, {"bce", "mmd", "kl"}, (recon, mu, logvar, z)) at the dtype of ``p``."""
    dtype = p["image_encoder.features.0.weight"].dtype
    if dtype == torch.float64 and fault is None:       # the oracle's pass is imageonly_ref's, literally
        recon, mu, logvar = IR.forward("coco", p, image, training, eps, None if masks is None else tuple(m.float() for m in masks), drop_p)
        z = R.reparametrize(mu, logvar, training, None if eps is None else eps.double())
    else:
        recon, mu, logvar, z = _forward(p, image, training, eps, masks, drop_p, dtype)
    bce = torch.nn.functional.binary_cross_entropy(recon, image.to(dtype))
    mmd = mmd_term(true_samples.to(dtype), z, fault)
    kl = R.kl_sum(mu, logvar)
    w_mmd = 1.0 if fault == "lambda_ignored" else lambda_mmd
    loss = lambda_x * bce + w_mmd * mmd + kl_lambda * kl / image.shape[0]
    return loss, {"bce": bce, "mmd": mmd, "kl": kl}, (recon, mu, logvar, z)


def reference_loss_function(recon_x, x, z, true_samples):
    """coco/train_infovae.py:44-55, as written there"""
    BCE = torch.nn.functional.binary_cross_entropy(recon_x.view(-1, 3 * 32 * 32), x.view(-1, 3 * 32 * 32))
    MMD = MR.formulation_mmd(true_samples, z)
    return BCE + MMD


def image_grads(p):
    """{name: gradient} of the image half after a backward"""
    return {n: p[n].grad for n in IR.image_names("coco", p["image_encoder.classifier.6.bias"].numel() // 2)}
