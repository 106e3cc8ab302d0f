"""float64 reference of the uni-modal image VAE (celeba/model.py:60-88, coco/model.py:93-117) and its loss
(celeba/train_imageonly.py:42-52, coco/train_imageonly.py:112-113), composed from the oracle's own functions:
``celeba_image_encoder`` / ``celeba_image_decoder``, ``coco_image_encoder`` / ``coco_image_decoder``, ``reparametrize``, ``kl_sum``
(inside the two losses), ``celeba_loss`` and ``coco_loss``.  There is NO product of experts here: mu and logvar are the two halves
of the encoder's output, untouched.
"""
import torch

from oracle import mmvae_ref as R

SIDE = {"celeba": 64, "coco": 32}
MASK_WIDTHS = {"celeba": (1024,), "coco": (1024, 256)}


def image_names(family, D):
    """The parameter names of the family's image half, in state_dict order."""
    return [n for n, _ in R.param_table(family, D) if n.startswith(("image_encoder.", "image_decoder."))]


def state_dict_keys(family, D):
    """The keys of ``ImageVAE(D).state_dict()``: the image half of ``R.param_table`` / ``R.bn_layers`` under ``encoder.`` /
    ``decoder.``, the three buffers of a BatchNorm right behind its bias (nn.Module order)."""
    bn = {p for p, _ in R.bn_layers(family, D)}
    keys = []
    for n in image_names(family, D):
        keys.append(n[len("image_"):])
        if n.endswith(".bias") and n[:-5] in bn:
            keys += [n[len("image_"):-5] + "." + b for b in ("running_mean", "running_var", "num_batches_tracked")]
    return keys


def params64(family, D, requires_grad=False):
    """``R.formula_params`` in float64 (every entry of the MMVAE's table: the second modality is there to show it is not used)."""
    p = {}
    for k, v in R.formula_params(family, D).items():
        if not v.is_floating_point():
            p[k] = v.clone()
        else:
            p[k] = v.detach().double().requires_grad_(requires_grad and "running_" not in k)
    return p


def forward(family, p, image, training, eps=None, masks=None, drop_p=R.DROP_P):
    """-> (recon, mu, logvar).  masks: celeba one keep mask (B,1024) or None; coco a pair or None."""
    image = image.double()
    if family == "celeba":
        o = R.celeba_image_encoder(p, image, training, None if masks is None else masks.double(), drop_p=drop_p)
    else:
        o = R.coco_image_encoder(p, image, training, None if masks is None else tuple(m.double() for m in masks), drop_p=drop_p)
    D = o.shape[1] // 2
    mu, logvar = o[:, :D], o[:, D:]
    z = R.reparametrize(mu, logvar, training, None if eps is None else eps.double())
    dec = R.celeba_image_decoder if family == "celeba" else R.coco_image_decoder
    return dec(p, z, training), mu, logvar


def loss(family, recon, image, mu, logvar, kl_lambda):
    image = image.double()
    if family == "celeba":
        return R.celeba_loss(mu, logvar, recon_x=recon, x=image, kl_lambda=kl_lambda)
    return R.coco_loss(mu, logvar, recon_image=recon, image=image, kl_lambda=kl_lambda, lambda_xy=1.)


def step_loss(family, p, image, training, eps=None, masks=None, drop_p=R.DROP_P, kl_lambda=1e-3):
    recon, mu, logvar = forward(family, p, image, training, eps, masks, drop_p)
    return loss(family, recon, image, mu, logvar, kl_lambda), (recon, mu, logvar)


# ---- the one-expert latent block alone (float64 formulas of mmvae_latent1_fwd / _bwd)
def latent1_fwd(enc_out, eps, training):
    enc_out = enc_out.double()
    D = enc_out.shape[1] // 2
    mu, lv = enc_out[:, :D], enc_out[:, D:]
    z = R.reparametrize(mu, lv, training, None if eps is None else eps.double())
    return mu, lv, z, R.kl_sum(mu, lv)


def latent1_bwd(mu, lv, eps, dz, kl_coef, training):
    mu, lv, dz = mu.double(), lv.double(), dz.double()
    gmu = dz + kl_coef * mu
    glv = -0.5 * kl_coef * (1.0 - torch.exp(lv))
    if training:
        glv = glv + dz * eps.double() * 0.5 * torch.exp(0.5 * lv)
    return torch.cat((gmu, glv), dim=1)
