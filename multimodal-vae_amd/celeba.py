"""Drop-in Python face of the reference's ``celeba/model.py`` + ``loss_function`` (celeba/train.py:60-81).

Same class names, constructor arguments, ``forward`` signatures (``vae(image=, attrs=)``) and ``state_dict`` keys as
the reference.  ``nn.*`` children are parameter containers only; every module forward/backward is a call into
libmmvae_hip.so.  No CPU fallback.  ``FusedTrainer`` = the train() closure body (celeba/train.py:131-149) as one enqueue.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from ._lib import MMVAEError  # noqa: F401
from .core import CelebaState, FusedCelebaStep, FusedImageStep, Trainer, load_vae_checkpoint
from .modules import DECODER, Draw, ExpertsVAEBase, ProductOfExperts, Swish, VAEBase, _BCEMeanFn, _Core, _dropout_on, _KLSumFn, run_module
from .modules import DROP_P, swish  # noqa: F401  (public names of this module, like MMVAEError)

N_ATTRS = 18          # celeba/datasets.py:26-28

# the 40 columns of CelebA's Anno/list_attr_celeba.txt, in the file's order
ATTR_NAMES = ('5_o_Clock_Shadow Arched_Eyebrows Attractive Bags_Under_Eyes Bald Bangs Big_Lips Big_Nose Black_Hair Blond_Hair Blurry '
              'Brown_Hair Bushy_Eyebrows Chubby Double_Chin Eyeglasses Goatee Gray_Hair Heavy_Makeup High_Cheekbones Male '
              'Mouth_Slightly_Open Mustache Narrow_Eyes No_Beard Oval_Face Pale_Skin Pointy_Nose Receding_Hairline Rosy_Cheeks Sideburns '
              'Smiling Straight_Hair Wavy_Hair Wearing_Earrings Wearing_Hat Wearing_Lipstick Wearing_Necklace Wearing_Necktie '
              'Young').split()
ATTR_TO_IX_DICT = {name: ix for ix, name in enumerate(ATTR_NAMES)}
IX_TO_ATTR_DICT = {ix: name for ix, name in enumerate(ATTR_NAMES)}
# the 18 columns the model sees (celeba/datasets.py:26): Bald, Bangs, Black_Hair, Blond_Hair, Brown_Hair, Bushy_Eyebrows, Eyeglasses,
# Gray_Hair, Heavy_Makeup, Male, Mouth_Slightly_Open, Mustache, Pale_Skin, Receding_Hairline, Smiling, Straight_Hair, Wavy_Hair,
# Wearing_Hat
ATTR_IX_TO_KEEP = [4, 5, 8, 9, 11, 12, 15, 17, 18, 20, 21, 22, 26, 28, 31, 32, 33, 35]
assert len(ATTR_NAMES) == 40 and len(ATTR_IX_TO_KEEP) == N_ATTRS


def tensor_to_attributes(tensor):
    """celeba/datasets.py:100-113: an (18,) tensor of probabilities -> the names of the kept attributes above 0.5"""
    tensor = torch.round(torch.as_tensor(tensor).detach().float().cpu().reshape(-1))
    if tensor.numel() != N_ATTRS:
        raise ValueError("tensor_to_attributes: %d values, need %d" % (tensor.numel(), N_ATTRS))
    return [IX_TO_ATTR_DICT[ATTR_IX_TO_KEEP[i]] for i in range(N_ATTRS) if float(tensor[i]) > 0.5]


def attrs_from_names(names):
    """celeba/sample.py:44-48 (``fetch_celeba_attrs``) for one name, a comma-separated string or a list of names -> a (1, 18) float
    tensor with those attributes set.  A name that is no CelebA attribute, or not one of the kept 18, is refused."""
    if isinstance(names, str):
        names = [v for v in names.split(',') if v]
    attrs = torch.zeros(1, N_ATTRS)
    for name in names:
        if name not in ATTR_TO_IX_DICT:
            raise ValueError("attrs_from_names: %r is not a CelebA attribute" % (name,))
        if ATTR_TO_IX_DICT[name] not in ATTR_IX_TO_KEEP:
            raise ValueError("attrs_from_names: %r is not one of the %d attributes the model keeps (%s)"
                             % (name, N_ATTRS, ", ".join(IX_TO_ATTR_DICT[i] for i in ATTR_IX_TO_KEEP)))
        attrs[0, ATTR_IX_TO_KEEP.index(ATTR_TO_IX_DICT[name])] = 1
    return attrs


class ImageEncoder(nn.Module):
    """celeba/model.py:91-128"""

    def __init__(self, n_latents):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(3, 32, 4, 2, 1, bias=False), Swish(),
            nn.Conv2d(32, 64, 4, 2, 1, bias=False), nn.BatchNorm2d(64), Swish(),
            nn.Conv2d(64, 128, 4, 2, 1, bias=False), nn.BatchNorm2d(128), Swish(),
            nn.Conv2d(128, 256, 4, 1, 0, bias=False), nn.BatchNorm2d(256), Swish())
        self.classifier = nn.Sequential(nn.Linear(256 * 5 * 5, 1024), Swish(), nn.Dropout(p=0.1), nn.Linear(1024, n_latents * 2))
        self.n_latents = n_latents
        self._core = None

    def weight_init(self, mean, std):
        """celeba/model.py:121-123: iterates the two nn.Sequential containers, so it initialises nothing (kept as is)."""
        for m in self._modules:
            normal_init(self._modules[m], mean, std)

    def forward(self, x, mask: Optional[torch.Tensor] = None):
        n = self.n_latents
        x = x.contiguous().float()
        assert x.shape[1:] == (3, 64, 64), "expected (B,3,64,64) images"
        m1 = None
        if _dropout_on(self, (self.classifier[2].p,), "the HIP image encoder supports Dropout p in {0, 0.1} (reference: 0.1)"):
            m1 = Draw((x.shape[0], 1024), 2) if mask is None else mask.to(torch.uint8).contiguous()
        out = run_module(self, "image_encoder.", CelebaState, x, "mmvae_celeba_image_encoder", (2 * n,),
                         ("x", m1, "training", "out"), ("d", m1))
        return out[:, :n], out[:, n:]


class ImageDecoder(nn.Module):
    """celeba/model.py:131-161"""

    def __init__(self, n_latents):
        super().__init__()
        self.upsample = nn.Sequential(nn.Linear(n_latents, 256 * 5 * 5), Swish())
        self.hallucinate = nn.Sequential(
            nn.ConvTranspose2d(256, 128, 4, 1, 0, bias=False), nn.BatchNorm2d(128), Swish(),
            nn.ConvTranspose2d(128, 64, 4, 2, 1, bias=False), nn.BatchNorm2d(64), Swish(),
            nn.ConvTranspose2d(64, 32, 4, 2, 1, bias=False), nn.BatchNorm2d(32), Swish(),
            nn.ConvTranspose2d(32, 3, 4, 2, 1, bias=False))
        self.n_latents = n_latents
        self._core = None

    def weight_init(self, mean, std):
        for m in self._modules:
            normal_init(self._modules[m], mean, std)

    def forward(self, z):
        return run_module(self, "image_decoder.", CelebaState, z.contiguous().float(), "mmvae_celeba_image_decoder", (3, 64, 64),
                          *DECODER)


class AttributeEncoder(nn.Module):
    """celeba/model.py:164-178"""

    def __init__(self, n_latents):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(N_ATTRS, 64), nn.BatchNorm1d(64), Swish(), nn.Linear(64, n_latents * 2))
        self.n_latents = n_latents
        self._core = None

    def forward(self, x):
        n = self.n_latents
        x = x.contiguous().float()
        assert x.dim() == 2 and x.shape[1] == N_ATTRS
        out = run_module(self, "attrs_encoder.", CelebaState, x, "mmvae_celeba_attrs_encoder", (2 * n,),
                         ("x", "training", "out"), ("d",), bn_values=1)
        return out[:, :n], out[:, n:]


class AttributeDecoder(nn.Module):
    """celeba/model.py:181-196"""

    def __init__(self, n_latents):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(n_latents, 64), nn.BatchNorm1d(64), Swish(), nn.Linear(64, N_ATTRS))
        self.n_latents = n_latents
        self._core = None

    def forward(self, z):
        return run_module(self, "attrs_decoder.", CelebaState, z.contiguous().float(), "mmvae_celeba_attrs_decoder", (N_ATTRS,),
                          *DECODER, bn_values=1)


def normal_init(m, mean, std):
    """celeba/model.py:214-217"""
    if isinstance(m, (nn.ConvTranspose2d, nn.Conv2d)):
        m.weight.data.normal_(mean, std)
        m.bias.data.zero_()


class MultimodalVAE(ExpertsVAEBase):
    """celeba/model.py:14-57"""

    def __init__(self, n_latents=20, use_cuda=False):
        super().__init__()
        self.image_encoder = ImageEncoder(n_latents)
        self.image_decoder = ImageDecoder(n_latents)
        self.attrs_encoder = AttributeEncoder(n_latents)
        self.attrs_decoder = AttributeDecoder(n_latents)
        self.experts = ProductOfExperts()
        self.n_latents = n_latents
        self._core = _Core(self, "", n_latents, CelebaState)
        self._adopt(self.image_encoder, self.image_decoder, self.attrs_encoder, self.attrs_decoder)

    def weight_init(self, mean, std):
        self.image_encoder.weight_init(mean=mean, std=std)
        self.image_decoder.weight_init(mean=mean, std=std)

    def forward(self, image=None, attrs=None, eps=None, enc_mask=None):
        assert image is not None or attrs is not None
        mu, logvar = self._product(None if image is None else self.image_encoder(image, enc_mask),
                                   None if attrs is None else self.attrs_encoder(attrs))
        z = self.reparametrize(mu, logvar, eps)
        return self.image_decoder(z), self.attrs_decoder(z), mu, logvar


def loss_function(mu, logvar, recon_x=None, x=None, recon_y=None, y=None, kl_lambda=1e-3, lambda_x=1., lambda_y=1.):
    """celeba/train.py:60-81.  The per-attribute BCE loop averaged over attributes equals the mean over all B*18
    elements, which is what the kernel sums."""
    batch_size = mu.size(0)
    x_BCE, y_BCE = 0, 0
    if recon_x is not None and x is not None:
        x_BCE = _BCEMeanFn.apply(recon_x.reshape(-1, 3 * 64 * 64), x.reshape(-1, 3 * 64 * 64))
    if recon_y is not None and y is not None:
        y_BCE = _BCEMeanFn.apply(recon_y.reshape(-1, N_ATTRS), y.reshape(-1, N_ATTRS))
    KLD = _KLSumFn.apply(mu, logvar)
    KLD = KLD / batch_size * kl_lambda
    return lambda_x * x_BCE + lambda_y * y_BCE + KLD


elbo_loss = loss_function


def load_checkpoint(file_path, use_cuda=False):
    """celeba/train.py:46-58: rebuilds a MultimodalVAE from the checkpoint dict (``state_dict``, ``n_latents``) of either code base;
    a dict without ``n_latents`` gets the default of celeba/train.py:87 (100)."""
    return load_vae_checkpoint(file_path, MultimodalVAE, use_cuda, 100)


class FusedTrainer(Trainer):
    """``FusedTrainer(vae, batch_size, lr)(image, attrs)``: celeba/train.py:131-149 (3 passes, 3 losses), lr 1e-3, kl_lambda 1e-3."""
    ENGINE = FusedCelebaStep
    ENC_DROPOUT = staticmethod(lambda vae: vae.image_encoder.classifier[2].p)


# ----------------------------------------------------------------------------------------------------------------
# the uni-modal image baseline (celeba/model.py:60-88, celeba/train_imageonly.py)
# ----------------------------------------------------------------------------------------------------------------
class ImageVAE(VAEBase):
    """celeba/model.py:60-88: ``ImageEncoder`` + ``reparametrize`` + ``ImageDecoder`` under the reference's ``encoder.`` /
    ``decoder.`` keys, with NO product of experts.  The two children live on the MultimodalVAE's plan (``encoder.features.0.weight``
    is its ``image_encoder.features.0.weight``); the attribute half of the flat buffers keeps its initial value and never shows
    in ``state_dict()``.  ``ImageVAETrainer`` is the train() closure of celeba/train_imageonly.py:105-117 as one enqueue."""

    def __init__(self, n_latents=20):
        super().__init__()
        self.encoder = ImageEncoder(n_latents)
        self.decoder = ImageDecoder(n_latents)
        self.n_latents = n_latents
        self._core = _Core(self, "image_", n_latents, CelebaState)
        self._adopt(self.encoder, self.decoder)

    def encode(self, x, mask: Optional[torch.Tensor] = None):
        return self.encoder(x, mask)

    def weight_init(self, mean, std):
        self.encoder.weight_init(mean=mean, std=std)
        self.decoder.weight_init(mean=mean, std=std)

    def decode(self, z):
        return self.decoder(z)

    def forward(self, x, eps: Optional[torch.Tensor] = None, enc_mask: Optional[torch.Tensor] = None):
        mu, logvar = self.encode(x, enc_mask)
        z = self.reparametrize(mu, logvar, eps)
        return self.decode(z), mu, logvar


def imageonly_loss_function(recon_x, x, mu, logvar, kl_lambda=1e-3):
    """celeba/train_imageonly.py:42-52"""
    return loss_function(mu, logvar, recon_x=recon_x, x=x, kl_lambda=kl_lambda)


def load_checkpoint_imageonly(file_path, use_cuda=False):
    """celeba/train_imageonly.py:29-39: rebuilds an ImageVAE from the checkpoint dict (``state_dict``, ``n_latents``)."""
    return load_vae_checkpoint(file_path, ImageVAE, use_cuda)


class ImageVAETrainer(Trainer):
    """``ImageVAETrainer(vae, batch_size, lr)(image)``: celeba/train_imageonly.py:108-117, lr 1e-3, kl_lambda 1e-3, on an
    ``ImageVAE``: one pass over B rows (core.FusedImageStep)."""
    ENGINE = FusedImageStep
    ENC_DROPOUT = staticmethod(lambda vae: vae.encoder.classifier[2].p)
