"""Drop-in Python face of the reference's ``multimnist/model.py`` + ``loss_function`` (multimnist/train.py:69-87).

Same class names, constructor arguments, ``forward`` signatures, ``state_dict`` keys and train/eval behaviour as the
reference, so a reference-style ``train.py`` loop runs unchanged:

    vae = MultimodalVAE(n_latents=100, use_cuda=True).cuda()
    optimizer = optim.Adam(vae.parameters(), lr=1e-3)
    recon_image, recon_text, mu, logvar = vae(image, text)
    loss = loss_function(mu, logvar, recon_image=..., image=..., recon_text=..., text=..., kl_lambda=..., ...)
    loss.backward(); optimizer.step()

The ``nn.Conv2d / nn.Linear / nn.GRU ...`` children are kept ONLY as parameter containers (default PyTorch
initialisation, ``state_dict`` names): their ``forward`` is never called.  Every module forward/backward is a call
into libmmvae_hip.so (hand-written HIP kernels); there is no PyTorch/CPU fallback -- on a machine without a gfx950
GPU the first forward raises ``MMVAEError``.  The whole 3-pass training step as ONE fused enqueue is
``FusedTrainer`` below (what ``bench.py`` measures).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn

from ._lib import MMVAEError
from .core import FusedELBOStep, FusedImageStep, FusedMMTextStep, MultimnistState, MultimnistTextState, Trainer, load_vae_checkpoint
from .modules import (DECODER, Draw, ExpertsVAEBase, ProductOfExperts, Swish, VAEBase, _BCEMeanFn, _Core, _dropout_on, _KLSumFn, _NLLMeanFn,
                      _seed_from_torch, run_module)
from .modules import DROP_P, swish  # noqa: F401  (public names of this module)

# multimnist/utils.py:14-19
max_length = 4
all_characters = '0123456789'
n_characters = len(all_characters)
SOS = n_characters
FILL = n_characters + 1
n_characters += 2


# ----------------------------------------------------------------------------------------------------------------
# modules (parameter containers mirror multimnist/model.py exactly)
# ----------------------------------------------------------------------------------------------------------------
class ImageEncoder(nn.Module):
    """multimnist/model.py:150-188"""

    def __init__(self, n_latents):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(1, 32, 4, 2, 1, bias=False), Swish(),
            nn.Conv2d(32, 64, 4, 2, 1, bias=False), nn.BatchNorm2d(64), Swish(),
            nn.Conv2d(64, 128, 4, 2, 1, bias=False), nn.BatchNorm2d(128), Swish(),
            nn.Conv2d(128, 256, 4, 2, 0, bias=False), nn.BatchNorm2d(256), Swish())
        self.classifier = nn.Sequential(
            nn.Linear(256 * 2 * 2, 400), Swish(), nn.Dropout(p=0.1),
            nn.Linear(400, 200), Swish(), nn.Dropout(p=0.1),
            nn.Linear(200, n_latents * 2))
        self.n_latents = n_latents
        self._core = None

    def forward(self, x, masks: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        n = self.n_latents
        x = x.contiguous().float()
        B = x.shape[0]
        assert x.shape[1:] == (1, 50, 50), "expected (B,1,50,50) images"
        m1 = m2 = None
        if _dropout_on(self, (self.classifier[2].p, self.classifier[5].p), "the HIP image encoder supports Dropout p in {0, 0.1} (reference: 0.1)"):
            if masks is not None:
                m1, m2 = (m.to(torch.uint8).contiguous() for m in masks)
            else:
                seed = _seed_from_torch()                            # one seed, two Philox streams
                m1, m2 = Draw((B, 400), 2, seed), Draw((B, 200), 3, seed)
        out = run_module(self, "image_encoder.", MultimnistState, x, "mmvae_mm_image_encoder", (2 * n,),
                         ("x", m1, m2, "training", "out"), ("d", m1, m2), bn_values=625)       # no gradient w.r.t. the image
        return out[:, :n], out[:, n:]


class ImageDecoder(nn.Module):
    """multimnist/model.py:191-216"""

    def __init__(self, n_latents):
        super().__init__()
        self.upsample = nn.Sequential(nn.Linear(n_latents, 256 * 2 * 2), Swish())
        self.hallucinate = nn.Sequential(
            nn.ConvTranspose2d(256, 128, 4, 2, 0, bias=False), nn.BatchNorm2d(128), Swish(),
            nn.ConvTranspose2d(128, 64, 4, 2, 1, bias=False), nn.BatchNorm2d(64), Swish(),
            nn.ConvTranspose2d(64, 32, 5, 2, 1, bias=False), nn.BatchNorm2d(32), Swish(),
            nn.ConvTranspose2d(32, 1, 4, 2, 1, bias=False))
        self.n_latents = n_latents
        self._core = None

    def forward(self, z):
        return run_module(self, "image_decoder.", MultimnistState, z.contiguous().float(), "mmvae_mm_image_decoder", (1, 50, 50),
                          *DECODER, bn_values=36)


class TextEncoder(nn.Module):
    """multimnist/model.py:219-247 (bidirectional=True is the only configuration MultimodalVAE uses)."""

    def __init__(self, n_latents, n_characters, n_hiddens=50, bidirectional=True, _textvae=False):
        super().__init__()
        # (_textvae: built by TextVAE, whose plan runs the kernels' hidden-size-50 instantiation)
        if n_hiddens != (50 if _textvae else 100) or not bidirectional or n_characters != 12:
            raise MMVAEError("the HIP TextEncoder implements the configuration used by MultimodalVAE: "
                             "n_characters=12, n_hiddens=100, bidirectional=True")
        self._base, self._pfx = ("mmvae_mmtext_encoder", "encoder.") if _textvae else ("mmvae_mm_text_encoder", "text_encoder.")
        self.embed = nn.Embedding(n_characters, n_hiddens)
        self.gru = nn.GRU(n_hiddens, n_hiddens, 1, dropout=0.0, bidirectional=bidirectional)   # dropout is a no-op for 1 layer
        self.h2p = nn.Linear(n_hiddens, n_latents * 2)
        self.n_latents = n_latents
        self.n_hiddens = n_hiddens
        self.bidirectional = bidirectional
        self._core = None

    def forward(self, x):
        n = self.n_latents
        x = x.contiguous().long()
        assert x.shape == (x.shape[0], max_length)
        out = run_module(self, self._pfx, MultimnistState, x, self._base, (2 * n,), ("x", "out"), ("x", "d"))
        return out[:, :n], out[:, n:]


class TextDecoder(nn.Module):
    """multimnist/model.py:250-307: 2-layer GRU, 4 greedy steps, log-softmax outputs (B, 4, 12)."""

    def __init__(self, n_latents, n_characters, n_hiddens=50, use_cuda=False, _textvae=False):
        super().__init__()
        if n_hiddens != (50 if _textvae else 100) or n_characters != 12:
            raise MMVAEError("the HIP TextDecoder implements the configuration used by MultimodalVAE: "
                             "n_characters=12, n_hiddens=100")
        self._base, self._pfx = ("mmvae_mmtext_decoder", "decoder.") if _textvae else ("mmvae_mm_text_decoder", "text_decoder.")
        self.n_hiddens = n_hiddens
        self.embed = nn.Embedding(n_characters, n_hiddens)
        self.z2h = nn.Linear(n_latents, n_hiddens)
        self.gru = nn.GRU(n_hiddens + n_latents, n_hiddens, 2, dropout=0.1)
        self.h2o = nn.Linear(n_hiddens + n_latents, n_characters)
        self.use_cuda = use_cuda
        self.n_latents = n_latents
        self.n_characters = n_characters
        self._core = None
        self.last_tokens = None

    def forward(self, z, keep: Optional[torch.Tensor] = None, force_tokens: Optional[torch.Tensor] = None):
        z = z.contiguous().float()
        B = z.shape[0]
        if not _dropout_on(self, (self.gru.dropout,), "the HIP text decoder supports GRU dropout in {0, 0.1} (reference: 0.1)"):
            keep = None
        elif keep is None:
            keep = Draw((max_length, B, self.n_hiddens), 4)
        else:
            keep = keep.to(torch.uint8).contiguous()
        ft = None if force_tokens is None else force_tokens.contiguous().long()
        tokens = torch.empty(B, max_length, dtype=torch.int64, device=z.device)
        words = run_module(self, self._pfx, MultimnistState, z, self._base, (max_length, n_characters),
                           ("x", "training", keep, ft, "out", tokens), ("x", keep, ft, "out", tokens, "d", "dx"))
        self.last_tokens = tokens
        return words

    def generate(self, z):
        """multimnist/model.py:290-296.  NB the reference samples ``torch.multinomial`` from LOG-probabilities (weights
        <= 0): under a modern torch that raises ("probability tensor contains ... element < 0"), and so does this method.
        The sampler runs on a host copy of the (B*4, 12) log-probabilities: on the GPU the same check is a device-side
        assertion that aborts the whole process instead of raising."""
        words = self.forward(z)
        batch_size, char_size = words.size(0), words.size(2)
        sample = torch.multinomial(words.detach().cpu().view(-1, char_size), 1)
        return sample.view(batch_size, max_length).to(words.device)


class MultimodalVAE(ExpertsVAEBase):
    """multimnist/model.py:21-93"""

    def __init__(self, n_latents=20, use_cuda=False):
        super().__init__()
        self.image_encoder = ImageEncoder(n_latents)
        self.image_decoder = ImageDecoder(n_latents)
        self.text_encoder = TextEncoder(n_latents, n_characters, n_hiddens=100, bidirectional=True)
        self.text_decoder = TextDecoder(n_latents, n_characters, n_hiddens=100, use_cuda=use_cuda)
        self.experts = ProductOfExperts()
        self.n_latents = n_latents
        self._core = _Core(self, "", n_latents)
        self._adopt(self.image_encoder, self.image_decoder, self.text_encoder, self.text_decoder)

    def encode_image(self, x):
        return self.image_encoder(x)

    def decode_image(self, z):
        return self.image_decoder(z)

    def encode_text(self, x):
        return self.text_encoder(x)

    def decode_text(self, z):
        return self.text_decoder(z)

    def forward(self, image=None, text=None, eps=None, enc_masks=None, gru_keep=None, force_tokens=None):
        assert image is not None or text is not None
        mu, logvar = self._product(None if image is None else self.image_encoder(image, enc_masks),
                                   None if text is None else self.encode_text(text))
        z = self.reparametrize(mu, logvar, eps)
        image_recon = self.decode_image(z)
        text_recon = self.text_decoder(z, gru_keep, force_tokens)
        return image_recon, text_recon, mu, logvar


class TextVAE(VAEBase):
    """multimnist/model.py:123-147: ``TextEncoder`` + ``reparametrize`` + ``TextDecoder`` at n_hiddens = 50 under the reference's
    ``encoder.`` / ``decoder.`` keys, with NO product of experts.  The two children share ONE core on a plan of their own
    (``core.MultimnistTextState``: the text kernels' hidden-size-50 instantiation), which is what ``TextVAETrainer`` steps in one
    enqueue."""

    N_HIDDENS = 50

    def __init__(self, n_latents=20, use_cuda=False):
        super().__init__()
        self.encoder = TextEncoder(n_latents, n_characters, _textvae=True)
        self.decoder = TextDecoder(n_latents, n_characters, use_cuda=use_cuda, _textvae=True)
        self.n_latents = n_latents
        self._core = _Core(self, "", n_latents, lambda n, d: MultimnistTextState(n, d, self.N_HIDDENS))
        self._adopt(self.encoder, self.decoder)

    def encode(self, x):
        return self.encoder(x)

    def decode(self, z, keep: Optional[torch.Tensor] = None, force_tokens: Optional[torch.Tensor] = None):
        return self.decoder(z, keep, force_tokens)

    def forward(self, x, eps=None, gru_keep=None, force_tokens=None):
        mu, logvar = self.encode(x)
        z = self.reparametrize(mu, logvar, eps)
        return self.decode(z, gru_keep, force_tokens), mu, logvar


class ImageVAE(VAEBase):
    """multimnist/model.py:96-120: ``ImageEncoder`` + ``reparametrize`` + ``ImageDecoder`` under the reference's ``encoder.`` /
    ``decoder.`` keys, with NO product of experts (no 1e-8 in a model that has no experts).  The two children live on the
    MultimodalVAE's plan (``encoder.features.0.weight`` is its ``image_encoder.features.0.weight``); the text half of the flat
    buffers keeps its initial value and never shows in ``state_dict()``.  ``ImageVAETrainer`` is the train() closure of
    multimnist/train_imageonly.py:91-106 as one enqueue."""

    def __init__(self, n_latents=20):
        super().__init__()
        self.encoder = ImageEncoder(n_latents)
        self.decoder = ImageDecoder(n_latents)
        self.n_latents = n_latents
        self._core = _Core(self, "image_", n_latents)
        self._adopt(self.encoder, self.decoder)

    def encode(self, x, masks: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        return self.encoder(x, masks)

    def decode(self, z):
        return self.decoder(z)

    def forward(self, x, eps: Optional[torch.Tensor] = None, enc_masks: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        mu, logvar = self.encode(x, enc_masks)
        z = self.reparametrize(mu, logvar, eps)
        return self.decode(z), mu, logvar


def load_checkpoint_imageonly(file_path, use_cuda=False):
    """multimnist/train_imageonly.py:29-40: rebuilds an ImageVAE from the checkpoint dict (``state_dict``, ``n_latents``)."""
    return load_vae_checkpoint(file_path, ImageVAE, use_cuda)


def load_checkpoint_textonly(file_path, use_cuda=False):
    """multimnist/train_textonly.py:31-42: rebuilds a TextVAE from the checkpoint dict (``state_dict``, ``n_latents``)."""
    return load_vae_checkpoint(file_path, TextVAE, use_cuda, use_cuda=use_cuda)


# ----------------------------------------------------------------------------------------------------------------
# loss_function (multimnist/train.py:69-87)
# ----------------------------------------------------------------------------------------------------------------
def loss_function(mu, logvar, recon_image=None, image=None, recon_text=None, text=None,
                  kl_lambda=1e-3, lambda_xy=1., lambda_yx=1.):
    """multimnist/train.py:69-87; returns a 0-d tensor supporting .backward() and .item()."""
    batch_size = mu.size(0)
    image_BCE, text_BCE = 0, 0
    if recon_image is not None and image is not None:
        image_BCE = lambda_xy * _BCEMeanFn.apply(recon_image.reshape(-1, 1 * 50 * 50), image.reshape(-1, 1 * 50 * 50))
    if recon_text is not None and text is not None:
        text_BCE = lambda_yx * _NLLMeanFn.apply(recon_text.reshape(-1, recon_text.size(2)), text.reshape(-1))
    KLD = _KLSumFn.apply(mu, logvar)
    KLD = KLD / batch_size * kl_lambda
    return image_BCE + text_BCE + KLD


elbo_loss = loss_function          # the name BASELINE.json uses


def imageonly_loss_function(recon_x, x, mu, logvar, kl_lambda=1e-3):
    """The loss of multimnist/train_imageonly.py:102-103: loss_function with the image term alone, lambda_xy = 1."""
    return loss_function(mu, logvar, recon_image=recon_x, image=x, kl_lambda=kl_lambda, lambda_xy=1.)


def textonly_loss_function(mu, logvar, recon_text, text, kl_lambda=1e-3):
    """The loss of multimnist/train_textonly.py:105-106: loss_function with the text term alone, lambda_yx = 1."""
    return loss_function(mu, logvar, recon_text=recon_text, text=text, kl_lambda=kl_lambda, lambda_yx=1.)


# ----------------------------------------------------------------------------------------------------------------
# fused trainer: the train() closure body of multimnist/train.py:146-173 as one enqueue
# ----------------------------------------------------------------------------------------------------------------
class FusedTrainer(Trainer):
    """``FusedTrainer(vae, batch_size, lr)(image, text)``: multimnist/train.py:146-173 (3 passes, 3 losses), lr 1e-3, kl_lambda 1e-3;
    ``evaluate`` is its test() closure body (:197-209)."""
    ENGINE = FusedELBOStep
    ENC_DROPOUT = staticmethod(lambda vae: vae.image_encoder.classifier[2].p)
    GRU_DROPOUT = staticmethod(lambda vae: vae.text_decoder.gru.dropout)


class TextVAETrainer(Trainer):
    """``TextVAETrainer(vae, batch_size, lr)(text)``: multimnist/train_textonly.py:95-113 (test(): :118-131), lr 1e-3, kl_lambda
    1e-3, on a ``TextVAE``: one pass over B rows."""
    ENGINE = FusedMMTextStep
    GRU_DROPOUT = staticmethod(lambda vae: vae.decoder.gru.dropout)


class ImageVAETrainer(Trainer):
    """``ImageVAETrainer(vae, batch_size, lr)(image)``: multimnist/train_imageonly.py:91-106 (test(): :115-128), lr 1e-3, kl_lambda
    1e-3, on an ``ImageVAE``: one pass over B rows (core.FusedImageStep)."""
    ENGINE = FusedImageStep
    ENC_DROPOUT = staticmethod(lambda vae: vae.encoder.classifier[2].p)
