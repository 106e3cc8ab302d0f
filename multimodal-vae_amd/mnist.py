"""Drop-in Python face of the reference's ``mnist/model.py`` + ``loss_function`` (mnist/train.py:64-81).

Same class names, constructor arguments, ``forward`` signatures and ``state_dict`` keys as the reference.  The
``nn.Linear / nn.BatchNorm1d / nn.Embedding`` children are parameter containers only; every module forward/backward
is a call into libmmvae_hip.so.  No CPU fallback.  ``FusedTrainer`` runs the whole train() closure body
(mnist/train.py:131-147 + optimizer.step()) as one enqueue.

``InfoVAE`` (mnist/model.py:238-279) is the exception: a plain torch module that runs wherever torch runs.
``set_infovae_backend(vae, "hip")`` routes its four bias-free 4 x 4 stride-2 convolutions, each with its activation, through
``conv4s2.down4s2`` / ``up4s2`` (csrc/conv4s2.hip); its four ``nn.Linear`` layers stay torch ops under both backends.
``FusedInfoVAE`` is the same model on a plan of its own: ``InfoVAETrainer`` runs its whole training step as one enqueue
(csrc/infovae_mnist.hip: the four Linears on the fp32 MFMA, the loss tail, the MMD sweep beside the decoder).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._lib import MMVAEError, call, ptr
from .core import (FusedImageStep, FusedInfoVAEStep, FusedMnistStep, MnistInfoVAEState, MnistState, StepOutputs, Trainer,
                   load_vae_checkpoint)
from .modules import DECODER, ExpertsVAEBase, ProductOfExperts, VAEBase, _BCEMeanFn, _Core, _KLSumFn, _NLLMeanFn, run_module

ENCODER_FWD = ("x", "training", "out")       # the C arguments of the two encoders' forward (modules.run_module); the decoders' are DECODER


class ImageEncoder(nn.Module):
    """mnist/model.py:99-118"""

    def __init__(self, n_latents):
        super().__init__()
        self.net = nn.Sequential(
            nn.Linear(784, 400), nn.BatchNorm1d(400), nn.ReLU(),
            nn.Linear(400, 200), nn.BatchNorm1d(200), nn.ReLU(),
            nn.Linear(200, n_latents * 2))
        self.n_latents = n_latents
        self._core = None

    def forward(self, x):
        n = self.n_latents
        x = x.contiguous().float()
        assert x.dim() == 2 and x.shape[1] == 784, "expected (B,784) flattened images (mnist/train.py:123)"
        out = run_module(self, "image_encoder.", MnistState, x, "mmvae_mnist_image_encoder", (2 * n,), ENCODER_FWD, ("d",), bn_values=1)
        return out[:, :n], out[:, n:]


class ImageDecoder(nn.Module):
    """mnist/model.py:121-133"""

    def __init__(self, n_latents):
        super().__init__()
        self.net = nn.Sequential(
            nn.Linear(n_latents, 200), nn.BatchNorm1d(200), nn.ReLU(),
            nn.Linear(200, 400), nn.BatchNorm1d(400), nn.ReLU(),
            nn.Linear(400, 784))
        self.n_latents = n_latents
        self._core = None

    def forward(self, z):
        return run_module(self, "image_decoder.", MnistState, z.contiguous().float(), "mmvae_mnist_image_decoder", (784,), *DECODER, bn_values=1)


class TextEncoder(nn.Module):
    """mnist/model.py:136-153"""

    def __init__(self, n_latents):
        super().__init__()
        self.net = nn.Sequential(nn.Embedding(10, 50), nn.BatchNorm1d(50), nn.ReLU(), nn.Linear(50, n_latents * 2))
        self.n_latents = n_latents
        self._core = None

    def forward(self, x):
        n = self.n_latents
        x = x.contiguous().long()
        assert x.dim() == 1, "expected (B,) digit labels"
        out = run_module(self, "text_encoder.", MnistState, x, "mmvae_mnist_text_encoder", (2 * n,), ENCODER_FWD, ("x", "d"), bn_values=1)
        return out[:, :n], out[:, n:]


class TextDecoder(nn.Module):
    """mnist/model.py:156-170"""

    def __init__(self, n_latents):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(n_latents, 10), nn.BatchNorm1d(10), nn.ReLU(), nn.Linear(10, 10))
        self.n_latents = n_latents
        self._core = None

    def forward(self, z):
        return run_module(self, "text_decoder.", MnistState, z.contiguous().float(), "mmvae_mnist_text_decoder", (10,), *DECODER, bn_values=1)


class MultimodalVAE(ExpertsVAEBase):
    """mnist/model.py:14-96"""

    def __init__(self, n_latents=20, precision="fp32"):
        """``precision``: "fp32" (default; the reference's own arithmetic, fp32 MFMA) or "bf16" (bf16 MFMA operands)."""
        super().__init__()
        self.image_encoder = ImageEncoder(n_latents)
        self.image_decoder = ImageDecoder(n_latents)
        self.text_encoder = TextEncoder(n_latents)
        self.text_decoder = TextDecoder(n_latents)
        self.experts = ProductOfExperts()
        self.n_latents = n_latents
        self.precision = precision
        self._core = _Core(self, "", n_latents, lambda n, d: MnistState(n, d, precision))
        self._adopt(self.image_encoder, self.image_decoder, self.text_encoder, self.text_decoder)

    def encode_image(self, x):
        return self.image_encoder(x)

    def decode_image(self, x):
        return self.image_decoder(x)

    def encode_text(self, x):
        return self.text_encoder(x)

    def decode_text(self, x):
        return self.text_decoder(x)

    def _latents(self, image, text):
        return self._product(None if image is None else self.encode_image(image), None if text is None else self.encode_text(text))

    def forward(self, image=None, text=None, eps=None):
        assert image is not None or text is not None
        mu, logvar = self._latents(image, text)
        z = self.reparametrize(mu, logvar, eps)
        return self.decode_image(z), self.decode_text(z), mu, logvar

    def gen_latents(self, image, text):
        """mnist/model.py:86-96"""
        mu, logvar = self._latents(image, text)
        return self.reparametrize(mu, logvar)


def loss_function(mu, logvar, recon_image=None, image=None, recon_text=None, text=None,
                  kl_lambda=1e-3, lambda_xy=1., lambda_yx=1.):
    """mnist/train.py:64-81 (``kl_lambda`` is accepted and ignored, as in the reference)."""
    batch_size = mu.size(0)
    image_BCE, text_BCE = 0, 0
    if recon_image is not None and image is not None:
        image_BCE = lambda_xy * _BCEMeanFn.apply(recon_image.reshape(-1, 784), image.reshape(-1, 784))
    if recon_text is not None and text is not None:
        text_BCE = lambda_yx * _NLLMeanFn.apply(recon_text, text)
    KLD = _KLSumFn.apply(mu, logvar)
    KLD = KLD / (batch_size * (784 / 3))
    return image_BCE + text_BCE + KLD


elbo_loss = loss_function


def load_checkpoint(file_path, use_cuda=False):
    """mnist/train.py:44-60: rebuilds a MultimodalVAE from the checkpoint dict (``state_dict``, ``n_latents``) of either code base."""
    return load_vae_checkpoint(file_path, MultimodalVAE, use_cuda, 20)


def plan_latents(n_latents):
    """The smallest latent size >= ``n_latents`` that the HIP plan accepts (a multiple of 4 from 4 to 124)."""
    return max(4, (int(n_latents) + 3) // 4 * 4)


def with_padded_latents(vae):
    """A ``MultimodalVAE`` of ``plan_latents(vae.n_latents)`` latents that computes what ``vae`` computes, for a model whose own
    latent size the HIP plan does not accept (``mnist/latent_viz.py`` wants n_latents = 2).  The extra latents get zero columns in
    the first Linear of either decoder, and zero rows and biases in the last Linear of either encoder (mu = logvar = 0 there), so
    ``decode_image(cat(z, 0))`` and ``decode_text(cat(z, 0))`` are ``vae``'s decoders at z, and the first n_latents entries of the
    encoders' outputs are ``vae``'s.  Every other parameter and buffer is copied; the result lives where ``vae`` lives, in its mode."""
    n, big_n = vae.n_latents, plan_latents(vae.n_latents)
    if big_n == n:
        return vae
    big = MultimodalVAE(n_latents=big_n, precision=vae.precision)
    small, sd = vae.state_dict(), big.state_dict()
    for k, v in small.items():
        if sd[k].shape == v.shape:
            sd[k] = v.detach().clone()
            continue
        t = torch.zeros_like(sd[k], device=v.device)
        if k.startswith(("image_decoder.net.0.", "text_decoder.net.0.")):          # (out, n) -> (out, big_n)
            t[:, :n] = v
        else:                                                                      # (2 n, ...) -> (2 big_n, ...): mu rows, logvar rows
            t[:n] = v[:n]
            t[big_n:big_n + n] = v[n:]
        sd[k] = t
    big.load_state_dict(sd)
    big.to(next(vae.parameters()).device)
    return big.train(vae.training)


class _FlatImageTrainer(Trainer):
    """The first input is a batch of images, handed to the engine as (B, 784) rows (the reference's ``x.view(-1, 784)``)."""

    def __call__(self, image, *rest, **kw) -> StepOutputs:
        return super().__call__(image.reshape(-1, 784), *rest, **kw)

    def evaluate(self, image, *rest, **kw) -> StepOutputs:
        return super().evaluate(image.reshape(-1, 784), *rest, **kw)


class FusedTrainer(_FlatImageTrainer):
    """``FusedTrainer(vae, batch_size, lr)(image, label)``: mnist/train.py:131-147,149 (3 passes, 3 losses; test(): :165-177), lr
    1e-3; the KL weight is fixed by the batch size (no ``kl_lambda``)."""
    ENGINE, KL_LAMBDA = FusedMnistStep, None


# ------------------------------------------------------------------------------------------------------ image-only VAE
class _ImageNet(nn.Sequential):
    """One half of ``VAE``: the reference's ``nn.Sequential`` as a parameter container (keys ``0.weight`` ... ``6.bias``, no
    ``.net.`` level) whose forward is the HIP image encoder / decoder module of the MMVAE plan.  The decoder half returns the
    sigmoid of its last Linear (the module entry point ends there), so ``VAE.decode`` adds nothing."""

    def __init__(self, name, n_latents, *layers):
        super().__init__(*layers)
        self._name, self.n_latents = name, n_latents

    def forward(self, x):
        x = x.contiguous().float()
        if self._name == "image_encoder":
            assert x.dim() == 2 and x.shape[1] == 784, "expected (B,784) flattened images (mnist/model.py:230)"
            return run_module(self, "image_encoder.net.", MnistState, x, "mmvae_mnist_image_encoder", (2 * self.n_latents,), ENCODER_FWD, ("d",), bn_values=1)
        return run_module(self, "image_decoder.net.", MnistState, x, "mmvae_mnist_image_decoder", (784,), *DECODER, bn_values=1)


class VAE(VAEBase):
    """mnist/model.py:188-232: the image-only baseline under the reference's ``state_dict`` keys (``encoder.0.weight`` ...
    ``decoder.6.bias``, BatchNorm buffers under ``encoder.1``, ``encoder.4``, ``decoder.1``, ``decoder.4``); a reference checkpoint
    loads strict.  No product of experts.  The two halves live on the fp32 MMVAE plan as its ``image_encoder.net.*`` /
    ``image_decoder.net.*``; the label half of the flat buffers keeps its initial value and never shows in ``state_dict()``.
    ``ImageVAETrainer`` is the train() closure of mnist/imageonly/train_imageonly.py:114-127 as one enqueue."""

    def __init__(self, n_latents=20):
        super().__init__()
        self.encoder = _ImageNet("image_encoder", n_latents,
                                 nn.Linear(784, 400), nn.BatchNorm1d(400), nn.ReLU(),
                                 nn.Linear(400, 200), nn.BatchNorm1d(200), nn.ReLU(),
                                 nn.Linear(200, n_latents * 2))
        self.decoder = _ImageNet("image_decoder", n_latents,
                                 nn.Linear(n_latents, 200), nn.BatchNorm1d(200), nn.ReLU(),
                                 nn.Linear(200, 400), nn.BatchNorm1d(400), nn.ReLU(),
                                 nn.Linear(400, 784))
        self.n_latents = n_latents
        # the plan's names of the same modules (image_encoder.net.0.weight is encoder.0.weight): an unregistered twin tree for _Core
        twin = nn.Module()
        twin.image_encoder, twin.image_decoder = nn.Module(), nn.Module()
        twin.image_encoder.net, twin.image_decoder.net = self.encoder, self.decoder
        object.__setattr__(self, "_twin", twin)
        self._core = _Core(twin, "", n_latents, lambda n, d: MnistState(n, d, "fp32"))
        self._adopt(self.encoder, self.decoder)

    @staticmethod
    def plan_name(key: str) -> str:
        """``encoder.0.weight`` -> ``image_encoder.net.0.weight``: the plan's name of a ``state_dict`` key"""
        half, rest = key.split(".", 1)
        return "image_%s.net.%s" % (half, rest)

    def encode(self, x):
        n = self.n_latents
        out = self.encoder(x)
        return out[:, :n], out[:, n:]

    def reparameterize(self, mu, logvar, eps: Optional[torch.Tensor] = None):
        return self.reparametrize(mu, logvar, eps)

    def decode(self, z):
        return self.decoder(z)

    def forward(self, x, eps: Optional[torch.Tensor] = None):
        mu, logvar = self.encode(x.view(-1, 784))
        z = self.reparameterize(mu, logvar, eps)
        return self.decode(z), mu, logvar


ImageVAE = VAE


def imageonly_loss(recon_x, x, mu, logvar):
    """mnist/imageonly/train_imageonly.py:60-71: (mean BCE over B * 784 elements + KLD / 784) / B; the extra 1 / B is the reference's."""
    batch_size = recon_x.size(0)
    if recon_x.device.type == "cuda" and recon_x.dtype == torch.float32:
        BCE = _BCEMeanFn.apply(recon_x.reshape(-1, 784), x.reshape(-1, 784))
        KLD = _KLSumFn.apply(mu, logvar)
    else:           # the same formula in torch ops, for tensors on the CPU or in another precision
        BCE = F.binary_cross_entropy(recon_x.reshape(-1, 784), x.reshape(-1, 784).to(recon_x.dtype))
        KLD = -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp())
    return (BCE + KLD / 784) / batch_size


def load_checkpoint_imageonly(file_path, use_cuda=False):
    """mnist/imageonly/train_imageonly.py:46-57: rebuilds a VAE from the checkpoint dict (``state_dict``, ``n_latents``)."""
    return load_vae_checkpoint(file_path, VAE, use_cuda)


class ImageVAETrainer(_FlatImageTrainer):
    """``ImageVAETrainer(vae, batch_size, lr)(image)``: mnist/imageonly/train_imageonly.py:114-127 (test(): :136-148), lr 1e-3, on a
    ``VAE``: one pass over B rows (core.FusedImageStep with lambda_x = 1 / B and kl_lambda = 1 / 784, which is the reference's
    (BCE + KLD / 784) / B).  ``out.losses()[0]`` is that loss."""
    ENGINE, KL_LAMBDA = FusedImageStep, 1.0 / 784
    ENC_DROPOUT = staticmethod(lambda vae: 0.0)        # the model has no dropout

    def _engine_kw(self, vae, batch_size):
        return {"lambda_x": 1.0 / batch_size}


# ------------------------------------------------------------------------------------------------------ InfoVAE
INFOVAE_BACKENDS = ("torch", "hip")


class InfoVAE(nn.Module):
    """mnist/model.py:238-279: the MMD-regularised convolutional autoencoder, same ``state_dict`` keys and shapes.  A plain torch
    module; ``conv_backend`` (``set_infovae_backend``) chooses what the four convolution + activation pairs run on."""

    def __init__(self, n_latents=20):
        super().__init__()
        self.n_latents = n_latents
        self.encoder_conv = nn.Sequential(
            nn.Conv2d(1, 64, 4, 2, 1, bias=False), nn.LeakyReLU(0.1, inplace=True),
            nn.Conv2d(64, 128, 4, 2, 1, bias=False), nn.LeakyReLU(0.1, inplace=True))
        self.encoder_fc = nn.Sequential(nn.Linear(128 * 7 * 7, 1024), nn.LeakyReLU(0.1, inplace=True), nn.Linear(1024, n_latents))
        self.decoder_fc = nn.Sequential(nn.Linear(n_latents, 1024), nn.ReLU(True), nn.Linear(1024, 128 * 7 * 7), nn.ReLU(True))
        self.decoder_conv = nn.Sequential(
            nn.ConvTranspose2d(128, 64, 4, 2, 1, bias=False), nn.ReLU(True),
            nn.ConvTranspose2d(64, 1, 4, 2, 1, bias=False))
        self.conv_backend = "torch"

    def encode(self, x):
        if self.conv_backend == "hip":
            from .conv4s2 import down4s2
            x = down4s2(x, self.encoder_conv[0].weight, "leaky", self.encoder_conv[1].negative_slope)
            x = down4s2(x, self.encoder_conv[2].weight, "leaky", self.encoder_conv[3].negative_slope)
        else:
            x = self.encoder_conv(x)
        # (the op returns channels-last storage: reshape, not view, flattens the logical (c, h, w) order encoder_fc.0 expects)
        return self.encoder_fc(x.reshape(x.size(0), -1))

    def decode(self, z):
        z = self.decoder_fc(z).view(-1, 128, 7, 7)
        if self.conv_backend == "hip":
            from .conv4s2 import up4s2
            z = up4s2(z, self.decoder_conv[0].weight, "relu")
            return up4s2(z, self.decoder_conv[2].weight, "sigmoid")
        return torch.sigmoid(self.decoder_conv(z))

    def forward(self, x):
        z = self.encode(x)
        return self.decode(z), z


def set_infovae_backend(vae, backend):
    """Chooses what the convolutions of an ``InfoVAE`` run on: ``"torch"`` (the default) or ``"hip"`` (each convolution with its
    activation is one ``down4s2`` / ``up4s2`` call; the model has to be on the device by the time of its forward: a CPU tensor
    raises ``MMVAEError``).  A plain attribute: no buffer, no parameter, the ``state_dict`` does not change.  The four ``nn.Linear``
    layers and their activations stay torch ops.  -> vae"""
    if backend not in INFOVAE_BACKENDS:
        raise MMVAEError("set_infovae_backend: %r, need one of %s" % (backend, INFOVAE_BACKENDS))
    if not isinstance(vae, InfoVAE):
        raise MMVAEError("set_infovae_backend: a mnist.InfoVAE expected (got %s)" % type(vae).__name__)
    vae.conv_backend = backend
    return vae


class FusedInfoVAE(nn.Module):
    """``InfoVAE`` (mnist/model.py:238-279) on the plan of the one-enqueue step (``mmvae_mnist_infovae_*``): same ``state_dict`` keys
    and shapes, so either class loads the other's checkpoint and a reference checkpoint loads strict.  On the device its parameters
    are views of the plan's flat buffer, which ``InfoVAETrainer`` updates in place.  ``encode`` / ``decode`` / ``forward`` run the HIP
    layers themselves (``conv4s2`` down / up, ``mmvae_lin_act_fwd`` with the (c, h, w) <-> channels-last permutation folded into the
    two large Linears) and build no autograd graph: this class is trained by ``InfoVAETrainer``, ``InfoVAE`` through autograd.
    Device-only: a CPU tensor raises ``MMVAEError``."""

    def __init__(self, n_latents=20):
        super().__init__()
        self.n_latents = n_latents
        self.encoder_conv = nn.Sequential(
            nn.Conv2d(1, 64, 4, 2, 1, bias=False), nn.LeakyReLU(0.1, inplace=True),
            nn.Conv2d(64, 128, 4, 2, 1, bias=False), nn.LeakyReLU(0.1, inplace=True))
        self.encoder_fc = nn.Sequential(nn.Linear(128 * 7 * 7, 1024), nn.LeakyReLU(0.1, inplace=True), nn.Linear(1024, n_latents))
        self.decoder_fc = nn.Sequential(nn.Linear(n_latents, 1024), nn.ReLU(True), nn.Linear(1024, 128 * 7 * 7), nn.ReLU(True))
        self.decoder_conv = nn.Sequential(
            nn.ConvTranspose2d(128, 64, 4, 2, 1, bias=False), nn.ReLU(True),
            nn.ConvTranspose2d(64, 1, 4, 2, 1, bias=False))
        self._core = _Core(self, "", n_latents, MnistInfoVAEState)

    def _sync(self, x):
        if not torch.is_tensor(x) or x.device.type != "cuda":
            raise MMVAEError("FusedInfoVAE runs on a gfx950 GPU only (got %s); mnist.InfoVAE is the torch module of the same weights"
                             % (x.device if torch.is_tensor(x) else type(x).__name__))
        self._core.sync(x.device)

    @staticmethod
    def _conv(entry, src, weight, act, dims, out_elems):
        from ._ops import CONV_WS, stream
        out = torch.empty(out_elems, dtype=torch.float32, device=src.device)
        ws = CONV_WS.get(src.device, int(call("mmvae_conv4s2_workspace_bytes", *dims)))
        call(entry, ptr(src), None, ptr(weight), ptr(out), 0, act, 0.1, *dims, ptr(ws), ws.numel(), stream())
        return out

    @staticmethod
    def _linear(x, lin, rows, act, perm):
        from ._ops import CONV_WS, stream
        N, K = lin.weight.shape
        y = torch.empty((rows, N), dtype=torch.float32, device=x.device)
        ws = CONV_WS.get(x.device, int(call("mmvae_lin_act_workspace_bytes", rows, N, K, 0)))
        call("mmvae_lin_act_fwd", ptr(x), ptr(lin.weight), ptr(lin.bias), ptr(y), rows, N, K, act, 0.1, perm, ptr(ws), ws.numel(), stream())
        return y

    @torch.no_grad()
    def encode(self, x):
        self._sync(x)
        B = x.shape[0]
        x = x.detach().float().contiguous().reshape(B, 784)          # (one channel: NCHW and channels-last coincide)
        with torch.cuda.device(x.device):
            h = self._conv("mmvae_conv4s2_down", x, self.encoder_conv[0].weight, 2, (B, 1, 64, 28, 28), B * 196 * 64)
            h = self._conv("mmvae_conv4s2_down", h, self.encoder_conv[2].weight, 2, (B, 64, 128, 14, 14), B * 6272)
            h = self._linear(h, self.encoder_fc[0], B, 2, 1)
            return self._linear(h, self.encoder_fc[2], B, 0, 0)

    @torch.no_grad()
    def decode(self, z):
        self._sync(z)
        B = z.shape[0]
        z = z.detach().float().contiguous()
        with torch.cuda.device(z.device):
            h = self._linear(z, self.decoder_fc[0], B, 1, 0)
            h = self._linear(h, self.decoder_fc[2], B, 1, 1)
            h = self._conv("mmvae_conv4s2_up", h, self.decoder_conv[0].weight, 1, (B, 64, 128, 14, 14), B * 196 * 64)
            return self._conv("mmvae_conv4s2_up", h, self.decoder_conv[2].weight, 3, (B, 1, 64, 28, 28), B * 784).view(B, 1, 28, 28)

    def forward(self, x):
        z = self.encode(x)
        return self.decode(z), z


class InfoVAETrainer(Trainer):
    """``InfoVAETrainer(vae, batch_size, lr=1e-3)(image)``: mnist/train_infovae.py:123-130 on a ``FusedInfoVAE`` as one enqueue
    (core.FusedInfoVAEStep on the model's own plan, mmvae_mnist_infovae_step) + one Adam launch over the flat buffer.
    ``out.total()`` is the reference's loss, mean squared error + MMD(prior samples, z); ``true_samples=`` supplies the prior samples
    (default: drawn on the device).  Images come as (B, 1, 28, 28) or flattened (B, 784)."""
    ENGINE, KL_LAMBDA = FusedInfoVAEStep, None

    def __init__(self, vae, batch_size: int, lr: float = 1e-3, seed: int = 1234, **engine_kw):
        if not isinstance(vae, FusedInfoVAE):
            raise MMVAEError("InfoVAETrainer: a mnist.FusedInfoVAE expected (got %s)" % type(vae).__name__)
        super().__init__(vae, batch_size, lr=lr, seed=seed, **engine_kw)


def mmd_terms_torch(x, y):
    """mnist/train_infovae.py:59-76 in torch ops, for a model that lives on the CPU -> (mean Kxx, mean Kyy, mean Kxy, MMD)"""
    def kernel(a, b):
        return torch.exp(-(a.unsqueeze(1) - b.unsqueeze(0)).pow(2).mean(dim=2) / float(a.size(1)))
    kxx, kyy, kxy = kernel(x, x).mean(), kernel(y, y).mean(), kernel(x, y).mean()
    return kxx, kyy, kxy, kxx + kyy - 2 * kxy


def infovae_loss(recon_x, x, z, true_samples: Optional[torch.Tensor] = None):
    """mnist/train_infovae.py:45-56: ``mean((recon_x - x)^2) + MMD(true_samples, z)``, ``true_samples ~ N(0, I)`` of z's shape drawn
    on z's device when not given.  On the device the MMD term is the fused op ``mmd.compute_mmd``; for a model on the CPU it is the
    same formula in torch ops."""
    if true_samples is None:
        true_samples = torch.randn(z.shape, device=z.device, dtype=z.dtype)
    NLL = F.mse_loss(recon_x, x)
    if z.device.type == "cuda":
        from .mmd import compute_mmd
        return NLL + compute_mmd(true_samples, z)
    return NLL + mmd_terms_torch(true_samples, z)[3]


def load_infovae_checkpoint(file_path, use_cuda=False):
    """mnist/train_infovae.py:28-42: rebuilds an InfoVAE (torch backend) from the checkpoint dict of either code base."""
    checkpoint = torch.load(file_path, map_location=None if use_cuda else 'cpu', weights_only=False)
    vae = InfoVAE(n_latents=checkpoint['n_latents'])
    vae.load_state_dict(checkpoint['state_dict'])
    if use_cuda:
        vae.cuda()
    return vae
