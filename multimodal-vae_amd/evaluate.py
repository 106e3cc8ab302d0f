"""Eval-mode consumers of the model surface: the reference's ``compute_nll``
(multimnist/loglikelihood.py:20-69) and ``test_multimnist`` accuracy (multimnist/test.py:23-59), running on the HIP
modules in eval mode (BatchNorm running statistics, no dropout, z = mu).

``compute_nll`` quirk kept out: the reference calls ``F.nll_loss(recon_text (B,4,12), text (B,4), size_average=False)``
directly, which modern torch rejects (class dimension mismatch); the evident intent -- the summed negative log-likelihood
of the 4 target characters -- is what is computed here (``recon_text.view(-1, 12)`` against ``text.view(-1)``).

What differs between the ten model kinds (the four ``MultimodalVAE``s and their ``ImageVAE`` / ``TextVAE`` baselines) is ONE table,
``_FAMILIES``: the NLL loop, the posterior helper under ``_proposal`` and the samplers, ``iw_estimate`` and the command line ask it
and hold no per-family branch of their own.
"""
from __future__ import annotations

import functools
import importlib

import numpy as np
import torch

from . import _ops
from ._lib import call, ptr
from .modules import _BCEMeanFn, _NLLMeanFn
from .utils import FILL, max_length


@torch.no_grad()
def _reference_nll(model, loader, family, posterior, n_samples, use_cuda, verbose):
    """The reference's per-particle NLL loop, shared by the ``compute_nll*`` wrappers: per batch the posterior's (mu, logvar), ONE set
    of ``n_samples`` standard-normal draws shared by the rows of the batch (the reference's behaviour, kept), the summed loss of every
    decoded particle -- the image term, then the second modality's -- averaged over the particles; in the end divided by the number
    of examples.  -> [image NLL per sample, second NLL per sample] (the second stays 0.0 for an ``ImageVAE``)."""
    fam = _FAMILIES[family]
    model.eval()
    totals, n_seen = [0.0, 0.0], 0
    for image, second in loader:
        if use_cuda:
            image, second = image.cuda(), None if fam.image_only else second.cuda()
        image = image.float().reshape(-1, *fam.image_shape)       # (MNIST: the reference's view(-1, 784); the others come in this shape)
        mu, logvar = _posterior_of(model, fam, image, second, posterior)
        batch_size, n_latents = mu.size(0), mu.size(1)
        sample = torch.randn(n_samples, n_latents)                # drawn on the host like the reference, after the encoders ran
        if use_cuda:
            sample = sample.cuda()
        z = sample.unsqueeze(0) * logvar.mul(0.5).exp().unsqueeze(1) + mu.unsqueeze(1)      # (B, n_samples, D)
        nll = [0.0, 0.0]
        for i in range(n_samples):
            zi = z[:, i].contiguous()
            nll[0] += float(_bce_rows(fam, fam.reach(model, "decode_image")(zi), image)) * image.numel()
            if not fam.image_only:
                nll[1] += float(fam.second_loss(fam, fam.reach(model, "decode_second")(zi), second)) * second.numel()
        totals = [t + v / n_samples for t, v in zip(totals, nll)]
        n_seen += batch_size
        if verbose:
            print('Evaluating: [{}/{}]'.format(n_seen, len(loader) * batch_size))
    return [t / max(n_seen, 1) for t in totals]


def _mode(image_only, second_only):
    assert not (image_only and second_only)
    return "image" if image_only else "text" if second_only else "joint"


def compute_nll(model, loader, image_only=False, text_only=False, n_samples=1, use_cuda=True, verbose=False):
    """-> (image NLL per sample, text NLL per sample), multimnist/loglikelihood.py:20-69."""
    return tuple(_reference_nll(model, loader, "multimnist", _mode(image_only, text_only), n_samples, use_cuda, verbose))


@torch.no_grad()
def test_multimnist(model, loader, use_cuda=True, verbose=True):
    """-> (character accuracy, length accuracy) of text predicted from the image alone, multimnist/test.py:23-59."""
    model.eval()
    char_correct, len_correct, n_seen = 0.0, 0.0, 0
    for image, text in loader:
        if use_cuda:
            image, text = image.cuda(), text.cuda()
        _, recon_text, _, _ = model(image=image)
        pred = torch.max(recon_text, dim=2)[1].cpu().numpy()
        gt = text.cpu().numpy()
        char_correct += float(np.sum(pred == gt))
        len_correct += float(np.sum(np.sum(pred == FILL, axis=1) == np.sum(gt == FILL, axis=1)))
        n_seen += len(gt)
    _char_correct = char_correct / max(n_seen * max_length, 1)
    _len_correct = len_correct / max(n_seen, 1)
    if verbose:
        print('\nTest set: Character Accuracy: {}/{} ({:.0f}%)\tLength Accuracy: {}/{} ({:.0f}%)\n'.format(
            int(char_correct), n_seen * max_length, 100. * _char_correct, int(len_correct), n_seen, 100. * _len_correct))
    return _char_correct, _len_correct


test_multimnist.__test__ = False          # not a pytest test


# ------------------------------------------------------------------------------------------------------------------
# MNIST consumers (mnist/loglikelihood.py:15-65, mnist/test.py:18-36)

def compute_nll_mnist(model, loader, image_only=False, text_only=False, n_samples=1, use_cuda=True, verbose=False):
    """-> (image NLL per sample, label NLL per sample), mnist/loglikelihood.py:15-65."""
    return tuple(_reference_nll(model, loader, "mnist", _mode(image_only, text_only), n_samples, use_cuda, verbose))


def compute_nll_mnist_imageonly(model, loader, n_samples=1, use_cuda=True, verbose=False):
    """-> image NLL per sample of a ``mnist.VAE``, mnist/imageonly/loglikelihood_imageonly.py:17-51: the eval-mode encoder's
    (mu, logvar), ONE set of ``n_samples`` standard-normal draws shared by the rows of a batch (the reference's behaviour, kept),
    the summed BCE of every decoded particle, averaged over the particles and divided by the number of examples."""
    return _reference_nll(model, loader, "mnist_image", "image", n_samples, use_cuda, verbose)[0]


@torch.no_grad()
def test_mnist(model, loader, use_cuda=True, verbose=True):
    """-> accuracy of the label predicted from the image alone, mnist/test.py:18-36."""
    model.eval()
    correct, n_seen = 0, 0
    for image, text in loader:
        if use_cuda:
            image, text = image.cuda(), text.cuda()
        _, recon_text, _, _ = model(image=image.float().reshape(-1, 784))
        pred = recon_text.max(1, keepdim=True)[1]
        correct += int(pred.eq(text.view_as(pred)).sum())
        n_seen += int(text.numel())
    if verbose:
        print('\nTest set: Accuracy: {}/{} ({:.0f}%)\n'.format(correct, n_seen, 100. * correct / max(n_seen, 1)))
    return correct / float(max(n_seen, 1))


test_mnist.__test__ = False               # not a pytest test


# ------------------------------------------------------------------------------------------------------------------
# CelebA consumers (celeba/loglikelihood.py:18-67, celeba/test.py:44-71)

def compute_nll_celeba(model, loader, image_only=False, attrs_only=False, n_samples=1, use_cuda=True, verbose=False):
    """-> (image NLL per sample, attribute NLL per sample), celeba/loglikelihood.py:18-67.

    Quirk kept out: the reference scores the attributes with ``F.nll_loss(recon_attrs (B,18), attrs (B,18) float,
    size_average=False)`` (:56), which no torch version accepts for a float target; the attribute decoder ends in a sigmoid and
    the training loss is a Bernoulli cross entropy (celeba/train.py:68-72), so the summed binary cross entropy is what is
    computed here."""
    return tuple(_reference_nll(model, loader, "celeba", _mode(image_only, attrs_only), n_samples, use_cuda, verbose))


@torch.no_grad()
def test_celeba(model, loader, use_cuda=True, verbose=True):
    """-> (joint, image-only, attribute-only) eval-mode losses averaged over the batches with kl_lambda = 1, celeba/test.py:44-71."""
    from .celeba import loss_function
    model.eval()
    sums, nb = [0.0, 0.0, 0.0], 0
    for image, attrs in loader:
        if use_cuda:
            image, attrs = image.cuda(), attrs.cuda()
        for k, kw in enumerate((dict(image=image, attrs=attrs), dict(image=image), dict(attrs=attrs))):
            recon_image, recon_attrs, mu, logvar = model(**kw)
            sums[k] += float(loss_function(mu, logvar, recon_x=recon_image, x=image, recon_y=recon_attrs, y=attrs,
                                           kl_lambda=1., lambda_x=1., lambda_y=1.))
        nb += 1
    out = tuple(s / max(nb, 1) for s in sums)
    if verbose:
        print('====> Test Epoch\tJoint loss: {:.4f}\tImage loss: {:.4f}\tAttrs loss:{:.4f}'.format(*out))
    return out


test_celeba.__test__ = False              # not a pytest test


# ------------------------------------------------------------------------------------------------------------------
# Importance-sampled marginal log-likelihood (the paper's evaluation: log p(x) and log p(y) with K particles per example,
# once for each posterior) on the HIP kernels of include/mmvae_hip.h: mmvae_iw_particles -> the model family's scoring call
# (mmvae_mm_iw_score, mmvae_mnist_iw_score) -> mmvae_iw_accumulate per particle chunk, mmvae_iw_finalize per batch.

IW_ROWS = 4096          # particle rows (examples x particles) per scoring call: the plan and workspace of one chunk
IW_ROWS_MNIST = 65536   # ... of the fused MNIST scorer: no plan or workspace per chunk, 32 rows per workgroup (2048 workgroups a call)
IW_ROWS_CELEBA = 512    # ... of the CelebA scorer: the one-pass workspace of a 512-row plan (mmvae_celeba_iw_workspace_bytes) stays below 1 GiB
IW_ROWS_COCO = 512      # ... of the COCO scorer (a multiple of 4): mmvae_coco_iw_workspace_bytes of a 512-row, 102-step plan (n_latents 100) is 214983680 bytes (205.0 MiB)
POSTERIORS = ("joint", "image", "text")


def iw_chunks(B, K, capacity):
    """Splits the B x K (example, particle) pairs of one batch into scoring calls of at most ``capacity`` rows:
    -> [(first_row, n_rows, first_particle, n_particles)], every pair covered exactly once.  All B rows go into one call
    when they fit (then the K particles are split into near-equal chunks); otherwise the rows are split into near-equal
    blocks too."""
    B, K, capacity = int(B), int(K), int(capacity)
    if B < 1 or K < 1 or capacity < 1:
        raise ValueError("iw_chunks: need B, K, capacity >= 1 (got %d, %d, %d)" % (B, K, capacity))
    nrb = -(-B // min(B, capacity))
    rb = -(-B // nrb)
    nkc = -(-K // (capacity // rb))
    kc = -(-K // nkc)
    return [(r0, min(rb, B - r0), k0, min(kc, K - k0)) for r0 in range(0, B, rb) for k0 in range(0, K, kc)]


class _Family:
    """The whole description of a model kind, for everything in this file:

    * ``cls``: the model class as "module.Class", imported on first use (``import evaluate`` stays light and acyclic);
    * the scoring call between particles and accumulate (``score``), the text decoder's steps T and classes V (words [rows][T][V]),
      the particle rows of one scoring call, and the scoring workspace as data: "mm" / "celeba" / "coco" ask
      mmvae_<api>_iw_workspace_bytes of the chunk's plan, "module" the state's ``module_workspace_bytes``, None needs none;
    * ``image_shape``: the layout of one image as the encoders and the NLL loop take it ((784,) for MNIST), ``picture``: the shape of
      one image a sampler returns ((1,28,28) for MNIST; else the same);
    * how to reach the encoders, decoders and experts on a model of the kind (``reach``): an attribute name, or a callable
      (model, input); ``captions``: the attribute of COCO's caption decoder (its ``sos``; its ``generate`` when sampling);
    * ``second_loss``: the mean-loss function (family, reconstruction, target) the reference's NLL uses for the second modality."""

    def __init__(self, name, cls, T, V, image_shape, rows, score, workspace, picture=None, encode_image=None, encode_second=None,
                 decode_image=None, decode_second=None, experts="experts", captions=None, second_loss=None, float_text=False,
                 image_only=False, text_only=False):
        self.name, self.cls, self.T, self.V, self.image_shape, self.rows = name, cls, T, V, image_shape, rows
        self.score, self.workspace, self.picture = score, workspace, picture or image_shape
        self.encode_image, self.encode_second, self.decode_image, self.decode_second = encode_image, encode_second, decode_image, decode_second
        self.experts, self.captions, self.second_loss = experts, captions, second_loss
        # text_only: a TextVAE baseline (coco): there is no image, the scoring call writes the caption term alone and the x / xy
        # columns of every result are NaN
        self.text_only = text_only
        # image_only: an ImageVAE baseline (celeba / coco): there is no second modality, the scoring call writes log p(x|z) alone
        # and the y / xy columns of every result are NaN
        self.image_only = image_only
        # float_text: the second modality is a float tensor (B, steps, 300) scored by a squared error (COCO captions), not int64
        # targets; the scoring call then also gets text / sos / sse / scale (``_coco_score``) and writes words = scale * sse
        self.float_text = float_text

    def module(self):
        return importlib.import_module("." + self.cls.split(".")[0], __package__)

    def model_class(self):
        return getattr(self.module(), self.cls.split(".")[1])

    def trainer(self):
        """The one-pass Trainer of a uni-modal kind (``test_imageonly`` / ``test_textonly``)."""
        return getattr(self.module(), "TextVAETrainer" if self.text_only else "ImageVAETrainer")

    def reach(self, model, role):
        """The callable of ``role`` ("encode_image", "encode_second", "decode_image", "decode_second", "experts", "captions")."""
        how = getattr(self, role)
        return getattr(model, how) if isinstance(how, str) else functools.partial(how, model)

    def workspace_bytes(self, st, rows):
        if self.workspace is None:
            return 0
        if self.workspace == "module":
            return st.module_workspace_bytes(rows)
        return call("mmvae_%s_iw_workspace_bytes" % self.workspace, st.plan(rows))


def _mm_score(st, rows, ws, ws_bytes, z, image, nr, nk, lx, words, stream):
    call("mmvae_mm_iw_score", st.plan(rows), ptr(ws), ws_bytes, ptr(z), ptr(image), nr, nk, ptr(lx), ptr(words), stream)


def _mnist_score(st, rows, ws, ws_bytes, z, image, nr, nk, lx, words, stream):
    call("mmvae_mnist_iw_score", st.plan(1), ptr(z), ptr(image), nr, nk, ptr(lx), ptr(words), stream)   # any bound plan: no row limit


def _celeba_score(st, rows, ws, ws_bytes, z, image, nr, nk, lx, words, stream):
    call("mmvae_celeba_iw_score", st.plan(rows), ptr(ws), ws_bytes, ptr(z), ptr(image), nr, nk, ptr(lx), ptr(words), stream)


def _coco_score(st, rows, ws, ws_bytes, z, image, nr, nk, lx, words, stream, text=None, sos=None, sse=None, scale=-0.5):
    """words [rows][1][1] = -sse / (2 sigma^2): the per-particle part of log p(y|z); the constant is added after finalize."""
    call("mmvae_coco_iw_score", st.plan(rows), ptr(ws), ws_bytes, ptr(z), ptr(image), ptr(text), ptr(sos), nr, nk, ptr(lx), ptr(sse), stream)
    torch.mul(sse[:rows], scale, out=words[:rows])


def _coco_text_score(st, rows, ws, ws_bytes, z, image, nr, nk, lx, words, stream, text=None, sos=None, sse=None, scale=-0.5):
    """The scoring call of a TextVAE: mmvae_coco_iw_score_text (the caption decoder and the squared error, no image decoder); log p(x|z) of
    the image that is not there is 0."""
    call("mmvae_coco_iw_score_text", st.plan(rows), ptr(ws), ws_bytes, ptr(z), ptr(text), ptr(sos), nr, nk, ptr(sse), stream)
    lx[:rows].zero_()
    torch.mul(sse[:rows], scale, out=words[:rows])


def _mmtext_score(st, rows, ws, ws_bytes, z, image, nr, nk, lx, words, stream):
    """The scoring call of a MultiMNIST TextVAE: mmvae_mmtext_iw_score (the text decoder alone, words [rows][4][12]); log p(x|z) of the
    image that is not there is 0."""
    call("mmvae_mmtext_iw_score", st.plan(rows), ptr(ws), ws_bytes, ptr(z), nr, nk, ptr(words), stream)
    lx[:rows].zero_()


def _mnist_image_score(st, rows, ws, ws_bytes, z, image, nr, nk, lx, words, stream):
    """The scoring call of a ``mnist.VAE``: mmvae_mnist_iw_score_image (the fused kernel without the label decoder); the words of its
    one dummy text position are 0."""
    call("mmvae_mnist_iw_score_image", st.plan(1), None, 0, ptr(z), ptr(image), nr, nk, ptr(lx), stream)   # any bound plan: no row limit
    words[:rows].zero_()


def _image_score(api):
    """The scoring call of an ImageVAE: mmvae_<family>_iw_score_image (decoder body + scoring tail, no second decoder); the words
    of its one dummy text position are 0."""
    def score(st, rows, ws, ws_bytes, z, image, nr, nk, lx, words, stream):
        call("mmvae_%s_iw_score_image" % api, st.plan(rows), ptr(ws), ws_bytes, ptr(z), ptr(image), nr, nk, ptr(lx), stream)
        words[:rows].zero_()
    return score


def coco_text_constant(steps, text_sigma):
    """-(steps * 300 / 2) log(2 pi sigma^2): the part of the Gaussian caption log-likelihood every particle shares (float64)."""
    import math
    text_sigma = float(text_sigma)
    if not text_sigma > 0 or not math.isfinite(text_sigma):
        raise ValueError("text_sigma must be a positive finite number (got %r)" % (text_sigma,))
    return -0.5 * int(steps) * 300 * math.log(2.0 * math.pi * text_sigma * text_sigma)


def _shift_text_terms(out, log_w, c):
    """Adds the constant c of log p(y|z) behind mmvae_iw_finalize: to the y and xy columns of log p^ (``out`` (B, 8): columns 1,
    2) and of log w (``log_w`` (B, K, 3) or None), and to the caption NLL (column 7, -c).  The same for every particle, so it
    commutes with the log-sum-exp; the ESS columns do not change."""
    out[:, 1:3] += c
    out[:, 7] -= c
    if log_w is not None:
        log_w[..., 1:3] += c


def _bce_rows(fam, recon, target):
    """The summed-over-a-row, averaged binary cross entropy of the reference's image (and CelebA attribute) term."""
    return _BCEMeanFn.apply(recon.reshape(target.shape[0], -1), target.reshape(target.shape[0], -1))


def _nll_rows(fam, recon, target):
    """``F.nll_loss`` of the log-softmax rows (B, V) or (B, T, V) against the targets (the module docstring's quirk)."""
    return _NLLMeanFn.apply(recon.reshape(-1, fam.V), target.reshape(-1))


_MULTIMODAL = dict(encode_image="image_encoder", encode_second="text_encoder", decode_image="decode_image", decode_second="decode_text")
_IMAGE_VAE = dict(encode_image="encoder", decode_image="decode", image_only=True)       # the same particle rows per call as the family
_TEXT_VAE = dict(encode_second="encoder", decode_second="decode", text_only=True)
_FAMILIES = {
    "multimnist": _Family("multimnist", "multimnist.MultimodalVAE", 4, 12, (1, 50, 50), IW_ROWS, _mm_score, "mm",
                          second_loss=_nll_rows, **_MULTIMODAL),
    "mnist": _Family("mnist", "mnist.MultimodalVAE", 1, 10, (784,), IW_ROWS_MNIST, _mnist_score, None, picture=(1, 28, 28),
                     second_loss=_nll_rows, **_MULTIMODAL),
    # the 18 attributes are 18 "text positions" of V = 2 classes: words [rows][18][2] = (log(1 - p), log p), targets 0 / 1
    "celeba": _Family("celeba", "celeba.MultimodalVAE", 18, 2, (3, 64, 64), IW_ROWS_CELEBA, _celeba_score, "celeba",
                      encode_image="image_encoder", encode_second=lambda model, t: model.attrs_encoder(t.float()),    # the (B,18) attributes as float
                      decode_image="image_decoder", decode_second="attrs_decoder", second_loss=_bce_rows),
    # the caption term goes through the accumulator as ONE position of ONE class: words [rows][1][1] = -SSE / (2 sigma^2), targets 0
    "coco": _Family("coco", "coco.MultimodalVAE", 1, 1, (3, 32, 32), IW_ROWS_COCO, _coco_score, "coco", captions="text_decoder",
                    float_text=True, **_MULTIMODAL),
    # the uni-modal baselines: the family's image half (its caption half) alone
    "celeba_image": _Family("celeba", "celeba.ImageVAE", 1, 1, (3, 64, 64), IW_ROWS_CELEBA, _image_score("celeba"), "celeba", **_IMAGE_VAE),
    "coco_image": _Family("coco", "coco.ImageVAE", 1, 1, (3, 32, 32), IW_ROWS_COCO, _image_score("coco"), "coco", **_IMAGE_VAE),
    "coco_text": _Family("coco", "coco.TextVAE", 1, 1, (3, 32, 32), IW_ROWS_COCO, _coco_text_score, "coco", captions="decoder",
                         float_text=True, **_TEXT_VAE),
    "multimnist_image": _Family("multimnist", "multimnist.ImageVAE", 1, 1, (1, 50, 50), IW_ROWS, _image_score("mm"), "mm", **_IMAGE_VAE),
    # (mnist.VAE's ``encoder`` is the bare Sequential: ``encode`` splits its output into mu, logvar)
    "mnist_image": _Family("mnist", "mnist.VAE", 1, 1, (784,), IW_ROWS_MNIST, _mnist_image_score, None, picture=(1, 28, 28),
                           **dict(_IMAGE_VAE, encode_image="encode")),
    # the MultiMNIST TextVAE: the text decoder alone on a plan of its own; its "image" is one dummy pixel
    "multimnist_text": _Family("multimnist", "multimnist.TextVAE", 4, 12, (1,), IW_ROWS, _mmtext_score, "module", **_TEXT_VAE),
}
IMAGE_ONLY_NAN_COLUMNS = (1, 2, 4, 5, 7)      # of mmvae_iw_finalize's (B, 8): everything that involves y
TEXT_ONLY_NAN_COLUMNS = (0, 2, 3, 5, 6)       # ... everything that involves x


def _family(model):
    """The entry of ``_FAMILIES`` whose class ``model`` is an instance of (a subclass or a padded-latent variant resolves alike);
    anything else is taken for a MultiMNIST model."""
    for fam in _FAMILIES.values():
        if isinstance(model, fam.model_class()):
            return fam
    return _FAMILIES["multimnist"]


def _posterior(posterior):
    """"attrs" (CelebA's name of the second modality) is a synonym of "text"."""
    return "text" if posterior == "attrs" else posterior


@torch.no_grad()
def iw_estimate(model, image, text, mu, logvar, n_particles, seed=0, first_row=0, particles_per_call=None, eps=None,
                return_z=False, return_log_w=False, text_sigma=1.0):
    """Importance-sampled log p(x), log p(y), log p(x, y) of one batch under the proposal q = N(mu, exp(logvar)).

    ``model``: a ``MultimodalVAE`` of one of the families below (its decoders run in eval mode); ``image``, ``text``, ``mu`` /
    ``logvar`` (B, n_latents), all on the GPU.

    Particles z_k = mu + exp(logvar/2) eps_k, k = 1..K, with eps keyed by (seed, first_row + example, particle, dimension) only, so
    a particle does not depend on the batch it comes in or on how the K particles are split into calls.  With
        log w_k^x = log p(x|z_k) + log p(z_k) - log q(z_k)       (y, xy alike)
    the estimate is log p^ = logsumexp_k(log w_k) - log K, a stochastic lower bound (K = 1: the one-sample ELBO), with the
    effective sample size (sum w)^2 / sum w^2.
    The reference's multimnist/loglikelihood.py (and ``compute_nll``) averages the reconstruction NLL over the particles
    instead: no prior / proposal ratio, no log-sum-exp, so it is not a bound on log p(x).  Its quantity is reported here as
    the by-product ``nll`` (mean over the particles of -log p(x|z), -log p(y|z); without the clamp).

    The families:
      * multimnist: ``image`` (B,1,50,50) float, ``text`` (B,4) int64.
        log p(x|z) = sum over the 2500 pixels of x*l - softplus(l) in fp32 from the decoder's pre-sigmoid logit l; it is NOT
        clamped at -100 like ``binary_cross_entropy`` (the two differ only where the decoder is confidently wrong).
        log p(y|z) = sum over the 4 positions of the text decoder's eval-mode log-softmax output at the target character,
        with the greedy feedback of its own argmax (the term ``loss_function`` trains, FILL positions included; not a
        teacher-forced likelihood).
      * mnist: ``image`` (B,784) (or anything that reshapes to it) and the labels ``text`` (B,) int64: one fused fp32 kernel scores
        its particles (mmvae_mnist_iw_score; 784 pixels, one text position of 10 classes, no greedy feedback), everything else is
        the same.
      * celeba: ``image`` (B,3,64,64) and the attributes ``text`` (B,18) with values 0 / 1 (any dtype; they are the int64
        targets): mmvae_celeba_iw_score runs the bf16 image decoder and scores 3x64x64 logits, log p(y|z) is the sum over the 18
        attributes of y*a - softplus(a) on the attribute decoder's fp32 logit a.  The result keys keep their names: the y / "text"
        columns are the attribute terms.
      * coco: ``image`` (B,3,32,32) and the captions ``text`` as floats (B, steps, 300) (``steps`` the model's):
        mmvae_coco_iw_score runs the bf16 image decoder and scores 3x32x32 logits, and runs the caption decoder in eval mode (its
        own output fed back, no dropout).  The reference trains captions with a mean squared error and defines no likelihood; the
        model under which that loss is the NLL up to scale is used:
        log p(y|z) = -SSE / (2 sigma^2) - (steps * 300 / 2) log(2 pi sigma^2) with sigma = ``text_sigma`` (the other families
        ignore it).  log p(y) and log p(x, y) of COCO therefore DEPEND ON sigma: compare checkpoints only at the same
        ``text_sigma``.  The kernels accumulate -SSE / (2 sigma^2) alone; the constant (about -28,119 at 102 steps and sigma = 1)
        is added to the y / xy columns of ``log_p`` and ``log_w`` and to the caption ``nll`` afterwards, so that fp32 keeps the
        digits of the per-particle terms.  ``return_log_w`` also returns ``sse`` (B, K) for this family.
      * an ``ImageVAE`` / ``TextVAE`` of a family: the modality it does not have is ignored (may be None), and every column that
        involves it is NaN.

    ``particles_per_call``: particles of one scoring call (default: as many as IW_ROWS rows allow; IW_ROWS_MNIST for MNIST).
    Test hooks: ``eps`` (B, K, n_latents) replaces the generator's draws; ``return_z`` adds z (B, K, n_latents), ``return_log_w`` log w
    (B, K, 3) (columns x, y, xy).
    -> dict of device tensors: ``log_p`` (B, 3) and ``ess`` (B, 3) (columns x, y, xy), ``nll`` (B, 2) (image, text)."""
    fam = _family(model)
    dev = mu.device
    st = model._core.sync(dev)
    B, D, K = int(mu.shape[0]), int(mu.shape[1]), int(n_particles)
    if K < 1:
        raise ValueError("n_particles must be >= 1")
    capacity = fam.rows if particles_per_call is None else B * int(particles_per_call)
    chunks = iw_chunks(B, K, capacity)
    rows_max = max(nr * nk for _, nr, _, nk in chunks)
    if fam.text_only:           # no image: ``image`` is ignored
        image = torch.zeros(B, int(np.prod(fam.image_shape)), dtype=torch.float32, device=dev) if image is None else image
    image = image.reshape(B, -1).contiguous().float()
    extra, sse_all, text_const = {}, None, 0.0
    if fam.image_only:
        text = torch.zeros(B, 1, dtype=torch.int64, device=mu.device)          # no second modality: ``text`` is ignored
    elif fam.float_text:
        steps = int(model.steps)
        text_const = coco_text_constant(steps, text_sigma)
        captions = text.contiguous().float()
        if tuple(captions.shape) != (B, steps, 300) or image.shape[1] != int(np.prod(fam.image_shape)):
            raise ValueError("iw_estimate: a coco model of %d steps takes images (B,3,32,32) and captions (B,%d,300) for its B = %d "
                             "proposals (got %s, %s)" % (steps, steps, B, tuple(image.shape), tuple(text.shape)))
        text = torch.zeros(B, 1, dtype=torch.int64, device=mu.device)          # the one "class" of the one caption position
        extra = dict(sos=fam.reach(model, "captions").sos.to(mu.device, torch.float32).contiguous(), scale=-0.5 / float(text_sigma) ** 2)
    else:
        text = text.contiguous().long()
    if image.shape[1] != int(np.prod(fam.image_shape)) or text.numel() != B * fam.T:
        raise ValueError("iw_estimate: a %s model takes images of %d pixels and %d target(s) per example (got %s, %s)" %
                         (fam.name, int(np.prod(fam.image_shape)), fam.T, tuple(image.shape), tuple(text.shape)))
    mu, logvar = mu.contiguous().float(), logvar.contiguous().float()
    if eps is not None:
        eps = eps.to(dev, torch.float32).reshape(B, K, D)
    f32 = dict(dtype=torch.float32, device=dev)
    ws_bytes = max(fam.workspace_bytes(st, nr * nk) for _, nr, _, nk in chunks)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    zbuf, lr, lx = torch.empty(rows_max * D, **f32), torch.empty(rows_max, **f32), torch.empty(rows_max, **f32)
    words = torch.empty(rows_max * fam.T * fam.V, **f32)
    state = torch.empty(B, 3, 4, **f32)
    z_all = torch.empty(B, K, D, **f32) if return_z else None
    lw_all = torch.empty(B, K, 3, **f32) if return_log_w else None
    if fam.float_text:
        extra["sse"] = torch.empty(rows_max, **f32)
        sse_all = torch.empty(B, K, **f32) if return_log_w else None
    stream = _ops.stream()
    call("mmvae_iw_init", ptr(state), B, stream)
    for r0, nr, k0, nk in chunks:
        rows = nr * nk
        e = None if eps is None else eps[r0:r0 + nr, k0:k0 + nk].contiguous()
        lwc = None if lw_all is None else torch.empty(nr, nk, 3, **f32)
        call("mmvae_iw_particles", ptr(mu[r0:]), ptr(logvar[r0:]), nr, D, nk, int(first_row) + r0, k0, int(seed) & (2 ** 64 - 1),
             ptr(e), ptr(zbuf), ptr(lr), stream)
        if fam.float_text:
            extra["text"] = captions[r0:]
        fam.score(st, rows, ws, ws_bytes, zbuf, image[r0:], nr, nk, lx, words, stream, **extra)
        call("mmvae_iw_accumulate", ptr(lx), ptr(words), ptr(text[r0:]), fam.T, fam.V, ptr(lr), nr, nk, ptr(state[r0:]), ptr(lwc), stream)
        if z_all is not None:
            z_all[r0:r0 + nr, k0:k0 + nk] = zbuf[:rows * D].view(nr, nk, D)
        if lw_all is not None:
            lw_all[r0:r0 + nr, k0:k0 + nk] = lwc
        if sse_all is not None:
            sse_all[r0:r0 + nr, k0:k0 + nk] = extra["sse"][:rows].view(nr, nk)
    out = torch.empty(B, 8, **f32)
    call("mmvae_iw_finalize", ptr(state), B, K, ptr(out), stream)
    if fam.float_text:
        _shift_text_terms(out, lw_all, text_const)
    if fam.image_only:          # an ImageVAE defines p(x) alone
        out[:, IMAGE_ONLY_NAN_COLUMNS] = float("nan")
        if lw_all is not None:
            lw_all[..., 1:3] = float("nan")
    if fam.text_only:           # a TextVAE defines p(y) alone
        out[:, TEXT_ONLY_NAN_COLUMNS] = float("nan")
        if lw_all is not None:
            lw_all[..., 0] = float("nan")
            lw_all[..., 2] = float("nan")
    res = {"log_p": out[:, 0:3], "ess": out[:, 3:6], "nll": out[:, 6:8]}
    if return_z:
        res["z"] = z_all
    if return_log_w:
        res["log_w"] = lw_all
        if sse_all is not None:
            res["sse"] = sse_all
    return res


def _posterior_of(model, fam, image, second, posterior):
    """(mu, logvar) of ``posterior`` ("joint", "image", "text" / "attrs") on a model of the kind ``fam``: the encoder of the one
    modality, or both encoders stacked image first, then the experts; a uni-modal model's own encoder is q itself (it has no
    experts).  No decoder runs."""
    posterior = _posterior(posterior)
    if fam.text_only:
        if posterior != "text":
            raise ValueError("a TextVAE has the text posterior alone: posterior must be \"text\" (got %r)" % (posterior,))
        return fam.reach(model, "encode_second")(second)
    if fam.image_only:
        if posterior != "image":
            raise ValueError("an ImageVAE has the image posterior alone: posterior must be \"image\" (got %r)" % (posterior,))
        return fam.reach(model, "encode_image")(image)
    if posterior not in POSTERIORS:
        raise ValueError("posterior must be one of %s (got %r)" % (POSTERIORS, posterior))
    parts = []
    if posterior != "text":
        parts.append(fam.reach(model, "encode_image")(image))
    if posterior != "image":
        parts.append(fam.reach(model, "encode_second")(second))
    return fam.reach(model, "experts")(torch.stack([p[0] for p in parts], dim=0), torch.stack([p[1] for p in parts], dim=0))


def _proposal(model, image, text, posterior):
    """(mu, logvar) of the eval-mode encoders + ProductOfExperts over the posterior's modalities (no decoder runs)."""
    fam = _family(model)
    if not fam.text_only:
        image = image.reshape(image.shape[0], *fam.image_shape)
    return _posterior_of(model, fam, image, text, posterior)


@torch.no_grad()
def log_marginal(model, loader, n_particles=1000, posterior="joint", seed=0, use_cuda=True, verbose=False, text_sigma=1.0):
    """Dataset means of the importance-sampled log p^(x), log p^(y), log p^(x, y) (``iw_estimate``) with the proposal of
    one posterior ("joint": q(z|x,y), "image": q(z|x), "text": q(z|y)), and of the two reconstruction NLLs.

    ``model``: a multimnist, mnist or celeba ``MultimodalVAE`` (``iw_estimate``; a CelebA loader yields (image, (B,18) attributes),
    ``posterior="attrs"`` is a synonym of "text", and ``log_py`` / ``text_nll`` are the attribute terms; a COCO loader yields
    (image, (B, steps, 300) float captions), and ``text_sigma`` is the sigma of its Gaussian caption likelihood, see ``iw_estimate``).  It runs in eval mode (BatchNorm running
    statistics, no dropout); per batch only the encoders and the experts run to form the proposal, then the particle chunks.  Nothing is read back to the host until the end.  Unlike the reference's
    multimnist/loglikelihood.py, the bounds weight each particle by p(z)/q(z) and take the log-sum-exp (see ``iw_estimate``);
    ``image_nll`` / ``text_nll`` are the reference's quantity (mean over particles of the summed reconstruction NLL), without
    its -100 clamp.
    -> dict: log_px, log_py, log_pxy, image_nll, text_nll (floats), n (examples), log_p (N, 3) and ess (N, 3) per example
    (CPU tensors, columns x, y, xy)."""
    if not use_cuda:
        raise ValueError("log_marginal runs on the GPU (the HIP kernels); there is no CPU path")
    posterior = _posterior(posterior)
    if posterior not in POSTERIORS:
        raise ValueError("posterior must be one of %s (got %r)" % (POSTERIORS, posterior))
    fam = _family(model)
    if fam.image_only and posterior != "image":
        raise ValueError("an ImageVAE has the image posterior alone: posterior must be \"image\" (got %r)" % (posterior,))
    if fam.text_only and posterior != "text":
        raise ValueError("a TextVAE has the text posterior alone: posterior must be \"text\" (got %r)" % (posterior,))
    model.eval()
    dev = next(model.parameters()).device
    logp, ess, nll, n_seen = [], [], [], 0
    for image, text in loader:
        image = None if fam.text_only else image.to(dev).float().reshape(-1, *fam.image_shape)      # (a TextVAE's loader may yield None there)
        text = None if fam.image_only else text.to(dev).float() if fam.float_text else text.to(dev).long()
        mu, logvar = _posterior_of(model, fam, image, text, posterior)
        r = iw_estimate(model, image, text, mu, logvar, n_particles, seed=seed, first_row=n_seen, text_sigma=text_sigma)
        logp.append(r["log_p"]); ess.append(r["ess"]); nll.append(r["nll"])
        n_seen += mu.shape[0]
        if verbose:
            print('Evaluating [{}]: {} examples'.format(posterior, n_seen))
    if n_seen == 0:
        raise ValueError("log_marginal: empty loader")
    logp, ess, nll = torch.cat(logp).cpu(), torch.cat(ess).cpu(), torch.cat(nll).cpu()
    m, mn = logp.double().mean(0), nll.double().mean(0)
    return {"log_px": m[0].item(), "log_py": m[1].item(), "log_pxy": m[2].item(), "image_nll": mn[0].item(),
            "text_nll": mn[1].item(), "n": n_seen, "log_p": logp, "ess": ess}


@torch.no_grad()
def marginal_table(model, loader, n_particles=1000, seed=0, text_sigma=1.0):
    """The paper's evaluation: log p^(x) and log p^(y) (plus log p^(x, y)) under each of the three posteriors, K particles
    per example.  -> {posterior: log_marginal(...) result} for "joint", "image", "text".  ``text_sigma``: COCO only."""
    return {post: log_marginal(model, loader, n_particles, post, seed=seed, text_sigma=text_sigma) for post in POSTERIORS}


# ------------------------------------------------------------------------------------------------------------------
# multimnist/sample.py:59-144 as a function and a script: `python -m multimodal_vae_amd.evaluate sample model.pth.tar ...`

def _sample_latents(vae, fam, n_samples, image, second, dev, seed=None):
    """z (n_samples, n_latents) on ``dev`` for the samplers: the prior (image = second = None: the one-element mu = 0, std = 1) or the
    posterior of what is given (``_posterior_of``), then ONE host-side draw -- from the global generator, or from a generator of
    its own when ``seed`` is given -- made after the encoders ran, moved to the device and combined as z * std + mu."""
    vae.eval()
    if image is None and second is None:
        mu, std = torch.zeros(1, device=dev), torch.ones(1, device=dev)
    else:
        posterior = "text" if image is None else "image" if second is None else "joint"
        mu, logvar = _posterior_of(vae, fam, None if image is None else image.to(dev), None if second is None else second.to(dev), posterior)
        std = logvar.mul(0.5).exp()
    z = torch.randn(n_samples, vae.n_latents, generator=None if seed is None else torch.Generator().manual_seed(seed)).to(dev)
    return (z * std.expand_as(z) + mu.expand_as(z)).contiguous()


def _pictures(fam, vae, z):
    """The image decoder's samples on the host, (n, *the family's picture shape)."""
    return fam.reach(vae, "decode_image")(z).cpu().view(z.shape[0], *fam.picture)


@torch.no_grad()
def sample(vae, n_samples=64, image=None, text=None, use_cuda=True):
    """Unconditional (image = text = None) or conditional generation: (image samples (n,1,50,50), token samples (n,4) LongTensor).
    ``image``: (1,1,50,50) float in [0,1]; ``text``: (1,4) LongTensor (utils.char_tensor) -- multimnist/sample.py:80-130."""
    fam = _FAMILIES["multimnist"]
    z = _sample_latents(vae, fam, n_samples, image, text, torch.device("cuda") if use_cuda else torch.device("cpu"))
    return _pictures(fam, vae, z), torch.max(fam.reach(vae, "decode_second")(z).cpu(), dim=2)[1]


@torch.no_grad()
def sample_textonly(vae, n_samples=64, text=None):
    """``sample`` for a multimnist ``TextVAE``: token samples (n,4) LongTensor, from the prior or from q(z|y) of ``text`` (1,4)."""
    fam = _FAMILIES["multimnist_text"]
    z = _sample_latents(vae, fam, n_samples, None, text, next(vae.parameters()).device)
    return torch.max(fam.reach(vae, "decode_second")(z).cpu(), dim=2)[1]


@torch.no_grad()
def sample_imageonly(vae, n_samples=64, image=None):
    """``sample`` for a multimnist ``ImageVAE``: image samples (n,1,50,50), from the prior or from q(z|x) of ``image`` (1,1,50,50); for
    a ``mnist.VAE`` (mnist/imageonly/sample_imageonly.py:58-83) samples (n,1,28,28), ``image`` (1,784)."""
    fam = _family(vae)
    return _pictures(fam, vae, _sample_latents(vae, fam, n_samples, image, None, next(vae.parameters()).device))


@torch.no_grad()
def sample_coco(vae, n_samples=64, image=None, text=None, stop_at_eos=False, seed=None):
    """multimnist/sample.py:80-130 for the COCO family: prior samples (image = text = None) or samples of the conditional
    posterior -> (images (n,3,32,32) float on the host, n caption strings).  ``image``: (1,3,32,32) float in [0,1]; ``text``:
    (1,102,300) caption vectors (``WordTable.embed``).  ``vae`` carries the word table (``MultimodalVAE(..., words=)``)."""
    fam = _family(vae)                          # a TextVAE: captions alone (the images are None), conditioned on a caption at most
    if fam.text_only and image is not None:
        raise ValueError("sample_coco: a TextVAE cannot be conditioned on an image")
    z = _sample_latents(vae, fam, n_samples, image, text, next(vae.parameters()).device, seed)
    return None if fam.text_only else _pictures(fam, vae, z), fam.reach(vae, "captions").generate(z, stop_at_eos=stop_at_eos)


@torch.no_grad()
def sample_celeba(vae, n_samples=64, image=None, attrs=None, seed=None):
    """celeba/sample.py:73-137, its four modes: prior samples (image = attrs = None) or samples of the posterior given an image, given
    attributes, or given both (product of experts) -> (images (n,3,64,64) float on the host, n lists of attribute names).
    ``image``: (1,3,64,64) float in [0,1]; ``attrs``: (1,18) float (``celeba.attrs_from_names``)."""
    from .celeba import tensor_to_attributes
    fam = _FAMILIES["celeba"]
    z = _sample_latents(vae, fam, n_samples, image, attrs, next(vae.parameters()).device, seed)
    return _pictures(fam, vae, z), [tensor_to_attributes(row) for row in fam.reach(vae, "decode_second")(z).cpu()]


def fetch_celeba_image(path, attr_str, seed=0):
    """What celeba/sample.py:18-41 means to do: a random image (seeded) among those of the dataset file ``path`` (``make_celeba``) that
    have the attribute -> (1,3,64,64) float in [0,1]."""
    from .celeba import attrs_from_names
    col = int(attrs_from_names([attr_str]).view(-1).nonzero()[0])           # (one name; an unknown or not-kept one is refused)
    x, a = load_celeba_eval_file(path)
    rows = (a[:, col] == 1).nonzero().view(-1)
    if len(rows) == 0:
        raise ValueError("%s: no image has the attribute %s" % (path, attr_str))
    pick = int(rows[int(torch.randint(len(rows), (1,), generator=torch.Generator().manual_seed(seed)))])
    return x[pick:pick + 1].float().div(255.0)


@torch.no_grad()
def sample_pixelcnn(model, n_samples=64, height=None, width=None, complete=None, rows=0, seed=0):
    """Images from a ``pixelcnn.PixelCNN`` / ``GatedPixelCNN`` on the device, in one launch of the incremental sampler
    (``pixelcnn.generate``) -> float32 (n_samples, C, H, W) in [0, 1].  ``complete`` (C, H, W) or (N, C, H, W) uint8: every sample
    keeps the first ``rows`` rows of (its) image, quantised to the model's levels, and draws the rest."""
    from . import pixelcnn as PX
    height = height or getattr(model, "height", None) or 28
    width = width or getattr(model, "width", None) or height
    given, n_given = None, 0
    if complete is not None:
        im = torch.as_tensor(complete)
        if im.dtype != torch.uint8 or im.dim() not in (3, 4) or tuple(im.shape[-3:]) != (model.data_channels, height, width):
            raise ValueError("sample_pixelcnn: --complete must be uint8 (%d, %d, %d) (got %s %s)"
                             % (model.data_channels, height, width, im.dtype, tuple(im.shape)))
        if not 0 <= rows <= height:
            raise ValueError("sample_pixelcnn: rows = %d, need 0..%d" % (rows, height))
        im = im.view(-1, model.data_channels, height, width)
        lev = torch.from_numpy(PX.quantisize(im.float().div(255.0).numpy(), model.out_dims)).long()
        given = lev.expand(n_samples, -1, -1, -1) if lev.shape[0] == 1 else lev[:n_samples]
        if given.shape[0] != n_samples:
            raise ValueError("sample_pixelcnn: %d images to complete for %d samples" % (given.shape[0], n_samples))
        given, n_given = given.contiguous().to(model.conv4.weight.device), rows * width
    return PX.generate(model, n_samples, height, width, seed=seed, given=given, n_given=n_given).image


@torch.no_grad()
def nll_pixelcnn(model, images_u8, batch_size=32, head="torch"):
    """Exact negative log-likelihood of uint8 images (N, C, H, W) under a ``pixelcnn.PixelCNN`` / ``GatedPixelCNN``, on the model's
    device.  The images are preprocessed as ``train_pixelcnn`` does (quantised to the model's levels); ``head="hip"`` evaluates the
    output head and the cross entropy in the fused forward kernel (``pixelcnn.head_nll``, device-only), ``"torch"`` runs anywhere.
    Prints the reference's test line (the mean over elements) and the mean per image in nats and bits/dim with standard errors ->
    {"per_image_nll", "nll_mean", "nll_se", "bits_per_dim", "bits_per_dim_se", "loss", "n", "head"}."""
    from . import pixelcnn as PX
    from .train_pixelcnn import preprocess
    PX.check_head(model, head, "nll_pixelcnn")
    im = torch.as_tensor(images_u8)
    if im.dtype != torch.uint8 or im.dim() != 4 or im.shape[0] < 1 or im.shape[1] != model.data_channels:
        raise ValueError("nll_pixelcnn: images must be uint8 (N, %d, H, W) with N >= 1 (got %s %s)"
                         % (model.data_channels, im.dtype, tuple(im.shape)))
    size = (getattr(model, "height", None), getattr(model, "width", None))
    if None not in size and tuple(im.shape[2:]) != size:
        raise ValueError("nll_pixelcnn: images are %d x %d, the checkpoint was trained on %d x %d" % (tuple(im.shape[2:]) + size))
    model.eval()
    dev = model.conv4.weight.device
    x = preprocess(im.cpu(), model.out_dims)
    per_image = []
    for k in range(0, x.shape[0], batch_size):
        per_image.append(PX.nll(model, x[k:k + batch_size].to(dev), head=head).double().flatten(1).sum(dim=1).cpu())
    per_image = torch.cat(per_image)
    n, dims = int(per_image.shape[0]), int(im.shape[1] * im.shape[2] * im.shape[3])
    mean = float(per_image.mean())
    se = float(per_image.std(unbiased=True) / n ** 0.5) if n > 1 else 0.0
    ln2 = float(np.log(2.0))
    out = {"per_image_nll": per_image.tolist(), "nll_mean": mean, "nll_se": se, "bits_per_dim": mean / (dims * ln2),
           "bits_per_dim_se": se / (dims * ln2), "loss": mean / dims, "n": n, "head": head}
    print('====> Test Epoch\tLoss: {:.4f}'.format(out["loss"]))
    print('NLL per image over {} images: {:.4f} +- {:.4f} nats\t{:.5f} +- {:.5f} bits/dim'.format(
        n, mean, se, out["bits_per_dim"], out["bits_per_dim_se"]))
    return out


@torch.no_grad()
def latent_mmd(vae, loader, seed=0):
    """MMD between the aggregate posterior of an ``coco.InfoVAE`` and its prior: encodes every image of ``loader`` (batches of
    (B,3,32,32) floats in [0,1], or tuples whose first entry is one) in eval mode (z = mu), draws as many N(0, I) samples from
    ``seed`` and compares the two sets in ONE call of the fused MMD op (``mmd.mmd_terms``; 10,000 x 10,000 pairs need no
    (N, N, D) tensor).  Prints and returns {"n", "k_prior", "k_posterior", "k_cross", "mmd"}: the means of k(prior, prior),
    k(z, z), k(prior, z) and MMD = k_prior + k_posterior - 2 k_cross.  A model whose ``encode`` returns z itself (``mnist.InfoVAE``,
    batches of (B,1,28,28)) is taken as it is; when such a model lives on the CPU the three means are torch ops."""
    from .mmd import mmd_terms
    vae.eval()
    dev = next(vae.parameters()).device
    zs = []
    for batch in loader:
        x = batch[0] if isinstance(batch, (tuple, list)) else batch
        enc = vae.encode(x.to(dev).float())
        zs.append((enc if torch.is_tensor(enc) else enc[0]).clone())          # (mu, logvar) or z itself
    z = torch.cat(zs).contiguous()
    prior = torch.randn(z.shape[0], z.shape[1], generator=torch.Generator().manual_seed(seed)).to(dev)
    if dev.type == "cuda":
        t = mmd_terms(prior, z).cpu().tolist()
    else:
        from .mnist import mmd_terms_torch
        t = [float(v) for v in mmd_terms_torch(prior, z)]
    out = {"n": int(z.shape[0]), "k_prior": t[0], "k_posterior": t[1], "k_cross": t[2], "mmd": t[3]}
    print('Latent MMD over {} examples: k(prior, prior) {:.6f}\tk(z, z) {:.6f}\tk(prior, z) {:.6f}\tMMD {:.6f}'.format(
        out["n"], out["k_prior"], out["k_posterior"], out["k_cross"], out["mmd"]))
    return out


@torch.no_grad()
def manifold(vae, loader, pca_only=False, perplexity=40, n_iter=300, seed=0):
    """mnist/manifold.py: encodes every (image, label) batch of ``loader`` with ``gen_latents`` in eval mode (z = mu of the joint
    posterior; for a ``mnist.VAE``, mnist/imageonly/manifold_imageonly.py, the encoder's ``mu`` of the image) and reduces the latents to 2-D: ``tsne.pca(., 2)`` with ``pca_only``, else ``tsne.tsne`` (exact t-SNE on the GPU,
    perplexity 40 and 300 iterations as the reference asks of sklearn) after ``pca(., 50)`` when n_latents > 50.  Returns CPU tensors
    {"latents" (N, n_latents), "labels" (N,), "embedding" (N, 2), "kl_trace" (n_iter,) or None with ``pca_only``}: the KL of every
    iteration, before its update."""
    from .tsne import pca, tsne
    vae.eval()
    dev = next(vae.parameters()).device
    fam = _family(vae)
    zs, labels = [], []
    for image, text in loader:
        x = image.to(dev).float().reshape(-1, *fam.image_shape)
        z = fam.reach(vae, "encode_image")(x)[0] if fam.image_only else vae.gen_latents(x, text.to(dev))
        zs.append(z.float().clone())
        labels.append(text.cpu())
    latents, labels = torch.cat(zs).contiguous(), torch.cat(labels)
    kl_trace = None
    if pca_only:
        embedding = pca(latents, 2)[0]
    else:
        z = pca(latents, 50)[0] if latents.shape[1] > 50 else latents
        embedding, kl_trace = tsne(z, perplexity=perplexity, n_iter=n_iter, seed=seed, return_trace=True)
        kl_trace = kl_trace.cpu()
    return {"latents": latents.cpu(), "labels": labels, "embedding": embedding.cpu(), "kl_trace": kl_trace}


def array2d_string(A):
    """mnist/latent_viz.py:20-21"""
    return '\n'.join([''.join(['{:4}'.format(item) for item in row]) for row in A])


@torch.no_grad()
def latent_viz(vae, nx=20, ny=20, lim=3.0):
    """mnist/latent_viz.py for a model with a 2-D latent: decodes the grid linspace(-lim, lim, nx) x linspace(-lim, lim, ny) in ONE
    batched call of each decoder.  Returns (canvas (28 ny, 28 nx), digits (ny, nx)), both on the CPU, in the reference's
    orientation: grid row i holds the latents (x_j, y_i); the canvas shows row i in its (ny - 1 - i)-th band of 28 pixel rows (the
    second latent grows upwards), ``digits[i, j]`` is the arg-max label of that point.  The HIP plan has no 2-latent size: the
    decoders run on ``mnist.with_padded_latents(vae)``, the same functions with two extra latents held at zero."""
    from .mnist import with_padded_latents
    if vae.n_latents != 2:
        raise ValueError("latent_viz: the model has n_latents = %d: the grid needs a 2-D latent" % vae.n_latents)
    dec = with_padded_latents(vae).eval()
    dev = next(dec.parameters()).device
    xs, ys = torch.linspace(-lim, lim, nx), torch.linspace(-lim, lim, ny)
    z = torch.zeros(nx * ny, dec.n_latents)
    z[:, 0], z[:, 1] = xs.repeat(ny), ys.repeat_interleave(nx)                                  # row i * nx + j = (x_j, y_i)
    z = z.to(dev)
    image = dec.decode_image(z).float().reshape(ny, nx, 28, 28).cpu()
    digits = dec.decode_text(z).argmax(dim=1).reshape(ny, nx).cpu()
    canvas = image.flip(0).permute(0, 2, 1, 3).reshape(28 * ny, 28 * nx).contiguous()
    return canvas, digits


# ------------------------------------------------------------------------------------------------------------------
# the command line

def _add_modes(p, image_help, second, second_help):
    """The posterior trio: --image_only | --<second>_only | --all."""
    mode = p.add_mutually_exclusive_group()
    mode.add_argument('--image_only', action='store_true', default=False, help=image_help)
    mode.add_argument('--%s_only' % second, action='store_true', default=False, help=second_help)
    mode.add_argument('--all', action='store_true', default=False, help='all three posteriors (the paper\'s table)')


def _add_source(p, data_help, synthetic_help, default=None, metavar='FILE.pt'):
    """--data | --synthetic N."""
    src = p.add_mutually_exclusive_group()
    src.add_argument('--data', type=str, default=default, metavar=metavar, help=data_help)
    src.add_argument('--synthetic', type=int, default=0, metavar='N', help=synthetic_help)


def _add_sos_words(p):
    tab = p.add_mutually_exclusive_group()
    tab.add_argument('--sos', type=str, default=None, metavar='FILE.pt', help="the 300 floats of GloVe('<s>') (default: sos.pt of --data)")
    tab.add_argument('--words', type=str, default=None, metavar='TABLE.pt', help="word table file (coco.save_word_table) that has '<s>'")


def _add_seed_json(p, seed_help, json_help='write the bounds to this file'):
    p.add_argument('--seed', type=int, default=0, help=seed_help)
    p.add_argument('--json', type=str, default=None, help=json_help)


def _parser():
    import argparse
    parser = argparse.ArgumentParser(prog="python -m multimodal_vae_amd.evaluate")
    sub = parser.add_subparsers(dest="cmd", required=True)
    ps = sub.add_parser("sample", help="multimnist/sample.py")
    ps.add_argument('model_path', type=str, help='path to trained model file.')
    ps.add_argument('--n_samples', type=int, default=64, help='Number of images and texts to sample.')
    ps.add_argument('--dataset', choices=('multimnist', 'mnist'), default='multimnist',
                    help='mnist: a checkpoint of train_imageonly --dataset mnist (mnist/imageonly/sample_imageonly.py)')
    ps.add_argument('--condition_on_image', type=str, default=None,
                    help='a .pt file holding a (50,50) uint8 or float image; mnist: a digit LABEL, an image of which is drawn from --data')
    ps.add_argument('--data', type=str, default=None, metavar='FILE.pt', help='mnist: (uint8 images (N,28,28), int64 labels (N,))')
    ps.add_argument('--seed', type=int, default=0, help='mnist: seed of the choice of the image')
    ps.add_argument('--condition_on_text', type=str, default=None, help='a digit string of at most 4 characters')
    ps.add_argument('--out', type=str, default='./results')
    # multimnist/loglikelihood.py's flags and defaults, plus the importance-sampled bounds (log_marginal / marginal_table)
    pl = sub.add_parser("loglik", help="multimnist/loglikelihood.py + importance-sampled log p(x), log p(y)")
    pl.add_argument('model_path', type=str, help='path to trained model file')
    pl.add_argument('--dataset', type=str, default='multimnist', choices=('multimnist', 'mnist'),
                    help='model family of the checkpoint (mnist: --data names a .pt file of (uint8 images (N,28,28), int64 labels (N,)))')
    _add_modes(pl, 'compute NLL of test data using reconstructions from image only',
               'text', 'compute NLL of test data using reconstructions from text only')
    pl.add_argument('--n_samples', type=int, default=100, help='number of samples to use to estimate the ELBO')
    pl.add_argument('--cuda', action='store_true', default=False, help='accepted for compatibility: the kernels run on the GPU')
    pl.add_argument('--batch_size', type=int, default=64)
    _add_source(pl, 'folder of the MultiMNIST test file', 'N synthetic MultiMNIST-shaped examples instead of files', './data', None)
    _add_seed_json(pl, 'seed of the particles')
    # celeba/loglikelihood.py's flags and defaults, plus the ones `loglik` adds
    pc = sub.add_parser("loglik_celeba", help="celeba/loglikelihood.py + importance-sampled log p(x), log p(y)")
    pc.add_argument('model_path', type=str, help='path to trained model file')
    _add_modes(pc, 'compute NLL of test data using reconstructions from image only',
               'attrs', 'compute NLL of test data using reconstructions from attributes only')
    pc.add_argument('--n_samples', type=int, default=100, help='number of samples to use to estimate the ELBO')
    pc.add_argument('--cuda', action='store_true', default=False, help='accepted for compatibility: the kernels run on the GPU')
    pc.add_argument('--batch_size', type=int, default=64)
    _add_source(pc, 'a .pt file of (uint8 images (N,3,64,64), attributes (N,18) with values 0 / 1)',
                'N synthetic CelebA-shaped examples instead of a file')
    _add_seed_json(pc, 'seed of the particles')
    # the flags of `loglik` for a checkpoint of train_coco; the '<s>' vector is not in the checkpoint
    pk = sub.add_parser("loglik_coco", help="importance-sampled log p(x), log p(y) for a checkpoint of train_coco")
    pk.add_argument('model_path', type=str, help='path to a checkpoint written by train_coco')
    _add_sos_words(pk)
    _add_modes(pk, 'proposal from the image only', 'text', 'proposal from the caption only')
    pk.add_argument('--n_samples', type=int, default=100, help='particles per example')
    pk.add_argument('--batch_size', type=int, default=64)
    pk.add_argument('--text_sigma', type=float, default=1.0,
                    help='sigma of the Gaussian caption likelihood; log p(y) depends on it (default: 1.0)')
    _add_source(pk, 'folder with images_u8.pt, captions.pt (and sos.pt), as train_coco reads',
                'N synthetic COCO-shaped examples instead of files', metavar='DIR')
    _add_seed_json(pk, 'seed of the particles (and of the synthetic examples)')
    pt = sub.add_parser("test_imageonly", help="celeba/test_imageonly.py: eval-mode loss (kl_lambda = 1) of a train_imageonly checkpoint")
    pt.add_argument('model_path', type=str)
    pt.add_argument('--dataset', choices=('celeba', 'coco', 'multimnist', 'mnist'), default='celeba')
    pt.add_argument('--data', type=str, default='',
                    help='celeba: FILE.pt of make_celeba; coco: DIR with images_u8.pt; multimnist: root of processed/test.pt; '
                         'mnist: FILE.pt of (uint8 images (N,28,28), int64 labels (N,)); its loss is (BCE + KLD / 784) / B')
    pt.add_argument('--synthetic', type=int, default=0, metavar='N')
    pt.add_argument('--batch_size', type=int, default=128, metavar='N')
    pt.add_argument('--seed', type=int, default=0)
    px = sub.add_parser("test_textonly", help="eval-mode loss (kl_lambda = 1) of a train_textonly checkpoint, as test_imageonly")
    px.add_argument('model_path', type=str)
    px.add_argument('--dataset', choices=('coco', 'multimnist'), default='coco',
                    help='multimnist: a checkpoint of train_textonly_multimnist; --data is then the folder of the MultiMNIST test file')
    px.add_argument('--data', type=str, default='', help='DIR with captions.pt (and sos.pt), as train_coco reads')
    px.add_argument('--synthetic', type=int, default=0, metavar='N')
    px.add_argument('--batch_size', type=int, default=64, metavar='N')
    px.add_argument('--seed', type=int, default=0)
    _add_sos_words(px)
    # multimnist/sample.py's flags for a checkpoint of train_coco; the captions are decoded through a word table
    pw = sub.add_parser("sample_coco", help="multimnist/sample.py for the COCO family: images + captions decoded to words")
    pw.add_argument('model_path', type=str, help='path to a checkpoint written by train_coco')
    tab = pw.add_mutually_exclusive_group(required=True)
    tab.add_argument('--words', type=str, default=None, metavar='TABLE.pt', help='word table file (coco.save_word_table)')
    tab.add_argument('--synthetic_words', type=int, default=0, metavar='V', help='a synthetic table of V words instead of a file')
    pw.add_argument('--n_samples', type=int, default=64, help='Number of images and captions to sample.')
    pw.add_argument('--condition_on_image', type=str, default=None, metavar='FILE.pt', help='a .pt file holding a (3,32,32) uint8 or float image')
    pw.add_argument('--condition_on_text', type=str, default=None, help='a caption, e.g. "a man riding a wave"')
    pw.add_argument('--stop_at_eos', action='store_true', default=False, help="cut every caption in front of its first '</s>'")
    pw.add_argument('--out', type=str, default='./results')
    pw.add_argument('--seed', type=int, default=0, help='seed of the latent samples (and of the synthetic table)')
    # celeba/sample.py's flags for a checkpoint of train_celeba
    pa = sub.add_parser("sample_celeba", help="celeba/sample.py: images + attribute names from a CelebA checkpoint")
    pa.add_argument('model_path', type=str, help='path to a checkpoint written by train_celeba')
    pa.add_argument('--n_samples', type=int, default=64, help='Number of images and texts to sample.')
    pa.add_argument('--condition_on_image', type=str, default=None, metavar='ATTR',
                    help='generate conditioned on a random image of --data that has this attribute')
    pa.add_argument('--data', type=str, default=None, metavar='FILE.pt', help='a dataset file of make_celeba (for --condition_on_image)')
    pa.add_argument('--condition_on_attrs', type=str, default=None, metavar='NAME[,NAME]', help='generate conditioned on these attributes')
    pa.add_argument('--out', type=str, default='./results')
    pa.add_argument('--seed', type=int, default=0, help='seed of the latent samples and of the image choice')
    # images from a checkpoint of train_pixelcnn, in one launch of the incremental sampler
    pp = sub.add_parser("sample_pixelcnn", help="images from a PixelCNN / GatedPixelCNN checkpoint of train_pixelcnn")
    pp.add_argument('model_path', type=str, help='path to a checkpoint written by train_pixelcnn')
    pp.add_argument('--n_samples', type=int, default=64, help='Number of images to sample.')
    pp.add_argument('--height', type=int, default=None, help="(default: the checkpoint's, else 28)")
    pp.add_argument('--width', type=int, default=None, help="(default: the checkpoint's, else the height)")
    pp.add_argument('--complete', type=str, default=None, metavar='FILE.pt', help='a uint8 image (C,H,W) whose first --rows rows are kept')
    pp.add_argument('--rows', type=int, default=0, metavar='R', help='rows of --complete to keep')
    pp.add_argument('--seed', type=int, default=0, help='seed of the uniforms')
    pp.add_argument('--out', type=str, default='./results')
    # exact log-likelihood of images under a checkpoint of train_pixelcnn
    pn = sub.add_parser("nll_pixelcnn", help="exact NLL per image and bits/dim for a PixelCNN / GatedPixelCNN checkpoint")
    pn.add_argument('model_path', type=str, help='path to a checkpoint written by train_pixelcnn')
    _add_source(pn, 'a .pt file of uint8 images (N,C,H,W)', 'N synthetic images instead of a file')
    pn.add_argument('--batch_size', type=int, default=32)
    pn.add_argument('--head', choices=('torch', 'hip'), default='torch',
                    help='conv4 + cross entropy as torch ops or as the fused HIP head (hip needs --cuda; default: torch)')
    pn.add_argument('--cuda', action='store_true', default=False, help='evaluate on the GPU (default: False)')
    _add_seed_json(pn, 'seed of the synthetic images', 'write the result to this file')
    # aggregate posterior against the prior for a checkpoint of train_infovae
    pm = sub.add_parser("latent_mmd", help="MMD between the encoded test images and the prior, for a checkpoint of train_infovae")
    pm.add_argument('model_path', type=str, help='path to a checkpoint written by train_infovae (mnist: train_infovae_mnist)')
    pm.add_argument('--dataset', type=str, default='coco', choices=('coco', 'mnist'),
                    help='model family of the checkpoint (mnist: uint8 images (N,28,28), alone or as the first entry of a tuple)')
    pm.add_argument('--conv_backend', choices=('torch', 'hip'), default='torch', help='mnist: what the convolutions run on (default: torch)')
    _add_source(pm, 'a .pt file of uint8 images (N,3,32,32)', 'N synthetic images of the family\'s shape instead of a file')
    pm.add_argument('--batch_size', type=int, default=500)
    _add_seed_json(pm, 'seed of the prior samples (and of the synthetic images)', 'write the terms to this file')
    # mnist/manifold.py: the test set's latents reduced to 2-D by PCA or by exact t-SNE on the GPU
    pf = sub.add_parser("manifold", help="mnist/manifold.py: latents of the test set, PCA or PCA + t-SNE to 2-D")
    pf.add_argument('model_path', type=str, help='path to trained model file (mnist family; a train_imageonly checkpoint embeds the encoder\'s mu)')
    pf.add_argument('--pca_only', action='store_true', default=False)
    pf.add_argument('--perplexity', type=float, default=40.0)
    pf.add_argument('--n_iter', type=int, default=300)
    _add_source(pf, 'a .pt file of (uint8 images (N,28,28), int64 labels (N,))', 'N synthetic MNIST-shaped examples instead of a file')
    pf.add_argument('--batch_size', type=int, default=128)
    pf.add_argument('--seed', type=int, default=0, help='seed of the initial embedding (and of the synthetic images)')
    pf.add_argument('--out', type=str, default='./results')
    # mnist/latent_viz.py: the decoders over a grid of a 2-D latent
    pv = sub.add_parser("latent_viz", help="mnist/latent_viz.py: decodes a 20 x 20 grid of a 2-D latent")
    pv.add_argument('model_path', type=str, help='path to trained model file (mnist family, n_latents = 2)')
    pv.add_argument('--out', type=str, default='./results')
    return parser


def load_celeba_eval_file(path):
    """The ``--data`` file of ``loglik_celeba``: (uint8 images (N,3,64,64), attributes (N,18)) -> (uint8 images, float32
    attributes).  Attributes other than 0 / 1 are refused here, on the host: the scorer indexes (log(1 - p), log p) with them."""
    x, a = torch.load(path, weights_only=False)
    x, a = torch.as_tensor(x), torch.as_tensor(a)
    if x.dtype != torch.uint8 or x.dim() != 4 or tuple(x.shape[1:]) != (3, 64, 64):
        raise ValueError("%s: images must be uint8 (N,3,64,64) (got %s %s)" % (path, x.dtype, tuple(x.shape)))
    if a.dim() != 2 or a.shape[0] != x.shape[0] or a.shape[1] != 18:
        raise ValueError("%s: attributes must be (N,18) for the N = %d images (got %s)" % (path, x.shape[0], tuple(a.shape)))
    a = a.float()
    if not bool(((a == 0) | (a == 1)).all()):
        raise ValueError("%s: every attribute must be 0 or 1" % path)
    return x, a


def check_coco_eval_data(images, captions, text_sigma=1.0, where="loglik_coco"):
    """The host-side refusals of ``loglik_coco``: images must be uint8 (N,3,32,32), captions float (N,102,300) for the same N >= 1,
    sigma > 0.  -> (uint8 images, float32 captions)."""
    from .coco import MAX_WORDS, N_EMBEDDING
    coco_text_constant(MAX_WORDS, text_sigma)                     # refuses sigma <= 0 / non-finite
    x, t = torch.as_tensor(images), torch.as_tensor(captions)
    if x.dtype != torch.uint8 or x.dim() != 4 or tuple(x.shape[1:]) != (3, 32, 32) or x.shape[0] < 1:
        raise ValueError("%s: images must be uint8 (N,3,32,32) with N >= 1 (got %s %s)" % (where, x.dtype, tuple(x.shape)))
    if not t.is_floating_point() or t.dim() != 3 or tuple(t.shape) != (x.shape[0], MAX_WORDS, N_EMBEDDING):
        raise ValueError("%s: captions must be float (N,%d,%d) for the N = %d images (got %s %s)"
                         % (where, MAX_WORDS, N_EMBEDDING, x.shape[0], t.dtype, tuple(t.shape)))
    return x, t.float()


def _eval_data(dataset, args, where, hint="--data FILE.pt", parts="xt"):
    """The one reader of evaluation data: ``--synthetic N`` (seeded by ``--seed``) or ``--data`` of "mnist" (a .pt file of (images,
    labels), or of the images alone), "multimnist" (the folder of the test file), "celeba" (a file of ``make_celeba``) or "coco" (a
    folder of images_u8.pt, captions.pt, sos.pt, read for the ``parts`` "x" / "t" the command uses; or the images' own .pt file).
    -> (uint8 images or None, second modality or None, extras: COCO's {"sos": the data's '<s>' vector}), after the shape and dtype
    refusals the command ``where`` makes."""
    import os
    from . import data as D
    load = functools.partial(torch.load, weights_only=False)
    n, path, extras = getattr(args, "synthetic", 0), args.data, {}
    if n <= 0 and not path:
        raise SystemExit("%s: give %s or --synthetic N" % (where, hint))
    if dataset == "mnist":
        f = D.synthetic_mnist(n, seed=args.seed) if n > 0 else load(path)      # (torchvision's processed/test.pt)
        x, t = (torch.as_tensor(v) for v in f) if isinstance(f, (tuple, list)) else (torch.as_tensor(f), None)
    elif dataset == "multimnist":
        if n > 0:
            from .utils import charlist_tensor
            x, labels = D.synthetic_multimnist(n, seed=args.seed)
            t = torch.stack([charlist_tensor(l) for l in labels])
        else:
            x, t = D.load_multimnist(path, train=False)
    elif dataset == "celeba":
        x, t = D.synthetic_celeba(n, seed=args.seed) if n > 0 else load_celeba_eval_file(path)
    else:
        x = t = None
        if n > 0:
            from .train_coco import synthetic_coco
            x, t, extras["sos"] = synthetic_coco(n, seed=args.seed)
        else:
            if "x" in parts:
                x = torch.as_tensor(load(os.path.join(path, "images_u8.pt") if os.path.isdir(path) else path))
            if "t" in parts:
                t = torch.as_tensor(load(os.path.join(path, "captions.pt")))
                if not args.sos and not args.words:
                    extras["sos"] = load(os.path.join(path, "sos.pt"))
    if where == "loglik_coco":
        x, t = check_coco_eval_data(x, t, args.text_sigma)
    elif where == "latent_mmd":
        shape = (28, 28) if dataset == "mnist" else (3, 32, 32)
        if x.dtype != torch.uint8 or tuple(x.shape[1:]) != shape:
            raise ValueError("latent_mmd: images must be uint8 (N,%s) (got %s %s)" % (",".join(map(str, shape)), x.dtype, tuple(x.shape)))
    elif where == "manifold":
        if x.dtype != torch.uint8 or tuple(x.shape[1:]) != (28, 28) or t is None or t.shape != x.shape[:1]:
            raise ValueError("manifold: need uint8 images (N,28,28) and N labels (got %s %s, %s)"
                             % (x.dtype, tuple(x.shape), None if t is None else tuple(t.shape)))
    return (x if "x" in parts else None), (t if "t" in parts else None), extras


def _batches(x, t, batch_size, whole_only=False):
    """[(rows of x, rows of t)] in batches of ``batch_size`` (either tensor may be None).  ``whole_only``: batches of one size, at most
    the whole set (the plans of ``test_imageonly`` / ``test_textonly`` take a fixed batch size); a trailing partial batch is dropped."""
    n = (t if x is None else x).shape[0]
    bs = min(batch_size, n) if whole_only else batch_size
    return [(None if x is None else x[i:i + bs], None if t is None else t[i:i + bs])
            for i in range(0, n - bs + 1 if whole_only else n, bs)]


def _sos_words(args, sos, where):
    """``--sos`` / ``--words`` over the '<s>' vector that came with the data -> (sos or None, word table or None)."""
    from . import coco as K
    words = None
    if args.sos:
        sos = torch.load(args.sos, weights_only=False)
    elif args.words:
        sos, words = None, K.load_word_table(args.words)
    if sos is not None:
        sos = torch.as_tensor(sos)
        if sos.numel() != K.N_EMBEDDING or not sos.is_floating_point():
            raise ValueError("%s: the '<s>' vector must be %d floats (got %s %s)" % (where, K.N_EMBEDDING, sos.dtype, tuple(sos.shape)))
    return sos, words


def _state_dict_keys(path):
    return list(torch.load(path, map_location='cpu', weights_only=False)['state_dict'].keys())


def _unimodal_keys(keys):
    return len(keys) > 0 and all(k.startswith(("encoder.", "decoder.")) for k in keys)


def _kind_of(keys):
    """"text" / "image" / "multimodal" from the keys of a ``state_dict``.  Text-only is asked BEFORE image-only, whose prefixes a
    text-only checkpoint shares."""
    return "text" if "encoder.gru.weight_ih_l0" in keys else "image" if _unimodal_keys(keys) else "multimodal"


def is_imageonly_checkpoint(path):
    """True for a checkpoint of ``train_imageonly`` (or the reference's train_imageonly.py): every key of its ``state_dict`` starts
    with ``encoder.`` or ``decoder.``."""
    return _unimodal_keys(_state_dict_keys(path))


def is_textonly_checkpoint(path):
    """True for a checkpoint of ``train_textonly`` (or the reference's train_textonly.py): its ``state_dict`` has the caption encoder's
    ``encoder.gru.weight_ih_l0``.  Asked BEFORE ``is_imageonly_checkpoint``, whose prefixes a text-only checkpoint shares."""
    return _kind_of(_state_dict_keys(path)) == "text"


_LOADERS = {          # (dataset, kind of checkpoint) -> "module.function": the combinations that exist
    ("mnist", "multimodal"): "mnist.load_checkpoint", ("mnist", "image"): "mnist.load_checkpoint_imageonly",
    ("multimnist", "multimodal"): "train.load_checkpoint", ("multimnist", "image"): "multimnist.load_checkpoint_imageonly",
    ("multimnist", "text"): "multimnist.load_checkpoint_textonly",
    ("celeba", "multimodal"): "celeba.load_checkpoint", ("celeba", "image"): "celeba.load_checkpoint_imageonly",
    ("coco", "multimodal"): "coco.load_checkpoint", ("coco", "image"): "coco.load_checkpoint_imageonly",
    ("coco", "text"): "coco.load_checkpoint_textonly",
}


def _loader(dataset, kind):
    if (dataset, kind) not in _LOADERS:
        raise SystemExit("there is no %s model of the %s family: the checkpoint belongs to another --dataset or command" % (
            {"multimodal": "multimodal", "image": "image-only", "text": "text-only"}[kind], dataset))
    module, fn = _LOADERS[dataset, kind].split(".")
    return getattr(importlib.import_module("." + module, __package__), fn)


def _open_checkpoint(dataset, path, use_cuda=True, **kw):
    """-> (model, kind) of a checkpoint of ``dataset``'s drivers, kind "multimodal" / "image" / "text": the file is read once to tell
    (``_kind_of``), then by the ``load_checkpoint*`` of that kind.  ``kw``: COCO's ``sos`` / ``words`` (an image-only model has neither)."""
    kind = _kind_of(_state_dict_keys(path))
    return _loader(dataset, kind)(path, use_cuda=use_cuda, **({} if kind == "image" else kw)), kind


def _which_posteriors(args, kind="multimodal"):
    """--all / --image_only / --text_only (--attrs_only) -> the posteriors to report; a uni-modal checkpoint has its own alone."""
    if kind != "multimodal":
        return (kind,)
    if args.all:
        return POSTERIORS
    second_only = getattr(args, "text_only", False) or getattr(args, "attrs_only", False)
    return ("image",) if args.image_only else ("text",) if second_only else ("joint",)


def _write_json(path, out):
    import json
    if path:
        with open(path, 'w') as fp:
            json.dump(out, fp, indent=1)


def _write_samples(out_dir, image=None, lines=None, text_file='sample_text.txt'):
    """sample_image.pt (no torchvision here: the tensor, not a PNG grid) and one line of text per sample, whichever there is."""
    import os
    os.makedirs(out_dir, exist_ok=True)                           # (the reference calls the non-existent os.mkdirs, sample.py:133)
    if image is not None:
        torch.save(image, os.path.join(out_dir, 'sample_image.pt'))
    if lines is not None:
        with open(os.path.join(out_dir, text_file), 'w') as fp:
            for line in lines:
                fp.write('%s\n' % line)


def _latent_mmd_main(args):
    x, _, _ = _eval_data(args.dataset, args, "latent_mmd", parts="x")
    x = x.float().div_(255.0)                                     # transforms.ToTensor()
    if args.dataset == "mnist":
        from .mnist import load_infovae_checkpoint, set_infovae_backend
        x = x.unsqueeze(1)
        vae = set_infovae_backend(load_infovae_checkpoint(args.model_path, use_cuda=True), args.conv_backend)
    else:
        from .train_infovae import load_checkpoint
        vae = load_checkpoint(args.model_path, use_cuda=True)
    out = latent_mmd(vae, _batches(x, None, args.batch_size), seed=args.seed)
    _write_json(args.json, out)
    return out


def _manifold_main(args):
    import os
    x, t, _ = _eval_data("mnist", args, "manifold")
    x, t = x.float().div_(255.0).view(-1, 784), t.long()          # transforms.ToTensor() + view(-1, 784)
    vae, _ = _open_checkpoint("mnist", args.model_path)           # (a checkpoint of train_imageonly --dataset mnist: the encoder's mu)
    out = manifold(vae, _batches(x, t, args.batch_size), pca_only=args.pca_only, perplexity=args.perplexity, n_iter=args.n_iter, seed=args.seed)
    os.makedirs(args.out, exist_ok=True)
    torch.save(out, os.path.join(args.out, 'manifold.pt'))
    if out["kl_trace"] is not None:
        print('t-SNE over {} latents: KL {:.4f} -> {:.4f} in {} iterations'.format(
            out["latents"].shape[0], float(out["kl_trace"][0]), float(out["kl_trace"][-1]), out["kl_trace"].shape[0]))
    try:                                                          # the figure is optional: matplotlib may not be installed
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.cm as cm
        import matplotlib.pyplot as plt
    except ImportError:
        return out
    plt.figure()
    emb, lab = out["embedding"].numpy(), out["labels"].numpy()
    for i, color in enumerate(cm.rainbow(np.linspace(0, 1, 10))):
        plt.scatter(emb[lab == i, 0], emb[lab == i, 1], color=color, label=str(i), alpha=0.3, edgecolors='none')
    plt.legend()
    plt.savefig(os.path.join(args.out, 'manifold.png'))
    plt.close()
    return out


def _latent_viz_main(args):
    import os
    if _kind_of(_state_dict_keys(args.model_path)) == "image":
        raise SystemExit("latent_viz: an image-only checkpoint is not supported (the grid needs a padded-latent variant of mnist.VAE)")
    vae = _loader("mnist", "multimodal")(args.model_path, use_cuda=True)
    canvas, digits = latent_viz(vae)
    os.makedirs(args.out, exist_ok=True)
    torch.save(canvas, os.path.join(args.out, 'latent_viz_image.pt'))
    with open(os.path.join(args.out, 'latent_viz_text.txt'), 'w') as fp:
        fp.write(array2d_string(digits.tolist()))
    return canvas, digits


def _nll_pixelcnn_main(args):
    from .pixelcnn import load_checkpoint
    from .train_pixelcnn import synthetic_images
    if args.head == 'hip' and not (args.cuda and torch.cuda.is_available()):
        raise SystemExit('--head hip runs on the GPU only: pass --cuda on a machine with a gfx950 device (there is no CPU fallback)')
    use_cuda = args.cuda and torch.cuda.is_available()
    model = load_checkpoint(args.model_path, use_cuda=False)
    if args.synthetic > 0:
        if model.height is None:
            raise SystemExit("nll_pixelcnn: the checkpoint records no image size: give --data FILE.pt")
        width = model.width or model.height                                            # (square images, cropped to the checkpoint's size)
        x = synthetic_images(args.synthetic, model.data_channels, max(model.height, width), args.seed)[:, :, :model.height, :width].contiguous()
    elif args.data:
        x = torch.as_tensor(torch.load(args.data, weights_only=False))
    else:
        raise SystemExit("nll_pixelcnn: give --data FILE.pt or --synthetic N")
    # (the images are checked against the checkpoint on the CPU, before anything is uploaded)
    size = (model.height, model.width)
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[0] < 1 or x.shape[1] != model.data_channels or (
            None not in size and tuple(x.shape[2:]) != size):
        raise SystemExit("nll_pixelcnn: images must be uint8 (N, %d, %s, %s) (got %s %s)"
                         % (model.data_channels, size[0] or 'H', size[1] or 'W', x.dtype, tuple(x.shape)))
    if use_cuda:
        model.cuda()
    out = nll_pixelcnn(model, x, args.batch_size, args.head)
    _write_json(args.json, out)
    return out


def _sample_pixelcnn_main(args):
    from .pixelcnn import load_checkpoint
    model = load_checkpoint(args.model_path, use_cuda=True)
    complete = torch.load(args.complete, weights_only=False) if args.complete else None
    image = sample_pixelcnn(model, args.n_samples, args.height, args.width, complete, args.rows, args.seed)
    _write_samples(args.out, image.cpu())
    return image


def _condition_image(path, *shape):
    """``--condition_on_image FILE.pt``: a uint8 or float image -> (1, *shape) float in [0,1]."""
    im = torch.load(path)
    return (im.float() / 255.0 if im.dtype == torch.uint8 else im.float()).view(1, *shape)


def _sample_coco_main(args):
    from . import coco as K, data as D
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.synthetic_words > 0:
        words = K.WordTable(*D.synthetic_word_table(args.synthetic_words, seed=args.seed), device=dev)
    else:
        words = K.load_word_table(args.words, dev)
    kind = _kind_of(_state_dict_keys(args.model_path))            # "text": a checkpoint of train_textonly, captions only
    if kind == "text" and args.condition_on_image:
        raise SystemExit("sample_coco: a text-only checkpoint cannot be conditioned on an image")
    vae = _loader("coco", "text" if kind == "text" else "multimodal")(args.model_path, use_cuda=True, words=words)
    image = _condition_image(args.condition_on_image, 3, 32, 32) if args.condition_on_image else None
    text = words.embed(args.condition_on_text).unsqueeze(0) if args.condition_on_text else None
    image_recon, captions = sample_coco(vae, args.n_samples, image, text, stop_at_eos=args.stop_at_eos, seed=args.seed)
    _write_samples(args.out, image_recon, captions)
    return captions


def _sample_celeba_main(args):
    from .celeba import attrs_from_names
    image = attrs = None
    if args.condition_on_attrs:
        attrs = attrs_from_names(args.condition_on_attrs)         # (refuses an unknown name before anything is loaded)
    if args.condition_on_image:
        if not args.data:
            raise SystemExit("sample_celeba: --condition_on_image ATTR needs --data FILE.pt to take the image from")
        image = fetch_celeba_image(args.data, args.condition_on_image, seed=args.seed)
    vae = _loader("celeba", "multimodal")(args.model_path, use_cuda=True)
    image_recon, names = sample_celeba(vae, args.n_samples, image, attrs, seed=args.seed)
    _write_samples(args.out, image_recon, [','.join(row) for row in names], 'sample_attrs.txt')
    return image_recon, names


def _report(vae, loader, posts, args, second, text_sigma=None):
    """Runs ``log_marginal`` per posterior, prints the reference's NLL line and the bounds, writes ``--json`` (``text_sigma``: the
    COCO command's, recorded in the file)."""
    table = {}
    for post in posts:
        r = log_marginal(vae, loader, n_particles=args.n_samples, posterior=post, seed=args.seed,
                         text_sigma=1.0 if text_sigma is None else text_sigma)
        table[post] = r
        mess = r["ess"].double().mean(0)
        print('\nTest Image NLL: {:.4f}\tTest {} NLL: {:.4f}'.format(r["image_nll"], second, r["text_nll"]))
        print('[{} posterior, K = {}] log p(x) >= {:.4f}\tlog p(y) >= {:.4f}\tlog p(x,y) >= {:.4f}\t'
              'mean ESS x / y / xy: {:.2f} / {:.2f} / {:.2f}'.format(post, args.n_samples, r["log_px"], r["log_py"], r["log_pxy"],
                                                                    *mess.tolist()))
    if args.json:
        out = {"n_samples": args.n_samples, "n_examples": table[posts[0]]["n"], "seed": args.seed}
        if text_sigma is not None:
            out["text_sigma"] = text_sigma
        for post, r in table.items():
            out[post] = {k: r[k] for k in ("log_px", "log_py", "log_pxy", "image_nll", "text_nll")}
            out[post]["mean_ess"] = r["ess"].double().mean(0).tolist()
        _write_json(args.json, out)
    return table


@torch.no_grad()
def _test_unimodal(vae, batches, kl_lambda, verbose, where):
    """The mean over the batches (whole batches of one size, already on the device) of the eval-mode loss of the kind's one-pass Trainer."""
    trainer_class = _family(vae).trainer()
    vae.eval()
    trainer, total, n = None, 0.0, 0
    for batch in batches:
        if trainer is None or trainer.engine.B != batch.shape[0]:
            trainer = trainer_class(vae, batch.shape[0], kl_lambda=kl_lambda)
        total += float(trainer.evaluate(batch).losses()[0].item())
        n += 1
    if n == 0:
        raise ValueError("%s: empty loader" % where)
    total /= n
    if verbose:
        print('====> Test set loss: {:.4f}'.format(total))
    return total


def test_textonly(vae, loader, kl_lambda=1.0, verbose=True):
    """The counterpart of ``test_imageonly`` for a ``TextVAE``: the mean over the batches of the eval-mode loss MSE + kl_lambda * KL / B
    (``kl_lambda`` = 1), on the one-pass caption step (a multimnist ``TextVAE``: (B, 4) int64 labels, lambda_y * NLL + kl_lambda * KL / B).
    ``loader`` yields (anything, captions (B, steps, 300)) whole batches of one size."""
    dev, dtype = next(vae.parameters()).device, torch.float32 if _family(vae).float_text else torch.int64
    return _test_unimodal(vae, (text.to(dev, dtype).contiguous() for _, text in loader), kl_lambda, verbose, "test_textonly")


test_textonly.__test__ = False            # not a pytest test


def test_imageonly(vae, loader, kl_lambda=1.0, verbose=True):
    """celeba/test_imageonly.py: the mean over the batches of the eval-mode loss BCE + kl_lambda * KL / B of an ``ImageVAE``
    (``kl_lambda`` = 1 there), on the one-pass step.  ``loader`` yields (image, anything) whole batches of one size."""
    dev = next(vae.parameters()).device
    return _test_unimodal(vae, (image.to(dev).float().contiguous() for image, _ in loader), kl_lambda, verbose, "test_imageonly")


test_imageonly.__test__ = False           # not a pytest test


def _loglik(args, dataset, second="Text", hint="--data FILE.pt"):
    """The body of `loglik`, `loglik_celeba` and `loglik_coco`: the data, then the checkpoint (multimodal: the posteriors the flags
    name; a checkpoint of train_imageonly / train_textonly: log p(x) / log p(y) alone), then ``_report``.  The result keys (and the
    JSON layout) are the same for all three; CelebA's ``log_py`` / ``text_nll`` are the attribute terms and its attribute-only
    posterior is filed under "text"; COCO adds ``text_sigma``."""
    kw, text_sigma = {}, None
    if dataset == "coco":
        from .coco import MAX_WORDS
        text_sigma = float(args.text_sigma)
        coco_text_constant(MAX_WORDS, text_sigma)                 # before anything is loaded
    x, t, extras = _eval_data(dataset, args, args.cmd, hint)
    if dataset == "coco":
        kw["sos"], kw["words"] = _sos_words(args, extras.get("sos"), args.cmd)
    loader = _batches(x.float().div_(255.0), t, args.batch_size)                 # transforms.ToTensor(); log_marginal shapes the batches
    vae, kind = _open_checkpoint(dataset, args.model_path, **kw)
    return _report(vae, loader, _which_posteriors(args, kind), args, second, text_sigma=text_sigma)


def _loglik_main(args):
    return _loglik(args, args.dataset)


def _loglik_celeba_main(args):
    return _loglik(args, "celeba", "Attrs")


def _loglik_coco_main(args):
    return _loglik(args, "coco", hint="--data DIR")


def _test_imageonly_main(args):
    """`test_imageonly`: whole batches only (the plan takes a fixed batch size); a trailing partial batch is dropped."""
    x, _, _ = _eval_data(args.dataset, args, "test_imageonly", "--data", parts="x")
    x = x.float().div_(255.0).view(-1, *_FAMILIES[args.dataset + "_image"].picture)
    kl_lambda = 1.0 / 784 if args.dataset == "mnist" else 1.0     # mnist: the reference's own loss, (BCE + KLD / 784) / B
    vae = _loader(args.dataset, "image")(args.model_path, use_cuda=True)
    return test_imageonly(vae, _batches(x, None, args.batch_size, whole_only=True), kl_lambda=kl_lambda)


def _test_textonly_main(args):
    """`test_textonly`: whole batches only (the plan takes a fixed batch size); a trailing partial batch is dropped."""
    _, t, extras = _eval_data(args.dataset, args, "test_textonly", "--data", parts="t")
    kw = dict(zip(("sos", "words"), _sos_words(args, extras.get("sos"), "test_textonly"))) if args.dataset == "coco" else {}
    vae = _loader(args.dataset, "text")(args.model_path, use_cuda=True, **kw)
    return test_textonly(vae, _batches(None, t, args.batch_size, whole_only=True))


def _sample_mnist_main(args):
    """`sample --dataset mnist` (mnist/imageonly/sample_imageonly.py): 64 images from the prior, or from q(z|x) of a test image of the
    digit ``--condition_on_image LABEL`` chosen from ``--data``.  Writes sample_image.pt (n,1,28,28)."""
    if _kind_of(_state_dict_keys(args.model_path)) != "image":
        raise SystemExit("sample --dataset mnist: an image-only checkpoint (train_imageonly --dataset mnist) expected")
    image = None
    if args.condition_on_image is not None:
        label = int(args.condition_on_image)
        if not args.data:
            raise SystemExit("sample --dataset mnist: --condition_on_image LABEL needs --data FILE.pt")
        x, t, _ = _eval_data("mnist", args, "sample --dataset mnist")
        idx = (t == label).nonzero().flatten()
        if idx.numel() == 0:
            raise SystemExit("sample --dataset mnist: --data has no image of the digit %d" % label)
        pick = idx[int(torch.randint(0, idx.numel(), (1,), generator=torch.Generator().manual_seed(args.seed)))]
        image = x[pick].float().div(255.0).view(1, 784)
    image_recon = sample_imageonly(_loader("mnist", "image")(args.model_path, use_cuda=True), args.n_samples, image)
    _write_samples(args.out, image_recon)
    return image_recon


def _sample_main(args):
    """`sample`: a multimodal checkpoint of MultiMNIST, or one of train_imageonly --dataset multimnist (image samples only) or of
    train_textonly_multimnist (text samples only); `--dataset mnist`: ``_sample_mnist_main``."""
    from .utils import char_tensor, tensor_to_string
    if args.dataset == "mnist":
        return _sample_mnist_main(args)
    vae, kind = _open_checkpoint("multimnist", args.model_path)
    if kind == "text" and args.condition_on_image:
        raise SystemExit("sample: a text-only checkpoint has no image encoder")
    if kind == "image" and args.condition_on_text:
        raise SystemExit("sample: an image-only checkpoint has no text encoder")
    image = _condition_image(args.condition_on_image, 1, 50, 50) if args.condition_on_image else None
    text = char_tensor(args.condition_on_text).unsqueeze(0) if args.condition_on_text else None
    if kind == "text":
        image_recon, text_recon = None, sample_textonly(vae, args.n_samples, text)
    elif kind == "image":
        image_recon, text_recon = sample_imageonly(vae, args.n_samples, image), None
    else:
        image_recon, text_recon = sample(vae, args.n_samples, image, text)
    _write_samples(args.out, image_recon, None if text_recon is None else [tensor_to_string(row) for row in text_recon])


_COMMANDS = {
    "sample": _sample_main, "loglik": _loglik_main, "loglik_celeba": _loglik_celeba_main, "loglik_coco": _loglik_coco_main,
    "test_imageonly": _test_imageonly_main, "test_textonly": _test_textonly_main, "sample_coco": _sample_coco_main,
    "sample_celeba": _sample_celeba_main, "sample_pixelcnn": _sample_pixelcnn_main, "nll_pixelcnn": _nll_pixelcnn_main,
    "latent_mmd": _latent_mmd_main, "manifold": _manifold_main, "latent_viz": _latent_viz_main,
}


def _main(argv=None):
    args = _parser().parse_args(argv)
    return _COMMANDS[args.cmd](args)


main = _main


if __name__ == "__main__":
    _main()
