"""Drop-in Python face of the reference's ``coco/model.py`` + ``loss_function`` (coco/train.py:66-84).

Same class names, constructor arguments, ``forward`` signatures (``vae(image=, text=)``) and ``state_dict`` keys as the
reference.  ``nn.*`` children are parameter containers only; every module forward/backward is a call into
libmmvae_hip.so.  No CPU fallback.  ``FusedTrainer`` = the train() closure body (coco/train.py:138-173) as one enqueue.

GloVe: the reference looks up exactly one vector at run time, ``GloVe('<s>')``, the decoder's first input
(coco/model.py:271-272; the ``</s>`` pre-fill of :275-277 is overwritten at every position).  It is passed in as ``sos``
(300 floats) and kept as a non-persistent buffer, so ``state_dict()`` has the reference's keys.  ``generate_vector`` is
``forward``.

Words: ``WordTable`` is the reference's ``coco/glove.py`` (``get_word``, ``closest``, ``closest_batch``, ``analogy``) over any
``(V, 300)`` float32 table, with the search on the device: one fused fp32 MFMA sweep + arg-min per call (csrc/nn_words.hip),
equal distances resolved to the LOWEST index (the reference's ``torch.sort(...)[1][0]`` leaves ties open).  A model built with
``words=`` decodes captions to strings in ``generate``; the table is neither a parameter nor a buffer, so ``state_dict()`` is
unchanged.  ``embed`` is ``coco/utils.py:36-47`` with ``str.split`` as the tokenizer (nltk is not a dependency: punctuation
stays attached to its word, a deliberate difference).  The table file is one ``.pt`` holding ``(float32 (V,300), list[str])``
(``save_word_table`` / ``load_word_table``; INTEGRATION.md shows the conversion from torchtext's GloVe cache).

InfoVAE: ``InfoVAE`` (coco/model.py:358-382) is ``ImageEncoder`` + ``ImageDecoder`` + ``reparametrize`` under the reference's
``encoder.`` / ``decoder.`` keys; ``infovae_loss`` is ``coco/train_infovae.py:44-55`` (mean BCE + MMD against prior samples) with
the MMD term on the fused op of ``mmd.py``; ``compute_mmd`` / ``compute_kernel`` are re-exported from there.  ``FusedInfoVAE`` is the
same model on ONE core (the construction of ``ImageVAE``), which ``InfoVAETrainer`` steps in one enqueue with the MMD sweep beside the
decoder (core.FusedInfoVAEStep); the two classes load each other's state dicts.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from ._lib import MMVAEError, call, ptr
from ._ops import geometry, stream as _stream
from .core import CocoState, FusedCocoStep, FusedImageStep, FusedInfoVAEStep, FusedTextStep, Trainer, load_vae_checkpoint
from .mmd import compute_kernel, compute_mmd, mmd_terms  # noqa: F401  (coco/model.py:385-402)
from .modules import (DECODER, Draw, ExpertsVAEBase, ProductOfExperts, Swish, VAEBase, _BCEMeanFn, _Core, _dropout_on, _KLSumFn, _MSEMeanFn,
                      _seed_from_torch, run_module)
from .modules import DROP_P, swish  # noqa: F401  (public names of this module)

MAX_WORDS = 102       # coco/utils.py:12-15
N_EMBEDDING = 300
N_HIDDENS = 200
SOS, EOS = '<s>', '</s>'   # coco/utils.py:13-14
MAX_DISTS = 8              # queries of one mmvae_nn_words_dists call


def nn_words_geometry() -> Tuple[int, int, int]:
    """(query rows per workgroup, words per vocabulary tile, largest number of vocabulary splits) of the search kernels."""
    return geometry("mmvae_nn_words_geometry", 3)


class WordTable:
    """``coco/glove.py``'s ``GloVe`` over a caller-supplied table: ``vectors`` (V, 300) float32, ``itos`` V distinct strings.
    Keeps the device copy of the table, its squared row norms (computed once, on the device), ``itos`` and ``stoi``.
    ``device=None`` keeps a host-only table: lookups (``get_word``, ``embed``) work, a search raises (there is no CPU search)."""

    def __init__(self, vectors: torch.Tensor, itos: Sequence[str], device=None):
        vectors = torch.as_tensor(vectors)
        if vectors.dim() != 2 or vectors.shape[1] != N_EMBEDDING or vectors.shape[0] < 1:
            raise MMVAEError("WordTable: vectors must be (V, %d) with V >= 1 (got %s)" % (N_EMBEDDING, tuple(vectors.shape)))
        if vectors.dtype != torch.float32:
            raise MMVAEError("WordTable: vectors must be float32 (got %s)" % vectors.dtype)
        itos = list(itos)
        if len(itos) != vectors.shape[0]:
            raise MMVAEError("WordTable: %d words for %d vectors" % (len(itos), vectors.shape[0]))
        if not all(isinstance(w, str) for w in itos):
            raise MMVAEError("WordTable: every word must be a str")
        stoi = {w: i for i, w in enumerate(itos)}
        if len(stoi) != len(itos):
            raise MMVAEError("WordTable: duplicate words (%d distinct of %d)" % (len(stoi), len(itos)))
        if not bool(torch.isfinite(vectors).all()):
            raise MMVAEError("WordTable: non-finite vector entries")
        self.itos, self.stoi = itos, stoi
        self.device = None if device is None else torch.device(device)
        self.vectors = vectors.detach().contiguous() if self.device is None else vectors.detach().to(self.device).contiguous()
        self.sqnorm = None
        if self.device is not None:
            if self.device.type != "cuda":
                raise MMVAEError("WordTable: the search runs on a gfx950 GPU only (device=None keeps a host-only table)")
            self.sqnorm = torch.empty(len(itos), dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                call("mmvae_nn_words_norms", ptr(self.vectors), len(itos), N_EMBEDDING, ptr(self.sqnorm), _stream())

    def __len__(self):
        return len(self.itos)

    def get_word(self, word: str) -> Optional[torch.Tensor]:
        """coco/glove.py:21-24: the word's vector (on the table's device), or None."""
        i = self.stoi.get(word)
        return None if i is None else self.vectors[i]

    def _queries(self, vecs: torch.Tensor) -> torch.Tensor:
        if self.device is None:
            raise MMVAEError("WordTable: a host-only table cannot search (build it with device=); there is no CPU fallback")
        vecs = torch.as_tensor(vecs)
        if vecs.dim() != 2 or vecs.shape[1] != N_EMBEDDING or vecs.shape[0] < 1:
            raise MMVAEError("WordTable: queries must be (N, %d) with N >= 1 (got %s)" % (N_EMBEDDING, tuple(vecs.shape)))
        return vecs.detach().to(device=self.device, dtype=torch.float32).contiguous()

    @torch.no_grad()
    def nearest(self, vecs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(N, 300) -> (index int64 (N,), dist float32 (N,)) device tensors: per row the nearest word (lowest index among equally
        near ones) and its Euclidean distance.  The result of a row does not depend on the rows it is batched with."""
        q = self._queries(vecs)
        n, v = q.shape[0], len(self.itos)
        index = torch.empty(n, dtype=torch.int64, device=self.device)
        dist = torch.empty(n, dtype=torch.float32, device=self.device)
        wsb = call("mmvae_nn_words_workspace_bytes", n, v)
        ws = torch.empty(wsb, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            call("mmvae_nn_words_nearest", ptr(q), n, ptr(self.vectors), ptr(self.sqnorm), v, N_EMBEDDING, ptr(ws), wsb,
                 ptr(index), ptr(dist), _stream())
        return index, dist

    @torch.no_grad()
    def dists(self, vecs: torch.Tensor) -> torch.Tensor:
        """(n, 300), n <= 8 -> (n, V) float32: the distance of every word to every row, computed directly (sqrt sum (q - w)^2)."""
        q = self._queries(vecs)
        n, v = q.shape[0], len(self.itos)
        if n > MAX_DISTS:
            raise MMVAEError("WordTable.dists: at most %d rows per call (got %d)" % (MAX_DISTS, n))
        out = torch.empty(n, v, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            call("mmvae_nn_words_dists", ptr(q), n, ptr(self.vectors), v, N_EMBEDDING, ptr(out), _stream())
        return out

    def closest(self, vec: torch.Tensor, n: int = 10) -> List[Tuple[str, float]]:
        """coco/glove.py:26-39: the n nearest words of one 300-vector as [(word, distance)], nearest first."""
        d = self.dists(torch.as_tensor(vec).reshape(1, N_EMBEDDING))[0]
        val, idx = torch.topk(d, min(int(n), d.numel()), largest=False, sorted=True)
        return [(self.itos[i], float(x)) for i, x in zip(idx.tolist(), val.tolist())]

    def closest_batch(self, vec_batch: torch.Tensor) -> List[str]:
        """coco/glove.py:41-70: the nearest word of every row of an (N, 300) batch."""
        index, _ = self.nearest(vec_batch)
        return [self.itos[i] for i in index.tolist()]

    def analogy(self, w1: str, w2: str, w3: str, n: int = 5, filter_given: bool = True) -> List[Tuple[str, float]]:
        """coco/glove.py:72-93: the words nearest to w2 - w1 + w3.  The reference's function lacks ``self`` and reads
        ``self.filter_given``; this is its evident intent: a method whose ``filter_given`` argument drops the three given words,
        and that looks at n + 3 candidates so that n remain after the drop."""
        vs = [self.get_word(w) for w in (w1, w2, w3)]
        for w, v in zip((w1, w2, w3), vs):
            if v is None:
                raise KeyError(w)
        found = self.closest(vs[1] - vs[0] + vs[2], n + 3 if filter_given else n)
        if filter_given:
            found = [t for t in found if t[0] not in (w1, w2, w3)]
        return found[:n]

    def embed(self, sentence: str, tokenizer: Callable[[str], List[str]] = str.split) -> torch.Tensor:
        """coco/utils.py:36-47: '<s>' + words + '</s>' as a (102, 300) float32 host tensor; at most 100 words are kept, an unknown
        word and the padding are zero rows.  The default tokenizer is ``str.split`` (the reference's is nltk's word_tokenize)."""
        words = list(tokenizer(sentence))[:MAX_WORDS - 2]
        words = [SOS] + words + [EOS]
        out = torch.zeros(MAX_WORDS, N_EMBEDDING)
        for i, w in enumerate(words):
            j = self.stoi.get(w)
            if j is not None:
                out[i] = self.vectors[j]
        return out


def save_word_table(path: str, vectors: torch.Tensor, itos: Sequence[str]) -> str:
    """One ``.pt`` file holding ``(float32 (V,300), list[str])``."""
    WordTable(torch.as_tensor(vectors), itos)                     # the refusals of the constructor, before anything is written
    torch.save((torch.as_tensor(vectors).detach().cpu().contiguous(), list(itos)), path)
    return path


def load_word_table(path: str, device=None) -> WordTable:
    vectors, itos = torch.load(path, map_location="cpu", weights_only=True)
    return WordTable(vectors, itos, device)


def _plan(steps):
    """the plan a stand-alone module builds: the family's, at the module's caption length"""
    return lambda n, d: CocoState(n, d, steps)


class ImageEncoder(nn.Module):
    """coco/model.py:147-187"""

    def __init__(self, n_latents, steps=MAX_WORDS):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(3, 64, 4, 2, 1, bias=False), Swish(),
            nn.Conv2d(64, 128, 4, 2, 1, bias=False), nn.BatchNorm2d(128), Swish(),
            nn.Conv2d(128, 256, 4, 2, 1, bias=False), nn.BatchNorm2d(256), Swish(),
            nn.Conv2d(256, 512, 4, 2, 1, bias=False), nn.BatchNorm2d(512), Swish())
        self.classifier = nn.Sequential(nn.Linear(512 * 2 * 2, 1024), Swish(), nn.Dropout(p=0.1),
                                        nn.Linear(1024, 256), Swish(), nn.Dropout(p=0.1), nn.Linear(256, n_latents * 2))
        self.n_latents = n_latents
        self.steps = steps
        self._core = None

    def forward(self, x, masks=None):
        n = self.n_latents
        x = x.contiguous().float()
        assert x.shape[1:] == (3, 32, 32), "expected (B,3,32,32) images (coco/train.py:107-112)"
        m1 = m2 = None
        if _dropout_on(self, (self.classifier[2].p, self.classifier[5].p),
                       "the HIP image encoder supports Dropout p in {0, 0.1} on both layers (reference: 0.1)"):
            if masks is not None:
                m1, m2 = (m.to(torch.uint8).contiguous() for m in masks)
            else:                                                    # one seed per mask
                m1, m2 = Draw((x.shape[0], 1024), 2), Draw((x.shape[0], 256), 3)
        out = run_module(self, "image_encoder.", _plan(self.steps), x, "mmvae_coco_image_encoder", (2 * n,),
                         ("x", m1, m2, "training", "out"), ("d", m1, m2))
        return out[:, :n], out[:, n:]


class ImageDecoder(nn.Module):
    """coco/model.py:190-216"""

    def __init__(self, n_latents, steps=MAX_WORDS):
        super().__init__()
        self.upsample = nn.Sequential(nn.Linear(n_latents, 512 * 2 * 2), Swish())
        self.hallucinate = nn.Sequential(
            nn.ConvTranspose2d(512, 256, 4, 2, 1, bias=False), nn.BatchNorm2d(256), Swish(),
            nn.ConvTranspose2d(256, 128, 4, 2, 1, bias=False), nn.BatchNorm2d(128), Swish(),
            nn.ConvTranspose2d(128, 64, 4, 2, 1, bias=False), nn.BatchNorm2d(64), Swish(),
            nn.ConvTranspose2d(64, 3, 4, 2, 1, bias=False))
        self.n_latents = n_latents
        self.steps = steps
        self._core = None

    def forward(self, z):
        return run_module(self, "image_decoder.", _plan(self.steps), z.contiguous().float(), "mmvae_coco_image_decoder", (3, 32, 32),
                          *DECODER)


class TextEncoder(nn.Module):
    """coco/model.py:219-245: biGRU(300 -> 200) over (B, steps, 300) GloVe vectors -> (mu, logvar)."""

    def __init__(self, n_latents, n_embedding=N_EMBEDDING, steps=MAX_WORDS):
        super().__init__()
        if n_embedding != N_EMBEDDING:
            raise MMVAEError("the HIP TextEncoder implements n_embedding=300 (GloVe-840B)")
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # dropout on a 1-layer GRU: a no-op the reference also asks for
            self.gru = nn.GRU(n_embedding, N_HIDDENS, 1, dropout=0.1, bidirectional=True)
        self.h2p = nn.Linear(N_HIDDENS, n_latents * 2)
        self.n_latents = n_latents
        self.n_embedding = n_embedding
        self.steps = steps
        self._core = None

    def forward(self, x):
        n = self.n_latents
        x = x.contiguous().float()
        assert x.dim() == 3 and x.shape[1] == self.steps and x.shape[2] == N_EMBEDDING, \
            "expected (B, %d, 300) caption tensors (coco/utils.py:36-47)" % self.steps
        out = run_module(self, "text_encoder.", _plan(self.steps), x, "mmvae_coco_text_encoder", (2 * n,), ("x", "out"), ("x", "d"))
        return out[:, :n], out[:, n:]


class TextDecoder(nn.Module):
    """coco/model.py:248-312: 2-layer GRU regressing one 300-d vector per step, fed back as the next input."""

    def __init__(self, n_latents, n_embedding=N_EMBEDDING, n_hiddens=N_HIDDENS, use_cuda=False, sos=None, steps=MAX_WORDS,
                 words: Optional[WordTable] = None):
        super().__init__()
        if n_embedding != N_EMBEDDING or n_hiddens != N_HIDDENS:
            raise MMVAEError("the HIP TextDecoder implements n_embedding=300, n_hiddens=200")
        self.z2h = nn.Linear(n_latents, n_hiddens)
        self.gru = nn.GRU(n_embedding + n_latents, n_hiddens, 2, dropout=0.1)
        self.h2o = nn.Linear(n_hiddens + n_latents, n_embedding)
        if sos is None and words is not None:
            sos = words.get_word(SOS)
            if sos is None:
                raise MMVAEError("TextDecoder: the word table has no '%s' (coco/model.py:268) and no sos= was given" % SOS)
            sos = sos.detach().cpu()                               # a buffer of the module: it moves with the module
        if sos is None:
            raise MMVAEError("TextDecoder needs sos= the 300-d GloVe vector of '<s>' (coco/model.py:271); the GloVe table "
                             "itself is not part of this engine")
        self.register_buffer("sos", torch.as_tensor(sos, dtype=torch.float32).reshape(n_embedding).clone(), persistent=False)
        self.words = words                                         # a plain attribute: no parameter, no buffer
        self.use_cuda = use_cuda
        self.n_latents = n_latents
        self.n_embedding = n_embedding
        self.n_hiddens = n_hiddens
        self.steps = steps
        self._core = None

    def forward(self, z, keep: Optional[torch.Tensor] = None):
        z = z.contiguous().float()
        if not _dropout_on(self, (self.gru.dropout,), "the HIP text decoder supports GRU dropout in {0, 0.1} (reference: 0.1)"):
            keep = None
        elif keep is None:
            keep = Draw((self.steps, z.shape[0], N_HIDDENS), 4)
        else:
            keep = keep.to(torch.uint8).contiguous()
        sos = self.sos.to(z.device).contiguous()
        return run_module(self, "text_decoder.", _plan(self.steps), z, "mmvae_coco_text_decoder", (self.steps, N_EMBEDDING),
                          ("x", sos, keep, "training", "out"), ("x", sos, keep, "out", "d", "dx"))

    def generate_vector(self, z):
        """coco/model.py:308-309"""
        return self.forward(z)

    def generate(self, z, stop_at_eos: bool = False):
        """coco/model.py:288-304 with a word table attached (``words=``): B strings of ``steps`` nearest words joined by spaces.
        This is the evident intent of the reference's reshape loop, which indexes ``strings`` out of range as written.
        ``stop_at_eos=True`` (an addition) cuts every sentence in front of its first '</s>'."""
        if self.words is None:
            raise MMVAEError("TextDecoder.generate (coco/model.py:290-306) decodes vectors to words through the GloVe table, "
                             "which is not part of this engine; use generate_vector")
        with torch.no_grad():
            vecs = self.forward(z)                                 # (B, steps, 300)
            strings = self.words.closest_batch(vecs.reshape(-1, self.n_embedding))
        return assemble_sentences(strings, vecs.shape[0], vecs.shape[1], stop_at_eos)


def assemble_sentences(strings: Sequence[str], batch: int, steps: int, stop_at_eos: bool = False) -> List[str]:
    """batch * steps words, example-major -> batch sentences (``stop_at_eos``: the words in front of the first '</s>')."""
    assert len(strings) == batch * steps
    out = []
    for i in range(batch):
        sentence = list(strings[i * steps:(i + 1) * steps])
        if stop_at_eos and EOS in sentence:
            sentence = sentence[:sentence.index(EOS)]
        out.append(' '.join(sentence))
    return out


class MultimodalVAE(ExpertsVAEBase):
    """coco/model.py:22-90"""

    def __init__(self, n_latents=20, use_cuda=False, sos=None, steps=MAX_WORDS, words: Optional[WordTable] = None):
        super().__init__()
        self.image_encoder = ImageEncoder(n_latents, steps=steps)
        self.image_decoder = ImageDecoder(n_latents, steps=steps)
        self.text_encoder = TextEncoder(n_latents, steps=steps)
        self.text_decoder = TextDecoder(n_latents, use_cuda=use_cuda, sos=sos, steps=steps, words=words)
        self.experts = ProductOfExperts()
        self.n_latents = n_latents
        self.steps = steps
        self._core = _Core(self, "", n_latents, lambda n, d: CocoState(n, d, steps))
        self._adopt(self.image_encoder, self.image_decoder, self.text_encoder, self.text_decoder)

    def encode_image(self, x):
        return self.image_encoder(x)

    def decode_image(self, z):
        return self.image_decoder(z)

    def encode_text(self, x):
        return self.text_encoder(x)

    def decode_text(self, z):
        return self.text_decoder(z)

    def forward(self, image=None, text=None, eps=None, enc_masks=None, gru_keep=None):
        assert image is not None or text is not None
        mu, logvar = self._product(None if image is None else self.image_encoder(image, enc_masks),
                                   None if text is None else self.text_encoder(text))
        z = self.reparametrize(mu, logvar, eps)
        return self.image_decoder(z), self.text_decoder(z, gru_keep), mu, logvar


def loss_function(mu, logvar, recon_image=None, image=None, recon_text=None, text=None,
                  kl_lambda=1e-3, lambda_xy=1., lambda_yx=1.):
    """coco/train.py:66-84"""
    batch_size = mu.size(0)
    image_BCE, text_BCE = 0, 0
    if recon_image is not None and image is not None:
        image_BCE = lambda_xy * _BCEMeanFn.apply(recon_image.reshape(-1, 3 * 32 * 32), image.reshape(-1, 3 * 32 * 32))
    if recon_text is not None and text is not None:
        text_BCE = lambda_yx * _MSEMeanFn.apply(recon_text, text)
    KLD = _KLSumFn.apply(mu, logvar)
    KLD = KLD / batch_size * kl_lambda
    return image_BCE + text_BCE + KLD


elbo_loss = loss_function


class InfoVAE(VAEBase):
    """coco/model.py:358-382.  ``encoder`` / ``decoder`` are the stand-alone HIP modules above, each on its own core, so
    ``state_dict()`` has the reference's keys (``encoder.features.0.weight`` ... ``decoder.hallucinate.9.weight``) and
    ``optim.Adam(vae.parameters())`` steps the ``nn.Parameter``s the kernels read."""

    def __init__(self, n_latents=20):
        super().__init__()
        self.encoder = ImageEncoder(n_latents)
        self.decoder = ImageDecoder(n_latents)
        self.n_latents = n_latents

    def encode(self, x, masks=None):
        return self.encoder(x, masks)

    def decode(self, z):
        return self.decoder(z)

    def forward(self, x, eps=None, enc_masks=None):
        mu, logvar = self.encode(x, enc_masks)
        z = self.reparametrize(mu, logvar, eps)
        return self.decode(z), z


TRUE_SAMPLES_STREAM = 5    # Philox stream of infovae_loss's prior samples (1: reparametrize, 2-4: the dropout masks)


def infovae_loss(recon_x, x, z, true_samples: Optional[torch.Tensor] = None):
    """coco/train_infovae.py:44-55: mean BCE + MMD(true_samples, z), ``true_samples`` ~ N(0, I) of z's shape, drawn on the device
    (seeded from torch's generator) unless given."""
    BCE = _BCEMeanFn.apply(recon_x.reshape(recon_x.shape[0], -1), x.reshape(x.shape[0], -1))
    if true_samples is None:
        true_samples = torch.empty(z.shape[0], z.shape[1], dtype=torch.float32, device=z.device)
        call("mmvae_normal", ptr(true_samples), true_samples.numel(), _seed_from_torch(), None, TRUE_SAMPLES_STREAM, _stream())
    MMD = compute_mmd(true_samples, z)
    return BCE + MMD


def load_checkpoint(file_path, use_cuda=False, sos=None, words: Optional[WordTable] = None):
    """coco/train.py:47-61: rebuilds a MultimodalVAE from the checkpoint dict (``state_dict``, ``n_latents``) that
    ``train_coco`` (or the reference) writes.  The '<s>' vector is not in the state dict (the reference reads it from GloVe
    at every forward): give ``sos=`` or a word table that has '<s>'."""
    return load_vae_checkpoint(file_path, MultimodalVAE, use_cuda, 100, use_cuda=use_cuda, sos=sos, words=words)


class FusedTrainer(Trainer):
    """``FusedTrainer(vae, batch_size, lr)(image, text)``: coco/train.py:138-173 (3 passes, 3 losses), lr 1e-4 (coco/train.py:94),
    kl_lambda 1e-3."""
    ENGINE, LR = FusedCocoStep, 1e-4
    ENC_DROPOUT = staticmethod(lambda vae: vae.image_encoder.classifier[2].p)
    GRU_DROPOUT = staticmethod(lambda vae: vae.text_decoder.gru.dropout)

    def _engine_kw(self, vae, batch_size):
        return {"sos": vae.text_decoder.sos}


# ----------------------------------------------------------------------------------------------------------------
# the uni-modal image baseline (coco/model.py:93-117, coco/train_imageonly.py)
# ----------------------------------------------------------------------------------------------------------------
IMAGE_VAE_STEPS = 1       # caption length of the plan an ImageVAE lives on: no caption ever runs, so its buffers are the smallest


class ImageVAE(VAEBase):
    """coco/model.py:93-117: ``ImageEncoder`` + ``reparametrize`` + ``ImageDecoder`` under the reference's ``encoder.`` / ``decoder.``
    keys, with NO product of experts.  Unlike ``InfoVAE`` (two stand-alone cores, autograd between them) the two children share ONE
    core on the MultimodalVAE's plan (``encoder.features.0.weight`` is its ``image_encoder.features.0.weight``), which is what
    ``ImageVAETrainer`` steps in one enqueue; the caption half of the flat buffers keeps its initial value and never shows in
    ``state_dict()``."""

    def __init__(self, n_latents=20):
        super().__init__()
        self.encoder = ImageEncoder(n_latents, steps=IMAGE_VAE_STEPS)
        self.decoder = ImageDecoder(n_latents, steps=IMAGE_VAE_STEPS)
        self.n_latents = n_latents
        self._core = _Core(self, "image_", n_latents, lambda n, d: CocoState(n, d, IMAGE_VAE_STEPS))
        self._adopt(self.encoder, self.decoder)

    def encode(self, x, masks=None):
        return self.encoder(x, masks)

    def decode(self, z):
        return self.decoder(z)

    def forward(self, x, eps=None, enc_masks=None):
        mu, logvar = self.encode(x, enc_masks)
        z = self.reparametrize(mu, logvar, eps)
        return self.decode(z), mu, logvar


def load_checkpoint_imageonly(file_path, use_cuda=False):
    """coco/train_imageonly.py:28-40: rebuilds an ImageVAE from the checkpoint dict (``state_dict``, ``n_latents``)."""
    return load_vae_checkpoint(file_path, ImageVAE, use_cuda)


class ImageVAETrainer(Trainer):
    """``ImageVAETrainer(vae, batch_size, lr)(image)``: coco/train_imageonly.py:105-116, lr 1e-4, kl_lambda 5e-4, on an
    ``ImageVAE``: one pass over B rows."""
    ENGINE, LR, KL_LAMBDA = FusedImageStep, 1e-4, 5e-4
    ENC_DROPOUT = staticmethod(lambda vae: vae.encoder.classifier[2].p)


# ----------------------------------------------------------------------------------------------------------------
# InfoVAE on one core: the fused step of coco/train_infovae.py
# ----------------------------------------------------------------------------------------------------------------
class FusedInfoVAE(ImageVAE):
    """coco/model.py:358-382 with ``ImageVAE``'s one-core construction: ``encoder`` / ``decoder`` share ONE core on the
    MultimodalVAE's plan, under the reference's ``encoder.`` / ``decoder.`` keys -- ``InfoVAE``'s keys, so a state dict of either class
    (and a reference checkpoint) loads strict into the other.  The surface is ``InfoVAE``'s: ``forward(x) -> (recon, z)``."""

    def forward(self, x, eps=None, enc_masks=None):
        mu, logvar = self.encode(x, enc_masks)
        z = self.reparametrize(mu, logvar, eps)
        return self.decode(z), z


class InfoVAETrainer(Trainer):
    """``InfoVAETrainer(vae, batch_size, lr)(image)``: coco/train_infovae.py:113-128 (mean BCE + MMD against prior samples, no KL
    term), lr 1e-4, on a ``FusedInfoVAE``: one pass over B rows, the MMD sweep beside the decoder."""
    ENGINE, LR, KL_LAMBDA = FusedInfoVAEStep, 1e-4, 0.0
    ENC_DROPOUT = staticmethod(lambda vae: vae.encoder.classifier[2].p)


# ----------------------------------------------------------------------------------------------------------------
# the uni-modal caption baseline (coco/model.py:120-144, coco/train_textonly.py)
# ----------------------------------------------------------------------------------------------------------------
MIN_LATENTS, MAX_LATENTS, LATENTS_STEP = 4, 124, 4     # what mmvae_coco_create takes: the operand padding of the caption kernels


def check_text_latents(n_latents) -> int:
    """The latent sizes the COCO plan is built for, refused on the host with the range in the message."""
    n = int(n_latents)
    if n < MIN_LATENTS or n > MAX_LATENTS or n % LATENTS_STEP != 0:
        raise MMVAEError("TextVAE: n_latents=%d does not fit the caption kernels' operand padding; the COCO plan takes n_latents in "
                         "%d..%d, a multiple of %d (the reference script's default of 200 is outside that range: train_textonly "
                         "defaults to 100)" % (n, MIN_LATENTS, MAX_LATENTS, LATENTS_STEP))
    return n


class TextVAE(VAEBase):
    """coco/model.py:120-144: ``TextEncoder`` + ``reparametrize`` + ``TextDecoder`` under the reference's ``encoder.`` / ``decoder.``
    keys, with NO product of experts.  The two children share ONE core on the MultimodalVAE's plan (``encoder.gru.weight_ih_l0`` is
    its ``text_encoder.gru.weight_ih_l0``), which is what ``TextVAETrainer`` steps in one enqueue; the image half of the flat
    buffers is never read or written and never shows in ``state_dict()``.  ``sos`` / ``words`` / ``steps`` as for ``TextDecoder``.
    ``n_latents``: 4..124 in multiples of 4 (the reference script's 200 is refused)."""

    def __init__(self, n_latents=20, use_cuda=False, words: Optional[WordTable] = None, sos=None, steps=MAX_WORDS):
        n_latents = check_text_latents(n_latents)
        super().__init__()
        self.encoder = TextEncoder(n_latents, steps=steps)
        self.decoder = TextDecoder(n_latents, use_cuda=use_cuda, sos=sos, steps=steps, words=words)
        self.n_latents = n_latents
        self.steps = steps
        self._core = _Core(self, "text_", n_latents, lambda n, d: CocoState(n, d, steps))
        self._adopt(self.encoder, self.decoder)

    def encode(self, x):
        return self.encoder(x)

    def decode(self, z, keep: Optional[torch.Tensor] = None):
        return self.decoder(z, keep)

    def forward(self, x, eps=None, gru_keep=None):
        mu, logvar = self.encode(x)
        z = self.reparametrize(mu, logvar, eps)
        return self.decode(z, gru_keep), mu, logvar


def load_checkpoint_textonly(file_path, use_cuda=False, sos=None, words: Optional[WordTable] = None, steps=MAX_WORDS):
    """coco/train_textonly.py:28-40: rebuilds a TextVAE from the checkpoint dict (``state_dict``, ``n_latents``).  The '<s>' vector is
    not in the state dict: give ``sos=`` or a word table that has '<s>'."""
    return load_vae_checkpoint(file_path, TextVAE, use_cuda, use_cuda=use_cuda, sos=sos, words=words, steps=steps)


class TextVAETrainer(Trainer):
    """``TextVAETrainer(vae, batch_size, lr)(text)``: coco/train_textonly.py:106-120, lr 1e-4, kl_lambda 1e-3, on a ``TextVAE``:
    one pass over B rows."""
    ENGINE, LR = FusedTextStep, 1e-4
    GRU_DROPOUT = staticmethod(lambda vae: vae.decoder.gru.dropout)

    def _engine_kw(self, vae, batch_size):
        return {"sos": vae.decoder.sos}
