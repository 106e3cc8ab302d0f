"""The family table of ``evaluate`` and what hangs on it, on the CPU: the table against literals, the posterior helper and the
samplers on pure-torch stand-ins of the encoders, experts and decoders (which calls, in which order, on which draw), and the
command line's shared helpers (dispatch, checkpoint opener, batch slicer, posterior chooser)."""
import pytest
import torch
import torch.nn as nn

D = 8          # n_latents of every model here


def _models():
    from multimodal_vae_amd import celeba as C, coco as K, mnist as N, multimnist as M
    sos = dict(sos=torch.zeros(300))
    return {"multimnist": (M.MultimodalVAE, {}), "mnist": (N.MultimodalVAE, {}), "celeba": (C.MultimodalVAE, {}),
            "coco": (K.MultimodalVAE, sos), "celeba_image": (C.ImageVAE, {}), "coco_image": (K.ImageVAE, {}),
            "coco_text": (K.TextVAE, sos), "multimnist_image": (M.ImageVAE, {}), "mnist_image": (N.VAE, {}),
            "multimnist_text": (M.TextVAE, {})}


# key: (name, T, V, image_shape, rows, float_text, image_only, text_only), the values before the table grew
LITERALS = {
    "multimnist": ("multimnist", 4, 12, (1, 50, 50), 4096, False, False, False),
    "mnist": ("mnist", 1, 10, (784,), 65536, False, False, False),
    "celeba": ("celeba", 18, 2, (3, 64, 64), 512, False, False, False),
    "coco": ("coco", 1, 1, (3, 32, 32), 512, True, False, False),
    "celeba_image": ("celeba", 1, 1, (3, 64, 64), 512, False, True, False),
    "coco_image": ("coco", 1, 1, (3, 32, 32), 512, False, True, False),
    "coco_text": ("coco", 1, 1, (3, 32, 32), 512, True, False, True),
    "multimnist_image": ("multimnist", 1, 1, (1, 50, 50), 4096, False, True, False),
    "mnist_image": ("mnist", 1, 1, (784,), 65536, False, True, False),
    "multimnist_text": ("multimnist", 4, 12, (1,), 4096, False, False, True),
}
PICTURES = {"multimnist": (1, 50, 50), "mnist": (1, 28, 28), "celeba": (3, 64, 64), "coco": (3, 32, 32)}
SECOND_SHAPES = {"multimnist": (4,), "mnist": (), "celeba": (18,), "coco": (102, 300)}


def test_the_table_has_the_ten_kinds():
    from multimodal_vae_amd import evaluate as E
    assert list(E._FAMILIES) == list(LITERALS) and (E.IW_ROWS, E.IW_ROWS_MNIST, E.IW_ROWS_CELEBA, E.IW_ROWS_COCO) == (4096, 65536, 512, 512)
    assert E._family(object()) is E._FAMILIES["multimnist"]                          # the fall-through stays


@pytest.mark.parametrize("key", list(LITERALS))
def test_table_against_literals(key):
    from multimodal_vae_amd import evaluate as E
    cls, kw = _models()[key]
    fam = E._FAMILIES[key]
    assert E._family(cls(D, **kw)) is fam
    assert (fam.name, fam.T, fam.V, fam.image_shape, fam.rows, fam.float_text, fam.image_only, fam.text_only) == LITERALS[key]
    assert fam.picture == (fam.image_shape if key == "multimnist_text" else PICTURES[fam.name])
    assert E._family(type("Sub", (cls,), {})(D, **kw)) is fam                        # a plain subclass resolves alike
    if key == "mnist":
        from multimodal_vae_amd.mnist import with_padded_latents
        assert E._family(with_padded_latents(cls(2))) is fam                         # ... and the padded-latent variant


# ---------------------------------------------------------------------------------------------------------- the stand-ins
class _Enc(nn.Module):
    """An affine map of the flattened input -> (mu, logvar) (or their concatenation, what ``mnist.VAE.encode`` splits); records
    its name, the input's dtype and shape."""

    def __init__(self, name, log, scale, cat=False):
        super().__init__()
        self.name, self.log, self.scale, self.cat = name, log, scale, cat
        self.w = nn.Parameter(torch.zeros(1))                    # (the samplers ask the model's parameters for its device)

    def forward(self, x, *rest):
        self.log.append((self.name, x.dtype, tuple(x.shape)))
        f = x.reshape(x.shape[0], -1).double()
        j = torch.arange(D, dtype=torch.float64)
        mu = (self.scale * f.mean(1, keepdim=True) + 0.1 * j).float()
        logvar = (-0.2 * self.scale * f[:, :1] - 0.05 * j).float()
        return torch.cat((mu, logvar), dim=1) if self.cat else (mu, logvar)


def _poe(mu, logvar, eps=1e-8):
    """``ProductOfExperts`` in closed form (multimnist/model.py:355-360, as written: no prior expert, variance-weighted mean)."""
    var = torch.exp(logvar) + eps
    return torch.sum(mu * var, dim=0) / torch.sum(var, dim=0), torch.log(1 / torch.sum(1 / var, dim=0))


class _Experts(nn.Module):
    def __init__(self, log):
        super().__init__()
        self.log, self.seen = log, None

    def forward(self, mu, logvar):
        self.log.append(("experts", mu.dtype, tuple(mu.shape)))
        self.seen = (mu.clone(), logvar.clone())
        return _poe(mu, logvar)


class _Dec(nn.Module):
    """z (n, D) -> sigmoid of a fixed linear map, in ``shape``; ``generate`` (COCO's caption decoder) -> one string per row."""

    def __init__(self, shape):
        super().__init__()
        self.shape = shape
        self.sos = torch.zeros(300)
        n_out = int(torch.tensor(shape).prod())
        self.register_buffer("weight", torch.linspace(-1, 1, D * n_out).reshape(D, n_out))

    def forward(self, z, *rest):
        return torch.sigmoid(z @ self.weight).reshape(z.shape[0], *self.shape)

    def generate(self, z, stop_at_eos=False):
        return ["%.4f %s" % (float(row.sum()), stop_at_eos) for row in z]


SECOND_DECODED = {"multimnist": (4, 12), "mnist": (10,), "celeba": (18,), "coco": (102, 300)}


def _stand_in(key):
    """A CPU model of the kind with every encoder, the experts and every decoder replaced -> (model, family, call log, experts)."""
    from multimodal_vae_amd import evaluate as E
    cls, kw = _models()[key]
    model, fam, log = cls(D, **kw), E._FAMILIES[key], []
    experts = _Experts(log)
    image_dec, second_dec = _Dec(PICTURES[fam.name] if fam.name != "mnist" else (784,)), _Dec(SECOND_DECODED[fam.name])
    if fam.image_only:
        model.encoder, model.decoder = _Enc("image", log, 1.0, cat=key == "mnist_image"), image_dec
    elif fam.text_only:
        model.encoder, model.decoder = _Enc("second", log, -0.5), second_dec
    else:
        second = "attrs" if key == "celeba" else "text"
        model.image_encoder, model.image_decoder, model.experts = _Enc("image", log, 1.0), image_dec, experts
        setattr(model, second + "_encoder", _Enc("second", log, -0.5))
        setattr(model, second + "_decoder", second_dec)
    return model.eval(), fam, log, experts


def _inputs(fam, B, seed=0):
    g = torch.Generator().manual_seed(seed)
    image = torch.rand(B, *fam.image_shape, generator=g)
    if fam.name == "coco":
        second = torch.randn(B, 102, 300, generator=g)
    else:
        second = torch.randint(0, 2, (B,) + SECOND_SHAPES[fam.name], generator=g)       # int64: CelebA's attributes go in as float
    return image, second


def _expected_posterior(fam, image, second, posterior):
    enc_i, enc_s = _Enc("image", [], 1.0), _Enc("second", [], -0.5)
    parts = ([enc_i(image)] if posterior != "text" else []) + ([enc_s(second.float() if fam.name == "celeba" else second)] if posterior != "image" else [])
    return torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts])


# ------------------------------------------------------------------------------------------------------ the posterior helper
@pytest.mark.parametrize("key", ["multimnist", "mnist", "celeba", "coco"])
def test_proposal_of_a_multimodal_family(key):
    from multimodal_vae_amd import evaluate as E
    model, fam, log, experts = _stand_in(key)
    image, second = _inputs(fam, 2)
    second_dtype = torch.float32 if key in ("celeba", "coco") else torch.int64
    for posterior in ("joint", "image", "text") + (("attrs",) if key == "celeba" else ()):
        del log[:]
        mu, logvar = E._proposal(model, image.reshape(2, -1), second, posterior)       # (the image comes flat or shaped)
        p = E._posterior(posterior)
        want_calls = ([("image", torch.float32, (2,) + fam.image_shape)] if p != "text" else []) + \
                     ([("second", second_dtype, tuple(second.shape))] if p != "image" else [])
        assert log[:-1] == want_calls and log[-1] == ("experts", torch.float32, (len(want_calls), 2, D)), (posterior, log)
        stack_mu, stack_lv = _expected_posterior(fam, image, second, p)
        assert torch.equal(experts.seen[0], stack_mu) and torch.equal(experts.seen[1], stack_lv)      # image first, then the second
        want_mu, want_lv = _poe(stack_mu, stack_lv)
        assert mu.shape == (2, D) and torch.equal(mu, want_mu) and torch.equal(logvar, want_lv)
        assert not torch.equal(mu[0], mu[1])
    with pytest.raises(ValueError, match="must be one of"):
        E._proposal(model, image, second, "nonsense")


@pytest.mark.parametrize("key", ["celeba_image", "coco_image", "multimnist_image", "mnist_image", "coco_text", "multimnist_text"])
def test_proposal_of_a_unimodal_kind(key):
    from multimodal_vae_amd import evaluate as E
    model, fam, log, _ = _stand_in(key)
    image, second = _inputs(fam, 2)
    own, others = ("text", ("joint", "image")) if fam.text_only else ("image", ("joint", "text", "attrs"))
    mu, logvar = E._proposal(model, None if fam.text_only else image, second if fam.text_only else None, own)
    want = _Enc("second", [], -0.5)(second) if fam.text_only else _Enc("image", [], 1.0)(image)
    assert len(log) == 1 and log[0][0] == ("second" if fam.text_only else "image")                  # the encoder alone: no experts
    assert torch.equal(mu, want[0]) and torch.equal(logvar, want[1])
    for posterior in others:
        with pytest.raises(ValueError, match="text posterior alone" if fam.text_only else "image posterior alone"):
            E._proposal(model, image, second, posterior)
    assert len(log) == 1                                                                            # refused before any encoder ran


# -------------------------------------------------------------------------------------------------------------- the samplers
def _next_global_draw_after(fn, seed):
    torch.manual_seed(seed)
    out = fn()
    return out, torch.randn(1)


def _next_global_draw_after_randn(n, seed):
    torch.manual_seed(seed)
    torch.randn(n, D)
    return torch.randn(1)


def _z(fam, image, second, eps):
    """decode's argument: eps * std + mu of the prior, or of the posterior of what is given."""
    if image is None and second is None:
        return eps
    posterior = "text" if image is None else "image" if second is None else "joint"
    if fam.image_only or fam.text_only:
        mu, logvar = _Enc("second", [], -0.5)(second) if fam.text_only else _Enc("image", [], 1.0)(image)
    else:
        mu, logvar = _poe(*_expected_posterior(fam, image, second, posterior))
    return eps * logvar.mul(0.5).exp() + mu


def _modes(fam):
    image, second = _inputs(fam, 1, seed=3)
    if fam.image_only:
        return [(None, None), (image, None)]
    if fam.text_only:
        return [(None, None), (None, second)]
    return [(None, None), (image, None), (None, second), (image, second)]


@pytest.mark.parametrize("key", ["multimnist", "multimnist_text", "multimnist_image", "mnist_image"])
def test_samplers_on_the_global_generator(key):
    from multimodal_vae_amd import evaluate as E
    model, fam, log, _ = _stand_in(key)
    n, seed = 3, 11
    for image, second in _modes(fam):
        if key == "multimnist":
            fn = lambda: E.sample(model, n, image, second, use_cuda=False)
        elif key == "multimnist_text":
            fn = lambda: (None, E.sample_textonly(model, n, second))
        else:
            fn = lambda: (E.sample_imageonly(model, n, image), None)
        (pictures, tokens), after = _next_global_draw_after(fn, seed)
        assert torch.equal(after, _next_global_draw_after_randn(n, seed))              # one draw of (n, D) and nothing more
        torch.manual_seed(seed)
        z = _z(fam, image, second, torch.randn(n, D))
        if pictures is not None:
            side = 28 if key == "mnist_image" else 50
            want = _Dec((784,) if key == "mnist_image" else (1, 50, 50))(z).view(n, 1, side, side)
            assert pictures.shape == (n, 1, side, side) and torch.equal(pictures, want)
        if tokens is not None:
            assert tokens.shape == (n, 4) and torch.equal(tokens, _Dec((4, 12))(z).max(dim=2)[1])


@pytest.mark.parametrize("key", ["coco", "coco_text", "celeba"])
def test_samplers_with_a_generator_of_their_own(key):
    from multimodal_vae_amd import evaluate as E
    from multimodal_vae_amd.celeba import tensor_to_attributes
    model, fam, log, _ = _stand_in(key)
    n, seed = 3, 5
    fn = E.sample_celeba if key == "celeba" else E.sample_coco
    for image, second in _modes(fam):
        (pictures, words), after = _next_global_draw_after(lambda: fn(model, n, image, second, seed=seed), 7)
        torch.manual_seed(7)
        assert torch.equal(after, torch.randn(1))                                      # seed=: the global generator is untouched
        z = _z(fam, image, second, torch.randn(n, D, generator=torch.Generator().manual_seed(seed)))
        if key == "coco_text":
            assert pictures is None
        else:
            assert pictures.shape == (n,) + PICTURES[fam.name] and torch.equal(pictures, _Dec(PICTURES[fam.name])(z))
        if key == "celeba":
            assert words == [tensor_to_attributes(row) for row in _Dec((18,))(z)]
        else:
            assert words == _Dec((1,)).generate(z) and fn(model, n, image, second, stop_at_eos=True, seed=seed)[1] == _Dec((1,)).generate(z, True)
        # without a seed: one draw of (n, D) from the global generator
        (pictures2, words2), after = _next_global_draw_after(lambda: fn(model, n, image, second), seed)
        assert torch.equal(after, _next_global_draw_after_randn(n, seed))
        torch.manual_seed(seed)
        z2 = _z(fam, image, second, torch.randn(n, D))
        if key != "coco_text":
            assert torch.equal(pictures2, _Dec(PICTURES[fam.name])(z2))
    if key == "coco_text":
        with pytest.raises(ValueError, match="cannot be conditioned on an image"):
            E.sample_coco(model, n, torch.zeros(1, 3, 32, 32), None)


# ---------------------------------------------------------------------------------------------------------- the command line
def test_every_subcommand_is_dispatched():
    from multimodal_vae_amd import evaluate as E
    sub = [a for a in E._parser()._actions if getattr(a, "choices", None) and a.dest == "cmd"][0]
    assert set(sub.choices) == set(E._COMMANDS) and len(E._COMMANDS) == 13
    assert all(callable(f) for f in E._COMMANDS.values()) and E._COMMANDS["loglik_coco"] is E._loglik_coco_main


OPENS = [("mnist", "multimodal", "mnist"), ("mnist", "image", "mnist_image"), ("multimnist", "multimodal", "multimnist"),
         ("multimnist", "image", "multimnist_image"), ("multimnist", "text", "multimnist_text"), ("celeba", "multimodal", "celeba"),
         ("celeba", "image", "celeba_image"), ("coco", "multimodal", "coco"), ("coco", "image", "coco_image"), ("coco", "text", "coco_text")]


def _save(tmp_path, key):
    cls, kw = _models()[key]
    path = str(tmp_path / (key + ".pth.tar"))
    torch.save({"state_dict": cls(D, **kw).state_dict(), "best_loss": 1.0, "n_latents": D, "optimizer": {}}, path)      # the drivers' four keys
    return path, cls


@pytest.mark.parametrize("dataset,kind,key", OPENS)
def test_checkpoint_opener(tmp_path, dataset, kind, key):
    from multimodal_vae_amd import evaluate as E
    path, cls = _save(tmp_path, key)
    kw = dict(sos=torch.zeros(300), words=None) if dataset == "coco" else {}
    model, got = E._open_checkpoint(dataset, path, use_cuda=False, **kw)
    assert got == kind and type(model) is cls and model.n_latents == D
    assert E.is_textonly_checkpoint(path) == (kind == "text") and E.is_imageonly_checkpoint(path) == (kind != "multimodal")


def test_checkpoint_opener_refuses_what_does_not_exist(tmp_path):
    from multimodal_vae_amd import evaluate as E
    text, _ = _save(tmp_path, "multimnist_text")
    for dataset in ("mnist", "celeba"):
        with pytest.raises(SystemExit, match="no text-only model of the %s family" % dataset):
            E._open_checkpoint(dataset, text, use_cuda=False)
    assert ("mnist", "text") not in E._LOADERS and ("celeba", "text") not in E._LOADERS and len(E._LOADERS) == len(OPENS)


def test_batches():
    from multimodal_vae_amd import evaluate as E
    x, t = torch.arange(5), torch.arange(5) * 10
    b = E._batches(x, t, 2)
    assert [len(a) for a, _ in b] == [2, 2, 1] and torch.equal(torch.cat([a for a, _ in b]), x) and torch.equal(torch.cat([c for _, c in b]), t)
    whole = E._batches(x, t, 2, whole_only=True)
    assert [len(a) for a, _ in whole] == [2, 2] and torch.equal(whole[1][1], t[2:4])
    assert [(a, len(c)) for a, c in E._batches(None, t, 8, whole_only=True)] == [(None, 5)]           # at most the whole set
    assert [(len(a), c) for a, c in E._batches(x, None, 8)] == [(5, None)]


def test_which_posteriors():
    from multimodal_vae_amd import evaluate as E
    parse = E._parser().parse_args
    for cmd, second in (("loglik", "--text_only"), ("loglik_celeba", "--attrs_only"), ("loglik_coco", "--text_only")):
        assert E._which_posteriors(parse([cmd, "m", "--all"]), "multimodal") == ("joint", "image", "text") == E.POSTERIORS
        assert E._which_posteriors(parse([cmd, "m", "--image_only"]), "multimodal") == ("image",)
        assert E._which_posteriors(parse([cmd, "m", second]), "multimodal") == ("text",)
        assert E._which_posteriors(parse([cmd, "m"]), "multimodal") == ("joint",)
        for flags in ([], ["--all"], ["--image_only"], [second]):                                     # a uni-modal checkpoint: its own alone
            assert E._which_posteriors(parse([cmd, "m"] + flags), "image") == ("image",)
            assert E._which_posteriors(parse([cmd, "m"] + flags), "text") == ("text",)
