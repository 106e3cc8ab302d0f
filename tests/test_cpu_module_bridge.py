"""CPU tests of the drop-in modules' bridge to the C entry points (no GPU, the library is never loaded): ``call``, ``ptr``,
``_stream`` and ``_core_of`` are replaced, wherever the package's modules bind them, by recorders and a fake core, and every one of
the 18 module routes runs forward and ``.backward()`` on CPU tensors.  Checked per route: which entry points are called and in which
order, every call against its prototype in ``_lib.SIGNATURES``, the arguments the test can know against the order the C header
declares, the keep-mask draws, the gradients handed to autograd, and the BatchNorm refusals."""
import ctypes as C
import importlib
import inspect
import re
import sys

import pytest
import torch

from multimodal_vae_amd import _lib

FAMILIES = ("multimnist", "mnist", "celeba", "coco")
B, N, T = 2, 8, 3
NUMBERS = (C.c_int, C.c_size_t, C.c_float, C.c_longlong, C.c_ulonglong, C.c_uint)
BN_TEXT = "Expected more than 1 value per channel when training"


def _family(name):
    return importlib.import_module("multimodal_vae_amd." + name)


class _Route:
    """One module route.  ``fwd`` / ``bwd``: the arguments of the two entry points between ``h, ws, wsb`` and the stream (x: the
    module's input, out / out2: what forward allocates, d: the incoming gradient, dz: the input gradient, the rest by name);
    ``given``: the optional tensors of ``forward``, ``as_arg``: which symbol each of them is; ``salts``: of the keep masks a
    training forward draws when none is given; ``draws``: torch generator draws of that forward; ``refuses``: the largest batch
    a training forward refuses (None: it refuses none that has a row)."""

    def __init__(self, family, base, build, x, fwd, bwd, given=None, as_arg=(), salts=(), draws=0, refuses=None, pair=True):
        self.family, self.base, self.build, self.x = family, base, build, x
        self.fwd, self.bwd = fwd.split(), bwd.split()
        self.given, self.as_arg, self.salts, self.draws, self.refuses, self.pair = given or (lambda b: {}), as_arg, salts, draws, refuses, pair


def _u8(*shape):
    return torch.ones(*shape, dtype=torch.uint8)


def _img(*shape):
    return lambda b: torch.zeros(b, *shape)


def _z(b):
    return torch.zeros(b, N)


def _tokens(b):
    return torch.zeros(b, 4, dtype=torch.int64)


ENC2, DEC = "x m1 m2 training out", "z training out"
MMTXT_FWD, MMTXT_BWD = "z training keep ft out out2", "z keep ft out out2 d dz"

ROUTES = {
    "mm.image_encoder": _Route("multimnist", "mmvae_mm_image_encoder", lambda m: m.ImageEncoder(N), _img(1, 50, 50), ENC2, "d m1 m2",
                               lambda b: {"masks": (_u8(b, 400), _u8(b, 200))}, ("m1", "m2"), (2, 3), 1, refuses=0),
    "mm.image_decoder": _Route("multimnist", "mmvae_mm_image_decoder", lambda m: m.ImageDecoder(N), _z, DEC, "d out dz", refuses=0, pair=False),
    "mm.text_encoder": _Route("multimnist", "mmvae_mm_text_encoder", lambda m: m.TextEncoder(N, 12, n_hiddens=100), _tokens, "x out", "x d"),
    "mm.text_decoder": _Route("multimnist", "mmvae_mm_text_decoder", lambda m: m.TextDecoder(N, 12, n_hiddens=100), _z, MMTXT_FWD, MMTXT_BWD,
                              lambda b: {"keep": _u8(4, b, 100), "force_tokens": _tokens(b)}, ("keep", "ft"), (4,), 1, pair=False),
    "mmtext.encoder": _Route("multimnist", "mmvae_mmtext_encoder", lambda m: m.TextEncoder(N, 12, _textvae=True), _tokens, "x out", "x d"),
    "mmtext.decoder": _Route("multimnist", "mmvae_mmtext_decoder", lambda m: m.TextDecoder(N, 12, _textvae=True), _z, MMTXT_FWD, MMTXT_BWD,
                             lambda b: {"keep": _u8(4, b, 50), "force_tokens": _tokens(b)}, ("keep", "ft"), (4,), 1, pair=False),
    "mnist.image_encoder": _Route("mnist", "mmvae_mnist_image_encoder", lambda m: m.ImageEncoder(N), _img(784), "x training out", "d", refuses=1),
    "mnist.image_decoder": _Route("mnist", "mmvae_mnist_image_decoder", lambda m: m.ImageDecoder(N), _z, DEC, "d out dz", refuses=1, pair=False),
    "mnist.text_encoder": _Route("mnist", "mmvae_mnist_text_encoder", lambda m: m.TextEncoder(N), lambda b: torch.zeros(b, dtype=torch.int64),
                                 "x training out", "x d", refuses=1),
    "mnist.text_decoder": _Route("mnist", "mmvae_mnist_text_decoder", lambda m: m.TextDecoder(N), _z, DEC, "d out dz", refuses=1, pair=False),
    "mnist.VAE.encoder": _Route("mnist", "mmvae_mnist_image_encoder", lambda m: m.VAE(N).encoder, _img(784), "x training out", "d", refuses=1,
                                pair=False),
    "mnist.VAE.decoder": _Route("mnist", "mmvae_mnist_image_decoder", lambda m: m.VAE(N).decoder, _z, DEC, "d out dz", refuses=1, pair=False),
    "celeba.image_encoder": _Route("celeba", "mmvae_celeba_image_encoder", lambda m: m.ImageEncoder(N), _img(3, 64, 64), "x m1 training out", "d m1",
                                   lambda b: {"mask": _u8(b, 1024)}, ("m1",), (2,), 1),
    "celeba.image_decoder": _Route("celeba", "mmvae_celeba_image_decoder", lambda m: m.ImageDecoder(N), _z, DEC, "d out dz", pair=False),
    "celeba.attrs_encoder": _Route("celeba", "mmvae_celeba_attrs_encoder", lambda m: m.AttributeEncoder(N), _img(18), "x training out", "d", refuses=1),
    "celeba.attrs_decoder": _Route("celeba", "mmvae_celeba_attrs_decoder", lambda m: m.AttributeDecoder(N), _z, DEC, "d out dz", refuses=1, pair=False),
    "coco.image_encoder": _Route("coco", "mmvae_coco_image_encoder", lambda m: m.ImageEncoder(N, steps=T), _img(3, 32, 32), ENC2, "d m1 m2",
                                 lambda b: {"masks": (_u8(b, 1024), _u8(b, 256))}, ("m1", "m2"), (2, 3), 2),
    "coco.image_decoder": _Route("coco", "mmvae_coco_image_decoder", lambda m: m.ImageDecoder(N, steps=T), _z, DEC, "d out dz", pair=False),
    "coco.text_encoder": _Route("coco", "mmvae_coco_text_encoder", lambda m: m.TextEncoder(N, steps=T), _img(T, 300), "x out", "x d"),
    "coco.text_decoder": _Route("coco", "mmvae_coco_text_decoder", lambda m: m.TextDecoder(N, sos=torch.zeros(300), steps=T), _z,
                                "z sos keep training out", "z sos keep out d dz", lambda b: {"keep": _u8(T, b, 200)}, ("keep",), (4,), 1, pair=False),
}
assert len({r.base for r in ROUTES.values()}) == 18


class _FakeState:
    def __init__(self, log, table, total):
        self.log, self.table, self.grads = log, table, torch.zeros(total)

    def plan(self, batch):
        return C.c_void_p(0x1000 + int(batch))

    def module_workspace_bytes(self, batch):
        return 64 * int(batch)


class _FakeCore:
    """What a module reads of a ``_Core``: ``sync`` (recorded), ``grads_for``, ``n_latents``."""

    def __init__(self, log, module, prefix):
        self.log, self.prefix, self.n_latents = log, prefix, module.n_latents
        table, off = [], 0
        for k, p in module.named_parameters():
            table.append((prefix + k, tuple(p.shape), off))
            off += p.numel()
        self.state = _FakeState(log, table, off)

    def sync(self, device):
        self.log.append(("sync", ()))
        return self.state

    def grads_for(self, names):
        st, out = self.state, []
        for n, shape, off in st.table:
            if n in names:
                numel = 1
                for s in shape:
                    numel *= s
                out.append(st.grads[off:off + numel].view(shape).clone())
        return out


class _Bridge:
    """The recorders.  A ``*_bwd`` entry point finds the gradient buffer zeroed and leaves 1, 2, 3 ... in it."""

    def __init__(self, monkeypatch):
        self.log, self.cores, self.draws = [], {}, 0
        mods = [_family(f) for f in FAMILIES]
        fakes = {"call": self.call, "ptr": self.ptr, "_stream": lambda: C.c_void_p(0), "_core_of": self.core_of}
        for name, mod in list(sys.modules.items()):
            if mod is not None and name.startswith("multimodal_vae_amd."):
                for attr, fake in fakes.items():
                    if attr in vars(mod):
                        monkeypatch.setattr(mod, attr, fake)
        randint = torch.randint

        def counting(*a, **kw):
            self.draws += 1
            return randint(*a, **kw)
        monkeypatch.setattr(torch, "randint", counting)
        assert mods

    def call(self, name, *args):
        self.log.append((name, args))
        if name.endswith("_bwd"):
            (core,) = self.cores.values()
            g = core.state.grads
            assert not g.any(), "the gradient buffer is zeroed before the backward entry point"
            g.copy_(torch.arange(1, g.numel() + 1))
        return 0

    @staticmethod
    def ptr(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def core_of(self, module, prefix, state_cls=None):
        if id(module) not in self.cores:
            self.cores[id(module)] = _FakeCore(self.log, module, prefix)
        return self.cores[id(module)]

    def names(self):
        return [n for n, _ in self.log]


def _check_prototype(name, args):
    res, argtypes = _lib.SIGNATURES[name]
    assert len(args) == len(argtypes), name
    for i, (a, t) in enumerate(zip(args, argtypes)):
        if t in NUMBERS:
            assert isinstance(a, (int, float)) and not isinstance(a, bool), (name, i, a)
        else:
            assert t is C.c_void_p and (a is None or isinstance(a, C.c_void_p)), (name, i, a)


def _addr(a):
    return None if a is None else a.value


def _check_order(route, name, args, symbols, known):
    """``args`` against ``h, ws, wsb, *symbols, stream``: the values the test knows, and non-null pointers elsewhere."""
    assert _addr(args[0]) == 0x1000 + B and args[1] is not None and args[2] == 64 * B and _addr(args[-1]) in (0, None), name
    mid = args[3:-1]
    assert len(mid) == len(symbols), name
    for sym, a in zip(symbols, mid):
        if sym in known:
            want = known[sym]
            got = a if isinstance(want, int) and sym == "training" else _addr(a)
            assert got == want, (name, sym)
        else:
            assert isinstance(a, C.c_void_p) and a.value, (name, sym)


@pytest.mark.parametrize("given", [False, True], ids=["drawn", "given"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("rid", list(ROUTES))
def test_route_calls_its_entry_points(rid, train, given, monkeypatch):
    route = ROUTES[rid]
    br = _Bridge(monkeypatch)
    mod = route.build(_family(route.family)).train(train)
    x = route.x(B)
    if x.is_floating_point():
        x.requires_grad_(True)
    kw = route.given(B) if given else {}
    out = mod(x, **kw)
    first = out[0] if route.pair else out
    if route.pair:
        mu, logvar = out
        assert mu.shape == logvar.shape == (B, N) and logvar.data_ptr() == mu.data_ptr() + 4 * N
    seed = None
    if route.pair:
        sum(o.sum() for o in out).backward()
    else:
        seed = torch.ones_like(out)                              # contiguous: the incoming gradient reaches the entry point as it is
        out.backward(seed)

    # which entry points, in which order: the core's sync, the mask draws, forward, backward
    salts = route.salts if train and not given else ()
    assert br.names() == ["sync"] + ["mmvae_keep_mask"] * len(salts) + [route.base + "_fwd", route.base + "_bwd"]
    assert br.draws == (route.draws if salts else 0)
    calls = [(n, a) for n, a in br.log if n != "sync"]
    for n, a in calls:
        _check_prototype(n, a)
    masks = calls[:len(salts)]
    assert [a[5] for _, a in masks] == list(salts)
    assert all(a[2] == pytest.approx(0.1) and a[4] is None and a[0].value for _, a in masks)
    if route.draws == 1 and len(salts) == 2:
        assert masks[0][1][3] == masks[1][1][3]                   # one seed for both masks
    # the arguments the test knows, in the order of the header
    known = {"x": x.data_ptr(), "z": x.data_ptr(), "training": int(train), "out": first.data_ptr()}
    flat = []
    for v in kw.values():
        flat += list(v) if isinstance(v, tuple) else [v]
    for sym, t in zip(route.as_arg, flat):
        known[sym] = t.data_ptr() if (train or sym == "ft") else None
    if not given:
        for sym in route.as_arg:
            known[sym] = None
        for sym, (_, a) in zip(route.as_arg, masks):
            known[sym] = a[0].value
    if seed is not None:
        known["d"] = seed.data_ptr()                             # ... which tells d from dz, the one pointer left unknown
    if "out2" in route.fwd:
        known["out2"] = mod.last_tokens.data_ptr()
    (_, fa), (_, ba) = calls[len(salts):]
    _check_order(route, route.base + "_fwd", fa, route.fwd, known)
    _check_order(route, route.base + "_bwd", ba, route.bwd, known)
    assert _addr(fa[1]) == _addr(ba[1])                           # the workspace of the forward

    # one gradient per parameter, in named_parameters() order; none for an encoder's input, one for a decoder's
    (core,) = br.cores.values()
    for (k, p), (name, shape, off) in zip(mod.named_parameters(), core.state.table):
        assert name.endswith(k) and p.grad is not None
        assert torch.equal(p.grad, torch.arange(off + 1, off + p.numel() + 1, dtype=torch.float32).view(shape)), k
    if x.is_floating_point():
        assert (x.grad is not None) == ("dz" in route.bwd)


@pytest.mark.parametrize("rid", list(ROUTES))
def test_batchnorm_refusals(rid, monkeypatch):
    """Which modules refuse a training batch without a second value per channel, and that nobody else refuses one row."""
    route = ROUTES[rid]
    br = _Bridge(monkeypatch)
    mod = route.build(_family(route.family))
    if route.refuses is not None:
        with pytest.raises(ValueError, match="^%s$" % re.escape(BN_TEXT)):
            mod.train()(route.x(route.refuses))
        assert not [n for n in br.names() if n != "sync"]
        if route.refuses == 1:
            mod.eval()(route.x(1))                                 # the running statistics need no second row
    if route.refuses != 1:
        mod.train()(route.x(1))
        assert br.names()[-1] == route.base + "_fwd"


@pytest.mark.parametrize("rid,where,text", [
    ("mm.image_encoder", lambda m: m.classifier[2], "the HIP image encoder supports Dropout p in {0, 0.1} (reference: 0.1)"),
    ("celeba.image_encoder", lambda m: m.classifier[2], "the HIP image encoder supports Dropout p in {0, 0.1} (reference: 0.1)"),
    ("coco.image_encoder", lambda m: m.classifier[5], "the HIP image encoder supports Dropout p in {0, 0.1} on both layers (reference: 0.1)"),
    ("mm.text_decoder", lambda m: m.gru, "the HIP text decoder supports GRU dropout in {0, 0.1} (reference: 0.1)"),
    ("mmtext.decoder", lambda m: m.gru, "the HIP text decoder supports GRU dropout in {0, 0.1} (reference: 0.1)"),
    ("coco.text_decoder", lambda m: m.gru, "the HIP text decoder supports GRU dropout in {0, 0.1} (reference: 0.1)"),
])
def test_other_dropout_probabilities_are_refused(rid, where, text, monkeypatch):
    route = ROUTES[rid]
    br = _Bridge(monkeypatch)
    mod = route.build(_family(route.family)).train()
    layer = where(mod)
    setattr(layer, "dropout" if hasattr(layer, "dropout") else "p", 0.2)
    with pytest.raises(_lib.MMVAEError, match="^%s$" % re.escape(text)):
        mod(route.x(B))
    assert not [n for n in br.names() if n != "sync"]
    mod.eval()(route.x(B))                                         # no dropout, no refusal


@pytest.mark.parametrize("rid,text", [("mm.image_encoder", r"expected \(B,1,50,50\) images"), ("celeba.image_encoder", r"expected \(B,3,64,64\) images"),
                                      ("coco.image_encoder", r"expected \(B,3,32,32\) images \(coco/train.py:107-112\)"),
                                      ("mnist.image_encoder", r"expected \(B,784\) flattened images \(mnist/train.py:123\)"),
                                      ("mnist.VAE.encoder", r"expected \(B,784\) flattened images \(mnist/model.py:230\)"),
                                      ("mnist.text_encoder", r"expected \(B,\) digit labels"),
                                      ("coco.text_encoder", r"expected \(B, 3, 300\) caption tensors \(coco/utils.py:36-47\)")])
def test_shape_asserts_keep_their_text(rid, text, monkeypatch):
    route = ROUTES[rid]
    _Bridge(monkeypatch)
    mod = route.build(_family(route.family))
    bad = torch.zeros(B, 5, 7, 9, 11, dtype=route.x(B).dtype)
    with pytest.raises(AssertionError, match="^%s$" % text):
        mod(bad)


def test_shared_classes_are_the_ones_of_modules():
    from multimodal_vae_amd import celeba, coco, mnist, modules, multimnist
    assert multimnist.ProductOfExperts is modules.ProductOfExperts and mnist.ProductOfExperts is modules.ProductOfExperts
    assert celeba.ProductOfExperts is modules.ProductOfExperts and coco.ProductOfExperts is modules.ProductOfExperts
    assert multimnist.Swish is modules.Swish and celeba.Swish is modules.Swish and coco.Swish is modules.Swish
    assert multimnist.swish is modules.swish


def test_no_family_imports_from_multimnist():
    """``mnist``, ``celeba`` and ``coco`` take the shared plumbing from ``modules``: the fourth family file is not their library."""
    for fam in ("mnist", "celeba", "coco"):
        text = inspect.getsource(_family(fam))
        assert not re.search(r"^\s*(from\s+\.?multimnist\b|from\s+\.\s+import\s+.*\bmultimnist\b|import\s+.*\bmultimnist\b|"
                             r"from\s+multimodal_vae_amd(\.multimnist\b|\s+import\s+.*\bmultimnist\b))", text, re.M), fam
        assert re.search(r"^from \.modules import ", text, re.M), fam
