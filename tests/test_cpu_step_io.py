"""CPU tests of the Python side of the fused steps (no GPU, the library is never loaded): what the shared step-io filler writes for
each of the seven structs, the optimizer launcher's argument lists against the declared prototypes, the fast path's cache key,
``grad_ranges`` and the drivers' epoch helper."""
import ctypes as C
import inspect
import types

import pytest
import torch

from multimodal_vae_amd import _lib, core, train_common

B, T = 2, 3


class _State:
    """What an engine reads of a PlanState, on CPU tensors."""
    pack_pending = True
    _pack_text_only = True
    nparams = 16

    def __init__(self, api="mm"):
        self.API = api
        self.params, self.grads, self.gpk, self.gpk_vec = (torch.zeros(16) for _ in range(4))
        self._gmap = torch.zeros(16, dtype=torch.int32)
        self.table = [("image_encoder.a", (4,), 0), ("image_decoder.a", (2, 2), 4), ("image_decoder.b", (2,), 8),
                      ("text_encoder.a", (2,), 10), ("text_decoder.a", (4,), 12)]

    def grad_map(self):
        return self._gmap

    def defer_text_pack(self):
        self.pack_pending = True


def _engine(cls, api="mm"):
    """An engine of class ``cls`` without its constructor (which needs a device): the attributes the constructors set."""
    eng = object.__new__(cls)
    eng.state, eng.B, eng.T, eng.h = _State(api), B, T, 1
    eng.ws, eng.adam_state, eng.sums = torch.zeros(64, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64), torch.zeros(16)
    eng.exp_avg, eng.exp_avg_sq = torch.zeros(16), torch.zeros(16)
    eng.lr, eng.betas, eng.eps, eng.seed = 1e-3, (0.9, 0.999), 1e-8, 77
    eng.world_size, eng.all_reduce = 1, None
    eng.enc_dropout, eng.gru_dropout = True, False
    eng.kl_lambda, eng.lambda_x, eng.lambda_y, eng.kl_coef = 0.25, 0.5, 0.75, 0.125
    eng.sos = torch.zeros(300)
    eng.channels, eng.side, eng.pixels, eng.flat_images = 3, 64, 3 * 64 * 64, False
    eng._three_pass((1.0, 2.0, 3.0), (4.0, 5.0, 6.0))
    return eng


def _f32(*shape):
    return torch.zeros(*shape)


def _i64(*shape):
    return torch.zeros(*shape, dtype=torch.int64)


# engine class, plan family, where core looks the struct up, the required inputs
STEPS = [
    (core.FusedELBOStep, "mm", (core, "StepIO"), lambda: (_f32(B, 1, 50, 50), _i64(B, 4))),
    (core.FusedMnistStep, "mnist", (_lib, "MnistStepIO"), lambda: (_f32(B, 784), _i64(B))),
    (core.FusedCelebaStep, "celeba", (_lib, "CelebaStepIO"), lambda: (_f32(B, 3, 64, 64), _f32(B, 18))),
    (core.FusedCocoStep, "coco", (_lib, "CocoStepIO"), lambda: (_f32(B, 3, 32, 32), _f32(B, T, 300))),
    (core.FusedImageStep, "celeba", (_lib, "ImageStepIO"), lambda: (_f32(B, 3, 64, 64),)),
    (core.FusedTextStep, "coco", (_lib, "TextStepIO"), lambda: (_f32(B, T, 300),)),
    (core.FusedMMTextStep, "mmtext", (_lib, "MMTextStepIO"), lambda: (_i64(B, 4),)),
]


@pytest.mark.parametrize("cls,api,where,inputs", STEPS, ids=[s[2][1] for s in STEPS])
def test_the_filler_writes_every_field_of_the_struct(cls, api, where, inputs, monkeypatch):
    """forward_backward with every optional tensor given: each field of the family's struct is assigned, with the value the engine
    holds for it -- none is left to the struct's zero initialisation (a list of exceptions would go here; there are none)."""
    struct = getattr(*where)
    written = set()

    class Recording(struct):
        def __setattr__(self, k, v):
            written.add(k)
            super().__setattr__(k, v)

    monkeypatch.setattr(where[0], where[1], Recording)
    eng = _engine(cls, api)
    got = []
    eng._step = lambda entry, io, training, backward: got.append((entry, io))
    params = inspect.signature(eng.forward_backward).parameters
    n_in = len(inputs())
    optional = {k: _f32(4) for k, p in list(params.items())[n_in:] if p.default is None and not k.startswith(("passes", "lambda", "_"))}
    extra = {k: v for k, v in (("_defer_unpack", True), ("_dp_split", True), ("_early_adam", 4096)) if k in params}
    given = inputs()
    eng.forward_backward(*given, True, True, **optional, **extra)
    (entry, io), = got
    assert entry.startswith("mmvae_") and entry.endswith("step")
    fields = [n for n, _ in struct._fields_]
    assert sorted(written) == sorted(fields), set(fields) ^ written
    # ... and with the engine's values
    assert (io.ws, io.ws_bytes, io.step_counter, io.sums, io.seed) == (eng.ws.data_ptr(), 64, eng.adam_state.data_ptr(), eng.sums.data_ptr(), 77)
    for (name, _), t in zip(struct._fields_[3:], given):            # the required inputs lead the struct, in call order
        assert getattr(io, name) == t.data_ptr(), name
    for k, t in optional.items():
        assert getattr(io, k) == t.data_ptr(), k
    want = {"enc_dropout": 1, "gru_dropout": 0, "kl_lambda": 0.25, "kl_coef": 0.125, "defer_unpack": 1, "pack_first": 1, "dp_split": 1,
            "early_adam": 4096, "optimizer_state": eng.adam_state.data_ptr(), "sos": eng.sos.data_ptr()}
    types_ = dict(struct._fields_)
    for k, v in want.items():
        if k in types_:
            assert getattr(io, k) == v, k
    lambdas = [n for n, t in struct._fields_ if n.startswith("lambda")]
    if "pass_skip" in types_:
        assert [list(getattr(io, n)) for n in lambdas] == [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]] and list(io.pass_skip) == [0, 0, 0]
    else:
        assert [getattr(io, n) for n in lambdas] == [{"lambda_x": 0.5, "lambda_y": 0.75}[n] for n in lambdas]
    # absent optional tensors are NULL, and a forward-only call hands over no optimizer state
    got.clear()
    eng.forward_backward(*given, False, False)
    io = got[0][1]
    assert all(getattr(io, k) is None for k in optional)
    if "optimizer_state" in types_:
        assert io.optimizer_state is None


def _matches(value, ctype):
    if ctype is C.c_void_p:
        return value is None or isinstance(value, C.c_void_p)
    if ctype in (C.c_int, C.c_longlong):
        return isinstance(value, int)
    if ctype is C.c_float:
        return isinstance(value, float)
    return isinstance(value, C.Array) and value._type_ is ctype._type_         # POINTER(c_longlong) takes a c_longlong array


def test_optimizer_argument_lists_match_the_prototypes():
    eng = _engine(core.FusedELBOStep)
    ranges = (C.c_longlong * 4)(0, 4, 8, 8)
    seen = {}
    for kw in (dict(packed=False), dict(packed=False, n=8, grad_scale=0.5), dict(), dict(ranges=ranges)):
        name, args = eng._adam_args(**kw)
        _, argtypes = _lib.SIGNATURES[name]
        assert len(args) + 1 == len(argtypes) and argtypes[-1] is C.c_void_p, name         # + the trailing stream
        assert all(_matches(a, t) for a, t in zip(args, argtypes)), (name, args)
        seen[name] = args
    assert sorted(seen) == ["mmvae_adam_step", "mmvae_adam_step_packed", "mmvae_adam_step_packed_ranges"]
    assert seen["mmvae_adam_step"][4] == 8 and seen["mmvae_adam_step"][-1] == 0.5
    late = seen["mmvae_adam_step_packed_ranges"]
    assert late[5] is ranges and late[6:8] == (2, 1) and late[4] == 16


def test_fast_path_rebuilds_its_blocks_when_a_hyper_parameter_changes(monkeypatch):
    """The default-argument call caches the step-io block and both optimizer argument lists: betas, eps and the default lambdas
    are part of what it compares, as lr always was, and the in-step part of the update (mmvae_early_adam) follows."""
    calls = []

    def entry(name):
        def f(*args):
            calls.append((name, args))
            return 0
        return f
    fake = types.SimpleNamespace(**{n: entry(n) for n in ("mmvae_mm_step", "mmvae_adam_step_packed", "mmvae_adam_step_packed_ranges")})
    monkeypatch.setattr(_lib, "load", lambda: fake)
    monkeypatch.setattr(core, "_stream", lambda: None)
    eng = _engine(core.FusedELBOStep)
    eng._ea, eng._ea_ran, eng._ea_late = _lib.EarlyAdam(), C.c_int(1), (C.c_longlong * 2)(0, 8)
    image, text = _f32(B, 1, 50, 50), _i64(B, 4)
    eng._call_fast(image, text)
    first = eng._fast
    eng._call_fast(image, text)
    assert eng._fast is first and [c[0] for c in calls] == ["mmvae_mm_step", "mmvae_adam_step_packed_ranges"] * 2
    keys = {first[0]}
    for attr, value in (("betas", (0.5, 0.9)), ("eps", 1e-3), ("_LA", (1.0, 1.0, 1.0)), ("_LB", (0.0, 0.0, 1.0)), ("lr", 0.5)):
        setattr(eng, attr, value)
        del calls[:]
        eng._call_fast(image, text)
        assert eng._fast[0] not in keys, attr
        keys.add(eng._fast[0])
    assert abs(eng._ea.beta1 - 0.5) < 1e-7 and abs(eng._ea.beta2 - 0.9) < 1e-7 and abs(eng._ea.eps - 1e-3) < 1e-9 and eng._ea.lr == 0.5
    io = eng._fast[1]
    assert list(io.lambda_xy) == [1.0, 1.0, 1.0] and list(io.lambda_yx) == [0.0, 0.0, 1.0]
    late = calls[1][1]
    assert late[9:13] == (0.5, 0.5, 0.9, 1e-3)                    # lr, beta1, beta2, eps of mmvae_adam_step_packed_ranges
    eng._ea_ran.value = 0                                         # the step declined the early part: one launch over everything
    del calls[:]
    eng._call_fast(image, text)
    assert calls[1][0] == "mmvae_adam_step_packed" and calls[1][1][6:10] == (0.5, 0.5, 0.9, 1e-3)


def test_grad_ranges_twice():
    eng = _engine(core.FusedELBOStep)
    once = eng.grad_ranges()
    assert once == ([(4, 6), (12, 4)], [(0, 4), (10, 2)])
    assert eng.grad_ranges() == once


LOSSES = [7.0, 6.5, 6.0, 5.5, 5.0, 4.5, 4.0, 3.5]
# what train_imageonly's loop printed before the helper existed, for the first 7 of LOSSES, epoch 2, batch size 4, --log_interval 3
WANT_LINES = ["Train Epoch: 2 [0/28 (0%)]\tLoss: 7.000000",
              "Train Epoch: 2 [12/28 (43%)]\tLoss: 6.250000",
              "Train Epoch: 2 [24/28 (86%)]\tLoss: 5.500000"]


@pytest.mark.parametrize("n_batches,read_backs", [(7, 3), (8, 3 + 1)])
def test_train_epoch_prints_and_reads_back_like_the_drivers_loop(n_batches, read_backs, capsys, monkeypatch):
    counts = {"cpu": 0, "update": 0}
    real_cpu, real_update = torch.Tensor.cpu, train_common.AverageMeter.update

    def cpu(self, *a, **kw):
        counts["cpu"] += 1
        return real_cpu(self, *a, **kw)

    def update(self, val, n=1):
        counts["update"] += 1
        assert n == 4
        real_update(self, val, n)
    monkeypatch.setattr(torch.Tensor, "cpu", cpu)
    monkeypatch.setattr(train_common.AverageMeter, "update", update)
    loader = [(torch.tensor(v), None) for v in LOSSES[:n_batches]]
    epoch = 2
    avg, = train_common.train_epoch(
        loader, lambda b: b[0], 4, 3,
        lambda seen, n_total, pct, avg: 'Train Epoch: {} [{}/{} ({:.0f}%)]\tLoss: {:.6f}'.format(epoch, seen, n_total, pct, *avg),
        len(loader) * 4)
    lines = capsys.readouterr().out.splitlines()
    if n_batches == 7:
        assert lines == WANT_LINES and avg == 5.5
    else:
        assert lines == ["Train Epoch: 2 [0/32 (0%)]\tLoss: 7.000000", "Train Epoch: 2 [12/32 (38%)]\tLoss: 6.250000",
                         "Train Epoch: 2 [24/32 (75%)]\tLoss: 5.500000"] and avg == 5.25
    assert counts == {"cpu": read_backs, "update": n_batches}


def test_train_epoch_three_losses_and_eval_epoch():
    rows = [torch.tensor([1.0, 2.0, 3.0]) * k for k in (1, 2, 3)]
    logged = []
    avgs = train_common.train_epoch(rows, lambda b: b, 8, 10, lambda seen, n_total, pct, avg: (seen, n_total, avg), 999, 3, log=logged.append)
    assert avgs == (2.0, 4.0, 6.0) and logged == [(0, 999, (1.0, 2.0, 3.0))]
    assert train_common.eval_epoch(rows, lambda b: b, 3, "cpu") == [2.0, 4.0, 6.0]
    assert train_common.eval_epoch(rows, lambda b: b, 3, "cpu", reduce=lambda acc: acc / 2) == [1.0, 2.0, 3.0]
    assert train_common.eval_epoch([], lambda b: b, 1, "cpu") == [0.0]
    assert train_common.kl_lambdas(5e-4, (1e-5, 1e-4), 12, True) == [1e-5] * 5 + [1e-4] * 7
