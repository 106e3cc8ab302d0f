"""Device-side state of one MMVAE instance (MultiMNIST, MNIST, CelebA, COCO) and the fused ELBO-step engines.

PyTorch is used for plumbing only: it owns the device allocations (``torch.empty``), the stream and
(optionally) the HIP graph; every arithmetic operation of the hot path runs in libmmvae_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from ._lib import MMVAEError, StepIO, call, ptr
from ._ops import stream as _stream


class PlanState:
    """Flat parameter / gradient / BatchNorm-buffer storage plus the packed bf16 GEMM copies of the weights.

    The nn.Module face (``multimnist.MultimodalVAE`` ...) exposes views of ``params`` as its nn.Parameters, so
    ``optim.Adam(vae.parameters())``, ``state_dict()`` and the fused engine all see the same memory.
    ``API`` is the C-ABI prefix of the model family (mmvae_<API>_create ...)."""

    API = "mm"

    def _c(self, fn, *args):
        return call("mmvae_%s_%s" % (self.API, fn), *args)

    def __init__(self, n_latents: int, device: torch.device):
        if device.type != "cuda":
            raise MMVAEError("the MMVAE HIP engine needs a gfx950 GPU (device=%s); there is no CPU fallback" % device)
        _lib.init_device(device.index if device.index is not None else torch.cuda.current_device())
        self.device = device
        self.n_latents = int(n_latents)
        self._plans: Dict[int, int] = {}
        h = self._handle(1, bind=False)
        self.nparams = self._c("param_count", h)
        self.table: List[Tuple[str, Tuple[int, ...], int]] = []
        name = C.create_string_buffer(128)
        nd, off = C.c_int(), C.c_longlong()
        shape = (C.c_int * 4)()
        for i in range(self._c("num_params", h)):
            self._c("param_info", h, i, name, C.byref(nd), shape, C.byref(off))
            self.table.append((name.value.decode(), tuple(shape[k] for k in range(nd.value)), off.value))
        self.bn_table: List[Tuple[str, int, int]] = []
        ch = C.c_int()
        for i in range(self._c("num_bn", h)):
            self._c("bn_info", h, i, name, C.byref(ch), C.byref(off))
            self.bn_table.append((name.value.decode(), ch.value, off.value))
        f32 = dict(dtype=torch.float32, device=device)
        self.params = torch.zeros(self.nparams, **f32)
        self.grads = torch.zeros(self.nparams, **f32)
        self.bn_stats = torch.zeros(self._c("bn_floats", h), **f32)
        for _, c, o in self.bn_table:
            self.bn_stats[o + c:o + 2 * c] = 1.0                       # running_var = 1
        self.bn_nbt = torch.zeros(len(self.bn_table), dtype=torch.int64, device=device)
        self.packed = torch.zeros(self._c("packed_elems", h), dtype=torch.bfloat16, device=device)
        self.packed_vec = torch.zeros(self._c("packed_vec_elems", h), **f32)
        self.gpk = torch.zeros(self._c("gpk_elems", h), **f32)
        self.gpk_vec = torch.zeros(self._c("gpk_vec_elems", h), **f32)
        self._desc = []
        for which in (0, 1):
            nbytes = self._c("desc_bytes", h, which)
            host = torch.empty(nbytes, dtype=torch.uint8)
            self._c("desc_copy", h, which, C.c_void_p(host.data_ptr()))
            self._desc.append(host.to(device))
        self._bind(h)
        self.packed_version = -1          # bumped by whoever changes params

    # ---- plans -------------------------------------------------------------------------------------
    def _handle(self, batch: int, bind: bool = True) -> int:
        h = self._plans.get(batch)
        if h is None:
            h = self._c("create", self.n_latents, int(batch))
            if not h:
                raise MMVAEError("mmvae_%s_create failed: %s" % (self.API, _lib.load().mmvae_last_error().decode()))
            self._plans[batch] = h
            if bind:
                self._bind(h)
        return h

    def _bind(self, h: int) -> None:
        self._c("bind", h, ptr(self.params), ptr(self.grads), ptr(self.bn_stats), ptr(self.bn_nbt),
             ptr(self.packed), ptr(self.packed_vec), ptr(self.gpk), ptr(self.gpk_vec), ptr(self._desc[0]), ptr(self._desc[1]))

    def rebind(self) -> None:
        """Re-point every plan at the current buffers (after the module moved its flat storage)."""
        for h in self._plans.values():
            self._bind(h)

    def plan(self, batch: int) -> int:
        return self._handle(int(batch))

    def workspace_bytes(self, batch: int) -> int:
        return self._c("workspace_bytes", self.plan(batch))

    def module_workspace_bytes(self, batch: int) -> int:
        """Workspace of one granular module call (one pass over ``batch`` rows), not of the whole 3-pass step."""
        return self._c("module_workspace_bytes", self.plan(batch))

    def grad_map(self) -> torch.Tensor:
        """int32 [nparams]: where each flat parameter's packed gradient lives (mmvae_<family>_grad_map), built once."""
        if getattr(self, "_gmap", None) is None:
            m = torch.empty(self.nparams, dtype=torch.int32, device=self.device)
            self._c("grad_map", self.plan(1), ptr(m), _stream())
            self._gmap = m
        return self._gmap

    def pack_weights(self) -> None:
        self._c("pack_weights", self.plan(1), _stream())
        self.pack_pending = False

    # the parameters changed and the bf16 GEMM copies were not refreshed yet.  Whoever sets the flag owes a refresh of every pack;
    # defer_text_pack() narrows that to the caption half when nothing else is owed (the text-only step's own update).
    _pack_pending = False
    _pack_text_only = False

    @property
    def pack_pending(self) -> bool:
        return self._pack_pending

    @pack_pending.setter
    def pack_pending(self, v) -> None:
        self._pack_pending, self._pack_text_only = bool(v), False

    def defer_text_pack(self) -> None:
        """Only text_encoder.* / text_decoder.* changed: a step that refreshes the caption half's packs settles the debt."""
        only = self._pack_text_only or not self._pack_pending
        self._pack_pending, self._pack_text_only = True, only

    def ensure_packed(self) -> None:
        """Refresh the packed weights if an optimizer step deferred it (the MultiMNIST fused step folds the refresh into
        its own prologue launch; everybody else who reads the packed weights calls this first)."""
        if self.pack_pending:
            self.pack_weights()

    def view(self, name: str) -> torch.Tensor:
        for n, shape, off in self.table:
            if n == name:
                numel = 1
                for s in shape:
                    numel *= s
                return self.params[off:off + numel].view(shape)
        raise KeyError(name)

    def __del__(self):
        try:
            for h in self._plans.values():
                self._c("destroy", h)
        except Exception:
            pass


class MultimnistState(PlanState):
    """multimnist/model.py MultimodalVAE"""
    API = "mm"


class MultimnistTextState(PlanState):
    """multimnist/model.py:123-147 TextVAE: a plan of its own (parameters ``encoder.*`` / ``decoder.*``), the MMVAE's text kernels
    instantiated for ``n_hiddens`` = 50 (the reference's TextVAE) or 100 (the MMVAE's width).  No BatchNorm."""
    API = "mmtext"

    def __init__(self, n_latents: int, device: torch.device, n_hiddens: int = 50):
        self.n_hiddens = int(n_hiddens)
        super().__init__(n_latents, device)

    def _c(self, fn, *args):
        if fn == "create":
            return call("mmvae_mmtext_create", args[0], self.n_hiddens, args[1])
        return super()._c(fn, *args)

    def _bind(self, h: int) -> None:
        # the model has no BatchNorm: bind still wants two valid pointers
        if getattr(self, "_no_bn", None) is None:
            self._no_bn = (torch.zeros(4, dtype=torch.float32, device=self.device), torch.zeros(1, dtype=torch.int64, device=self.device))
        self._c("bind", h, ptr(self.params), ptr(self.grads), ptr(self._no_bn[0]), ptr(self._no_bn[1]),
                ptr(self.packed), ptr(self.packed_vec), ptr(self.gpk), ptr(self.gpk_vec), ptr(self._desc[0]), ptr(self._desc[1]))


class MnistState(PlanState):
    """mnist/model.py MultimodalVAE.  ``precision``: "fp32" (default: the reference's own arithmetic on fp32 MFMA) or
    "bf16" (bf16 MFMA operands like the conv models)."""
    API = "mnist"

    def __init__(self, n_latents: int, device: torch.device, precision: str = "fp32"):
        assert precision in ("fp32", "bf16")
        self.precision = precision
        super().__init__(n_latents, device)

    def _c(self, fn, *args):
        if fn == "create":
            return call("mmvae_mnist_create_p", *args, 0 if self.precision == "fp32" else 1)
        return super()._c(fn, *args)


class CelebaState(PlanState):
    """celeba/model.py MultimodalVAE"""
    API = "celeba"


class CocoState(PlanState):
    """coco/model.py MultimodalVAE.  ``steps``: caption length (coco/utils.py:12-15: 102)."""
    API = "coco"

    def __init__(self, n_latents: int, device: torch.device, steps: int = 102):
        self.steps = int(steps)
        super().__init__(n_latents, device)

    def _c(self, fn, *args):
        if fn == "create":
            return call("mmvae_coco_create_t", *args, self.steps)
        return super()._c(fn, *args)


class MnistInfoVAEState(PlanState):
    """mnist/model.py:238-279 InfoVAE: a small fp32 plan of its own (mmvae_mnist_infovae_*), the 12 tensors of its ``state_dict``
    flat in ``params`` (each starts 16-byte aligned: ``table`` offsets, not a running sum), every gradient in ``grads``.  No
    BatchNorm, no packed weight copies: ``pack_weights`` has nothing to do."""
    API = "mnist_infovae"

    def __init__(self, n_latents: int, device: torch.device):
        if device.type != "cuda":
            raise MMVAEError("the MMVAE HIP engine needs a gfx950 GPU (device=%s); there is no CPU fallback" % device)
        _lib.init_device(device.index if device.index is not None else torch.cuda.current_device())
        self.device = device
        self.n_latents = int(n_latents)
        self._plans: Dict[int, int] = {}
        h = self._handle(1, bind=False)
        self.nparams = self._c("param_count", h)
        self.table: List[Tuple[str, Tuple[int, ...], int]] = []
        name = C.create_string_buffer(128)
        nd, off = C.c_int(), C.c_longlong()
        shape = (C.c_int * 4)()
        for i in range(self._c("num_params", h)):
            self._c("param_info", h, i, name, C.byref(nd), shape, C.byref(off))
            self.table.append((name.value.decode(), tuple(shape[k] for k in range(nd.value)), off.value))
        self.bn_table: List[Tuple[str, int, int]] = []
        f32 = dict(dtype=torch.float32, device=device)
        self.params = torch.zeros(self.nparams, **f32)
        self.grads = torch.zeros(self.nparams, **f32)
        self.bn_stats = torch.zeros(4, **f32)
        self.bn_nbt = torch.zeros(1, dtype=torch.int64, device=device)
        self._bind(h)
        self.packed_version = -1

    def _bind(self, h: int) -> None:
        self._c("bind", h, ptr(self.params), ptr(self.grads))

    def workspace_bytes(self, batch: int) -> int:
        return self._c("step_workspace_bytes", self.plan(batch))

    module_workspace_bytes = workspace_bytes

    def grad_map(self):
        raise MMVAEError("the MNIST InfoVAE plan keeps no packed gradients")

    def pack_weights(self) -> None:
        self.pack_pending = False


class StepOutputs:
    """Lazy view of the loss sums of one fused step (no host sync until a value is read)."""

    def __init__(self, sums: torch.Tensor, bce_div: float, nll_div: float, kl_scale: float, lambda_xy, lambda_yx,
                 passes=(True, True, True)):
        self.sums, self.bce_div, self.nll_div, self.kl_scale = sums, bce_div, nll_div, kl_scale
        self.lxy, self.lyx = tuple(float(x) for x in lambda_xy), tuple(float(x) for x in lambda_yx)
        self.passes = tuple(bool(x) for x in passes)

    def losses(self) -> torch.Tensor:
        """loss_1, loss_2, loss_3 of the reference's train() closure as a device tensor [3]: the weighted sums that end each
        loss_function call (multimnist/train.py:33-62), evaluated by the library (mmvae_step_losses) on the step's stream --
        the weights travel as kernel arguments, nothing is synchronised."""
        s = self.sums
        w = [(C.c_float * 3)() for _ in range(3)]
        for k in range(3):
            on = 1.0 if self.passes[k] else 0.0                   # absent passes (weak supervision) report 0
            w[0][k] = on * self.lxy[k] / self.bce_div
            w[1][k] = on * self.lyx[k] / self.nll_div
            w[2][k] = on * self.kl_scale
        out = torch.empty(3, dtype=torch.float32, device=s.device)
        call("mmvae_step_losses", ptr(s), w[0], w[1], w[2], ptr(out), _stream())
        return out

    def check(self) -> None:
        """Synchronises, then raises MMVAEError if the step declared itself void (mmvae_step_status: a device-side exchange of
        the COCO caption decoder gave up; the optimizer update of that step was skipped on every rank)."""
        call("mmvae_step_status", ptr(self.sums), _stream())

    def parts(self):
        """(mean BCE, mean NLL, KL sum) per pass"""
        s = self.sums
        return s[0:3] / self.bce_div, s[4:7] / self.nll_div, s[8:11]


# fields that only some step-io structs have: the engine attribute of the same name / an argument of the call
_ENGINE_FIELDS = ("enc_dropout", "gru_dropout", "kl_lambda", "lambda_x", "lambda_y", "kl_coef", "lambda_mmd")
_CALL_FIELDS = ("defer_unpack", "pack_first", "optimizer_state", "dp_split", "early_adam")
_LAYOUTS: Dict[type, tuple] = {}


def _io_layout(cls) -> tuple:
    """What a step-io struct has of the optional fields, decided once per struct from ``_fields_``: (engine attributes it takes as a
    scalar, with the conversion), (per-call fields), (names of its two per-pass lambda arrays; none for a one-pass struct)."""
    lay = _LAYOUTS.get(cls)
    if lay is None:
        types = dict(cls._fields_)
        conv = {C.c_int: int, C.c_float: float}
        lay = _LAYOUTS[cls] = (tuple((n, conv[types[n]]) for n in _ENGINE_FIELDS if types.get(n) in conv),
                               tuple(n for n in _CALL_FIELDS if n in types),
                               tuple(n for n, t in cls._fields_ if t is C.c_float * 3))
    return lay


class _FusedStepBase:
    """zero_grad -> 3-pass forward -> 3 losses -> backward -> [grad all-reduce] -> Adam, as ONE enqueue of HIP kernels."""

    _DEFER_PACK = False         # the family's step prologue can refresh the packed weights itself (pack_first)
    separate_unpack = False     # tests: unpack the gradient + plain Adam instead of the packed-gradient Adam (same numbers)

    def __init__(self, state: PlanState, batch: int, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 seed: int = 1234, world_size: int = 1, all_reduce=None):
        self.state, self.B, self.D = state, int(batch), state.n_latents
        self.lr, self.betas, self.eps, self.seed = lr, betas, eps, seed
        self.world_size, self.all_reduce = world_size, all_reduce
        if self._dp_active():
            # the collective library may enqueue on a stream of its own: mixed stream priorities then slow the whole
            # process down (include/mmvae_hip.h: mmvae_set_stream_policy)
            call("mmvae_set_stream_policy", 1)
        dev = state.device
        self.h = state.plan(batch)
        self.ws = torch.empty(self._workspace_bytes(state, batch), dtype=torch.uint8, device=dev)
        self.exp_avg = torch.zeros_like(state.params)
        self.exp_avg_sq = torch.zeros_like(state.params)
        self.adam_state = torch.zeros(2, dtype=torch.int64, device=dev)      # {step, ticket}
        self.sums = torch.zeros(16, dtype=torch.float32, device=dev)
        self._graph = None
        state.pack_weights()

    def _outputs(self) -> StepOutputs:
        raise NotImplementedError

    def _workspace_bytes(self, state: PlanState, batch: int) -> int:
        return state.workspace_bytes(batch)

    def _three_pass(self, lambda_a, lambda_b) -> None:
        """The default per-pass loss weights of a 3-pass family."""
        self._LA, self._LB = lambda_a, lambda_b
        self._last = ((True, True, True), lambda_a, lambda_b)

    def _pass_config(self, io, passes, la, lb, name_a, name_b):
        """Fills the lambda arrays and pass_skip flags of a step-io struct; returns (passes, lambda_a, lambda_b)."""
        passes = (True, True, True) if passes is None else tuple(bool(x) for x in passes)
        assert len(passes) == 3 and any(passes), "at least one of the three passes must be present"
        la = tuple(float(x) for x in (self._LA if la is None else la))
        lb = tuple(float(x) for x in (self._LB if lb is None else lb))
        setattr(io, name_a, (C.c_float * 3)(*la))
        setattr(io, name_b, (C.c_float * 3)(*lb))
        io.pass_skip = (C.c_int * 3)(*[0 if x else 1 for x in passes])
        self._last = (passes, la, lb)
        return passes, la, lb

    def _io(self, cls, inputs, optional, backward=True, passes=None, lambda_a=None, lambda_b=None, defer_unpack=False,
            dp_split=False, early_adam=None):
        """One filled step-io struct of type ``cls``: the engine's workspace, counters, seed and loss sums; the required ``inputs``
        ((field, tensor) pairs); every ``optional`` tensor ({field: tensor or None}, NULL when absent); and whatever ``cls`` has of
        the fields that only some families know (``_io_layout``)."""
        scalars, per_call, lambdas = _io_layout(cls)
        io = cls()
        io.ws, io.ws_bytes = self.ws.data_ptr(), self.ws.numel()
        io.step_counter = self.adam_state.data_ptr()
        io.seed = self.seed
        io.sums = self.sums.data_ptr()
        for k, t in inputs:
            setattr(io, k, t.data_ptr())
        for k, t in optional.items():
            setattr(io, k, None if t is None else t.data_ptr())
        for k, conv in scalars:
            setattr(io, k, conv(getattr(self, k)))
        if lambdas:
            self._pass_config(io, passes, lambda_a, lambda_b, *lambdas)
        values = {"defer_unpack": int(bool(defer_unpack)), "pack_first": int(self.state.pack_pending), "dp_split": int(bool(dp_split)),
                  "early_adam": early_adam,
                  # (a void step, the exchange time-out of the caption decoder, skips its Adam update)
                  "optimizer_state": self.adam_state.data_ptr() if backward else None}
        for k in per_call:
            setattr(io, k, values[k])
        return io

    def _step(self, entry: str, io, training, backward) -> StepOutputs:
        """Enqueues the family's step.  optimizer.zero_grad() happens inside its prologue kernel when backward is requested; a
        prologue that was asked to (pack_first) has refreshed the packed weights."""
        call(entry, self.h, C.byref(io), int(training), int(backward), _stream())
        if self._DEFER_PACK:
            self.state.pack_pending = False
        return self._outputs()

    # -- optimizer --------------------------------------------------------------------------------------
    def _adam_args(self, ranges=None, packed=True, n=None, grad_scale=1.0):
        """(entry point, its arguments up to the trailing stream) of one optimizer launch.  ``packed``: the GEMM-weight gradients are
        still in their packed layout and the kernel gathers them (and completes ``grads``) itself, over everything or over the
        (offset, length) pairs of the ``c_longlong`` array ``ranges``; else plain Adam over the first ``n`` elements (default: all)."""
        st = self.state
        bufs = (ptr(st.params), ptr(st.grads), ptr(self.exp_avg), ptr(self.exp_avg_sq), st.nparams if n is None else n)
        hyper = (ptr(self.adam_state), self.lr, self.betas[0], self.betas[1], self.eps, grad_scale)
        if not packed:
            return "mmvae_adam_step", bufs + hyper
        gathered = (ptr(st.grad_map()), ptr(st.gpk), ptr(st.gpk_vec))
        if ranges is None:
            return "mmvae_adam_step_packed", bufs + hyper + gathered
        return "mmvae_adam_step_packed_ranges", bufs + (ranges, len(ranges) // 2, 1) + hyper + gathered       # (1: the step count advances)

    def _adam(self, **kw) -> None:
        name, args = self._adam_args(**kw)
        call(name, *args, _stream())

    def optimizer_step(self) -> None:
        """torch.optim.Adam(lr) semantics on the flat buffers, then refresh the packed bf16 weights."""
        if self._dp_active():
            self.all_reduce(self.state.grads)                          # sum over ranks (RCCL), scaled inside Adam
        self._adam(packed=False, grad_scale=1.0 / self.world_size)
        self._after_update()

    def _after_update(self) -> None:
        if self._DEFER_PACK:
            self.state.pack_pending = True
        else:
            self.state.pack_weights()

    def _dp_active(self) -> bool:
        """The data-parallel exchange is on: more than one rank, or a collective that asks to run even on one rank
        (``all_reduce.force``: the single-rank RCCL test that puts this branch on hardware)."""
        return self.all_reduce is not None and (self.world_size > 1 or bool(getattr(self.all_reduce, "force", False)))

    def __call__(self, a, b, **kw) -> StepOutputs:
        out = self.forward_backward(a, b, True, True, **kw)
        self.optimizer_step()
        return out

    def _call_packed(self, a, b, **kw) -> StepOutputs:
        """backward + optimizer.step() (multimnist/train.py:168,173) in one pass over the parameters: the GEMM-weight
        gradients stay in their packed layout and the Adam kernel gathers them (and completes ``grads``) itself.  The
        data-parallel path needs the complete flat gradient BEFORE Adam (all-reduce), so it keeps the separate unpack."""
        if self._dp_active() or self.separate_unpack:
            return _FusedStepBase.__call__(self, a, b, **kw)
        out = self.forward_backward(a, b, True, True, _defer_unpack=True, **kw)
        self._adam()
        self._after_update()
        return out

    # -- HIP graph ------------------------------------------------------------------------------------
    def capture(self, a: torch.Tensor, b: torch.Tensor) -> None:
        """Capture the whole step (static input buffers) into a HIP graph; ``replay()`` launches it."""
        self._static = (a, b)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):          # warm-up: sets kernel attributes, primes the allocator
                self(a, b)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self(a, b)
        self._graph = g

    def replay(self) -> StepOutputs:
        self._graph.replay()
        return self._outputs()


class FusedELBOStep(_FusedStepBase):
    """The 3-pass ELBO step of multimnist/train.py:146-173."""

    LAMBDA_XY = (1.0, 1.0, 0.0)
    LAMBDA_YX = (1.0, 0.5, 1.0)
    _DEFER_PACK = True

    def __init__(self, state: PlanState, batch: int, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 kl_lambda: float = 1e-3, seed: int = 1234, world_size: int = 1, all_reduce=None):
        super().__init__(state, batch, lr, betas, eps, seed, world_size, all_reduce)
        self.kl_lambda = kl_lambda
        self.enc_dropout = self.gru_dropout = True
        self._three_pass(self.LAMBDA_XY, self.LAMBDA_YX)

    def _outputs(self) -> StepOutputs:
        passes, lxy, lyx = self._last
        return StepOutputs(self.sums, self.B * 2500, self.B * 4, self.kl_lambda / self.B, lxy, lyx, passes)

    def forward_backward(self, image, text, training=True, backward=True, eps=None, enc_mask1=None, enc_mask2=None,
                         gru_keep=None, force_tokens=None, recon_image=None, recon_text=None, mu=None, logvar=None,
                         tokens=None, passes=None, lambda_xy=None, lambda_yx=None, _defer_unpack=False, _dp_split=False,
                         _early_adam=None) -> StepOutputs:
        """``passes`` = which of (joint, image-only, text-only) exist in this step and ``lambda_xy/lambda_yx`` = their loss
        weights: the weak-supervision steps of multimnist/paired_weak.py:84-117 and modal_weak.py:87-117."""
        assert image.is_contiguous() and text.is_contiguous() and image.dtype == torch.float32 and text.dtype == torch.int64
        assert image.shape[0] == self.B and text.shape == (self.B, 4)
        io = self._io(StepIO, (("image", image), ("text", text)),
                      dict(eps=eps, enc_mask1=enc_mask1, enc_mask2=enc_mask2, gru_keep=gru_keep, force_tokens=force_tokens,
                           recon_image=recon_image, recon_text=recon_text, mu=mu, logvar=logvar, tokens=tokens),
                      backward, passes, lambda_xy, lambda_yx, _defer_unpack, _dp_split, _early_adam)
        return self._step("mmvae_mm_step", io, training, backward)

    # -- data parallelism: the decoders' gradients are exchanged while the encoders' backward still runs -------------
    EARLY_PREFIXES = ("image_decoder.", "text_decoder.")     # what mmvae_mm_step_io.dp_split completes early
    _dp_ranges = None

    def grad_ranges(self):
        """(early, late): lists of (offset, length) runs of the flat gradient buffer, early = complete at the event of
        ``mmvae_mm_wait_early_grads``.  Adjacent parameters of the same kind are merged: a few large messages."""
        runs = ([], [])
        end, last_kind = 0, None
        for name, shape, off in self.state.table:
            n = 1
            for d in shape:
                n *= int(d)
            kind = 0 if name.startswith(self.EARLY_PREFIXES) else 1
            r = runs[kind]
            if r and r[-1][0] + r[-1][1] == off and last_kind == kind:
                r[-1] = (r[-1][0], r[-1][1] + n)
            else:
                r.append((off, n))
            last_kind = kind
            end = max(end, off + n)
        assert end == self.state.nparams
        return runs

    def _call_dp_overlap(self, image, text, **kw) -> StepOutputs:
        """One data-parallel step with the gradient exchange in two parts: the early ranges are all-reduced on a
        communication stream ordered behind the step's early-gradient event (they overlap latent/encoder backward and the
        encoders' weight gradients), the late ranges after the step; Adam (1/world folded in) waits for both.

        Opt-in (``GradAllReduce(overlap=True)``), correct (tests/test_gpu_configs_r2.py) but NOT faster on this runtime: a
        stream parked on an event occupies its hardware queue, and when the runtime maps the communication stream onto a
        queue shared with one of the step's streams the step stalls behind it (0.91 -> 2.2 ms measured with a world-1 RCCL
        group, GPU_MAX_HW_QUEUES=8).  The plain exchange after the step is the default."""
        st = self.state
        if self._dp_ranges is None:
            self._dp_ranges = self.grad_ranges()
            self._comm_owner = _lib.OwnedStream(st.device)      # (not torch.cuda.Stream(): see _lib.OwnedStream)
            self._comm = self._comm_owner.stream
        early, late = self._dp_ranges
        out = self.forward_backward(image, text, True, True, _dp_split=True, **kw)
        # async collectives: the library's stream is ordered behind the stream that is current at the call (the
        # communication stream, whose only content is the wait for the early-gradient event, for the early ranges; the main
        # stream for the late ones) and Work.wait() orders the main stream behind the results.  NOT main.wait_stream(comm):
        # an event recorded on a stream that holds nothing but a pending wait costs ~1.3 ms per step on this runtime.
        works = []
        call("mmvae_mm_wait_early_grads", self.h, C.c_void_p(self._comm.cuda_stream))
        with torch.cuda.stream(self._comm):
            for off, n in early:
                works.append(self.all_reduce(st.grads[off:off + n], async_op=True))
        for off, n in late:
            works.append(self.all_reduce(st.grads[off:off + n], async_op=True))
        for w in works:
            if w is not None:
                w.wait()
        self._adam(packed=False, grad_scale=1.0 / self.world_size)
        self._after_update()
        return out

    early_adam = True       # the decoders' Adam update is issued inside the step, beside the encoders' backward (mmvae_early_adam)
    _ea = _ea_ran = _fast = None

    def _early_setup(self):
        """ctypes block handed to mmvae_mm_step_io.early_adam + the ranges the call behind the step still has to update."""
        st = self.state
        rg = (C.c_longlong * 8)()
        n = call("mmvae_mm_early_ranges", self.h, rg, 4)
        early = [(int(rg[2 * i]), int(rg[2 * i + 1])) for i in range(n)]
        late, pos = [], 0
        for off, ln in sorted(early):
            if off > pos:
                late.append((pos, off - pos))
            pos = off + ln
        if pos < st.nparams:
            late.append((pos, st.nparams - pos))
        self._ea_ran = C.c_int(0)
        ea = _lib.EarlyAdam()
        ea.m, ea.v, ea.state = self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.adam_state.data_ptr()
        ea.grad_scale = 1.0
        ea.gmap = st.grad_map().data_ptr()
        ea.ran = C.pointer(self._ea_ran)
        self._ea = ea
        self._ea_late = (C.c_longlong * (2 * len(late)))(*[x for r in late for x in r])
        self._ea_ok = 0 < n and 0 < len(late) <= 4 and all(o % 4 == 0 and l % 4 == 0 for o, l in late[:-1]) and late[-1][0] % 4 == 0

    def _early_hyper(self) -> None:
        """The optimizer's hyper-parameters as the in-step part of the update reads them."""
        ea = self._ea
        ea.lr, ea.beta1, ea.beta2, ea.eps = self.lr, self.betas[0], self.betas[1], self.eps

    def _call_packed(self, image, text, **kw) -> StepOutputs:
        """backward + optimizer.step() with the decoders' part of the update inside the step (multimnist/train.py:168,173)."""
        if self._dp_active() or self.separate_unpack or not self.early_adam:
            return _FusedStepBase._call_packed(self, image, text, **kw)
        if self._ea is None:
            self._early_setup()
        if not self._ea_ok:
            return _FusedStepBase._call_packed(self, image, text, **kw)
        if not kw:
            return self._call_fast(image, text)
        self._early_hyper()
        self._fast = None           # (the fast path writes that block only when its key changes: make it look again)
        out = self.forward_backward(image, text, True, True, _defer_unpack=True, _early_adam=C.addressof(self._ea), **kw)
        # the step updated image_decoder.* / text_decoder.* (then: the rest, and the step count) or declined to
        self._adam(ranges=self._ea_late if self._ea_ran.value else None)
        self._after_update()
        return out

    def _call_fast(self, image, text) -> StepOutputs:
        """The training loop's call with default arguments: the step-io block and the optimizer calls' argument lists are built
        once and only the fields that change are written (input pointers, pack_first, the stream).  The enqueue thread's Python
        time per step is what makes a loader-fed loop host-bound: 49 launches are 250 us of runtime calls,
        filling a 30-field ctypes structure and converting 18 arguments per call was another 60."""
        st = self.state
        fast = self._fast
        key = (self.enc_dropout, self.gru_dropout, self.kl_lambda, self.seed, self.lr, tuple(self.betas), self.eps, self._LA, self._LB)
        if fast is None or fast[0] != key:      # everything the cached blocks below hold by value
            self._early_hyper()
            io = self._io(StepIO, (), {}, defer_unpack=True, early_adam=C.addressof(self._ea))
            lib = _lib.load()
            (n_late, late), (n_full, full) = self._adam_args(ranges=self._ea_late), self._adam_args()
            fast = self._fast = (key, io, C.byref(io), lib.mmvae_mm_step, getattr(lib, n_late), getattr(lib, n_full), late, full, lib)
        _, io, io_ref, f_step, f_late, f_full, late, full, lib = fast
        assert image.is_contiguous() and text.is_contiguous() and image.dtype == torch.float32 and text.dtype == torch.int64
        assert image.shape[0] == self.B and text.shape == (self.B, 4)
        self._last = ((True, True, True), self._LA, self._LB)
        io.image, io.text = image.data_ptr(), text.data_ptr()
        io.pack_first = int(st.pack_pending)
        stream = _stream()
        rc = f_step(self.h, io_ref, 1, 1, stream)
        if rc != 0:
            raise _lib.MMVAEError("mmvae_mm_step failed (%d): %s" % (rc, lib.mmvae_last_error().decode()))
        st.pack_pending = False
        rc = f_late(*late, stream) if self._ea_ran.value else f_full(*full, stream)
        if rc != 0:
            raise _lib.MMVAEError("optimizer launch failed (%d): %s" % (rc, lib.mmvae_last_error().decode()))
        self._after_update()
        return self._outputs()

    def __call__(self, image, text, **kw) -> StepOutputs:
        if self._dp_active() and getattr(self.all_reduce, "overlap", False):
            return self._call_dp_overlap(image, text, **kw)
        return self._call_packed(image, text, **kw)


class FusedMnistStep(_FusedStepBase):
    """The 3-pass step of mnist/train.py:131-147 (all lambdas 1, KL divided by B*784/3, no annealing)."""

    LAMBDA_XY = (1.0, 1.0, 1.0)
    LAMBDA_YX = (1.0, 1.0, 1.0)

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.kl_coef = 1.0 / (self.B * (784 / 3))
        self._three_pass(self.LAMBDA_XY, self.LAMBDA_YX)

    def _outputs(self) -> StepOutputs:
        passes, lxy, lyx = self._last
        return StepOutputs(self.sums, self.B * 784, self.B, self.kl_coef, lxy, lyx, passes)

    def forward_backward(self, image, label, training=True, backward=True, eps=None, recon_image=None, recon_text=None,
                         mu=None, logvar=None, passes=None, lambda_xy=None, lambda_yx=None) -> StepOutputs:
        assert image.is_contiguous() and label.is_contiguous() and image.dtype == torch.float32 and label.dtype == torch.int64
        assert image.numel() == self.B * 784 and label.shape == (self.B,)
        io = self._io(_lib.MnistStepIO, (("image", image), ("label", label)),
                      dict(eps=eps, recon_image=recon_image, recon_text=recon_text, mu=mu, logvar=logvar),
                      backward, passes, lambda_xy, lambda_yx)
        return self._step("mmvae_mnist_step", io, training, backward)


class FusedCelebaStep(_FusedStepBase):
    """The 3-pass step of celeba/train.py:131-147 (loss_function defaults: lambdas 1, kl_lambda 1e-3)."""

    LAMBDA_X = (1.0, 1.0, 1.0)
    LAMBDA_Y = (1.0, 1.0, 1.0)
    N_ATTRS = 18

    def __init__(self, state: PlanState, batch: int, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 kl_lambda: float = 1e-3, seed: int = 1234, world_size: int = 1, all_reduce=None):
        super().__init__(state, batch, lr, betas, eps, seed, world_size, all_reduce)
        self.kl_lambda = kl_lambda
        self.enc_dropout = True
        self._three_pass(self.LAMBDA_X, self.LAMBDA_Y)

    def _outputs(self) -> StepOutputs:
        passes, lx, ly = self._last
        return StepOutputs(self.sums, self.B * 3 * 64 * 64, self.B * self.N_ATTRS, self.kl_lambda / self.B, lx, ly, passes)

    def __call__(self, image, attrs, **kw) -> StepOutputs:
        return self._call_packed(image, attrs, **kw)

    def forward_backward(self, image, attrs, training=True, backward=True, eps=None, enc_mask=None, recon_image=None,
                         recon_attrs=None, mu=None, logvar=None, passes=None, lambda_x=None, lambda_y=None,
                         _defer_unpack=False) -> StepOutputs:
        assert image.is_contiguous() and attrs.is_contiguous() and image.dtype == torch.float32 and attrs.dtype == torch.float32
        assert image.shape == (self.B, 3, 64, 64) and attrs.shape == (self.B, self.N_ATTRS)
        io = self._io(_lib.CelebaStepIO, (("image", image), ("attrs", attrs)),
                      dict(eps=eps, enc_mask=enc_mask, recon_image=recon_image, recon_attrs=recon_attrs, mu=mu, logvar=logvar),
                      backward, passes, lambda_x, lambda_y, _defer_unpack)
        return self._step("mmvae_celeba_step", io, training, backward)


class FusedCocoStep(_FusedStepBase):
    """The 3-pass step of coco/train.py:138-173 (lambda_xy = (1,1,0), lambda_yx = (1,1,1), kl_lambda 1e-3)."""

    LAMBDA_XY = (1.0, 1.0, 0.0)
    LAMBDA_YX = (1.0, 1.0, 1.0)
    EMB = 300
    _DEFER_PACK = True          # the step refreshes the packed weights itself, the two halves on their own streams

    def __init__(self, state: PlanState, batch: int, sos: torch.Tensor, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 kl_lambda: float = 1e-3, seed: int = 1234, world_size: int = 1, all_reduce=None):
        super().__init__(state, batch, lr, betas, eps, seed, world_size, all_reduce)
        self.kl_lambda = kl_lambda
        self.T = state.steps
        self.sos = sos.to(device=state.device, dtype=torch.float32).contiguous().reshape(self.EMB)
        self.enc_dropout = self.gru_dropout = True
        self._three_pass(self.LAMBDA_XY, self.LAMBDA_YX)

    def _outputs(self) -> StepOutputs:
        passes, lxy, lyx = self._last
        return StepOutputs(self.sums, self.B * 3 * 32 * 32, self.B * self.T * self.EMB, self.kl_lambda / self.B, lxy, lyx, passes)

    def __call__(self, image, text, **kw) -> StepOutputs:
        return self._call_packed(image, text, **kw)

    def forward_backward(self, image, text, training=True, backward=True, eps=None, enc_mask1=None, enc_mask2=None,
                         gru_keep=None, recon_image=None, recon_text=None, mu=None, logvar=None, passes=None,
                         lambda_xy=None, lambda_yx=None, _defer_unpack=False) -> StepOutputs:
        assert image.is_contiguous() and text.is_contiguous() and image.dtype == torch.float32 and text.dtype == torch.float32
        assert image.shape == (self.B, 3, 32, 32) and text.shape == (self.B, self.T, self.EMB)
        io = self._io(_lib.CocoStepIO, (("image", image), ("text", text), ("sos", self.sos)),
                      dict(eps=eps, enc_mask1=enc_mask1, enc_mask2=enc_mask2, gru_keep=gru_keep, recon_image=recon_image,
                           recon_text=recon_text, mu=mu, logvar=logvar),
                      backward, passes, lambda_xy, lambda_yx, _defer_unpack)
        return self._step("mmvae_coco_step", io, training, backward)


class _SinglePassStep(_FusedStepBase):
    """A uni-modal baseline's step: zero_grad -> ONE pass over B rows (one encoder, reparametrize, one decoder; no product of
    experts) -> backward -> Adam over that modality's parameters, ``self._ranges`` ((offset, length) as a ``c_longlong`` pair) when
    they are a 4-aligned part of the flat buffers, else over everything (the other half's gradient is exactly 0)."""

    _KIND = ""              # "image-only" / "text-only", for messages
    _ranges = None
    _packed, _adam_n = True, None       # MNIST: plain Adam over the leading ``_adam_n`` elements

    IMAGE_PREFIXES = ("image_encoder.", "image_decoder.")

    def _image_range(self, state, restrict: bool = True) -> int:
        """The image half is one run at the head of the flat buffers in every family: its length (``n_image_params``); ``restrict``:
        the optimizer visits nothing else (``_ranges``) when the run is 4-aligned and not the whole buffer."""
        n_img = 0
        for name, shape, off in state.table:
            if name.startswith(self.IMAGE_PREFIXES):
                n = 1
                for d in shape:
                    n *= int(d)
                assert off == n_img, "the image parameters are expected to be contiguous at the head of the table"
                n_img = off + n
        self.n_image_params = n_img
        if restrict and n_img % 4 == 0 and 0 < n_img < state.nparams:
            self._ranges = (C.c_longlong * 2)(0, n_img)
        return n_img

    def evaluate(self, x, **kw) -> StepOutputs:
        """Eval-mode forward (z = mu, no dropout, nothing drawn), no backward."""
        return self.forward_backward(x, False, False, **kw)

    def __call__(self, x, **kw) -> StepOutputs:
        """backward + optimizer.step() in one pass over the modality's parameters: the packed-gradient Adam (see _call_packed)."""
        if self.separate_unpack and self._packed:
            out = self.forward_backward(x, True, True, **kw)
            self.optimizer_step()
            return out
        out = self.forward_backward(x, True, True, _defer_unpack=self._packed, **kw)
        self._adam(ranges=self._ranges, packed=self._packed, n=self._adam_n)
        self._after_update()
        return out

    def capture(self, x: torch.Tensor) -> None:
        raise MMVAEError("%s: HIP-graph capture is not offered for the %s step" % (type(self).__name__, self._KIND))


class FusedImageStep(_SinglePassStep):
    """The step of celeba/train_imageonly.py:95-113, coco/train_imageonly.py, multimnist/train_imageonly.py:91-106 and
    mnist/imageonly/train_imageonly.py:114-127 on the family's plan: zero_grad -> ONE pass over B rows (image encoder, reparametrize,
    image decoder; no product of experts) -> lambda_x * BCE + kl_lambda * KL / B -> backward -> Adam.  ``state`` is a ``CelebaState``, a
    ``CocoState``, a ``MultimnistState`` or a fp32 ``MnistState``; the second modality's parameters keep their values and get a gradient
    of exactly 0.  ``StepOutputs`` slot 0 carries the pass.  MNIST images may come as (B, 1, 28, 28) or flattened (B, 784); its plan
    keeps no packed gradients, so its optimizer is the plain Adam kernel over the leading image parameters."""

    SIDE = {"celeba": 64, "coco": 32, "mm": 50, "mnist": 28}
    CHANNELS = {"celeba": 3, "coco": 3, "mm": 1, "mnist": 1}
    FAMILIES = "CelebA, COCO and MultiMNIST have one, MNIST has one on its fp32 plan"
    _KIND = "image-only"
    flat_images = False         # MNIST: (B, 784) batches are taken too

    def __init__(self, state: PlanState, batch: int, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 kl_lambda: float = 1e-3, lambda_x: float = 1.0, seed: int = 1234):
        if state.API not in self.SIDE:
            raise MMVAEError("FusedImageStep: no image-only step for the '%s' family (%s)" % (state.API, self.FAMILIES))
        if state.API == "mnist" and getattr(state, "precision", None) != "fp32":     # the baseline is the reference's fp32 model
            raise MMVAEError("FusedImageStep: no image-only step for the 'mnist' family at precision %r (%s)"
                             % (getattr(state, "precision", None), self.FAMILIES))
        super().__init__(state, batch, lr, betas, eps, seed)
        self.kl_lambda, self.lambda_x = kl_lambda, lambda_x
        self.enc_dropout = True
        self.side, self.channels = self.SIDE[state.API], self.CHANNELS[state.API]
        self.pixels = self.channels * self.side * self.side      # per image: the BCE is a mean over B * pixels
        self.flat_images = state.API == "mnist"
        n_img = self._image_range(state, restrict=state.API != "mnist")
        if state.API == "mnist":        # the fp32 plan writes every gradient into ``grads``
            self._packed, self._adam_n = False, n_img

    def _workspace_bytes(self, state: PlanState, batch: int) -> int:
        return state._c("image_step_workspace_bytes", state.plan(batch))

    def _outputs(self) -> StepOutputs:
        return StepOutputs(self.sums, self.B * self.pixels, 1.0, self.kl_lambda / self.B, (self.lambda_x, 0.0, 0.0),
                           (0.0, 0.0, 0.0), (True, False, False))

    def forward_backward(self, image, training=True, backward=True, eps=None, enc_mask1=None, enc_mask2=None, recon_image=None,
                         mu=None, logvar=None, _defer_unpack=False) -> StepOutputs:
        assert image.is_contiguous() and image.dtype == torch.float32
        # (MNIST batches may come flattened, as the reference's x.view(-1, 784) takes them)
        flat_ok = self.flat_images and tuple(image.shape) == (self.B, self.channels * self.side * self.side)
        if tuple(image.shape) != (self.B, self.channels, self.side, self.side) and not flat_ok:
            raise MMVAEError("FusedImageStep: expected images of shape %s (got %s)"
                             % ((self.B, self.channels, self.side, self.side), tuple(image.shape)))
        io = self._io(_lib.ImageStepIO, (("image", image),),
                      dict(eps=eps, enc_mask1=enc_mask1, enc_mask2=enc_mask2, recon_image=recon_image, mu=mu, logvar=logvar),
                      backward, defer_unpack=_defer_unpack)
        return self._step("mmvae_%s_image_step" % self.state.API, io, training, backward)


class InfoVAEStepOutputs(StepOutputs):
    """``StepOutputs`` of the InfoVAE step: slot 0 carries the pass, the loss sums' slots 12..15 the MMD term
    ({mean Kxx, mean Kyy, mean Kxy, MMD}, include/mmvae_hip.h MMVAE_SUM_MMD_*)."""

    MMD_SLOTS = slice(12, 16)

    def __init__(self, sums, bce_div, kl_scale, lambda_x, lambda_mmd):
        super().__init__(sums, bce_div, 1.0, kl_scale, (lambda_x, 0.0, 0.0), (0.0, 0.0, 0.0), (True, False, False))
        self.lambda_mmd = float(lambda_mmd)

    def bce(self) -> torch.Tensor:
        """mean BCE (0-d device tensor)"""
        return self.sums[0] / self.bce_div

    def mmd(self) -> torch.Tensor:
        """MMD(prior samples, z) (0-d device tensor)"""
        return self.sums[15]

    def mmd_terms(self) -> torch.Tensor:
        """{mean Kxx, mean Kyy, mean Kxy, MMD}"""
        return self.sums[self.MMD_SLOTS]

    def total(self) -> torch.Tensor:
        """lambda_x * mean BCE + lambda_mmd * MMD + kl_lambda * KL / B: the reference's one ``Loss:`` figure at its weights (1, 1, 0)"""
        return self.losses()[0]

    def losses(self) -> torch.Tensor:
        out = super().losses()
        out[0] += self.lambda_mmd * self.sums[15]
        return out


class FusedInfoVAEStep(_SinglePassStep):
    """The step of coco/train_infovae.py:113-128 on the COCO plan: zero_grad -> ONE pass over B rows (image encoder, reparametrize,
    image decoder) -> lambda_x * mean BCE + lambda_mmd * MMD(prior samples, z) + kl_lambda * KL / B -> backward -> Adam over the image
    parameters, one enqueue (mmvae_coco_infovae_step: the image-only step with the MMD sweep beside the decoder).  ``state`` is a
    ``CocoState``; the caption half keeps its values and gets a gradient of exactly 0.  The reference's loss is the default
    (1, 1, 0).  On a ``MnistInfoVAEState`` it is the step of mnist/train_infovae.py:123-130 (mmvae_mnist_infovae_step):
    lambda_x * mean squared error + lambda_mmd * MMD, no KL term, plain Adam over the whole flat buffer (the reference's lr is 1e-3)."""

    _KIND = "InfoVAE"

    def __init__(self, state: PlanState, batch: int, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 lambda_x: float = 1.0, lambda_mmd: float = 1.0, kl_lambda: float = 0.0, seed: int = 1234):
        if state.API not in ("coco", "mnist_infovae"):
            raise MMVAEError("FusedInfoVAEStep: no InfoVAE step for the '%s' family (COCO has one on its plan, MNIST's InfoVAE a "
                             "plan of its own: MnistInfoVAEState)" % state.API)
        super().__init__(state, batch, lr, betas, eps, seed)
        self.lambda_x, self.lambda_mmd, self.kl_lambda = lambda_x, lambda_mmd, kl_lambda
        self.mnist = state.API == "mnist_infovae"
        if self.mnist:
            # mnist/train_infovae.py:45-76: mean squared error + MMD, no KL term; every gradient lands in ``grads`` and the optimizer
            # is the plain Adam kernel over the flat buffer
            self.kl_lambda = 0.0
            self.pixels = 784
            self._packed = False
            return
        self.enc_dropout = True
        self.pixels = 3 * 32 * 32
        self._image_range(state)

    def _workspace_bytes(self, state: PlanState, batch: int) -> int:
        if state.API == "mnist_infovae":
            return state.workspace_bytes(batch)
        return state._c("infovae_step_workspace_bytes", state.plan(batch))

    def _outputs(self) -> InfoVAEStepOutputs:
        return InfoVAEStepOutputs(self.sums, self.B * self.pixels, self.kl_lambda / self.B, self.lambda_x, self.lambda_mmd)

    def _mnist_forward_backward(self, image, training, backward, true_samples, recon_image, z) -> InfoVAEStepOutputs:
        """mmvae_mnist_infovae_step: images (B, 1, 28, 28) or flattened (B, 784); slot 0 of the sums is the squared-error sum"""
        if tuple(image.shape) not in ((self.B, 1, 28, 28), (self.B, 784)):
            raise MMVAEError("FusedInfoVAEStep: expected images of shape %s (got %s)" % ((self.B, 1, 28, 28), tuple(image.shape)))
        io = self._io(_lib.MnistInfoVAEStepIO, (("image", image),), dict(true_samples=true_samples, recon_image=recon_image, z=z), backward)
        return self._step("mmvae_mnist_infovae_step", io, training, backward)

    def forward_backward(self, image, training=True, backward=True, eps=None, enc_mask1=None, enc_mask2=None, true_samples=None,
                         recon_image=None, mu=None, logvar=None, z=None, _defer_unpack=False) -> InfoVAEStepOutputs:
        assert image.is_contiguous() and image.dtype == torch.float32
        if true_samples is not None:
            assert true_samples.is_contiguous() and true_samples.dtype == torch.float32 and tuple(true_samples.shape) == (self.B, self.D)
        if self.mnist:
            return self._mnist_forward_backward(image, training, backward, true_samples, recon_image, z)
        if tuple(image.shape) != (self.B, 3, 32, 32):
            raise MMVAEError("FusedInfoVAEStep: expected images of shape %s (got %s)" % ((self.B, 3, 32, 32), tuple(image.shape)))
        if true_samples is not None:
            assert true_samples.is_contiguous() and true_samples.dtype == torch.float32 and tuple(true_samples.shape) == (self.B, self.D)
        io = self._io(_lib.InfoVAEStepIO, (("image", image),),
                      dict(eps=eps, enc_mask1=enc_mask1, enc_mask2=enc_mask2, true_samples=true_samples, recon_image=recon_image,
                           mu=mu, logvar=logvar, z=z),
                      backward, defer_unpack=_defer_unpack)
        return self._step("mmvae_coco_infovae_step", io, training, backward)


class FusedTextStep(_SinglePassStep):
    """The step of coco/train_textonly.py:106-120 on the COCO plan: zero_grad -> ONE pass over B rows (caption encoder, reparametrize,
    caption decoder; no product of experts) -> lambda_y * MSE + kl_lambda * KL -> backward -> Adam.  ``state`` is a ``CocoState``; the
    image half is never launched: its parameters and BatchNorm buffers keep their values and its gradient is exactly 0.
    ``StepOutputs`` carries the pass in slot 0 of the text terms (``parts()[1][0]``, ``parts()[2][0]``)."""

    EMB = 300
    TEXT_PREFIXES = ("text_encoder.", "text_decoder.")
    _DEFER_PACK = True          # the step refreshes the caption half's packed weights itself (pack_first)
    _KIND = "text-only"

    def __init__(self, state: PlanState, batch: int, sos: torch.Tensor, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 kl_lambda: float = 1e-3, lambda_y: float = 1.0, seed: int = 1234):
        if state.API != "coco":
            raise MMVAEError("FusedTextStep: no text-only step for the '%s' family (COCO has one)" % state.API)
        super().__init__(state, batch, lr, betas, eps, seed)
        self.kl_lambda, self.lambda_y = kl_lambda, lambda_y
        self.T = state.steps
        self.sos = sos.to(device=state.device, dtype=torch.float32).contiguous().reshape(self.EMB)
        self.gru_dropout = True
        # the caption half is one run at the tail of the flat buffers: the optimizer visits nothing else when the run is 4-aligned
        first = min(off for name, _, off in state.table if name.startswith(self.TEXT_PREFIXES))
        assert all(name.startswith(self.TEXT_PREFIXES) == (off >= first) for name, _, off in state.table), \
            "the caption parameters are expected to be contiguous at the tail of the table"
        self.text_param_range = (first, state.nparams - first)
        if first % 4 == 0 and state.nparams % 4 == 0 and first > 0:
            self._ranges = (C.c_longlong * 2)(*self.text_param_range)

    def _workspace_bytes(self, state: PlanState, batch: int) -> int:
        return state._c("text_step_workspace_bytes", state.plan(batch))

    def _outputs(self) -> StepOutputs:
        return StepOutputs(self.sums, 1.0, self.B * self.T * self.EMB, self.kl_lambda / self.B, (0.0, 0.0, 0.0),
                           (self.lambda_y, 0.0, 0.0), (True, False, False))

    def forward_backward(self, text, training=True, backward=True, eps=None, gru_keep=None, recon_text=None, mu=None, logvar=None,
                         _defer_unpack=False) -> StepOutputs:
        assert text.is_contiguous() and text.dtype == torch.float32
        assert text.shape == (self.B, self.T, self.EMB)
        st = self.state
        if st.pack_pending and not st._pack_text_only:      # somebody else changed parameters of the image half as well
            st.pack_weights()
        io = self._io(_lib.TextStepIO, (("text", text), ("sos", self.sos)),
                      dict(eps=eps, gru_keep=gru_keep, recon_text=recon_text, mu=mu, logvar=logvar),
                      backward, defer_unpack=_defer_unpack)
        return self._step("mmvae_coco_text_step", io, training, backward)

    def _after_update(self) -> None:
        self.state.defer_text_pack()


class FusedMMTextStep(_SinglePassStep):
    """The step of multimnist/train_textonly.py:95-113 on the text-only plan (``MultimnistTextState``): zero_grad -> ONE pass over B
    rows (text encoder, reparametrize, text decoder; no product of experts) -> lambda_y * NLL + kl_lambda * KL -> backward -> Adam over
    every parameter.  ``StepOutputs`` carries the pass in slot 0 of the text terms (``parts()[1][0]``, ``parts()[2][0]``)."""

    _DEFER_PACK = True          # the step's prologue refreshes the packed weights itself (pack_first)
    _KIND = "text-only"

    def __init__(self, state: PlanState, batch: int, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 kl_lambda: float = 1e-3, lambda_y: float = 1.0, seed: int = 1234):
        if state.API != "mmtext":
            raise MMVAEError("FusedMMTextStep: needs a MultimnistTextState (got the '%s' family)" % state.API)
        super().__init__(state, batch, lr, betas, eps, seed)
        self.kl_lambda, self.lambda_y = kl_lambda, lambda_y
        self.gru_dropout = True

    def _workspace_bytes(self, state: PlanState, batch: int) -> int:
        return state.module_workspace_bytes(batch)

    def _outputs(self) -> StepOutputs:
        return StepOutputs(self.sums, 1.0, self.B * 4, self.kl_lambda / self.B, (0.0, 0.0, 0.0), (self.lambda_y, 0.0, 0.0),
                           (True, False, False))

    def forward_backward(self, text, training=True, backward=True, eps=None, gru_keep=None, force_tokens=None, recon_text=None,
                         mu=None, logvar=None, tokens=None, _defer_unpack=False) -> StepOutputs:
        assert text.is_contiguous() and text.dtype == torch.int64 and text.shape == (self.B, 4)
        io = self._io(_lib.MMTextStepIO, (("text", text),),
                      dict(eps=eps, gru_keep=gru_keep, force_tokens=force_tokens, recon_text=recon_text, mu=mu, logvar=logvar,
                           tokens=tokens),
                      backward, defer_unpack=_defer_unpack)
        return self._step("mmvae_mmtext_step", io, training, backward)


# ----------------------------------------------------------------------------------------------------------------
# the nn.Module side: one trainer and one checkpoint loader, declared per family in multimnist / mnist / celeba / coco
# ----------------------------------------------------------------------------------------------------------------
class Trainer:
    """``Trainer(vae, batch_size, lr)(*inputs)`` == zero_grad + forward + loss(es) + backward + Adam step, the train() closure body
    of a reference script as one enqueue, operating directly on ``vae``'s parameters (which stay ordinary nn.Parameters /
    state_dict entries; the engine updates the flat buffer in place and refreshes the packed bf16 copies itself).  A family
    declares its engine class, the reference script's ``lr`` / ``kl_lambda`` defaults and where its dropout probabilities live."""

    ENGINE = None
    LR, KL_LAMBDA = 1e-3, 1e-3          # (KL_LAMBDA None: the engine has none)
    ENC_DROPOUT = GRU_DROPOUT = None    # vae -> dropout probability (None: the engine has no such flag)

    def __init__(self, vae, batch_size: int, lr: Optional[float] = None, kl_lambda: Optional[float] = None, seed: int = 1234,
                 **engine_kw):
        """``engine_kw``: ``world_size`` / ``all_reduce`` of the three-pass engines."""
        self.vae = vae
        st = vae._core.sync(next(vae.parameters()).device)
        if self.KL_LAMBDA is not None:
            engine_kw["kl_lambda"] = self.KL_LAMBDA if kl_lambda is None else kl_lambda
        self.engine = self.ENGINE(st, batch_size, lr=self.LR if lr is None else lr, seed=seed, **self._engine_kw(vae, batch_size),
                                  **engine_kw)

    def _engine_kw(self, vae, batch_size) -> dict:
        """What else the family's engine is built from (COCO: the '<s>' vector)."""
        return {}

    def _flags(self, kw) -> None:
        eng = self.engine
        if "kl_lambda" in kw:
            eng.kl_lambda = kw.pop("kl_lambda")
        if self.ENC_DROPOUT is not None:
            eng.enc_dropout = self.ENC_DROPOUT(self.vae) > 0
        if self.GRU_DROPOUT is not None:
            eng.gru_dropout = self.GRU_DROPOUT(self.vae) > 0

    def __call__(self, *inputs, **kw) -> StepOutputs:
        self._flags(kw)
        return self.engine(*inputs, **kw)

    def evaluate(self, *inputs, **kw) -> StepOutputs:
        """The test() closure body: eval-mode forward, no backward."""
        self._flags(kw)
        return self.engine.forward_backward(*inputs, training=False, backward=False, **kw)


def load_vae_checkpoint(file_path, build, use_cuda=False, default_n_latents=None, /, **kw):
    """Rebuilds ``build(n_latents=..., **kw)`` from a checkpoint dict (``state_dict``, ``n_latents``) of either code base;
    ``default_n_latents`` stands in where an old dict has no ``n_latents``.  (Positional-only: ``kw`` may carry a ``use_cuda``.)"""
    checkpoint = torch.load(file_path, map_location=None if use_cuda else 'cpu', weights_only=False)
    if default_n_latents is not None:
        checkpoint.setdefault('n_latents', default_n_latents)
    vae = build(n_latents=checkpoint['n_latents'], **kw)
    vae.load_state_dict(checkpoint['state_dict'])
    if use_cuda:
        vae.cuda()
    return vae
