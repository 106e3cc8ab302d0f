"""What the four drop-in families (``multimnist``, ``mnist``, ``celeba``, ``coco``) share on the module side: the core that binds a
module tree to a plan's flat buffers, ONE bridge from a module's ``forward`` to its ``mmvae_<family>_<module>_fwd`` / ``_bwd`` entry
points (``run_module``), the family-neutral ops (``Swish``, ``ProductOfExperts``, reparametrisation, the loss terms) and the base
class of the VAEs.  The engine side (plans, fused steps, trainers) is ``core.py``; no family file imports from another."""
from __future__ import annotations

import weakref
from types import SimpleNamespace
from typing import List, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib
from ._lib import MMVAEError, call, ptr
from ._ops import stream as _stream
from .core import MultimnistState

DROP_P = 0.1          # the one dropout probability the kernels implement besides 0 (the reference's)


def _seed_from_torch() -> int:
    """A 63-bit seed drawn from torch's default CPU generator (so torch.manual_seed makes runs reproducible)."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


# ----------------------------------------------------------------------------------------------------------------
# shared device state of a module tree
# ----------------------------------------------------------------------------------------------------------------
class _Core:
    """Binds the nn.Parameters / BatchNorm buffers of a module tree to one flat ``PlanState``."""

    def __init__(self, owner: nn.Module, prefix: str, n_latents: int, state_cls=MultimnistState):
        self.state_cls = state_cls
        self.owner = weakref.ref(owner)
        self.prefix = prefix            # "" for MultimodalVAE, "image_encoder." for a standalone ImageEncoder, ...
        self.n_latents = n_latents
        self.state: Optional[MultimnistState] = None
        self._sig = None

    def _named(self):
        owner = self.owner()
        params = {self.prefix + n: p for n, p in owner.named_parameters()}
        bufs = {self.prefix + n: b for n, b in owner.named_buffers()}
        return owner, params, bufs

    def sync(self, device: torch.device) -> MultimnistState:
        """Make every parameter / BN buffer of the tree a view of the flat device buffers (no copy if it already is)."""
        if device.type != "cuda":
            raise MMVAEError("MMVAE HIP modules need CUDA/HIP tensors (got %s); move the module and its inputs to the GPU. "
                             "There is no CPU fallback." % device)
        if self.state is None or self.state.device != device:
            self.state = self.state_cls(self.n_latents, device)
            self._sig = None
        st = self.state
        st.ensure_packed()                 # a fused step may have deferred the refresh of the bf16 weight copies
        owner, params, bufs = self._named()
        base = st.params.data_ptr()
        for name, shape, off in st.table:
            p = params.get(name)
            if p is None:
                continue
            if p.device != device:
                raise MMVAEError("parameter %s is on %s but the input is on %s" % (name, p.device, device))
            if p.data_ptr() != base + 4 * off or p.dtype != torch.float32:
                view = st.view(name)
                view.copy_(p.data.to(torch.float32).reshape(shape))
                p.data = view
                self._sig = None
        bbase = st.bn_stats.data_ptr()
        for i, (pre, c, off) in enumerate(st.bn_table):
            for j, nm in enumerate(("running_mean", "running_var")):
                b = bufs.get("%s.%s" % (pre, nm))
                if b is None:
                    continue
                if b.data_ptr() != bbase + 4 * (off + j * c):
                    view = st.bn_stats[off + j * c: off + (j + 1) * c]
                    view.copy_(b.to(device))
                    _set_buffer(owner, (pre + "." + nm)[len(self.prefix):], view)
            nb = bufs.get(pre + ".num_batches_tracked")
            if nb is not None and nb.data_ptr() != st.bn_nbt.data_ptr() + 8 * i:
                view = st.bn_nbt[i]
                view.copy_(nb.to(device))
                _set_buffer(owner, (pre + ".num_batches_tracked")[len(self.prefix):], view)
        # repack the bf16 GEMM copies when any parameter changed (optimizer.step(), load_state_dict, ...)
        sig = tuple(p._version for p in params.values())
        if sig != self._sig:
            st.pack_weights()
            self._sig = sig
        return st

    def param_list(self) -> List[nn.Parameter]:
        owner, params, _ = self._named()
        return [params[n] for n, _, _ in self.state.table if n in params]

    def grads_for(self, names: List[str]) -> List[torch.Tensor]:
        st = self.state
        out = []
        for n, shape, off in st.table:
            if n in names:
                numel = 1
                for s in shape:
                    numel *= s
                out.append(st.grads[off:off + numel].view(shape).clone())
        return out


def _set_buffer(root: nn.Module, dotted: str, value: torch.Tensor) -> None:
    mod = root
    parts = dotted.split(".")
    for p in parts[:-1]:
        mod = getattr(mod, p)
    mod._buffers[parts[-1]] = value


def _core_of(module: nn.Module, prefix: str, state_cls=MultimnistState) -> _Core:
    root = getattr(module, "_mmvae_root", None)
    root = root() if root is not None else None
    if root is not None:
        return root._core
    if getattr(module, "_core", None) is None:
        module._core = _Core(module, prefix, module.n_latents, state_cls)
    return module._core


# ----------------------------------------------------------------------------------------------------------------
# the bridge: a module's forward -> mmvae_<family>_<module>_fwd, its backward -> ..._bwd
# ----------------------------------------------------------------------------------------------------------------
ONE_ROW_TEXT = "Expected more than 1 value per channel when training"     # torch's own refusal of such a BatchNorm batch
DECODER = (("x", "training", "out"), ("d", "out", "dx"))                  # run_module's fwd, bwd of every image / attribute decoder


class Draw(NamedTuple):
    """A keep mask ``run_module`` has yet to draw (behind the core's sync, the order the C calls have always had): uint8 ``shape``, keep
    probability 1 - DROP_P, Philox stream ``salt`` (2, 3: the encoder's two dropouts, 4: the GRU's); ``seed``: one drawn from torch's
    generator at that moment unless given."""
    shape: Tuple[int, ...]
    salt: int
    seed: Optional[int] = None


def _keep(shape, device, salt, seed=None):
    m = torch.empty(*shape, dtype=torch.uint8, device=device)
    call("mmvae_keep_mask", ptr(m), m.numel(), DROP_P, _seed_from_torch() if seed is None else seed, None, salt, _stream())
    return m


def _dropout_on(mod: nn.Module, probs, text: str) -> bool:
    """Whether this forward of ``mod`` drops anything.  A probability other than 0 or DROP_P is refused with ``text``."""
    if not (mod.training and any(p > 0 for p in probs)):
        return False
    if any(abs(p - DROP_P) > 1e-9 for p in probs):
        raise MMVAEError(text)
    return True


def _c_args(order, marks):
    return [marks[a] if type(a) is str else ptr(a) for a in order]


class _ModuleFn(torch.autograd.Function):
    """The autograd half of ``run_module``; the parameters are listed as inputs so that autograd routes their gradients."""

    @staticmethod
    def forward(ctx, job, x, *params):
        ws = torch.empty(job.wsb, dtype=torch.uint8, device=x.device)
        out = torch.empty(job.out_shape, dtype=torch.float32, device=x.device)
        marks = {"x": ptr(x), "training": job.training, "out": ptr(out)}
        call(job.base + "_fwd", job.h, ptr(ws), job.wsb, *_c_args(job.fwd, marks), _stream())
        # (the output is held only for a backward that reads it: held, it forms a cycle through its own grad_fn)
        ctx.job, ctx.marks, ctx.held = job, marks, (ws, x, out if "out" in job.bwd_marks else None)
        return out

    @staticmethod
    def backward(ctx, d_out):
        job, (ws, x, _) = ctx.job, ctx.held
        job.st.grads.zero_()
        d = d_out.contiguous()
        dx = torch.empty_like(x) if "dx" in job.bwd_marks else None
        call(job.base + "_bwd", job.h, ptr(ws), job.wsb, *_c_args(job.bwd, dict(ctx.marks, d=ptr(d), dx=ptr(dx))), _stream())
        return (None, dx) + tuple(job.core.grads_for(job.names))


def run_module(mod: nn.Module, prefix: str, state_cls, x: torch.Tensor, base: str, out_shape, fwd, bwd, bn_values=None):
    """One module forward through ``<base>_fwd``, differentiable through ``<base>_bwd`` -> the (B, *out_shape) fp32 output.

    ``x`` is the module's converted input, ``prefix`` its parameters' place in the plan (``"image_encoder."``), ``state_cls`` the
    plan a stand-alone module builds.  ``fwd`` / ``bwd`` are the C arguments between ``h, ws, ws_bytes`` and the stream, in order:
    the markers ``"x"``, ``"out"``, ``"training"``, ``"d"`` (the incoming gradient, made contiguous) and ``"dx"`` (the input
    gradient: a module whose ``bwd`` lacks it returns none), and between them what the module captured: a tensor, None (a null
    pointer) or a ``Draw`` (equal ``Draw``s are one mask).  ``bn_values``: values per row and channel at the module's narrowest
    BatchNorm; a training batch without a second value per channel is refused as torch refuses it."""
    core = _core_of(mod, prefix, state_cls)
    st = core.sync(x.device)
    B = x.shape[0]
    if bn_values is not None and mod.training and B * bn_values <= 1:
        raise ValueError(ONE_ROW_TEXT)
    job = SimpleNamespace(base=base, core=core, st=st, h=st.plan(B), wsb=st.module_workspace_bytes(B), out_shape=(B,) + tuple(out_shape),
                          training=int(mod.training), names=[], bwd_marks={a for a in bwd if type(a) is str})
    params = []
    for k, p in mod.named_parameters():
        job.names.append(prefix + k)
        params.append(p)
    masks = {}
    for a in (*fwd, *bwd):
        if type(a) is Draw and a not in masks:
            masks[a] = _keep(a.shape, x.device, a.salt, a.seed)
    job.fwd, job.bwd = ([masks[a] if type(a) is Draw else a for a in order] for order in (fwd, bwd))
    return _ModuleFn.apply(job, x, *params)


# ----------------------------------------------------------------------------------------------------------------
# family-neutral ops
# ----------------------------------------------------------------------------------------------------------------
def swish(x):
    """multimnist/model.py:375-376"""
    return _Elementwise.apply(x)


class _Elementwise(torch.autograd.Function):
    # x*sigmoid(x) as a standalone op is not on the hot path (it is fused into the GEMM kernels); it exists only so
    # that ``Swish()(tensor)`` keeps working for user code.
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return x * torch.sigmoid(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        s = torch.sigmoid(x)
        return g * s * (1 + x * (1 - s))


class Swish(nn.Module):
    """multimnist/model.py:379-381"""
    def forward(self, x):
        return swish(x)


class _PoEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, logvar):
        M = mu.shape[0]
        n = mu[0].numel()
        mu, logvar = mu.contiguous().float(), logvar.contiguous().float()
        omu = torch.empty_like(mu[0]); olv = torch.empty_like(mu[0])
        call("mmvae_poe_fwd", ptr(mu), ptr(logvar), M, n, ptr(omu), ptr(olv), _stream())
        ctx.save_for_backward(mu, logvar)
        return omu, olv

    @staticmethod
    def backward(ctx, gmu, glv):
        mu, logvar = ctx.saved_tensors
        M, n = mu.shape[0], mu[0].numel()
        gmu = torch.zeros_like(mu[0]) if gmu is None else gmu.contiguous()
        glv = torch.zeros_like(mu[0]) if glv is None else glv.contiguous()
        dmu = torch.empty_like(mu); dlv = torch.empty_like(mu)
        call("mmvae_poe_bwd", ptr(mu), ptr(logvar), M, n, ptr(gmu), ptr(glv), ptr(dmu), ptr(dlv), _stream())
        return dmu, dlv


class ProductOfExperts(nn.Module):
    """multimnist/model.py:348-360 (variance-weighted mean, reproduced as written)."""
    def forward(self, mu, logvar, eps=1e-8):
        if eps != 1e-8:
            raise MMVAEError("ProductOfExperts: only eps=1e-8 (the reference default) is implemented")
        if mu.device.type != "cuda":
            raise MMVAEError("ProductOfExperts needs GPU tensors; there is no CPU fallback")
        _lib.init_device(mu.device.index if mu.device.index is not None else torch.cuda.current_device())
        return _PoEFn.apply(mu, logvar)


class _ReparamFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, logvar, eps):
        mu, logvar = mu.contiguous(), logvar.contiguous()
        z = torch.empty_like(mu)
        call("mmvae_reparam_fwd", ptr(mu), ptr(logvar), ptr(eps), mu.numel(), ptr(z), _stream())
        ctx.save_for_backward(logvar, eps)
        return z

    @staticmethod
    def backward(ctx, dz):
        logvar, eps = ctx.saved_tensors
        dz = dz.contiguous()
        dmu = torch.empty_like(dz); dlv = torch.empty_like(dz)
        call("mmvae_reparam_bwd", ptr(logvar), ptr(eps), ptr(dz), dz.numel(), ptr(dmu), ptr(dlv), _stream())
        return dmu, dlv, None


# ----------------------------------------------------------------------------------------------------------------
# what the VAEs of every family share
# ----------------------------------------------------------------------------------------------------------------
class VAEBase(nn.Module):
    """What every VAE here has: ``reparametrize`` and the wiring of the children to the root's core."""

    def _adopt(self, *children: nn.Module) -> None:
        """The children run on this module's ``_core`` (``_core_of`` follows the weak reference, which is no submodule link)."""
        for m in children:
            object.__setattr__(m, "_mmvae_root", weakref.ref(self))

    def reparametrize(self, mu, logvar, eps: Optional[torch.Tensor] = None):
        """Sample in training (``eps``: the noise, drawn on the device unless given), the mean in eval."""
        if self.training:
            if eps is None:
                eps = torch.empty_like(mu)
                call("mmvae_normal", ptr(eps), eps.numel(), _seed_from_torch(), None, 1, _stream())
            return _ReparamFn.apply(mu, logvar, eps.contiguous())
        return mu


class ExpertsVAEBase(VAEBase):
    """The MultimodalVAEs: ``prior`` and the product of the present experts on top."""

    def prior(self, size, use_cuda=False):
        mu = torch.zeros(size)
        logvar = torch.log(torch.ones(size))
        if use_cuda:
            mu, logvar = mu.cuda(), logvar.cuda()
        return mu, logvar

    def _product(self, *experts):
        """``self.experts`` over the ``(mu, logvar)`` pairs that are not None (one per present modality, image first)."""
        present = [e for e in experts if e is not None]
        if len(present) == 1:
            (mu, logvar), = present
            mu, logvar = mu.unsqueeze(0), logvar.unsqueeze(0)
        else:
            mu = torch.stack([m for m, _ in present], dim=0)
            logvar = torch.stack([lv for _, lv in present], dim=0)
        return self.experts(mu, logvar)


# ----------------------------------------------------------------------------------------------------------------
# loss terms (each family's loss_function weighs them as its reference does)
# ----------------------------------------------------------------------------------------------------------------
def _gscale(g: torch.Tensor) -> torch.Tensor:
    """The upstream gradient of a 0-d loss as a contiguous fp32 device scalar: the backward kernels read it themselves
    (a host ``.item()`` here would synchronise the stream three times per loss_function call)."""
    return g.detach().reshape(1).to(torch.float32).contiguous()


class _BCEMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t):
        p, t = p.contiguous().float(), t.contiguous().float()
        out = torch.zeros(1, dtype=torch.float32, device=p.device)
        call("mmvae_bce_fwd", ptr(p), ptr(t), p.numel(), ptr(out), _stream())
        ctx.save_for_backward(p, t)
        return (out / p.numel()).squeeze(0)

    @staticmethod
    def backward(ctx, g):
        p, t = ctx.saved_tensors
        dp = torch.empty_like(p)
        call("mmvae_bce_bwd", ptr(p), ptr(t), p.numel(), 1.0 / p.numel(), ptr(_gscale(g)), ptr(dp), _stream())
        return dp, None


class _NLLMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, target):
        logp, target = logp.contiguous().float(), target.contiguous().long()
        rows, classes = logp.shape
        out = torch.zeros(1, dtype=torch.float32, device=logp.device)
        call("mmvae_nll_fwd", ptr(logp), ptr(target), rows, classes, ptr(out), _stream())
        ctx.target, ctx.shape = target, (rows, classes)
        return (out / rows).squeeze(0)

    @staticmethod
    def backward(ctx, g):
        rows, classes = ctx.shape
        d = torch.empty(rows, classes, dtype=torch.float32, device=ctx.target.device)
        call("mmvae_nll_bwd", ptr(ctx.target), rows, classes, 1.0 / rows, ptr(_gscale(g)), ptr(d), _stream())
        return d, None


class _KLSumFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, logvar):
        mu, logvar = mu.contiguous().float(), logvar.contiguous().float()
        out = torch.zeros(1, dtype=torch.float32, device=mu.device)
        call("mmvae_kl_fwd", ptr(mu), ptr(logvar), mu.numel(), ptr(out), _stream())
        ctx.save_for_backward(mu, logvar)
        return out.squeeze(0)

    @staticmethod
    def backward(ctx, g):
        mu, logvar = ctx.saved_tensors
        dmu = torch.empty_like(mu); dlv = torch.empty_like(mu)
        call("mmvae_kl_bwd", ptr(mu), ptr(logvar), mu.numel(), 1.0, ptr(_gscale(g)), ptr(dmu), ptr(dlv), _stream())
        return dmu, dlv


class _MSEMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous().float(), b.contiguous().float()
        out = torch.zeros(1, dtype=torch.float32, device=a.device)
        call("mmvae_mse_fwd", ptr(a), ptr(b), a.numel(), ptr(out), _stream())
        ctx.save_for_backward(a, b)
        return (out / a.numel()).squeeze(0)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        da = torch.empty_like(a)
        call("mmvae_mse_bwd", ptr(a), ptr(b), a.numel(), 1.0 / a.numel(), ptr(_gscale(g)), ptr(da), _stream())
        return da, None
