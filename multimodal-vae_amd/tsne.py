"""The latent manifold of ``mnist/manifold.py``: PCA, and exact t-SNE with a 2-component embedding on one fused HIP op
(csrc/tsne.hip; the reference calls sklearn's ``PCA`` and ``TSNE(n_components=2, perplexity=40, n_iter=300)``)::

    p_{j|i} = exp(-beta_i (d_ij - min_j d_ij)) / sum_j ...,   entropy(p_{.|i}) = log(perplexity)       (sklearn's search for beta_i)
    P_ij    = (p_{j|i} + p_{i|j}) / 2n                                                               (dense, n x n, fp32)
    w_ij    = 1 / (1 + |y_i - y_j|^2),   Z = sum_{i != j} w_ij
    grad_i  = 4 (exaggeration sum_j P_ij w_ij (y_i - y_j) - sum_j w_ij^2 (y_i - y_j) / Z)
    KL      = sum P log P - sum P log w + log Z

``tsne`` enqueues all of its iterations (sklearn's ``_gradient_descent``: gains, momentum 0.5 then 0.8, no recentring) on the
caller's current stream without a host synchronisation in between; every iteration reads P once.  The t-SNE functions take fp32
device tensors only and there is no CPU fallback; ``pca`` is torch ops and runs wherever torch runs.  Results depend on the
shape alone: two calls give identical bits.  P is n * n * 4 bytes (400 MB at n = 10,000) and n is at most 32768.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from ._lib import MMVAEError, call, ptr
from ._ops import WorkspaceCache, geometry, stream

_WS = WorkspaceCache(4)          # cached workspaces (the oldest goes first)


def tsne_geometry() -> Tuple[int, int, int, int, int]:
    """(rows per sweep workgroup, columns per column tile of the sweep, side of a symmetrisation tile, threads per affinity row,
    largest D) of the kernels; include/mmvae_hip.h states the split rule."""
    return geometry("mmvae_tsne_geometry", 5)


def _device_f32(t, what: str, name: str, cols: Optional[int] = None) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dim() != 2 or (cols is not None and t.shape[1] != cols):
        raise MMVAEError("%s: %s (n, %s) expected" % (what, name, "D" if cols is None else cols))
    if t.device.type != "cuda":
        raise MMVAEError("%s runs on a gfx950 GPU only (got %s on %s): move the tensor to the device.  There is no CPU fallback."
                         % (what, name, t.device))
    if t.dtype != torch.float32:
        raise MMVAEError("%s: float32 tensors expected (got %s for %s)" % (what, t.dtype, name))
    return t.detach().contiguous()


def _workspace(dev: torch.device, n: int) -> Tuple[torch.Tensor, int]:
    need = call("mmvae_tsne_workspace_bytes", n)
    if need <= 0:
        raise MMVAEError("tsne: n = %d: need 3..32768 rows" % n)
    return _WS.get(dev, need, n), need


@torch.no_grad()
def joint_probabilities(x: torch.Tensor, perplexity: float = 40.0, return_stats: bool = False):
    """x (n, D) -> (P (n, n), beta (n,)): the symmetric joint probabilities of t-SNE and the precision found for every row.  With
    ``return_stats`` also a device tensor (sum P log P, sum P)."""
    x = _device_f32(x, "joint_probabilities", "x")
    n, dim = x.shape
    if dim < 1 or dim > tsne_geometry()[4]:
        raise MMVAEError("joint_probabilities: D = %d: need 1..%d columns" % (dim, tsne_geometry()[4]))
    if not (1.0 <= float(perplexity) < n - 1):
        raise MMVAEError("joint_probabilities: perplexity = %g: need 1 <= perplexity < n - 1 = %d" % (perplexity, n - 1))
    with torch.cuda.device(x.device):
        ws, need = _workspace(x.device, n)
        P = torch.empty(n, n, dtype=torch.float32, device=x.device)
        beta = torch.empty(n, dtype=torch.float32, device=x.device)
        out = torch.empty(2, dtype=torch.float32, device=x.device)
        call("mmvae_tsne_affinities", ptr(x), n, dim, float(perplexity), ptr(P), ptr(beta), ptr(out), ptr(ws), need, stream())
    return (P, beta, out) if return_stats else (P, beta)


def _square(P, n, what):
    P = _device_f32(P, what, "P")
    if P.shape[0] != n or P.shape[1] != n:
        raise MMVAEError("%s: P (%d, %d) expected for y (%d, 2)" % (what, n, n, n))
    return P


@torch.no_grad()
def kl_grad(P: torch.Tensor, y: torch.Tensor, exaggeration: float = 1.0):
    """(KL(P || Q) as a 0-d device tensor, dKL/dy (n, 2)) with ``exaggeration * P`` in the attractive term of the gradient (the KL
    is always that of P itself).  P must be symmetric, as ``joint_probabilities`` returns it."""
    y = _device_f32(y, "kl_grad", "y", 2)
    n = y.shape[0]
    P = _square(P, n, "kl_grad")
    if P.device != y.device:
        raise MMVAEError("kl_grad: P on %s, y on %s" % (P.device, y.device))
    with torch.cuda.device(y.device):
        ws, need = _workspace(y.device, n)
        grad = torch.empty_like(y)
        out = torch.empty(3, dtype=torch.float32, device=y.device)
        call("mmvae_tsne_grad", ptr(P), float(exaggeration), ptr(y), n, ptr(ws), need, ptr(grad), ptr(out), stream())
    return out[0].clone(), grad


def initial_embedding(n: int, seed: int = 0) -> torch.Tensor:
    """(n, 2) draws of N(0, 1e-4^2) from a seeded CPU generator: sklearn's init='random'."""
    return torch.randn(n, 2, generator=torch.Generator().manual_seed(seed)) * 1e-4


@torch.no_grad()
def tsne(x: torch.Tensor, perplexity: float = 40.0, n_iter: int = 300, learning_rate: float = 200.0, early_exaggeration: float = 12.0,
         exaggeration_iters: int = 250, init: Optional[torch.Tensor] = None, seed: int = 0, return_trace: bool = False):
    """x (n, D) on the device -> the (n, 2) embedding (and, with ``return_trace``, the KL of every iteration measured before its
    update, a device tensor of n_iter).  The defaults are what the reference's ``TSNE(n_components=2, perplexity=40, n_iter=300)``
    resolves to: learning rate 200, early exaggeration 12 over the first 250 iterations, a random N(0, 1e-4^2) start."""
    x = _device_f32(x, "tsne", "x")
    n = x.shape[0]
    if int(n_iter) < 1:
        raise MMVAEError("tsne: n_iter = %d: need at least 1" % n_iter)
    P, _ = joint_probabilities(x, perplexity)
    if init is None:
        y = initial_embedding(n, seed).to(x.device)
    else:
        if not torch.is_tensor(init) or tuple(init.shape) != (n, 2):
            raise MMVAEError("tsne: init (%d, 2) expected" % n)
        y = init.detach().to(device=x.device, dtype=torch.float32).clone().contiguous()
    with torch.cuda.device(x.device):
        ws, need = _workspace(x.device, n)
        update, gains = torch.zeros_like(y), torch.ones_like(y)
        trace = torch.empty(int(n_iter), dtype=torch.float32, device=x.device)
        call("mmvae_tsne_run", ptr(P), n, ptr(y), ptr(update), ptr(gains), 0, int(n_iter), float(learning_rate), float(early_exaggeration),
             int(exaggeration_iters), ptr(trace), ptr(ws), need, stream())
    return (y, trace) if return_trace else y


@torch.no_grad()
def pca(x: torch.Tensor, n_components: int):
    """x (n, D) on any device -> (projected (n, k), components (k, D), explained_variance (k,)), sklearn's ``PCA(k).fit_transform``:
    the data are centred, the float64 covariance (n - 1 in the denominator) is formed with torch ops on x's device, its
    eigen-decomposition (a D x D matrix) runs on the host, and every component's sign makes its largest-magnitude loading
    positive.  The results have x's dtype and device."""
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[0] < 2:
        raise ValueError("pca: x (n >= 2, D) expected")
    k = int(n_components)
    if k < 1 or k > x.shape[1]:
        raise ValueError("pca: n_components = %d: need 1..%d" % (k, x.shape[1]))
    xc = x.double()
    xc = xc - xc.mean(0, keepdim=True)
    cov = (xc.t() @ xc) / (x.shape[0] - 1)
    evals, evecs = torch.linalg.eigh(cov.cpu())                   # ascending
    order = torch.argsort(evals, descending=True)[:k]
    comps = evecs[:, order].t().contiguous()                      # (k, D)
    big = comps.abs().argmax(dim=1, keepdim=True)
    comps = comps * torch.sign(torch.gather(comps, 1, big))
    var = evals[order].clamp_min(0.0)
    comps_d = comps.to(x.device)
    return (xc @ comps_d.t()).to(x.dtype), comps_d.to(x.dtype), var.to(device=x.device, dtype=x.dtype)
