"""Reference code of the MMD tests (tests/test_cpu_mmd.py, tests/test_gpu_mmd.py, tests/test_gpu_infovae.py).

  k(a, b)   = exp(-(sum_k (a_k - b_k)^2 / D) / D)
  MMD(x, y) = mean_ij k(x_i, x_j) + mean_ij k(y_i, y_j) - 2 mean_ij k(x_i, y_j)
  dMMD/dx_i = -(4 / (n_x^2 D^2)) sum_j k(x_i, x_j) (x_i - x_j) + (4 / (n_x n_y D^2)) sum_j k(x_i, y_j) (x_i - y_j)     (dy alike)

``mmd64``: the formula and its analytic gradient in float64, a block of rows at a time, never holding (N, M, D) for more than
one block.  It works per (row class, column class) quarter like the kernel does, so that a fault -- the pairs of some rows of one
class with some columns of one class left out -- can be injected: the CPU tests show that every gate of the GPU tests sees one
row tile, one column tile or one column split missing.

``formulation``: the reference's formulation (coco/model.py:385-402: both operands expanded to (N, M, D), subtract, square, mean
over D, divide by D, exp; three kernels, three means) in torch ops at the dtype of its inputs, with autograd: at fp32 on the CPU
its error against ``mmd64`` is the yardstick of the GPU gates.  Above ``FORMULATION_ROWS`` expanded elements it runs over blocks
of rows (same ops and autograd per block; the blocks' sums and gradients are added in float64, which can only make the
yardstick smaller and the gate stricter): the (4099, 4099, 100) operands of the largest GPU case are 6.7 GB each.
"""
import functools

import torch

GATE_FACTOR = 4.0                 # GPU error <= 4 x the error of the fp32 formulation on the CPU (same inputs)
BLOCK_ELEMS = 1 << 24             # (rows, M, D) elements per block
FORMULATION_ROWS = 1 << 27        # expanded elements above which ``formulation`` goes block by block,
FORMULATION_BLOCK = 1 << 23       # this many at a time (they stay in the CPU's caches: 3x faster than blocks of 2^27)


# ------------------------------------------------------------------------------------------------------------- float64
def sqdist64(a, b):
    """(n, D), (m, D) float64 -> (n, m) squared distances from coordinate differences."""
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(2)


def kernel64(x, y):
    """-> (n_x, n_y) float64 kernel matrix, block by block."""
    x, y = x.double(), y.double()
    D = x.shape[1]
    rows = max(1, BLOCK_ELEMS // max(1, y.shape[0] * D))
    return torch.cat([torch.exp(-(sqdist64(x[i:i + rows], y) / D) / D) for i in range(0, x.shape[0], rows)])


def _quarter(r, c, fault=None, expand=False):
    """rows r (n, D), columns c (m, D) float64 -> (S (n,), G (n, D)): S_i = sum_j k_ij, G_i = sum_j k_ij (r_i - c_j).
    ``fault`` = (row slice, column slice): those pairs are left out.  ``expand``: distances as |a|^2 + |b|^2 - 2 a.b and G as
    r S - K c (float64 carries both to ~1e-13 of the result; used where the direct form would take minutes on a CPU)."""
    n, D = r.shape
    S = torch.zeros(n, dtype=torch.float64)
    G = torch.zeros(n, D, dtype=torch.float64)
    rows = max(1, BLOCK_ELEMS // max(1, c.shape[0] * D))
    for i in range(0, n, rows):
        ri = r[i:i + rows]
        if expand:
            d2 = ((ri * ri).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2.0 * (ri @ c.t())).clamp_min(0.0)
        else:
            diff = ri[:, None, :] - c[None, :, :]
            d2 = (diff * diff).sum(2)
        K = torch.exp(-(d2 / D) / D)
        if fault is not None:
            rs, cs = fault
            lo, hi = max(rs.start, i) - i, min(rs.stop, i + rows) - i
            if lo < hi:
                K[lo:hi, cs] = 0.0
        S[i:i + rows] = K.sum(1)
        G[i:i + rows] = ri * K.sum(1)[:, None] - K @ c if expand else (K[:, :, None] * diff).sum(1)
    return S, G


def mmd64(x, y, fault=None, expand=None):
    """-> {"terms": float64 (4,) = (mean Kxx, mean Kyy, mean Kxy, MMD), "dx": (n_x, D), "dy": (n_y, D)} in float64.
    ``fault`` = (row class, row slice, column class, column slice) with classes "x" / "y"."""
    x, y = x.double(), y.double()
    nx, ny, D = x.shape[0], y.shape[0], x.shape[1]
    if expand is None:
        expand = (nx + ny) ** 2 * D > (1 << 30)
    T = {"x": x, "y": y}
    q = {}
    for a in "xy":
        for c in "xy":
            f = (fault[1], fault[3]) if fault is not None and (fault[0], fault[2]) == (a, c) else None
            q[a + c] = _quarter(T[a], T[c], f, expand)
    kxx, kyy, kxy = q["xx"][0].sum() / (nx * nx), q["yy"][0].sum() / (ny * ny), q["xy"][0].sum() / (nx * ny)
    dd = float(D) * float(D)
    dx = -(4.0 / (nx * nx * dd)) * q["xx"][1] + (4.0 / (nx * ny * dd)) * q["xy"][1]
    dy = -(4.0 / (ny * ny * dd)) * q["yy"][1] + (4.0 / (nx * ny * dd)) * q["yx"][1]
    return {"terms": torch.stack((kxx, kyy, kxy, (kxx + kyy) - 2.0 * kxy)), "dx": dx, "dy": dy}


# ------------------------------------------------------------------------------------------------------------- the formulation
def formulation_kernel(x, y):
    """coco/model.py:385-394 in torch ops at the inputs' dtype."""
    n, m, D = x.shape[0], y.shape[0], x.shape[1]
    a = x.unsqueeze(1).expand(n, m, D)
    b = y.unsqueeze(0).expand(n, m, D)
    return torch.exp(-torch.mean(torch.pow(a - b, 2), dim=2) / D)


def formulation_mmd(x, y):
    """coco/model.py:397-402, differentiable (for a loss built in torch autograd)"""
    return torch.mean(formulation_kernel(x, x)) + torch.mean(formulation_kernel(y, y)) - 2 * torch.mean(formulation_kernel(x, y))


def _blockwise_mean(a, b, weight, ga, gb):
    """mean of formulation_kernel(a, b) over blocks of rows of a -> the mean (float64 sum of the blocks' sums, rounded to the
    input dtype); adds weight * d mean / d a to ga and weight * d mean / d b to gb (float64)."""
    n, m, D = a.shape[0], b.shape[0], a.shape[1]
    rows = max(1, FORMULATION_BLOCK // (m * D))
    total = 0.0
    for i in range(0, n, rows):
        ab = a[i:i + rows].detach().clone().requires_grad_(True)
        bb = b.detach().clone().requires_grad_(True)
        s = formulation_kernel(ab, bb).sum()
        s.backward()
        total += float(s.detach())
        ga[i:i + rows] += (weight / (n * m)) * ab.grad.double()
        gb += (weight / (n * m)) * bb.grad.double()
    return torch.tensor(total / (n * m), dtype=torch.float64).to(a.dtype)


def formulation(x, y):
    """coco/model.py:397-402 -> (terms (4,), dx, dy) at the inputs' dtype, the gradients by autograd."""
    same = y is x
    nmax, D = max(x.shape[0], y.shape[0]), x.shape[1]
    if nmax * nmax * D > FORMULATION_ROWS:
        gx = torch.zeros(x.shape, dtype=torch.float64)
        gy = gx if same else torch.zeros(y.shape, dtype=torch.float64)
        kxx = _blockwise_mean(x, x, 1.0, gx, gx)
        kyy = _blockwise_mean(y, y, 1.0, gy, gy)
        kxy = _blockwise_mean(x, y, -2.0, gx, gy)
        return torch.stack((kxx, kyy, kxy, kxx + kyy - 2 * kxy)), gx.to(x.dtype), gy.to(x.dtype)
    xl = x.detach().clone().requires_grad_(True)
    yl = xl if same else y.detach().clone().requires_grad_(True)
    kxx, kyy, kxy = torch.mean(formulation_kernel(xl, xl)), torch.mean(formulation_kernel(yl, yl)), torch.mean(formulation_kernel(xl, yl))
    mmd = kxx + kyy - 2 * kxy
    mmd.backward()
    terms = torch.stack((kxx, kyy, kxy, mmd)).detach()
    if same:
        return terms, xl.grad, xl.grad
    return terms, xl.grad, yl.grad


# ------------------------------------------------------------------------------------------------------------- errors and gates
def value_error(terms, ref):
    """largest |error| of the four terms over (mean Kxx + mean Kyy + 2 mean Kxy)"""
    ref = ref.double()
    return float((terms.double().cpu() - ref).abs().max() / (ref[0] + ref[1] + 2.0 * ref[2]))


def grad_error(g, ref, scale=None):
    """max |error| / max |gradient| (``scale``: the denominator, where the gradient itself vanishes)"""
    ref = ref.double()
    return float((g.double().cpu() - ref).abs().max() / (ref.abs().max() if scale is None else scale))


def real_inputs(nx, ny, D, seed=0, same=False):
    """x ~ N(0, 1), y ~ 1.5 N(0, 1) + 0.3, fp32, from a seed."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * nx + 3 * ny + D)
    x = torch.randn(nx, D, generator=g)
    if same:
        return x, x
    return x, 1.5 * torch.randn(ny, D, generator=g) + 0.3


@functools.lru_cache(maxsize=None)
def real_case(nx, ny, D, same=False):
    """Inputs, the float64 reference and the yardsticks of one real-valued case, computed once per process.
    ``same``: x and y are one tensor.  MMD and both gradients then vanish identically (the two sums of a gradient cancel), so the
    gradient that autograd leaves on the tensor is compared with zero, on the scale of ONE of the two sums,
    max |4 / (n^2 D^2) sum_j k_ij (x_i - x_j)|: that is what a missing tile or a rounding error is relative to."""
    x, y = real_inputs(nx, ny, D, same=same)
    ref = mmd64(x, y)
    terms32, dx32, dy32 = formulation(x, y)
    scale = None
    if same:
        xd = x.double()
        scale = float((4.0 / (nx * nx * float(D) ** 2)) * _quarter(xd, xd)[1].abs().max())
        ref["dx"] = ref["dy"] = torch.zeros_like(ref["dx"])
    yard = {"value": value_error(terms32, ref["terms"]), "dx": grad_error(dx32, ref["dx"], scale),
            "dy": grad_error(dy32, ref["dy"], scale)}
    return {"x": x, "y": y, "ref": ref, "yardstick": yard, "scale": scale}


def split_rule(nx, ny, row_tile, col_tile):
    """include/mmvae_hip.h: (row tiles of x, of y, column tiles of x, of y, splits over x, over y)"""
    cd = lambda a, b: (a + b - 1) // b
    rtx, rty, tx, ty = cd(nx, row_tile), cd(ny, row_tile), cd(nx, col_tile), cd(ny, col_tile)
    cap = 1024 // (rtx + rty)
    return rtx, rty, tx, ty, max(1, min(tx, 64, cap)), max(1, min(ty, 64, cap))


def split_rows(tiles, splits, s, col_tile, n):
    """rows [lo, hi) of a class that column split s of ``splits`` covers"""
    return min(n, (tiles * s // splits) * col_tile), min(n, (tiles * (s + 1) // splits) * col_tile)
