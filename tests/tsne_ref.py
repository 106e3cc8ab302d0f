"""Reference code of the t-SNE tests (tests/test_cpu_tsne.py, tests/test_gpu_tsne.py), numpy, written from the formulas:

  d_ij    = sum_k (x_ik - x_jk)^2
  p_{j|i} = exp(-beta_i (d_ij - min_{j != i} d_ij)) / sum_{j != i} ...      beta_i: start 1, double (entropy too high) or halve until
            bracketed, then halve the bracket; stop at |H_i - log perplexity| <= 1e-5 or after 100 steps
  P_ij    = max((p_{j|i} + p_{i|j}) / 2n, 1e-12), P_ii = 0
  w_ij    = 1 / (1 + |y_i - y_j|^2),  Z = sum_{i != j} w_ij
  grad_i  = 4 (exaggeration sum_j P_ij w_ij (y_i - y_j) - sum_j w_ij^2 (y_i - y_j) / Z)
  KL      = sum P log P - sum P log w + log Z
  update:   gains + 0.2 where update * grad < 0, else * 0.8, floor 0.01; update = momentum update - learning_rate gains grad;
            y += update; momentum 0.5 and the exaggeration while iter < exaggeration_iters, then 0.8 and 1

Every function takes ``dtype``: numpy.float64 is the reference, numpy.float32 (every array, scalar and sum in fp32) the yardstick
of the GPU gates: the op may err GATE_FACTOR times as much against float64 as the yardstick does on the same input.  ``drop`` /
``fault`` arguments leave pairs out the way a kernel with a missing row tile, column tile, column split or transpose half would;
tests/test_cpu_tsne.py shows that every gate sees them.
"""
import functools

import numpy as np

GATE_FACTOR = 4.0
RUN_GATE_FACTOR = 8.0             # ten dependent steps compound
TOL = 1e-5
STEPS = 100
P_FLOOR = 1e-12


def sqdist(x):
    """(n, D) -> (n, n) squared distances from coordinate differences, at x's dtype, a block of rows at a time."""
    n, D = x.shape
    out = np.empty((n, n), dtype=x.dtype)
    rows = max(1, (1 << 23) // max(1, n * D))
    for i in range(0, n, rows):
        diff = x[i:i + rows, None, :] - x[None, :, :]
        out[i:i + rows] = (diff * diff).sum(2, dtype=x.dtype)
    return out


def _shifted(x):
    n = x.shape[0]
    d = sqdist(x)
    off = ~np.eye(n, dtype=bool)
    dmin = np.where(off, d, np.inf).min(1).astype(x.dtype)
    return d - dmin[:, None], off


def affinities(x, perplexity, dtype=np.float64, drop_cols=None, fault=None):
    """-> {"P", "beta", "cond", "H" (the entropy the search stopped at), "plogp", "sum"}.
    ``drop_cols``: a slice of columns the search and the conditional row never see (a column tile dropped by the row kernel).
    ``fault`` = ("rows", slice): those rows of P are never written (zeros); ("transpose", row slice, column slice): the block and
    its mirror are built without the transposed half, p_{j|i} / n."""
    x = np.asarray(x).astype(dtype)
    n = x.shape[0]
    dd, off = _shifted(x)
    mask = off.copy()
    if drop_cols is not None:
        mask[:, drop_cols] = False
    log_perp = dtype(np.log(dtype(perplexity)))
    beta = np.ones(n, dtype=dtype)
    bmin = np.full(n, -np.inf, dtype=dtype)
    bmax = np.full(n, np.inf, dtype=dtype)
    used, sum_p, H = beta.copy(), np.ones(n, dtype=dtype), np.zeros(n, dtype=dtype)
    active = np.ones(n, dtype=bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(STEPS):
            idx = np.flatnonzero(active)
            if idx.size == 0:
                break
            b = beta[idx]
            p = np.where(mask[idx], np.exp(-b[:, None] * dd[idx]), dtype(0))
            sp = p.sum(1, dtype=dtype)
            sdp = np.where(mask[idx], dd[idx] * p, dtype(0)).sum(1, dtype=dtype)
            h = np.log(sp) + b * sdp / sp
            used[idx], sum_p[idx], H[idx] = b, sp, h
            diff = h - log_perp
            done = np.abs(diff) <= TOL
            up = ~done & (diff > 0)
            dn = ~done & ~(diff > 0)
            iu, idn = idx[up], idx[dn]
            bmin[iu] = beta[iu]
            beta[iu] = np.where(np.isinf(bmax[iu]), beta[iu] * dtype(2), (beta[iu] + bmax[iu]) * dtype(0.5))
            bmax[idn] = beta[idn]
            beta[idn] = np.where(np.isinf(bmin[idn]), beta[idn] * dtype(0.5), (beta[idn] + bmin[idn]) * dtype(0.5))
            active[idx[done]] = False
        cond = (np.where(mask, np.exp(-used[:, None] * dd), dtype(0)) / sum_p[:, None]).astype(dtype)
    den = dtype(2) * dtype(n)
    P = (cond + cond.T) / den
    if fault is not None and fault[0] == "transpose":
        rs, cs = fault[1], fault[2]
        P[rs, cs] = (cond[rs, cs] + cond[rs, cs]) / den
        P[cs, rs] = (cond[cs, rs] + cond[cs, rs]) / den
    P = np.where(off, np.maximum(P, dtype(P_FLOOR)), dtype(0)).astype(dtype)
    if fault is not None and fault[0] == "rows":
        P[fault[1], :] = 0
    P64 = P.astype(np.float64)
    plogp = float(np.where(P64 > 0, P64 * np.log(np.where(P64 > 0, P64, 1.0)), 0.0).sum())
    return {"P": P, "beta": used, "cond": cond, "H": H, "plogp": plogp, "sum": float(P64.sum())}


def row_entropies(x, beta):
    """float64 entropies of p_{.|i} at the given beta, from float64 distances."""
    dd, off = _shifted(np.asarray(x).astype(np.float64))
    b = np.asarray(beta).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.where(off, np.exp(-b[:, None] * dd), 0.0)
        sdp = np.where(off, dd * p, 0.0).sum(1)
    sp = p.sum(1)
    return np.log(sp) + b * sdp / sp


def kl_grad(P, y, exaggeration=1.0, dtype=np.float64, drop=None):
    """-> (KL, grad (n, 2), Z).  ``drop`` = (row slice, column slice): those pairs are left out of every sum."""
    P = np.asarray(P).astype(dtype)
    y = np.asarray(y).astype(dtype)
    n = y.shape[0]
    diff = y[:, None, :] - y[None, :, :]
    w = dtype(1) / (dtype(1) + (diff * diff).sum(2, dtype=dtype))
    keep = np.ones((n, n), dtype=bool)
    if drop is not None:
        keep[drop[0], drop[1]] = False
    off = keep & ~np.eye(n, dtype=bool)
    Z = np.where(off, w, dtype(0)).sum(dtype=dtype)
    pk = np.where(keep, P, dtype(0))
    attr = ((pk * w)[:, :, None] * diff).sum(1, dtype=dtype)
    rep = (np.where(keep, w * w, dtype(0))[:, :, None] * diff).sum(1, dtype=dtype)
    grad = dtype(4) * (dtype(exaggeration) * attr - rep / Z)
    plogp = np.where(pk > 0, pk * np.log(np.where(pk > 0, pk, dtype(1))), dtype(0)).sum(dtype=dtype)
    plogw = (pk * np.log(w)).sum(dtype=dtype)
    return dtype(plogp - plogw + np.log(Z)), grad.astype(dtype), Z


def run(P, y, update, gains, first_iter, n_iter, learning_rate, early_exaggeration, exaggeration_iters, dtype=np.float64):
    """-> (y, update, gains, kl_trace): n_iter iterations continuing at ``first_iter`` of the schedule."""
    y, update, gains = (np.array(a).astype(dtype) for a in (y, update, gains))
    trace = np.zeros(n_iter, dtype=dtype)
    for k in range(n_iter):
        early = first_iter + k < exaggeration_iters
        kl, grad, _ = kl_grad(P, y, early_exaggeration if early else 1.0, dtype)
        trace[k] = kl
        inc = update * grad < 0
        gains = np.where(inc, gains + dtype(0.2), gains * dtype(0.8))
        gains = np.maximum(gains, dtype(0.01))
        update = dtype(0.5 if early else 0.8) * update - dtype(learning_rate) * (gains * grad)
        y = y + update
    return y, update, gains, trace


# ------------------------------------------------------------------------------------------------------------- geometry
def split_rule(n, row_tile, col_tile):
    """include/mmvae_hip.h: (row tiles, column tiles, column splits) of the gradient sweep"""
    cd = lambda a, b: (a + b - 1) // b
    r, t = cd(n, row_tile), cd(n, col_tile)
    return r, t, max(1, min(t, 64, 2048 // r))


def split_cols(tiles, splits, s, col_tile, n):
    """columns [lo, hi) that column split s of ``splits`` covers"""
    return min(n, (tiles * s // splits) * col_tile), min(n, (tiles * (s + 1) // splits) * col_tile)


# ------------------------------------------------------------------------------------------------------------- errors and cases
def p_error(P, P64):
    """max |P - P64| / max P64"""
    P64 = np.asarray(P64, dtype=np.float64)
    return float(np.abs(np.asarray(P, dtype=np.float64) - P64).max() / P64.max())


def beta_error(beta, beta64):
    """max_i |beta_i - beta64_i| / beta64_i"""
    b64 = np.asarray(beta64, dtype=np.float64)
    return float((np.abs(np.asarray(beta, dtype=np.float64) - b64) / b64).max())


def grad_error(g, g64):
    """max |error| / max |gradient|"""
    g64 = np.asarray(g64, dtype=np.float64)
    return float(np.abs(np.asarray(g, dtype=np.float64) - g64).max() / np.abs(g64).max())


def entropy_miss(x, beta, perplexity):
    """max_i |H64_i(beta_i) - log perplexity|"""
    return float(np.abs(row_entropies(x, beta) - np.log(float(perplexity))).max())


def inputs(n, D, seed=0):
    return np.random.default_rng(1000 * seed + 7 * n + D).standard_normal((n, D)).astype(np.float32)


def embedding(n, scale, seed=0):
    return (np.random.default_rng(77 + 1000 * seed + n).standard_normal((n, 2)) * scale).astype(np.float32)


@functools.lru_cache(maxsize=None)
def affinity_case(n, D, perplexity):
    """Inputs, the float64 reference and the fp32 yardsticks of one affinity case, computed once per process.

    The seed: a search stops at the first step with |H - log perplexity| <= 1e-5, and fp32 distances move H by about 1e-7, so
    in roughly 3 rows of 100 an fp32 search stops one step before or after the float64 one and beta (and with it P) is off by
    that step, about 1e-5 of its value; in every other row the two searches visit the same dyadic numbers and agree exactly.
    On an input where the yardstick happens to take the float64 path in every row its beta error is 0 and its P error one
    rounding, and 4 x that would ask the op for bit-equal searches, which no fp32 implementation can promise.  So a case uses the
    first seed of 0..63 on which the YARDSTICK's beta error is not zero (a property of the reference code alone), seed 0 if
    there is none."""
    first = None
    for seed in range(64):
        x = inputs(n, D, seed)
        ref = affinities(x, perplexity, np.float64)
        y32 = affinities(x, perplexity, np.float32)
        yard = {"p": p_error(y32["P"], ref["P"]), "beta": beta_error(y32["beta"], ref["beta"]),
                "entropy": entropy_miss(x, y32["beta"], perplexity)}
        case = {"x": x, "ref": ref, "yardstick": yard, "seed": seed}
        if yard["beta"] > 0:
            return case
        first = first or case
    return first


@functools.lru_cache(maxsize=None)
def grad_case(n, scale, exaggeration):
    """P (the float64 reference's, rounded to fp32) of a 20-D input at perplexity max(2, min(30, (n - 2) // 3)), a
    seeded y at ``scale``, the float64 KL and gradient, the fp32 yardsticks."""
    perplexity = float(max(2, min(30, (n - 2) // 3)))
    P = affinities(inputs(n, 20, seed=1), perplexity, np.float64)["P"].astype(np.float32)
    y = embedding(n, scale)
    kl, grad, Z = kl_grad(P, y, exaggeration, np.float64)
    kl32, grad32, _ = kl_grad(P, y, exaggeration, np.float32)
    yard = {"grad": grad_error(grad32, grad), "kl": abs(float(kl32) - float(kl))}
    return {"P": P, "y": y, "kl": float(kl), "grad": grad, "Z": float(Z), "yardstick": yard}


def blobs(seed=0):
    """3 x 32 points in 10-D, unit variance, centres on a sphere of radius 10 -> (x fp32 (96, 10), labels (96,))."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((3, 10))
    c = 10.0 * c / np.linalg.norm(c, axis=1, keepdims=True)
    labels = np.repeat(np.arange(3), 32)
    return (c[labels] + rng.standard_normal((96, 10))).astype(np.float32), labels


def separation(emb, labels):
    """-> (share of points whose nearest neighbour has their label, smallest between-cluster / largest within-cluster distance)"""
    emb = np.asarray(emb, dtype=np.float64)
    d = np.sqrt(((emb[:, None, :] - emb[None, :, :]) ** 2).sum(2))
    same = labels[:, None] == labels[None, :]
    nn = np.where(np.eye(len(emb), dtype=bool), np.inf, d).argmin(1)
    return float((labels[nn] == labels).mean()), float(d[~same].min() / d[same].max())
