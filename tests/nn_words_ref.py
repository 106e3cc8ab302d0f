"""Shared reference code of the nearest-word tests (test_cpu_nn_words.py, test_gpu_nn_words.py): float64 direct distances with a
lowest-index arg-min, the error gate of an fp32 score, and the test inputs (built once per process and never modified).

The gate.  The device ranks the words of a query by the fp32 score  s(w) = |w|^2 - 2 q.w : a chain of 300 fused multiply-adds
for the dot product, one more rounding for the subtraction, and the 300-term chain behind |w|^2 -- at most 301 roundings on any
path plus the last one.  To first order each rounding is at most 2^-24 of a partial result, and every partial result of the
dot product is at most |q||w| (Cauchy-Schwarz), of the norm at most |w|^2, so

    |s_fp32(w) - s_exact(w)|  <=  E(w) = 302 * 2^-24 * (|w|^2 + 2 |q| |w|).

d^2(q, w) = |q|^2 + s(w), hence a conforming fp32 implementation can return w instead of the true nearest b only when
d^2(w) - d^2(b) <= E(w) + E(b).  Every norm in the gate is taken in float64.
"""
import functools

import torch

DIM = 300
GATE_C = 302 * 2.0 ** -24
DIST_RTOL, DIST_ATOL = 4 * 2.0 ** -24, 1e-6       # direct-difference bound of the reported distance (issue, tests 2 and 4)


def sqdist64(Q, W):
    """float64 (N, V): sum_k (q_k - w_k)^2 from the differences themselves (no |q|^2 + |w|^2 - 2 q.w expansion)."""
    d = torch.cdist(Q.double(), W.double(), compute_mode="donot_use_mm_for_euclid_dist")
    return d * d


def sqdist64_int(Q, W):
    """The same for small-integer entries, where the expansion is exact in float64 (every term is an integer below 2^53)."""
    Q, W = Q.double(), W.double()
    return (Q * Q).sum(1)[:, None] + (W * W).sum(1)[None, :] - 2.0 * (Q @ W.t())


def sqrt_f32_of_int(d2):
    """The correctly rounded fp32 square root of exact integers below 2^24 (float64 in, float32 out): the float64 root rounded
    to fp32.  The two roundings cannot disagree with one: for a midpoint m between two fp32 values below 70, m^2 is a multiple
    of 2^-38 and is not the integer, so a root that is not itself an fp32 value lies at least 2^-38 / (2 * 70) > 2^-46 from m,
    while float64's rounding moves it by at most 2^-47 there.  NOT ``d2.float().sqrt()``: torch's vectorised fp32 sqrt on the
    CPU is not correctly rounded on every host (seen: 36 of 255 roots of integers near 1200 one ulp off, where the float64
    root, the device's sqrtf and torch's sqrt on the device agree with each other)."""
    assert d2.dtype == torch.float64 and bool((d2 == d2.round()).all()) and float(d2.max()) < 4900.0
    return d2.sqrt().float()


def argmin_lowest(d2):
    """Row-wise arg-min; the LOWEST index among equal minima."""
    m = d2.min(dim=1, keepdim=True).values
    ar = torch.arange(d2.shape[1]).expand_as(d2)
    return torch.where(d2 == m, ar, torch.full_like(ar, d2.shape[1])).min(dim=1).values


def gate(Q, W, idx):
    """E(w_idx[i]) for query i, float64 (N,)."""
    qn = Q.double().norm(dim=1)
    wn = W.double()[idx].norm(dim=1)
    return GATE_C * (wn * wn + 2.0 * qn * wn)


def judge(Q, W, returned, d2=None):
    """Compares returned indices (N,) with the float64 ranking.  -> dict: best (float64 lowest-index arg-min), decided (bool:
    the gap to the second best exceeds E(best) + E(second)), wrong_decided (count), regret_ratio (worst
    (d2(returned) - d2(best)) / (E(returned) + E(best))), undecided_share, min_gap_ratio (smallest gap / gate)."""
    d2 = sqdist64(Q, W) if d2 is None else d2
    returned = returned.cpu().long()
    two = torch.topk(d2, 2, dim=1, largest=False, sorted=True)
    best = argmin_lowest(d2)
    second = torch.where(two.indices[:, 0] == best, two.indices[:, 1], two.indices[:, 0])
    gap = two.values[:, 1] - two.values[:, 0]
    g12 = gate(Q, W, best) + gate(Q, W, second)
    decided = gap > g12
    rows = torch.arange(d2.shape[0])
    regret = d2[rows, returned] - d2[rows, best]
    ratio = regret / (gate(Q, W, returned) + gate(Q, W, best))
    return {"best": best, "decided": decided, "wrong_decided": int((decided & (returned != best)).sum()),
            "regret_ratio": float(ratio.max()), "undecided_share": float((~decided).double().mean()),
            "min_gap_ratio": float((gap / g12).min()), "d2": d2}


def dist_within_bound(dist32, d2_64):
    """|dist - sqrt(d2_64)| <= 4 * 2^-24 * sqrt(d2_64) + 1e-6 everywhere; also returns the worst relative error."""
    ref = d2_64.sqrt()
    err = (dist32.cpu().double() - ref).abs()
    return bool((err <= DIST_RTOL * ref + DIST_ATOL).all()), float((err / ref.clamp_min(1e-30)).max())


# ---------------------------------------------------------------------------------------------------------------- inputs
REAL_N, REAL_V = 512, 4099


@functools.lru_cache(maxsize=None)
def real_inputs():
    """-> W (4099, 300) = 0.4 randn, idx (512,), Q_near = W[idx] + 0.05 randn, Q_rand = 0.4 randn; one generator, seed 1."""
    g = torch.Generator().manual_seed(1)
    W = 0.4 * torch.randn(REAL_V, DIM, generator=g)
    idx = torch.randint(0, REAL_V, (REAL_N,), generator=g)
    Q_near = W[idx] + 0.05 * torch.randn(REAL_N, DIM, generator=g)
    Q_rand = 0.4 * torch.randn(REAL_N, DIM, generator=g)
    return W, idx, Q_near, Q_rand


@functools.lru_cache(maxsize=None)
def real_d2(kind):
    W, _, Q_near, Q_rand = real_inputs()
    return sqdist64(Q_near if kind == "near" else Q_rand, W)


def int_rows(n, seed):
    """(n, 300) float32 with integer entries in {-2..2}: every product, sum and norm of such rows is exact in fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, (n, DIM), generator=g).float()


def duplicate_rows(V, TV, last_split_first):
    """The rows that receive a copy of row 3 (issue, test 1): TV-1, TV, V-1 and the first row of the last split."""
    return sorted({r for r in (TV - 1, TV, V - 1, last_split_first) if 3 < r < V})


@functools.lru_cache(maxsize=None)
def int_tables(V, TV, last_split_first):
    """-> (A, B, C): A has V distinct integer rows; B = A with row 3 copied to duplicate_rows(); C = B with row 3 (the lowest
    copy) replaced by another row, so that the lowest duplicate is the first of duplicate_rows()."""
    A = int_rows(V, 100 + V)
    assert torch.unique(A, dim=0).shape[0] == V
    B = A.clone()
    for r in duplicate_rows(V, TV, last_split_first):
        B[r] = A[3]
    C = B.clone()
    if V > 3:
        C[3] = int_rows(1, 7)[0]
    return A, B, C
