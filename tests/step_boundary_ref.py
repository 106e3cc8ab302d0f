"""References, float32 baselines, stand-in faults, gates and cases of the kernels at the step boundary (csrc/elementwise.hip: adam_kernel,
normal_kernel / keep_mask_kernel / the draws of step_begin_kernel).  Nothing here needs a GPU.  The records and their gate are those
of tests/elementwise_ref.py (``rec_f32``: err / magnitude <= max(4 err32, 2^-22); ``rec_exact``).

Philox4x32-10 is written here from the algorithm's definition (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11):
ten rounds of  (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),  the key raised by the two Weyl
constants between rounds -- and tied to the two published known-answer vectors in tests/test_cpu_step_boundary_ref.py.  The library's
layout on top of it:
  counter  (q lo, q hi, stream, 0x5bd1e995), q = the index of a group of 4 consecutive elements
  key      seed ^ (step * 0x9E3779B97F4A7C15) mod 2^64, low word first
  u01(x)   ((x >> 8) + 0.5f) * 2^-24 in fp32 (x >> 8 = 2^24 - 1 rounds to exactly 1.0)
  mask     u01 >= p, compared in fp32
  normals  Box-Muller: words 0, 1 give elements 4q (cos) and 4q + 1 (sin), words 2, 3 give 4q + 2, 4q + 3; radius sqrt(-2 ln u),
           angle the fp32 product 6.28318530718f * u (its rounding belongs to the definition).  Reference: float64 on the fp32 u and the
           fp32 angle; baseline: the same chain in numpy float32; magnitude of both outputs of a pair: the radius.

Adam: torch.optim.Adam's arithmetic (tied to it on float64 tensors in the CPU test) with the hyper-parameters as the fp32 values the
kernel receives and t = counter + 1.  Baseline: the kernel's order of operations in numpy float32 (no fused multiply-adds).  Records per
launch: m (magnitude b1 |m| + (1 - b1) |s g|), v (likewise, squares), dp = p_old - p_new formed in float64 from the two fp32 values
(magnitude |dp_ref| + half an ulp of p_old: the stored parameter rounds once); every element outside the launch's ranges, the counter,
the skip word and (packed launches) the written-back gradient exact.

``FAULTS``: each name is the float32 emulation with one defect; tests/test_cpu_step_boundary_ref.py shows that the gates below -- the
ones tests/test_gpu_step_boundary.py calls -- pass the fault-free emulation at every case of the GPU module and catch every fault.

The dp record above has the half ulp of p_old in its magnitude, so an element whose dp drowns in the parameter's rounding sets the
baseline (err32 up to 0.5) and the gate cannot see a large wrong dp elsewhere.  ``gate_adam`` therefore adds a sharper record of its own,
"dp past p's rounding": the distance of dp_ref from the interval of updates that would have stored the p_new that was read back, against
step_size (b1 |m| + (1 - b1) |s g|) / denominator (the sum of the absolute terms: m_old and g of opposite signs cancel), same gate.

Worst error / gate over all cases, one MI355X run (tests/test_gpu_step_boundary.py): m 0.25, v 0.28, dp 0.68, dp past p's rounding 0.59,
normal draws 0.48 (1.17e-7 of the radius against 4 err32 = 2.42e-7); everything else exact.
"""
import collections
import itertools

import numpy as np
import torch

from elementwise_ref import describe, rec_exact, rec_f32, violations  # noqa: F401  (re-exported: the test modules use them from here)

F32, F64 = np.float32, np.float64
VOID_MARK = 0x7FC0DEAD
GOLDEN64 = 0x9E3779B97F4A7C15
CTR3 = 0x5BD1E995
TWO_PI_F32 = np.float32(6.28318530718)

ADAM_FAULTS = ("eps_in_root", "bias_t_minus_1", "scale_after_square", "scale_ignored", "tail_dropped", "range2_skipped",
               "no_advance_ignored", "gpk_vec_ignored", "nan_is_void")
DRAW_FAULTS = ("stream_ignored", "seed_hi_dropped", "step_ignored", "words_1_2_swapped", "gt_for_ge", "last_not_written")
FAULTS = ADAM_FAULTS + DRAW_FAULTS


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ====================================================================================================== Philox4x32-10
_M0, _M1, _W0, _W1, _MASK32 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays (or ints) holding 32-bit words, key: two ints -> four uint64 arrays of 32-bit words"""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & _MASK32, int(key[1]) & _MASK32
    m32 = np.uint64(_MASK32)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]             # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + _W0) & _MASK32, (k1 + _W1) & _MASK32
    return c


def draw_words(seed, step, stream, n, fault=None):
    """the 32-bit words behind elements 0 .. n of one (seed, step counter, stream): uint64 [4 ceil(n / 4)]"""
    seed, step = int(seed) & (2 ** 64 - 1), (0 if step is None else int(step)) & (2 ** 64 - 1)
    if fault == "seed_hi_dropped":
        seed &= _MASK32
    if fault == "step_ignored":
        step = 0
    key = seed ^ ((step * GOLDEN64) & (2 ** 64 - 1))
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    sid = 0 if fault == "stream_ignored" else int(stream) & _MASK32
    w = philox4x32_10((q & np.uint64(_MASK32), q >> np.uint64(32), sid, CTR3), (key & _MASK32, key >> 32))
    if fault == "words_1_2_swapped":
        w = [w[0], w[2], w[1], w[3]]
    return np.stack(w, 1).reshape(-1)


def u01(words):
    return ((words >> np.uint64(8)).astype(F32) + F32(0.5)) * F32(2.0 ** -24)


def keep_mask(seed, step, stream, n, p, fault=None, prefill=7):
    """-> uint8 [n]: the exact bytes"""
    u = u01(draw_words(seed, step, stream, n, fault))[:n]
    out = ((u > F32(p)) if fault == "gt_for_ge" else (u >= F32(p))).astype(np.uint8)
    if fault == "last_not_written" and n % 4:
        out[n - 1] = prefill
    return out


def normals(seed, step, stream, n, dtype=F64, fault=None):
    """-> (values [n] of ``dtype``, magnitude [n] float64).  dtype float64: the reference; float32: the baseline / the emulation"""
    u = u01(draw_words(seed, step, stream, n, fault)).reshape(-1, 4)
    ang = (TWO_PI_F32 * u[:, 1::2]).astype(dtype)                          # the fp32 product, then the chain's own precision
    rad = np.sqrt(dtype(-2.0) * np.log(u[:, 0::2].astype(dtype)))
    out = np.stack((rad * np.cos(ang), rad * np.sin(ang)), 2).reshape(-1)[:n]
    mag = np.repeat(np.sqrt(-2.0 * np.log(u[:, 0::2].astype(F64))), 2, 1).reshape(-1)[:n]
    if fault == "last_not_written" and n % 4:
        out[n - 1] = np.nan
    return out, mag


def gate_normals(got, seed, step, stream, n):
    """got: fp32 tensor [n]"""
    r64, mag = normals(seed, step, stream, n, F64)
    r32, _ = normals(seed, step, stream, n, F32)
    return [rec_f32("normal", got, _t(r64), _t(mag), _t(r32))]


def gate_mask(got, seed, step, stream, n, p):
    return [rec_exact("mask p=%g" % p, got, _t(keep_mask(seed, step, stream, n, p)))]


def emulate_normals(seed, step, stream, n, fault=None):
    return _t(normals(seed, step, stream, n, F32, fault)[0])


def emulate_mask(seed, step, stream, n, p, fault=None):
    return _t(keep_mask(seed, step, stream, n, p, fault))


# -- cases ---------------------------------------------------------------------------------------------------------------------------
DRAW_N = (1, 3, 4, 5, 1023, 524293)            # 524293: one vector past 512 blocks x 256 threads x 4 -- the grid-stride loop
DRAW_SEEDS = (0x123456789ABCDEF0, 1234, 0)
DRAW_STEPS = (None, 0, 1, 2 ** 33 + 5)         # None: a null step pointer
DRAW_STREAMS = (1, 2, 3, 4, 5, 0xFFFFFFFF)
MASK_P = (0.0, 0.1, 0.5, 1.0)
# A draw that EQUALS p: x >> 8 = 2^23 gives (2^23 + 0.5) -> 2^23 (ties to even) -> u = 0.5 exactly.  Found by searching the seeds
# 0, 1, 2, ... at step 0 on stream 2 for the first with such a word among its first 20000 draws (seed 3638, element 15511;
# tests/test_cpu_step_boundary_ref.py checks the pin): ">" where ">=" was meant drops exactly this element.
TIE = dict(seed=3638, step=0, stream=2, n=15513, p=0.5, index=15511)


def find_tie(seed, step, stream, n, p):
    """indices of the draws that equal p"""
    return np.nonzero(u01(draw_words(seed, step, stream, n))[:n] == F32(p))[0]


def draw_cases():
    """(n, seed, step, stream).  The key and counter faults do not depend on n: the full product of seeds, steps and streams runs at
    n = 5 and 1023 (the first is asserted to be the prefix of the second); the sizes that are about the tail and the grid-stride loop
    take a diagonal that still has every seed, step and stream once."""
    full = list(itertools.product(DRAW_SEEDS, DRAW_STEPS, DRAW_STREAMS))
    diag = [(DRAW_SEEDS[i % 3], DRAW_STEPS[i % 4], DRAW_STREAMS[i]) for i in range(6)]
    return [(n,) + c for n in DRAW_N for c in (full if n in (5, 1023) else diag)]


# ====================================================================================================== Adam
HYPER = ((1e-3, 0.9, 0.999, 1e-8), (5e-2, 0.5, 0.9, 1e-3), (2e-3, 0.0, 0.99, 1e-6))       # lr, b1, b2, eps
ADAM_N = (1, 3, 4, 5, 1023, 1024, 4101)       # a block covers 1024 elements per pass: 4101 under a cap of 1 is five passes and a tail
ADAM_BLOCKS = (1, 2, None)                    # knob adam_blocks (None: the default)
COUNTERS = (0, 1, 2, 999, 99999)
SCALES = (1.0, 0.125, 1.0 / 3.0)
RANGE_N = 4101
RANGES = ([(0, 8)], [(8, 0), (1024, 2052)], [(0, 4), (4, 4), (4096, 5)], [(16, 1000), (2048, 0), (3000, 4), (4000, 101)])
PARTITION = ([(0, 1024), (2048, 1024)], [(1024, 1024), (3072, 1029)])       # first launch advance = 0, second 1: one whole step
GUARD = 8

Launch = collections.namedtuple("Launch", "p g m v counter skip hyper scale ranges advance gmap gpk gpk_vec")


def f32_hyper(hyper, scale):
    return tuple(F32(x) for x in hyper) + (F32(scale),)


def adam_inputs(n, hyper, counter, scale, seed=None):
    """-> Launch over all of [0, n).  Gradients log-uniform in magnitude over 1e-9 .. 10 with both signs, exact zeros among them;
    m and v carried from a float64 history (``counter`` steps of one constant earlier gradient: m = (1 - b1^c) s g', v = (1 - b2^c)
    (s g')^2, rounded to fp32), so they are consistent with each other and with the counter; a block with g = 0, v = 0 and m != 0;
    parameters of the size of lr, so that dp is not below the parameter's own rounding."""
    rng = np.random.default_rng(8000 + 17 * n + counter if seed is None else seed)
    lr, b1, b2, eps, s = (F64(x) for x in f32_hyper(hyper, scale))

    def loguniform():
        return (rng.choice((-1.0, 1.0), n) * 10.0 ** rng.uniform(-9.0, 1.0, n))
    g, gh = loguniform(), loguniform()
    g[rng.random(n) < 0.1] = 0.0
    m, v = (1 - b1 ** counter) * s * gh, (1 - b2 ** counter) * (s * gh) ** 2
    if n >= 16:
        blk = slice(8, 14)                         # crosses a 4-vector boundary
        g[blk], v[blk], m[blk] = 0.0, 0.0, rng.choice((-1.0, 1.0), 6) * 1e-10 * rng.uniform(0.5, 2.0, 6)
    p = lr * rng.uniform(-2.0, 2.0, n)
    return Launch(p.astype(F32), g.astype(F32), m.astype(F32), v.astype(F32), int(counter), 0, tuple(hyper), float(scale), None, 1,
                  None, None, None)


def packed_inputs(n=RANGE_N, seed=77):
    """a synthetic gradient map with all three kinds of entry: >= 0 (into gpk), -1 (none), < -1 (-(index + 2) into gpk_vec); the first
    4-vector mixes the three, the scalar tail (n % 4 elements) holds a gpk_vec and a gpk entry -> (gmap int32, gpk, gpk_vec)"""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 3, n)
    kind[:4] = (0, 1, 2, 0)
    kind[n - (n % 4 or 4):] = 2
    kind[n - 1] = 0
    gmap = np.full(n, -1, dtype=np.int32)
    n0, n2 = int((kind == 0).sum()), int((kind == 2).sum())
    gmap[kind == 0] = rng.permutation(n0 + 5)[:n0]
    gmap[kind == 2] = -(rng.permutation(n2 + 3)[:n2]) - 2
    return gmap, rng.standard_normal(n0 + 5).astype(F32), rng.standard_normal(n2 + 3).astype(F32)


def _is_mark(x):
    return (int(np.asarray(x, dtype=F32).view(np.uint32)) & 0x7FFFFFFF) == VOID_MARK


def adam_launch(L, dtype=F64, fault=None):
    """One launch of the optimizer kernel on ``L`` -> dict(p, m, v [n], g_out [n] (packed launches), counter, skip, touched [n] bool).
    dtype float64: the reference (outputs float64); float32: the kernel's order of operations in numpy float32 (outputs float32)."""
    n = L.p.shape[0]
    lr, b1, b2, eps, s = (dtype(x) for x in f32_hyper(L.hyper, L.scale))
    ranges = [(0, n)] if L.ranges is None else list(L.ranges)
    if fault == "range2_skipped" and len(ranges) >= 3:
        ranges = ranges[:1] + ranges[2:]
    touched = np.zeros(n, dtype=bool)
    for o, l in ranges:
        touched[o:o + l] = True
        if fault == "tail_dropped" and l % 4:
            touched[o + l - l % 4:o + l] = False
    out = dict(p=L.p.astype(dtype), m=L.m.astype(dtype), v=L.v.astype(dtype), counter=L.counter, skip=0, touched=touched)
    g = L.g.copy()
    if L.gmap is not None:                           # one fp32 add, whatever the precision of the rest
        pk, vec = L.gmap >= 0, L.gmap < -1
        g[pk] = g[pk] + L.gpk[L.gmap[pk]]
        if fault != "gpk_vec_ignored":
            g[vec] = g[vec] + L.gpk_vec[-L.gmap[vec] - 2]
        out["g_out"] = np.where(touched, g, L.g)
    void = L.skip != 0 or _is_mark(L.g[0]) or (fault == "nan_is_void" and bool(np.isnan(L.g).any()))
    if void:                                         # nothing moves, the step is not counted, the skip word is taken down
        out["touched"] = np.zeros(n, dtype=bool)
        if L.gmap is not None:
            out["g_out"] = L.g.copy()
        return out
    t = L.counter + 1
    tb = t - 1 if fault == "bias_t_minus_1" else t
    one = dtype(1.0)
    with np.errstate(all="ignore"):
        bc1, bc2 = one - np.power(b1, dtype(tb)), one - np.power(b2, dtype(tb))
        step_size, inv_sqrt_bc2 = lr / bc1, one / np.sqrt(bc2)
        gj = g.astype(dtype) * (one if fault == "scale_ignored" else s)
        m = b1 * out["m"] + (one - b1) * gj
        if fault == "scale_after_square":
            v = b2 * out["v"] + (one - b2) * (g.astype(dtype) * g.astype(dtype)) * s
        else:
            v = b2 * out["v"] + ((one - b2) * gj) * gj
        den = np.sqrt(v + eps) * inv_sqrt_bc2 if fault == "eps_in_root" else np.sqrt(v) * inv_sqrt_bc2 + eps
        p = out["p"] - step_size * m / den
    for k, new in (("p", p), ("m", m), ("v", v)):
        out[k] = np.where(touched, new, out[k])
    if L.advance or fault == "no_advance_ignored":
        out["counter"] = t
    return out


def emulate_adam(L, fault=None):
    """what a float32 kernel (with one fault) leaves behind, as the GPU test reads it back"""
    return adam_launch(L, F32, fault)


def _ulp_half(x):
    return 0.5 * np.spacing(np.abs(x.astype(F32))).astype(F64)


def _dp_past_rounding(p_old, p_new, dp_ref):
    """|dp_ref - d| for the d nearest to dp_ref among those with fl32(p_old - d) == p_new: what of a stored parameter's distance from
    the reference the rounding of the store cannot explain (0 where dp_ref itself would have stored p_new) -> float64 [n]"""
    p_new = p_new.astype(F32)
    hi = 0.5 * (p_new.astype(F64) + np.nextafter(p_new, F32(np.inf)).astype(F64))
    lo = 0.5 * (p_new.astype(F64) + np.nextafter(p_new, F32(-np.inf)).astype(F64))
    d_lo, d_hi = p_old - hi, p_old - lo
    return np.maximum(0.0, np.maximum(d_lo - dp_ref, dp_ref - d_hi))


def gate_adam(got, L):
    """got: dict(p, m, v fp32 arrays [n], counter, skip, g_out for a packed launch), read back after the launch on ``L``"""
    r64, r32 = adam_launch(L, F64), adam_launch(L, F32)
    tch = r64["touched"]
    _, b1, b2, _, s = (F64(x) for x in f32_hyper(L.hyper, L.scale))
    g = L.g.copy()
    if L.gmap is not None:
        g = r64["g_out"] if tch.any() else g
    gj = np.abs(g.astype(F64) * s)
    mag = dict(m=b1 * np.abs(L.m.astype(F64)) + (1 - b1) * gj, v=b2 * np.abs(L.v.astype(F64)) + (1 - b2) * gj * gj)
    p_old = L.p.astype(F64)
    fin = tch & np.isfinite(r64["p"]) & np.isfinite(r64["m"]) & np.isfinite(r64["v"])        # a NaN gradient: exact pattern below
    recs = []
    for k in ("m", "v"):
        recs.append(rec_f32(k, _t(got[k][fin]), _t(r64[k][fin]), _t(mag[k][fin]), _t(r32[k][fin])))
    dp64 = p_old - r64["p"]
    recs.append(rec_f32("dp", _t((p_old - got["p"].astype(F64))[fin]), _t(dp64[fin]), _t((np.abs(dp64) + _ulp_half(L.p))[fin]),
                        _t((p_old - r32["p"].astype(F64))[fin])))
    # The half ulp in that magnitude lets an element whose dp is below the parameter's rounding set the baseline (err32 up to 0.5), and
    # the gate is then blind to an element with a large, wrong dp.  So a second, sharper record: the part of the error that the rounding of
    # the stored parameter cannot explain, against the magnitude of dp alone -- step_size (b1 |m| + (1 - b1) |s g|) / denominator, the
    # sum of the absolute terms as everywhere (m_old and g of opposite signs cancel in m, and dp inherits that) -- with the same gate,
    # the baseline measured the same way.
    with np.errstate(all="ignore"):
        past, past32 = (_dp_past_rounding(p_old, x["p"], dp64)[fin] for x in (got, r32))
        ratio = np.where(r64["m"] != 0, mag["m"] / np.abs(r64["m"]), 1.0)
        dp_mag = np.maximum(np.abs(dp64) * ratio, np.abs(dp64))[fin]
    zero = np.zeros_like(past)
    recs.append(rec_f32("dp past p's rounding", _t(past), _t(zero), _t(dp_mag), _t(past32)))
    for k, before in (("p", L.p), ("m", L.m), ("v", L.v)):
        recs.append(rec_exact(k + " outside the ranges", _t(got[k][~tch]), _t(before[~tch])))
        recs.append(rec_exact(k + " NaN where the reference has one", _t(np.isnan(got[k][tch & ~fin])), _t(np.isnan(r64[k][tch & ~fin]))))
    if L.gmap is not None:
        recs.append(rec_exact("g_out", _t(got["g_out"]), _t(r64["g_out"])))
    recs.append(rec_exact("counter", torch.tensor(int(got["counter"])), torch.tensor(int(r64["counter"]))))
    recs.append(rec_exact("skip word and ticket", torch.tensor(int(got["skip"])), torch.tensor(0)))
    return recs


def carry(L, got, **kw):
    """the next launch's inputs: what a launch left (``got``), new fields from ``kw``"""
    if L.gmap is not None:
        kw.setdefault("g", np.asarray(got["g_out"], dtype=F32))              # a packed launch completes the gradient of its ranges in place
    return L._replace(p=got["p"].astype(F32), m=got["m"].astype(F32), v=got["v"].astype(F32), counter=int(got["counter"]), skip=0, **kw)


def adam_cases():
    """(n, hyper, counter, scale) of the whole-buffer launches; each runs under every entry of ADAM_BLOCKS"""
    return list(itertools.product(ADAM_N, HYPER, COUNTERS, SCALES))


def packed_base(hyper=HYPER[0], counter=2, scale=0.125):
    """a launch over RANGE_N elements on a packed gradient (the synthetic map)"""
    gmap, gpk, gvec = packed_inputs()
    return adam_inputs(RANGE_N, hyper, counter, scale)._replace(gmap=gmap, gpk=gpk, gpk_vec=gvec)


def range_launches():
    """Launches over RANGE_N elements: every entry of RANGES with advance 1 and 0, on a packed gradient (synthetic map)"""
    base = packed_base()
    return [base._replace(ranges=r, advance=a) for r in RANGES for a in (1, 0)]


def void_launches():
    """(name, launch): the void mark in g[0] with either sign, the skip word, a quiet NaN of another payload in g[5]"""
    base = adam_inputs(1023, HYPER[0], 2, 1.0)
    out = []
    for name, bits in (("mark +", VOID_MARK), ("mark -", VOID_MARK | 0x80000000)):
        g = base.g.copy()
        g[:1] = np.array([bits], dtype=np.uint32).view(F32)
        out.append((name, base._replace(g=g)))
    out.append(("skip word", base._replace(skip=1)))
    for name, bits in (("NaN 0x7fc00000", 0x7FC00000), ("NaN 0x7fc0dea5", 0x7FC0DEA5), ("NaN 0xffc0dead at 5", VOID_MARK | 0x80000000)):
        g = base.g.copy()
        g[5:6] = np.array([bits], dtype=np.uint32).view(F32)
        out.append((name, base._replace(g=g)))
    return out
