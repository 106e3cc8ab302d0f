"""GPU tests of the t-SNE op (csrc/tsne.hip) through the C boundary, against float64 numpy (tests/tsne_ref.py).

Real-valued cases: every gate is 4 x the error of the same algorithm in fp32 numpy on the CPU (the yardstick), on the same input,
against float64; the ten-iteration run is gated at 8 x, because the errors of ten dependent steps compound.  Longer trajectories
are not compared: the optimisation is chaotic (fp32 against float64 in numpy: 2e-5 after 10 iterations, of order 1 after 50).
tests/test_cpu_tsne.py shows that each gate sees a dropped row tile, column tile, column split and transpose half.

Exact cases: identical rows give P_ij = 1 / (n (n - 1)) and a search that runs out of steps; identical y give a gradient of exact
zeros and Z = n (n - 1) exactly at n = 4099, above 2^24.

N = 4 runs at perplexity 2: no listed perplexity is below (4 - 1) / 3, and 2 is the only one the op's own limit
(perplexity < n - 1) admits.

MEASURED on an MI355X (error of the op / yardstick; `pytest -s` prints them): see MEASURED below and profiles/tsne_bench.txt.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsne_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

MEASURED = """
error of the op / yardstick (= error of the same algorithm in fp32 numpy on the CPU), both against float64; MI355X
affinities (N, D, perplexity), gates 4 x, 4 x and 1e-5 + yardstick:
(N, D, perplexity)  seed  max |dP| / max P      max |dbeta| / beta   max |H64(beta) - log perplexity|
(4, 2, 2)         51    6.1e-08 / 8.9e-06   0 / 9.2e-05         9.9e-06 / 7.5e-06
(31, 1, 2)        1     1.4e-07 / 1.1e-05   0 / 2.2e-04         1.0e-05 / 9.5e-06
(33, 20, 5)       2     2.7e-06 / 2.7e-06   1.0e-05 / 1.0e-05   9.0e-06 / 9.0e-06
(63, 50, 5)       0     3.0e-06 / 2.6e-06   5.6e-06 / 7.3e-06   1.0e-05 / 1.0e-05
(64, 256, 2)      0     8.3e-06 / 8.3e-06   3.7e-05 / 2.6e-05   1.5e-05 / 1.8e-05
(65, 2, 5)        3     2.8e-07 / 4.6e-06   0 / 1.3e-05         9.8e-06 / 9.8e-06
(127, 20, 30)     0     2.3e-07 / 1.9e-06   0 / 6.5e-06         9.9e-06 / 9.8e-06
(129, 50, 30)     0     4.0e-07 / 4.0e-06   0 / 3.2e-06         9.8e-06 / 9.8e-06
(257, 1, 30)      0     7.6e-08 / 4.7e-06   0 / 3.2e-05         1.0e-05 / 1.0e-05
(1031, 20, 30)    0     4.0e-06 / 2.9e-06   6.7e-06 / 7.6e-06   1.0e-05 / 1.0e-05
A beta error of 0: the op's search stopped at the step of the float64 search in every row.  The largest ratios: P 1.4 at
(1031, 20, 30), beta 1.4 at (64, 256, 2).
gradient and KL (N, scale of y, exaggeration), gates 4 x:
(N, scale, e)       max |dgrad| / max |grad|  |dKL|
(4, 0.0001, 1)      1.3e-07 / 2.4e-07   1.5e-08 / 1.5e-08
(31, 0.0001, 1)     1.5e-07 / 3.8e-07   1.6e-08 / 2.5e-07
(33, 0.0001, 1)     1.1e-07 / 4.2e-07   3.4e-08 / 3.4e-08
(63, 0.0001, 1)     1.0e-07 / 3.4e-07   1.6e-08 / 1.4e-07
(64, 0.0001, 1)     1.4e-07 / 4.0e-07   1.6e-08 / 4.4e-08
(65, 0.0001, 1)     7.0e-08 / 5.7e-07   2.6e-08 / 4.5e-07
(127, 0.0001, 1)    7.3e-08 / 1.4e-06   4.7e-08 / 1.7e-07
(129, 0.0001, 1)    7.5e-08 / 5.1e-07   5.7e-08 / 1.8e-07
(257, 0.0001, 1)    3.0e-08 / 8.3e-07   5.0e-08 / 1.9e-07
(1031, 0.0001, 1)   5.6e-08 / 9.5e-07   1.2e-07 / 1.3e-06
(4, 0.0001, 12)     5.2e-08 / 4.6e-08   1.5e-08 / 1.5e-08
(31, 0.0001, 12)    5.0e-08 / 1.9e-07   1.6e-08 / 2.5e-07
(33, 0.0001, 12)    5.4e-08 / 1.8e-07   3.4e-08 / 3.4e-08
(63, 0.0001, 12)    6.5e-08 / 1.6e-07   1.6e-08 / 1.4e-07
(64, 0.0001, 12)    3.8e-08 / 2.2e-07   1.6e-08 / 4.4e-08
(65, 0.0001, 12)    6.7e-08 / 2.0e-07   2.6e-08 / 4.5e-07
(127, 0.0001, 12)   3.8e-08 / 5.3e-07   4.7e-08 / 1.7e-07
(129, 0.0001, 12)   3.7e-08 / 2.3e-07   5.7e-08 / 1.8e-07
(257, 0.0001, 12)   2.8e-08 / 6.6e-07   5.0e-08 / 1.9e-07
(1031, 0.0001, 12)  5.3e-08 / 8.1e-07   1.2e-07 / 1.3e-06
(4, 10, 1)          7.9e-08 / 1.8e-07   1.5e-08 / 1.6e-07
(31, 10, 1)         2.1e-07 / 2.1e-07   1.1e-07 / 5.9e-07
(33, 10, 1)         9.8e-08 / 1.9e-07   1.9e-09 / 1.2e-07
(63, 10, 1)         2.1e-07 / 3.4e-07   1.2e-07 / 3.5e-07
(64, 10, 1)         9.9e-08 / 3.2e-07   2.9e-08 / 5.1e-07
(65, 10, 1)         1.5e-07 / 2.3e-07   7.5e-08 / 7.5e-08
(127, 10, 1)        1.2e-07 / 3.3e-07   1.5e-09 / 4.8e-07
(129, 10, 1)        1.4e-07 / 2.7e-07   1.2e-07 / 6.0e-07
(257, 10, 1)        7.2e-08 / 2.6e-07   2.2e-08 / 2.2e-08
(1031, 10, 1)       1.3e-07 / 1.2e-06   1.2e-07 / 2.0e-06
(4, 10, 12)         9.3e-08 / 1.0e-07   1.5e-08 / 1.6e-07
(31, 10, 12)        2.6e-07 / 1.7e-07   1.1e-07 / 5.9e-07
(33, 10, 12)        7.1e-08 / 1.5e-07   1.9e-09 / 1.2e-07
(63, 10, 12)        5.8e-08 / 2.2e-07   1.2e-07 / 3.5e-07
(64, 10, 12)        7.6e-08 / 1.6e-07   2.9e-08 / 5.1e-07
(65, 10, 12)        1.0e-07 / 2.2e-07   7.5e-08 / 7.5e-08
(127, 10, 12)       6.6e-08 / 1.9e-07   1.5e-09 / 4.8e-07
(129, 10, 12)       6.9e-08 / 2.7e-07   1.2e-07 / 6.0e-07
(257, 10, 12)       3.5e-08 / 2.1e-07   2.2e-08 / 2.2e-08
(1031, 10, 12)      7.5e-08 / 7.3e-07   1.2e-07 / 2.0e-06
Where the two KL figures agree the error is the rounding of the exact KL to fp32.  The largest ratios: gradient 1.6 at (31, 10, 12), KL 1.0.
ten iterations at N = 96 against float64, max |dy| / max |y|: 3.9e-07 / 8.1e-07 (gate 8 x); KL 1.020 -> 1.519 (exaggerated phase)
three blobs, 300 iterations: purity 1.0, smallest between / largest within distance 1.67, KL 2.115 -> 0.434
"""

def _geometry():
    from multimodal_vae_amd.tsne import tsne_geometry               # (the library loads without a GPU)
    return tsne_geometry()


# row_tile, col_tile, sym_tile, row_threads of the kernels: the cases move with them
RT, CT, ST, AT, MAX_DIM = _geometry()
AFFINITY_CASES = [(4, 2, 2.0), (ST - 1, 1, 2.0), (ST + 1, 20, 5.0), (RT - 1, 50, 5.0), (RT, MAX_DIM, 2.0), (RT + 1, 2, 5.0),
                  (CT - 1, 20, 30.0), (CT + 1, 50, 30.0), (AT + 1, 1, 30.0), (1031, 20, 30.0)]
SIZES = [c[0] for c in AFFINITY_CASES]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _report(label, **kw):
    print("TSNE %-34s %s" % (label, "  ".join("%s %.3e" % (k, v) for k, v in kw.items())))


def _ws(n, dev):
    from multimodal_vae_amd._lib import call
    need = call("mmvae_tsne_workspace_bytes", n)
    return torch.empty(need, dtype=torch.uint8, device=dev), need


def _affinities(x, perplexity, dev):
    from multimodal_vae_amd._lib import call, ptr
    xd = torch.as_tensor(x).to(dev).contiguous()
    n, dim = xd.shape
    ws, need = _ws(n, dev)
    P = torch.empty(n, n, device=dev)
    beta, out = torch.empty(n, device=dev), torch.empty(2, device=dev)
    call("mmvae_tsne_affinities", ptr(xd), n, dim, float(perplexity), ptr(P), ptr(beta), ptr(out), ptr(ws), need, _stream())
    return P.cpu().numpy(), beta.cpu().numpy(), out.cpu().numpy()


def _grad(P, y, exaggeration, dev, ws=None):
    from multimodal_vae_amd._lib import call, ptr
    Pd, yd = torch.as_tensor(P).to(dev).contiguous(), torch.as_tensor(y).to(dev).contiguous()
    n = yd.shape[0]
    if ws is None:
        ws, _ = _ws(n, dev)
    grad, out = torch.empty_like(yd), torch.empty(3, device=dev)
    call("mmvae_tsne_grad", ptr(Pd), float(exaggeration), ptr(yd), n, ptr(ws), ws.numel(), ptr(grad), ptr(out), _stream())
    return grad.cpu().numpy(), out.cpu().numpy()


def _run(Pd, y, update, gains, first_iter, n_iter, lr, ee, ex_iters, dev, ws=None):
    """-> (y, update, gains, trace) as device tensors; the inputs are not modified"""
    from multimodal_vae_amd._lib import call, ptr
    y, update, gains = (torch.as_tensor(a).to(dev).clone().contiguous() for a in (y, update, gains))
    n = y.shape[0]
    if ws is None:
        ws, _ = _ws(n, dev)
    trace = torch.empty(n_iter, device=dev)
    call("mmvae_tsne_run", ptr(Pd), n, ptr(y), ptr(update), ptr(gains), first_iter, n_iter, float(lr), float(ee), ex_iters, ptr(trace),
         ptr(ws), ws.numel(), _stream())
    return y, update, gains, trace


def test_cases_cover_the_geometry():
    rt, ct, st, at, md = _geometry()
    assert {rt - 1, rt, rt + 1, ct - 1, ct + 1, st - 1, st + 1, at + 1, 4} <= set(SIZES)
    assert R.split_rule(1031, rt, ct)[2] >= 2 and 1031 > 4 * at
    assert {c[1] for c in AFFINITY_CASES} == {1, 2, 20, 50, md} and {c[2] for c in AFFINITY_CASES} == {2.0, 5.0, 30.0}
    assert all(p < (n - 1) / 3 for n, _, p in AFFINITY_CASES if n != 4)


# ------------------------------------------------------------------------------------------------------ affinities
@pytest.mark.parametrize("n,D,perplexity", AFFINITY_CASES)
def test_affinities(n, D, perplexity):
    dev = _dev()
    c = R.affinity_case(n, D, perplexity)
    P, beta, out = _affinities(c["x"], perplexity, dev)
    ref, yard = c["ref"], c["yardstick"]
    assert np.array_equal(P, P.T), "P is not symmetric bit for bit"
    assert not P.diagonal().any() and P[~np.eye(n, dtype=bool)].min() >= np.float32(R.P_FLOOR)
    err = {"p": R.p_error(P, ref["P"]), "beta": R.beta_error(beta, ref["beta"]), "entropy": R.entropy_miss(c["x"], beta, perplexity)}
    _report("affinities (%d, %d, %g) seed %d" % (n, D, perplexity, c["seed"]), **err, **{"yard_" + k: v for k, v in yard.items()})
    assert err["p"] <= R.GATE_FACTOR * yard["p"], (err["p"], yard["p"])
    assert err["beta"] <= R.GATE_FACTOR * yard["beta"], (err["beta"], yard["beta"])
    assert err["entropy"] <= R.TOL + yard["entropy"], (err["entropy"], yard["entropy"])
    P64 = P.astype(np.float64)
    plogp = float((P64[P64 > 0] * np.log(P64[P64 > 0])).sum())
    assert abs(float(out[0]) - plogp) <= 2e-7 * abs(plogp) and abs(float(out[1]) - P64.sum()) <= 2e-7      # float64 folds, one rounding


def test_identical_rows_exhaust_the_search():
    dev = _dev()
    n = 65
    P, beta, out = _affinities(np.full((n, 3), 0.75, dtype=np.float32), 5.0, dev)
    want = np.float32(1.0 / 4160.0)
    off = ~np.eye(n, dtype=bool)
    ulp = np.spacing(want)
    assert np.abs(P[off].astype(np.float64) - np.float64(want)).max() <= 2 * ulp and not P.diagonal().any()
    assert np.all(beta == np.float32(2.0 ** (R.STEPS - 1)))         # doubled at every one of the 100 steps but the last
    assert abs(float(out[1]) - 1.0) < 1e-6


# ------------------------------------------------------------------------------------------------------ gradient / KL
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("scale,exaggeration", [(1e-4, 1.0), (1e-4, 12.0), (10.0, 1.0), (10.0, 12.0)])
def test_gradient_and_kl(n, scale, exaggeration):
    dev = _dev()
    c = R.grad_case(n, scale, exaggeration)
    grad, out = _grad(c["P"], c["y"], exaggeration, dev)
    err = {"grad": R.grad_error(grad, c["grad"]), "kl": abs(float(out[0]) - c["kl"])}
    _report("grad (%d, %g, %g)" % (n, scale, exaggeration), **err, **{"yard_" + k: v for k, v in c["yardstick"].items()})
    for k in err:
        assert err[k] <= R.GATE_FACTOR * c["yardstick"][k], (k, err[k], c["yardstick"][k])
    assert abs(float(out[1]) - c["Z"]) <= 2e-7 * c["Z"]


def test_identical_points_give_zero_gradient_and_exact_z():
    dev = _dev()
    n = 4099
    assert n * (n - 1) > 2 ** 24
    P = torch.full((n, n), 1.0 / (n * (n - 1)), device=dev)
    P.fill_diagonal_(0.0)
    y = torch.tensor([0.25, -1.5]).repeat(n, 1)
    grad, out = _grad(P, y, 12.0, dev)
    assert not grad.any()
    assert float(out[1]) == float(n * (n - 1))
    assert abs(float(out[0])) < 1e-5                                # P = Q: the KL vanishes


def test_gradient_reads_p_through_its_transpose():
    """the documented contract: P must be symmetric, because the sweep reads P_ji where the formula says P_ij.  An unsymmetric
    P gives the gradient and KL of its transpose, not garbage and not a fault."""
    dev = _dev()
    c = R.grad_case(CT + 1, 10.0, 1.0)
    n = CT + 1
    skew = (c["P"] * (1.0 + 0.5 * np.triu(np.ones((n, n), dtype=np.float32), 1))).astype(np.float32)
    assert not np.array_equal(skew, skew.T)
    grad, out = _grad(skew, c["y"], 1.0, dev)
    kl_t, grad_t, _ = R.kl_grad(skew.T, c["y"], 1.0)
    kl_s, grad_s, _ = R.kl_grad(skew, c["y"], 1.0)
    kl_32, grad_32, _ = R.kl_grad(skew.T, c["y"], 1.0, np.float32)                      # the yardstick on this input
    assert R.grad_error(grad, grad_t) <= R.GATE_FACTOR * R.grad_error(grad_32, grad_t) < R.grad_error(grad, grad_s)
    assert abs(float(out[0]) - float(kl_t)) <= R.GATE_FACTOR * abs(float(kl_32) - float(kl_t))       # (the KL of P^T is that of P)


# ------------------------------------------------------------------------------------------------------ run
N_RUN = 96


def _run_case():
    c = R.grad_case(N_RUN, 1e-4, 1.0)
    return c["P"], c["y"], np.zeros_like(c["y"]), np.ones_like(c["y"])


def test_ten_iterations_against_float64():
    dev = _dev()
    P, y0, u0, g0 = _run_case()
    args = (0, 10, 20.0, 12.0, 6)                                   # the schedule changes inside the ten iterations
    y64, _, _, t64 = R.run(P, y0, u0, g0, *args)
    y32, _, _, _ = R.run(P, y0, u0, g0, *args, dtype=np.float32)
    y, _, _, trace = _run(torch.as_tensor(P).to(dev), y0, u0, g0, *args, dev)
    scale = np.abs(y64).max()
    yard = float(np.abs(y32.astype(np.float64) - y64).max() / scale)
    err = float(np.abs(y.cpu().numpy().astype(np.float64) - y64).max() / scale)
    _report("run 10 iterations, N = %d" % N_RUN, err=err, yard=yard, kl0=float(trace[0]), kl9=float(trace[-1]))
    assert err <= R.RUN_GATE_FACTOR * yard, (err, yard)
    assert np.abs(trace.cpu().numpy() - t64).max() <= 1e-4


def test_run_continues_and_repeats_bit_for_bit():
    dev = _dev()
    P, y0, u0, g0 = _run_case()
    Pd = torch.as_tensor(P).to(dev)
    ws, _ = _ws(N_RUN, dev)
    full = _run(Pd, y0, u0, g0, 0, 10, 20.0, 12.0, 6, dev, ws)
    ws.fill_(0xFF)                                                  # NaN in every float64 of the workspace
    a = _run(Pd, y0, u0, g0, 0, 5, 20.0, 12.0, 6, dev, ws)
    ws.fill_(0xFF)
    b = _run(Pd, a[0], a[1], a[2], 5, 5, 20.0, 12.0, 6, dev, ws)
    bits = lambda t: t.view(torch.int32)
    for u, v in zip(full[:3], b[:3]):
        assert bool(torch.isfinite(v).all()) and torch.equal(bits(u), bits(v))
    assert torch.equal(bits(full[3]), bits(torch.cat((a[3], b[3]))))
    ws.fill_(0xFF)
    again = _run(Pd, y0, u0, g0, 0, 10, 20.0, 12.0, 6, dev, ws)
    assert all(torch.equal(bits(u), bits(v)) for u, v in zip(full, again))


def test_two_calls_give_identical_bits():
    dev = _dev()
    c = R.affinity_case(CT + 1, 50, 30.0)
    P1, b1, o1 = _affinities(c["x"], 30.0, dev)
    P2, b2, o2 = _affinities(c["x"], 30.0, dev)
    assert np.array_equal(P1, P2) and np.array_equal(b1, b2) and np.array_equal(o1, o2)
    g = R.grad_case(1031, 10.0, 12.0)
    ws, _ = _ws(1031, dev)
    g1, k1 = _grad(g["P"], g["y"], 12.0, dev, ws)
    ws.fill_(0xFF)
    g2, k2 = _grad(g["P"], g["y"], 12.0, dev, ws)
    assert np.isfinite(g2).all() and np.array_equal(g1.view(np.int32), g2.view(np.int32)) and np.array_equal(k1.view(np.int32), k2.view(np.int32))


# ------------------------------------------------------------------------------------------------------ end to end
def test_three_blobs_separate():
    from multimodal_vae_amd import tsne as T
    dev = _dev()
    x, labels = R.blobs()
    xd = torch.from_numpy(x).to(dev)
    y, trace = T.tsne(xd, perplexity=10.0, n_iter=300, learning_rate=20.0, exaggeration_iters=100, seed=0, return_trace=True)
    assert y.shape == (96, 2) and trace.shape == (300,) and bool(torch.isfinite(y).all())
    purity, ratio = R.separation(y.cpu().numpy(), labels)
    _report("blobs", purity=purity, ratio=ratio, kl_first=float(trace[0]), kl_last=float(trace[-1]))
    assert purity == 1.0 and ratio > 1.0
    assert float(trace[-1]) < 1.0 and float(trace[-1]) < float(trace[0])
    # the module's functions are the C entry points: the KL of the final state is the next iteration's trace entry
    P, beta = T.joint_probabilities(xd, 10.0)
    kl, grad = T.kl_grad(P, y)
    assert kl.dim() == 0 and grad.shape == (96, 2) and abs(float(kl) - float(trace[-1])) < 0.05
    y2 = T.tsne(xd, perplexity=10.0, n_iter=300, learning_rate=20.0, exaggeration_iters=100, init=T.initial_embedding(96, 0))
    assert torch.equal(y2, y)


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_do_not_launch():
    from multimodal_vae_amd import MMVAEError, tsne as T
    from multimodal_vae_amd._lib import call, ptr
    dev = _dev()
    x = torch.zeros(8, 4, device=dev)
    P = torch.full((8, 8), 7.0, device=dev)
    beta, out = torch.full((8,), 7.0, device=dev), torch.full((3,), 7.0, device=dev)
    ws, need = _ws(8, dev)
    for args in ([ptr(x), 8, 4, 7.0, ptr(P), ptr(beta), ptr(out), ptr(ws), need, _stream()],
                 [ptr(x), 8, 4, 0.5, ptr(P), ptr(beta), ptr(out), ptr(ws), need, _stream()],
                 [ptr(x), 8, 0, 2.0, ptr(P), ptr(beta), ptr(out), ptr(ws), need, _stream()],
                 [ptr(x), 2, 4, 2.0, ptr(P), ptr(beta), ptr(out), ptr(ws), need, _stream()],
                 [ptr(x), 8, 4, 2.0, ptr(P), ptr(beta), ptr(out), ptr(ws), need - 1, _stream()]):
        with pytest.raises(MMVAEError):
            call("mmvae_tsne_affinities", *args)
    with pytest.raises(MMVAEError):
        call("mmvae_tsne_grad", ptr(P), 0.0, ptr(x), 8, ptr(ws), need, ptr(beta), ptr(out), _stream())
    torch.cuda.synchronize()
    assert bool((P == 7.0).all()) and bool((beta == 7.0).all()) and bool((out == 7.0).all())       # nothing ran
    for bad in (lambda: T.joint_probabilities(x, 7.0), lambda: T.joint_probabilities(x.double(), 2.0),
                lambda: T.joint_probabilities(torch.zeros(2, 4, device=dev), 1.0), lambda: T.kl_grad(P, torch.zeros(7, 2, device=dev)),
                lambda: T.kl_grad(P, torch.zeros(8, 3, device=dev)), lambda: T.tsne(x, perplexity=2.0, n_iter=0),
                lambda: T.tsne(x, perplexity=2.0, init=torch.zeros(7, 2))):
        with pytest.raises(MMVAEError):
            bad()


# ------------------------------------------------------------------------------------------------------ the commands
def _checkpoint(tmp_path, n_latents):
    from multimodal_vae_amd.mnist import MultimodalVAE
    torch.manual_seed(n_latents)
    vae = MultimodalVAE(n_latents=n_latents)
    path = os.path.join(str(tmp_path), "mnist_%d.pth.tar" % n_latents)
    torch.save({"state_dict": vae.state_dict(), "n_latents": n_latents}, path)
    return path


def test_manifold_command(tmp_path):
    from multimodal_vae_amd import data as D, evaluate as E
    from multimodal_vae_amd.tsne import pca
    _dev()
    path = _checkpoint(tmp_path, 20)
    out_dir = os.path.join(str(tmp_path), "out")
    out = E.main(["manifold", path, "--synthetic", "256", "--n_iter", "20", "--out", out_dir])
    saved = torch.load(os.path.join(out_dir, "manifold.pt"), weights_only=False)
    assert set(out) == set(saved) == {"latents", "labels", "embedding", "kl_trace"}
    assert out["latents"].shape == (256, 20) and out["embedding"].shape == (256, 2) and out["kl_trace"].shape == (20,)
    assert all(bool(torch.isfinite(out[k]).all()) for k in ("latents", "embedding", "kl_trace"))
    assert torch.equal(out["labels"], D.synthetic_mnist(256, seed=0)[1]) and torch.equal(saved["embedding"], out["embedding"])
    only = E.main(["manifold", path, "--synthetic", "256", "--pca_only", "--out", out_dir])
    assert only["kl_trace"] is None and torch.equal(only["latents"], out["latents"])
    assert torch.equal(only["embedding"], pca(only["latents"], 2)[0])


def test_latent_viz_command(tmp_path):
    """the real 2-latent MultimodalVAE through load_checkpoint: every checked tile against that grid point decoded alone, and
    against the module's own layers as float64 torch ops on the CPU (fp32 kernels: the module tests' 1e-5)"""
    from multimodal_vae_amd import evaluate as E
    from multimodal_vae_amd.mnist import load_checkpoint, with_padded_latents
    dev = _dev()
    path = _checkpoint(tmp_path, 2)
    out_dir = os.path.join(str(tmp_path), "out")
    canvas, digits = E.main(["latent_viz", path, "--out", out_dir])
    assert canvas.shape == (560, 560) and digits.shape == (20, 20)
    assert torch.equal(torch.load(os.path.join(out_dir, "latent_viz_image.pt")), canvas)
    with open(os.path.join(out_dir, "latent_viz_text.txt")) as fp:
        assert fp.read() == E.array2d_string(digits.tolist())
    vae = load_checkpoint(path, use_cuda=True).eval()
    assert vae.n_latents == 2
    dec = with_padded_latents(vae)
    cpu = load_checkpoint(path, use_cuda=False).eval().double()
    grid = torch.linspace(-3, 3, 20)
    with torch.no_grad():
        for i, j in [(0, 0), (0, 19), (7, 12), (19, 0), (19, 19)]:
            tile = canvas[(19 - i) * 28:(20 - i) * 28, j * 28:(j + 1) * 28]      # mnist/latent_viz.py:65
            z = torch.tensor([[float(grid[j]), float(grid[i])]])
            alone = dec.decode_image(torch.cat((z, torch.zeros(1, 2)), dim=1).to(dev)).reshape(28, 28).cpu()
            want = torch.sigmoid(cpu.image_decoder.net(z.double())).reshape(28, 28)
            logits = cpu.text_decoder.net(z.double())[0]
            assert float((tile - alone).abs().max()) <= 1e-5, (i, j)
            assert float((tile.double() - want).abs().max()) <= 1e-5, (i, j)
            top = torch.topk(logits, 2).values
            if float(top[0] - top[1]) > 1e-4:                      # (a tie in float64 decides nothing)
                assert int(digits[i, j]) == int(logits.argmax())
    with pytest.raises(ValueError):
        E.latent_viz(load_checkpoint(_checkpoint(tmp_path, 20), use_cuda=True))
