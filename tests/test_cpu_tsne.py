"""Host side of the t-SNE op and of the manifold / latent_viz commands (no GPU): the reference code of tests/tsne_ref.py checks
its gradient against a finite difference of its own KL and its affinities against their defining properties, ``pca`` is checked
against numpy's SVD, every gate of tests/test_gpu_tsne.py is shown to see a dropped row tile, a dropped column tile or split
and a missed transpose half, the C boundary refuses bad arguments before it would launch anything, and the two commands parse."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsne_ref as R  # noqa: E402


def _geometry():
    from multimodal_vae_amd.tsne import tsne_geometry
    return tsne_geometry()


# ------------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("n,scale,exaggeration", [(7, 1.0, 1.0), (33, 1e-2, 1.0), (33, 3.0, 1.0)])
def test_reference_gradient_is_the_derivative_of_its_kl(n, scale, exaggeration):
    c = R.grad_case(n, scale, exaggeration)
    P, y = c["P"].astype(np.float64), c["y"].astype(np.float64)
    h = 1e-4 * scale                                               # roundoff eps KL / h and truncation h^2 both below the bound
    for i, k in [(0, 0), (n // 2, 1), (n - 1, 0)]:
        yp, ym = y.copy(), y.copy()
        yp[i, k] += h
        ym[i, k] -= h
        fd = (float(R.kl_grad(P, yp)[0]) - float(R.kl_grad(P, ym)[0])) / (2 * h)
        assert abs(fd - c["grad"][i, k]) <= 1e-6 * np.abs(c["grad"]).max() + 1e-9, (i, k, fd, c["grad"][i, k])


def test_exaggeration_scales_the_attractive_term_only():
    c1, c12 = R.grad_case(33, 10.0, 1.0), R.grad_case(33, 10.0, 12.0)
    assert c1["kl"] == c12["kl"] and c1["Z"] == c12["Z"]
    P, y = c1["P"].astype(np.float64), c1["y"].astype(np.float64)
    rep = R.kl_grad(np.zeros_like(P), y)[1]                         # -4 rep / Z alone
    np.testing.assert_allclose(c12["grad"] - rep, 12.0 * (c1["grad"] - rep), rtol=1e-11, atol=1e-15)


@pytest.mark.parametrize("n,D,perplexity", [(40, 7, 5.0), (131, 20, 30.0), (4, 2, 2.0)])
def test_reference_affinities_sum_to_one_and_meet_the_perplexity(n, D, perplexity):
    x = R.inputs(n, D)
    a = R.affinities(x, perplexity)
    P = a["P"]
    assert abs(a["sum"] - 1.0) < 1e-9 + n * n * R.P_FLOOR and np.array_equal(P, P.T) and not P.diagonal().any()
    assert np.abs(a["cond"].sum(1) - 1.0).max() < 1e-12
    assert np.abs(a["H"] - np.log(perplexity)).max() <= R.TOL
    assert R.entropy_miss(x, a["beta"], perplexity) <= R.TOL + 1e-12
    cond = a["cond"]
    H = -np.where(cond > 0, cond * np.log(np.where(cond > 0, cond, 1.0)), 0.0).sum(1)      # the entropy from its definition
    assert np.abs(H - np.log(perplexity)).max() <= R.TOL + 1e-9


def test_reference_search_exhausts_its_steps_on_identical_rows():
    a = R.affinities(np.ones((65, 3), dtype=np.float32), 5.0)
    assert np.all(a["beta"] == 2.0 ** (R.STEPS - 1))
    off = ~np.eye(65, dtype=bool)
    assert np.all(a["P"][off] == 1.0 / 4160.0)


def test_reference_run_continues_bit_for_bit():
    c = R.grad_case(33, 1e-4, 1.0)
    z, o = np.zeros_like(c["y"]), np.ones_like(c["y"])
    full = R.run(c["P"], c["y"], z, o, 0, 6, 20.0, 12.0, 4)
    a = R.run(c["P"], c["y"], z, o, 0, 3, 20.0, 12.0, 4)
    b = R.run(c["P"], a[0], a[1], a[2], 3, 3, 20.0, 12.0, 4)
    assert all(np.array_equal(u, v) for u, v in zip(full[:3], b[:3]))
    assert np.array_equal(full[3], np.concatenate((a[3], b[3])))


def test_end_to_end_conditions_hold_for_the_reference():
    """what tests/test_gpu_tsne.py asks of the op on the three blobs, asked of the reference in float64 and in fp32"""
    x, labels = R.blobs()
    for dtype in (np.float64, np.float32):
        a = R.affinities(x, 10.0, dtype)
        y0 = R.embedding(96, 1e-4)
        y, _, _, trace = R.run(a["P"], y0, np.zeros_like(y0), np.ones_like(y0), 0, 300, 20.0, 12.0, 100, dtype)
        purity, ratio = R.separation(y, labels)
        assert purity == 1.0 and ratio > 1.0 and trace[-1] < 1.0 and trace[-1] < trace[0], (purity, ratio, trace[0], trace[-1])


# ------------------------------------------------------------------------------------------------------ pca
@pytest.mark.parametrize("D,k", [(7, 2), (7, 7), (60, 50)])
def test_pca_against_numpy_svd(D, k):
    from multimodal_vae_amd.tsne import pca
    N = 40
    x = torch.from_numpy(np.random.default_rng(D).standard_normal((N, D)) * np.linspace(1.0, 3.0, D)).float()
    proj, comps, var = pca(x, k)
    assert proj.shape == (N, k) and comps.shape == (k, D) and var.shape == (k,) and proj.dtype == torch.float32
    xc = x.double().numpy() - x.double().numpy().mean(0)
    _, s, vt = np.linalg.svd(xc, full_matrices=False)
    k_ref = min(k, N - 1)                                          # centred data have rank N - 1 at most
    np.testing.assert_allclose(var.double().numpy()[:k_ref], (s ** 2 / (N - 1))[:k_ref], rtol=1e-5)
    assert np.all(np.diff(var.double().numpy()) <= 1e-7)
    for c in range(k_ref):
        v = vt[c] * np.sign(vt[c][np.abs(vt[c]).argmax()])
        np.testing.assert_allclose(comps[c].double().numpy(), v, atol=2e-5)
        assert comps[c][comps[c].abs().argmax()] > 0               # the sign rule
    np.testing.assert_allclose(proj.double().numpy()[:, :k_ref], xc @ comps.double().numpy()[:k_ref].T, atol=1e-4)
    with pytest.raises(ValueError):
        pca(x, D + 1)
    with pytest.raises(ValueError):
        pca(x[0], 1)


# ------------------------------------------------------------------------------------------------------ the gates see the faults
@pytest.mark.parametrize("n,D,perplexity", [(131, 20, 30.0), (300, 2, 5.0)])
def test_every_affinity_gate_sees_a_fault(n, D, perplexity):
    rt, ct, st, at, _ = _geometry()
    c = R.affinity_case(n, D, perplexity)
    x, ref, yard = c["x"], c["ref"], c["yardstick"]
    gate = {k: R.GATE_FACTOR * v for k, v in yard.items()}
    assert 0 < gate["p"] < 1e-3 and gate["beta"] < 1e-3
    last_sym = slice(((n - 1) // st) * st, n)
    # a symmetrisation row tile that is never written
    bad = R.affinities(x, perplexity, fault=("rows", last_sym))
    assert R.p_error(bad["P"], ref["P"]) > gate["p"] and not np.array_equal(bad["P"], bad["P"].T)
    # the columns of the last thread stride / symmetrisation tile missing from the row sums
    for cols in ([slice(((n - 1) // at) * at, n)] if n > at else []) + [last_sym]:
        bad = R.affinities(x, perplexity, drop_cols=cols)
        assert R.p_error(bad["P"], ref["P"]) > gate["p"]
        assert R.beta_error(bad["beta"], ref["beta"]) > gate["beta"]
        assert R.entropy_miss(x, bad["beta"], perplexity) > R.TOL + yard["entropy"]
    # a tile pair built without its transposed half
    bad = R.affinities(x, perplexity, fault=("transpose", slice(0, st), last_sym))
    assert R.p_error(bad["P"], ref["P"]) > gate["p"] and not np.array_equal(bad["P"], bad["P"].T)
    # the diagonal
    bad = ref["P"].copy()
    bad[n - 1, n - 1] = bad[0, 1]
    assert bad.diagonal().any()


@pytest.mark.parametrize("n", [131, 300])
@pytest.mark.parametrize("scale,exaggeration", [(1e-4, 12.0), (10.0, 1.0)])
def test_every_gradient_gate_sees_a_fault(n, scale, exaggeration):
    rt, ct, _, _, _ = _geometry()
    c = R.grad_case(n, scale, exaggeration)
    gate = {k: R.GATE_FACTOR * v for k, v in c["yardstick"].items()}
    assert 0 < gate["grad"] < 1e-4 and 0 < gate["kl"] < 1e-4
    R_, T, S = R.split_rule(n, rt, ct)
    assert S >= 2
    every = slice(0, n)
    faults = {"row tile": (slice(((n - 1) // rt) * rt, n), every),
              "column tile": (every, slice(((n - 1) // ct) * ct, n)),
              "wave's columns": (every, slice(ct // 4, ct // 2)),
              "column split": (every, slice(*R.split_cols(T, S, S - 1, ct, n)))}
    for what, drop in faults.items():
        kl, grad, _ = R.kl_grad(c["P"], c["y"], exaggeration, drop=drop)
        assert R.grad_error(grad, c["grad"]) > gate["grad"], what
        assert abs(float(kl) - c["kl"]) > gate["kl"], what


def test_exact_z_needs_a_float64_fold():
    n = 4099
    assert n * (n - 1) > 2 ** 24 and np.float32(2 ** 24) + np.float32(1) == np.float32(2 ** 24)
    assert float(np.float32(n * (n - 1))) == n * (n - 1)            # the exact count is an fp32 number: the test asks for it exactly
    rt, ct, _, _, _ = _geometry()
    for missing in (1, 8, ct // 4, ct, n - 1):                      # a pair, a group of 8, a wave's part of a tile, a tile, a row
        assert float(np.float32(n * (n - 1) - missing)) != n * (n - 1)


# ------------------------------------------------------------------------------------------------------ the C boundary
def test_split_rule_of_the_header_matches_the_workspace_size():
    from multimodal_vae_amd._lib import call
    rt, ct, st, at, md = _geometry()
    assert (rt, ct, st, at) == (64, 128, 32, 256) and md >= 256
    cd = lambda a, b: (a + b - 1) // b
    for n in (3, 4, 64, 65, 131, 1031, 4099, 10000, 32768):
        r, t, s = R.split_rule(n, rt, ct)
        sweep = s * r * rt * 4 + s * r * 3 + 4
        assert call("mmvae_tsne_workspace_bytes", n) == 8 * max(sweep, 2 * cd(n, st) ** 2), n
    assert R.split_rule(1031, rt, ct)[2] >= 2 and R.split_rule(131, rt, ct)[2] == 2 and R.split_rule(127, rt, ct)[2] == 1
    for n in (-1, 0, 2, 32769):
        assert call("mmvae_tsne_workspace_bytes", n) == 0


def test_c_boundary_refuses_without_launching():
    from multimodal_vae_amd._lib import MMVAEError, SIGNATURES, call
    assert [len(SIGNATURES["mmvae_tsne_" + k][1]) for k in ("affinities", "grad", "run")] == [10, 9, 14]
    need = call("mmvae_tsne_workspace_bytes", 100)
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    aff = lambda **kw: [kw.get("x", p), kw.get("n", 100), kw.get("dim", 20), kw.get("perp", 30.0), kw.get("P", p), kw.get("beta", p),
                        kw.get("out", p), kw.get("ws", p), kw.get("ws_bytes", need), None]
    grad = lambda **kw: [kw.get("P", p), kw.get("ex", 1.0), kw.get("y", p), kw.get("n", 100), kw.get("ws", p), kw.get("ws_bytes", need),
                         kw.get("grad", p), kw.get("out", p), None]
    run = lambda **kw: [kw.get("P", p), kw.get("n", 100), kw.get("y", p), kw.get("update", p), kw.get("gains", p), kw.get("first", 0),
                        kw.get("n_iter", 10), kw.get("lr", 200.0), kw.get("ee", 12.0), 250, kw.get("trace", p), kw.get("ws", p),
                        kw.get("ws_bytes", need), None]
    for name, args, word in [
        ("affinities", aff(x=None), "null"), ("affinities", aff(P=None), "null"), ("affinities", aff(beta=None), "null"),
        ("affinities", aff(out=None), "null"), ("affinities", aff(ws=None), "null"),
        ("affinities", aff(n=2), "n = 2"), ("affinities", aff(n=32769), "n = 32769"),
        ("affinities", aff(dim=0), "dim = 0"), ("affinities", aff(dim=257), "dim = 257"),
        ("affinities", aff(perp=0.5), "perplexity"), ("affinities", aff(perp=99.0), "perplexity"),
        ("affinities", aff(perp=float("nan")), "perplexity"), ("affinities", aff(ws_bytes=need - 1), "workspace too small"),
        ("grad", grad(P=None), "null"), ("grad", grad(y=None), "null"), ("grad", grad(grad=None), "null"), ("grad", grad(out=None), "null"),
        ("grad", grad(ws=None), "null"), ("grad", grad(n=2), "n = 2"), ("grad", grad(ex=0.0), "exaggeration"),
        ("grad", grad(ex=float("inf")), "exaggeration"), ("grad", grad(ws_bytes=need - 1), "workspace too small"),
        ("run", run(P=None), "null"), ("run", run(y=None), "null"), ("run", run(update=None), "null"), ("run", run(gains=None), "null"),
        ("run", run(trace=None), "null"), ("run", run(ws=None), "null"), ("run", run(n=32769), "n = 32769"),
        ("run", run(first=-1), "first_iter = -1"), ("run", run(n_iter=0), "n_iter = 0"), ("run", run(lr=0.0), "learning_rate"),
        ("run", run(ee=float("nan")), "early_exaggeration"), ("run", run(ws_bytes=need - 1), "workspace too small"),
    ]:
        with pytest.raises(MMVAEError) as e:
            call("mmvae_tsne_" + name, *args)
        assert word in str(e.value), (name, word, str(e.value))


def test_python_surface_refuses_host_tensors():
    from multimodal_vae_amd import MMVAEError, tsne
    x = torch.zeros(8, 4)
    with pytest.raises(MMVAEError, match="no CPU fallback"):
        tsne.joint_probabilities(x, 2.0)
    with pytest.raises(MMVAEError, match="no CPU fallback"):
        tsne.kl_grad(torch.zeros(8, 8), torch.zeros(8, 2))
    with pytest.raises(MMVAEError, match="no CPU fallback"):
        tsne.tsne(x, perplexity=2.0)
    y0 = tsne.initial_embedding(10, seed=3)
    assert y0.shape == (10, 2) and torch.equal(y0, tsne.initial_embedding(10, seed=3)) and 1e-5 < float(y0.std()) < 1e-3


# ------------------------------------------------------------------------------------------------------ the commands
def test_evaluate_has_the_manifold_and_latent_viz_subcommands():
    from multimodal_vae_amd import evaluate as E
    a = E._parser().parse_args(["manifold", "ckpt.pth.tar", "--synthetic", "256", "--n_iter", "20"])
    assert (a.cmd, a.model_path, a.pca_only, a.perplexity, a.n_iter, a.data, a.synthetic, a.seed, a.out) == (
        "manifold", "ckpt.pth.tar", False, 40.0, 20, None, 256, 0, "./results")
    a = E._parser().parse_args(["manifold", "ckpt.pth.tar", "--pca_only", "--data", "test.pt", "--perplexity", "30", "--seed", "2"])
    assert (a.pca_only, a.perplexity, a.n_iter, a.data, a.synthetic, a.seed) == (True, 30.0, 300, "test.pt", 0, 2)
    with pytest.raises(SystemExit):
        E._parser().parse_args(["manifold", "ckpt.pth.tar", "--data", "x.pt", "--synthetic", "4"])
    a = E._parser().parse_args(["latent_viz", "ckpt.pth.tar", "--out", "somewhere"])
    assert (a.cmd, a.model_path, a.out) == ("latent_viz", "ckpt.pth.tar", "somewhere")
    assert E.array2d_string([[1, 2], [3, 10]]) == "   1   2\n   3  10"


def test_padded_latents_compute_the_small_models_functions():
    """latent_viz decodes a 2-latent model on the 4-latent HIP plan: the padded model's layers, as torch ops, are the small model's"""
    from multimodal_vae_amd.mnist import MultimodalVAE, plan_latents, with_padded_latents
    assert [plan_latents(n) for n in (1, 2, 4, 5, 20, 21)] == [4, 4, 4, 8, 20, 24]
    torch.manual_seed(0)
    small = MultimodalVAE(n_latents=2).eval()
    for m in small.modules():                                      # running statistics other than (0, 1)
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.normal_()
            m.running_var.uniform_(0.5, 2.0)
    big = with_padded_latents(small)
    assert big.n_latents == 4 and not big.training and big is not small
    assert list(big.state_dict()) == list(small.state_dict())
    with torch.no_grad():
        z = torch.randn(7, 2)
        zp = torch.cat((z, torch.zeros(7, 2)), dim=1)
        assert torch.equal(small.image_decoder.net(z), big.image_decoder.net(zp))
        assert torch.equal(small.text_decoder.net(z), big.text_decoder.net(zp))
        x, t = torch.rand(7, 784), torch.arange(7)
        for enc, inp in (("image_encoder", x), ("text_encoder", t)):
            o, ob = getattr(small, enc).net(inp), getattr(big, enc).net(inp)
            assert torch.equal(o[:, :2], ob[:, :2]) and torch.equal(o[:, 2:], ob[:, 4:6])          # mu, logvar
            assert not ob[:, 2:4].any() and not ob[:, 6:].any()                                        # the extra latents: mu = logvar = 0
    same = MultimodalVAE(n_latents=20)
    assert with_padded_latents(same) is same


def test_latent_viz_refuses_other_latent_sizes():
    from multimodal_vae_amd import evaluate as E
    from multimodal_vae_amd.mnist import MultimodalVAE
    with pytest.raises(ValueError, match="n_latents = 20"):
        E.latent_viz(MultimodalVAE(n_latents=20))
