"""Host side of the MMD op and the InfoVAE surface (no GPU): the reference code of tests/mmd_ref.py checks itself against autograd
and against values recorded from the reference's own compute_mmd, every gate of tests/test_gpu_mmd.py is shown to see a missing
row tile, column tile and column split, the C boundary refuses bad sizes before it would launch anything, and the module's
state_dict and the driver's flags are the reference's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mmd_ref as R  # noqa: E402


def _geometry():
    from multimodal_vae_amd.mmd import mmd_geometry
    return mmd_geometry()


# ------------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("nx,ny,D", [(5, 7, 3), (33, 70, 21), (64, 65, 100)])
def test_float64_reference_equals_the_formulation_with_autograd(nx, ny, D):
    x, y = R.real_inputs(nx, ny, D)
    ref = R.mmd64(x, y)
    terms, dx, dy = R.formulation(x.double(), y.double())
    assert torch.allclose(ref["terms"], terms, rtol=1e-13, atol=1e-15)
    assert torch.allclose(ref["dx"], dx, rtol=1e-11, atol=1e-18) and torch.allclose(ref["dy"], dy, rtol=1e-11, atol=1e-18)
    assert torch.allclose(R.kernel64(x, y), R.formulation_kernel(x.double(), y.double()), rtol=1e-13, atol=0)
    # the expanded float64 form that the largest GPU case uses agrees with the direct one far below any fp32 gate
    exp = R.mmd64(x, y, expand=True)
    assert R.value_error(exp["terms"], ref["terms"]) < 1e-13
    assert R.grad_error(exp["dx"], ref["dx"]) < 1e-11 and R.grad_error(exp["dy"], ref["dy"]) < 1e-11


def test_blockwise_formulation_equals_the_whole_one(monkeypatch):
    x, y = R.real_inputs(40, 50, 20)
    whole = R.formulation(x, y)
    monkeypatch.setattr(R, "FORMULATION_ROWS", 1)
    monkeypatch.setattr(R, "FORMULATION_BLOCK", 50 * 20 * 7)      # 7 rows per block
    parts = R.formulation(x, y)
    assert float((whole[0] - parts[0]).abs().max()) < 5e-7
    assert float((whole[1] - parts[1]).abs().max()) <= 1e-6 * float(whole[1].abs().max())


@pytest.mark.parametrize("tag", ["a", "b"])
def test_float64_reference_equals_the_recorded_reference_values(tag, golden_dir):
    fx = np.load(os.path.join(golden_dir, "mmd_reference.npz"))
    x, y = torch.from_numpy(fx[tag + "_x"]), torch.from_numpy(fx[tag + "_y"])
    assert tuple(x.shape) + tuple(y.shape) == ((5, 3, 7, 3) if tag == "a" else (16, 20, 16, 20))
    ref = R.mmd64(x, y)
    np.testing.assert_allclose(ref["terms"].numpy(), fx[tag + "_terms"], rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(ref["dx"].numpy(), fx[tag + "_dx"], rtol=1e-11, atol=1e-18)
    np.testing.assert_allclose(ref["dy"].numpy(), fx[tag + "_dy"], rtol=1e-11, atol=1e-18)
    np.testing.assert_allclose(R.kernel64(x, y).numpy(), fx[tag + "_kernel_xy"], rtol=1e-13, atol=0)


def test_same_tensor_case_vanishes_and_has_a_scale():
    c = R.real_case(70, 70, 20, same=True)
    assert c["x"] is c["y"] and float(c["ref"]["terms"][3].abs()) < 1e-15
    assert c["scale"] > 0 and 0 < c["yardstick"]["dx"] < 1e-4 and c["yardstick"]["value"] < 1e-6


# ------------------------------------------------------------------------------------------------------ the gates see the faults
def _faults(nx, ny, rt, ct):
    """One row tile, one column tile and one column split missing, in each quarter (row class, column class)."""
    rtx, rty, tx, ty, sx, sy = R.split_rule(nx, ny, rt, ct)
    n, tiles, splits = {"x": nx, "y": ny}, {"x": tx, "y": ty}, {"x": sx, "y": sy}
    out = []
    for a in "xy":
        for c in "xy":
            last_row_tile = slice(((n[a] - 1) // rt) * rt, n[a])
            out.append(("row tile", a, last_row_tile, c, slice(0, n[c])))
            out.append(("column tile", a, slice(0, n[a]), c, slice(((n[c] - 1) // ct) * ct, n[c])))
            lo, hi = R.split_rows(tiles[c], splits[c], splits[c] - 1, ct, n[c])
            out.append(("column split", a, slice(0, n[a]), c, slice(lo, hi)))
    return out


@pytest.mark.parametrize("nx,ny,D", [(131, 65, 20), (2, 63, 100), (300, 257, 2)])
def test_every_real_valued_gate_sees_a_missing_tile(nx, ny, D):
    rt, ct, _ = _geometry()
    c = R.real_case(nx, ny, D)
    gate = {k: R.GATE_FACTOR * v for k, v in c["yardstick"].items()}
    assert 0 < gate["value"] < 5e-6 and 0 < gate["dx"] < 1e-4 and 0 < gate["dy"] < 1e-4
    for what, a, rs, cc, cs in _faults(nx, ny, rt, ct):
        bad = R.mmd64(c["x"], c["y"], fault=(a, rs, cc, cs))
        if (a, cc) != ("y", "x"):                                 # the value does not use the y-rows-by-x-columns quarter
            assert R.value_error(bad["terms"], c["ref"]["terms"]) > gate["value"], (what, a, cc)
        g = "dx" if a == "x" else "dy"
        assert R.grad_error(bad[g], c["ref"][g]) > gate[g], (what, a, cc)


def test_exact_count_cases_see_a_missing_tile():
    """The exact tests compare fp32-rounded float64 means with torch.equal: one missing pair of 16.8 million changes the sum
    by 1 of an integer below 2^25, and float64 -> fp32 rounding of sum / n^2 keeps sums apart that differ by a whole tile."""
    rt, ct, _ = _geometry()
    nx, ny = 4099, 4100
    full = np.float32(np.float64(nx) * nx / (np.float64(nx) * nx))
    for missing in (ct, rt * ct, nx):                             # one pair row of a tile, a tile, a whole row
        assert np.float32((np.float64(nx) * nx - missing) / (np.float64(nx) * nx)) != full
    assert nx * ny > 2 ** 24
    # the same means summed in fp32 are wrong: the exact test fails for an fp32 fold
    assert np.float32(2 ** 24) + np.float32(1) == np.float32(2 ** 24)


# ------------------------------------------------------------------------------------------------------ the C boundary
def test_c_boundary_refuses_without_launching():
    from multimodal_vae_amd._lib import MMVAEError, SIGNATURES, call
    rt, ct, md = _geometry()
    assert rt >= 1 and ct >= 1 and md >= 256
    assert len(SIGNATURES["mmvae_mmd"][1]) == 11 and len(SIGNATURES["mmvae_mmd_kernel_matrix"][1]) == 7
    need = call("mmvae_mmd_workspace_bytes", 128, 128, 100)
    assert need >= 8 * 256 * 101
    assert call("mmvae_mmd_workspace_bytes", 0, 5, 3) == 0 and call("mmvae_mmd_workspace_bytes", 5, 5, md + 1) == 0
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    for name, args, word in [
        ("mmvae_mmd", [None, 2, p, 2, 3, p, need, p, None, None, None], "null"),
        ("mmvae_mmd", [p, 2, None, 2, 3, p, need, p, None, None, None], "null"),
        ("mmvae_mmd", [p, 2, p, 2, 3, None, need, p, None, None, None], "null"),
        ("mmvae_mmd", [p, 2, p, 2, 3, p, need, None, None, None, None], "null"),
        ("mmvae_mmd", [p, 0, p, 2, 3, p, need, p, None, None, None], "n_x = 0"),
        ("mmvae_mmd", [p, 2, p, 0, 3, p, need, p, None, None, None], "n_y = 0"),
        ("mmvae_mmd", [p, 2, p, 65537, 3, p, need, p, None, None, None], "n_y = 65537"),
        ("mmvae_mmd", [p, 2, p, 2, 0, p, need, p, None, None, None], "dim = 0"),
        ("mmvae_mmd", [p, 2, p, 2, md + 1, p, need, p, None, None, None], "dim = %d" % (md + 1)),
        ("mmvae_mmd", [p, 128, p, 128, 100, p, need - 1, p, None, None, None], "workspace too small"),
        ("mmvae_mmd_kernel_matrix", [None, 2, p, 2, 3, p, None], "null"),
        ("mmvae_mmd_kernel_matrix", [p, 2, p, 2, 3, None, None], "null"),
        ("mmvae_mmd_kernel_matrix", [p, 0, p, 2, 3, p, None], "n_x = 0"),
        ("mmvae_mmd_kernel_matrix", [p, 2, p, 2, 0, p, None], "dim = 0"),
        ("mmvae_mmd_kernel_matrix", [p, 2, p, 2, md + 1, p, None], "dim = %d" % (md + 1)),
    ]:
        with pytest.raises(MMVAEError) as e:
            call(name, *args)
        assert word in str(e.value), (name, word, str(e.value))


def test_split_rule_of_the_header_matches_the_workspace_size():
    from multimodal_vae_amd._lib import call
    rt, ct, _ = _geometry()
    for nx, ny, D in [(128, 128, 100), (1, 1, 1), (2051, 4099, 100), (4099, 4100, 4), (10000, 10000, 100), (65536, 65536, 256)]:
        rtx, rty, tx, ty, sx, sy = R.split_rule(nx, ny, rt, ct)
        assert call("mmvae_mmd_workspace_bytes", nx, ny, D) == (sx + sy) * (rtx + rty) * rt * (1 + D) * 8, (nx, ny, D)
    assert R.split_rule(128, 128, rt, ct)[4:] == (min(128 // ct, 64), min(128 // ct, 64))
    assert R.split_rule(2051, 4099, rt, ct)[4] > 1                # "crosses several splits"


def test_python_surface_refuses_host_tensors():
    from multimodal_vae_amd import MMVAEError, mmd
    x = torch.zeros(3, 4)
    for fn in (mmd.compute_mmd, mmd.compute_kernel, mmd.mmd_terms):
        with pytest.raises(MMVAEError):
            fn(x, x)
    assert "autograd" in mmd.compute_kernel.__doc__


# ------------------------------------------------------------------------------------------------------ InfoVAE, the driver
def _bn(prefix, c):
    return [(prefix + ".weight", (c,)), (prefix + ".bias", (c,)), (prefix + ".running_mean", (c,)), (prefix + ".running_var", (c,)),
            (prefix + ".num_batches_tracked", ())]


def infovae_keys(n):
    """state_dict of coco/model.py's InfoVAE(n_latents=n): ImageEncoder under 'encoder.', ImageDecoder under 'decoder.'"""
    return ([("encoder.features.0.weight", (64, 3, 4, 4)), ("encoder.features.2.weight", (128, 64, 4, 4))] + _bn("encoder.features.3", 128)
            + [("encoder.features.5.weight", (256, 128, 4, 4))] + _bn("encoder.features.6", 256)
            + [("encoder.features.8.weight", (512, 256, 4, 4))] + _bn("encoder.features.9", 512)
            + [("encoder.classifier.0.weight", (1024, 2048)), ("encoder.classifier.0.bias", (1024,)),
               ("encoder.classifier.3.weight", (256, 1024)), ("encoder.classifier.3.bias", (256,)),
               ("encoder.classifier.6.weight", (2 * n, 256)), ("encoder.classifier.6.bias", (2 * n,)),
               ("decoder.upsample.0.weight", (2048, n)), ("decoder.upsample.0.bias", (2048,)),
               ("decoder.hallucinate.0.weight", (512, 256, 4, 4))] + _bn("decoder.hallucinate.1", 256)
            + [("decoder.hallucinate.3.weight", (256, 128, 4, 4))] + _bn("decoder.hallucinate.4", 128)
            + [("decoder.hallucinate.6.weight", (128, 64, 4, 4))] + _bn("decoder.hallucinate.7", 64)
            + [("decoder.hallucinate.9.weight", (64, 3, 4, 4))])


@pytest.mark.parametrize("n", [20, 100])
def test_infovae_state_dict_is_the_references(n):
    from multimodal_vae_amd import coco as M
    vae = M.InfoVAE() if n == 20 else M.InfoVAE(n_latents=n)
    assert vae.n_latents == n
    sd = vae.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == infovae_keys(n)
    assert len(list(vae.parameters())) == 28 and all(isinstance(p, torch.nn.Parameter) for p in vae.parameters())
    torch.optim.Adam(vae.parameters(), lr=1e-4)
    other = M.InfoVAE(n_latents=n)
    other.load_state_dict(sd, strict=True)
    assert M.compute_mmd is __import__("multimodal_vae_amd.mmd", fromlist=["x"]).compute_mmd
    assert M.compute_kernel is __import__("multimodal_vae_amd.mmd", fromlist=["x"]).compute_kernel


def test_infovae_eval_mode_returns_the_mean_and_there_is_no_cpu_path():
    from multimodal_vae_amd import coco as M, MMVAEError
    vae = M.InfoVAE().eval()
    mu = torch.randn(3, 20)
    assert vae.reparametrize(mu, torch.zeros(3, 20)) is mu
    with pytest.raises(MMVAEError):
        vae(torch.zeros(2, 3, 32, 32))


def test_train_infovae_parser_defaults_are_the_references():
    from multimodal_vae_amd import train_infovae as T
    a = T.build_parser().parse_args([])
    assert (a.n_latents, a.batch_size, a.epochs, a.lr, a.log_interval, a.cuda) == (100, 128, 10, 1e-4, 10, False)
    assert (a.data, a.synthetic, a.out, a.results, a.seed) == ('./data/coco', 0, './trained_models', '', 1234)
    with pytest.raises(SystemExit):
        T.main(["--synthetic", "8"])                               # no --cuda: refuses, there is no CPU training


def test_evaluate_has_the_latent_mmd_subcommand():
    from multimodal_vae_amd import evaluate as E
    a = E._parser().parse_args(["latent_mmd", "ckpt.pth.tar", "--synthetic", "512"])
    assert (a.cmd, a.model_path, a.synthetic, a.data, a.seed, a.json) == ("latent_mmd", "ckpt.pth.tar", 512, None, 0, None)
