"""CPU tests of the description of the MNIST InfoVAE step (tests/infovae_mnist_step_ref.py, the GPU tests' reference) and of the host
side of the feature: the float64 restatement against torch autograd on the reference formulation and against what the reference's
own class computed (tests/golden/mnist_infovae_reference.npz), the GPU test's per-tensor gate against injected faults at every GPU
shape, the float32 layer against its own gate, and what needs no GPU (symbols, refusals, key sets, the driver's flag)."""
import ctypes as C_
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv4s2_ref as C  # noqa: E402
import infovae_mnist_step_ref as R  # noqa: E402


def _weights(D):
    return {k: v.float() for k, v in R.formula_weights(D).items()}


# ------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("B,D", [(3, 5), (1, 20)])
def test_restatement_is_torch_autograd(B, D):
    sd = _weights(D)
    x = C.formula_input(B)
    ts = torch.randn(B, D, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    for lx, lm in ((1.0, 1.0), R.STEP_LAMBDAS, (0.0, 1.0), (1.0, 0.0)):
        a, b = R.step(sd, x, ts, lx, lm), R.torch_step(sd, x, ts, lx, lm)
        ta, tb = R.tensors(a), R.tensors(b)
        for k in ta:
            assert float((ta[k] - tb[k]).abs().max()) < 1e-12, (k, lx, lm)
        assert float((a["sums"] - b["sums"]).abs().max()) < 1e-9 * max(1.0, float(b["sums"][0]))
        assert float(a["sums"][1:12].abs().max()) == 0.0
        if lx == 0.0:
            assert all(float(a["grads"][k].abs().max()) == 0.0 for k in R.DECODER)


def test_restatement_reproduces_the_reference(golden_dir):
    golden = np.load(os.path.join(golden_dir, "mnist_infovae_reference.npz"))
    assert [str(n) for n in golden["names"]] == list(R.NAMES)
    out = R.step(R.formula_weights(20), C.formula_input(4), torch.zeros(4, 20, dtype=torch.float64))
    for key in ("recon", "z"):
        assert out[key].shape == golden[key].shape and float((out[key] - torch.from_numpy(golden[key])).abs().max()) < 1e-12, key


def test_layout_helpers_are_inverse_permutations():
    t = torch.arange(2 * 6272, dtype=torch.float64).view(2, 6272)
    assert torch.equal(R.from_cl(R.to_cl(t)), t)
    c, p = 5, 17
    assert float(R.to_cl(t)[1, p * 128 + c]) == float(t[1, c * 49 + p])


# ------------------------------------------------------------------------------------------------------ the gates see faults
@functools.lru_cache(maxsize=None)
def _case(B, D):
    x = C.formula_input(B).float()
    ts = torch.randn(B, D, generator=torch.Generator().manual_seed(5))
    sd = _weights(D)
    return (x, ts, sd) + R.step_yardsticks(sd, x, ts, *R.STEP_LAMBDAS)


@pytest.mark.parametrize("B,D", R.STEP_SHAPES)
def test_yardsticks(B, D):
    x, ts, sd, ref, e_emu, e_f32, gates = _case(B, D)
    want = R.tensors(ref)
    for k in want:
        print("B=%d D=%d %-24s max|ref| %.3e  E_emu %.3e  E_f32 %.3e  gate %.3e" % (B, D, k, float(want[k].abs().max()), e_emu[k], e_f32[k], gates[k]))
        assert 0 < gates[k] < float(want[k].abs().max()), k          # a gate stays below what it guards


@pytest.mark.parametrize("fault", R.FAULTS)
@pytest.mark.parametrize("B,D", R.STEP_SHAPES)
def test_gate_sees_fault(B, D, fault):
    x, ts, sd, ref, e_emu, e_f32, gates = _case(B, D)
    bad = R.tensors(R.step(sd, x, ts, *R.STEP_LAMBDAS, fault=fault))
    want = R.tensors(ref)
    miss = {k: float((bad[k] - want[k]).abs().max()) / gates[k] for k in want}
    worst = max(miss, key=miss.get)
    print("B=%d D=%d %-20s misses the gate of %s by %.1f x" % (B, D, fault, worst, miss[worst]))
    assert miss[worst] >= 2.0, (fault, miss)


@pytest.mark.parametrize("kind", R.ACTS)
@pytest.mark.parametrize("shape", [s for s in R.LAYER_SHAPES if s[1] * s[2] < 1 << 20])
def test_float32_layer_passes_its_own_gate(shape, kind):
    x, w, b, g = R.lin_operands(shape)
    ref, yard, gates = R.lin_reference(x, w, b, g, kind, 0.1)
    f32 = R.lin_layer(x, w, b, g, kind, C.slope32(0.1), torch.float32, y=ref["y"].float())
    for k in ref:
        assert float((f32[k].double() - ref[k]).abs().max()) <= gates[k], k
    # and the layer gate sees a dropped bias gradient or a wrong activation backward
    bad = R.lin_layer(x, w, b, g, kind, C.slope32(0.1), torch.float64, y=ref["y"].float())
    assert float(bad["db"].abs().max()) > 2 * gates["db"]
    if kind != "none":
        wrong = R.gp(g.double(), ref["y"], kind, C.slope32(0.1), fault="relu_sign_g") @ w.double()
        assert float((wrong - ref["dx"]).abs().max()) > 2 * gates["dx"]


# ------------------------------------------------------------------------------------------------------ the host side
SYMBOLS = ("mmvae_lin_act_fwd", "mmvae_lin_act_dgrad", "mmvae_lin_act_wgrad", "mmvae_lin_act_workspace_bytes", "mmvae_mnist_infovae_create",
           "mmvae_mnist_infovae_destroy", "mmvae_mnist_infovae_num_params", "mmvae_mnist_infovae_param_info", "mmvae_mnist_infovae_param_count",
           "mmvae_mnist_infovae_bind", "mmvae_mnist_infovae_step_workspace_bytes", "mmvae_mnist_infovae_step")


def test_symbols_and_plan_table():
    from multimodal_vae_amd import _lib
    lib = _lib.load()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmvae_hip.h")).read()
    assert all(s + "(" in hdr for s in SYMBOLS)
    for D in (20, 2, 33):
        h = lib.mmvae_mnist_infovae_create(D, 8)
        assert h and lib.mmvae_mnist_infovae_num_params(h) == 12
        name, nd, off, shape = C_.create_string_buffer(128), C_.c_int(), C_.c_longlong(), (C_.c_int * 4)()
        end = 0
        for i, (want, shp) in enumerate(zip(R.NAMES, R.shapes_of(D))):
            assert lib.mmvae_mnist_infovae_param_info(h, i, name, C_.byref(nd), shape, C_.byref(off)) == 0
            assert name.value.decode() == want and tuple(shape[k] for k in range(nd.value)) == shp
            assert off.value % 4 == 0 and off.value >= end            # every tensor starts 16-byte aligned, none overlaps
            end = off.value + int(np.prod(shp))
        assert lib.mmvae_mnist_infovae_param_count(h) >= end
        assert lib.mmvae_mnist_infovae_step_workspace_bytes(h) > 0
        lib.mmvae_mnist_infovae_destroy(h)


def test_create_refuses_latent_sizes_outside_the_mmd_range():
    from multimodal_vae_amd import _lib
    lib = _lib.load()
    for D in (0, 257):
        assert not lib.mmvae_mnist_infovae_create(D, 8)
        assert "1..256" in lib.mmvae_last_error().decode()
    assert not lib.mmvae_mnist_infovae_create(20, 0)
    assert "batch" in lib.mmvae_last_error().decode()


def test_layer_workspace_query():
    from multimodal_vae_amd._lib import call
    ws = lambda *a: int(call("mmvae_lin_act_workspace_bytes", *a))
    assert ws(128, 1024, 6272, 0) > 0 and ws(128, 6272, 1024, 1) > 0
    assert ws(7, 1024, 6272, 0) * 128 == ws(128, 1024, 6272, 0) * 7          # the split is the layer's, never the batch's
    assert ws(0, 8, 8, 0) == 0 and ws(8, 0, 8, 0) == 0 and ws(8, 8, 8, 2) == 0 and ws(1 << 17, 8, 8, 0) == 0


def test_key_sets_and_checkpoints_are_interchangeable():
    import multimodal_vae_amd.mnist as M
    torch.manual_seed(3)
    a, b = M.InfoVAE(n_latents=6), M.FusedInfoVAE(n_latents=6)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) == list(R.NAMES) and all(sa[k].shape == sb[k].shape for k in sa)
    b.load_state_dict(sa, strict=True)
    a2 = M.InfoVAE(n_latents=6)
    a2.load_state_dict(b.state_dict(), strict=True)
    assert all(torch.equal(a2.state_dict()[k], sa[k]) for k in sa)
    with pytest.raises(M.MMVAEError):
        b(torch.zeros(2, 1, 28, 28))                       # device-only: no CPU fallback
    with pytest.raises(M.MMVAEError):
        M.InfoVAETrainer(a, 8)


def test_driver_refuses_fused_without_cuda():
    import multimodal_vae_amd.train_infovae_mnist as T
    a = T.build_parser().parse_args([])
    assert a.fused is False
    with pytest.raises(SystemExit) as e:
        T.resolve(T.build_parser().parse_args(["--fused"]))
    assert "--fused" in str(e.value) and "--cuda" in str(e.value)


def test_engine_takes_the_new_family_and_refuses_others():
    from multimodal_vae_amd import core
    with pytest.raises(core.MMVAEError, match="COCO has one"):
        core.FusedInfoVAEStep(type("S", (), {"API": "mnist"})(), 8)
    assert core.MnistInfoVAEState.API == "mnist_infovae"
    with pytest.raises(core.MMVAEError, match="gfx950"):
        core.MnistInfoVAEState(20, torch.device("cpu"))
