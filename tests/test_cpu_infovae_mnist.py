"""CPU tests of the MNIST InfoVAE and of the description of its convolution op: ``mnist.InfoVAE`` against what the reference's own
class computed (tests/golden/mnist_infovae_reference.npz), ``conv4s2_ref`` (the GPU tests' reference) against torch in float64, the
op-level gate against injected faults at the GPU tests' shapes, and the host-side surface (workspace query, errors, loss, checkpoint,
parser, ``latent_mmd``)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv4s2_ref as C  # noqa: E402

SHAPES = C.SHAPES + [C.chunk_shape(), C.chunk_shape(cs=1)]
SLOPE = 0.2


def _id(v):
    return v if isinstance(v, str) else "B%d-cs%d-cl%d-%dx%d" % v


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "mnist_infovae_reference.npz"))


# ------------------------------------------------------------------------------------------------------ the model
def test_state_dict_is_the_references(golden):
    import multimodal_vae_amd.mnist as M
    sd = M.InfoVAE().state_dict()
    assert list(sd) == [str(n) for n in golden["names"]]
    for v, shp in zip(sd.values(), golden["shapes"]):
        assert list(v.shape) == [int(d) for d in shp[:v.dim()]] and not shp[v.dim():].any()
    assert len(sd) == 12 and M.InfoVAE(n_latents=7).state_dict()["encoder_fc.2.weight"].shape == (7, 1024)


def test_torch_backend_reproduces_the_reference(golden):
    import multimodal_vae_amd.mnist as M
    vae = M.InfoVAE(n_latents=20).double().eval()
    sd = vae.state_dict()
    vae.load_state_dict(C.formula_state_dict(list(sd), [tuple(v.shape) for v in sd.values()]))
    x = C.formula_input(4)
    with torch.no_grad():
        recon, z = vae(x)
        enc = vae.encoder_conv(x[:2].clone())
        dec = vae.decoder_conv(C.formula_latent_grid(4))
        assert torch.equal(vae.decode(vae.encode(x)), recon)
    assert recon.shape == (4, 1, 28, 28) and z.shape == (4, 20)
    for got, key in ((recon, "recon"), (z, "z"), (enc, "encoder_conv"), (dec, "decoder_conv")):
        assert got.shape == golden[key].shape and float((got - torch.from_numpy(golden[key])).abs().max()) < 1e-12, key
    assert 0.05 < float(recon.min()) and float(recon.max()) < 0.95            # (not saturated: the comparison means something)
    # the functional form the GPU test differentiates is the same model
    r2, z2 = C.infovae_forward(vae.state_dict(), x)
    assert float((r2 - recon).abs().max()) < 1e-12 and float((z2 - z).abs().max()) < 1e-12


def test_backend_switch_on_the_cpu():
    import multimodal_vae_amd.mnist as M
    from multimodal_vae_amd._lib import MMVAEError
    from multimodal_vae_amd.conv4s2 import down4s2, up4s2
    torch.manual_seed(2)
    vae = M.InfoVAE(n_latents=4)
    keys = list(vae.state_dict())
    x = torch.rand(2, 1, 28, 28)
    want = vae(x)[0]
    assert vae.conv_backend == "torch" and M.set_infovae_backend(vae, "hip") is vae and list(vae.state_dict()) == keys
    with pytest.raises(MMVAEError):
        vae(x)                                             # selecting is fine on the CPU, running is not: there is no CPU fallback
    with pytest.raises(MMVAEError):
        vae.decode(torch.zeros(2, 4))
    M.set_infovae_backend(vae, "torch")
    assert torch.equal(vae(x)[0], want)
    with pytest.raises(MMVAEError):
        M.set_infovae_backend(vae, "triton")
    with pytest.raises(MMVAEError):
        M.set_infovae_backend(torch.nn.Linear(2, 2), "hip")
    with pytest.raises(MMVAEError):
        down4s2(torch.zeros(1, 3, 4, 4), torch.zeros(5, 3, 4, 4))
    with pytest.raises(MMVAEError):
        up4s2(torch.zeros(1, 5, 2, 2), torch.zeros(5, 3, 4, 4))


def test_workspace_query_refuses_each_broken_limit():
    from multimodal_vae_amd.conv4s2 import conv4s2_workspace_bytes as ws
    assert ws(2, 3, 5, 4, 10) > 0 and ws(1, 1, 1, 2, 2) > 0 and ws(1, 128, 128, 64, 64) > 0
    for bad in ((2, 3, 5, 5, 10), (2, 3, 5, 4, 9), (2, 3, 5, 66, 10), (2, 3, 5, 4, 66), (2, 0, 5, 4, 10), (2, 3, 0, 4, 10),
                (2, 129, 5, 4, 10), (2, 3, 129, 4, 10), (0, 3, 5, 4, 10), (2, 3, 5, 0, 10)):
        assert ws(*bad) == 0, bad


def test_infovae_loss_is_the_reference_formulation():
    import multimodal_vae_amd.mnist as M

    def compute_kernel(x, y):                              # mnist/train_infovae.py:59-68
        x_size, y_size, dim = x.size(0), y.size(0), x.size(1)
        tiled_x = x.unsqueeze(1).expand(x_size, y_size, dim)
        tiled_y = y.unsqueeze(0).expand(x_size, y_size, dim)
        return torch.exp(-torch.mean(torch.pow(tiled_x - tiled_y, 2), dim=2) / float(dim))

    def compute_mmd(x, y):
        return torch.mean(compute_kernel(x, x)) + torch.mean(compute_kernel(y, y)) - 2 * torch.mean(compute_kernel(x, y))

    g = torch.Generator().manual_seed(8)
    recon, x = torch.rand(6, 1, 28, 28, generator=g, dtype=torch.float64), torch.rand(6, 1, 28, 28, generator=g, dtype=torch.float64)
    z = torch.randn(6, 5, generator=g, dtype=torch.float64).requires_grad_()
    ts = torch.randn(6, 5, generator=g, dtype=torch.float64)
    got = M.infovae_loss(recon, x, z, ts)
    want = torch.mean(torch.pow(recon - x, 2)) + compute_mmd(ts, z)
    assert abs(float(got.detach()) - float(want.detach())) < 1e-14
    (gz,) = torch.autograd.grad(got, z)
    (wz,) = torch.autograd.grad(want, z)
    assert float((gz - wz).abs().max()) < 1e-14
    torch.manual_seed(1)
    drawn = M.infovae_loss(recon, x, z.detach())           # true_samples drawn on z's device, in z's shape and dtype
    torch.manual_seed(1)
    assert float(drawn) == float(M.infovae_loss(recon, x, z.detach(), torch.randn(6, 5, dtype=torch.float64)))


def test_checkpoint_round_trip(tmp_path):
    import multimodal_vae_amd.mnist as M
    from multimodal_vae_amd.train import save_checkpoint
    torch.manual_seed(4)
    vae = M.set_infovae_backend(M.InfoVAE(n_latents=6), "hip")
    save_checkpoint({"state_dict": vae.state_dict(), "best_loss": 1.0, "n_latents": 6, "optimizer": {}}, True, folder=str(tmp_path))
    loaded = M.load_infovae_checkpoint(os.path.join(str(tmp_path), "model_best.pth.tar"))
    assert loaded.n_latents == 6 and loaded.conv_backend == "torch"          # the default: runs on the CPU
    x = torch.rand(2, 1, 28, 28)
    with torch.no_grad():
        assert torch.equal(loaded(x)[0], M.set_infovae_backend(vae, "torch")(x)[0])


def test_trainer_parser_defaults_are_the_references():
    import multimodal_vae_amd.train_infovae_mnist as T
    a = T.build_parser().parse_args([])
    assert (a.n_latents, a.batch_size, a.epochs, a.lr, a.log_interval, a.cuda) == (20, 128, 20, 1e-3, 10, False)
    assert a.conv_backend == "torch" and a.synthetic == 0
    with pytest.raises(SystemExit) as e:
        T.resolve(T.build_parser().parse_args(["--conv_backend", "hip"]))
    assert "--cuda" in str(e.value)


def test_train_step_on_the_cpu():
    import multimodal_vae_amd.mnist as M
    import multimodal_vae_amd.train_infovae_mnist as T
    torch.manual_seed(5)
    vae = M.InfoVAE(n_latents=3)
    opt = torch.optim.Adam(vae.parameters(), lr=1e-3)
    x = torch.rand(4, 1, 28, 28)
    before = vae.encoder_conv[0].weight.detach().clone()
    loss = T.train_step(vae, opt, x)
    assert loss.dim() == 0 and torch.isfinite(loss) and not torch.equal(vae.encoder_conv[0].weight, before)


def test_latent_mmd_takes_z_from_a_tensor_encoder():
    import multimodal_vae_amd.evaluate as E
    import multimodal_vae_amd.mnist as M
    torch.manual_seed(6)
    vae = M.InfoVAE(n_latents=3)
    x = torch.rand(5, 1, 28, 28)
    out = E.latent_mmd(vae, [x[:3], (x[3:], None)], seed=1)
    assert set(out) == {"n", "k_prior", "k_posterior", "k_cross", "mmd"} and out["n"] == 5          # all five rows, not the first
    # (the terms are float32 means in (0, 1]: two float32 additions of values below 2, each within 2^-24 of it)
    assert abs(out["mmd"] - (out["k_prior"] + out["k_posterior"] - 2 * out["k_cross"])) <= 4 * 2.0 ** -24
    args = E._parser().parse_args(["latent_mmd", "x.pth.tar"])
    assert args.dataset == "coco"                          # the default is unchanged
    assert E._parser().parse_args(["latent_mmd", "x.pth.tar", "--dataset", "mnist"]).dataset == "mnist"


# ------------------------------------------------------------------------------------------------------ the reference is torch's
@pytest.mark.parametrize("act", C.ACTS)
@pytest.mark.parametrize("shape", [(2, 3, 5, 4, 10), (1, 1, 1, 2, 2), (3, 8, 4, 6, 2)], ids=_id)
def test_reference_is_torch(shape, act):
    B, Cs, Cl, Hs, Ws = shape
    g = torch.Generator().manual_seed(9)
    w = torch.randn(Cl, Cs, 4, 4, generator=g, dtype=torch.float64)

    def torch_act(pre):
        return {"none": pre, "relu": torch.relu(pre), "leaky": F.leaky_relu(pre, C.slope32(SLOPE)), "sigmoid": torch.sigmoid(pre)}[act]

    for direction in ("down", "up"):
        xs = (B, Cs, Hs, Ws) if direction == "down" else (B, Cl, Hs // 2, Ws // 2)
        x = torch.randn(xs, generator=g, dtype=torch.float64).requires_grad_()
        wl = w.clone().requires_grad_()
        conv = F.conv2d if direction == "down" else F.conv_transpose2d
        want = torch_act(conv(x, wl, stride=2, padding=1))
        up = torch.randn(want.shape, generator=g, dtype=torch.float64)
        wx, ww = torch.autograd.grad(want, (x, wl), up)
        fwd, bwd = (C.down, C.up) if direction == "down" else (C.up, C.down)
        y = C.act(fwd(x.detach(), w), act, C.slope32(SLOPE))
        assert y.shape == want.shape and float((y - want.detach()).abs().max()) < 1e-12
        # the backward written out, from the saved output, in float64 (gp itself is float32 by contract: checked below)
        if act == "sigmoid":
            gpre = (up * y) * (1.0 - y)
        elif act == "none":
            gpre = up
        else:
            gpre = torch.where(y > 0, up, (C.slope32(SLOPE) if act == "leaky" else 0.0) * up)
        assert float((bwd(gpre, w) - wx).abs().max()) < 1e-12
        dw = C.dw(gpre, x.detach()) if direction == "down" else C.dw(x.detach(), gpre)
        assert float((dw - ww).abs().max()) < 1e-12
        assert float((C.gp(up, y, act, SLOPE).double() - gpre).abs().max()) <= 2.0 ** -21 * float(up.abs().max())        # three roundings of 2^-24 on |.| <= |g|
        # and the emulated convolutions of the whole-model test have these gradients on rounded operands
        xq = C.round_bf16(x.detach()).requires_grad_()
        wq = C.round_bf16(w).requires_grad_()
        q = (C.qdown if direction == "down" else C.qup)(xq, wq, act, SLOPE)
        t = torch_act(conv(xq, wq, stride=2, padding=1))
        assert float((q - t).detach().abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------------ the gate sees faults
@functools.lru_cache(maxsize=None)
def _case(direction, shape):
    x, w, g = C.operands(direction, shape, seed=1)
    return (x, w, g) + C.reference(direction, x, w, g, "leaky", SLOPE)


def _visible(fault, shape):
    if fault == "transpose_up":
        return shape[1] > 1 and shape[2] > 1               # a (Cl, 1) or (1, Cs) matrix is its own transpose in memory
    return True


@pytest.mark.parametrize("fault,shape", [(f, s) for f in C.FAULTS for s in SHAPES if _visible(f, s)], ids=_id)
def test_gate_sees_fault(fault, shape):
    broken = {}
    for direction in ("down", "up"):
        x, w, g, ref, yard, gates = _case(direction, shape)
        saved = ref["y"].float()
        bad = C.all_(direction, x, w, g, "leaky", SLOPE, torch.float64, fault=fault, y=None if fault == "no_slope" else saved)
        for k in ref:
            broken[direction + "." + k] = float((bad[k] - ref[k]).abs().max()) / gates[k]
    assert max(broken.values()) > 10, (fault, broken)
    where = {"parity": ("up.y", "down.dx"), "transpose_up": ("up.y", "down.dx"), "last_chunk": ("down.dw", "up.dw"),
             "drop_cell": ("down.y", "up.y", "down.dx", "up.dx", "down.dw", "up.dw"), "no_round": ("down.y", "up.y")}.get(fault, ())
    for k in where:
        assert broken[k] > 1, (fault, k, broken)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_float32_passes_its_own_gate(shape):
    for direction in ("down", "up"):
        x, w, g, ref, yard, gates = _case(direction, shape)
        f32 = C.all_(direction, x, w, g, "leaky", SLOPE, torch.float32, y=ref["y"].float())
        for k in ref:
            assert float((f32[k].double() - ref[k]).abs().max()) <= gates[k], (direction, k)
