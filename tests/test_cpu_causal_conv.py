"""CPU tests of the causal tap-list convolution's description: ``taps_of`` against an independent tap list, ``tapconv`` (the GPU
tests' reference) against the torch modules in float64, the op-level gate against injected faults, and ``set_conv_backend``."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import causal_conv_ref as C  # noqa: E402

import multimodal_vae_amd.pixelcnn as P  # noqa: E402
from multimodal_vae_amd._lib import MMVAEError  # noqa: E402

IMAGES = [(1, 1), (1, 6), (5, 1), (6, 9)]


def _modules(cin=3, hid=4):
    """(id, module, kind, kh, kw): every convolution form of both models"""
    g7, g3 = P.GatedResidualBlock("A", cin, hid, 7), P.GatedResidualBlock("B", hid, hid, 3)
    return [("maskA7", P.MaskedConv2d("A", cin, hid, 7, 1, 3), "A", 7, 7), ("maskB3", P.MaskedConv2d("B", hid, hid, 3, 1, 1), "B", 3, 3),
            ("vert4x7", g7.vertical_conv, "vertical", 4, 7), ("vert2x3", g3.vertical_conv, "vertical", 2, 3),
            ("hor1x4", g7.horizontal_conv, "horizontal", 1, 4), ("hor1x2", g3.horizontal_conv, "horizontal", 1, 2),
            ("maskB1", P.MaskedConv2d("B", hid, hid, 1), "one", 1, 1), ("plain1", g3.vertical_gate_conv, "one", 1, 1)]


def test_mask_counts():
    assert len(C.taps_ref("A", 7, 7)) == 24 and len(C.taps_ref("B", 3, 3)) == 5 and len(C.taps_ref("B", 1, 1)) == 1


@pytest.mark.parametrize("gated", [False, True])
def test_taps_of_every_module(gated):
    model = (P.GatedPixelCNN if gated else P.PixelCNN)(n_blocks=2, data_channels=3, hid_dims=16, out_dims=8)
    seen = 0
    for name, m in model.named_modules():
        if not isinstance(m, torch.nn.Conv2d):
            continue
        kh, kw = m.kernel_size
        if isinstance(m, P.MaskedConv2d):
            kind = m.mask_type if min(kh, kw) > 1 else "one"
        elif isinstance(m, P.CroppedConv2d):
            kind = "vertical" if "vertical" in name else "horizontal"
        else:
            kind = "one"
        assert P.taps_of(m) == C.taps_ref(kind, kh, kw), name
        seen += 1
    assert seen == (2 + 6 * 3 if gated else 2 + 3)


def test_taps_of_refuses_other_modules():
    with pytest.raises(MMVAEError):
        P.taps_of(torch.nn.Conv2d(4, 4, 3, padding=1))
    with pytest.raises(MMVAEError):
        P.taps_of(torch.nn.Linear(4, 4))


@pytest.mark.parametrize("mod", _modules(), ids=lambda m: m[0])
@pytest.mark.parametrize("image", IMAGES, ids=lambda s: "%dx%d" % s)
def test_tapconv_is_the_module(mod, image):
    _, m, _, _, _ = mod
    torch.manual_seed(5)
    m = m.double()
    x = torch.randn(2, m.in_channels, *image, dtype=torch.float64, requires_grad=True)
    want = m(x)
    g = torch.randn_like(want)
    wx, ww, wb = torch.autograd.grad(want, (x, m.weight, m.bias), g)
    taps = P.taps_of(m)
    w = m.weight.detach().clone().requires_grad_()
    x2 = x.detach().clone().requires_grad_()
    b = m.bias.detach().clone().requires_grad_()
    got = C.tapconv(x2, w, b, taps)
    assert got.shape == want.shape and float((got - want).detach().abs().max()) < 1e-12
    gx, gw, gb = torch.autograd.grad(got, (x2, w, b), g)
    if isinstance(m, P.MaskedConv2d):
        ww = ww * m.mask                                   # torch hands masked cells a gradient; the op (and tapconv) 0
    for a, b_ in ((gx, wx), (gw, ww), (gb, wb)):
        assert float((a - b_).abs().max()) < 1e-12
    # the gradients written out (what the GPU tests compare against) are autograd's
    assert float((C.tapconv_dx(g, w.detach(), taps) - gx).abs().max()) < 1e-12
    assert float((C.tapconv_dw(g, x.detach(), w.shape, taps) - gw).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------------ the gate sees faults
CHUNK = 16                                   # a stand-in for the weight-gradient chunk: 6 x 9 x 2 positions are 6.75 of them
KIND_SHAPES = [("A", 7, 7), ("B", 3, 3), ("vertical", 4, 7), ("vertical", 2, 3), ("horizontal", 1, 4), ("horizontal", 1, 2), ("one", 1, 1)]


def _visible(fault, kind):
    if fault == "masked_grad":
        return kind in ("A", "B")                          # the others have no cell outside their taps
    if fault == "border_bias":
        return kind != "one"                               # a 1 x 1 tap never leaves the image
    return True


@pytest.mark.parametrize("image", [(6, 9), (9, 5)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("fault,ks", [(f, k) for f in C.FAULTS for k in KIND_SHAPES if _visible(f, k[0])],
                         ids=lambda v: v if isinstance(v, str) else "%s%dx%d" % v)
def test_gate_sees_fault(fault, ks, image):
    kind, kh, kw = ks
    taps = C.taps_ref(kind, kh, kw)
    x, w, b, g = C.operands(2, 8, 8, image[0], image[1], kh, kw)
    ref, yard, gates = C.reference(x, w, b, g, taps)
    bad = C.all_four(x, w, b, g, taps, torch.float64, fault=fault, chunk=CHUNK)
    ratio = {k: float((bad[k] - ref[k]).abs().max()) / gates[k] for k in ref}
    where = {"drop_tap": ("y", "dx", "dw"), "col_off": ("y", "dx", "dw"), "row_off": ("y", "dx", "dw"), "no_round": ("y", "dx", "dw"),
             "swap_dgrad": ("dx",), "masked_grad": ("dw",), "border_bias": ("y",), "last_chunk": ("dw",)}[fault]
    if len(taps) == 1 and fault == "drop_tap":
        where = ("y", "dx", "dw")
    for k in where:
        assert ratio[k] > 10, (fault, k, ratio)
    # and the fault-free float32 computation passes its own gate
    f32 = C.all_four(x, w, b, g, taps, torch.float32)
    for k in ref:
        assert float((f32[k].double() - ref[k]).abs().max()) <= gates[k]


def test_one_column_image_cannot_see_a_left_tap():
    taps = C.taps_ref("horizontal", 1, 2)
    x, w, b, g = C.operands(2, 8, 8, 5, 1, 1, 2)
    a = C.all_four(x, w, b, g, taps, torch.float64)
    d = C.all_four(x, w, b, g, taps, torch.float64, fault="drop_tap")
    assert torch.equal(a["y"], d["y"])                     # hence visibility is asserted on 6 x 9 and 9 x 5


# ------------------------------------------------------------------------------------------------------ set_conv_backend
@pytest.mark.parametrize("gated", [False, True])
def test_set_conv_backend_on_the_cpu(gated):
    torch.manual_seed(3)
    model = (P.GatedPixelCNN if gated else P.PixelCNN)(n_blocks=1, data_channels=3, hid_dims=16, out_dims=8)
    x = torch.rand(2, 3, 5, 4)
    keys = list(model.state_dict())
    want = model(x)
    assert P.set_conv_backend(model, "torch") is model
    assert list(model.state_dict()) == keys and torch.equal(model(x), want)
    P.set_conv_backend(model, "hip")                       # selecting is fine on the CPU ...
    assert list(model.state_dict()) == keys
    with pytest.raises(MMVAEError):
        model(x)                                           # ... running is not: there is no CPU fallback
    P.set_conv_backend(model, "torch")
    assert torch.equal(model(x), want)
    with pytest.raises(MMVAEError):
        P.set_conv_backend(model, "triton")
    with pytest.raises(MMVAEError, match="set_conv_backend"):
        P.set_conv_backend(torch.nn.Linear(2, 2), "hip")


def test_train_script_refuses_hip_without_cuda():
    import multimodal_vae_amd.train_pixelcnn as T
    args = T.build_parser().parse_args(["--conv_backend", "hip"])
    with pytest.raises(SystemExit) as e:
        T.resolve(args)
    assert "--cuda" in str(e.value)
    assert T.resolve(T.build_parser().parse_args([])).conv_backend == "torch"


def test_checkpoint_records_the_backend_and_loading_ignores_it(tmp_path):
    torch.manual_seed(4)
    model = P.set_conv_backend(P.GatedPixelCNN(n_blocks=1, data_channels=1, hid_dims=16, out_dims=8), "hip")
    P.save_checkpoint({"state_dict": model.state_dict(), "gated": True, "n_blocks": 1, "data_channels": 1, "hid_dims": 16, "out_dims": 8,
                       "height": 8, "width": 8, "conv_backend": "hip"}, False, folder=str(tmp_path))
    ckpt = torch.load(os.path.join(str(tmp_path), "checkpoint.pth.tar"), weights_only=False)
    assert ckpt["conv_backend"] == "hip"
    loaded = P.load_checkpoint(os.path.join(str(tmp_path), "checkpoint.pth.tar"))
    assert all(getattr(m, "conv_backend", "torch") == "torch" for m in loaded.modules())       # the default: runs on the CPU
    assert list(loaded.state_dict()) == list(model.state_dict())
    x = torch.rand(1, 1, 8, 8)
    assert torch.equal(loaded(x), P.set_conv_backend(model, "torch")(x))
