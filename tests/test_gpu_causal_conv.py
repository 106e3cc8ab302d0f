"""GPU tests of ``pixelcnn.causal_conv2d`` (csrc/causal_conv.hip): forward, data gradient, weight gradient and bias gradient against
``tapconv`` in float64 on bf16-rounded operands (tests/causal_conv_ref.py).

Gate per output = 8 x max(yardstick, 2^-23 max |reference|): the yardstick is max |tapconv in float32 on the CPU - float64| on the
same rounded operands, the factor 8 the project's margin for another summation order (``pixelcnn_ref.GATE_FACTOR``), the floor half
an ulp of the stored fp32 result for the cases whose float32 CPU sum happens to be exact.  tests/test_cpu_causal_conv.py shows that
this gate sees a dropped tap, a tap shifted by a column or a row, unrounded operands, Cin and Cout exchanged in the data gradient, a
masked cell given a gradient, a bias dropped at a border and a left-out last weight-gradient chunk.

MEASURED (largest kernel error / max(yardstick, floor) per tap list over the shapes below; `pytest -s` prints every case):

largest (kernel error) / max(yardstick, 2^-23 max |reference|) over the SHAPES, per tap list and output; the gate is 8.  MI355X:
tap list                y       dx       dw       db   (shape of the largest)
A7x7                 1.00     1.35     1.46     2.52   B1-ci16-co16-300x7
B3x3                 1.00     1.13     2.19     1.73   B1-ci16-co16-300x7
one1x1               0.81     1.54     2.46     1.79   B1-ci16-co16-300x7
vertical4x7          1.00     1.17     1.89     2.63   B1-ci16-co16-300x7
vertical2x3          0.96     1.26     2.44     1.53   B1-ci16-co16-300x7
horizontal1x4        0.89     0.92     1.98     1.48   B1-ci16-co16-300x7
horizontal1x2        0.88     1.15     2.01     2.36   B1-ci16-co16-300x7
The largest ratio is 2.63; yardsticks ran from 0 (all-outside cases, exact) and 5e-8 to 2e-5.  Cells in no tap were exactly 0 in every case.
(With ONE fp32 accumulator chain over taps x Cin instead of a chain per tap the forward stood at up to 3.37 and dx at up to 5.60.)
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import causal_conv_ref as C  # noqa: E402

pytestmark = pytest.mark.gpu

TILE, CHUNK = 64, 1024                       # checked against mmvae_causal_conv_geometry in a test
KINDS = [("A", 7, 7), ("B", 3, 3), ("one", 1, 1), ("vertical", 4, 7), ("vertical", 2, 3), ("horizontal", 1, 4), ("horizontal", 1, 2)]
# (B, Cin, Cout, H, W): every Cin of {1, 3, 16, 40, 128}, Cout of {16, 32, 96, 256}, image of {1x1, 1x6, 5x1, 6x9, 9x5, 4x4} and B of
# {1, 2, 3}; then B H W = TILE - 1, TILE, TILE + 1; then 2100 positions = 2 weight-gradient chunks and a partial third (a tall
# narrow image at 16 channels).  Every shape runs with every tap list.
SHAPES = [(1, 1, 16, 1, 1), (2, 3, 32, 1, 6), (3, 16, 96, 5, 1), (1, 40, 256, 6, 9), (2, 128, 16, 9, 5), (3, 16, 32, 4, 4),
          (1, 3, 16, 7, 9), (1, 16, 16, 8, 8), (1, 16, 32, 5, 13), (1, 16, 16, 300, 7)]
CASES = [(k, s) for k in KINDS for s in SHAPES]


def _id(v):
    return "%s%dx%d" % v if isinstance(v[0], str) else "B%d-ci%d-co%d-%dx%d" % v


def _ratio(err, yard):
    return err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _run(x, w, b, g, taps, dev, need_dx=True):
    """-> {"y", "dx", "dw", "db"} on the CPU, from one forward and one backward of the op"""
    from multimodal_vae_amd.pixelcnn import causal_conv2d
    xd, wd, bd = x.to(dev).requires_grad_(need_dx), w.to(dev).requires_grad_(), b.to(dev).requires_grad_()
    y = causal_conv2d(xd, wd, bd, taps)
    assert y.shape == g.shape and y.dtype == torch.float32 and y.is_contiguous(memory_format=torch.channels_last)
    y.backward(g.to(dev))
    torch.cuda.synchronize()
    return {"y": y.detach().cpu(), "dx": None if xd.grad is None else xd.grad.cpu(), "dw": wd.grad.cpu(), "db": bd.grad.cpu()}


def test_geometry():
    from multimodal_vae_amd.pixelcnn import causal_conv_geometry, pixelcnn_geometry
    _dev()
    tile, ctile, chunk, max_taps, max_off, max_ch = causal_conv_geometry()
    assert (tile, chunk) == (TILE, CHUNK) and ctile >= 16
    assert max_taps >= 49 and max_off >= 7 and max_ch >= 2 * pixelcnn_geometry()[1]
    B, _, _, H, W = SHAPES[-1]
    assert B * H * W > 2 * CHUNK and (B * H * W) % CHUNK != 0
    assert {TILE - 1, TILE, TILE + 1} <= {s[0] * s[3] * s[4] for s in SHAPES}


@pytest.mark.parametrize("kind,shape", CASES, ids=_id)
def test_against_float64(kind, shape):
    dev = _dev()
    B, Cin, Cout, H, W = shape
    taps = C.taps_ref(*kind)
    x, w, b, g = C.operands(B, Cin, Cout, H, W, kind[1], kind[2], seed=len(taps))
    ref, yard, gates = C.reference(x, w, b, g, taps)
    got = _run(x, w, b, g, taps, dev)
    cells = {(t[0], t[1]) for t in taps}
    line = "%-16s %-24s" % (_id(kind), _id(shape))
    errs = {}
    for k in ("y", "dx", "dw", "db"):
        errs[k] = float((got[k].double() - ref[k]).abs().max())
        line += "  %s %.2e/%.2e %5.2f" % (k, errs[k], gates[k] / C.GATE_FACTOR, _ratio(errs[k], gates[k] / C.GATE_FACTOR))
    print(line)
    for k in errs:
        assert errs[k] <= gates[k], (k, errs[k], gates[k])
    for r in range(kind[1]):
        for c in range(kind[2]):
            if (r, c) not in cells:
                assert torch.equal(got["dw"][:, :, r, c], torch.zeros(Cout, Cin)), (r, c)


def test_all_outside():
    dev = _dev()
    taps = C.taps_ref("A", 7, 7)
    x, w, b, g = C.operands(2, 3, 16, 1, 1, 7, 7)
    got = _run(x, w, b, g, taps, dev)
    assert torch.equal(got["y"], b.view(1, -1, 1, 1).expand(2, 16, 1, 1))
    assert torch.equal(got["dx"], torch.zeros_like(x)) and torch.equal(got["dw"], torch.zeros_like(w))
    assert torch.equal(got["db"], g.sum(dim=(0, 2, 3)))                      # (two summands per channel: exact in any order)


@pytest.mark.parametrize("kind,shape", [(("A", 7, 7), (3, 3, 32, 6, 9)), (("vertical", 2, 3), (1, 16, 16, 300, 7)), (("B", 3, 3), (3, 40, 96, 9, 5))],
                         ids=_id)
def test_same_bits_twice(kind, shape):
    import multimodal_vae_amd.pixelcnn as P
    dev = _dev()
    B, Cin, Cout, H, W = shape
    taps = C.taps_ref(*kind)
    x, w, b, g = C.operands(B, Cin, Cout, H, W, kind[1], kind[2])
    first = _run(x, w, b, g, taps, dev)
    for ws in P._CONV_WS.values():
        ws.view(torch.float32).fill_(float("nan"))
    again = _run(x, w, b, g, taps, dev)
    for k in first:
        assert torch.equal(first[k], again[k]), k
        assert not torch.isnan(first[k]).any()


@pytest.mark.parametrize("kind", [("A", 7, 7), ("vertical", 2, 3), ("horizontal", 1, 4)], ids=_id)
def test_sample_does_not_depend_on_the_batch(kind):
    dev = _dev()
    taps = C.taps_ref(*kind)
    x, w, b, g = C.operands(3, 16, 32, 6, 9, kind[1], kind[2])
    three = _run(x, w, b, g, taps, dev)
    one = _run(x[:1].clone(), w, b, g[:1].clone(), taps, dev)
    assert torch.equal(three["y"][:1], one["y"]) and torch.equal(three["dx"][:1], one["dx"])


def test_no_grad_and_needs_input_grad():
    from multimodal_vae_amd.pixelcnn import causal_conv2d
    dev = _dev()
    taps = C.taps_ref("B", 3, 3)
    x, w, b, g = C.operands(2, 16, 32, 6, 9, 3, 3)
    got = _run(x, w, b, g, taps, dev, need_dx=False)
    assert got["dx"] is None                                                 # conv1's input is the image: no data gradient
    with torch.no_grad():
        y = causal_conv2d(x.to(dev), w.to(dev), b.to(dev), taps)
    assert not y.requires_grad and torch.equal(y.cpu(), got["y"])
    full = _run(x, w, b, g, taps, dev)
    assert full["dx"] is not None and torch.equal(full["dw"], got["dw"]) and torch.equal(full["db"], got["db"])
    # a frozen weight: only the data gradient is computed
    xd = x.to(dev).requires_grad_()
    causal_conv2d(xd, w.to(dev), b.to(dev), taps).backward(g.to(dev))
    assert torch.equal(xd.grad.cpu(), full["dx"])
    # a frozen weight with a trainable bias: the bias gradient alone (workspace filled with NaN first: no partial of dw is read)
    import multimodal_vae_amd.pixelcnn as P
    for ws in P._CONV_WS.values():
        ws.view(torch.float32).fill_(float("nan"))
    bd = b.to(dev).requires_grad_()
    causal_conv2d(x.to(dev), w.to(dev), bd, taps).backward(g.to(dev))
    assert torch.equal(bd.grad.cpu(), full["db"])


def test_argument_errors_leave_the_device_usable():
    from multimodal_vae_amd._lib import MMVAEError
    from multimodal_vae_amd.pixelcnn import causal_conv2d, causal_conv_geometry
    dev = _dev()
    taps = C.taps_ref("B", 3, 3)
    x, w, b, g = C.operands(2, 16, 32, 6, 9, 3, 3)
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    max_off = causal_conv_geometry()[4]
    for bad in (((0, 0, max_off + 1, 0),), ((0, 0, 0, -max_off - 1),), (), ((3, 0, 0, 0),), ((0, 0, 0, 0), (0, 0, -1, 0))):
        with pytest.raises(MMVAEError):
            causal_conv2d(xd, wd, bd, bad)
    with pytest.raises(MMVAEError):
        causal_conv2d(x, wd, bd, taps)                                       # a CPU tensor
    with pytest.raises(MMVAEError):
        causal_conv2d(xd, w[:, :8].contiguous().to(dev), bd, taps)           # the wrong Cin
    with pytest.raises(MMVAEError):
        causal_conv2d(xd.double(), wd, bd, taps)
    ref, _, gates = C.reference(x, w, b, g, taps)
    got = _run(x, w, b, g, taps, dev)
    assert float((got["y"].double() - ref["y"]).abs().max()) <= gates["y"]
