"""GPU tests of ``conv4s2.down4s2`` / ``up4s2`` (csrc/conv4s2.hip): forward, data gradient and weight gradient of both directions
under all four activations against the products written out in float64 on bf16-rounded operands (tests/conv4s2_ref.py).

Gate per output = 8 x max(yardstick, 2^-23 max |reference|): the yardstick is max |the same computation in float32 on the CPU -
float64| on the same rounded operands, the factor 8 the project's margin for another summation order (``pixelcnn_ref.GATE_FACTOR``),
the floor half an ulp of the stored fp32 result.  The reference's backward is given the op's own output y: the mask of relu / leaky
and the sigmoid factor come from the saved output, so no rounding-boundary flip can enter.  tests/test_cpu_infovae_mnist.py shows
that this gate sees every fault of ``conv4s2_ref.FAULTS`` at these shapes.

`pytest -s` prints error / max(yardstick, floor) per case; MEASURED figures are in profiles/infovae_mnist_bench.txt.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv4s2_ref as C  # noqa: E402

pytestmark = pytest.mark.gpu

SLOPE = 0.2                                   # not the default: a slope that is ignored shows
# the last two: B * Hs/2 * Ws/2 one more than a weight-gradient chunk (test_geometry), on the matrix and on the one-channel path
SHAPES = C.SHAPES + [C.chunk_shape(), C.chunk_shape(cs=1)]
CASES = [(d, a, s) for d in ("down", "up") for a in C.ACTS for s in SHAPES]


def _id(v):
    return v if isinstance(v, str) else "B%d-cs%d-cl%d-%dx%d" % v


def _ratio(err, yard):
    return err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _op(direction):
    from multimodal_vae_amd.conv4s2 import down4s2, up4s2
    return down4s2 if direction == "down" else up4s2


def _run(direction, x, w, g, act, dev, need_dx=True, need_dw=True, prepare=lambda t: t):
    """-> {"y", "dx", "dw"} on the CPU, from one forward and one backward of the op"""
    xd, wd = prepare(x.to(dev)).requires_grad_(need_dx), w.to(dev).requires_grad_(need_dw)
    y = _op(direction)(xd, wd, act, SLOPE)
    assert y.shape == g.shape and y.dtype == torch.float32 and y.is_contiguous(memory_format=torch.channels_last)
    if need_dx or need_dw:
        y.backward(g.to(dev))
    torch.cuda.synchronize()
    return {"y": y.detach().cpu(), "dx": None if xd.grad is None else xd.grad.cpu(), "dw": None if wd.grad is None else wd.grad.cpu()}


def test_geometry():
    from multimodal_vae_amd.conv4s2 import conv4s2_geometry, conv4s2_workspace_bytes
    _dev()
    tile, ctile, chunk, max_chunks, max_ch, max_side = conv4s2_geometry()
    assert chunk == C.CHUNK and max_ch == 128 and max_side == 64 and tile >= 16 and ctile >= 16 and max_chunks >= 1
    for B, _, _, Hs, Ws in SHAPES[-2:]:
        assert B * (Hs // 2) * (Ws // 2) == chunk + 1 and max(Hs, Ws) <= max_side
    assert any(s[0] * (s[3] // 2) * (s[4] // 2) > tile and s[0] * (s[3] // 2) * (s[4] // 2) % tile for s in SHAPES)
    assert all(conv4s2_workspace_bytes(*s) > 0 for s in SHAPES)


@pytest.mark.parametrize("direction,act,shape", CASES, ids=_id)
def test_against_float64(direction, act, shape):
    dev = _dev()
    x, w, g = C.operands(direction, shape, seed=C.ACTS.index(act))
    got = _run(direction, x, w, g, act, dev)
    ref, yard, gates = C.reference(direction, x, w, g, act, SLOPE, y=got["y"])
    line = "%-5s %-8s %-24s" % (direction, act, _id(shape))
    errs = {}
    for k in ("y", "dx", "dw"):
        assert got[k].shape == ref[k].shape, k
        errs[k] = float((got[k].double() - ref[k]).abs().max())
        line += "  %s %.2e/%.2e %5.2f" % (k, errs[k], gates[k] / C.GATE_FACTOR, _ratio(errs[k], gates[k] / C.GATE_FACTOR))
    print(line)
    for k in errs:
        assert errs[k] <= gates[k], (k, errs[k], gates[k])


@pytest.mark.parametrize("direction,act,shape", [("down", "leaky", (3, 64, 128, 14, 14)), ("up", "sigmoid", (2, 1, 64, 28, 28)),
                                                 ("up", "relu", SHAPES[-2]), ("down", "none", (4, 72, 40, 8, 8)), ("down", "leaky", SHAPES[-1])], ids=_id)
def test_same_bits_twice(direction, act, shape):
    import multimodal_vae_amd.pixelcnn as P
    dev = _dev()
    x, w, g = C.operands(direction, shape)
    first = _run(direction, x, w, g, act, dev)
    for ws in P._CONV_WS.values():
        ws.view(torch.float32).fill_(float("nan"))
    again = _run(direction, x, w, g, act, dev)
    for k in first:
        assert torch.equal(first[k], again[k]), k
        assert not torch.isnan(first[k]).any()


@pytest.mark.parametrize("direction", ["down", "up"])
def test_sample_does_not_depend_on_the_batch(direction):
    dev = _dev()
    x, w, g = C.operands(direction, (17, 16, 8, 2, 6))
    many = _run(direction, x, w, g, "leaky", dev)
    for b in (0, 16):
        one = _run(direction, x[b:b + 1].clone(), w, g[b:b + 1].clone(), "leaky", dev)
        assert torch.equal(many["y"][b:b + 1], one["y"]) and torch.equal(many["dx"][b:b + 1], one["dx"])


@pytest.mark.parametrize("direction", ["down", "up"])
def test_needs_input_grad(direction):
    dev = _dev()
    x, w, g = C.operands(direction, (2, 3, 5, 4, 10))
    full = _run(direction, x, w, g, "relu", dev)
    no_dx = _run(direction, x, w, g, "relu", dev, need_dx=False)
    assert no_dx["dx"] is None and torch.equal(no_dx["dw"], full["dw"])
    no_dw = _run(direction, x, w, g, "relu", dev, need_dw=False)
    assert no_dw["dw"] is None and torch.equal(no_dw["dx"], full["dx"])
    with torch.no_grad():
        y = _op(direction)(x.to(dev), w.to(dev), "relu", SLOPE)
    assert not y.requires_grad and torch.equal(y.cpu(), full["y"])


@pytest.mark.parametrize("direction", ["down", "up"])
def test_memory_formats(direction):
    dev = _dev()
    shape = (2, 8, 16, 6, 10)
    x, w, g = C.operands(direction, shape)
    want = _run(direction, x, w, g, "leaky", dev, prepare=lambda t: t.contiguous(memory_format=torch.channels_last))
    nchw = _run(direction, x, w, g, "leaky", dev, prepare=lambda t: t.contiguous())
    strided = _run(direction, x, w, g, "leaky", dev, prepare=lambda t: torch.stack([t, t], dim=-1)[..., 0])     # every other element
    for got in (nchw, strided):
        for k in want:
            assert torch.equal(got[k], want[k]), k


def test_argument_errors_leave_the_device_usable():
    from multimodal_vae_amd._lib import MMVAEError
    from multimodal_vae_amd.conv4s2 import down4s2, up4s2
    dev = _dev()
    x, w, g = C.operands("down", (2, 3, 5, 4, 10))
    xd, wd = x.to(dev), w.to(dev)
    for bad in (lambda: down4s2(x, wd), lambda: up4s2(xd, w), lambda: down4s2(xd.double(), wd), lambda: down4s2(xd, wd, "tanh"),
                lambda: down4s2(xd[:, :, :3], wd), lambda: down4s2(xd, wd[:, :2]), lambda: up4s2(xd, wd),
                lambda: down4s2(torch.zeros(1, 3, 66, 4, device=dev), wd), lambda: down4s2(xd, torch.zeros(129, 3, 4, 4, device=dev))):
        with pytest.raises(MMVAEError):
            bad()
    got = _run("down", x, w, g, "none", dev)
    ref, _, gates = C.reference("down", x, w, g, "none", SLOPE, y=got["y"])
    assert float((got["y"].double() - ref["y"]).abs().max()) <= gates["y"]
