"""GPU tests of PixelCNN / GatedPixelCNN under ``set_conv_backend(model, "hip")``: every module type in isolation, whole models
(logits, loss and the gradient of every parameter) and a short training run.

Per module: forward and both gradients of ``m(x)`` against ``tapconv`` in float64 on bf16-rounded operands with the op-level gate of
tests/test_gpu_causal_conv.py (the tap list comes from ``causal_conv_ref.taps_ref``, not from the package): wrong wiring of taps to
modules shows here.

Whole model: the reference is pure float64 (``pixelcnn_ref.forward``).  The yardstick per tensor is the error of the emulated model
(``causal_conv_ref.QConv``: float64 arithmetic on operands rounded to bf16 as the op rounds them) against pure float64, that is the
bf16 quantisation itself; the kernel's error against pure float64 must be <= 2 x that yardstick, per tensor.  The factor 2: rounding
boundaries flip between two correct realisations (an fp32-accumulating emulation stood at <= 1.07 x the float64-accumulating one per
tensor, yet differed from it by up to half the yardstick on gated logits), so a gate on |kernel - emulation| would be wrong.

Training: the step-0 loss under "hip" against the torch backend's.  The yardstick is the loss's own emulation error, |cross entropy
of the emulated logits - cross entropy of the float64 logits| at step 0, as in the whole-model loss row; the bound is 2 x that.

MEASURED (kernel error / yardstick per tensor, the largest over the parameters for the gradients; `pytest -s` prints them):

kernel error / emulation yardstick, both against pure float64; the gate is 2.  MI355X:
plain-b3-c3-h48-v8-B3-6x9
  logits  3.236e-03 / 3.236e-03  1.00
  loss  2.464e-05 / 2.456e-05  1.00
  worst gradient: conv2.bias  5.988e-04 / 5.988e-04  1.00
gated-b3-c3-h48-v8-B3-6x9
  logits  5.732e-02 / 5.732e-02  1.00
  loss  9.480e-04 / 9.088e-04  1.04
  worst gradient: blocks.blocks.1.vertical_conv.weight  7.935e-04 / 7.743e-04  1.02
gated-b1-c1-h128-v8-B2-4x4
  logits  1.567e-02 / 1.567e-02  1.00
  loss  7.673e-04 / 5.174e-04  1.48
  worst gradient: conv4.bias  5.267e-04 / 5.036e-04  1.05
plain-b1-c3-h16-v256-B3-9x5
  logits  6.959e-03 / 6.959e-03  1.00
  loss  6.603e-05 / 6.600e-05  1.00
  worst gradient: conv4.bias  5.374e-06 / 5.374e-06  1.00
training plain: step 0 2.083780 (torch backend 2.083790, |difference| 1.07e-05 / loss yardstick 1.07e-05  1.01; gate 2), step 29 2.021025
training gated: step 0 2.114776 (torch backend 2.114779, |difference| 2.38e-06 / loss yardstick 2.37e-06  1.01; gate 2), step 29 2.053120
per module in isolation (op-level gate 8): the largest error / yardstick over 18 modules x {y, dx, dw, db} is 1.62
"""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import causal_conv_ref as C  # noqa: E402
import pixelcnn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# (gated, n_blocks, C, hid, V, B, H, W)
MODELS = [(0, 3, 3, 48, 8, 3, 6, 9), (1, 3, 3, 48, 8, 3, 6, 9), (1, 1, 1, 128, 8, 2, 4, 4), (0, 1, 3, 16, 256, 3, 9, 5)]


def _ratio(err, yard):
    return err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------ per module
def _module_cases():
    import multimodal_vae_amd.pixelcnn as P
    out = []
    for hid in (16, 48):
        g7, g3 = P.GatedResidualBlock("A", 3, hid, 7), P.GatedResidualBlock("B", hid, hid, 3)
        out += [("maskA7-h%d" % hid, P.MaskedConv2d("A", 3, hid, 7, 1, 3), ("A", 7, 7)),
                ("maskB3-h%d" % hid, P.MaskedConv2d("B", hid, hid, 3, 1, 1), ("B", 3, 3)),
                ("maskB1-h%d" % hid, P.MaskedConv2d("B", hid, 24, 1), ("one", 1, 1)),
                ("vert4x7-h%d" % hid, g7.vertical_conv, ("vertical", 4, 7)), ("vert2x3-h%d" % hid, g3.vertical_conv, ("vertical", 2, 3)),
                ("hor1x4-h%d" % hid, g7.horizontal_conv, ("horizontal", 1, 4)), ("hor1x2-h%d" % hid, g3.horizontal_conv, ("horizontal", 1, 2)),
                ("x_to_h-h%d" % hid, g3.x_to_h_conv, ("one", 1, 1)), ("gate1x1-h%d" % hid, g3.vertical_gate_conv, ("one", 1, 1))]
    return out


@pytest.mark.parametrize("case", _module_cases(), ids=lambda c: c[0])
def test_module_in_isolation(case):
    import multimodal_vae_amd.pixelcnn as P
    dev = _dev()
    name, module, kind = case
    torch.manual_seed(11)
    m = copy.deepcopy(module)
    with torch.no_grad():
        m.weight.mul_(3.0)
        m.bias.uniform_(-0.5, 0.5)
    taps = C.taps_ref(*kind)
    x = torch.randn(3, m.in_channels, 6, 9)
    g = torch.randn(3, m.out_channels, 6, 9)
    w = m.weight.detach().clone()
    if isinstance(m, P.MaskedConv2d):
        w = w * m.mask                                     # what the forward leaves in the parameter
    ref, yard, gates = C.reference(x, w, m.bias.detach().clone(), g, taps)
    m = m.to(dev)
    m.conv_backend = "hip"
    xd = x.to(dev).requires_grad_()
    y = P._conv1x1(m, xd) if type(m) is torch.nn.Conv2d else m(xd)
    y.backward(g.to(dev))
    got = {"y": y.detach().cpu(), "dx": xd.grad.cpu(), "dw": m.weight.grad.cpu(), "db": m.bias.grad.cpu()}
    line = "%-14s" % name
    for k in got:
        err = float((got[k].double() - ref[k]).abs().max())
        line += "  %s %.2e/%.2e %5.2f" % (k, err, gates[k] / C.GATE_FACTOR, _ratio(err, gates[k] / C.GATE_FACTOR))
        assert err <= gates[k], (k, err, gates[k])
    print(line)
    if isinstance(m, P.MaskedConv2d):
        assert torch.equal(m.weight.detach().cpu(), w)     # the forward masked the parameter in place
        assert torch.equal(got["dw"] * (1 - m.mask.cpu()), torch.zeros_like(w))


# ------------------------------------------------------------------------------------------------------ whole model
def _loss_and_grads(fwd, sd, cfg, x, target):
    from multimodal_vae_amd.pixelcnn import cross_entropy_by_dim
    leaves = {k: v.double().clone().requires_grad_(k.endswith(("weight", "bias"))) for k, v in sd.items()}
    logits = fwd(leaves, cfg, x)
    loss = cross_entropy_by_dim(logits, target)
    names = [k for k, v in leaves.items() if v.requires_grad]
    grads = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)      # (the last block's vertical gate feeds nothing)
    return logits.detach(), float(loss.detach()), {k: g for k, g in zip(names, grads) if g is not None}


@pytest.mark.parametrize("spec", MODELS, ids=lambda s: "%s-b%d-c%d-h%d-v%d-B%d-%dx%d" % (("gated" if s[0] else "plain",) + tuple(s[1:])))
def test_whole_model(spec):
    import multimodal_vae_amd.pixelcnn as P
    dev = _dev()
    c = R.case(*spec)
    cfg, sd = c["cfg"], c["sd"]
    target = c["given"]
    x32 = target.float() / (cfg["out_dims"] - 1)
    l64, loss64, g64 = _loss_and_grads(R.forward, sd, cfg, x32.double(), target)
    lem, lossem, gem = _loss_and_grads(C.emulated_forward, sd, cfg, x32.double(), target)

    model = P.set_conv_backend(copy.deepcopy(c["model"]), "hip").to(dev)
    logits = model(x32.to(dev))
    loss = P.cross_entropy_by_dim(logits, target.to(dev))
    loss.backward()
    rows = [("logits", float((logits.detach().cpu().double() - l64).abs().max()), float((lem - l64).abs().max())),
            ("loss", abs(float(loss.detach()) - loss64), abs(lossem - loss64))]
    masked = 0
    for name, p in model.named_parameters():
        assert (p.grad is not None) == (name in g64), name
        if p.grad is None:
            continue
        got = p.grad.cpu().double()
        rows.append((name, float((got - g64[name]).abs().max()), float((gem[name] - g64[name]).abs().max())))
        mod = model.get_submodule(name.rsplit(".", 1)[0])
        if name.endswith("weight") and isinstance(mod, P.MaskedConv2d):
            assert torch.equal(got * (1 - mod.mask.cpu().double()), torch.zeros_like(got)), name
            masked += int((mod.mask == 0).sum())
    assert masked > 0 or spec[0]                           # (the gated model masks 1 x 1 kernels only: nothing to zero)
    worst = max(rows[2:], key=lambda r: r[1] / r[2] if r[2] > 0 else float("inf"))
    for label, (n, e, yd) in (("logits", rows[0]), ("loss", rows[1]), ("worst gradient: " + worst[0], worst)):
        print("%-60s %.3e / %.3e  %5.2f" % (label, e, yd, e / yd if yd > 0 else float("inf")))
    for n, e, yd in rows:
        assert e <= 2 * yd, (n, e, yd)


# ------------------------------------------------------------------------------------------------------ training
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_training(gated):
    import multimodal_vae_amd.pixelcnn as P
    import multimodal_vae_amd.train_pixelcnn as T
    dev = _dev()
    V = 8
    data = T.preprocess(T.synthetic_images(16, 1, 8, seed=3), V)
    torch.manual_seed(21)
    model = (P.GatedPixelCNN if gated else P.PixelCNN)(n_blocks=1, data_channels=1, hid_dims=16, out_dims=V)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    cfg = R.make_cfg(gated, 1, 1, 16, V)
    target = (data * (V - 1)).long()
    with torch.no_grad():
        yard = abs(float(P.cross_entropy_by_dim(C.emulated_forward(sd, cfg, data.double()), target))
                   - float(P.cross_entropy_by_dim(R.forward(sd, cfg, data.double()), target)))
        loss_torch = float(P.cross_entropy_by_dim(copy.deepcopy(model).to(dev)(data.to(dev)), target.to(dev)))
    model = P.set_conv_backend(model, "hip").to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    losses = [T.train_step(model, opt, data.to(dev), V)[0] for _ in range(30)]
    print("%s: step 0 %.6f (torch backend %.6f, |difference| %.2e / loss yardstick %.2e  %.2f), step 29 %.6f"
          % ("gated" if gated else "plain", losses[0], loss_torch, abs(losses[0] - loss_torch), yard, _ratio(abs(losses[0] - loss_torch), yard),
             losses[-1]))
    assert losses[-1] < losses[0]
    assert abs(losses[0] - loss_torch) <= 2 * yard
    for m in model.modules():
        if isinstance(m, P.MaskedConv2d):
            assert torch.equal(m.weight.detach() * (1 - m.mask), torch.zeros_like(m.weight))
    # the same model still evaluates and samples
    with torch.no_grad():
        model.eval()
        assert torch.isfinite(model(data.to(dev))).all()
    out = P.generate(model, 2, 8, 8, seed=1)
    assert out.levels.shape == (2, 1, 8, 8)
