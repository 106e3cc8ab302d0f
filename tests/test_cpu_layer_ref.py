"""CPU companion of tests/test_gpu_layers.py: the float64 layer reference (tests/layer_ref.py) the GPU test trusts is tied to the
model definition in oracle/mmvae_ref.py, and its operand generator stays inside the regime where bf16 operands with fp32
accumulation reproduce float64 bit for bit."""
import pytest
import torch
import torch.nn.functional as F

import layer_ref as LR
from oracle import mmvae_ref as R

BMAX = max(LR.BATCHES)


@pytest.mark.parametrize("name", list(LR.LAYERS))
def test_operands_stay_in_the_exact_regime(name):
    """largest batch of the matrix: forward on gf * B images, both gradients on gb * B images"""
    L = LR.LAYERS[name]
    ws, xs = [], []
    for seed in LR.SEEDS:
        x, w, _ = LR.layer_operands(name, L.gf * BMAX, seed)
        out = LR.ref_forward(L, x, w)
        LR.assert_exact_regime(out=out, groups=L.gf, what="%s forward seed %d" % (name, seed))
        assert float(out.abs().max()) > 0
        xb, wb, dy = LR.layer_operands(name, L.gb * BMAX, seed)
        LR.assert_exact_regime(dw=LR.ref_wgrad(L, xb, dy), what="%s wgrad seed %d" % (name, seed))
        acc = LR.ref_dgrad_acc(L, dy, wb)
        assert bool((acc == acc.round()).all()) and float(acc.abs().max()) <= 256, (name, float(acc.abs().max()))
        ws.append(w)
        xs.append(x)
    LR.assert_operand_coverage(ws, xs)


class _Recorder:
    """stands in for torch.nn.functional inside the oracle module: records every conv / transposed conv call"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return getattr(F, name)

    def _rec(self, fn, transposed, x, w, b, stride, pad):
        x.retain_grad()
        out = fn(x, w, b, stride, pad)
        out.retain_grad()
        self.calls.append(dict(transposed=transposed, x=x, w=w, out=out, stride=stride, pad=pad))
        return out

    def conv2d(self, x, w, b, stride, pad):
        return self._rec(F.conv2d, False, x, w, b, stride, pad)

    def conv_transpose2d(self, x, w, b, stride, pad):
        return self._rec(F.conv_transpose2d, True, x, w, b, stride, pad)


def test_reference_agrees_with_autograd_on_the_oracle_modules(monkeypatch):
    """every conv of oracle.mmvae_ref's MultiMNIST image encoder / decoder, run in float64 with autograd: the layer table's
    geometry (kernel, stride, padding, transposed, sizes, parameter name) reproduces the module's output, weight gradient and
    input gradient from the recorded operands"""
    torch.manual_seed(0)
    B = 3
    P = {k: (v.double().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.double() if v.is_floating_point() else v)
         for k, v in R.formula_params("multimnist", 100).items()}
    rec = _Recorder()
    monkeypatch.setattr(R, "F", rec)
    image = torch.rand(B, 1, 50, 50, dtype=torch.float64).requires_grad_(True)
    z = torch.randn(B, 100, dtype=torch.float64)
    enc = R.multimnist_image_encoder(P, image * 1.0, True, None, drop_p=0.0)
    dec = R.multimnist_image_decoder_logits(P, z, True)
    ((enc * torch.randn_like(enc)).sum() + (dec * torch.randn_like(dec)).sum()).backward()
    monkeypatch.undo()
    assert len(rec.calls) == 8
    by_weight = {id(c["w"]): c for c in rec.calls}
    for name, L in LR.LAYERS.items():
        c = by_weight[id(P[L.param])]
        assert c["transposed"] == L.transposed and c["stride"] == L.stride and c["pad"] == L.pad, name
        assert tuple(c["w"].shape) == LR.weight_shape(L), name
        x, dy = LR._nhwc(c["x"].detach()), LR._nhwc(c["out"].grad)
        assert tuple(x.shape) == (B, L.ih, L.ih, L.cin) and tuple(dy.shape) == (B, L.oh, L.oh, L.cout), name
        w = c["w"].detach()
        torch.testing.assert_close(LR.ref_forward(L, x, w), LR._nhwc(c["out"].detach()), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(LR.ref_wgrad(L, x, dy), c["w"].grad, rtol=1e-10, atol=1e-12)
        torch.testing.assert_close(LR.ref_dgrad_acc(L, dy, w), LR._nhwc(c["x"].grad), rtol=1e-10, atol=1e-12)


def test_epilogue_reference_is_swish_batchnorm_backward():
    """ref_dgrad_epilogue == autograd of Swish(scale * r + shift) times the incoming gradient, and its sums are the two reductions
    of the BatchNorm backward: sum dy_bn and sum dy_bn * xhat"""
    g = LR.gen(5, 1)
    groups, n, C = 2, 4, 8
    acc = LR.ternary((groups * n, 3, 3, C), 0.7, g) * torch.randint(1, 40, (groups * n, 3, 3, C), generator=g)
    r = LR.eighths((groups * n, 3, 3, C), g)
    aff, mr = LR.dyadic_tables(groups, C, g)
    v, red, red_abs = LR.ref_dgrad_epilogue(acc, r, aff, mr, groups)
    rr = r.clone().reshape(groups, -1, C).requires_grad_(True)
    pre = rr * aff[:, None, :, 0] + aff[:, None, :, 1]
    y = pre * torch.sigmoid(pre)
    # d/d(pre) of sum(acc * Swish(pre)): the gradient w.r.t. the BatchNorm output
    (gpre,) = torch.autograd.grad((y * acc.reshape(groups, -1, C)).sum(), pre)
    torch.testing.assert_close(v.reshape(groups, -1, C), gpre, rtol=1e-13, atol=1e-13)
    xhat = (rr.detach() - mr[:, None, :, 0]) * mr[:, None, :, 1]
    torch.testing.assert_close(red[..., 0], gpre.sum(1), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(red[..., 1], (gpre * xhat).sum(1), rtol=1e-13, atol=1e-13)
    assert bool((red_abs >= red.abs() - 1e-12).all())
    # no tables: plain Swish'(r), no sums
    v0, red0, _ = LR.ref_dgrad_epilogue(acc, r, None, None, groups)
    r0 = r.clone().requires_grad_(True)
    (g0,) = torch.autograd.grad((r0 * torch.sigmoid(r0) * acc).sum(), r0)
    torch.testing.assert_close(v0, g0, rtol=1e-13, atol=1e-13)
    assert red0 is None


def test_epilogue_inputs_are_exact_in_their_formats():
    g = LR.gen(6, 2)
    r = LR.eighths((1000,), g)
    assert torch.equal(r.to(torch.bfloat16).double(), r) and float(r.abs().max()) <= 4
    aff, mr = LR.dyadic_tables(3, 64, g)
    for t in (aff, mr):
        assert torch.equal(t.float().double(), t)
    pre32 = r.float()[:, None, None] * aff[..., 0].float() + aff[..., 1].float()
    assert torch.equal(pre32.double(), r[:, None, None] * aff[..., 0] + aff[..., 1])
    xh32 = (r.float()[:, None, None] - mr[..., 0].float()) * mr[..., 1].float()
    assert torch.equal(xh32.double(), (r[:, None, None] - mr[..., 0]) * mr[..., 1])
