"""The float64 reference of classifier.0's data gradient (tests/gemm_small_forms_ref.py) against torch.autograd, and the gates of
tests/test_gpu_gemm_small_forms.py against the faults this launch can have.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import layer_ref as LR
import gemm_small_forms_ref as GR

BATCHES = (7, 8, 12)


@pytest.mark.parametrize("B", BATCHES)
def test_reference_is_autograd_through_linear_batchnorm_swish(B):
    """multimnist/model.py: features end in BatchNorm2d + Swish on the 2x2x256 map, classifier.0 is a Linear over its NCHW
    flatten.  With b = scale * r4 + shift (the BatchNorm output, one copy per row: both dropout variants share the B images) the
    launch's result is d sum(y1 * dy1) / d b, and its sums are those of the BatchNorm backward."""
    for seed in LR.SEEDS:
        dy1, W1, r4, aff, mr = GR.fc1_dgrad_operands(B, seed)
        acc, v, red, red_abs = GR.ref_fc1_dgrad(dy1, W1, r4, aff, mr)
        b = (LR._nchw(r4) * aff[0, :, 0][None, :, None, None] + aff[0, :, 1][None, :, None, None]).repeat(2, 1, 1, 1).requires_grad_(True)
        y1 = F.linear((b * torch.sigmoid(b)).reshape(2 * B, 1024), W1)
        y1.backward(dy1)
        want = LR._nhwc(b.grad)
        assert float((v - want).abs().max()) <= 1e-12 * float(want.abs().max())
        xhat = (r4.repeat(2, 1, 1, 1) - mr[0, :, 0]) * mr[0, :, 1]
        assert torch.allclose(red[0, :, 0], want.reshape(-1, 256).sum(0), rtol=0, atol=1e-9)
        assert torch.allclose(red[0, :, 1], (want * xhat).reshape(-1, 256).sum(0), rtol=0, atol=1e-9)
        # the regime of the comparison: integer accumulator that bf16 holds, operands exact in their formats
        assert bool((acc == acc.round()).all()) and float(acc.abs().max()) <= 256
        assert torch.equal(r4.to(torch.bfloat16).double(), r4) and torch.equal(aff.float().double(), aff)


@pytest.mark.parametrize("fault", ["pixel0", "pixel3", "broadcast", "affine"])
def test_gates_see_every_fault(fault):
    """the reference passes its own gates; a dropped pixel class, a second variant that reads other images and a missing affine do not"""
    kw = {"pixel0": dict(pixels=(1, 2, 3)), "pixel3": dict(pixels=(0, 1, 2)), "broadcast": dict(broadcast=False), "affine": dict(affine=False)}[fault]
    for B in BATCHES:
        for seed in LR.SEEDS:
            ops = GR.fc1_dgrad_operands(B, seed)
            acc, v, red, red_abs = GR.ref_fc1_dgrad(*ops)
            LR.gate_elements(v.to(torch.bfloat16), v, acc, "reference")
            LR.gate_sums(red.float(), red, red_abs, "reference")
            _, bad_v, bad_red, _ = GR.ref_fc1_dgrad(*ops, **kw)
            with pytest.raises(AssertionError):
                LR.gate_elements(bad_v.to(torch.bfloat16), v, acc, fault)
            with pytest.raises(AssertionError):
                LR.gate_sums(bad_red.float(), red, red_abs, fault)
