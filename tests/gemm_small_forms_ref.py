"""Operands and float64 reference of classifier.0's data gradient as the MultiMNIST encoder backward launches it (csrc/multimnist.hip
fc1_dgrad_gemm, replay name enc_fc1_dgrad), shared by tests/test_gpu_gemm_small_forms.py and tests/test_cpu_gemm_small_forms.py.

The launch: rows = 2B samples (both dropout variants) of dy1 [rows][400] times classifier.0's weight, one [256][400] matrix per
pixel of the 2x2 map (4 pixel classes), into the NHWC gradient db4 [rows][2][2][256]; the epilogue multiplies by
Swish'(scale * r4 + shift) with the saved raw conv4 output r4 [B][2][2][256] that BOTH variants share (row n reads image n % B:
d_bcast_n = B) and the BatchNorm tables of conv4 (d_affine, d_meanrstd), and adds the BatchNorm-backward sums into d_red.
Operand recipes are those of tests/test_gpu_layers.py test_dense_layers: ternary dy1 and weights, eighths for r4, dyadic tables."""
import functools

import torch

import layer_ref as LR


@functools.lru_cache(maxsize=None)
def fc1_dgrad_operands(B, seed):
    """-> dy1 [2B][400], W1 [400][1024] (the parameter's layout: column c * 4 + y * 2 + x of torch's NCHW flatten),
    r4 [B][2][2][256], aff [1][256][2], mr [1][256][2]"""
    g = LR.gen(seed, 13, B)
    dy1 = LR.ternary((2 * B, 400), 0.5, g)
    W1 = LR.ternary((400, 1024), 0.25, g)
    r4 = LR.eighths((B, 2, 2, 256), g)
    aff, mr = LR.dyadic_tables(1, 256, g)
    return dy1, W1, r4, aff, mr


def ref_fc1_dgrad(dy1, W1, r4, aff, mr, pixels=(0, 1, 2, 3), broadcast=True, affine=True):
    """-> acc (the exact integer accumulator), v (= db4), red [1][256][2], red_abs, all float64; NHWC [2B][2][2][256].
    The keyword arguments build the WRONG results the CPU test shows the gates to reject: a pixel class left out, the second
    variant reading other images than the first, the BatchNorm affine left out."""
    rows, B = dy1.shape[0], r4.shape[0]
    acc = LR._nhwc((dy1.double() @ W1.double()).reshape(rows, 256, 2, 2))
    for pix in range(4):
        if pix not in pixels:
            acc[:, pix // 2, pix % 2, :] = 0
    assert rows == 2 * B
    r = torch.cat([r4.double(), r4.double() if broadcast else r4.double().roll(1, 0)])
    v, red, red_abs = LR.ref_dgrad_epilogue(acc, r, aff if affine else None, mr, 1)
    return acc, v, red, red_abs
