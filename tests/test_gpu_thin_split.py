"""The half-image forms of the thin MultiMNIST kernels against float64: conv1.hip's forward (two workgroups per image) and the
training form of dec_last.hip's fused decoder tail (grid (B, G, 2)), launched through mmvae_mm_bench_layer on operands this test
wrote into the workspace -- "enc_conv1_mfma", "enc_conv1_wgrad_mfma" (the image batch in tmp_f32) and "dec_last_fused_reduce" (the
tail, the sum of its weight-gradient partials, and its optional outputs logits / recon / dlogit).  B = 7 and 8: the harness's
smallest, odd and even; the geometry of a workgroup does not depend on B.

conv1: Tier A of tests/test_gpu_layers.py (ternary image, integer weights: torch.equal), the Swish copy within its Tier B gate.

Decoder tail.  Its operands are not integers (A = Swish(BatchNorm(q3)) rounded to bf16, dlogit = coef (p - t) rounded to bf16 for
the patches), so the chain is checked link by link, every link against float64 on inputs that are exact:
  * the BatchNorm tables the launch writes, and the running statistics, from the slot sums the test wrote (exact in fp32): the
    gates of test_gpu_coco_layers.py::test_bn_forward (fp32 roundings of csrc/bn_dev.h counted there);
  * logits from A = Swish(scale * q3 + shift) of the gated tables: A reaches the MFMA as bf16, 2^-8 |A| either rounding, and 128
    fp32 additions (32 channels x 4 overlapping taps) follow: |err| <= (2^-8 + 128 * 2^-24) sum |A| |w|;
  * recon, dlogit and the BCE sums from the logits the launch wrote: the last-layer gates of test_gpu_coco_layers.py::test_dec_last_fwd
    (targets 0 / 1 and |logit| <= 3 keep |p - t| >= 0.047: the no-cancellation margin of LAST_TARGETS);
  * the input gradient d3 and the BatchNorm-backward sums red_d2 from the dlogit the launch wrote, rounded to bf16 as the patches
    are: weights of +-1/16 and dlogit within a factor 2^12 make every accumulator a sum of at most 16 products that is exact in fp32,
    so Tier B of test_gpu_layers.py applies as it stands (one bf16 ulp + 1e-5 |acc|; 2^-16 sum |terms| for the sums);
  * the weight gradient after the reduction from bf16(A) and bf16(dlogit): 2^-16 sum |terms| for the order of the fp32 sums (the
    gate of the BatchNorm-backward sums), plus |A_hi - A_lo| |dlogit| over the elements whose bf16 rounding the fp32 error of the
    staging (16 eps |A| + 2 eps (|scale q3| + |shift|)) can flip.
test_tail_seam: what a wrong split would break -- a row counted twice or never, a halo row read from the wrong place, a pixel
owned by both workgroups or none -- on one-hot activations around the seam (input rows 11 - 13, 24, the corners) and one-hot
targets at output rows 24 - 27, at image 0 and at the last image of the last group."""
import math

import pytest
import torch
import torch.nn.functional as F

import layer_ref as LR
from layer_ref import SEEDS

pytestmark = pytest.mark.gpu

BATCHES = (7, 8)
_H = {}
F0, F9, BN7 = "image_encoder.features.0.weight", "image_decoder.hallucinate.9.weight", "image_decoder.hallucinate.7"
E = LR.EPS32


def _harness(B):
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    if B not in _H:
        _H.clear()
        torch.cuda.empty_cache()
        h = LR.LayerHarness(B)
        for n in ("sums", "recon"):          # names mmvae_mm_debug_offset knows beyond layer_ref.WS_NAMES
            h.offsets[n] = int(h.call("mmvae_mm_debug_offset", h.eng.h, n.encode()))
            assert h.offsets[n] >= 0
        _H[B] = h
    return _H[B]


def _within(got, ref, gate, what):
    got = got.double().cpu()
    err = (got - ref).abs()
    if LR.REPORT:
        print("SPLIT %s: worst err/gate %.3f" % (what, float((err / gate.clamp_min(1e-300)).max())))
    bad = ~(err <= gate)
    assert not bool(bad.any()), (what, "%d of %d outside the gate; first %s got %s want %s gate %s" % (
        int(bad.sum()), bad.numel(), torch.nonzero(bad)[:6].tolist(), got[bad][:6].tolist(), ref[bad][:6].tolist(), gate[bad][:6].tolist()))


def _bf16(t):
    return t.to(torch.bfloat16).double()


# ------------------------------------------------------------------------------------------------ conv1
@pytest.mark.parametrize("B", BATCHES)
def test_conv1_forward_exact(B):
    """r1 = conv2d(image, w0, stride 2, padding 1) bit for bit on a ternary image and integer weights; a1 within one bf16 ulp of
    Swish(r1).  The image batch is read as fp32 from tmp_f32."""
    h = _harness(B)
    for seed in SEEDS:
        g = LR.gen(seed, 31, B)
        img = LR.ternary((B, 1, 50, 50), 0.5, g)
        w0 = torch.randint(-3, 4, (32, 1, 4, 4), generator=g).double()
        ref = LR._nhwc(F.conv2d(img, w0, None, 2, 1))
        LR.assert_exact_regime(out=ref, what="enc_conv1_mfma")
        h.set_weight(F0, w0)
        h.put("tmp_f32", img, torch.float32)
        h.zero("r1", ref.numel(), torch.bfloat16)
        h.zero("a1", ref.numel(), torch.bfloat16)
        launches = h.run("enc_conv1_mfma")
        assert any("conv1_fwd_half_kernel" in k for _, k in launches), launches
        got = h.get("r1", ref.shape).double().cpu()
        assert torch.equal(got, ref), (B, seed, launches, LR.describe_mismatch(got, ref))
        LR.gate_elements(h.get("a1", ref.shape), ref * torch.sigmoid(ref), ref, "enc_conv1_mfma a1 B=%d seed %d" % (B, seed))


@pytest.mark.parametrize("B", BATCHES)
def test_conv1_forward_one_hot(B):
    """a single +1 in the image at the seam rows of the two workgroups (output rows 11 - 13 read image rows 21 - 28) and at the
    corners, distinct integer weights: every output pixel carries the tap the geometry says"""
    h = _harness(B)
    w0 = ((torch.arange(512, dtype=torch.int64) * 2654435761 >> 7) % 253 - 126).double().reshape(32, 1, 4, 4)
    h.set_weight(F0, w0)
    for (im, y, x) in ((0, 0, 0), (B - 1, 49, 49), (0, 49, 0), (B - 1, 0, 49), (0, 22, 10), (B - 1, 23, 40), (B // 2, 24, 39), (0, 25, 41),
                       (B - 1, 26, 0), (0, 27, 49)):
        img = torch.zeros(B, 1, 50, 50, dtype=torch.float64)
        img[im, 0, y, x] = 1.0
        ref = LR._nhwc(F.conv2d(img, w0, None, 2, 1))
        h.put("tmp_f32", img, torch.float32)
        h.zero("r1", ref.numel(), torch.bfloat16)
        h.run("enc_conv1_mfma")
        got = h.get("r1", ref.shape).double().cpu()
        assert torch.equal(got, ref), (B, (im, y, x), LR.describe_mismatch(got, ref))


@pytest.mark.parametrize("B", BATCHES)
def test_conv1_wgrad_exact(B):
    """the in-step weight gradient of conv1 (float atomics into the packed gradient): ternary image and gradient, then one-hot
    gradient pixels at output rows 11, 12, 13 and the corners on a dense image of small integers"""
    h = _harness(B)
    for seed in SEEDS:
        g = LR.gen(seed, 32, B)
        img = LR.ternary((B, 1, 50, 50), 0.5, g)
        d1 = LR.ternary((B, 25, 25, 32), 0.5, g)
        wz = torch.zeros(32, 1, 4, 4, dtype=torch.float64, requires_grad=True)
        F.conv2d(img, wz, None, 2, 1).backward(LR._nchw(d1))
        h.put("tmp_f32", img, torch.float32)
        h.put("d1e", d1)
        LR.check_wgrad(h, "enc_conv1_wgrad_mfma", F0, wz.grad, ({},), "enc_conv1_wgrad_mfma B=%d seed %d" % (B, seed))
    g = LR.gen(0, 33, B)
    img = torch.randint(-3, 4, (B, 1, 50, 50), generator=g).double()
    h.put("tmp_f32", img, torch.float32)
    for (im, oy, ox, ch) in ((0, 0, 0, 0), (B - 1, 24, 24, 31), (0, 11, 3, 5), (B - 1, 12, 19, 7), (0, 12, 20, 9), (B // 2, 13, 24, 30), (0, 24, 0, 16)):
        d1 = torch.zeros(B, 25, 25, 32, dtype=torch.float64)
        d1[im, oy, ox, ch] = 1.0
        wz = torch.zeros(32, 1, 4, 4, dtype=torch.float64, requires_grad=True)
        F.conv2d(img, wz, None, 2, 1).backward(LR._nchw(d1))
        if float(wz.grad.abs().max()) == 0:
            continue
        h.put("d1e", d1)
        LR.check_wgrad(h, "enc_conv1_wgrad_mfma", F0, wz.grad, ({},), "enc_conv1_wgrad_mfma B=%d one-hot %s" % (B, (im, oy, ox, ch)))


# ------------------------------------------------------------------------------------------------ decoder tail
def _bn_slot(h, bn):
    for i, (n, C, off) in enumerate(h.st.bn_table):
        if n == bn:
            return i, C, off
    raise KeyError(bn)


def _run_tail(h, B, q3, stats, gamma, beta, w9, target, rm0, rv0):
    """writes the operands, runs dec_last_fused_reduce once -> dict of what the launch left"""
    idx, C, soff = _bn_slot(h, BN7)
    assert C == 32
    h.set_weight(BN7 + ".weight", gamma)
    h.set_weight(BN7 + ".bias", beta)
    h.set_weight(F9, w9)
    h.st.bn_stats[soff:soff + C] = rm0.float().to(h.dev)
    h.st.bn_stats[soff + C:soff + 2 * C] = rv0.float().to(h.dev)
    h.st.bn_nbt[idx] = 5
    h.put("q3", q3)
    h.put("st_d2", stats, torch.float32)
    h.put("tmp_f32", target, torch.float32)
    n2 = 2 * B * 2500
    for name in ("logits", "recon", "dlogit"):
        h.buf(name, n2, torch.float32).fill_(7.0)
    h.buf("d3", 2 * B * 625 * 32, torch.bfloat16).fill_(7.0)
    h.zero("red_d2", 3 * LR.STAT_SLOTS * 32 * 2, torch.float32)
    h.zero("aff_d2", 3 * 32 * 2, torch.float32)
    h.zero("mr_d2", 3 * 32 * 2, torch.float32)
    h.zero("sums", 16 * LR.LOSS_SLOTS, torch.float32)
    h.st.gpk.zero_()
    launches = h.run("dec_last_fused_reduce")
    assert any("dec_last_half_kernel" in k for _, k in launches), launches
    out = {n: h.get(n, (2 * B, 1, 50, 50), torch.float32).double().cpu() for n in ("logits", "recon", "dlogit")}
    out["d3"] = h.get("d3", (2 * B, 25, 25, 32))
    out["red"] = h.stats("red_d2", 2, 32)
    out["aff"] = h.get("aff_d2", (3, 32, 2), torch.float32).double().cpu()
    out["mr"] = h.get("mr_d2", (3, 32, 2), torch.float32).double().cpu()
    out["sums"] = h.get("sums", (LR.LOSS_SLOTS, 16), torch.float32).double().cpu()
    out["dw"], out["dw_others"] = h.packed_grad(F9)
    out["rm"] = h.st.bn_stats[soff:soff + C].double().cpu()
    out["rv"] = h.st.bn_stats[soff + C:soff + 2 * C].double().cpu()
    out["nbt"] = int(h.st.bn_nbt[idx])
    return out


def _check_backward(B, q3, w9, out, what):
    """d3, red_d2 and the reduced weight gradient from what the launch itself wrote in front of them (tables, dlogit)"""
    aff, mr = out["aff"][:2], out["mr"][:2]
    r = q3[:2 * B]
    dlb = _bf16(out["dlogit"])                                   # the patches: dlogit as bf16
    ex = dlb[dlb != 0].abs().log2().floor()
    assert float(ex.max() - ex.min()) <= 12          # 8 bits + 12 + 4 (16 terms) <= 24: every accumulator is exact in fp32
    acc = LR._nhwc(F.conv2d(dlb, w9, None, 2, 1))                # input gradient of the transposed conv: the same weight as a conv
    v, red, red_abs = LR.ref_dgrad_epilogue(acc, r, aff, mr, 2)
    LR.gate_elements(out["d3"], v, acc, what + " d3")
    LR.gate_sums(out["red"], red, red_abs, what + " red_d2")
    # weight gradient: A = bf16(Swish(scale r + shift)); an element whose rounding the fp32 error of the staging can flip may take
    # either neighbour
    C = 32
    y = r.reshape(2, -1, C) * aff[:, None, :, 0] + aff[:, None, :, 1]
    a64 = (y * torch.sigmoid(y)).reshape(r.shape)
    slack = 16 * E * a64.abs() + (2 * E * ((r.reshape(2, -1, C) * aff[:, None, :, 0]).abs() + aff[:, None, :, 1].abs())).reshape(r.shape)
    a_lo, a_hi = _bf16(a64 - slack), _bf16(a64 + slack)
    def dw_of(a, d):
        wz = torch.zeros(32, 1, 4, 4, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(LR._nchw(a), wz, None, 2, 1).backward(d)
        return wz.grad
    ref = dw_of(_bf16(a64), dlb)
    gate = 2.0 ** -16 * dw_of(_bf16(a64).abs(), dlb.abs()) + dw_of((a_hi - a_lo).abs(), dlb.abs())
    assert float(ref.abs().max()) > 0
    _within(out["dw"], ref, gate, what + " dW")
    assert out["dw_others"] == 0.0, what + ": another parameter's packed gradient was written"
    return ref, gate


@pytest.mark.parametrize("B", BATCHES)
def test_tail_against_float64(B):
    h = _harness(B)
    count, C = B * 625, 32
    for seed in SEEDS:
        g = LR.gen(seed, 34, B)
        what = "dec_last_fused_reduce B=%d seed %d" % (B, seed)
        q3 = LR.eighths((3 * B, 25, 25, C), g)
        gamma = torch.tensor([1.0, 2.0, -1.0])[torch.randint(0, 3, (C,), generator=g)].double()
        beta = torch.randint(-1, 2, (C,), generator=g).double() / 2
        rm0 = torch.randint(-4, 5, (C,), generator=g).double() / 4
        rv0 = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)].double()
        w9 = LR.ternary((C, 1, 4, 4), 0.125, g) / 16        # logits of a few tenths: max |logit| <= 3 is asserted below
        target = torch.randint(0, 2, (B, 1, 50, 50), generator=g).double()
        stats = LR.slot_stats_any(q3, 3)
        assert torch.equal(stats.float().double(), stats)
        out = _run_tail(h, B, q3, stats, gamma, beta, w9, target, rm0, rv0)
        # tables of all 3 groups, running statistics (3 groups x 1 update), the batch counter: once per launch
        scale, shift, mean, rstd = LR.ref_bn_tables(stats, count, gamma, beta)
        _within(out["aff"][..., 0], scale, 12 * E * scale.abs(), what + " scale")
        _within(out["aff"][..., 1], shift, 16 * E * ((mean.abs() + 4) * scale.abs() + beta.abs()[None]), what + " shift")
        _within(out["mr"][..., 0], mean, 16 * E * 4 * torch.ones_like(mean), what + " mean")
        _within(out["mr"][..., 1], rstd, 11 * E * rstd, what + " rstd")
        rm, rv, unb = LR.ref_bn_running(stats, count, rm0, rv0, 1)
        _within(out["rm"], rm, (16 + 5 * 3) * E * 4 * torch.ones_like(rm), what + " running_mean")
        _within(out["rv"], rv, (22 + 5 * 3) * E * torch.maximum(unb, rv0), what + " running_var")
        assert out["nbt"] == 5 + 3, (what, out["nbt"])
        # logits from the gated tables
        a64, _ = LR.ref_stage_fwd(q3[:2 * B], out["aff"][:2, :, 0], out["aff"][:2, :, 1], 2)
        lref = F.conv_transpose2d(LR._nchw(a64), w9, None, 2, 1)
        labs = F.conv_transpose2d(LR._nchw(a64.abs()), w9.abs(), None, 2, 1)
        _within(out["logits"], lref, (2.0 ** -8 + 128 * E) * labs, what + " logits")
        assert float(out["logits"].abs().max()) <= 3.0, float(out["logits"].abs().max())        # |p - t| >= 0.047 for t in {0, 1}
        # recon, dlogit, BCE sums from the logits the launch wrote
        coef = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(B * 2500), dtype=torch.float32)
        lg = out["logits"]
        p = torch.sigmoid(lg)
        t = target.repeat(2, 1, 1, 1)
        LR.gate_last_layer(out["recon"], p, LR.LAST_RECON_MULT, what + " recon")
        LR.gate_last_layer(out["dlogit"], float(coef) * (p - t), LR.LAST_DLOGIT_MULT, what + " dlogit")
        terms = -(t * F.logsigmoid(lg).clamp_min(-100.0) + (1 - t) * F.logsigmoid(-lg).clamp_min(-100.0)).reshape(2, -1)
        LR.gate_last_sums(out["sums"][:, :2].sum(0), terms.sum(1), terms.abs().sum(1), what + " BCE sums")
        assert float(out["sums"][:, 2:].abs().max()) == 0.0, what + " wrote a loss column other than its two"
        _check_backward(B, q3, w9, out, what)


@pytest.mark.parametrize("B", BATCHES)
def test_tail_seam(B):
    h = _harness(B)
    count, C = B * 625, 32
    # statistics with mean 0 and variance 1 in every group and channel (slot 0 carries the sums), gamma 1, beta 0: shift is exactly 0
    stats = torch.zeros(3, LR.STAT_SLOTS, C, 2, dtype=torch.float64)
    stats[:, 0, :, 1] = count
    gamma, beta = torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    rm0, rv0 = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    g = LR.gen(0, 35, B)
    # every logit 0: each of the 2500 pixels of an image adds ln 2 exactly once, whatever its target
    what = "dec_last_fused_reduce zero weights B=%d" % B
    q3 = LR.eighths((3 * B, 25, 25, C), g)
    target = torch.randint(0, 5, (B, 1, 50, 50), generator=g).double() / 4
    out = _run_tail(h, B, q3, stats, gamma, beta, torch.zeros(C, 1, 4, 4, dtype=torch.float64), target, rm0, rv0)
    assert float(out["logits"].abs().max()) == 0.0
    want = torch.full((2,), B * 2500 * math.log(2.0), dtype=torch.float64)
    LR.gate_last_sums(out["sums"][:, :2].sum(0), want, want, what + " BCE sums")
    # one-hot activations around the seam and at the corners, at image 0 and at the last image of the last group; distinct small
    # integer weights per channel (|logit| <= 4 * 8 * Swish(1/2) = 10: no saturated sigmoid); one-hot targets at output rows 24 - 27
    what = "dec_last_fused_reduce one-hot B=%d" % B
    w9 = (((torch.arange(16)[None, :] * 5 + torch.arange(C)[:, None] * 3) % 17) - 8).double().reshape(C, 1, 4, 4)
    q3 = torch.zeros(3 * B, 25, 25, C, dtype=torch.float64)
    spots = ((0, 0, 0), (0, 24, 1), (24, 0, 2), (24, 24, 3), (11, 7, 4), (12, 7, 5), (13, 7, 6), (12, 24, 7), (13, 0, 8), (24, 12, 9),
             (11, 20, 10), (12, 21, 11), (13, 22, 12))
    for im in (0, 2 * B - 1):
        for (iy, ix, ch) in spots:
            q3[im, iy, ix, ch] = 0.5
    target = torch.zeros(B, 1, 50, 50, dtype=torch.float64)
    for im in (0, B - 1):
        for (oy, ox) in ((24, 3), (25, 14), (26, 15), (27, 40), (25, 0), (26, 49)):
            target[im, 0, oy, ox] = 1.0
    out = _run_tail(h, B, q3, stats, gamma, beta, w9, target, rm0, rv0)
    a64, _ = LR.ref_stage_fwd(q3[:2 * B], out["aff"][:2, :, 0], out["aff"][:2, :, 1], 2)
    lref = F.conv_transpose2d(LR._nchw(a64), w9, None, 2, 1)
    labs = F.conv_transpose2d(LR._nchw(a64.abs()), w9.abs(), None, 2, 1)
    _within(out["logits"], lref, (2.0 ** -8 + 128 * E) * labs, what + " logits")
    assert float(out["logits"].abs().max()) <= 14.0
    coef = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(B * 2500), dtype=torch.float32)
    p, t = torch.sigmoid(out["logits"]), target.repeat(2, 1, 1, 1)
    near = (p - t).abs() >= 0.04                                     # (the margin of the gate; saturated pixels are compared below through d3)
    dref = float(coef) * (p - t)
    LR.gate_last_layer(torch.where(near, out["dlogit"], dref), dref, LR.LAST_DLOGIT_MULT, what + " dlogit")
    ref, gate = _check_backward(B, q3, w9, out, what)               # d3 of every image, dW: element by element
    # a pixel owned twice or never shows in dW at full size: the one-hot channels carry every term of their rows
    assert bool((ref[:13].abs().amax((1, 2, 3)) > 64 * gate[:13].amax((1, 2, 3))).all())
