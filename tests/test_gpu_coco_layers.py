"""Layer-level tests of the COCO image half -- conv, data-gradient and weight-gradient kernels, the dense layers with their
permuted packings and the stand-alone passes -- against a float64 reference.

One launch of the COCO step is replayed through mmvae_coco_bench_layer -- which builds its arguments with the same tower_gemm /
tower_wgrad / pass builders of csrc/img_tower.h and layer_gemm / layer_wgrad of csrc/coco.hip the step calls -- on operands this test wrote into the workspace, and compared with
torch.nn.functional.conv2d / conv_transpose2d / linear / unfold / batch_norm-style float64 formulas and torch.autograd
(tests/layer_ref.py), never with another engine kernel.  Tiers and gates are those of tests/test_gpu_layers.py, derived there from
the number formats:
Tier A, torch.equal on ternary / integer operands (every product and partial sum an integer below 2^24; asserted on the reference);
Tier B, |got - ref| <= 2^-8 |ref| + 1e-5 |acc| per element for what passes through Swish / Swish' and a bf16 store, and
|got - ref| <= 2^-16 sum |terms| for the BatchNorm-backward, bias-gradient and statistics sums.
The BatchNorm passes use the gates of tests/test_gpu_celeba_layers_staged.py (layer_ref.gate_stage_fwd, the table gates counted at
the check, 2^-8 |ref| for dr on exact operands), the running statistics a count of fp32 roundings written at the check.

The last layer (dec_last_fwd): logits exact; behind them sit the hardware exp / rcp / log.  Gates: recon and dlogit a multiple of
one fp32 rounding 2^-24 of |ref|, the three BCE sums a multiple of 2^-16 sum |terms|.  Measured against the float64 reference
(MMVAE_TOL_REPORT=1, every batch and seed of this module), worst error in these units: recon 7.65, dlogit 6.81, sums 0.0049; the
multiples in layer_ref are recon 24, dlogit 24, sums 1 / 64 -- at most 4 times the measurement (the margin covers other seeds and
batches; the reference defines the centre).  p - t loses up to a factor p / |p - t| <= 0.73 / 0.044 of relative accuracy; the
targets (layer_ref.LAST_TARGETS) keep that factor bounded, so dlogit's ratio stays beside recon's.
Measured worst error / gate of the other gated checks in the same run: Swish copies (enc_conv1 a1, up au) 0.63, (fc1 ay1, fc2 ay2)
0.73; every data gradient through Swish' (conv layers, dec_last_dgrad_gemm, fc1 / fc2 / fc3_dgrad) 0.97; their sums d_red 0.016 /
0.003 / 0.020, d_colsum 0.017 / 0.020; BatchNorm forward: activated tensor 0.99, scale 0.16, shift 0.05, mean 0.02, rstd 0.17,
running mean 0.01, running variance 0.04; BatchNorm backward: dr, dgamma, dbeta 0.00 (exact operands).

Batches (layer_ref.BATCHES_COCO = 3, 4, 6, 8, 128, 256), read off the dispatch:
  csrc/convres.hip try_launch_convres: features.2 (64 -> 128, 16x16 -> 8x8) and hallucinate.6 (128 -> 64, 8x8 -> 16x16) match the
  G_ca_conv3 (NI = 2) and G_ca_convT2 (NI = 4) lines, forward and -- the other way round -- as data gradients; try_cr takes a launch
  when group_n % NI == 0 with group_n = B (the encoder runs 1 group, the decoder 3 groups of B).  B = 3 leaves both lines to the
  generic kernels, B = 6 leaves G_ca_convT2, B = 4 and 8 take both.  Every other conv layer has no image-resident kernel.
  csrc/wgrad_ring.hip try_wr, ca_conv3 (IB = 2): features.2 with nimg = B, hallucinate.6 with nimg = 3B: not at B = 3, else both.
  At B = 256 a ring workgroup runs 5.3 (encoder) / 12 (decoder) batches, more than SLOTS + 1 = 3 (derivation: docstring of
  tests/test_gpu_celeba_layers.py, same geometry).
  csrc/gemm.hip launch_gemm_gather, csrc/gemm_small.hip try_launch_gemm_small, csrc/plan_base.h gemm_of, with nclasses = 1 (forward
  form) or 4 (the stride parities of the class form), rows = rows per group and class:
    gemm_small takes a launch when tiles128 = ceil(rows / 128) groups nclasses ceil(N / 128) <= 128, FLOPs <= 8e9 and
    tiles22 = nclasses ceil(rows / 32) groups ceil(N / 32) <= 1536; KS = min(4, max(1, ceil(K / 64) / 2), max(1, 1024 / tiles22))
    rounded down to 4 / 2 / 1; the DGRAD form when the launch has a d-activation.
      B = 3 .. 8  : every conv and dense launch is gemm_small; KS 4 for the long-K layers, 2 for fc3 / fc3_dgrad / fc2_dgrad,
                    1 for enc_conv1, up and dec_last_dgrad_gemm; forward and DGRAD forms of KS 4, 2 and 1 all occur
      B = 128     : dec_convT1 (4 classes x 512 rows x 3 groups x N 256) has tiles22 = 4 * 16 * 3 * 8 = 1536, exactly on the boundary:
                    gemm_small KS 1; dec_convT2 (tiles22 = 4 * 64 * 3 * 4 = 3072) leaves for gemm_gather_kernel<8> without split-K
                    (gemm_of: 192 tiles > 128); enc_conv1 and dec_last_dgrad_gemm (N = 64) run gemm_gather_kernel<4>
      B = 256     : dec_convT1, dec_convT2, dec_convT2_dgrad on gemm_gather_kernel<8>; enc_conv3_dgrad (128 tiles, K 1024) and
                    dec_convT1_dgrad (96 tiles, K 4096) with split-K 2 and splitk_finish_kernel<8>
    gemm_rowtile needs 96 <= K <= 384 behind a refusal of gemm_small: no COCO launch has that at B <= 256 (fc3 / fc3_dgrad have the
    K, and at most 112 tiles22).
  csrc/gemm.hip launch_wgrad / wgrad_cfg: K = 48 (enc_conv1_wgrad, dec_last_wgrad) runs the 32 x 64 tile wgrad_kernel<2,1,1,4>,
  every other COCO weight gradient has N >= 128: the 128 x 128 tile wgrad_kernel<4,4,2,2>.
Not covered, because no COCO launch reaches it at B <= 256 with default knobs: gemm_rowtile_kernel<4 / 8 / 16>, gemm_gather_kernel<1>
and <2> (N <= 32), split-K on gemm_gather_kernel<4>, the 32 x 256 wgrad tile (N <= 32 with K > 64; the 64 x 256 tile
wgrad_kernel<4,4,1,4> only at latent sizes below 32, where classifier.6 has N = 2D <= 64: test_dense_layers_other_latent_sizes runs it
at D = 20), wgrad_multi_kernel (launch_wgrad_group: the caption half), split-K factors above 2 (dec_convT1_dgrad runs 3 and 4 between B = 159 and 224).  Only
through a knob: convres_alt, wr_pair, wgrad_atomic, MMVAE_SERIAL.  The generic kernels on features.2 / hallucinate.6 at even
batches run only with convres = 0; they are compared here all the same.

The image-side im2col (image -> patches1) is the kernel and the argument list of im2col_dlogit except the row count (B instead
of 3B), and its source is the caller's image pointer, not a workspace buffer: no replay name, test_im2col covers the kernel.

test_coverage reads the probe's records of every compared launch (launcher tag with the instantiation note, kernel text) and
prints which kernel took which layer at which batch (-s).

What stays with the whole-step tests: launch_latent3_fwd / bwd and batches above 256.  The caption half -- the bf16 persistent
kernels of csrc/coco_text_bf16.hip -- has its own float64 suite, tests/test_gpu_coco_text_modules.py (tests/test_gpu_text_modules.py
is MultiMNIST's: csrc/text.hip)."""
import re

import pytest
import torch
import torch.nn.functional as F

import layer_ref as LR
from layer_ref import LAYERS_COCO as LAYERS

pytestmark = pytest.mark.gpu

BATCHES = LR.BATCHES_COCO
HID1, HID2, FEAT = 1024, 256, 2048
_H = {}


def _harness(B, D=100):
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    if (B, D) not in _H:
        _H.clear()
        torch.cuda.empty_cache()
        _H[(B, D)] = LR.coco_harness(B, D)
    return _H[(B, D)]


def _seeds(B):
    """both seeds at the small batches, one at the large ones (their float64 references take a second each)"""
    return LR.SEEDS if B <= 8 else LR.SEEDS[:1]


CR_KNOBS = (dict(convres=1), dict(convres=0))
# ring off; ring on with the atomic epilogue; ring on with partial copies + reduce (csrc/wgrad_ring.hip try_wr: `atomic`)
WG_KNOBS = (dict(wgrad_ring=0, wr_atomic_kb=256), dict(wgrad_ring=1, wr_atomic_kb=4096), dict(wgrad_ring=1, wr_atomic_kb=0))
SIDE = {"enc": (("e0", 1, 128), ("e1", 1, 256), ("e2", 1, 512)), "dec": (("d0", 3, 256), ("d1", 3, 128), ("d2", 3, 64))}


# ------------------------------------------------------------------------------------------------ Tier A: conv layers
@pytest.mark.parametrize("name", list(LAYERS))
@pytest.mark.parametrize("B", BATCHES)
def test_forward_exact(B, name):
    h = _harness(B)
    L = LAYERS[name]
    ws, xs = [], []
    for seed in _seeds(B):
        x, w, _ = LR.layer_operands(name, L.gf * B, seed, LAYERS)
        LR.check_forward(h, L, name, x, w, CR_KNOBS, "%s B=%d seed %d" % (name, B, seed))
        ws.append(w)
        xs.append(x)
    if len(ws) == len(LR.SEEDS):
        LR.assert_operand_coverage(ws, xs)


def _distinct_ints(shape):
    """dense, distinct-looking integer weights, |w| <= 126: a slice landing in another tap's or channel's place cannot pass"""
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n, dtype=torch.int64) * 2654435761 >> 7) % 253 - 126).double().reshape(shape)


@pytest.mark.parametrize("name", list(LAYERS))
@pytest.mark.parametrize("B", [3, 8])
def test_weight_packing_one_hot(B, name):
    """Packing alone: on a single +1 at one (image, pixel, channel) a forward layer reproduces the weight slice of that channel,
    tap by tap, at the output pixels the geometry says.  The +1 sits at the four corners, an edge midpoint and the centre, in the
    first and last image and channel; on the 2x2 and 4x4 maps every position is a border position (padding 1)."""
    h = _harness(B)
    L = LAYERS[name]
    nimg, e, c = L.gf * B, L.ih - 1, L.ih // 2
    w = _distinct_ints(LR.weight_shape(L))
    for (im, y, xx, ch) in ((0, 0, 0, 0), (nimg - 1, e, e, L.cin - 1), (0, 0, e, L.cin - 1), (nimg - 1, e, 0, 0),
                            (nimg // 2, 0, c, L.cin // 2), (nimg - 1, c, c, 0), (0, c, c, L.cin - 1)):
        x = torch.zeros(nimg, L.ih, L.ih, L.cin, dtype=torch.float64)
        x[im, y, xx, ch] = 1.0
        LR.check_forward(h, L, name, x, w, CR_KNOBS, "%s B=%d one-hot %s" % (name, B, (im, y, xx, ch)))


@pytest.mark.parametrize("name", list(LAYERS))
@pytest.mark.parametrize("B", BATCHES)
def test_wgrad_exact(B, name):
    h = _harness(B)
    L = LAYERS[name]
    for seed in _seeds(B):
        x, _, dy = LR.layer_operands(name, L.gb * B, seed, LAYERS)
        h.put(L.x, x)
        h.put(L.dy, dy)
        LR.check_wgrad(h, name + "_wgrad", L.param, LR.ref_wgrad(L, x, dy), WG_KNOBS, "%s_wgrad B=%d seed %d" % (name, B, seed))


# ------------------------------------------------------------------------------------------------ Tier B: data gradients
def _poison_tables(h, side):
    """NaN into every (scale, shift) / (mean, rstd) table of one half and a pattern into its BatchNorm-backward sums
    -> {name: copy of the sums} to compare after the launch"""
    before = {}
    for tag, G, C in SIDE[side]:
        h.buf("aff_" + tag, G * C * 2, torch.float32).fill_(float("nan"))
        h.buf("mr_" + tag, G * C * 2, torch.float32).fill_(float("nan"))
        red = h.buf("red_" + tag, G * LR.STAT_SLOTS * C * 2, torch.float32)
        red.copy_(torch.arange(red.numel(), device=red.device, dtype=torch.float32) % 251 - 125)
        before["red_" + tag] = red.clone()
    return before


@pytest.mark.parametrize("name", list(LAYERS))
@pytest.mark.parametrize("B", BATCHES)
def test_dgrad_epilogue(B, name):
    """enc_conv2_dgrad and dec_convT1_dgrad end at a layer without BatchNorm (features.0 / upsample): their launch must neither read
    a table (the poisoned ones are NaN: the result would not pass its gate) nor write a sum (compared bit for bit afterwards)."""
    h = _harness(B)
    L = LAYERS[name]
    for seed in _seeds(B):
        _, w, dy = LR.layer_operands(name, L.gb * B, seed, LAYERS)
        g = LR.gen(seed, list(LAYERS).index(name), 4, L.gb * B)
        before = _poison_tables(h, name[:3]) if L.aff is None else {}
        LR.check_dgrad(h, L, name, dy, w, g, CR_KNOBS, "%s_dgrad B=%d seed %d" % (name, B, seed))
        for tag, G, C in (SIDE[name[:3]] if before else ()):
            after = h.buf("red_" + tag, G * LR.STAT_SLOTS * C * 2, torch.float32)
            assert torch.equal(after, before["red_" + tag]), "%s_dgrad wrote BatchNorm-backward sums into red_%s" % (name, tag)


# ------------------------------------------------------------------------------------------------ the 3-channel ends
@pytest.mark.parametrize("B", BATCHES)
def test_thin_layers_exact(B):
    """The 3-channel ends of the network as dense K = 48 GEMMs over an im2col buffer: enc_conv1 (raw output r1 exact, Swish copy a1
    gated), enc_conv1_wgrad, dec_last_wgrad (rows (n, iy, ix), 3 passes) and dec_last_dgrad_gemm with the Swish' /
    BatchNorm-backward epilogue of hallucinate.7.  The patch buffers are a real unfold of a ternary image / logit gradient in the
    column order of im2col_small_kernel, the references the conv2d / conv_transpose2d of coco/model.py:158,207 on that image."""
    h = _harness(B)
    f0, f9 = "image_encoder.features.0.weight", "image_decoder.hallucinate.9.weight"
    for seed in _seeds(B):
        g = LR.gen(seed, 9, B)
        img = LR.ternary((B, 3, 32, 32), 0.5, g)
        w0 = LR.ternary((64, 3, 4, 4), 0.5, g)
        d1 = LR.ternary((B, 16, 16, 64), 0.5, g)
        h.put("patches1", LR.patches_k4s2(img))
        ref = LR._nhwc(F.conv2d(img, w0, None, 2, 1))
        LR.assert_exact_regime(out=ref, what="enc_conv1")
        h.set_weight(f0, w0)
        h.zero("r1", ref.numel(), torch.bfloat16)
        h.zero("a1", ref.numel(), torch.bfloat16)
        launches = h.run("enc_conv1")
        got = h.get("r1", ref.shape).double().cpu()
        assert torch.equal(got, ref), (B, seed, launches, LR.describe_mismatch(got, ref))
        LR.gate_elements(h.get("a1", ref.shape), ref * torch.sigmoid(ref), ref, "enc_conv1 a1 B=%d seed %d" % (B, seed))
        wz = torch.zeros(64, 3, 4, 4, dtype=torch.float64, requires_grad=True)
        F.conv2d(img, wz, None, 2, 1).backward(LR._nchw(d1))
        h.put("d1e", d1)
        # (the K = 48 ends match no ring geometry -- csrc/wgrad_ring_geos.h -- so the partial-copies knob set would repeat the
        #  same launch: ring off / on only)
        LR.check_wgrad(h, "enc_conv1_wgrad", f0, wz.grad, WG_KNOBS[:2], "enc_conv1_wgrad B=%d seed %d" % (B, seed))
        # last transposed conv (64 -> 3 channels): dW from its activated input aq3 and im2col(dlogit), 3 passes
        dl = LR.ternary((3 * B, 3, 32, 32), 0.25, g)
        a3 = LR.ternary((3 * B, 16, 16, 64), 0.25, g)
        w9 = torch.zeros(64, 3, 4, 4, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(LR._nchw(a3), w9, None, 2, 1).backward(dl)
        h.put("patches4", LR.patches_k4s2(dl))
        h.put("aq3", a3)
        LR.check_wgrad(h, "dec_last_wgrad", f9, w9.grad, WG_KNOBS[:2], "dec_last_wgrad B=%d seed %d" % (B, seed))
        # its input gradient with the epilogue of hallucinate.7
        dl = LR.ternary((3 * B, 3, 32, 32), 0.5, g)
        w9 = LR.ternary((64, 3, 4, 4), 0.5, g)
        x = torch.zeros(3 * B, 64, 16, 16, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(x, w9, None, 2, 1).backward(dl)
        acc = LR._nhwc(x.grad)
        assert bool((acc == acc.round()).all()) and float(acc.abs().max()) <= 256
        r = LR.eighths(acc.shape, g)
        aff, mr = LR.dyadic_tables(3, 64, g)
        v, red, red_abs = LR.ref_dgrad_epilogue(acc, r, aff, mr, 3)
        h.set_weight(f9, w9)
        h.put("patches4", LR.patches_k4s2(dl))
        h.put("q3", r)
        h.put("aff_d2", aff, torch.float32)
        h.put("mr_d2", mr, torch.float32)
        h.zero("d3", acc.numel(), torch.bfloat16)
        h.zero("red_d2", 3 * LR.STAT_SLOTS * 64 * 2, torch.float32)
        launches = h.run("dec_last_dgrad_gemm")
        what = "dec_last_dgrad_gemm B=%d seed %d" % (B, seed)
        LR.gate_elements(h.get("d3", acc.shape), v, acc, what, launches)
        LR.gate_sums(h.stats("red_d2", 3, 64), red, red_abs, what + " d_red", launches)


@pytest.mark.parametrize("B", BATCHES)
def test_im2col(B):
    """im2col_dlogit: dlogit [3B][3][32][32] fp32 -> patches4 [3B * 256][48] bf16 against F.unfold on values exact in bf16 -- the
    zero columns of the windows that leave the image included, and the row stride 48 (a wrong leading dimension shifts every row)."""
    h = _harness(B)
    g = LR.gen(0, 14, B)
    dl = LR.eighths((3 * B, 3, 32, 32), g)
    dl[dl == 0] = 0.125                       # no zeros inside the image: a padding column is the only way to a zero
    want = LR.patches_k4s2(dl)
    assert float((want == 0).double().mean()) > 0.05
    h.put("dlogit", dl, torch.float32)
    h.buf("patches4", want.numel(), torch.bfloat16).fill_(7.0)
    h.run("im2col_dlogit")
    got = h.get("patches4", want.shape).double().cpu()
    bad = got != want
    assert not bool(bad.any()), ("im2col_dlogit B=%d" % B, "%d of %d elements differ; first [row, column] %s got %s want %s" % (
        int(bad.sum()), bad.numel(), torch.nonzero(bad)[:6].tolist(), got[bad][:6].tolist(), want[bad][:6].tolist()))


# ------------------------------------------------------------------------------------------------ dense layers
DROP_SCALE = 1.0 / (1.0 - 0.1)      # nn.Dropout(0.1) keep scale (coco/model.py:172,175; the engine's is the fp32 rounding of it)
C0, C3, C6, UP = "image_encoder.classifier.0.", "image_encoder.classifier.3.", "image_encoder.classifier.6.", "image_decoder.upsample.0."


def _swish(x):
    return x * torch.sigmoid(x)


def _flat_nchw(t):
    """[n][2][2][512] NHWC -> torch's flatten of (512, 2, 2): column c * 4 + y * 2 + x"""
    return LR._nchw(t).reshape(t.shape[0], FEAT)


def _map_nhwc(t):
    """[n][2048] in torch's order c * 4 + s -> the engine's NHWC column s * 512 + c, as [n][2][2][512]"""
    return LR._nhwc(t.reshape(t.shape[0], 512, 2, 2))


def _z_rows(z, D):
    """z_bf operand [rows][ldz]: the latent, a 1.0 in column D (the bias rides in the packed weights), zero padding"""
    out = torch.zeros(z.shape[0], (D + 1 + 7) // 8 * 8, dtype=torch.float64)
    out[:, :D] = z
    out[:, D] = 1.0
    return out


def _only_bias(h, pname, n, what):
    """the flat gradients hold nothing outside the n elements of the named bias"""
    boff, _, _ = h.param_range(pname)
    others = h.st.grads.clone()
    others[boff:boff + n] = 0
    assert float(others.abs().max()) == 0.0, what + " wrote a gradient other than " + pname
    return boff


def _check_fc3(h, B, D, g, tag):
    """classifier.6 (Linear(256, 2D), fp32 output), its weight gradient and its data gradient with Swish'(y2), keep mask m2 and the
    column sums that are classifier.3's bias gradient"""
    rows = 2 * B
    tern = lambda shape, d=0.5: LR.ternary(shape, d, g)
    W6, b6 = tern((2 * D, HID2), 0.25), torch.randint(-2, 3, (2 * D,), generator=g).double()
    h.set_weight(C6 + "weight", W6)
    h.set_weight(C6 + "bias", b6)
    m2 = (torch.rand((rows, HID2), generator=g) < 0.9).to(torch.uint8)
    h.put("m2", m2, torch.uint8)
    ay2 = tern((rows, HID2))
    h.put("ay2", ay2)
    h.zero("encout", rows * 2 * D, torch.float32)
    h.run("fc3")
    LR.check_exact(h.get("encout", (rows, 2 * D), torch.float32), F.linear(ay2, W6, b6), "fc3 " + tag, limit=2 ** 24)
    de = tern((rows, 2 * D))
    h.put("d_encout", de)
    LR.check_wgrad(h, "fc3_wgrad", C6 + "weight", de.t() @ ay2, WG_KNOBS[:1], "fc3_wgrad " + tag)
    r2 = LR.eighths((rows, HID2), g)
    h.put("y2", r2)
    acc = de @ W6
    for mask in (0, 1):
        v = acc * LR.dswish(r2) * (m2 * DROP_SCALE if mask else 1.0)
        h.zero("dy2", rows * HID2, torch.bfloat16)
        h.st.grads.zero_()              # d_colsum adds into the flat gradients at classifier.3.bias, as in the step
        h.run("fc3_dgrad", coco_layer_mask=mask)
        LR.gate_elements(h.get("dy2", (rows, HID2)), v, acc, "fc3_dgrad mask %d %s" % (mask, tag))
        boff = _only_bias(h, C3 + "bias", HID2, "fc3_dgrad")
        LR.gate_sums(h.st.grads[boff:boff + HID2], v.sum(0), v.abs().sum(0), "fc3_dgrad d_colsum mask %d %s" % (mask, tag))


def _check_up(h, B, D, g, tag):
    """upsample.0 (Linear(D, 2048) viewed as 512x2x2, written as NHWC, bias folded into the packed weights): forward, weight +
    bias gradient, dz -- all exact"""
    tern = lambda shape, d=0.5: LR.ternary(shape, d, g)
    Wu, bu = tern((FEAT, D), 0.25), torch.randint(-2, 3, (FEAT,), generator=g).double()
    h.set_weight(UP + "weight", Wu)
    h.set_weight(UP + "bias", bu)
    z = tern((3 * B, D))
    h.put("z_bf", _z_rows(z, D))
    u = _map_nhwc(F.linear(z, Wu, bu)).reshape(3 * B, FEAT)
    h.zero("u", 3 * B * FEAT, torch.bfloat16)
    h.zero("au", 3 * B * FEAT, torch.bfloat16)
    h.run("up")
    LR.check_exact(h.get("u", (3 * B, FEAT)), u, "up u " + tag)
    LR.gate_elements(h.get("au", (3 * B, FEAT)), _swish(u), u, "up au " + tag)
    du = tern((3 * B, 2, 2, 512), 0.25)
    h.put("du", du)
    duf = _flat_nchw(du)
    LR.check_wgrad(h, "up_wgrad", UP + "weight", duf.t() @ z, WG_KNOBS[:1], "up_wgrad " + tag, also={UP + "bias": duf.sum(0)})
    h.zero("dz_img", 3 * B * D, torch.float32)
    h.run("up_dgrad")
    LR.check_exact(h.get("dz_img", (3 * B, D), torch.float32), duf @ Wu, "up_dgrad " + tag, limit=2 ** 24)


@pytest.mark.parametrize("B", BATCHES)
def test_dense_layers(B):
    """classifier.0 (coco/model.py:170: Linear(2048, 1024) on the NCHW flatten c * 4 + y * 2 + x of the 512x2x2 map, held here as
    NHWC and shared by the 2 dropout variants: a_bcast_n), classifier.3 (bias, Swish, mask m2), classifier.6 (fp32 output) and
    upsample.0, each with its weight and data gradient.  Integer weights, biases and operands make the pre-activations, the weight
    gradients, encout and dz exact; the Swish / keep-mask copies and the gradients through Swish' take the per-element gate, the
    BatchNorm-backward / bias sums the 2^-16 gate.  The keep masks are the test's."""
    h = _harness(B)
    rows, D = 2 * B, 100
    for seed in _seeds(B):
        g = LR.gen(seed, 11, B)
        tern = lambda shape, d=0.5: LR.ternary(shape, d, g)
        ibias = lambda n: torch.randint(-2, 3, (n,), generator=g).double()
        W1, W3 = tern((HID1, FEAT), 0.25), tern((HID2, HID1), 0.25)
        b1, b3 = ibias(HID1), ibias(HID2)
        for n, t in ((C0 + "weight", W1), (C0 + "bias", b1), (C3 + "weight", W3), (C3 + "bias", b3)):
            h.set_weight(n, t)
        m1 = (torch.rand((rows, HID1), generator=g) < 0.9).to(torch.uint8)
        m2 = (torch.rand((rows, HID2), generator=g) < 0.9).to(torch.uint8)
        h.put("m1", m1, torch.uint8)
        h.put("m2", m2, torch.uint8)
        tag = "B=%d seed %d" % (B, seed)

        # ---- classifier.0 / classifier.3 forward: row r of the 2B rows reads image r % B
        a4 = tern((B, 2, 2, 512), 0.25)
        h.put("a4", a4)
        x1 = _flat_nchw(a4).repeat(2, 1)
        y1 = F.linear(x1, W1, b1)
        ay1 = tern((rows, HID1), 0.25)
        y2 = F.linear(ay1, W3, b3)
        for mask in (0, 1):
            for nm, n in (("y1", HID1), ("ay1", HID1), ("y2", HID2), ("ay2", HID2)):
                h.zero(nm, rows * n, torch.bfloat16)
            h.run("fc1", coco_layer_mask=mask)
            LR.check_exact(h.get("y1", (rows, HID1)), y1, "fc1 y1 mask %d %s" % (mask, tag))
            LR.gate_elements(h.get("ay1", (rows, HID1)), _swish(y1) * (m1 * DROP_SCALE if mask else 1.0), y1, "fc1 ay1 mask %d %s" % (mask, tag))
            h.put("ay1", ay1)
            h.run("fc2", coco_layer_mask=mask)
            LR.check_exact(h.get("y2", (rows, HID2)), y2, "fc2 y2 mask %d %s" % (mask, tag))
            LR.gate_elements(h.get("ay2", (rows, HID2)), _swish(y2) * (m2 * DROP_SCALE if mask else 1.0), y2, "fc2 ay2 mask %d %s" % (mask, tag))

        # ---- classifier.6 and its gradients
        _check_fc3(h, B, D, g, tag)
        h.put("m2", m2, torch.uint8)

        # ---- classifier.3 gradients: dy1 = (dy2 W3) * Swish'(y1) [* keep / 0.9], column sums = classifier.0's bias gradient
        dy2, r1 = tern((rows, HID2)), LR.eighths((rows, HID1), g)
        h.put("dy2", dy2)
        h.put("ay1", ay1)
        LR.check_wgrad(h, "fc2_wgrad", C3 + "weight", dy2.t() @ ay1, WG_KNOBS[:1], "fc2_wgrad " + tag)
        h.put("y1", r1)
        acc = dy2 @ W3
        for mask in (0, 1):
            v = acc * LR.dswish(r1) * (m1 * DROP_SCALE if mask else 1.0)
            h.zero("dy1", rows * HID1, torch.bfloat16)
            h.st.grads.zero_()
            h.run("fc2_dgrad", coco_layer_mask=mask)
            LR.gate_elements(h.get("dy1", (rows, HID1)), v, acc, "fc2_dgrad mask %d %s" % (mask, tag))
            boff = _only_bias(h, C0 + "bias", HID1, "fc2_dgrad")
            LR.gate_sums(h.st.grads[boff:boff + HID1], v.sum(0), v.abs().sum(0), "fc2_dgrad d_colsum mask %d %s" % (mask, tag))

        # ---- classifier.0 gradients.  dy1 dense, and with the zeros a keep mask upstream leaves in it (the step with dropout)
        for masked in (0, 1):
            dy1 = tern((rows, HID1)) * (m1.double() if masked else 1.0)
            h.put("dy1", dy1)
            wz = torch.zeros(HID1, FEAT, dtype=torch.float64, requires_grad=True)
            F.linear(x1, wz).backward(dy1)
            LR.check_wgrad(h, "fc1_wgrad", C0 + "weight", wz.grad, WG_KNOBS[:1], "fc1_wgrad masked %d %s" % (masked, tag))
            # db4[n][s * 512 + c] = (dy1 W1)[n][c * 4 + s] * Swish'(scale_c * r4[n % B] + shift_c); sums per channel c = column % 512
            acc = _map_nhwc(dy1 @ W1)
            r4 = LR.eighths((B, 2, 2, 512), g)
            aff, mr = LR.dyadic_tables(1, 512, g)
            v, red, red_abs = LR.ref_dgrad_epilogue(acc, r4.repeat(2, 1, 1, 1), aff, mr, 1)
            h.put("r4", r4)
            h.put("aff_e2", aff, torch.float32)
            h.put("mr_e2", mr, torch.float32)
            h.zero("db4", rows * FEAT, torch.bfloat16)
            h.zero("red_e2", LR.STAT_SLOTS * 512 * 2, torch.float32)
            launches = h.run("fc1_dgrad")
            LR.gate_elements(h.get("db4", acc.shape), v, acc, "fc1_dgrad masked %d %s" % (masked, tag), launches)
            LR.gate_sums(h.stats("red_e2", 1, 512), red, red_abs, "fc1_dgrad d_red masked %d %s" % (masked, tag), launches)

        # ---- upsample.0
        _check_up(h, B, D, g, tag)


@pytest.mark.parametrize("B", [3, 8])
@pytest.mark.parametrize("D", [20, 64])
def test_dense_layers_other_latent_sizes(D, B):
    """The layers whose shape depends on the latent size, at D = 20 and 64 (ldz = round_up(D + 1, 8) = 24 / 72; at D = 64, D + 1
    crosses a multiple of 64 and the packed K of upsample.0 doubles): fc3, fc3_wgrad, fc3_dgrad, up, up_wgrad, up_dgrad."""
    h = _harness(B, D)
    g = LR.gen(0, 15, B, D)
    tag = "D=%d B=%d" % (D, B)
    _check_fc3(h, B, D, g, tag)
    _check_up(h, B, D, g, tag)


@pytest.mark.parametrize("B", [3, 8])
def test_dense_packing_one_hot(B):
    """The permuted packings of classifier.0 and upsample.0 (csrc/coco.hip build(): PackDesc TW / C / s_ty / s_tx / s_c, NL / s_nhi
    / s_nlo, b_nhi / b_nlo) and the plain ones of classifier.3 / classifier.6 with dense, distinct integer weights.
    fc1: a single +1 at (row, y, x, c) of the 2x2x512 map gives column c * 4 + y * 2 + x of classifier.0.weight plus the bias, in
    both row blocks of the broadcast, and the bias alone in every other row.
    fc2 / fc3: a single +1 at (row, k) gives column k of the weight plus the bias in that row.
    up: a single +1 at z_bf[row][k] gives upsample.0.weight[c * 4 + s][k] plus bias[c * 4 + s] at NHWC column s * 512 + c."""
    h = _harness(B)
    rows, D = 2 * B, 100
    W1, W3, W6, Wu = _distinct_ints((HID1, FEAT)), _distinct_ints((HID2, HID1)), _distinct_ints((2 * D, HID2)), _distinct_ints((FEAT, D))
    b1, b3 = (torch.arange(HID1) % 5 - 2).double(), (torch.arange(HID2) % 3 - 1).double()
    b6, bu = (torch.arange(2 * D) % 9 - 4).double(), (torch.arange(FEAT) % 7 - 3).double()
    for n, t in ((C0 + "weight", W1), (C0 + "bias", b1), (C3 + "weight", W3), (C3 + "bias", b3), (C6 + "weight", W6), (C6 + "bias", b6),
                 (UP + "weight", Wu), (UP + "bias", bu)):
        h.set_weight(n, t)
    for (n, y, x, c) in ((0, 0, 0, 0), (B - 1, 1, 1, 511), (B // 2, 0, 1, 256), (0, 1, 0, 7), (B - 1, 1, 0, 1)):
        a4 = torch.zeros(B, 2, 2, 512, dtype=torch.float64)
        a4[n, y, x, c] = 1.0
        want = b1.repeat(rows, 1)
        want[n] += W1[:, c * 4 + y * 2 + x]
        want[n + B] += W1[:, c * 4 + y * 2 + x]
        assert torch.equal(want, F.linear(_flat_nchw(a4).repeat(2, 1), W1, b1))
        h.put("a4", a4)
        h.zero("y1", rows * HID1, torch.bfloat16)
        h.run("fc1")
        LR.check_exact(h.get("y1", (rows, HID1)), want, "fc1 one-hot %s B=%d" % ((n, y, x, c), B))
    for (row, k) in ((0, 0), (rows - 1, HID1 - 1), (B, 513)):
        x = torch.zeros(rows, HID1, dtype=torch.float64)
        x[row, k] = 1.0
        h.put("ay1", x)
        h.zero("y2", rows * HID2, torch.bfloat16)
        h.run("fc2")
        LR.check_exact(h.get("y2", (rows, HID2)), F.linear(x, W3, b3), "fc2 one-hot %s B=%d" % ((row, k), B))
    for (row, k) in ((0, 0), (rows - 1, HID2 - 1), (B, 129)):
        x = torch.zeros(rows, HID2, dtype=torch.float64)
        x[row, k] = 1.0
        h.put("ay2", x)
        h.zero("encout", rows * 2 * D, torch.float32)
        h.run("fc3")
        LR.check_exact(h.get("encout", (rows, 2 * D), torch.float32), F.linear(x, W6, b6), "fc3 one-hot %s B=%d" % ((row, k), B), limit=2 ** 24)
    for (row, k) in ((0, 0), (3 * B - 1, D - 1), (B, 37), (2 * B - 1, 64)):
        z = torch.zeros(3 * B, D, dtype=torch.float64)
        z[row, k] = 1.0
        want = bu.repeat(3 * B, 1)
        want[row] += Wu[:, k]
        assert torch.equal(want, F.linear(z, Wu, bu))
        want = _map_nhwc(want).reshape(3 * B, FEAT)
        s, c = 3, 200
        assert float(want[row, s * 512 + c]) == float(Wu[c * 4 + s, k] + bu[c * 4 + s])
        h.put("z_bf", _z_rows(z, D))
        h.zero("u", 3 * B * FEAT, torch.bfloat16)
        h.run("up")
        LR.check_exact(h.get("u", (3 * B, FEAT)), want, "up one-hot %s B=%d" % ((row, k), B))


# ------------------------------------------------------------------------------------------------ stand-alone passes
# pass name -> (conv layer whose raw output it normalises, BatchNorm module, activated tensor, table suffix, updates per group)
BN_PASSES = {
    "enc_bn2": ("enc_conv2", "image_encoder.features.3", "a2", "e0", 2), "enc_bn3": ("enc_conv3", "image_encoder.features.6", "a3", "e1", 2),
    "enc_bn4": ("enc_conv4", "image_encoder.features.9", "a4", "e2", 2), "dec_bn1": ("dec_convT1", "image_decoder.hallucinate.1", "aq1", "d0", 1),
    "dec_bn2": ("dec_convT2", "image_decoder.hallucinate.4", "aq2", "d1", 1), "dec_bn3": ("dec_convT3", "image_decoder.hallucinate.7", "aq3", "d2", 1),
}


def _within(got, ref, gate, what):
    got = got.double().cpu()
    err = (got - ref).abs()
    if LR.REPORT:
        print("PASS %s: worst err/gate %.3f" % (what, float((err / gate.clamp_min(1e-30)).max())))
    bad = ~(err <= gate)
    assert not bool(bad.any()), (what, "%d of %d outside the gate; first %s got %s want %s gate %s" % (
        int(bad.sum()), bad.numel(), torch.nonzero(bad)[:6].tolist(), got[bad][:6].tolist(), ref[bad][:6].tolist(), gate[bad][:6].tolist()))


def _bn_slot(h, bn):
    for i, (n, C, off) in enumerate(h.st.bn_table):
        if n == bn:
            return i, C, off
    raise KeyError(bn)


@pytest.mark.parametrize("name", list(BN_PASSES))
@pytest.mark.parametrize("B", BATCHES)
def test_bn_forward(B, name):
    """launch_bn_act in training mode: from the column statistics the test wrote (exact in fp32) the (scale, shift) / (mean, rstd)
    tables, Swish(BatchNorm(raw)) and the running mean / variance / batch counter after the default step's updates (encoder: 2
    per step -- the features are shared by two passes --, decoder: 1 per group, groups in pass order)."""
    h = _harness(B)
    lname, bn, act, tb, updates = BN_PASSES[name]
    L = LAYERS[lname]
    G, C, nimg, count = L.gf, L.cout, L.gf * B, B * L.oh * L.oh
    g = LR.gen(0, list(BN_PASSES).index(name), 16, nimg)
    r = LR.eighths((nimg, L.oh, L.oh, C), g)
    gamma = torch.tensor([1.0, 2.0, -1.0])[torch.randint(0, 3, (C,), generator=g)].double()
    beta = torch.randint(-1, 2, (C,), generator=g).double()
    rm0 = torch.randint(-4, 5, (C,), generator=g).double() / 4
    rv0 = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)].double()
    stats = LR.slot_stats_any(r, G)
    assert torch.equal(stats.float().double(), stats)
    idx, Cb, soff = _bn_slot(h, bn)
    assert Cb == C
    what = "%s B=%d" % (name, B)
    h.set_weight(bn + ".weight", gamma)
    h.set_weight(bn + ".bias", beta)
    h.st.bn_stats[soff:soff + C] = rm0.float().to(h.dev)
    h.st.bn_stats[soff + C:soff + 2 * C] = rv0.float().to(h.dev)
    h.st.bn_nbt[idx] = 5
    h.put(L.out, r)
    h.put("st_" + tb, stats, torch.float32)
    h.zero(act, r.numel(), torch.bfloat16)
    h.zero("aff_" + tb, G * C * 2, torch.float32)
    h.zero("mr_" + tb, G * C * 2, torch.float32)
    h.run(name)
    scale, shift, mean, rstd = LR.ref_bn_tables(stats, count, gamma, beta)
    aff = h.get("aff_" + tb, (G, C, 2), torch.float32)
    mr = h.get("mr_" + tb, (G, C, 2), torch.float32)
    # fp32 roundings of csrc/bn_dev.h bn_channel_tables, counted in tests/test_gpu_celeba_layers_staged.py: mean 16 (of 4), rstd 11,
    # scale 12, shift 16 of (4 + |mean|) |scale| + |beta|
    e = LR.EPS32
    _within(aff[..., 0], scale, 12 * e * scale.abs(), what + " scale")
    _within(aff[..., 1], shift, 16 * e * ((mean.abs() + 4) * scale.abs() + beta.abs()[None]), what + " shift")
    _within(mr[..., 0], mean, 16 * e * 4 * torch.ones_like(mean), what + " mean")
    _within(mr[..., 1], rstd, 11 * e * rstd, what + " rstd")
    a_ref, _ = LR.ref_stage_fwd(r, scale, shift, G)
    _within(h.get(act, r.shape), a_ref, LR.gate_stage_fwd(r, scale, shift, mean, beta, a_ref, G), what + " activated")
    # running statistics after n = G * updates momentum steps: the mean's 16 roundings (of 4), the variance's 20 and 2 more of
    # the unbiased factor, then per step 2 products, 1 addition and the two rounded constants 0.1f / (1.f - 0.1f): 5 per step
    n = G * updates
    rm, rv, unb = LR.ref_bn_running(stats, count, rm0, rv0, updates)
    _within(h.st.bn_stats[soff:soff + C], rm, (16 + 5 * n) * e * 4 * torch.ones_like(rm), what + " running_mean")
    _within(h.st.bn_stats[soff + C:soff + 2 * C], rv, (22 + 5 * n) * e * torch.maximum(unb, rv0), what + " running_var")
    assert int(h.st.bn_nbt[idx]) == 5 + n, (what, int(h.st.bn_nbt[idx]))


@pytest.mark.parametrize("name", list(BN_PASSES))
@pytest.mark.parametrize("B", BATCHES)
def test_bn_backward(B, name):
    """launch_bn_bwd_apply: dr = gamma rstd (db - m1 - xhat m2) from the sums in red_*, dgamma / dbeta added to the flat gradients.
    The encoder passes write dr into the buffer db came from (d2e, d3e) except enc_bn4_bwd, which sums the gradients of the two
    classifier variants -- db = first B rows of db4, db2 = the next B rows, two different ternary draws -- into dr4."""
    h = _harness(B)
    lname, bn, _, tb, _ = BN_PASSES[name]
    L = LAYERS[lname]
    G, C, nimg, count = L.gb, L.cout, L.gb * B, B * L.oh * L.oh
    g = LR.gen(0, list(BN_PASSES).index(name), 17, nimg)
    db, r, red, mr, gamma = LR.staged_bwd_operands(L, nimg, G, count, g, integer_slots=False)
    assert torch.equal(red.float().double(), red)
    db2 = LR.ternary(db.shape, LR.G_DENSITY, g) if name == "enc_bn4" else None
    total = db if db2 is None else db + db2
    dr, dgamma, dbeta, mag_g, mag_b = LR.ref_bn_backward(total, r, red, mr, gamma, count, G)
    if count & (count - 1) == 0:
        assert torch.equal(dr.float().double(), dr)
    goff, _, _ = h.param_range(bn + ".weight")
    boff, _, _ = h.param_range(bn + ".bias")
    what = "%s_bwd B=%d" % (name, B)
    h.set_weight(bn + ".weight", gamma)
    if name == "enc_bn4":
        assert bool((db != db2).any())
        h.put("db4", torch.cat([db.reshape(B, -1), db2.reshape(B, -1)]))
        h.zero("dr4", dr.numel(), torch.bfloat16)
        out = "dr4"
    else:
        h.put(L.dy, db)
        out = L.dy
    h.put(L.out, r)
    h.put("red_" + tb, red, torch.float32)
    h.put("mr_" + tb, mr, torch.float32)
    h.st.grads.zero_()
    h.run(name + "_bwd")
    _within(h.get(out, dr.shape), dr, LR.gate_bn_backward(total, r, red, mr, gamma, count, G, dr), what + " dr")
    LR.gate_sums(h.st.grads[goff:goff + C], dgamma, mag_g, what + " dgamma")
    LR.gate_sums(h.st.grads[boff:boff + C], dbeta, mag_b, what + " dbeta")
    others = h.st.grads.clone()
    others[goff:goff + C] = 0
    others[boff:boff + C] = 0
    assert float(others.abs().max()) == 0.0, what + " wrote another parameter's gradient"


@pytest.mark.parametrize("B", BATCHES)
def test_dec_last_fwd(B):
    """launch_convt_last_fwd with 3 output channels, 3 passes: logits exact against conv_transpose2d (ternary activations and
    weights); recon, dlogit = coef[g] (sigmoid - target) with the loss weights (1, 1/2, 0) / (B * 3072) and the three BCE sums within
    the measured gates of layer_ref (module docstring).  The target sits in tmp_f32, logits and recon in the weight-gradient slab."""
    h = _harness(B)
    n3 = 3 * B * 3072
    for seed in _seeds(B):
        g = LR.gen(seed, 21, B)
        a3 = LR.ternary((3 * B, 16, 16, 64), LR.LAST_X_DENSITY, g)
        w9 = LR.ternary((64, 3, 4, 4), LR.LAST_W_DENSITY, g)
        target = torch.tensor(LR.LAST_TARGETS, dtype=torch.float64)[torch.randint(0, len(LR.LAST_TARGETS), (B, 3, 32, 32), generator=g)]
        coef = LR.last_layer_coef(B)
        logits, recon, dlogit, sums, mags = LR.ref_dec_last(a3, w9, target, coef)
        LR.assert_last_layer_regime(logits)
        h.set_weight("image_decoder.hallucinate.9.weight", w9)
        h.put("aq3", a3)
        h.put("tmp_f32", target, torch.float32)
        h.zero("slab", 2 * n3, torch.float32)
        h.buf("dlogit", n3, torch.float32).fill_(7.0)
        h.zero("sums", 16 * LR.LOSS_SLOTS, torch.float32)
        h.run("dec_last_fwd")
        what = "dec_last_fwd B=%d seed %d" % (B, seed)
        both = h.get("slab", (2,) + tuple(logits.shape), torch.float32)
        LR.check_exact(both[0], logits, what + " logits")
        LR.gate_last_layer(both[1], recon, LR.LAST_RECON_MULT, what + " recon")
        got_dl = h.get("dlogit", logits.shape, torch.float32)
        assert float(got_dl[2 * B:].abs().max()) == 0.0, what + ": the pass with loss weight 0 has a gradient"
        LR.gate_last_layer(got_dl, dlogit, LR.LAST_DLOGIT_MULT, what + " dlogit")
        table = h.get("sums", (LR.LOSS_SLOTS, 16), torch.float32).double().cpu()
        LR.gate_last_sums(table[:, :3].sum(0), sums, mags, what + " BCE sums")
        assert float(table[:, 3:].abs().max()) == 0.0, what + " wrote a loss column other than its three"


# ------------------------------------------------------------------------------------------------ which kernels ran
# The probe reports the launcher's tag -- "convres form<F> <C>><N> <AH>x<AW>><OH>x<OW> k<K> s<S> fwd|dgrad tr<kind> img<nimg>", or
# "gemm ..." / "wgrad ..." followed by the note of the generic launcher that took it: "small<2,2,KS,fwd|dgrad>", "gather<NT> ksplit<n>",
# "rowtile<NTW>", "wgrad<NWT,KWT,WN,WK> slab|atomic" -- and the kernel text of the launch macro.
CR_LINES = (
    ("G_ca_conv3 <2, 0, 8, 4>", "form0 64>128 16x16>8x8 k4 s2", 2),
    ("G_ca_convT2 <4, 0, 8, 2>", "form1 128>64 8x8>16x16 k4 s2", 4),
)
# try_cr line of each conv launch (csrc/convres.hip); None: no image-resident kernel for the geometry
CR_OF = {
    "enc_conv2": 0, "dec_convT3": 1, "enc_conv2_dgrad": 1, "dec_convT3_dgrad": 0,
    "enc_conv3": None, "enc_conv4": None, "dec_convT1": None, "dec_convT2": None,
    "enc_conv3_dgrad": None, "enc_conv4_dgrad": None, "dec_convT1_dgrad": None, "dec_convT2_dgrad": None,
}
RING_LAYERS = ("enc_conv2_wgrad", "dec_convT3_wgrad")        # ca_conv3 of WGRAD_RING_GEOS (csrc/wgrad_ring_geos.h), IB = 2
# every generic instantiation a COCO launch reaches at B <= 256 with default knobs (module docstring)
GENERIC = ["small<2,2,%d,%s>" % (ks, f) for ks in (4, 2, 1) for f in ("fwd", "dgrad")] + [
    "gather<4> ksplit1", "gather<8> ksplit1", "gather<8> ksplit2", "splitk_finish_kernel", "wgrad<2,1,1,4>", "wgrad<4,4,2,2>"]


def test_coverage():
    """Over the launches the tests above compared (run the whole module: this test reads their records): both G_ca_* lines ran as
    forward and as data gradient, each of the four launches has its generic fallback, the ca_conv3 ring ran in both epilogue modes
    on both sides and at the large batch, every generic instantiation of the docstring ran in a launch with default knobs, and no
    image-resident / ring kernel ran with its knob off."""
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from multimodal_vae_amd._lib import knob_default
    recs = LR.RECORDS_COCO
    assert {r[0] for r in recs} >= set(BATCHES), "run the whole module: the compared launches of every batch size are the input of this test"
    hit, fallback, ring_hit, generic, table = {}, {}, {}, {}, {}
    for B, layer, knobs, launches in recs:
        cr = [t for t, k in launches if t.startswith("convres ")]
        ring = [k for t, k in launches if "wgrad_ring_kernel" in k]
        reduce_ = [k for t, k in launches if "wgrad_ring_reduce_kernel" in k]
        # knobs that bear on this launch: the ring knobs on the ring geometry only, convres where a try_cr line exists
        relevant = {k: v for k, v in knobs.items() if k != "coco_layer_mask"}
        if layer not in RING_LAYERS:
            relevant.pop("wgrad_ring", None)
            relevant.pop("wr_atomic_kb", None)
        if CR_OF.get(layer) is None:
            relevant.pop("convres", None)
        default = all(knob_default(k) == v for k, v in relevant.items())
        for t, k in launches:
            note = re.split(r" img\d+ ?", t, 1)[1] if t.startswith(("gemm ", "wgrad ")) and " img" in t else ""
            if t.startswith("convres "):
                what = "convres " + [ln for ln, geo, _ in CR_LINES if geo in t][0]
            else:
                what = note or k.strip("() ")
            table.setdefault((layer, what), set()).add(B)
            if default:
                for inst in GENERIC:
                    if inst in t or inst in k:
                        generic.setdefault(inst, set()).add((layer, B))
        if layer in CR_OF:
            groups = LAYERS[layer].gf if layer in LAYERS else LAYERS[layer[:-6]].gb
            line = CR_OF[layer]
            if line is not None and knobs.get("convres", 1) and B % CR_LINES[line][2] == 0:
                assert len(cr) == 1 and CR_LINES[line][1] in cr[0] and cr[0].endswith("img%d" % (groups * B)), (B, layer, knobs, launches)
                assert ("dgrad" in cr[0]) == layer.endswith("_dgrad") and " tr0 " in cr[0], cr
                hit.setdefault((CR_LINES[line][0], "dgrad" if layer.endswith("_dgrad") else "fwd"), set()).add((layer, B))
            else:       # knob off, the line does not divide this batch, or no such kernel: a generic kernel
                assert not cr and any(t.startswith("gemm ") for t, k in launches), (B, layer, knobs, launches)
                if line is not None:
                    fallback.setdefault(layer, set()).add(B)
        elif layer in RING_LAYERS:
            nimg = 3 * B if layer.startswith("dec_") else B
            if not knobs.get("wgrad_ring", 1) or nimg % 2 != 0:
                assert not ring and launches, (B, layer, knobs, launches)
                continue
            assert len(ring) == 1, (B, layer, knobs, launches)
            # wr_atomic_kb = 4096: fp32 atomics into the packed gradient, no reduce launch; 0: partial copies + reduce
            assert bool(reduce_) == (knobs["wr_atomic_kb"] == 0), (B, layer, knobs, launches)
            ring_hit.setdefault((layer, "atomic" if knobs["wr_atomic_kb"] else "copies"), set()).add(B)
        else:
            assert not cr and not ring, (B, layer, knobs, launches)
    for (layer, what), bs in sorted(table.items()):
        print("%-22s %-40s B %s" % (layer, what, sorted(bs)))
    missing = [(ln, f) for ln, _, _ in CR_LINES for f in ("fwd", "dgrad") if (ln, f) not in hit]
    missing += [l for l, line in CR_OF.items() if line is not None and l not in fallback]
    missing += [(l, m) for l in RING_LAYERS for m in ("atomic", "copies") if (l, m) not in ring_hit]
    missing += [(l, "B=%d" % max(BATCHES)) for l in RING_LAYERS if not any(max(BATCHES) in v for k, v in ring_hit.items() if k[0] == l)]
    missing += [inst for inst in GENERIC if inst not in generic]
    assert not missing, missing
    # the boundary case of the docstring: B = 128, dec_convT1 still on gemm_small, dec_convT2 past it
    assert ("dec_convT1", 128) in generic["small<2,2,1,fwd>"] and ("dec_convT2", 128) in generic["gather<8> ksplit1"]
