"""Layer-level tests of the MultiMNIST conv, data-gradient and weight-gradient kernels against a float64 reference.

One layer of the step is launched through mmvae_mm_bench_layer on operands this test wrote into the workspace and compared with
torch.nn.functional.conv2d / conv_transpose2d / torch.autograd in float64 (tests/layer_ref.py) -- never with another engine kernel.

Tier A (torch.equal): ternary operands make every product and every partial sum an integer below 2^24, so bf16 operands with
fp32 accumulation reproduce float64 bit for bit, in any accumulation order, with partial copies or atomics, with either rounding
of the bf16 store.  The conditions are asserted on the reference before every comparison.
Tier B (data gradients): the exact integer accumulator is multiplied by Swish'(scale * r + shift) in fp32 and stored as bf16;
per element |got - ref| <= 2^-8 |ref| + 1e-5 |acc| (one bf16 ulp of the stored value, either rounding mode; 100 fp32 epsilons
for the exp inside Swish') -- a dropped or misplaced tap moves acc by at least 1, i.e. by 1e5 times the second term.  The
BatchNorm-backward sums: |got - ref| <= 2^-16 sum |terms| (256 fp32 epsilons for the order of the partial sums; 85 times smaller
than one image's share at 768 images); both kernels sum the fp32 value BEFORE the bf16 store and so does the reference.

Batch sizes are read off the dispatch (csrc/convres.hip try_launch_convres, csrc/wgrad_ring.hip try_wr); test_coverage checks
from the probe's records that every instantiation reachable with default knobs ran in a compared launch.

The layer launches are the plain forms (GemmParams::tr kind 0).  What stays with the whole-step tests: the staged forms of the
fused step (kinds 1 and 2), dec_last_fused, conv1.hip's in-step form and the fused classifier tail (mlp_tail.hip); the text kernels
have a module of their own, tests/test_gpu_text_modules.py.  The CelebA plan has its own modules, tests/test_gpu_celeba_layers.py and
tests/test_gpu_celeba_layers_staged.py (mmvae_celeba_bench_layer), and so has the COCO plan: tests/test_gpu_coco_layers.py
(mmvae_coco_bench_layer: its conv and dense layers and its stand-alone passes)."""
import pytest
import torch
import torch.nn.functional as F

import layer_ref as LR
from layer_ref import LAYERS, SEEDS

pytestmark = pytest.mark.gpu
# MMVAE_TOL_REPORT=1 prints the worst error / gate ratio of every Tier B check (layer_ref.REPORT)

BATCHES = LR.BATCHES
_H = {}


def _harness(B, D=100):
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    if (B, D) not in _H:
        _H.clear()
        torch.cuda.empty_cache()
        _H[(B, D)] = LR.LayerHarness(B, n_latents=D)
    return _H[(B, D)]


# ------------------------------------------------------------------------------------------------ Tier A: forward
def _check_forward(h, name, x, w, knob_sets, what):
    LR.check_forward(h, LAYERS[name], name, x, w, knob_sets, what)


@pytest.mark.parametrize("name", list(LAYERS))
@pytest.mark.parametrize("B", BATCHES)
def test_forward_exact(B, name):
    h = _harness(B)
    L = LAYERS[name]
    ws, xs = [], []
    for seed in SEEDS:
        x, w, _ = LR.layer_operands(name, L.gf * B, seed)
        _check_forward(h, name, x, w, (dict(convres=1), dict(convres=0)), "%s B=%d seed %d" % (name, B, seed))
        ws.append(w)
        xs.append(x)
    LR.assert_operand_coverage(ws, xs)


@pytest.mark.parametrize("name", list(LAYERS))
@pytest.mark.parametrize("B", [8, 96])
def test_weight_packing_one_hot(B, name):
    """Packing alone: on a single +1 at one (image, pixel, channel) a forward layer reproduces the weight slice of that channel,
    tap by tap, at the output pixels the geometry says -- with distinct integer weights (|w| <= 126), so a slice landing in another
    tap's or channel's place cannot pass."""
    h = _harness(B)
    L = LAYERS[name]
    nimg, c = L.gf * B, L.ih // 2
    shape = LR.weight_shape(L)
    n = 1
    for s in shape:
        n *= s
    w = ((torch.arange(n, dtype=torch.int64) * 2654435761 >> 7) % 253 - 126).double().reshape(shape)
    for (im, y, xx, ch) in ((0, 0, 0, 0), (nimg - 1, L.ih - 1, L.ih - 1, L.cin - 1), (0, c, c, L.cin - 1), (nimg - 1, c, c, 0),
                            (nimg // 2, 0, L.ih - 1, L.cin // 2)):
        x = torch.zeros(nimg, L.ih, L.ih, L.cin, dtype=torch.float64)
        x[im, y, xx, ch] = 1.0
        _check_forward(h, name, x, w, (dict(convres=1), dict(convres=0)), "%s B=%d one-hot %s" % (name, B, (im, y, xx, ch)))


# ------------------------------------------------------------------------------------------------ Tier A: weight gradients
WG_KNOBS = (dict(wgrad_ring=0, wr_atomic_kb=256, wr_pair=0),) + tuple(
    dict(wgrad_ring=1, wr_atomic_kb=kb, wr_pair=pair) for kb in (0, 4096) for pair in (1, 0))


_check_wgrad = LR.check_wgrad


@pytest.mark.parametrize("name", list(LAYERS))
@pytest.mark.parametrize("B", BATCHES)
def test_wgrad_exact(B, name):
    h = _harness(B)
    L = LAYERS[name]
    for seed in SEEDS:
        x, _, dy = LR.layer_operands(name, L.gb * B, seed)
        h.put(L.x, x)
        h.put(L.dy, dy)
        _check_wgrad(h, name + "_wgrad", L.param, LR.ref_wgrad(L, x, dy), WG_KNOBS, "%s_wgrad B=%d seed %d" % (name, B, seed))


def _patches(img, g):
    """im2col of [g][1][50][50] for a 4x4 / stride 2 / padding 1 window: [g * 625][16], column ky * 4 + kx (torch's unfold order)"""
    return F.unfold(img, 4, padding=1, stride=2).permute(0, 2, 1).reshape(g * 625, 16).contiguous()


@pytest.mark.parametrize("B", BATCHES)
def test_thin_layers_exact(B):
    """The 1-channel ends of the network as dense GEMMs over an im2col buffer: enc_conv1 (raw output r1 exact, Swish copy a1 gated),
    enc_conv1_wgrad and dec_last_wgrad.  The patch buffers are a real im2col (torch unfold) of a ternary image / logit gradient, the references the
    conv2d / conv_transpose2d of multimnist/model.py:160,208 on that image."""
    h = _harness(B)
    f0, f9 = "image_encoder.features.0.weight", "image_decoder.hallucinate.9.weight"
    for seed in SEEDS:
        g = LR.gen(seed, 9, B)
        img = LR.ternary((B, 1, 50, 50), 0.5, g)
        w0 = LR.ternary((32, 1, 4, 4), 0.5, g)
        d1 = LR.ternary((B, 25, 25, 32), 0.5, g)
        h.put("patches1", _patches(img, B))
        # forward: r1 = conv2d(image, w0, stride 2, padding 1)
        ref = LR._nhwc(F.conv2d(img, w0, None, 2, 1))
        LR.assert_exact_regime(out=ref, what="enc_conv1")
        h.set_weight(f0, w0)
        h.zero("r1", ref.numel(), torch.bfloat16)
        launches = h.run("enc_conv1")
        got = h.get("r1", ref.shape).double().cpu()
        assert torch.equal(got, ref), (B, seed, launches, LR.describe_mismatch(got, ref))
        # its Swish copy a1 (the epilogue's second output): Tier B
        _gated(h.get("a1", ref.shape), ref * torch.sigmoid(ref), ref, "enc_conv1 a1 B=%d seed %d" % (B, seed))
        # weight gradient of the same layer from d1e
        wz = torch.zeros(32, 1, 4, 4, dtype=torch.float64, requires_grad=True)
        F.conv2d(img, wz, None, 2, 1).backward(LR._nchw(d1))
        h.put("d1e", d1)
        _check_wgrad(h, "enc_conv1_wgrad", f0, wz.grad, WG_KNOBS[:1] + WG_KNOBS[-1:], "enc_conv1_wgrad B=%d seed %d" % (B, seed))
        # last transposed conv (32 -> 1 channel): dW from its activated input aq3 and im2col(dlogit), 2 passes
        dl = LR.ternary((2 * B, 1, 50, 50), 0.5, g)
        a3 = LR.ternary((2 * B, 25, 25, 32), 0.5, g)
        w9 = torch.zeros(32, 1, 4, 4, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(LR._nchw(a3), w9, None, 2, 1).backward(dl)
        h.put("patches4", _patches(dl, 2 * B))
        h.put("aq3", a3)
        _check_wgrad(h, "dec_last_wgrad", f9, w9.grad, WG_KNOBS[:1] + WG_KNOBS[-1:], "dec_last_wgrad B=%d seed %d" % (B, seed))


# ------------------------------------------------------------------------------------------------ Tier B: data gradients
def _check_dgrad(h, name, dy, w, seed, knob_sets, what):
    g = LR.gen(seed, list(LAYERS).index(name), 4, dy.shape[0])
    LR.check_dgrad(h, LAYERS[name], name, dy, w, g, knob_sets, what)


@pytest.mark.parametrize("name", list(LAYERS))
@pytest.mark.parametrize("B", BATCHES)
def test_dgrad_epilogue(B, name):
    h = _harness(B)
    L = LAYERS[name]
    for seed in SEEDS:
        _, w, dy = LR.layer_operands(name, L.gb * B, seed)
        _check_dgrad(h, name, dy, w, seed, (dict(convres=1), dict(convres=0)), "%s_dgrad B=%d seed %d" % (name, B, seed))


# ------------------------------------------------------------------------------------------------ Tier B: dense layers
DROP_SCALE = 1.0 / (1.0 - 0.1)      # nn.Dropout(0.1) keep scale (multimnist/model.py:175,178; the engine's is the fp32 rounding of it)


def _swish(x):
    return x * torch.sigmoid(x)


# the comparisons are tests/layer_ref.py's, shared with the CelebA modules and shown on the CPU to see a dropped tap, image or
# column tile (tests/test_cpu_layer_ref.py)
_gated = LR.gate_elements
_exact = LR.check_exact


def _colsum_gate(h, N, v, what):
    LR.gate_sums(h.get("tmp_f32", (N,), torch.float32), v.sum(0), v.abs().sum(0), what + " d_colsum")


# Latent sizes of the dense layers: 100 at every batch; 20 (the reference's other default: N = 40, K = 20, ldz = 24), 99 (odd: the
# parameter offsets behind classifier.6 are no multiple of 4 floats, ldz = 104 as at 100) and 127 (the upper limit of
# mmvae_mm_create: N = 254, K = 127 with the bias in the last column of ldz = 128) at the odd and the even small batch.  At
# D = 100 the case keeps the id it had before the latent size became a parameter.
DENSE_CASES = [pytest.param(B, 100, id=str(B)) for B in BATCHES] + [
    pytest.param(B, D, id="%d-D%d" % (B, D)) for D in (20, 99, 127) for B in (7, 8)]


@pytest.mark.parametrize("B,D", DENSE_CASES)
def test_dense_layers(B, D):
    """The classifier (multimnist/model.py:173-179) and upsample (:195) Linears and their data gradients.  Integer weights, bias
    and operands make the pre-activation outputs (y1, y2, u, tmp_f32) exact; the Swish / keep-mask copies (ay1, ay2, au) and the
    data gradients (times Swish'(y) and the keep mask) take the per-element gate, d_colsum (the bias gradient of the Linear below)
    the 2^-16 gate.  The keep masks are written by the test.  The latent size D sets N = 2D of classifier.6 (enc_fc3), K = 2D of its
    data gradient, K = D of upsample.0 (dec_up, bias in column D of the ldz-wide z rows) and N = D of its data gradient."""
    h = _harness(B, D)
    rows = 2 * B
    pre, up = "image_encoder.classifier.", "image_decoder.upsample.0."
    for seed in SEEDS:
        g = LR.gen(seed, 11, B) if D == 100 else LR.gen(seed, 11, B, D)
        tern = lambda shape, d=0.5: LR.ternary(shape, d, g)
        ibias = lambda n: torch.randint(-2, 3, (n,), generator=g).double()
        keep = lambda shape: (torch.rand(shape, generator=g) < 0.9).to(torch.uint8)
        W1, W3, W6, Wu = tern((400, 1024), 0.25), tern((200, 400), 0.25), tern((2 * D, 200), 0.25), tern((1024, D), 0.25)
        b1, b3, b6, bu = ibias(400), ibias(200), ibias(2 * D), ibias(1024)
        for n, t in ((pre + "0.weight", W1), (pre + "0.bias", b1), (pre + "3.weight", W3), (pre + "3.bias", b3),
                     (pre + "6.weight", W6), (pre + "6.bias", b6), (up + "weight", Wu), (up + "bias", bu)):
            h.set_weight(n, t)
        m1, m2 = keep((rows, 400)), keep((rows, 200))
        h.put("m1", m1, torch.uint8)
        h.put("m2", m2, torch.uint8)
        tag = "B=%d D=%d seed %d" % (B, D, seed)

        # classifier.0 on the NHWC 2x2x256 map shared by both dropout variants (row r reads image r % B); torch flattens NCHW
        a4 = tern((B, 2, 2, 256))
        h.put("a4", a4)
        y1 = F.linear(LR._nchw(a4).reshape(B, 1024).repeat(2, 1), W1, b1)
        h.zero("y1", rows * 400, torch.bfloat16); h.zero("ay1", rows * 400, torch.bfloat16)
        h.run("enc_fc1")
        _exact(h.get("y1", (rows, 400)), y1, "enc_fc1 y1 " + tag)
        _gated(h.get("ay1", (rows, 400)), _swish(y1) * m1 * DROP_SCALE, y1, "enc_fc1 ay1 " + tag)

        x1 = tern((rows, 400))
        h.put("ay1", x1)
        y2 = F.linear(x1, W3, b3)
        h.zero("y2", rows * 200, torch.bfloat16); h.zero("ay2", rows * 200, torch.bfloat16)
        h.run("enc_fc2")
        _exact(h.get("y2", (rows, 200)), y2, "enc_fc2 y2 " + tag)
        _gated(h.get("ay2", (rows, 200)), _swish(y2) * m2 * DROP_SCALE, y2, "enc_fc2 ay2 " + tag)

        x2 = tern((rows, 200))
        h.put("ay2", x2)
        h.zero("tmp_f32", rows * 2 * D, torch.float32)
        h.run("enc_fc3")
        _exact(h.get("tmp_f32", (rows, 2 * D), torch.float32), F.linear(x2, W6, b6), "enc_fc3 " + tag)

        # data gradients: dy2 = (d_encout W6) * Swish'(y2) * keep2 / 0.9, dy1 = (dy2 W3) * Swish'(y1) * keep1 / 0.9
        # (d_encout rows are round_up(2D, 8) wide with zero pad columns: the stride the step's latent backward writes)
        de, r2, r1 = tern((rows, 2 * D)), LR.eighths((rows, 200), g), LR.eighths((rows, 400), g)
        de_rows = torch.zeros(rows, (2 * D + 7) // 8 * 8, dtype=torch.float64)
        de_rows[:, :2 * D] = de
        h.put("d_encout", de_rows); h.put("y2", r2); h.put("y1", r1)
        acc = de @ W6
        v = acc * LR.dswish(r2) * m2 * DROP_SCALE
        h.zero("dy2", rows * 200, torch.bfloat16); h.zero("tmp_f32", 200, torch.float32)
        h.run("enc_fc3_dgrad")
        _gated(h.get("dy2", (rows, 200)), v, acc, "enc_fc3_dgrad " + tag)
        _colsum_gate(h, 200, v, "enc_fc3_dgrad " + tag)
        d2 = tern((rows, 200))
        h.put("dy2", d2)
        acc = d2 @ W3
        v = acc * LR.dswish(r1) * m1 * DROP_SCALE
        h.zero("dy1", rows * 400, torch.bfloat16); h.zero("tmp_f32", 400, torch.float32)
        h.run("enc_fc2_dgrad")
        _gated(h.get("dy1", (rows, 400)), v, acc, "enc_fc2_dgrad " + tag)
        _colsum_gate(h, 400, v, "enc_fc2_dgrad " + tag)

        # upsample: z rows carry a 1.0 in column D (the bias rides in the packed weights); the output is the NHWC 2x2x256 map
        # of torch's view(-1, 256, 2, 2)
        ldz = (D + 1 + 7) // 8 * 8
        z = torch.zeros(3 * B, ldz, dtype=torch.float64)
        z[:, :D] = tern((3 * B, D))
        z[:, D] = 1.0
        h.put("z_bf", z)
        u = LR._nhwc(F.linear(z[:, :D], Wu, bu).reshape(3 * B, 256, 2, 2)).reshape(3 * B, 1024)
        h.zero("u", 3 * B * 1024, torch.bfloat16); h.zero("au", 3 * B * 1024, torch.bfloat16)
        h.run("dec_up")
        _exact(h.get("u", (3 * B, 1024)), u, "dec_up u " + tag)
        _gated(h.get("au", (3 * B, 1024)), _swish(u), u, "dec_up au " + tag)
        du = tern((rows, 2, 2, 256))
        h.put("du", du)
        h.zero("tmp_f32", rows * D, torch.float32)
        h.run("dec_up_dgrad")
        _exact(h.get("tmp_f32", (rows, D), torch.float32), LR._nchw(du).reshape(rows, 1024) @ Wu, "dec_up_dgrad " + tag)


@pytest.mark.parametrize("B", BATCHES)
def test_last_layer_dgrad(B):
    """dec_last_dgrad_gemm: the input gradient of the 32 -> 1 channel transposed conv (multimnist/model.py:208) as a dense GEMM over
    im2col(dlogit), with the Swish' / BatchNorm-backward epilogue of the layer below (hallucinate.7), 2 passes."""
    h = _harness(B)
    for seed in SEEDS:
        g = LR.gen(seed, 12, B)
        dl = LR.ternary((2 * B, 1, 50, 50), 0.5, g)
        w9 = LR.ternary((32, 1, 4, 4), 0.5, g)
        x = torch.zeros(2 * B, 32, 25, 25, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(x, w9, None, 2, 1).backward(dl)
        acc = LR._nhwc(x.grad)
        r = LR.eighths(acc.shape, g)
        aff, mr = LR.dyadic_tables(2, 32, g)
        v, red, red_abs = LR.ref_dgrad_epilogue(acc, r, aff, mr, 2)
        h.set_weight("image_decoder.hallucinate.9.weight", w9)
        h.put("patches4", _patches(dl, 2 * B))
        h.put("q3", r)
        h.put("aff_d2", aff, torch.float32)
        h.put("mr_d2", mr, torch.float32)
        h.zero("d3", acc.numel(), torch.bfloat16)
        h.zero("red_d2", 2 * LR.STAT_SLOTS * 32 * 2, torch.float32)
        h.run("dec_last_dgrad_gemm")
        what = "dec_last_dgrad_gemm B=%d seed %d" % (B, seed)
        _gated(h.get("d3", acc.shape), v, acc, what)
        LR.gate_sums(h.stats("red_d2", 2, 32), red, red_abs, what + " d_red")


# ------------------------------------------------------------------------------------------------ measurement-aid forms
# convres_alt -> the layers whose try_cr line it changes (csrc/convres.hip try_launch_convres)
ALT_FORMS = {
    1: (("dec_convT3",), ()),                                       # G_mm_convT3 <4, 20, 8, 1>
    3: (("enc_conv3", "dec_convT2"), ("enc_conv3", "dec_convT2")),  # LDS-chunk forms of G_mm_conv3 / G_mm_convT2
    4: (("enc_conv4", "dec_convT1"), ("enc_conv4", "dec_convT1")),  # the bottleneck pair on the generic GEMM
    5: (("dec_convT1",), ()),                                       # G_mm_convT1 <8, ...> at nimg > 256
}


@pytest.mark.parametrize("alt", sorted(ALT_FORMS))
def test_convres_alt_forms(alt):
    B, seed = 256, 0
    h = _harness(B)
    fwd, dgr = ALT_FORMS[alt]
    for name in fwd:
        x, w, _ = LR.layer_operands(name, LAYERS[name].gf * B, seed)
        _check_forward(h, name, x, w, (dict(convres=1, convres_alt=alt),), "%s B=%d alt %d" % (name, B, alt))
    for name in dgr:
        _, w, dy = LR.layer_operands(name, LAYERS[name].gb * B, seed)
        _check_dgrad(h, name, dy, w, seed, (dict(convres=1, convres_alt=alt),), "%s_dgrad B=%d alt %d" % (name, B, alt))


# ------------------------------------------------------------------------------------------------ which kernels ran
# The probe (mmvae_debug_probe) reports the launch macro's kernel text, "convres_kernel<G, NI, CH, ...>" with the template
# parameters unexpanded, and the launcher's tag "convres form<F> <C>><N> <AH>x<AW>><OH>x<OW> k<K> s<S> fwd|dgrad tr<kind> img<nimg>":
# the geometry and the image count, not NI / CH / NSPLIT.  Two instantiations of one geometry are told apart here by the image
# count and batch the dispatch keys on, restated from try_launch_convres; the assertion is at that granularity.
#   (try_cr line, geometry part of the tag, lambda nimg, B: this line takes the launch)
CR_LINES = (
    ("G_mm_conv2 <1, 16, 8, 2>", "form0 32>64 25x25>12x12 k4 s2", lambda n, B: True),
    ("G_mm_conv3 <2, 0, 8, 4>", "form0 64>128 12x12>6x6 k4 s2", lambda n, B: B % 2 == 0),
    ("G_mm_convT2 <2, 0, 8, 2>", "form1 128>64 6x6>12x12 k4 s2", lambda n, B: n <= 256 and B % 2 == 0),
    ("G_mm_convT2 <4, 0, 8, 2>", "form1 128>64 6x6>12x12 k4 s2", lambda n, B: n > 256 and B % 4 == 0),
    ("G_mm_convT3 <2, 16, 4, 1>", "form1 64>32 12x12>25x25 k5 s2", lambda n, B: B % 2 == 0),
    ("G_mm_conv2d <1, 16, 8, 1>", "form1 64>32 12x12>25x25 k4 s2", lambda n, B: True),
    ("G_mm_convT1 <16, 0, 5, 1, 4, 1>", "form1 256>128 2x2>6x6 k4 s2", lambda n, B: n > 256 and B % 16 == 0),
    ("G_mm_convT1 <8, 0, 6, 1, 4, 2>", "form1 256>128 2x2>6x6 k4 s2", lambda n, B: B % 8 == 0 and not (n > 256 and B % 16 == 0)),
    ("G_mm_conv4 <8, 0, 8, 2, 4, 4>", "form0 128>256 6x6>2x2 k4 s2", lambda n, B: B % 8 == 0),
    ("G_mm_convT3d <2, 10, 8, 2>", "form0 32>64 25x25>12x12 k5 s2", lambda n, B: B % 2 == 0),
)
# geometry tag of each layer launch (forward, data gradient): csrc/convres.hip, the typedefs under try_cr
GEO_OF = {
    "enc_conv2": CR_LINES[0][1], "enc_conv3": CR_LINES[1][1], "enc_conv4": CR_LINES[8][1],
    "dec_convT1": CR_LINES[6][1], "dec_convT2": CR_LINES[2][1], "dec_convT3": CR_LINES[4][1],
    "enc_conv2_dgrad": CR_LINES[5][1], "enc_conv3_dgrad": CR_LINES[2][1], "enc_conv4_dgrad": CR_LINES[6][1],
    "dec_convT1_dgrad": CR_LINES[8][1], "dec_convT2_dgrad": CR_LINES[1][1], "dec_convT3_dgrad": CR_LINES[9][1],
}
# ring geometries of WGRAD_RING_GEOS (csrc/wgrad_ring_geos.h) that match a MultiMNIST layer: (name, layers, images per ring slot IB,
# needs wr_pair).  The probe names the kernel "wgrad_ring_kernel<G>" without the geometry and carries no tag: a geometry counts as
# reached when the ring kernel ran for one of its layers at an image count it accepts (nimg % IB == 0), the pair form with wr_pair = 1
# (if try_wr declined the pair form the single form behind it in the list would run and be credited here: the result is compared
# exactly whichever ran, only the attribution is the dispatch's, not an observation).
RING_GEOS = (
    ("mm_convT3p", ("dec_convT3_wgrad",), 1, True),
    ("mm_convT3", ("dec_convT3_wgrad",), 1, False),
    ("mm_conv2", ("enc_conv2_wgrad",), 1, False),
    ("mm_conv3", ("enc_conv3_wgrad", "dec_convT2_wgrad"), 2, False),
    ("mm_conv4", ("enc_conv4_wgrad", "dec_convT1_wgrad"), 16, False),
)


def test_coverage():
    """Over the launches the tests above compared (run the whole module: this test reads their records): every try_cr line
    reachable with default knobs and every MultiMNIST ring geometry ran at least once, the generic kernels took the launches the
    dispatch leaves to them, and no image-resident / ring kernel ran with its knob off."""
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    recs = [r for r in LR.RECORDS if r[2].get("convres_alt", 0) == 0]
    assert {r[0] for r in recs} >= set(BATCHES), "run the whole module: the compared launches of every batch size are the input of this test"
    hit, ring_hit = {}, {}
    for B, layer, knobs, launches in recs:
        cr = [t for t, k in launches if t.startswith("convres ")]
        ring = [k for t, k in launches if "wgrad_ring_kernel" in k]
        reduce_ = [k for t, k in launches if "wgrad_ring_reduce_kernel" in k]
        if layer in GEO_OF:
            groups = (LAYERS[layer].gf if layer in LAYERS else LAYERS[layer[:-6]].gb)
            nimg = groups * B
            lines = [ln for ln, geo, pred in CR_LINES if geo == GEO_OF[layer] and pred(nimg, B)]
            assert len(lines) <= 1, (layer, B, lines)
            if knobs.get("convres", 1) and lines:
                assert len(cr) == 1 and GEO_OF[layer] in cr[0] and cr[0].endswith("img%d" % nimg), (B, layer, knobs, launches)
                assert ("dgrad" in cr[0]) == layer.endswith("_dgrad") and " tr0 " in cr[0], cr
                hit.setdefault(lines[0], []).append((layer, B))
            else:       # knob off, or no instantiation divides this batch: the generic gather GEMM
                assert not cr, (B, layer, knobs, launches)
                assert launches, (B, layer, knobs, "the probe saw no launch")
        if layer.endswith("_wgrad"):
            geo = [g for g in RING_GEOS if layer in g[1]]
            nimg = 2 * B if layer.startswith("dec_") else B
            if not knobs.get("wgrad_ring", 1) or not geo or nimg % geo[0][2] != 0:
                assert not ring, (B, layer, knobs, launches)
                assert launches, (B, layer, knobs, "the probe saw no launch")
                continue
            assert len(ring) == 1, (B, layer, knobs, launches)
            # wr_atomic_kb = 4096: fp32 atomics into the packed gradient, no reduce launch; 0: partial copies + reduce
            assert bool(reduce_) == (knobs["wr_atomic_kb"] == 0), (B, layer, knobs, launches)
            for gname, _, _, pair in geo:
                if pair == bool(knobs.get("wr_pair", 0)) or (len(geo) == 1):
                    ring_hit.setdefault(gname, []).append((layer, B, knobs["wr_atomic_kb"]))
    for ln, geo, _ in CR_LINES:
        print("convres %-34s %s: %s" % (ln, geo, sorted(set(hit.get(ln, [])))))
    for gname, _, _, _ in RING_GEOS:
        print("wgrad_ring %-12s: %s" % (gname, sorted(set(ring_hit.get(gname, [])))))
    missing = [ln for ln, _, _ in CR_LINES if ln not in hit] + [g[0] for g in RING_GEOS if g[0] not in ring_hit]
    assert not missing, missing
    alts = {r[2]["convres_alt"] for r in LR.RECORDS if r[2].get("convres_alt", 0)}
    assert alts == set(ALT_FORMS), alts
