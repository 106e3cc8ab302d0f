"""Layer-level tests of the CelebA conv, data-gradient and weight-gradient kernels against a float64 reference (plain forms).

One layer of the CelebA step is launched through mmvae_celeba_bench_layer -- which builds its launch parameters with the same
tower_gemm / tower_wgrad of csrc/img_tower.h (and fc2_dgrad_gemm of csrc/celeba.hip) the step calls -- on operands this test wrote into the workspace, and compared with
torch.nn.functional.conv2d / conv_transpose2d / linear / torch.autograd in float64 (tests/layer_ref.py), never with another
engine kernel.  Tiers and gates are those of tests/test_gpu_layers.py, derived there from the number formats:
Tier A, torch.equal on ternary operands (every product and partial sum an integer below 2^24; asserted on the reference first);
Tier B, |got - ref| <= 2^-8 |ref| + 1e-5 |acc| per element for what passes through Swish / Swish' and a bf16 store, and
|got - ref| <= 2^-16 sum |terms| for the BatchNorm-backward and bias-gradient sums.

Batches, read off the dispatch:
  csrc/convres.hip try_launch_convres, the four G_ca_* lines: try_cr takes a launch when group_n % NI == 0 with group_n = B
  (encoder: 1 group, decoder: 3 groups of B) and NI = 1 (G_ca_conv2) / 2 (G_ca_conv3) / 4 (G_ca_convT2) / 2 (G_ca_convT3):
  B = 3 leaves all but G_ca_conv2 to gemm_gather, B = 6 (2 mod 4) leaves G_ca_convT2, B = 4 and 8 take every line.  The
  stride-1 8x8 <-> 5x5 pair (features.8, hallucinate.0) has no image-resident kernel: gemm_gather at every batch.
  csrc/wgrad_ring.hip try_wr, ca_conv2 / ca_conv3 / ca_conv4: needs nimg % IB == 0 with IB = 1 / 2 / 4 and nimg = B (encoder)
  or 3B (decoder): B = 3 reaches only ca_conv2, B = 6 not ca_conv4, B = 4 and 8 all three.
  B = 256: some workgroup of every ring geometry runs more ring batches than SLOTS + 1 = 3, on both sides.  With 256 CUs
  (mmvae_cu_count on the MI355X), units = nimg / IB, target = 3 or 4 quarters of the CUs (4 when the layer has >= 4e9 MACs or
  WGQ = 4), NJ = 4 job classes of equal weight (the 4 stride parities of a 4x4 stride-2 window, or ca_conv4's 4 tap rows) and
  MS = N / 64 channel slices, groups[i] = target / (NJ * MS) and a workgroup runs units / groups[i] batches:
    ca_conv2 (MS 1): encoder units 256, 2.1e9 MACs, target 192, groups 48: 5.3 batches; decoder units 768, target 256, groups 64: 12
    ca_conv3 (MS 2): encoder units 128, target 192, groups 24: 5.3; decoder units 384, 6.4e9 MACs, target 256, groups 32: 12
    ca_conv4 (MS 4, WGQ 4): encoder units 64, target 256, groups 16: 4; decoder units 192: 12
  (with fewer CUs the groups shrink and the batches per workgroup grow: the condition still holds).

test_coverage checks from the probe's records that each G_ca_* instantiation, each ca_* ring geometry in both epilogue modes,
the gemm_gather fallback of every conv layer and the gemm_gather path of the stride-1 pair ran in a compared launch.

The staged forms of the fused step (GatherTransform kinds 1 and 2) have their own module, tests/test_gpu_celeba_layers_staged.py.
What stays with the whole-step tests: dec_last_ca_kernel and the attribute MLPs."""
import pytest
import torch
import torch.nn.functional as F

import layer_ref as LR
from layer_ref import LAYERS_CELEBA as LAYERS

pytestmark = pytest.mark.gpu

BATCHES = LR.BATCHES_CELEBA
D, HID, FEAT = 100, 1024, 6400
LDZ = (D + 1 + 7) // 8 * 8
_H = {}


def _harness(B):
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    if B not in _H:
        _H.clear()
        torch.cuda.empty_cache()
        _H[B] = LR.celeba_harness(B)
    return _H[B]


def _seeds(B):
    """both seeds at the small batches, one at the large one (its float64 references take a second each)"""
    return LR.SEEDS if B <= 8 else LR.SEEDS[:1]


CR_KNOBS = (dict(convres=1), dict(convres=0))
# ring off; ring on with the atomic epilogue; ring on with partial copies + reduce (csrc/wgrad_ring.hip try_wr: `atomic`)
WG_KNOBS = (dict(wgrad_ring=0, wr_atomic_kb=256), dict(wgrad_ring=1, wr_atomic_kb=4096), dict(wgrad_ring=1, wr_atomic_kb=0))


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
    tap by tap, at the output pixels the geometry says."""
    h = _harness(B)
    L = LAYERS[name]
    nimg, c = L.gf * B, L.ih // 2
    w = _distinct_ints(LR.weight_shape(L))
    for (im, y, xx, ch) in ((0, 0, 0, 0), (nimg - 1, L.ih - 1, L.ih - 1, L.cin - 1), (0, c, c, L.cin - 1), (nimg - 1, c, c, 0),
                            (nimg // 2, 0, L.ih - 1, L.cin // 2)):
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


def _patches(img):
    """im2col of [n][3][64][64] for a 4x4 / stride 2 / padding 1 window: [n * 1024][48], column (ky * 4 + kx) * 3 + channel
    (csrc/elementwise.hip im2col_small_kernel; torch's unfold has the channel slowest)"""
    n = img.shape[0]
    u = F.unfold(img, 4, padding=1, stride=2).reshape(n, 3, 16, 1024)
    return u.permute(0, 3, 2, 1).reshape(n * 1024, 48).contiguous()


@pytest.mark.parametrize("B", BATCHES)
def test_thin_layers_exact(B):
    """The 3-channel ends of the network as dense K = 48 GEMMs over an im2col buffer: enc_conv1 (raw output r1 exact, Swish copy a1
    gated), enc_conv1_wgrad and dec_last_wgrad (3 passes).  The patch buffers are a real unfold of a ternary image / logit
    gradient, the references the conv2d / conv_transpose2d of celeba/model.py:101,150 on that image."""
    h = _harness(B)
    f0, f9 = "image_encoder.features.0.weight", "image_decoder.hallucinate.9.weight"
    for seed in _seeds(B):
        g = LR.gen(seed, 9, B)
        img = LR.ternary((B, 3, 64, 64), 0.5, g)
        w0 = LR.ternary((32, 3, 4, 4), 0.5, g)
        d1 = LR.ternary((B, 32, 32, 32), 0.5, g)
        h.put("patches1", _patches(img))
        ref = LR._nhwc(F.conv2d(img, w0, None, 2, 1))
        LR.assert_exact_regime(out=ref, what="enc_conv1")
        h.set_weight(f0, w0)
        h.zero("r1", ref.numel(), torch.bfloat16)
        h.zero("a1", ref.numel(), torch.bfloat16)
        launches = h.run("enc_conv1")
        got = h.get("r1", ref.shape).double().cpu()
        assert torch.equal(got, ref), (B, seed, launches, LR.describe_mismatch(got, ref))
        LR.gate_elements(h.get("a1", ref.shape), ref * torch.sigmoid(ref), ref, "enc_conv1 a1 B=%d seed %d" % (B, seed))
        wz = torch.zeros(32, 3, 4, 4, dtype=torch.float64, requires_grad=True)
        F.conv2d(img, wz, None, 2, 1).backward(LR._nchw(d1))
        h.put("d1e", d1)
        # (the K = 48 im2col ends and the two Linears below match no ring geometry -- csrc/wgrad_ring_geos.h, and a_bcast_n keeps
        #  fc1 out of try_launch_wgrad_ring -- so the partial-copies knob set would repeat the same launch: ring off / on only)
        LR.check_wgrad(h, "enc_conv1_wgrad", f0, wz.grad, WG_KNOBS[:2], "enc_conv1_wgrad B=%d seed %d" % (B, seed))
        # last transposed conv (32 -> 3 channels): dW from its activated input aq3 and im2col(dlogit), 3 passes
        dl = LR.ternary((3 * B, 3, 64, 64), 0.25, g)
        a3 = LR.ternary((3 * B, 32, 32, 32), 0.25, g)
        w9 = torch.zeros(32, 3, 4, 4, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(LR._nchw(a3), w9, None, 2, 1).backward(dl)
        h.put("patches4", _patches(dl))
        h.put("aq3", a3)
        LR.check_wgrad(h, "dec_last_wgrad", f9, w9.grad, WG_KNOBS[:2], "dec_last_wgrad B=%d seed %d" % (B, seed))


# ------------------------------------------------------------------------------------------------ Tier B: data gradients
@pytest.mark.parametrize("name", list(LAYERS))
@pytest.mark.parametrize("B", BATCHES)
def test_dgrad_epilogue(B, name):
    h = _harness(B)
    L = LAYERS[name]
    for seed in _seeds(B):
        _, w, dy = LR.layer_operands(name, L.gb * B, seed, LAYERS)
        g = LR.gen(seed, list(LAYERS).index(name), 4, L.gb * B)
        LR.check_dgrad(h, L, name, dy, w, g, CR_KNOBS, "%s_dgrad B=%d seed %d" % (name, B, seed))


@pytest.mark.parametrize("B", BATCHES)
def test_last_layer_dgrad(B):
    """dec_last_dgrad_gemm: the input gradient of the 32 -> 3 channel transposed conv (celeba/model.py:150) as a dense K = 48 GEMM
    over im2col(dlogit), with the Swish' / BatchNorm-backward epilogue of hallucinate.7, 3 passes."""
    h = _harness(B)
    for seed in _seeds(B):
        g = LR.gen(seed, 12, B)
        dl = LR.ternary((3 * B, 3, 64, 64), 0.5, g)
        w9 = LR.ternary((32, 3, 4, 4), 0.5, g)
        x = torch.zeros(3 * B, 32, 32, 32, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(x, w9, None, 2, 1).backward(dl)
        acc = LR._nhwc(x.grad)
        r = LR.eighths(acc.shape, g)
        aff, mr = LR.dyadic_tables(3, 32, g)
        v, red, red_abs = LR.ref_dgrad_epilogue(acc, r, aff, mr, 3)
        h.set_weight("image_decoder.hallucinate.9.weight", w9)
        h.put("patches4", _patches(dl))
        h.put("q3", r)
        h.put("aff_d2", aff, torch.float32)
        h.put("mr_d2", mr, torch.float32)
        h.zero("d3", acc.numel(), torch.bfloat16)
        h.zero("red_d2", 3 * LR.STAT_SLOTS * 32 * 2, torch.float32)
        launches = h.run("dec_last_dgrad_gemm")
        what = "dec_last_dgrad_gemm B=%d seed %d" % (B, seed)
        LR.gate_elements(h.get("d3", acc.shape), v, acc, what, launches)
        LR.gate_sums(h.stats("red_d2", 3, 32), red, red_abs, what + " d_red", launches)


# ------------------------------------------------------------------------------------------------ the two permuted Linears
DROP_SCALE = 1.0 / (1.0 - 0.1)      # nn.Dropout(0.1) keep scale (celeba/model.py:117; the engine's is the fp32 rounding of it)
C0, C3, UP = "image_encoder.classifier.0.", "image_encoder.classifier.3.", "image_decoder.upsample.0."


def _swish(x):
    return x * torch.sigmoid(x)


def _flat_nchw(t):
    """[n][5][5][256] NHWC -> torch's flatten of (256, 5, 5): column c * 25 + y * 5 + x"""
    return LR._nchw(t).reshape(t.shape[0], FEAT)


def _map_nhwc(t):
    """[n][6400] in torch's order c * 25 + s -> the engine's NHWC column s * 256 + c, as [n][5][5][256]"""
    return LR._nhwc(t.reshape(t.shape[0], 256, 5, 5))


def _z_rows(z):
    """z_bf operand [rows][LDZ]: the latent, a 1.0 in column D (the bias rides in the packed weights), zero padding"""
    out = torch.zeros(z.shape[0], LDZ, dtype=torch.float64)
    out[:, :D] = z
    out[:, D] = 1.0
    return out


@pytest.mark.parametrize("B", BATCHES)
def test_dense_layers(B):
    """classifier.0 (celeba/model.py:115: Linear(6400, 1024) on the NCHW flatten of the 256x5x5 map, held here as NHWC and shared
    by the 2 dropout variants: a_bcast_n) and upsample.0 (:136: Linear(D, 6400) viewed as 256x5x5, written here as NHWC, bias
    folded into the packed weights) with their weight and data gradients, and classifier.3's data gradient.  Integer weights, biases
    and operands make the pre-activations y1 / u, the weight gradients and dz exact; the Swish / keep-mask copies and the gradients
    through Swish' take the per-element gate, the BatchNorm-backward / bias sums the 2^-16 gate.  The keep mask is the test's."""
    h = _harness(B)
    rows = 2 * B
    for seed in _seeds(B):
        g = LR.gen(seed, 11, B)
        tern = lambda shape, d=0.5: LR.ternary(shape, d, g)
        ibias = lambda n: torch.randint(-2, 3, (n,), generator=g).double()
        W1, W3, Wu = tern((HID, FEAT), 0.25), tern((2 * D, HID), 0.25), tern((FEAT, D), 0.25)
        b1, bu = ibias(HID), ibias(FEAT)
        for n, t in ((C0 + "weight", W1), (C0 + "bias", b1), (C3 + "weight", W3), (UP + "weight", Wu), (UP + "bias", bu)):
            h.set_weight(n, t)
        m1 = (torch.rand((rows, HID), generator=g) < 0.9).to(torch.uint8)
        h.put("m1", m1, torch.uint8)
        tag = "B=%d seed %d" % (B, seed)

        # ---- classifier.0 forward: row r of the 2B rows reads image r % B
        a4 = tern((B, 5, 5, 256), 0.25)
        h.put("a4", a4)
        x1 = _flat_nchw(a4).repeat(2, 1)
        y1 = F.linear(x1, W1, b1)
        for mask in (0, 1):
            h.zero("y1", rows * HID, torch.bfloat16)
            h.zero("ay1", rows * HID, torch.bfloat16)
            h.run("fc1", celeba_layer_mask=mask)
            LR.check_exact(h.get("y1", (rows, HID)), y1, "fc1 y1 mask %d %s" % (mask, tag))
            LR.gate_elements(h.get("ay1", (rows, HID)), _swish(y1) * (m1 * DROP_SCALE if mask else 1.0), y1, "fc1 ay1 mask %d %s" % (mask, tag))

        # ---- classifier.3 data gradient: dy1 = (d_encout W3) * Swish'(y1) [* keep / 0.9], column sums = classifier.0's bias gradient
        de, r1 = tern((rows, 2 * D)), LR.eighths((rows, HID), g)
        h.put("d_encout", de)
        h.put("y1", r1)
        acc = de @ W3
        for mask in (0, 1):
            v = acc * LR.dswish(r1) * (m1 * DROP_SCALE if mask else 1.0)
            h.zero("dy1", rows * HID, torch.bfloat16)
            h.st.grads.zero_()              # d_colsum adds into the flat gradients at classifier.0.bias, as in the step
            h.run("fc2_dgrad", celeba_layer_mask=mask)
            LR.gate_elements(h.get("dy1", (rows, HID)), v, acc, "fc2_dgrad mask %d %s" % (mask, tag))
            boff, _, _ = h.param_range(C0 + "bias")
            LR.gate_sums(h.st.grads[boff:boff + HID], v.sum(0), v.abs().sum(0), "fc2_dgrad d_colsum mask %d %s" % (mask, tag))
            others = h.st.grads.clone()
            others[boff:boff + HID] = 0
            assert float(others.abs().max()) == 0.0, "fc2_dgrad wrote a gradient other than classifier.0.bias"

        # ---- classifier.0 gradients.  dy1 dense, and with the zeros a keep mask upstream leaves in it (the step with dropout)
        for masked in (0, 1):
            dy1 = tern((rows, HID)) * (m1.double() if masked else 1.0)
            h.put("dy1", dy1)
            wz = torch.zeros(HID, FEAT, dtype=torch.float64, requires_grad=True)
            F.linear(x1, wz).backward(dy1)
            LR.check_wgrad(h, "fc1_wgrad", C0 + "weight", wz.grad, WG_KNOBS[:1], "fc1_wgrad masked %d %s" % (masked, tag))
            # db4[n][s * 256 + c] = (dy1 W1)[n][c * 25 + s] * Swish'(scale_c * r4[n % B] + shift_c); sums per channel c = column % 256
            acc = _map_nhwc(dy1 @ W1)
            r4 = LR.eighths((B, 5, 5, 256), g)
            aff, mr = LR.dyadic_tables(1, 256, g)
            v, red, red_abs = LR.ref_dgrad_epilogue(acc, r4.repeat(2, 1, 1, 1), aff, mr, 1)
            h.put("r4", r4)
            h.put("aff_e2", aff, torch.float32)
            h.put("mr_e2", mr, torch.float32)
            h.zero("db4", rows * FEAT, torch.bfloat16)
            h.zero("red_e2", LR.STAT_SLOTS * 256 * 2, torch.float32)
            launches = h.run("fc1_dgrad")
            LR.gate_elements(h.get("db4", acc.shape), v, acc, "fc1_dgrad masked %d %s" % (masked, tag), launches)
            LR.gate_sums(h.stats("red_e2", 1, 256), red, red_abs, "fc1_dgrad d_red masked %d %s" % (masked, tag), launches)

        # ---- upsample.0: forward, weight + folded bias gradient, dz
        z = tern((3 * B, D))
        h.put("z_bf", _z_rows(z))
        u = _map_nhwc(F.linear(z, Wu, bu)).reshape(3 * B, FEAT)
        h.zero("u", 3 * B * FEAT, torch.bfloat16)
        h.zero("au", 3 * B * FEAT, torch.bfloat16)
        h.run("up")
        LR.check_exact(h.get("u", (3 * B, FEAT)), u, "up u " + tag)
        LR.gate_elements(h.get("au", (3 * B, FEAT)), _swish(u), u, "up au " + tag)
        du = tern((3 * B, 5, 5, 256), 0.25)
        h.put("du", du)
        duf = _flat_nchw(du)
        LR.check_wgrad(h, "up_wgrad", UP + "weight", duf.t() @ z, WG_KNOBS[:1], "up_wgrad " + tag, also={UP + "bias": duf.sum(0)})
        h.zero("dz_img", 3 * B * D, torch.float32)
        h.run("up_dgrad")
        LR.check_exact(h.get("dz_img", (3 * B, D), torch.float32), duf @ Wu, "up_dgrad " + tag, limit=2 ** 24)


@pytest.mark.parametrize("B", [3, 8])
def test_dense_packing_one_hot(B):
    """The permuted packings of classifier.0 and upsample.0 (csrc/celeba.hip build(): PackDesc TW / C / s_ty / s_tx / s_c, NL / s_nhi
    / s_nlo, b_nhi / b_nlo) with dense, distinct integer weights.
    fc1: a single +1 at (row, y, x, c) of the 5x5x256 map gives column c * 25 + y * 5 + x of classifier.0.weight plus the bias, in
    both row blocks of the broadcast, and the bias alone in every other row.
    up: a single +1 at z_bf[row][k] gives upsample.0.weight[c * 25 + s][k] plus bias[c * 25 + s] at NHWC column s * 256 + c."""
    h = _harness(B)
    rows = 2 * B
    W1, Wu = _distinct_ints((HID, FEAT)), _distinct_ints((FEAT, D))
    b1 = (torch.arange(HID) % 5 - 2).double()
    bu = (torch.arange(FEAT) % 7 - 3).double()
    for n, t in ((C0 + "weight", W1), (C0 + "bias", b1), (UP + "weight", Wu), (UP + "bias", bu)):
        h.set_weight(n, t)
    for (n, y, x, c) in ((0, 0, 0, 0), (B - 1, 4, 4, 255), (B // 2, 1, 3, 128), (0, 4, 0, 7), (B - 1, 2, 2, 1)):
        a4 = torch.zeros(B, 5, 5, 256, dtype=torch.float64)
        a4[n, y, x, c] = 1.0
        want = b1.repeat(rows, 1)
        want[n] += W1[:, c * 25 + y * 5 + x]
        want[n + B] += W1[:, c * 25 + y * 5 + x]
        assert torch.equal(want, F.linear(_flat_nchw(a4).repeat(2, 1), W1, b1))
        h.put("a4", a4)
        h.zero("y1", rows * HID, torch.bfloat16)
        h.run("fc1")
        LR.check_exact(h.get("y1", (rows, HID)), want, "fc1 one-hot %s B=%d" % ((n, y, x, c), B))
    for (row, k) in ((0, 0), (3 * B - 1, D - 1), (B, 37), (2 * B - 1, 64)):
        z = torch.zeros(3 * B, D, dtype=torch.float64)
        z[row, k] = 1.0
        want = bu.repeat(3 * B, 1)
        want[row] += Wu[:, k]
        assert torch.equal(want, F.linear(z, Wu, bu))
        want = _map_nhwc(want).reshape(3 * B, FEAT)
        s, c = 13, 200
        assert float(want[row, s * 256 + c]) == float(Wu[c * 25 + s, k] + bu[c * 25 + s])
        h.put("z_bf", _z_rows(z))
        h.zero("u", 3 * B * FEAT, torch.bfloat16)
        h.run("up")
        LR.check_exact(h.get("u", (3 * B, FEAT)), want, "up one-hot %s B=%d" % ((row, k), B))


# ------------------------------------------------------------------------------------------------ which kernels ran
# The probe reports the launcher's tag "convres form<F> <C>><N> <AH>x<AW>><OH>x<OW> k<K> s<S> fwd|dgrad tr<kind> img<nimg>" and the
# kernel text of the launch macro.  (try_cr line, geometry part of the tag, NI: the line takes a launch when B % NI == 0)
CR_LINES = (
    ("G_ca_conv2 <1, 16, 8, 2>", "form0 32>64 32x32>16x16 k4 s2", 1),
    ("G_ca_conv3 <2, 0, 8, 4>", "form0 64>128 16x16>8x8 k4 s2", 2),
    ("G_ca_convT2 <4, 0, 8, 2>", "form1 128>64 8x8>16x16 k4 s2", 4),
    ("G_ca_convT3 <2, 16, 4, 1>", "form1 64>32 16x16>32x32 k4 s2", 2),
)
# try_cr line index of each layer launch (csrc/convres.hip, the typedefs under try_cr); None: the stride-1 pair, no such kernel
CR_OF = {
    "enc_conv2": 0, "enc_conv3": 1, "dec_convT2": 2, "dec_convT3": 3,
    "enc_conv2_dgrad": 3, "enc_conv3_dgrad": 2, "dec_convT2_dgrad": 1, "dec_convT3_dgrad": 0,
    "enc_conv4": None, "dec_convT1": None, "enc_conv4_dgrad": None, "dec_convT1_dgrad": None,
}
# ring geometries of WGRAD_RING_GEOS (csrc/wgrad_ring_geos.h) of the CelebA layers: (name, layers, images per ring slot IB)
RING_GEOS = (
    ("ca_conv2", ("enc_conv2_wgrad", "dec_convT3_wgrad"), 1),
    ("ca_conv3", ("enc_conv3_wgrad", "dec_convT2_wgrad"), 2),
    ("ca_conv4", ("enc_conv4_wgrad", "dec_convT1_wgrad"), 4),
)


def _generic(launches):
    return [k for t, k in launches if "gemm_gather_kernel" in k or "gemm_rowtile_kernel" in k or "gemm_small_kernel" in k]


def test_coverage():
    """Over the launches the tests above compared (run the whole module: this test reads their records): every G_ca_* line and
    every ca_* ring geometry in both epilogue modes ran, the generic gather GEMM took the launches the dispatch leaves to it -- the
    fallback of each conv layer and the stride-1 pair at every batch -- and no image-resident / ring kernel ran with its knob off."""
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    recs = [r for r in LR.RECORDS_CELEBA if r[1] in CR_OF or any(r[1] in g[1] for g in RING_GEOS)]
    assert {r[0] for r in recs} >= set(BATCHES), "run the whole module: the compared launches of every batch size are the input of this test"
    hit, fallback, stride1, ring_hit = {}, {}, {}, {}
    for B, layer, knobs, launches in recs:
        cr = [t for t, k in launches if t.startswith("convres ")]
        ring = [k for t, k in launches if "wgrad_ring_kernel" in k]
        reduce_ = [k for t, k in launches if "wgrad_ring_reduce_kernel" in k]
        if layer in CR_OF:
            groups = LAYERS[layer].gf if layer in LAYERS else LAYERS[layer[:-6]].gb
            nimg = groups * B
            line = CR_OF[layer]
            if line is not None and knobs.get("convres", 1) and B % CR_LINES[line][2] == 0:
                assert len(cr) == 1 and CR_LINES[line][1] in cr[0] and cr[0].endswith("img%d" % nimg), (B, layer, knobs, launches)
                assert ("dgrad" in cr[0]) == layer.endswith("_dgrad") and " tr0 " in cr[0], cr
                hit.setdefault(CR_LINES[line][0], []).append((layer, B))
            else:       # knob off, no instantiation divides this batch, or the stride-1 pair: the generic gather GEMM
                assert not cr and _generic(launches), (B, layer, knobs, launches)
                (stride1 if line is None else fallback).setdefault(layer, []).append(B)
        else:
            gname, _, ib = [g for g in RING_GEOS if layer in g[1]][0]
            nimg = 3 * B if layer.startswith("dec_") else B
            if not knobs.get("wgrad_ring", 1) or nimg % ib != 0:
                assert not ring and launches, (B, layer, knobs, launches)
                continue
            assert len(ring) == 1, (B, layer, knobs, launches)
            # wr_atomic_kb = 4096: fp32 atomics into the packed gradient, no reduce launch; 0: partial copies + reduce
            assert bool(reduce_) == (knobs["wr_atomic_kb"] == 0), (B, layer, knobs, launches)
            ring_hit.setdefault((gname, "atomic" if knobs["wr_atomic_kb"] else "copies"), []).append((layer, B))
    for ln, geo, _ in CR_LINES:
        print("convres %-28s %s: %s" % (ln, geo, sorted(set(hit.get(ln, [])))))
    for layer in CR_OF:
        print("gemm_gather %-18s: B %s" % (layer, sorted(set((stride1 if CR_OF[layer] is None else fallback).get(layer, [])))))
    for key in sorted(ring_hit):
        print("wgrad_ring %-10s %-6s: %s" % (key[0], key[1], sorted(set(ring_hit[key]))))
    missing = [ln for ln, _, _ in CR_LINES if ln not in hit]
    missing += [l for l, line in CR_OF.items() if line is not None and l not in fallback]
    missing += [l for l, line in CR_OF.items() if line is None and set(stride1.get(l, [])) != set(BATCHES)]
    missing += [(g[0], m) for g in RING_GEOS for m in ("atomic", "copies") if (g[0], m) not in ring_hit]
    # each ring geometry on both sides (encoder nimg = B, decoder 3B) at the large batch, where a workgroup outruns the ring depth
    missing += [(g[0], l) for g in RING_GEOS for l in g[1] if not any((l, max(BATCHES)) in v for k, v in ring_hit.items() if k[0] == g[0])]
    assert not missing, missing
