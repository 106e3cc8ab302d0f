"""Layer-level tests of the staged forms of the CelebA conv kernels: what the default step runs whenever B % 4 == 0
(csrc/celeba.hip stage_fwd_* / stage_bwd_*, csrc/gemm.h GatherTransform kinds 1 and 2, csrc/convres.hip TR 1 / TR 2), replayed
through mmvae_celeba_bench_layer under the <layer>_staged / <layer>_dgrad_staged names and compared with float64
(tests/layer_ref.py).  Every gate is derived from the number formats.

Kind 1 (enc_conv3_staged, dec_convT2_staged, dec_convT3_staged): the operand is the RAW output of the layer below (eighths), the
launch makes the BatchNorm tables of that layer from its column statistics (written by the test, exact in fp32), stages
Swish(BatchNorm(r)), leaves the staged tensor behind and convolves it with ternary weights.
  (a) the by-product and the written (scale, shift) / (mean, rstd) tables against float64 from the same statistics:
      layer_ref.gate_stage_fwd (one bf16 ulp + 32 fp32 roundings, counted there); tables: 11 to 16 roundings, counted at the check;
  (b) the conv output and its column statistics against the float64 conv of the READ-BACK by-product (bf16 values are exact in
      float64): 2^-8 |ref| + K 2^-24 sum |terms| (layer_ref.gate_stage_conv / gate_stage_colstats).
Kind 2 (enc_conv3_dgrad_staged, enc_conv2_dgrad_staged, dec_convT3_dgrad_staged, dec_convT2_dgrad_staged): the operand is db, the
launch applies the BatchNorm backward while staging, writes dr back in place and adds dgamma / dbeta.  The operands
(layer_ref.staged_bwd_operands) keep every coefficient and dr itself on a dyadic grid that fp32 holds exactly:
  the in-place dr against float64 within one bf16 ulp (2^-8 |ref|), dgamma / dbeta within 2^-16 sum |slot sums|;
  the data gradient against the float64 data gradient of the read-back dr (an exact fp32 accumulation again) with the Tier B
  epilogue gate of tests/test_gpu_layers.py.

Batches: multiples of 4 only (the step stages nothing otherwise): 4, 8 and the large batch of tests/test_gpu_celeba_layers.py.
The probe's tag of every launch must carry tr1 / tr2."""
import pytest
import torch

import layer_ref as LR
from layer_ref import LAYERS_CELEBA as LAYERS

pytestmark = pytest.mark.gpu

BATCHES = (4, 8, 256)
# BatchNorm that follows each conv layer (celeba/model.py:103-148)
BN_OF = {"enc_conv2": "image_encoder.features.3", "enc_conv3": "image_encoder.features.6", "dec_convT1": "image_decoder.hallucinate.1",
         "dec_convT2": "image_decoder.hallucinate.4", "dec_convT3": "image_decoder.hallucinate.7"}
BELOW = {"enc_conv3": "enc_conv2", "dec_convT2": "dec_convT1", "dec_convT3": "dec_convT2"}
_H = {}


def _harness(B):
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    if B not in _H:
        _H.clear()
        torch.cuda.empty_cache()
        _H[B] = LR.celeba_harness(B)
    return _H[B]


def _report(what, err, gate):
    if LR.REPORT:
        print("STAGED %s: worst err/gate %.3f" % (what, float((err / gate.clamp_min(1e-30)).max())))


def _within(got, ref, gate, what, launches):
    got = got.double().cpu()
    err = (got - ref).abs()
    _report(what, err, gate)
    bad = ~(err <= gate)
    assert not bool(bad.any()), (what, launches, "%d of %d outside the gate; first %s got %s want %s gate %s" % (
        int(bad.sum()), bad.numel(), torch.nonzero(bad)[:6].tolist(), got[bad][:6].tolist(), ref[bad][:6].tolist(), gate[bad][:6].tolist()))


def _tagged(launches, kind, dgrad):
    cr = [t for t, k in launches if t.startswith("convres ")]
    assert len(cr) == 1 and (" tr%d " % kind) in cr[0] and ((" dgrad " in cr[0]) == dgrad), launches


@pytest.mark.parametrize("name", list(BELOW))
@pytest.mark.parametrize("B", BATCHES)
def test_staged_forward(B, name):
    h = _harness(B)
    L, bn = LAYERS[name], BN_OF[BELOW[name]]
    G, nimg, count = L.gf, L.gf * B, B * L.ih * L.ih
    seed = 0
    g = LR.gen(seed, list(LAYERS).index(name), 5, nimg)
    w = LR.ternary(LR.weight_shape(L), LR.W_DENSITY, g)
    r = LR.eighths((nimg, L.ih, L.ih, L.cin), g)
    gamma = torch.tensor([1.0, 2.0, -1.0])[torch.randint(0, 3, (L.cin,), generator=g)].double()
    beta = torch.randint(-1, 2, (L.cin,), generator=g).double()
    stats = LR.slot_stats(r, G)
    st_name = L.red.replace("red", "st")
    what = "%s_staged B=%d" % (name, B)
    h.set_weight(L.param, w)
    h.set_weight(bn + ".weight", gamma)
    h.set_weight(bn + ".bias", beta)
    h.put(L.r, r)
    h.put(st_name, stats, torch.float32)
    for nm, n, dt in ((L.x, r.numel(), torch.bfloat16), (L.aff, G * L.cin * 2, torch.float32), (L.mr, G * L.cin * 2, torch.float32),
                      (L.out, nimg * L.oh * L.oh * L.cout, torch.bfloat16), (L.stats, G * LR.STAT_SLOTS * L.cout * 2, torch.float32)):
        h.zero(nm, n, dt)
    launches = h.run(name + "_staged")
    _tagged(launches, 1, False)
    # (a) tables and by-product
    scale, shift, mean, rstd = LR.ref_bn_tables(stats, count, gamma, beta)
    aff = h.get(L.aff, (G, L.cin, 2), torch.float32)
    mr = h.get(L.mr, (G, L.cin, 2), torch.float32)
    # fp32 roundings of csrc/bn_dev.h bn_channel_tables, each relative to the magnitude it is gated with:
    #   mean  : 15 additions of the 16 slot sums (partial sums bounded by count * max |r| = 4 count) + the division = 16, of 4
    #   rstd  : 15 additions (all terms positive) + division of the sum of squares, mean^2, the subtraction (mean^2 << variance
    #           for these operands: no cancellation), + eps, rsqrt = 20 roundings of the variance, halved by the -1/2 power = 10,
    #           and rsqrt's own = 11 of rstd
    #   scale : rstd's 11 + the product with gamma = 12 of |scale|
    #   shift : mean's 16 (of 4 |scale|) + scale's 12 + the product (of |mean scale|) + the subtraction (of |shift| <= |beta| +
    #           |mean scale|): at most 16 of (4 + |mean|) |scale| + |beta|
    e = LR.EPS32
    _within(aff[..., 0], scale, 12 * e * scale.abs(), what + " scale", launches)
    _within(aff[..., 1], shift, 16 * e * ((mean.abs() + 4) * scale.abs() + beta.abs()[None]), what + " shift", launches)
    _within(mr[..., 0], mean, 16 * e * 4 * torch.ones_like(mean), what + " mean", launches)
    _within(mr[..., 1], rstd, 11 * e * rstd, what + " rstd", launches)
    a_ref, _ = LR.ref_stage_fwd(r, scale, shift, G)
    a_got = h.get(L.x, r.shape)
    _within(a_got, a_ref, LR.gate_stage_fwd(r, scale, shift, mean, beta, a_ref, G), what + " by-product", launches)
    # (b) the conv of what was staged
    a_rb = a_got.double().cpu()
    ref, absterms = LR.ref_forward(L, a_rb, w), LR.ref_abs_terms(L, a_rb, w)
    _within(h.get(L.out, ref.shape), ref, LR.gate_stage_conv(L, ref, absterms), what + " output", launches)
    _within(h.stats(L.stats, G, L.cout), LR.ref_colstats(ref, G), LR.gate_stage_colstats(L, ref, absterms, G), what + " colstats", launches)


@pytest.mark.parametrize("name", ["enc_conv3", "enc_conv2", "dec_convT3", "dec_convT2"])
@pytest.mark.parametrize("B", BATCHES)
def test_staged_dgrad(B, name):
    h = _harness(B)
    L, bn = LAYERS[name], BN_OF[name]
    G, nimg, count = L.gb, L.gb * B, B * L.oh * L.oh
    seed = 0
    g = LR.gen(seed, list(LAYERS).index(name), 6, nimg)
    w = LR.ternary(LR.weight_shape(L), LR.W_DENSITY, g)
    db, r, red, mr, gamma = LR.staged_bwd_operands(L, nimg, G, count, g)
    dr, dgamma, dbeta, mag_g, mag_b = LR.ref_bn_backward(db, r, red, mr, gamma, count, G)
    assert torch.equal(dr.float().double(), dr)
    own_mr, own_red = L.stats.replace("st", "mr"), L.stats.replace("st", "red")
    what = "%s_dgrad_staged B=%d" % (name, B)
    goff, _, _ = h.param_range(bn + ".weight")
    boff, _, _ = h.param_range(bn + ".bias")
    h.set_weight(L.param, w)
    h.set_weight(bn + ".weight", gamma)
    h.put(L.dy, db)
    h.put(L.out, r)                 # the layer's own raw output: the tensor its BatchNorm normalised (stage_bwd_*: tr.r)
    h.put(own_red, red, torch.float32)
    h.put(own_mr, mr, torch.float32)
    # epilogue of the layer below (Swish' and its BatchNorm-backward sums), as in the plain data-gradient test
    r_in = LR.eighths((nimg, L.ih, L.ih, L.cin), g)
    aff_in, mr_in = LR.dyadic_tables(G, L.cin, g) if L.aff else (None, None)
    h.put(L.r, r_in)
    if L.aff:
        h.put(L.aff, aff_in, torch.float32)
        h.put(L.mr, mr_in, torch.float32)
        h.zero(L.red, G * LR.STAT_SLOTS * L.cin * 2, torch.float32)
    h.zero(L.dx, nimg * L.ih * L.ih * L.cin, torch.bfloat16)
    h.st.grads.zero_()
    launches = h.run(name + "_dgrad_staged")
    _tagged(launches, 2, True)
    # in-place dr, dgamma / dbeta
    dr_got = h.get(L.dy, dr.shape)
    _within(dr_got, dr, 2.0 ** -8 * dr.abs(), what + " dr", launches)
    C = L.cout
    LR.gate_sums(h.st.grads[goff:goff + C], dgamma, mag_g, what + " dgamma", launches)
    LR.gate_sums(h.st.grads[boff:boff + C], dbeta, mag_b, what + " dbeta", launches)
    # data gradient of what was stored
    dr_rb = dr_got.double().cpu()
    acc = LR.ref_dgrad_acc(L, dr_rb, w)
    assert bool((acc * 256 == (acc * 256).round()).all()) and float(acc.abs().max()) * 256 < 2 ** 24, what
    v, red_in, red_abs = LR.ref_dgrad_epilogue(acc, r_in, aff_in, mr_in, G)
    LR.gate_elements(h.get(L.dx, acc.shape), v, acc, what + " data gradient", launches)
    if L.red:
        LR.gate_sums(h.stats(L.red, G, L.cin), red_in, red_abs, what + " d_red", launches)

