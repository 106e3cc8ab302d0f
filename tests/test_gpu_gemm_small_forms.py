"""gemm_small_kernel (csrc/gemm_small.hip): classifier.0's data gradient against float64, and the prefetching form against the
form it replaced, bit for bit.

Knob gemm_small_prefetch: 0 launches gemm_small_kernel_v0 (a two-buffer ping-pong, every epilogue operand loaded where it is
used), 2 .. 4 gemm_small_kernel with that many chunks of both operands in flight per wave (default 2).  Both forms give a wave the
same chunks in the same order and sum the waves of a workgroup in the same order, so every stored tensor is equal bit for bit; the
sums that go through float atomics (d_red, d_colsum) depend on the order of the workgroups and take the 2^-16 gate of
tests/test_gpu_layers.py against float64.

Batches 7, 8, 12 (rows 14, 16, 24 at two variants; 21, 24, 36 for the three decoder passes): below one 16-row fragment, exactly
one, and a partial second one.  Chunks of K per wave (csrc/gemm_small.hip try_launch_gemm_small): 4 for classifier.0 and the
upsample data gradient (K = 1024, 4 waves), 3 and 4 for classifier.0's data gradient (K = 400: 7 chunks over 2 waves), 2 for
upsample.0 (K = 104) and the data gradients of classifier.3 / classifier.6 (4 chunks over 2 waves): depth 2 wraps the ring with and
without a remainder, depth 3 wraps with one, depth 4 holds every range, and a range is shorter than, equal to and longer than
the depth.  One more case at n_latents = 99 (batch 7): N = 198 and N = 99 are no multiples of 4, so classifier.6, its data
gradient's operand rows and the upsample data gradient take the prefetching form's element-wise epilogue."""
import pytest
import torch

import layer_ref as LR
import gemm_small_forms_ref as GR

pytestmark = pytest.mark.gpu

BATCHES = (7, 8, 12)
KNOB = "gemm_small_prefetch"
DEPTHS = (2, 3, 4)
_H = {}


def _harness(B, D=100):
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    if (B, D) not in _H:
        _H[(B, D)] = LR.LayerHarness(B, n_latents=D)
    return _H[(B, D)]


def _put_fc1_dgrad(h, B, seed):
    dy1, W1, r4, aff, mr = GR.fc1_dgrad_operands(B, seed)
    h.set_weight("image_encoder.classifier.0.weight", W1)
    h.put("dy1", dy1)
    h.put("r4", r4)
    h.put("aff_e2", aff, torch.float32)
    h.put("mr_e2", mr, torch.float32)
    return GR.ref_fc1_dgrad(dy1, W1, r4, aff, mr)


def _run_fc1_dgrad(h, B, **knobs):
    h.zero("db4", 2 * B * 1024, torch.bfloat16)
    h.zero("red_e2", LR.STAT_SLOTS * 256 * 2, torch.float32)
    launches = h.run("enc_fc1_dgrad", **knobs)
    assert any("gemm_small_kernel" in k for _, k in launches), launches
    return h.get("db4", (2 * B, 2, 2, 256)), h.stats("red_e2", 1, 256), launches


@pytest.mark.parametrize("B", BATCHES)
def test_fc1_dgrad_against_float64(B):
    """both forms of classifier.0's data gradient: gate_elements for db4, gate_sums for the BatchNorm-backward sums"""
    h = _harness(B)
    for seed in LR.SEEDS:
        acc, v, red, red_abs = _put_fc1_dgrad(h, B, seed)
        for knob in (0,) + DEPTHS:
            got, sums, launches = _run_fc1_dgrad(h, B, **{KNOB: knob})
            tag = "enc_fc1_dgrad B=%d seed %d knob %d" % (B, seed, knob)
            LR.gate_elements(got, v, acc, tag, launches)
            LR.gate_sums(sums, red, red_abs, tag + " d_red", launches)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _forms_agree(h, layer, outputs, sums, what):
    """outputs: [(buffer, shape, dtype)] compared bit for bit between knob 0 and every depth; sums: [(zero, read, ref, mag)] gated
    against float64 under every knob value"""
    res = {}
    for knob in (0,) + DEPTHS:
        for name, shape, dtype in outputs:
            n = 1
            for s in shape:
                n *= s
            h.zero(name, n, dtype)
        for zero, _, _, _ in sums:
            zero()
        launches = h.run(layer, **{KNOB: knob})
        kernels = [k for _, k in launches if "gemm_small_kernel" in k]
        assert len(kernels) == 1 and ("gemm_small_kernel_v0" in kernels[0]) == (knob == 0), (what, knob, launches)
        res[knob] = [h.get(name, shape, dtype) for name, shape, dtype in outputs]
        for _, read, ref, mag in sums:
            LR.gate_sums(read(), ref, mag, "%s knob %d sums" % (what, knob), launches)
    for (name, shape, dtype), old in zip(outputs, res[0]):
        assert float(old.float().abs().max()) > 0, (what, name, "the reference form wrote nothing")
    for depth in DEPTHS:
        for (name, shape, dtype), old, new in zip(outputs, res[0], res[depth]):
            same = _bits(old) == _bits(new)
            assert bool(same.all()), (what, name, "depth %d: %d of %d elements differ from the replaced form, first %s: %s vs %s" % (
                depth, int((~same).sum()), same.numel(), torch.nonzero(~same)[:4].tolist(), new[~same][:4].tolist(), old[~same][:4].tolist()))


@pytest.mark.parametrize("B,D", [(B, 100) for B in BATCHES] + [(7, 99)])
def test_prefetch_form_equals_replaced_form_bitwise(B, D):
    h = _harness(B, D)
    rows = 2 * B
    bf, f32 = torch.bfloat16, torch.float32
    pre, up = "image_encoder.classifier.", "image_decoder.upsample.0."
    colsum = lambda n: (lambda: h.zero("tmp_f32", n, f32), lambda: h.get("tmp_f32", (n,), f32))
    for seed in LR.SEEDS:
        tag = "B=%d seed %d" % (B, seed)
        g = LR.gen(seed, 14, B)
        tern = lambda shape, d=0.5: LR.ternary(shape, d, g)
        ibias = lambda n: torch.randint(-2, 3, (n,), generator=g).double()
        keep = lambda shape: (torch.rand(shape, generator=g) < 0.9).to(torch.uint8)
        W3, W6, Wu = tern((200, 400), 0.25), tern((2 * D, 200), 0.25), tern((1024, D), 0.25)
        for n, t in ((pre + "0.bias", ibias(400)), (pre + "3.weight", W3), (pre + "6.weight", W6), (up + "weight", Wu), (up + "bias", ibias(1024))):
            h.set_weight(n, t)
        m1, m2 = keep((rows, 400)), keep((rows, 200))
        h.put("m1", m1, torch.uint8)
        h.put("m2", m2, torch.uint8)

        # classifier.0's data gradient (its operands also set classifier.0's weight for the forward below)
        acc, v, red, red_abs = _put_fc1_dgrad(h, B, seed)
        _forms_agree(h, "enc_fc1_dgrad", [("db4", (rows, 1024), bf)],
                     [(lambda: h.zero("red_e2", LR.STAT_SLOTS * 512, f32), lambda: h.stats("red_e2", 1, 256), red, red_abs)], "enc_fc1_dgrad " + tag)
        h.put("a4", tern((B, 2, 2, 256)))
        _forms_agree(h, "enc_fc1", [("y1", (rows, 400), bf), ("ay1", (rows, 400), bf)], [], "enc_fc1 " + tag)

        de, r2, r1 = tern((rows, 2 * D)), LR.eighths((rows, 200), g), LR.eighths((rows, 400), g)
        de_rows = torch.zeros(rows, (2 * D + 7) // 8 * 8, dtype=torch.float64)
        de_rows[:, :2 * D] = de
        h.put("d_encout", de_rows); h.put("y2", r2); h.put("y1", r1)
        h.set_weight(pre + "6.bias", ibias(2 * D))
        h.put("ay2", tern((rows, 200)))
        _forms_agree(h, "enc_fc3", [("tmp_f32", (rows, 2 * D), f32)], [], "enc_fc3 " + tag)
        v3 = (de @ W6) * LR.dswish(r2) * m2 * (1.0 / 0.9)
        _forms_agree(h, "enc_fc3_dgrad", [("dy2", (rows, 200), bf)], [colsum(200) + (v3.sum(0), v3.abs().sum(0))], "enc_fc3_dgrad " + tag)
        d2 = tern((rows, 200))
        h.put("dy2", d2)
        v2 = (d2 @ W3) * LR.dswish(r1) * m1 * (1.0 / 0.9)
        _forms_agree(h, "enc_fc2_dgrad", [("dy1", (rows, 400), bf)], [colsum(400) + (v2.sum(0), v2.abs().sum(0))], "enc_fc2_dgrad " + tag)

        ldz = (D + 1 + 7) // 8 * 8
        z = torch.zeros(3 * B, ldz, dtype=torch.float64)
        z[:, :D] = tern((3 * B, D))
        z[:, D] = 1.0
        h.put("z_bf", z)
        _forms_agree(h, "dec_up", [("u", (3 * B, 1024), bf), ("au", (3 * B, 1024), bf)], [], "dec_up " + tag)
        h.put("du", tern((rows, 2, 2, 256)))
        _forms_agree(h, "dec_up_dgrad", [("tmp_f32", (rows, D), f32)], [], "dec_up_dgrad " + tag)
