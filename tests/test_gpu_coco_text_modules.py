"""The bf16 persistent kernels of the COCO caption GRUs (csrc/coco_text_bf16.hip) on their own, against the float64 oracle:
through the drop-in TextEncoder / TextDecoder of multimodal_vae_amd.coco with the knob coco_module_bf16 = 1, which makes
mmvae_coco_text_{encoder,decoder}_{fwd,bwd} run the training step's kernels on the module's one group of B rows.  The forms
are chosen with the knobs coco_cluster, coco_no_comb, coco_no_comb_bwd and coco_enc_streamed; every test restores every knob.

Reference, emulation, gates, stand-in faults and the bit-for-bit helpers: tests/coco_text_ref.py (its docstring lists what each
kernel rounds); tests/test_cpu_coco_text_ref.py prints the yardsticks of every case below and shows that the comparisons see
each fault.  Gates: 4 times what the float64 emulation of the case's own form differs from the unrounded oracle on the same
inputs; nothing is taken from the engine.  MMVAE_TOL_REPORT=1 prints the engine's error next to every gate.

Which decoder kernels run cannot be read from the probe records (the persistent launches do not go through the tagged
launcher, and coco_text_dec_composed is not part of the C interface); restated from csrc/coco_text.hip coco_dec_cluster /
coco_dec_composed: ranks per 16-row block = coco_cluster (default 8) halved while ceil(blocks / 8) * 8 * ranks exceeds 7/8 of the
compute units (never at the sizes here: at most 16 padded blocks x 8 = 128 of 256), 4 or 8 else one workgroup; composed when
ranks == 8, coco_no_comb == 0 and 200 + D <= 320; composed BPTT when also coco_no_comb_bwd == 0.  test_composed_rule observes
the rule's two sides: at D = 124 the default run equals the coco_no_comb = 1 run bit for bit, at D = 120 it does not.

Cases and the kernels / instantiations they run (KEEP: with keep masks; SAVE: knob value 1, SAVE = false: knob value 2 in
test_*_rows_bit_for_bit, forward only):
  coco_dec_fwd_kernel<KEEP, SAVE>, coco_dec_bwd_kernel<KEEP>                 wg1-*: KEEP at T = 1, 2, 3, 7, no KEEP at T = 102
  coco_dec_fwd_cl_kernel<KEEP, SAVE, 4>, coco_dec_bwd_cl_kernel<KEEP, 4>     cl4-*
  coco_dec_fwd_cl_kernel<KEEP, SAVE, 8>, coco_dec_bwd_cl_kernel<KEEP, 8>     cl8x3-*, comb-D124 (forward and BPTT), comb_fwd-* (BPTT)
  coco_dec_fwd_c8_kernel<KEEP, SAVE> without its MSE branch, coco_comb_kernel   comb-*, comb_fwd-* at D <= 120
  coco_dec_bwd_c8_kernel<KEEP>, dw16_kernel, dout_combine_kernel             comb-* at D <= 120 (T = 1: M = (T-1) R = 0 in coco_text_dec_dout)
  time_sum_bf16_kernel                                                       every decoder case but comb-* at D <= 120
  coco_enc_fwd_res_kernel<SAVE>, coco_enc_bwd_res_kernel                     encoder B = 4, 20, 36
  coco_enc_fwd_kernel<SAVE>, coco_enc_bwd_kernel                             encoder B = 1, 23, and 20 with coco_enc_streamed
  text_tb_kernel                                                             every encoder case (resident: forward; streamed: backward)
  T = 1, 2: no feedback step, first = last step.  B = 23: a full row block and a ragged one of 7; B = 1, 16, 17: one row, a
  full block, a block of one row; B = 133: nine blocks, nblk_pad = 16, a second octet with idle padding workgroups.
  D = 4, 20, 120 (last composed size), 124 (falls to three exchanges).  Encoder: T B reaches the three launcher bands of the resident
  form's bf16 input projection (gemm_small with 2 and with 1 k-slices, the 128-row tile kernel) and KS = 8 and 1 of the streamed
  form's fp32 `lin` (coco_text_ref.enc_dispatch; KS = 4 and 2 of that fp32 GEMM are not reached at these sizes).

Not covered here, and why:
  * the MSE fused into the composed forward's output pass (CocoDecFwdArgs::mse_target): the module entry has no target; it runs
    in the fused step only (A/B knob coco_no_mse_fuse, tests/test_gpu_configs_r2.py::test_coco_caption_kernel_forms_agree);
  * the three-group row layout (R = 3B, the group index of a row in the fused MSE): the module runs one group;
  * side-stream ordering of the deferred weight gradients (coco_text_dec_wgrads behind the encoder's BPTT on st_wgrad2): the
    module issues them inline on its one stream;
  * ranks chosen by the compute-unit limit instead of the knob: needs more than 28 row blocks (B > 448 module rows);
  * the timeout path: no test sets a timeout word, lowers CL_SPIN_MAX or shrinks the co-residency check; a launch that gave up
    would put a NaN into element 0 of sentence / dz, and every comparison asserts finite results.

The forward result with knob value 2 (nothing saved) must equal the saving run bit for bit: SAVE only adds stores.  It does in
coco_dec_fwd_kernel, coco_dec_fwd_cl_kernel<4|8> and both encoder kernels.  It cannot in coco_dec_fwd_c8_kernel: the library is
built with -ffp-contract=fast, and where SAVE stores r, z, n and the products around them the compiler keeps the state update
h = (1 - z) n + z h as two multiplies and an add, where it does not it fuses them (in the gfx950 code of the two instantiations:
6 packed multiplies and 14 fused multiply-adds with SAVE, 4 and 16 without).  The fp32 state then differs in its last bit, and
now and then that flips the bf16 rounding of a published state element (one MI355X run: at T = 102, 66893 of the 703800
sentence elements differ from the saving run, by at most 8.3e-4; at nine row blocks 2091 elements, 4.7e-4; at D = 4 and 120 a
few dozen elements in their last fp32 bit; none at the other ten composed cases).  Both are correct evaluations, so for the
composed forward the unsaved result is compared with the float64 reference under the case's own sentence gate instead
(measured error / gate 0.25 at every case, as for the saving run).

Measured on the MI355X in one run with MMVAE_TOL_REPORT=1, worst error / gate over the cases (the gates in force are 4 times the
yardsticks tests/test_cpu_coco_text_ref.py prints; their range in brackets): decoder sentence 0.26 (yardsticks 1.2e-3 to 3.4e-3
absolute), dz 0.26 (8.9e-4 to 2.2e-3), worst gradient tensor 0.25 (3.4e-3 to 4.6e-3); single latent column: sentence 0.27, dz
column 0.30; encoder output 0.25 (resident 4.1e-4 to 9.7e-4; streamed 0 to 2.2e-4, fp32 floor 2e-5 at T = 1 where the engine is
1e-7 off), worst gradient tensor 0.36 (1.6e-3 to 3.6e-3; the streamed form, whose W_ih gradient reads bf16 captions the
emulation does not round).  The engine's errors sit at the emulation's own figure (ratio 1/4): the emulation rounds what the
kernels round.  187 tests in 11.6 s.
"""
import os

import pytest
import torch

from oracle import mmvae_ref as R
import coco_text_ref as C
from multimodal_vae_amd._lib import knob_default, knobs

pytestmark = pytest.mark.gpu

REPORT = os.environ.get("MMVAE_TOL_REPORT") is not None
_REF, _COL, _MODS = {}, {}, {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _knobs(module_bf16=1, **kw):
    """the bf16 persistent kernels behind the module entry points (coco_module_bf16) and the given knobs for the block"""
    return knobs(coco_module_bf16=module_bf16, **kw)


# ------------------------------------------------------------------------------------------------ references, cached per case
def _dec_setup(form, D, B, T, keep):
    """parameters, inputs, the oracle's result, gates and yardsticks of one decoder case: computed once, shared, never changed"""
    kind = C.dec_emulation_form(form, D)
    base = ("dec", D, B, T, keep)
    if base not in _REF:
        P, inp = C.text_params(D), C.make_inputs(D, B, T)
        _REF[base] = (P, inp, C.run_decoder(P, inp, keep))
    P, inp, ref = _REF[base]
    if base + (kind,) not in _REF:
        _REF[base + (kind,)] = C.gates(C.run_decoder(P, inp, keep, rounded=True, form=kind), ref)
    gate, yard = _REF[base + (kind,)]
    return P, inp, ref, gate, yard, kind


def _enc_setup(D, B, T, knob):
    form = C.enc_form(B, knob)
    base = ("enc", D, B, T)
    if base not in _REF:
        P, inp = C.text_params(D), C.make_inputs(D, B, T)
        _REF[base] = (P, inp, C.run_encoder(P, inp))
    P, inp, ref = _REF[base]
    if base + (form,) not in _REF:
        _REF[base + (form,)] = C.gates(C.run_encoder(P, inp, rounded=True, form=form), ref)
    gate, yard = _REF[base + (form,)]
    return P, inp, ref, gate, yard, form


def _module(which, D, T, P, dev):
    """the drop-in module at latent size D and T steps holding the parameters P (float32)"""
    from multimodal_vae_amd import coco as M
    key = (which, D, T)
    if key not in _MODS:
        for k in [k for k in _MODS if k[0] == which]:
            del _MODS[k]
        m = M.TextDecoder(D, use_cuda=True, sos=R.formula_sos(), steps=T) if which == "dec" else M.TextEncoder(D, steps=T)
        _MODS[key] = m.cuda().train()
    m = _MODS[key]
    pre = C.DEC if which == "dec" else C.ENC
    m.load_state_dict({k[len(pre):]: v for k, v in P.items() if k.startswith(pre)}, strict=True)
    return m


def _dec_full(dec, inp, keep, dev):
    dec.zero_grad(set_to_none=True)
    dec.gru.dropout = 0.1 if keep else 0.0
    z = inp["z"].to(dev).requires_grad_(True)
    sent = dec(z, inp["keep"].to(dev) if keep else None)
    sent.backward(inp["gs"].to(dev))
    torch.cuda.synchronize()
    return dict(sentence=sent.detach().cpu(), dz=z.grad.detach().cpu(),
                grads={C.DEC + n: p.grad.detach().cpu() for n, p in dec.named_parameters()})


def _dec_forward(dec, inp, keep, dev):
    dec.gru.dropout = 0.1 if keep else 0.0
    with torch.no_grad():
        sent = dec(inp["z"].to(dev), inp["keep"].to(dev) if keep else None)
    torch.cuda.synchronize()
    return sent.cpu()


def _enc_full(enc, inp, dev):
    enc.zero_grad(set_to_none=True)
    mu, lv = enc(inp["text"].to(dev))
    out = torch.cat((mu, lv), 1)
    out.backward(inp["ge"].to(dev))
    torch.cuda.synchronize()
    return dict(encout=out.detach().cpu(), grads={C.ENC + n: p.grad.detach().cpu() for n, p in enc.named_parameters()})


def _enc_forward(enc, inp, dev):
    with torch.no_grad():
        mu, lv = enc(inp["text"].to(dev))
    torch.cuda.synchronize()
    return torch.cat((mu, lv), 1).cpu()


def _report(what, e, gate, yard, ref):
    if REPORT:
        r = C.worst_ratio(e, gate, ref)
        print("TOL coco text %s: " % what + ", ".join("%s %.2e (emulation %.2e, gate %.2e, ratio %.2f)" % (k, e[k], yard[k], gate[k], r[k])
                                                      for k in C.quantities(ref)) + " [worst gradient: %s]" % e["grads_worst"])


# ------------------------------------------------------------------------------------------------ decoder
@pytest.mark.parametrize("case", C.DEC_CASES, ids=C.dec_id)
def test_decoder_matches_float64(case):
    """sentence element-wise, dz and every parameter gradient by relative L2, random z, injected keep masks, random upstream
    gradients; finite results (a cluster launch that gave up waiting marks element 0 with a NaN)"""
    dev = _dev()
    form, D, B, T, keep = case
    P, inp, ref, gate, yard, kind = _dec_setup(*case)
    dec = _module("dec", D, T, P, dev)
    with _knobs(**C.DEC_FORM_KNOBS[form][0]):
        got = _dec_full(dec, inp, keep, dev)
    assert bool(torch.isfinite(got["sentence"]).all()) and bool(torch.isfinite(got["dz"]).all())
    bad, e = C.violations(got, ref, gate, C.dec_id(case))
    _report("decoder %s (%s)" % (C.dec_id(case), kind), e, gate, yard, ref)
    assert not bad, bad


@pytest.mark.parametrize("case", C.DEC_CASES, ids=C.dec_id)
def test_decoder_rows_bit_for_bit(case):
    """a wrong `r0 + row < R` guard, a rank that reads its neighbour's block or a stale exchange buffer moves a few rows of a
    tensor: no tolerance sees that, equality of a row's result across row orders and batches does.  Also: the forward result
    without saving (knob value 2) is the saving run's."""
    dev = _dev()
    form, D, B, T, keep = case
    P, inp, ref, gate, _, kind = _dec_setup(*case)
    dec = _module("dec", D, T, P, dev)
    form_knobs = C.DEC_FORM_KNOBS[form][0]
    cluster = form_knobs.get("coco_cluster", knob_default("coco_cluster"))

    def run(i):
        r = _dec_full(dec, i, keep, dev)
        return dict(sentence=r["sentence"], dz=r["dz"])

    with _knobs(**form_knobs):
        full = run(inp)
        assert not C.permutation_violations(run, inp, ("sentence", "dz"), full)
        sets = [s for s in (list(range(min(16, B))), list(range(16, B))) if 0 < len(s) < B
                and C.dec_dispatch(len(s), D, cluster) == C.dec_dispatch(B, D, cluster)]
        assert B <= 16 or len(sets) == 2, "the sub-batches of %d rows do not keep the dispatch" % B
        assert not C.sub_batch_violations(run, inp, sets, ("sentence", "dz"), full)
    with _knobs(2, **form_knobs):
        nosave = _dec_forward(dec, inp, keep, dev)
        with pytest.raises(RuntimeError, match="saved nothing"):          # the backward entry refuses (MMVAE_EINVAL)
            _dec_full(dec, inp, keep, dev)
    if kind == "composed":      # (module docstring: the two instantiations of coco_dec_fwd_c8_kernel fuse the state update differently)
        err = float((nosave.double() - ref["sentence"]).abs().max())
        if REPORT:
            print("TOL coco text decoder %s without saving: sentence %.2e (gate %.2e), %d elements differ from the saving run by at most %.2e"
                  % (C.dec_id(case), err, gate["sentence"], int((nosave != full["sentence"]).sum()), float((nosave - full["sentence"]).abs().max())))
        assert bool(torch.isfinite(nosave).all()) and err <= gate["sentence"], (err, gate["sentence"])
    else:
        assert torch.equal(nosave, full["sentence"]), "the forward pass without saving differs from the saving one"


@pytest.mark.parametrize("case", C.DEC_CASES, ids=C.dec_id)
def test_decoder_single_latent_column(case):
    """only latent column D-1 (then only column 0) reaches the decoder, scaled by 4: a dropped last k-step or last column of a
    z-term gives the z-independent answer"""
    dev = _dev()
    form, D, B, T, keep = case
    P, inp, _, _, _, kind = _dec_setup(*case)

    def run(Q, i):
        return _dec_full(_module("dec", D, T, Q, dev), i, keep, dev)

    with _knobs(**C.DEC_FORM_KNOBS[form][0]):
        for col in (D - 1, 0):
            bad, fig = C.single_column_violations(run, P, D, col, inp, keep, kind, cache=_COL)
            if REPORT:
                print("TOL coco text decoder %s column %d: sentence %.2e (gate %.2e), dz column %.2e (gate %.2e)"
                      % (C.dec_id(case), col, fig["sentence"], fig["gate_sentence"], fig["dz"], fig["gate_dz"]))
            assert not bad, bad


def test_composed_rule():
    """200 + D <= 320 decides between the composed and the three-exchange cluster of 8: at D = 124 switching the composed form
    off changes nothing, at D = 120 it changes the rounding"""
    dev = _dev()
    for D, same in ((124, True), (120, False)):
        P, inp, _, _, _, _ = _dec_setup("comb", D, 23, 7, True)
        dec = _module("dec", D, 7, P, dev)
        with _knobs():
            a = _dec_forward(dec, inp, True, dev)
        with _knobs(coco_no_comb=1):
            b = _dec_forward(dec, inp, True, dev)
        assert torch.equal(a, b) == same, D


# ------------------------------------------------------------------------------------------------ encoder
@pytest.mark.parametrize("case", C.ENC_CASES, ids=C.enc_id)
def test_encoder_matches_float64(case):
    """encoder output element-wise, every parameter gradient by relative L2 (the hidden weights of the reverse direction, and at
    T = 1 of the forward direction, exactly zero), random captions and upstream gradients"""
    dev = _dev()
    D, B, T, knob = case
    P, inp, ref, gate, yard, form = _enc_setup(*case)
    enc = _module("enc", D, T, P, dev)
    with _knobs(coco_enc_streamed=knob):
        got = _enc_full(enc, inp, dev)
    assert bool(torch.isfinite(got["encout"]).all())
    bad, e = C.violations(got, ref, gate, C.enc_id(case))
    _report("encoder %s" % C.enc_id(case), e, gate, yard, ref)
    assert not bad, bad


@pytest.mark.parametrize("case", C.ENC_CASES, ids=C.enc_id)
def test_encoder_rows_bit_for_bit(case):
    """row permutations at the same batch size; sub-batches at the sizes that keep the form and the launcher's choice for the
    input projection (coco_text_ref.enc_dispatch); the forward result without saving is the saving run's"""
    dev = _dev()
    D, B, T, knob = case
    P, inp, _, _, _, _ = _enc_setup(*case)
    enc = _module("enc", D, T, P, dev)

    def run(i):
        return dict(encout=_enc_full(enc, i, dev)["encout"])

    with _knobs(coco_enc_streamed=knob):
        full = run(inp)
        assert not C.permutation_violations(run, inp, ("encout",), full)
        ok = [n for n in range(1, B) if C.enc_dispatch(n, T, D, knob) == C.enc_dispatch(B, T, D, knob)]
        sets = [list(range(ok[0])), list(range(B - ok[0], B)), list(range(B - ok[-1], B))] if ok else []
        assert not C.sub_batch_violations(run, inp, sets, ("encout",), full)
    with _knobs(2, coco_enc_streamed=knob):
        nosave = _enc_forward(enc, inp, dev)
        with pytest.raises(RuntimeError, match="saved nothing"):
            _enc_full(enc, inp, dev)
    assert torch.equal(nosave, full["encout"]), "the forward pass without saving differs from the saving one"
