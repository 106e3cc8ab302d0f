"""CPU companion of tests/test_gpu_coco_text_modules.py: the float64 restatement of the COCO caption modules
(tests/coco_text_ref.py) with its rounding off IS the oracle; the yardsticks the GPU gates are 4 times of are printed for every
case of the GPU table; and every stand-in fault is shown to be seen: at each case at which the fault is a defect at all, at
least one compared quantity exceeds its gate by a factor of at least 2, while the fault-free stand-in passes every comparison.
Run with -s to read the figures."""
import pytest
import torch

from oracle import mmvae_ref as R
import coco_text_ref as C

SEEN = 2.0            # a fault counts as seen when some quantity is at least this many times its gate
_CACHE = {}


def _dec(form, D, B, T, keep):
    """parameters, inputs, oracle result, emulation, gates, yardsticks of a decoder case; shared by the cases of equal inputs
    and emulation form, never changed"""
    kind = C.dec_emulation_form(form, D)
    key = ("dec", kind, D, B, T, keep)
    if key not in _CACHE:
        P, inp = C.text_params(D), C.make_inputs(D, B, T)
        ref = C.run_decoder(P, inp, keep)
        emu = C.run_decoder(P, inp, keep, rounded=True, form=kind)
        _CACHE[key] = (P, inp, ref, emu) + C.gates(emu, ref) + (kind,)
    return _CACHE[key]


def _enc(D, B, T, knob):
    form = C.enc_form(B, knob)
    key = ("enc", form, D, B, T)
    if key not in _CACHE:
        P, inp = C.text_params(D), C.make_inputs(D, B, T)
        ref = C.run_encoder(P, inp)
        emu = C.run_encoder(P, inp, rounded=True, form=form)
        _CACHE[key] = (P, inp, ref, emu) + C.gates(emu, ref) + (form,)
    return _CACHE[key]


def _same(a, b):
    """every gradient tensor bit for bit"""
    return a["grads"].keys() == b["grads"].keys() and all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"])


@pytest.mark.parametrize("D,B,T,keep", [(100, 23, 7, True), (100, 23, 2, False), (4, 5, 3, True), (124, 17, 1, True)])
def test_decoder_emulation_with_rounding_off_is_the_oracle(D, B, T, keep):
    P, inp = C.text_params(D), C.make_inputs(D, B, T)
    ora = C.run_decoder(P, inp, keep, oracle=True)
    three = C.run_decoder(P, inp, keep, form="three")
    assert torch.equal(ora["sentence"], three["sentence"]) and torch.equal(ora["dz"], three["dz"]) and _same(ora, three)
    # the composed form is the same function written with W_comb: equal to float64 rounding (a few hundred terms of 1e-16)
    comp = C.run_decoder(P, inp, keep, form="composed")
    e = C.errors(comp, ora)
    assert e["sentence"] < 1e-12 and e["dz"] < 1e-12 and e["grads"] < 1e-11, e


@pytest.mark.parametrize("D,B,T", [(100, 23, 7), (4, 4, 1), (100, 5, 2)])
def test_encoder_emulation_with_rounding_off_is_the_oracle(D, B, T):
    P, inp = C.text_params(D), C.make_inputs(D, B, T)
    ora = C.run_encoder(P, inp, oracle=True)
    for form in C.ENC_FORMS:
        emu = C.run_encoder(P, inp, form=form)
        assert torch.equal(ora["encout"], emu["encout"]) and _same(ora, emu)
    # the hidden weights of the one-step reverse direction (and at T = 1 of the forward direction) get an exactly zero gradient
    assert float(ora["grads"][C.ENC + "gru.weight_hh_l0_reverse"].abs().max()) == 0.0
    assert (float(ora["grads"][C.ENC + "gru.weight_hh_l0"].abs().max()) == 0.0) == (T == 1)


@pytest.mark.parametrize("case", C.DEC_CASES, ids=C.dec_id)
def test_decoder_yardsticks_and_faults(case):
    """What the bf16 roundings alone move (the figures the GPU gates are 4 times of) must be of the size bf16 operands give
    (2^-9 relative per operand, a few hundred terms); the fault-free stand-in passes; every fault that is a defect at this
    case is seen."""
    form, D, B, T, keep = case
    P, inp, ref, emu, gate, e, kind = _dec(*case)
    print("YARDSTICK decoder %-28s (%s): sentence %.2e abs, dz %.2e rel, worst gradient tensor %.2e (%s)"
          % (C.dec_id(case), kind, e["sentence"], e["dz"], e["grads"], e["grads_worst"]))
    for k in ("sentence", "dz", "grads"):
        assert 1e-4 < e[k] < 2e-2, (k, e[k])
        assert gate[k] == C.GATE_FACTOR * e[k]
    bad, _ = C.violations(emu, ref, gate)
    assert not bad, bad
    for fault in C.DEC_FAULTS:
        if not C.dec_fault_applies(fault, D, B, T, keep):
            continue
        key = ("decfault", kind, D, B, T, keep, fault)
        if key not in _CACHE:
            if fault == "row16":                 # a defect of the answer, not of the computation: no second run
                got = dict(sentence=C._row16(emu["sentence"], fault), dz=C._row16(emu["dz"], fault), grads=emu["grads"])
            else:
                got = C.run_decoder(P, inp, keep, rounded=True, form=kind, fault=fault)
            bad, fe = C.violations(got, ref, gate)
            _CACHE[key] = (bad, C.worst_ratio(fe, gate, ref))
        bad, ratio = _CACHE[key]
        print("FAULT %-11s decoder %-28s: error / gate sentence %.1f, dz %.1f, worst gradient tensor %.1f"
              % (fault, C.dec_id(case), ratio["sentence"], ratio["dz"], ratio["grads"]))
        assert bad and max(ratio.values()) >= SEEN, (fault, ratio)


@pytest.mark.parametrize("case", C.ENC_CASES, ids=C.enc_id)
def test_encoder_yardsticks_and_faults(case):
    """as for the decoder.  The streamed form's forward pass rounds only the state copy fed to W_hh: its output yardstick is
    small, and exactly zero at T = 1 (h = 0), where the gate is the fp32 floor."""
    D, B, T, knob = case
    P, inp, ref, emu, gate, e, form = _enc(*case)
    print("YARDSTICK encoder %-26s: output %.2e abs, worst gradient tensor %.2e (%s)" % (C.enc_id(case), e["encout"], e["grads"], e["grads_worst"]))
    assert 1e-4 < e["grads"] < 2e-2 and gate["grads"] == C.GATE_FACTOR * e["grads"]
    assert e["encout"] < 2e-2 and gate["encout"] == max(C.GATE_FACTOR * e["encout"], C.FLOOR_ABS)
    if form == "resident":
        assert e["encout"] > 1e-4
    elif T == 1:
        assert e["encout"] == 0.0
    bad, _ = C.violations(emu, ref, gate)
    assert not bad, bad
    for fault in C.ENC_FAULTS:
        if not C.enc_fault_applies(fault, B, T):
            continue
        if fault == "row16":
            got = dict(encout=C._row16(emu["encout"], fault), grads=emu["grads"])
        else:
            got = C.run_encoder(P, inp, rounded=True, form=form, fault=fault)
        bad, fe = C.violations(got, ref, gate)
        ratio = C.worst_ratio(fe, gate, ref)
        print("FAULT %-11s encoder %-26s: error / gate output %.1f, worst gradient tensor %.1f" % (fault, C.enc_id(case), ratio["encout"], ratio["grads"]))
        assert bad and max(ratio.values()) >= SEEN, (fault, ratio)


@pytest.mark.parametrize("form", C.DEC_FORMS)
def test_single_column_comparison_sees_an_ignored_last_latent_column(form):
    """the comparison made for it: the fault-free stand-in passes at both columns, the faulty one misses column D-1 by far"""
    D, B, T, keep = 100, 23, 7, True
    P, inp = C.text_params(D), C.make_inputs(D, B, T)
    cache = {}
    for col in (D - 1, 0):
        bad, _ = C.single_column_violations(lambda Q, i: C.run_decoder(Q, i, keep, rounded=True, form=form), P, D, col, inp, keep, form, cache)
        assert not bad, bad
    bad, fig = C.single_column_violations(lambda Q, i: C.run_decoder(Q, i, keep, rounded=True, form=form, fault="last_column"),
                                          P, D, D - 1, inp, keep, form, cache)
    print("FAULT last_column single-column (%s): sentence %.2e (gate %.2e), dz %.2e (gate %.2e)"
          % (form, fig["sentence"], fig["gate_sentence"], fig["dz"], fig["gate_dz"]))
    assert bad and fig["sentence"] >= SEEN * fig["gate_sentence"]


def test_bit_for_bit_helpers_see_a_swapped_row():
    """permutation_violations / sub_batch_violations on a stand-in whose rows do not depend on each other (a per-row function of
    the inputs): clean as it is, and row16 is reported in the row it lands in"""
    inp = C.make_inputs(8, 23, 2)

    def run(i, fault=None):
        return dict(out=C._row16(i["z"].double().cumsum(1) * i["gs"][:, 0, :8].double(), fault))

    assert not C.permutation_violations(run, inp, ("out",))
    assert not C.sub_batch_violations(run, inp, [list(range(16)), list(range(16, 23))], ("out",))
    assert C.permutation_violations(lambda i: run(i, "row16"), inp, ("out",))
    bad = C.sub_batch_violations(lambda i: run(i, "row16"), inp, [list(range(16)), list(range(16, 23))], ("out",))
    assert bad and all("rows 16..22" in b for b in bad)


def test_dispatch_restatements():
    """the sub-batch sizes the GPU tests use, derived in the docstring of coco_text_ref, as the functions give them"""
    assert [C.f32_gemm_ks(n, 600, 300) for n in (192, 193, 416, 417, 832, 833)] == [8, 4, 4, 2, 2, 1]
    assert C.dec_dispatch(16, 100) == C.dec_dispatch(7, 100) == C.dec_dispatch(23, 100) == C.dec_dispatch(133, 100)
    assert C.enc_dispatch(36, 102, 100)[1] == "tile128" and C.enc_dispatch(20, 102, 100)[1] == "small1" and C.enc_dispatch(4, 102, 100)[1] == "small2"
    assert C.enc_dispatch(28, 102, 100) == C.enc_dispatch(36, 102, 100) != C.enc_dispatch(24, 102, 100)
    assert C.enc_dispatch(23, 102, 100) == C.enc_dispatch(9, 102, 100) != C.enc_dispatch(7, 102, 100)
    assert C.enc_dispatch(16, 7, 100)[0] == "resident" and C.enc_dispatch(16, 7, 100, True)[0] == "streamed"
