"""CPU companion of tests/test_gpu_text_modules.py: the float64 restatement of the text modules (tests/text_ref.py) with its
rounding off IS the oracle; the yardsticks the GPU gates are built from are printed; and the comparisons are shown to see three
faults a text kernel can have, each put into a stand-in engine (the bf16-operand emulation) one at a time, while the fault-free
stand-in passes every comparison.  Run with -s to read the figures."""
import pytest
import torch

from oracle import mmvae_ref as R
import text_ref as TR

ALL_SIZES = TR.SIZES + (100,)
_CACHE = {}


def _setup(D):
    """parameters, inputs, gates and the oracle's result of one latent size: computed once, shared by the tests, never changed"""
    if D not in _CACHE:
        P = TR.text_params(D)
        inp = TR.make_inputs(D)
        gate, ref, emu_err = TR.gates(P, inp)
        _CACHE[D] = (P, inp, gate, ref, emu_err)
    return _CACHE[D]


@pytest.mark.parametrize("D", ALL_SIZES)
def test_emulation_with_rounding_off_is_the_oracle(D):
    P, inp, _, ref, _ = _setup(D)
    P64 = TR.f64(P)
    keep = [inp["keep"][t].double() for t in range(TR.T)]
    with torch.no_grad():
        for ft in (inp["force"], None):
            w0, t0 = R.multimnist_text_decoder(P64, inp["z"].double(), True, keep, ft)
            w1, t1 = TR.text_decoder(P64, inp["z"].double(), keep, ft)
            assert torch.equal(w0, w1) and torch.equal(t0, t1)
        w0, _ = R.multimnist_text_decoder(P64, inp["z"].double(), False)
        w1, _ = TR.text_decoder(P64, inp["z"].double())
        assert torch.equal(w0, w1)
        assert torch.equal(R.multimnist_text_encoder(P64, inp["text"]), TR.text_encoder(P64, inp["text"]))
        # and the result the gates are measured against (run_full) is that oracle's
        assert torch.equal(ref["words"], R.multimnist_text_decoder(P64, inp["z"].double(), True, keep, inp["force"])[0])


@pytest.mark.parametrize("D", ALL_SIZES)
def test_yardsticks(D):
    """What the bf16 rounding of the GEMM operands alone moves, per latent size: the figures the GPU gates are 4 times of.  They
    must be of the size bf16 operands give (2^-9 relative per operand, a few hundred terms): a gate built from a figure far
    above that would see nothing, one far below it would be a rounding accident."""
    _, _, gate, _, e = _setup(D)
    print("YARDSTICK D=%3d: words %.2e abs, encoder output %.2e abs, dz %.2e rel, worst gradient tensor %.2e (%s)"
          % (D, e["words"], e["encout"], e["dz"], e["grads"], e["grads_worst"]))
    for k in ("words", "encout", "dz", "grads"):
        assert 1e-4 < e[k] < 2e-2, (D, k, e[k])
        assert gate[k] == TR.GATE_FACTOR * e[k]


def _stand_in(fault):
    return lambda Q, inp: TR.run_full(Q, inp, rounded=True, fault=fault)


def _columns(D):
    return (D - 1,) if D == 1 else (D - 1, 0)


@pytest.mark.parametrize("D", ALL_SIZES)
def test_fault_free_stand_in_passes(D):
    P, inp, gate, ref, _ = _setup(D)
    bad, _ = TR.violations(TR.run_full(P, inp, rounded=True), ref, gate)
    assert not bad, bad
    assert not TR.row_independence_violations(lambda i: TR.run_forward(P, i, rounded=True, rowwise=True), inp)
    assert not TR.row_independence_violations(lambda i: TR.run_forward(P, i, rounded=True, rowwise=True, free_running=True), inp)
    for col in _columns(D):
        bad, _ = TR.single_column_violations(_stand_in(None), P, D, col, inp)
        assert not bad, bad


@pytest.mark.parametrize("D", ALL_SIZES)
def test_gates_see_an_ignored_last_latent_column(D):
    """seen by the single-column comparison at every size (that is what it is for); the plain comparison is printed too"""
    P, inp, gate, ref, _ = _setup(D)
    bad, fig = TR.single_column_violations(_stand_in("last_column"), P, D, D - 1, inp)
    plain, _ = TR.violations(TR.run_full(P, inp, rounded=True, fault="last_column"), ref, gate)
    print("FAULT last_column D=%3d: single-column words %.2e (gate %.2e), dz %.2e (gate %.2e); plain comparison misses %d checks"
          % (D, fig["words"], fig["gate_words"], fig["dz"], fig["gate_dz"], len(plain)))
    assert bad
    assert fig["words"] > fig["gate_words"]
    assert plain, "the plain comparison does not see it at D = %d" % D


@pytest.mark.parametrize("D", ALL_SIZES)
def test_gates_see_a_row_answered_with_another_rows_result(D):
    P, inp, gate, ref, _ = _setup(D)
    rows = TR.row_independence_violations(lambda i: TR.run_forward(P, i, rounded=True, rowwise=True, fault="row16"), inp)
    plain, e = TR.violations(TR.run_full(P, inp, rounded=True, fault="row16"), ref, gate)
    print("FAULT row16 D=%3d: row comparison misses %d checks; plain words %.2e (gate %.2e), encoder output %.2e (gate %.2e)"
          % (D, len(rows), e["words"], gate["words"], e["encout"], gate["encout"]))
    assert rows
    assert any("rows 16..22 in front" in b for b in rows) and not any("first 16 rows" in b for b in rows)
    assert plain


@pytest.mark.parametrize("D", ALL_SIZES)
def test_gates_see_an_ignored_keep_mask(D):
    P, inp, gate, ref, _ = _setup(D)
    plain, e = TR.violations(TR.run_full(P, inp, rounded=True, fault="mask3"), ref, gate)
    print("FAULT mask3 D=%3d: words %.2e (gate %.2e), dz %.2e (gate %.2e), worst gradient tensor %.2e (gate %.2e)"
          % (D, e["words"], gate["words"], e["dz"], gate["dz"], e["grads"], gate["grads"]))
    assert plain
    assert e["words"] > gate["words"]
