"""The MultiMNIST text encoder and decoder kernels on their own (csrc/text.hip through the drop-in TextEncoder / TextDecoder of
multimodal_vae_amd.multimnist: mmvae_mm_text_{encoder,decoder}_{fwd,bwd}) against the float64 oracle, at the latent sizes of
tests/test_gpu_latent_sizes.py plus 100, B = 23 (one full 16-row tile and a ragged one of 7).

Which decoder forward kernel runs cannot be observed (launch_text_decoder_fwd does not go through the probe); restated from
csrc/text.hip launch_text_decoder_fwd: the weights-resident text_decoder_fwd2_kernel<7> runs when kx == 224 and kz == 128, that
is 97 <= D <= 100, and the knob text_fwd2 is 1 (its default); every other D, and D = 100 with text_fwd2 = 0, runs the streamed
text_decoder_fwd_kernel.  D = 100 is run both ways on identical inputs, each against the oracle.

Gates (tests/text_ref.py): 4 times what a float64 emulation that rounds the GEMM operands text.hip rounds differs from the
unrounded oracle at that D on the same inputs -- 2 for the backward's bf16-stored gate gradients the emulation leaves out, 2 the
project's usual margin; nothing is taken from the engine.  tests/test_cpu_text_ref.py prints the yardsticks and shows that these
comparisons see an ignored last latent column, a row answered with another row's result and an ignored keep mask.
MMVAE_TOL_REPORT=1 prints the engine's error next to every gate."""
import os

import pytest
import torch

import text_ref as TR

pytestmark = pytest.mark.gpu

REPORT = os.environ.get("MMVAE_TOL_REPORT") is not None
# (D, text_fwd2): the knob matters at 97 <= D <= 100 only
CASES = [(D, 1) for D in TR.SIZES] + [(100, 0), (100, 1)]
IDS = ["D%d" % D if D != 100 else "D100-%s" % ("resident" if k else "streamed") for D, k in CASES]
_REF = {}
_MODS = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _setup(D):
    """parameters, inputs, gates and the oracle's result of one latent size: computed once, shared, never changed"""
    if D not in _REF:
        P = TR.text_params(D)
        inp = TR.make_inputs(D)
        gate, ref, emu = TR.gates(P, inp)
        _REF[D] = (P, inp, gate, ref, emu)
    return _REF[D]


def _modules(D, P, dev):
    """the two drop-in modules at latent size D holding the parameters P (float32)"""
    from multimodal_vae_amd import multimnist as M
    if D not in _MODS:
        _MODS.clear()
        enc = M.TextEncoder(D, 12, n_hiddens=100, bidirectional=True)
        dec = M.TextDecoder(D, 12, n_hiddens=100, use_cuda=True)
        _MODS[D] = (enc.cuda().train(), dec.cuda().train())
    enc, dec = _MODS[D]
    enc.load_state_dict({k[len(TR.ENC):]: v for k, v in P.items() if k.startswith(TR.ENC)}, strict=True)
    dec.load_state_dict({k[len(TR.DEC):]: v for k, v in P.items() if k.startswith(TR.DEC)}, strict=True)
    return enc, dec


def _forward(enc, dec, inp, dev, free_running=False):
    with torch.no_grad():
        words = dec(inp["z"].to(dev), keep=inp["keep"].to(dev), force_tokens=None if free_running else inp["force"].to(dev))
        toks = dec.last_tokens.clone()
        mu, lv = enc(inp["text"].to(dev))
    return dict(words=words, tokens=toks, encout=torch.cat((mu, lv), 1))


def _full(enc, dec, inp, dev):
    for m in (enc, dec):
        m.zero_grad(set_to_none=True)
    z = inp["z"].to(dev).requires_grad_(True)
    words = dec(z, keep=inp["keep"].to(dev), force_tokens=inp["force"].to(dev))
    toks = dec.last_tokens.clone()
    words.backward(inp["gw"].to(dev))
    mu, lv = enc(inp["text"].to(dev))
    out = torch.cat((mu, lv), 1)
    out.backward(inp["ge"].to(dev))
    grads = {TR.ENC + n: p.grad.detach().cpu() for n, p in enc.named_parameters()}
    grads.update({TR.DEC + n: p.grad.detach().cpu() for n, p in dec.named_parameters()})
    return dict(words=words.detach(), tokens=toks, encout=out.detach(), dz=z.grad.detach(), grads=grads)


def _knob(value):
    from multimodal_vae_amd._lib import knobs
    return knobs(text_fwd2=value)


@pytest.mark.parametrize("D,fwd2", CASES, ids=IDS)
def test_modules_match_float64(D, fwd2):
    """words and the encoder output element-wise, dz and every parameter gradient by relative L2, with random z, random forced
    tokens, injected keep masks and random upstream gradients"""
    dev = _dev()
    P, inp, gate, ref, emu = _setup(D)
    enc, dec = _modules(D, P, dev)
    with _knob(fwd2):
        got = _full(enc, dec, inp, dev)
        torch.cuda.synchronize()
    bad, e = TR.violations(got, ref, gate, "D=%d" % D)
    if REPORT:
        print("TOL text modules D=%d fwd2=%d: words %.2e abs (emulation %.2e), encoder output %.2e abs (%.2e), dz %.2e rel (%.2e), "
              "worst gradient tensor %.2e (%s; emulation %.2e) [gates = 4 x emulation]"
              % (D, fwd2, e["words"], emu["words"], e["encout"], emu["encout"], e["dz"], emu["dz"], e["grads"], e["grads_worst"], emu["grads"]))
    assert not bad, bad
    # the greedy tokens are the argmax of the engine's own log-probabilities (first maximum, like torch.max)
    assert torch.equal(got["tokens"].cpu(), got["words"].argmax(-1).cpu())


@pytest.mark.parametrize("D,fwd2", CASES, ids=IDS)
def test_rows_are_independent_bit_for_bit(D, fwd2):
    """a wrong `r0 + row < R` guard or a tile that reads its neighbour moves 1/23 of a tensor: no tolerance sees that, equality
    of a row's result across batches does (tests/text_ref.py row_independence_violations)"""
    dev = _dev()
    P, inp, _, _, _ = _setup(D)
    enc, dec = _modules(D, P, dev)
    with _knob(fwd2):
        for free in (False, True):
            bad = TR.row_independence_violations(lambda i: _forward(enc, dec, i, dev, free), inp)
            assert not bad, (D, fwd2, "free-running" if free else "forced", bad)


@pytest.mark.parametrize("D,fwd2", CASES, ids=IDS)
def test_single_latent_column(D, fwd2):
    """only latent column D-1 (then only column 0) reaches the decoder, scaled by 4: a dropped last k-step or last column of
    kz / kx gives the z-independent answer"""
    dev = _dev()
    P, inp, _, _, _ = _setup(D)

    def run(Q, i):
        enc, dec = _modules(D, Q, dev)
        return _full(enc, dec, i, dev)

    with _knob(fwd2):
        for col in ((D - 1,) if D == 1 else (D - 1, 0)):
            bad, fig = TR.single_column_violations(run, P, D, col, inp)
            if REPORT:
                print("TOL text modules D=%d fwd2=%d column %d: words %.2e (gate %.2e), dz column %.2e (gate %.2e)"
                      % (D, fwd2, col, fig["words"], fig["gate_words"], fig["dz"], fig["gate_dz"]))
            assert not bad, bad
