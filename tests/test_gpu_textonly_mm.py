"""The MultiMNIST text-only VAE baseline on the MI355X: the text kernels' hidden-size-50 instantiation (csrc/text.hip), the
text-only plan (mmvae_mmtext_*), its one-enqueue step, the trainer, the scorer and the driver, against the float64 restatement of
tests/textonly_mm_ref.py.

Module gates: 4 times what a float64 emulation that rounds the GEMM operands text.hip rounds differs from the unrounded result at
H = 50 on the same inputs (tests/test_cpu_textonly_mm.py prints them and shows the faults they see).  Step gates: the project's
MultiMNIST gates for these kernels (loss rel 1e-3, mu / logvar abs 1e-2, per-tensor gradient rel-L2 4e-2, total gradient norm 2e-3).
MMVAE_TOL_REPORT=1 prints the engine's error next to every gate."""
import ctypes as C
import os

import pytest
import torch

import textonly_mm_ref as TM
from oracle import mmvae_ref as R

pytestmark = pytest.mark.gpu

REPORT = os.environ.get("MMVAE_TOL_REPORT") is not None
SIZES = (1, 20, 100, 127)            # kx = 64, 96, 160, 192 at H = 50: a single latent column and the widest
H = 50
_REF, _ENG = {}, {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class Engine:
    """The four module entry points of one plan family on explicit tensors: ``api`` "mmtext" (the text-only plan, hidden size
    ``H``) or "mm" (the MMVAE's plan; parameters under text_encoder.* / text_decoder.*)."""

    def __init__(self, D, H, dev, api="mmtext"):
        from multimodal_vae_amd import core
        self.D, self.H, self.dev, self.api = D, H, dev, api
        self.st = core.MultimnistTextState(D, dev, H) if api == "mmtext" else core.MultimnistState(D, dev)
        self.fn = "mmvae_mmtext_%s" if api == "mmtext" else "mmvae_mm_text_%s"
        self.pre = ("encoder.", "decoder.") if api == "mmtext" else ("text_encoder.", "text_decoder.")

    def _name(self, n):
        return n if self.api == "mmtext" else "text_" + n

    def load(self, P):
        for n, v in P.items():
            self.st.view(self._name(n)).copy_(v.to(self.dev))
        self.st.pack_weights()

    def grads(self):
        out = {}
        for n, shape, off in self.st.table:
            if n.startswith(self.pre):
                numel = 1
                for s in shape:
                    numel *= s
                out[n if self.api == "mmtext" else n[len("text_"):]] = self.st.grads[off:off + numel].view(shape).clone().cpu()
        return out

    def _call(self, fn, *a):
        from multimodal_vae_amd._lib import call
        from multimodal_vae_amd._ops import stream
        return call(self.fn % fn, *a, stream())

    def forward(self, inp, free_running=False, training=True, ws=None):
        from multimodal_vae_amd._lib import ptr
        B = inp["z"].shape[0]
        h, wsb = self.st.plan(B), self.st.module_workspace_bytes(B)
        dev = self.dev
        ws_d = torch.empty(wsb, dtype=torch.uint8, device=dev) if ws is None else ws[0]
        ws_e = torch.empty(wsb, dtype=torch.uint8, device=dev) if ws is None else ws[1]
        z, keep, text = inp["z"].to(dev).contiguous(), inp["keep"].to(dev).contiguous(), inp["text"].to(dev).contiguous()
        force = None if free_running else inp["force"].to(dev).contiguous()
        words = torch.empty(B, 4, 12, device=dev)
        toks = torch.empty(B, 4, dtype=torch.int64, device=dev)
        enc = torch.empty(B, 2 * self.D, device=dev)
        self._call("decoder_fwd", h, ptr(ws_d), wsb, ptr(z), int(training), ptr(keep), ptr(force), ptr(words), ptr(toks))
        self._call("encoder_fwd", h, ptr(ws_e), wsb, ptr(text), ptr(enc))
        self._last = (h, wsb, ws_d, ws_e, z, keep, text, force, words, toks)
        return dict(words=words, tokens=toks, encout=enc)

    def full(self, inp):
        from multimodal_vae_amd._lib import ptr
        out = self.forward(inp)
        h, wsb, ws_d, ws_e, z, keep, text, force, words, toks = self._last
        dz = torch.empty_like(z)
        self.st.grads.zero_()
        self._call("decoder_bwd", h, ptr(ws_d), wsb, ptr(z), ptr(keep), ptr(force), ptr(words), ptr(toks),
                   ptr(inp["gw"].to(self.dev).contiguous()), ptr(dz))
        g = self.grads()
        self.st.grads.zero_()
        self._call("encoder_bwd", h, ptr(ws_e), wsb, ptr(text), ptr(inp["ge"].to(self.dev).contiguous()))
        ge = self.grads()
        for n in g:
            if n.startswith("encoder."):
                g[n] = ge[n]
        torch.cuda.synchronize()
        out.update(dz=dz, grads=g)
        return out


def _engine(D, Hh, dev, api="mmtext"):
    key = (D, Hh, api)
    if key not in _ENG:
        if len(_ENG) > 6:
            _ENG.clear()
        _ENG[key] = Engine(D, Hh, dev, api)
    return _ENG[key]


def _setup(D):
    """parameters, inputs, gates and the float64 result of one latent size: computed once, shared, never changed"""
    if D not in _REF:
        P = TM.make_params(D, H)
        inp = TM.make_inputs(D, H)
        gate, ref, emu = TM.gates(P, inp)
        _REF[D] = (P, inp, gate, ref, emu)
    return _REF[D]


# ------------------------------------------------------------------------------------------------ 1. modules at H = 50
@pytest.mark.parametrize("D", SIZES)
def test_modules_match_float64(D):
    dev = _dev()
    P, inp, gate, ref, emu = _setup(D)
    eng = _engine(D, H, dev)
    eng.load(P)
    got = eng.full(inp)
    bad, e = TM.violations(got, ref, gate, "D=%d" % D)
    if REPORT:
        print("TOL mmtext modules H=50 D=%d: words %.2e (gate %.2e), encout %.2e (%.2e), dz %.2e (%.2e), worst grad %.2e %s (%.2e)"
              % (D, e["words"], gate["words"], e["encout"], gate["encout"], e["dz"], gate["dz"], e["grads"], e["grads_worst"], gate["grads"]))
    assert not bad, bad
    assert torch.equal(got["tokens"].cpu(), got["words"].argmax(-1).cpu())
    # two calls give equal bits
    again = eng.full(inp)
    for k in ("words", "tokens", "encout", "dz"):
        assert torch.equal(got[k], again[k]), k
    for n in got["grads"]:
        assert torch.equal(got["grads"][n], again["grads"][n]), n


@pytest.mark.parametrize("D", (20, 127))
def test_small_batch_matches_float64(D):
    """B = 5: one ragged tile"""
    dev = _dev()
    P, inp, _, _, _ = _setup(D)
    part = TM.take_rows(inp, [3, 17, 0, 22, 9])
    gate, ref, _ = TM.gates(P, part)
    eng = _engine(D, H, dev)
    eng.load(P)
    bad, _ = TM.violations(eng.full(part), ref, gate, "B=5 D=%d" % D)
    assert not bad, bad


@pytest.mark.parametrize("D", SIZES)
def test_free_running_tokens(D):
    """the greedy path with the decoder's own tokens fed back: every token equals float64's -- the inputs are chosen so that the
    float64 top-two margin at every (row, step) is at least 10 x the words gate, so no row is excluded"""
    dev = _dev()
    P, inp, ref, margin, g_words = TM.free_running_case(D, H)
    if REPORT:
        print("TOL mmtext free-running D=%d: margin %.3e, words gate %.3e" % (D, margin, g_words))
    assert margin >= 10 * g_words, (margin, g_words)
    eng = _engine(D, H, dev)
    eng.load(P)
    got = eng.forward(inp, free_running=True)
    assert torch.equal(got["tokens"].cpu(), ref["tokens"])
    assert float((got["words"].double().cpu() - ref["words"]).abs().max()) <= g_words


@pytest.mark.parametrize("D", SIZES)
def test_rows_are_independent_bit_for_bit(D):
    dev = _dev()
    P, inp, _, _, _ = _setup(D)
    eng = _engine(D, H, dev)
    eng.load(P)
    for free in (False, True):
        bad = TM.row_independence_violations(lambda i: eng.forward(i, free), inp)
        assert not bad, (D, free, bad)


def test_eval_mode_ignores_keep():
    dev = _dev()
    D = 20
    P, inp, gate, _, _ = _setup(D)
    eng = _engine(D, H, dev)
    eng.load(P)
    a = eng.forward(inp, training=False)["words"].clone()
    other = dict(inp, keep=1 - inp["keep"])
    b = eng.forward(other, training=False)["words"]
    assert torch.equal(a, b)
    ref = TM.run_forward(P, inp, eval_mode=True)
    assert float((a.double().cpu() - ref["words"]).abs().max()) <= gate["words"]
    assert not torch.equal(a, eng.forward(inp, training=True)["words"])


# ------------------------------------------------------------------------------------------------ 2. the new plan at H = 100
@pytest.mark.parametrize("D", (20, 100))
def test_h100_plan_equals_mm_text_modules_bit_for_bit(D):
    """the same kernels: the text-only plan at n_hiddens = 100 holding the MMVAE's text parameters gives the bits of mmvae_mm_text_*"""
    dev = _dev()
    P = TM.make_params(D, 100)
    inp = TM.make_inputs(D, 100)
    a, b = _engine(D, 100, dev), _engine(D, 100, dev, "mm")
    a.load(P); b.load(P)
    ga, gb = a.full(inp), b.full(inp)
    for k in ("words", "tokens", "encout", "dz"):
        assert torch.equal(ga[k], gb[k]), k
    for n in ga["grads"]:
        assert torch.equal(ga["grads"][n], gb["grads"][n]), n


# ------------------------------------------------------------------------------------------------ 3. zero-embedding cross-check
@pytest.mark.parametrize("D", (20, 127))
def test_h50_embedded_in_h100_is_the_same_function(D):
    dev = _dev()
    P, inp, gate50, ref, _ = _setup(D)
    Q, M = TM.embed_into(P, D)
    inp100 = dict(inp, keep=torch.cat((inp["keep"], torch.ones_like(inp["keep"])), dim=2).contiguous())
    gate100, ref100, _ = TM.gates(Q, inp100)
    e50, e100 = _engine(D, 50, dev), _engine(D, 100, dev)
    e50.load(P); e100.load(Q)
    g50, g100 = e50.full(inp), e100.full(inp100)
    for k in ("words", "encout"):
        tol = gate50[k] + gate100[k]
        assert float((g50[k].double() - g100[k].double()).abs().max()) <= tol, k
    assert TM.rel_l2(g50["dz"].cpu(), g100["dz"].cpu()) <= gate50["dz"] + gate100["dz"]
    kept = TM.extract_from(g100["grads"], M)
    for n, m in M.items():
        assert float(g100["grads"][n][m].abs().max()) == 0.0 if bool(m.any()) else True, "added entries of %s" % n
        if float(ref["grads"][n].abs().max()) > 0:
            assert TM.rel_l2(kept[n], g50["grads"][n].reshape(-1)) <= gate50["grads"] + gate100["grads"], n


# ------------------------------------------------------------------------------------------------ 4. the step
def _step_case(B, D, seed=0):
    g = torch.Generator().manual_seed(500 + 7 * B + D + seed)
    return dict(text=torch.randint(0, 12, (B, 4), generator=g), eps=torch.randn(B, D, generator=g),
                keep=(torch.rand(4, B, H, generator=g) >= R.DROP_P).to(torch.uint8), force=torch.randint(0, 12, (B, 4), generator=g))


def _step_engine(B, D, dev, P, kl_lambda=1e-3, lambda_y=1.0):
    from multimodal_vae_amd import core
    st = core.MultimnistTextState(D, dev, H)
    for n, v in P.items():
        st.view(n).copy_(v.to(dev))
    return core.FusedMMTextStep(st, B, lr=1e-3, kl_lambda=kl_lambda, lambda_y=lambda_y, seed=11)


@pytest.mark.parametrize("B,D", [(2, 20), (4, 100)])
def test_module_face_trains_like_float64(B, D):
    """``TextVAE`` through its drop-in modules in training mode (mmvae_mmtext_encoder / decoder, fwd and bwd, with autograd between
    them): forward, ``textonly_loss_function`` and ``.backward()`` against the float64 step, at the gates of the fused step above;
    then once more with a keep mask the decoder draws itself."""
    from multimodal_vae_amd import multimnist as M
    dev = _dev()
    P = TM.make_params(D, H)
    c = _step_case(B, D)
    ref = TM.run_step(P, c["text"], c["eps"], c["keep"], c["force"])
    vae = M.TextVAE(D, use_cuda=True)
    vae.load_state_dict(P, strict=True)
    vae = vae.cuda().train()
    text = c["text"].to(dev)
    recon, mu, lv = vae(text, eps=c["eps"].to(dev), gru_keep=c["keep"].to(dev), force_tokens=c["force"].to(dev))
    loss = M.textonly_loss_function(mu, lv, recon, text, kl_lambda=1e-3)
    loss.backward()
    g = {n: p.grad.detach().cpu() for n, p in vae.named_parameters()}
    assert sorted(g) == sorted(ref["grads"])
    rel = abs(float(loss) - ref["loss"]) / abs(ref["loss"])
    e_mu = float((mu.double().cpu() - ref["mu"]).abs().max())
    e_lv = float((lv.double().cpu() - ref["logvar"]).abs().max())
    by = {n: TM.rel_l2(g[n], ref["grads"][n]) for n in g if float(ref["grads"][n].abs().max()) > 0}
    tot = torch.sqrt(sum((g[n].double() ** 2).sum() for n in g))
    tot_ref = torch.sqrt(sum((ref["grads"][n] ** 2).sum() for n in g))
    e_tot = abs(float(tot) - float(tot_ref)) / float(tot_ref)
    if REPORT:
        print("TOL mmtext modules B=%d D=%d: loss rel %.2e, mu %.2e, logvar %.2e, worst grad %.2e (%s), total norm %.2e"
              % (B, D, rel, e_mu, e_lv, max(by.values()), max(by, key=by.get), e_tot))
    assert rel <= 1e-3 and e_mu <= 1e-2 and e_lv <= 1e-2
    assert all(v <= 4e-2 for v in by.values()), {n: v for n, v in by.items() if v > 4e-2}
    assert e_tot <= 2e-3
    assert float(g["encoder.gru.weight_hh_l0_reverse"].abs().max()) == 0.0
    assert torch.equal(vae.decoder.last_tokens.cpu(), ref["tokens"])
    # a mask of its own: seeded, the same mask and so the same bits twice; another seed, another mask
    got = []
    for seed in (3, 3, 4):
        vae.zero_grad()
        torch.manual_seed(seed)
        recon, mu, lv = vae(text, eps=c["eps"].to(dev), force_tokens=c["force"].to(dev))
        M.textonly_loss_function(mu, lv, recon, text).backward()
        got.append((recon.detach().clone(), vae.decoder.z2h.weight.grad.clone()))
        assert all(bool(torch.isfinite(p.grad).all()) for p in vae.parameters())
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert not torch.equal(got[0][0], got[2][0])


def _grads_of(st):
    out = {}
    for n, shape, off in st.table:
        numel = 1
        for s in shape:
            numel *= s
        out[n] = st.grads[off:off + numel].view(shape).clone().cpu()
    return out


@pytest.mark.parametrize("B,D", [(5, 20), (23, 127), (16, 100)])
def test_step_matches_float64(B, D):
    dev = _dev()
    P = TM.make_params(D, H)
    c = _step_case(B, D)
    ref = TM.run_step(P, c["text"], c["eps"], c["keep"], c["force"])
    eng = _step_engine(B, D, dev, P)
    mu, lv = torch.empty(B, D, device=dev), torch.empty(B, D, device=dev)
    kw = dict(eps=c["eps"].to(dev), gru_keep=c["keep"].to(dev), force_tokens=c["force"].to(dev), mu=mu, logvar=lv)
    out = eng.forward_backward(c["text"].to(dev), True, True, **kw)
    loss = float(out.losses()[0])
    g = _grads_of(eng.state)
    sums = eng.sums.clone().cpu()
    rel = abs(loss - ref["loss"]) / abs(ref["loss"])
    e_mu = float((mu.double().cpu() - ref["mu"]).abs().max())
    e_lv = float((lv.double().cpu() - ref["logvar"]).abs().max())
    by = {n: TM.rel_l2(g[n], ref["grads"][n]) for n in g if float(ref["grads"][n].abs().max()) > 0}
    tot = torch.sqrt(sum((g[n].double() ** 2).sum() for n in g))
    tot_ref = torch.sqrt(sum((ref["grads"][n] ** 2).sum() for n in g))
    e_tot = abs(float(tot) - float(tot_ref)) / float(tot_ref)
    if REPORT:
        print("TOL mmtext step B=%d D=%d: loss rel %.2e, mu %.2e, logvar %.2e, worst grad %.2e (%s), total norm %.2e"
              % (B, D, rel, e_mu, e_lv, max(by.values()), max(by, key=by.get), e_tot))
    assert rel <= 1e-3 and e_mu <= 1e-2 and e_lv <= 1e-2
    assert all(v <= 4e-2 for v in by.values()), {n: v for n, v in by.items() if v > 4e-2}
    assert e_tot <= 2e-3
    assert float(g["encoder.gru.weight_hh_l0_reverse"].abs().max()) == 0.0
    assert abs(float(sums[4]) - float(ref["nll_sum"])) <= 1e-3 * abs(float(ref["nll_sum"])) and all(float(sums[i]) == 0 for i in (0, 1, 2, 3, 5, 6, 7, 9, 10))
    # equal bits on a second run
    out = eng.forward_backward(c["text"].to(dev), True, True, **kw)
    g2 = _grads_of(eng.state)
    assert all(torch.equal(g[n], g2[n]) for n in g) and torch.equal(sums, eng.sums.cpu())


def test_step_modes():
    dev = _dev()
    B, D = 16, 20
    P = TM.make_params(D, H)
    c = _step_case(B, D)
    text = c["text"].to(dev)
    kw = dict(eps=c["eps"].to(dev), gru_keep=c["keep"].to(dev), force_tokens=c["force"].to(dev))
    # training = 0: z = mu, no dropout: the eval-mode loss of the restatement
    eng = _step_engine(B, D, dev, P)
    ref = TM.run_step(P, c["text"], None, None, c["force"])
    words = torch.empty(B, 4, 12, device=dev)
    loss = float(eng.forward_backward(text, False, False, force_tokens=kw["force_tokens"], recon_text=words).losses()[0])
    assert abs(loss - ref["loss"]) <= 1e-3 * abs(ref["loss"])
    emu = TM.run_step(P, c["text"], None, None, c["force"], rounded=True)
    assert float((words.double().cpu() - ref["words"]).abs().max()) <= TM.GATE_FACTOR * float((emu["words"] - ref["words"]).abs().max())
    # do_backward = 0 writes no gradient
    eng.state.grads.fill_(3.0)
    eng.forward_backward(text, True, False, **kw)
    assert bool((eng.state.grads == 3.0).all())
    # lambda_y = 0 leaves only KL gradients: the decoder's are exactly 0
    eng0 = _step_engine(B, D, dev, P, lambda_y=0.0)
    eng0.forward_backward(text, True, True, **kw)
    g = _grads_of(eng0.state)
    ref0 = TM.run_step(P, c["text"], c["eps"], c["keep"], c["force"], lambda_y=0.0)
    for n in g:
        if n.startswith("decoder."):
            assert float(g[n].abs().max()) == 0.0, n
        elif float(ref0["grads"][n].abs().max()) > 0:
            assert TM.rel_l2(g[n], ref0["grads"][n]) <= 4e-2, n


def test_defer_unpack_packed_adam_equals_unpack_adam():
    dev = _dev()
    B, D = 16, 20
    P = TM.make_params(D, H)
    c = _step_case(B, D)
    text = c["text"].to(dev)
    kw = dict(eps=c["eps"].to(dev), gru_keep=c["keep"].to(dev), force_tokens=c["force"].to(dev))
    a, b = _step_engine(B, D, dev, P), _step_engine(B, D, dev, P)
    b.separate_unpack = True
    for _ in range(2):
        a(text, **kw)
        b(text, **kw)
    torch.cuda.synchronize()
    assert torch.equal(a.state.params, b.state.params)
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)


# ------------------------------------------------------------------------------------------------ 5. trainer
def test_trainer_three_steps_and_checkpoints(tmp_path):
    from multimodal_vae_amd import multimnist as M
    dev = _dev()
    B, D = 8, 20
    P = TM.make_params(D, H)
    vae = M.TextVAE(D, use_cuda=True)
    vae.load_state_dict(P, strict=True)
    vae = vae.cuda().train()
    trainer = M.TextVAETrainer(vae, B, lr=1e-3, kl_lambda=1e-3, seed=5)
    eng = trainer.engine
    ref_p = {n: v.double().clone() for n, v in P.items()}
    m = {n: torch.zeros_like(v) for n, v in ref_p.items()}
    v2 = {n: torch.zeros_like(v) for n, v in ref_p.items()}
    for step in range(1, 4):
        c = _step_case(B, D, seed=step)
        before = {n: t.detach().clone() for n, t in vae.state_dict().items()}
        eng.separate_unpack = True              # the gradient of this step stays readable
        trainer(c["text"].to(dev), eps=c["eps"].to(dev), gru_keep=c["keep"].to(dev), force_tokens=c["force"].to(dev))
        g = _grads_of(eng.state)
        # the reference optimizer on the ENGINE's gradients: parameters agree to the project's optimizer gate
        names = list(ref_p)
        R.adam_step([ref_p[n] for n in names], [g[n].double() for n in names], [m[n] for n in names], [v2[n] for n in names], step, lr=1e-3)
        after = vae.state_dict()
        for n in ref_p:
            assert float((after[n].double().cpu() - ref_p[n]).abs().max()) <= 2e-6, n
            changed = not torch.equal(after[n], before[n])
            assert changed == (n != "encoder.gru.weight_hh_l0_reverse"), n
        # ... and the engine's gradients agree with float64 on the parameters the step started from
        ref = TM.run_step({n: t.cpu() for n, t in before.items()}, c["text"], c["eps"], c["keep"], c["force"])
        for n in g:
            if float(ref["grads"][n].abs().max()) > 0:
                assert TM.rel_l2(g[n], ref["grads"][n]) <= 4e-2, n
    # checkpoint round trip
    path = str(tmp_path / "ck.pth.tar")
    from multimodal_vae_amd.train_textonly_multimnist import checkpoint_dict
    torch.save(checkpoint_dict(vae, eng, 1.0, D), path)
    back = M.load_checkpoint_textonly(path, use_cuda=True)
    for n, t in vae.state_dict().items():
        assert torch.equal(back.state_dict()[n].cpu(), t.cpu()), n
    # ... and one produced on the CPU by plain torch modules with the reference shapes
    import torch.nn as nn

    class Enc(nn.Module):
        def __init__(s):
            super().__init__()
            s.embed, s.gru, s.h2p = nn.Embedding(12, 50), nn.GRU(50, 50, 1, bidirectional=True), nn.Linear(50, 2 * D)

    class Dec(nn.Module):
        def __init__(s):
            super().__init__()
            s.embed, s.z2h, s.gru, s.h2o = nn.Embedding(12, 50), nn.Linear(D, 50), nn.GRU(50 + D, 50, 2, dropout=0.1), nn.Linear(50 + D, 12)

    class Plain(nn.Module):
        def __init__(s):
            super().__init__()
            s.encoder, s.decoder = Enc(), Dec()

    plain = Plain()
    path2 = str(tmp_path / "cpu.pth.tar")
    torch.save({'state_dict': plain.state_dict(), 'best_loss': 0.0, 'n_latents': D, 'optimizer': {}}, path2)
    got = M.load_checkpoint_textonly(path2, use_cuda=True).eval()
    sd = {n: t.detach() for n, t in plain.state_dict().items()}
    c = _step_case(B, D)
    with torch.no_grad():
        recon, mu, lv = got(c["text"].to(dev), force_tokens=c["force"].to(dev))
    ref = TM.run_step(sd, c["text"], None, None, c["force"])
    emu = TM.run_step(sd, c["text"], None, None, c["force"], rounded=True)
    assert float((mu.double().cpu() - ref["mu"]).abs().max()) <= 1e-2
    assert float((recon.double().cpu() - ref["words"]).abs().max()) <= TM.GATE_FACTOR * float((emu["words"] - ref["words"]).abs().max())


# ------------------------------------------------------------------------------------------------ 6. scorer
def test_iw_scorer():
    from multimodal_vae_amd import evaluate as E, multimnist as M
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd._ops import stream
    dev = _dev()
    Bn, K, D = 3, 7, 20
    P = TM.make_params(D, H, out_scale=8.0)
    g = torch.Generator().manual_seed(77)
    z = torch.randn(Bn, K, D, generator=g)
    eng = _engine(D, H, dev)
    eng.load(P)
    rows = Bn * K
    inp = dict(z=z.reshape(rows, D), keep=torch.ones(4, rows, H, dtype=torch.uint8), text=torch.zeros(rows, 4, dtype=torch.int64),
               force=torch.zeros(rows, 4, dtype=torch.int64))
    mod = eng.forward(inp, free_running=True, training=False)["words"].clone()
    h, wsb = eng.st.plan(rows), eng.st.module_workspace_bytes(rows)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    words = torch.empty(rows, 4, 12, device=dev)
    call("mmvae_mmtext_iw_score", h, ptr(ws), wsb, ptr(z.to(dev).contiguous()), Bn, K, ptr(words), stream())
    assert torch.equal(words, mod)
    # iw_estimate's log p(y) against float64 with the same particles
    vae = M.TextVAE(D, use_cuda=True)
    vae.load_state_dict(P, strict=True)
    vae = vae.cuda().eval()
    text = torch.randint(0, 12, (Bn, 4), generator=g)
    mu, lv = torch.randn(Bn, D, generator=g) * 0.3, torch.randn(Bn, D, generator=g) * 0.2 - 1.0
    eps = torch.randn(Bn, K, D, generator=g)
    r = E.iw_estimate(vae, None, text.to(dev), mu.to(dev), lv.to(dev), K, eps=eps.to(dev), return_z=True)
    zz = r["z"].double().cpu()
    P64 = TM.f64(P)
    with torch.no_grad():
        w, _ = TM.decoder(P64, zz.reshape(rows, D))
    emu, _ = TM.decoder(P64, zz.reshape(rows, D), rounded=True)
    gate = TM.GATE_FACTOR * float((emu.detach() - w).abs().max()) * 4
    lpy = w.reshape(Bn, K, 4, 12).gather(3, text.reshape(Bn, 1, 4, 1).expand(Bn, K, 4, 1)).sum((2, 3))
    std = torch.exp(0.5 * lv.double()).unsqueeze(1)
    log_pz = (-0.5 * zz ** 2).sum(-1)
    log_q = (-0.5 * ((zz - mu.double().unsqueeze(1)) / std) ** 2 - torch.log(std)).sum(-1)
    ref = torch.logsumexp(lpy + log_pz - log_q, dim=1) - torch.log(torch.tensor(float(K), dtype=torch.float64))
    got = r["log_p"][:, 1].double().cpu()
    assert float((got - ref).abs().max()) <= gate, (got, ref, gate)
    assert bool(torch.isnan(r["log_p"][:, 0]).all())


# ------------------------------------------------------------------------------------------------ 7. driver
def test_driver_and_evaluate(tmp_path, capsys):
    from multimodal_vae_amd import evaluate as E, train_textonly_multimnist as T
    _dev()
    out, res = str(tmp_path / "models"), str(tmp_path / "results")
    hist = T.main(["--cuda", "--synthetic", "512", "--epochs", "2", "--batch_size", "64", "--n_latents", "20", "--out", out, "--results", res])
    assert hist["train"][1] < hist["train"][0]
    ck = os.path.join(out, "checkpoint.pth.tar")
    for f in (ck, os.path.join(out, "model_best.pth.tar"), os.path.join(res, "sample_text_epoch1.txt"), os.path.join(res, "sample_text_epoch2.txt")):
        assert os.path.exists(f), f
    d = torch.load(ck, map_location="cpu", weights_only=False)
    assert sorted(d) == ["best_loss", "n_latents", "optimizer", "state_dict"]
    assert len(open(os.path.join(res, "sample_text_epoch2.txt")).read().splitlines()) == 64
    loss = E.main(["test_textonly", ck, "--dataset", "multimnist", "--synthetic", "128", "--batch_size", "64"])
    assert loss == loss and loss > 0
    table = E.main(["loglik", ck, "--synthetic", "64", "--n_samples", "8", "--batch_size", "32"])
    assert list(table) == ["text"] and table["text"]["log_py"] < 0 and table["text"]["log_px"] != table["text"]["log_px"]
    E.main(["sample", ck, "--n_samples", "8", "--out", str(tmp_path / "s")])
    assert len(open(str(tmp_path / "s" / "sample_text.txt")).read().splitlines()) == 8
    assert not os.path.exists(str(tmp_path / "s" / "sample_image.pt"))
