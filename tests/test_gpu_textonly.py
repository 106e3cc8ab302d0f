"""GPU tests of the text-only VAE baseline (COCO): the fp32 backward of the one-expert latent block alone, the one-pass fused caption step
against the float64 reference (tests/textonly_ref.py), its exact properties, the nn.Module / trainer / driver face and the scorer.

Gates of the step are the project's own for the COCO step (tests/test_gpu_coco.py), none widened: loss rel 1e-3 | mu / logvar abs 1e-2 |
per-tensor gradient rel-L2 4.5e-2 | total gradient norm rel 1e-2 | caption output abs 4x the bf16-operand emulation's own distance from
float64 on the case (tests/test_cpu_textonly.py shows the emulation alone inside a quarter of every gate, and five stand-in faults
outside one).  Every test prints what it measured (run with -s).
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import mmvae_ref as R
import coco_text_ref as CT
import textonly_ref as TR
from multimodal_vae_amd._lib import knobs as _knobs

pytestmark = pytest.mark.gpu

IMG = ("image_encoder.", "image_decoder.")
STILL = "text_encoder.gru.weight_hh_l0_reverse"     # zero gradient in the model itself: one step from h = 0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _state(D, T, dev):
    """The COCO plan state with the formula parameters of EVERY tensor, the image half's included."""
    from multimodal_vae_amd import core
    st = core.CocoState(D, dev, T)
    P = R.formula_params("coco", D)
    assert [t[0] for t in st.table] == [n for n, _ in R.param_table("coco", D)]
    for n, shape, off in st.table:
        st.params[off:off + P[n].numel()] = P[n].detach().reshape(-1).to(dev)
    return st


# ====================================================================================================== latent1_bwd_f32 alone
def _latent_inputs(B, D, seed):
    """the recipe of tests/test_gpu_imageonly.py: log-variances down to -20"""
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(B, D, generator=g)
    lv = torch.linspace(-20.0, 2.0, B * D).view(B, D) if B * D > 1 else torch.full((1, 1), -20.0)
    lv = lv.flatten()[torch.randperm(B * D, generator=g)].view(B, D).contiguous()
    eps = torch.randn(B, D, generator=g)
    dz = torch.randn(B, D, generator=g)
    return mu.contiguous(), lv, eps, dz


@pytest.mark.parametrize("B,D", [(1, 1), (3, 4), (5, 20), (7, 100), (4, 124)])
def test_latent1_bwd_f32_alone(B, D):
    """mmvae_latent1_bwd_f32 on its own operands: every element within 8 * 2^-24 * sum|terms| of the float64 formula; bf16(result) is the
    output of mmvae_latent1_bwd on the same operands bit for bit; the pad columns are exact zeros; training = 0 drops the eps term (and
    reads no eps); two calls give equal bits.  Measured on MI355X: worst error 1.05e-7 of sum|terms| (gate 4.77e-7)."""
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd._ops import stream
    dev = _dev()
    mu, lv, eps, dz = _latent_inputs(B, D, 100 * B + D)
    assert float(lv.min()) == -20.0
    mu_d, lv_d, eps_d, dz_d = (t.to(dev).contiguous() for t in (mu, lv, eps, dz))
    ld = 2 * D + 5
    kl_coef = 1e-3 / B
    nscr = call("mmvae_latent1_scratch_floats", B, D)
    for training in (True, False):
        def run():
            out = torch.full((B, ld), 7.0, dtype=torch.float32, device=dev)
            call("mmvae_latent1_bwd_f32", ptr(mu_d), ptr(lv_d), ptr(eps_d) if training else None, ptr(dz_d), B, D, int(training), kl_coef,
                 ptr(out), ld, stream())
            return out
        out = run()
        val, mag = TR.latent1_bwd_f32_terms(mu, lv, eps, dz, kl_coef, training)
        err = ((out[:, :2 * D].double().cpu() - val).abs() / mag).max().item()
        print("latent1_bwd_f32 (B=%d, D=%d, training=%d): worst error / sum|terms| %.3e (gate %.3e)" % (B, D, training, err, 8 * 2.0 ** -24))
        assert err <= 8 * 2.0 ** -24, err
        assert float(out[:, 2 * D:].abs().max()) == 0.0
        assert torch.equal(out, run())
        old = torch.full((B, ld), 7.0, dtype=torch.bfloat16, device=dev)
        scr = torch.zeros(nscr, dtype=torch.float32, device=dev)
        call("mmvae_latent1_bwd", ptr(mu_d), ptr(lv_d), ptr(eps_d) if training else None, ptr(dz_d), B, D, int(training), kl_coef, ptr(old), ld,
             None, None, None, ptr(scr), stream())
        assert torch.equal(out.to(torch.bfloat16), old)
        if not training:        # the eps term is gone: d_logvar is the KL term alone
            kl_only = -0.5 * kl_coef * (1.0 - torch.exp(lv.double()))
            assert ((out[:, D:2 * D].double().cpu() - kl_only).abs() <= 8 * 2.0 ** -24 * mag[:, D:]).all()
    # no reconstruction term: dz = NULL
    out = torch.full((B, ld), 7.0, dtype=torch.float32, device=dev)
    call("mmvae_latent1_bwd_f32", ptr(mu_d), ptr(lv_d), ptr(eps_d), None, B, D, 1, kl_coef, ptr(out), ld, stream())
    val0, mag0 = TR.latent1_bwd_f32_terms(mu, lv, eps, torch.zeros_like(dz), kl_coef, True)
    assert ((out[:, :2 * D].double().cpu() - val0).abs() <= 8 * 2.0 ** -24 * mag0).all()


# ====================================================================================================== the step
@functools.lru_cache(maxsize=None)
def _case(T, B, D, keep):
    """parameters, inputs and the float64 step of a case, computed once and left unchanged"""
    P32 = CT.text_params(D)
    inp = TR.make_inputs(T, B, D, keep)
    return P32, inp, TR.step64(P32, inp)


@functools.lru_cache(maxsize=None)
def _yardstick(T, B, D, keep, forms):
    P32, inp, ref = _case(T, B, D, keep)
    return TR.measure(TR.emulate(P32, inp, *forms), ref)["sentence"]


def _run_step(st, eng, inp, dev, backward=True, training=True):
    B, T = inp["text"].shape[:2]
    D = st.n_latents
    keep = inp["keep"]
    eng.gru_dropout = keep is not None
    mu, lv = torch.zeros(B, D, device=dev), torch.zeros(B, D, device=dev)
    recon = torch.zeros(B, T, 300, device=dev)
    kw = {} if keep is None else dict(gru_keep=keep.to(dev).contiguous())
    out = eng.forward_backward(inp["text"].to(dev).contiguous(), training, backward, eps=inp["eps"].to(dev).contiguous(), mu=mu, logvar=lv,
                               recon_text=recon, **kw)
    losses = out.losses().cpu()
    torch.cuda.synchronize()
    g = st.grads.cpu()
    grads = {n: g[off:off + _numel(shape)].view(shape).clone() for n, shape, off in st.table}
    return dict(loss=float(losses[0]), losses=losses, sums=eng.sums.cpu().clone(), mu=mu.cpu(), logvar=lv.cpu(), sentence=recon.cpu(), grads=grads)


def _check_against_oracle(case, knobs):
    from multimodal_vae_amd.core import FusedTextStep
    dev = _dev()
    T, B, D, keep = case
    P32, inp, ref = _case(*case)
    forms = TR.forms_of(B, D, knobs)
    gate_s = TR.sentence_gate(_yardstick(*case, forms))
    st = _state(D, T, dev)
    eng = FusedTextStep(st, B, R.formula_sos(), kl_lambda=1e-3)
    assert eng.ws.numel() == st.module_workspace_bytes(B) < st.workspace_bytes(B)
    with _knobs(**knobs):
        got = _run_step(st, eng, inp, dev)
    m = TR.measure(got, ref)
    print("text step %s %s (%s encoder, %s decoder): %s | sentence gate %.3e" % (TR.case_id(case), knobs or "", forms[0], forms[1], TR.describe(m), gate_s))
    for k, v in sorted(m["tensors"].items()):
        print("    %-44s %.3e" % (k, v))
    assert got["losses"][1].item() == 0.0 and got["losses"][2].item() == 0.0
    assert all(float(got["sums"][i]) == 0.0 for i in range(16) if i not in (4, 8)), got["sums"]
    for n, g in got["grads"].items():
        if n.startswith(IMG):
            assert float(g.abs().max()) == 0.0, n
    assert bool(torch.isfinite(got["sentence"]).all())
    bad = TR.violations(m, gate_s)
    assert not bad, bad


@pytest.mark.parametrize("case", TR.CASES, ids=TR.case_id)
def test_step_matches_float64(case):
    """One training step of FusedTextStep (given eps, given or no keep masks, formula parameters) against tests/textonly_ref.step64:
    loss, mu, logvar, the sentence, every caption gradient tensor and the total norm; every image gradient exactly 0; sums zero but
    for [4] and [8].  Measured on MI355X over the six cases (gates in brackets): loss rel <= 5.5e-5 (1e-3); mu / logvar abs <= 8.0e-4
    (1e-2); sentence abs <= 1.7e-3 (4.3e-3 .. 7.4e-3, 4x the emulation's); worst gradient tensor 3.1e-3 .. 4.1e-3 (4.5e-2); total
    gradient norm <= 1.3e-4 (1e-2)."""
    _check_against_oracle(case, {})


@pytest.mark.parametrize("knobs", TR.KNOB_RUNS, ids=lambda k: ",".join("%s=%d" % kv for kv in k.items()))
def test_step_matches_float64_in_the_other_kernel_forms(knobs):
    """(7, 17, 100) with keep masks again: cluster of 4 and one workgroup per row block (three-exchange kernels, unfused MSE), and with
    the streamed-encoder knob set.  Every knob is put back."""
    _check_against_oracle((7, 17, 100, True), knobs)


@pytest.mark.parametrize("case", [(7, 17, 100, True), (5, 23, 120, False)], ids=TR.case_id)
def test_fused_one_group_mse_agrees_with_the_stand_alone_pass(case):
    """The MSE branch of the composed decoder forward with ONE row group against coco_mse3 behind the same kernel (knob
    coco_no_mse_fuse), under the tolerances of tests/test_gpu_configs_r2.py::test_coco_caption_kernel_forms_agree.  Measured on
    MI355X: no difference at all in the sentence or in any gradient tensor at either shape."""
    from multimodal_vae_amd.core import FusedTextStep
    dev = _dev()
    T, B, D, keep = case
    assert TR.forms_of(B, D)[1] == "composed"
    _, inp, _ = _case(*case)
    st = _state(D, T, dev)
    eng = FusedTextStep(st, B, R.formula_sos(), kl_lambda=1e-3)
    a = _run_step(st, eng, inp, dev)
    with _knobs(coco_no_mse_fuse=1):
        b = _run_step(st, eng, inp, dev)
    np.testing.assert_allclose(a["losses"].numpy(), b["losses"].numpy(), rtol=2e-4)
    d_s = float((a["sentence"] - b["sentence"]).abs().max())
    ga, gb = torch.cat([g.reshape(-1) for g in a["grads"].values()]), torch.cat([g.reshape(-1) for g in b["grads"].values()])
    d_g = float((ga - gb).norm() / gb.norm())
    worst = max(float((a["grads"][n] - b["grads"][n]).norm()) / max(float(b["grads"][n].norm()), 1e-30) for n in a["grads"] if float(b["grads"][n].norm()) > 0)
    print("fused vs stand-alone MSE %s: loss %.6g | %.6g, sentence max diff %.3e, gradient rel %.3e, worst tensor %.3e"
          % (TR.case_id(case), a["loss"], b["loss"], d_s, d_g, worst))
    assert d_s < 1e-2 and d_g < 1e-2
    for n in a["grads"]:
        assert float((a["grads"][n] - b["grads"][n]).norm()) <= 5e-2 * float(b["grads"][n].norm()) + 1e-7, n


# ====================================================================================================== exact properties
def test_exact_properties():
    """At T = 5, B = 6, D = 20.  mu / logvar are the halves of mmvae_coco_text_encoder_fwd's output (knob coco_module_bf16 = 1) bit for
    bit; eval mode ignores eps and the step counter bit for bit (z = mu, nothing drawn) and its sentence is the decoder module's on mu
    inside the case's sentence gate (the same kernels, the forward-only instantiation); mu, logvar and the sentence of two calls with
    the same eps are bit-equal.  The gradients of two such calls are NOT asserted bit-equal: the caption weight gradients go through
    split-K GEMMs whose partial tiles are folded with fp32 atomics (csrc/gemm.hip, gemm_f32.hip), so their order is not fixed; the
    difference is printed and must be of fp32 summation size (1e-4 relative).  Measured on MI355X at this shape: 0."""
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd._ops import stream
    from multimodal_vae_amd.core import FusedTextStep
    dev = _dev()
    T, B, D = 5, 6, 20
    inp = TR.make_inputs(T, B, D, True)
    st = _state(D, T, dev)
    eng = FusedTextStep(st, B, R.formula_sos(), kl_lambda=1e-3)
    a = _run_step(st, eng, inp, dev)
    b = _run_step(st, eng, inp, dev)
    for n, g in a["grads"].items():
        if n.startswith(IMG):
            assert float(g.abs().max()) == 0.0, n
    for k in ("mu", "logvar", "sentence"):
        assert torch.equal(a[k], b[k]), k
    ga, gb = torch.cat([g.reshape(-1) for g in a["grads"].values()]), torch.cat([g.reshape(-1) for g in b["grads"].values()])
    d = float((ga - gb).norm() / gb.norm())
    print("two equal steps: gradient rel difference %.3e, loss %.9g | %.9g" % (d, a["loss"], b["loss"]))
    assert d <= 1e-4
    # the encoder module's output
    text_d = inp["text"].to(dev).contiguous()
    wsb = st.module_workspace_bytes(B)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = torch.empty(B, 2 * D, dtype=torch.float32, device=dev)
    with _knobs(coco_module_bf16=1):
        call("mmvae_coco_text_encoder_fwd", st.plan(B), ptr(ws), wsb, ptr(text_d), ptr(out), stream())
    assert torch.equal(out[:, :D].cpu(), a["mu"]) and torch.equal(out[:, D:].cpu(), a["logvar"])
    # eval mode
    inp_e = dict(inp, eps=torch.full((B, D), 1e30))
    e1 = _run_step(st, eng, inp, dev, backward=False, training=False)
    eng.adam_state[0] = 5
    e2 = _run_step(st, eng, inp_e, dev, backward=False, training=False)
    eng.adam_state[0] = 0
    for k in ("mu", "logvar", "sentence"):
        assert torch.equal(e1[k], e2[k]), k
    assert torch.equal(e1["mu"], a["mu"])
    sent = torch.empty(B, T, 300, dtype=torch.float32, device=dev)
    sos = R.formula_sos().to(dev)
    with _knobs(coco_module_bf16=2):
        call("mmvae_coco_text_decoder_fwd", st.plan(B), ptr(ws), wsb, ptr(e1["mu"].to(dev).contiguous()), ptr(sos), None, 0, ptr(sent), stream())
    P32 = CT.text_params(D)
    ref = TR.step64(P32, inp)
    yard = TR.measure(TR.emulate(P32, inp, *TR.forms_of(B, D)), ref)["sentence"]
    d_e = float((sent.cpu() - e1["sentence"]).abs().max())
    print("eval-mode sentence vs the decoder module on mu: max diff %.3e (gate %.3e)" % (d_e, TR.sentence_gate(yard)))
    assert d_e <= TR.sentence_gate(yard)
    np.testing.assert_allclose(e1["sums"].numpy(), e2["sums"].numpy(), rtol=1e-6)


def test_trainer_step_leaves_the_image_half_alone():
    """After TextVAETrainer.__call__ (T = 5, B = 6, D = 20): the image parameters, every BatchNorm buffer and num_batches_tracked are
    bit-unchanged, and every caption tensor has changed -- but for encoder.gru.weight_hh_l0_reverse, which cannot: the reverse
    direction contributes its FIRST step only (coco/model.py:239), taken from h = 0, so the gradient of its hidden weights is exactly
    zero in the model itself (tests/textonly_ref.step64 and autograd through the reference agree) and Adam leaves the tensor alone."""
    from multimodal_vae_amd import coco as M
    dev = _dev()
    T, B, D = 5, 6, 20
    inp = TR.make_inputs(T, B, D, False)
    vae = M.TextVAE(D, sos=R.formula_sos(), steps=T)
    vae.load_state_dict({k[len("text_"):]: v.clone() for k, v in CT.text_params(D).items()}, strict=True)
    vae.cuda().train()
    tr = M.TextVAETrainer(vae, B, lr=1e-3)
    st = tr.engine.state
    P = R.formula_params("coco", D)
    for n, shape, off in st.table:                   # give the image half values worth keeping
        if n.startswith(IMG):
            st.params[off:off + P[n].numel()] = P[n].detach().reshape(-1).to(dev)
    st.bn_stats.copy_(torch.rand_like(st.bn_stats) + 0.5)
    st.bn_nbt.fill_(3)
    st.pack_weights()
    p0, bn0, nbt0 = st.params.clone(), st.bn_stats.clone(), st.bn_nbt.clone()
    out = tr(inp["text"].to(dev).contiguous())
    out.check()
    assert np.isfinite(out.losses()[0].item())
    for n, shape, off in st.table:
        same = torch.equal(st.params[off:off + _numel(shape)], p0[off:off + _numel(shape)])
        assert same == (n.startswith(IMG) or n == STILL), n
    assert torch.equal(st.bn_stats, bn0) and torch.equal(st.bn_nbt, nbt0)
    assert int(tr.engine.adam_state[0]) == 1
    # the module face reads the updated parameters: forward() through the two children equals the engine's eval pass
    vae.eval()
    mu = torch.zeros(B, D, device=dev)
    tr.evaluate(inp["text"].to(dev).contiguous(), mu=mu)
    with torch.no_grad(), _knobs(coco_module_bf16=1):
        _, mu2, _ = vae(inp["text"].to(dev))
    assert torch.equal(mu, mu2)


def test_step_draws_its_own_noise_and_masks():
    """eps = NULL, gru_keep = NULL, gru_dropout = 1: the loss is finite, differs between two step counters and is the same for the same
    counter and seed (the sentence bit for bit; the loss sums up to the order of their fp32 atomics)."""
    from multimodal_vae_amd.core import FusedTextStep
    dev = _dev()
    T, B, D = 5, 6, 20
    text = TR.make_inputs(T, B, D, False)["text"].to(dev).contiguous()
    st = _state(D, T, dev)
    eng = FusedTextStep(st, B, R.formula_sos(), seed=11)
    assert eng.gru_dropout

    def run(counter):
        eng.adam_state[0] = counter
        recon = torch.zeros(B, T, 300, device=dev)
        loss = eng.forward_backward(text, True, True, recon_text=recon).losses()[0].item()
        return loss, recon.clone()
    l0, r0 = run(0)
    l1, r1 = run(1)
    l0b, r0b = run(0)
    print("drawn noise: loss at counter 0: %.9g, at counter 1: %.9g, at counter 0 again: %.9g" % (l0, l1, l0b))
    assert np.isfinite(l0) and np.isfinite(l1)
    assert abs(l1 - l0) > 1e-5 * abs(l0) and not torch.equal(r0, r1)
    assert torch.equal(r0, r0b)
    np.testing.assert_allclose(l0b, l0, rtol=1e-6)
    eng.gru_dropout = False
    eng.adam_state[0] = 0
    recon = torch.zeros(B, T, 300, device=dev)
    eng.forward_backward(text, True, True, recon_text=recon)
    assert not torch.equal(recon, r0)                # the masks took part


# ====================================================================================================== trainer, driver, commands
def test_trainer_lowers_the_loss_and_checkpoint_round_trips(tmp_path, capsys):
    from multimodal_vae_amd import coco as M, evaluate as E, train_textonly as TT
    dev = _dev()
    T, B, D = 4, 8, 20
    g = torch.Generator().manual_seed(2)
    text = (0.4 * torch.randn(1, 1, 300, generator=g) + 0.05 * torch.randn(B, T, 300, generator=g)).contiguous().to(dev)   # one word, jittered
    torch.manual_seed(0)
    sos = R.formula_sos()
    vae = M.TextVAE(D, sos=sos, steps=T).cuda()
    tr = M.TextVAETrainer(vae, B, lr=3e-3)
    first = tr(text).losses()[0].item()
    for _ in range(29):
        last = tr(text).losses()[0].item()
    print("TextVAETrainer: loss %.5f -> %.5f after 30 steps" % (first, last))
    assert np.isfinite(last) and last < 0.95 * first, (first, last)
    path = str(tmp_path / "ck.pth.tar")
    ck = TT.checkpoint_dict(vae, tr.engine, last, D)
    assert sorted(ck) == ["best_loss", "n_latents", "optimizer", "state_dict"] and float(ck["optimizer"]["state"][0]["step"]) == 30
    torch.save(ck, path)
    assert E.is_textonly_checkpoint(path)
    vae2 = M.load_checkpoint_textonly(path, use_cuda=True, sos=sos, steps=T)
    assert isinstance(vae2, M.TextVAE) and list(vae2.state_dict()) == TR.state_dict_keys(D)
    for k, v in vae2.state_dict().items():
        assert torch.equal(v.cpu(), ck["state_dict"][k].cpu()), k
    ev = tr.evaluate(text).losses()[0].item()
    ev2 = M.TextVAETrainer(vae2, B).evaluate(text).losses()[0].item()
    np.testing.assert_allclose(ev2, ev, rtol=1e-6)
    # eval-mode loss against float64 on the trained parameters
    P32 = {"text_" + k: v.detach().cpu() for k, v in vae.state_dict().items()}
    ref = TR.step64(P32, dict(text=text.cpu(), eps=None, keep=None), sos=sos, training=False, backward=False)
    print("evaluate: %.6f, float64 %.6f" % (ev, ref["loss"]))
    np.testing.assert_allclose(ev, ref["loss"], rtol=1e-3)
    capsys.readouterr()
    loss = E.test_textonly(vae2, [(None, text), (None, text)])
    assert "====> Test set loss: {:.4f}".format(loss) in capsys.readouterr().out
    np.testing.assert_allclose(loss, tr.__class__(vae2, B, kl_lambda=1.0).evaluate(text).losses()[0].item(), rtol=1e-6)


def test_driver_and_commands(tmp_path, capsys):
    """train_textonly --synthetic 64 --epochs 1 --batch_size 8 runs and writes the four-key dict; evaluate test_textonly prints the
    reference's line; loglik_coco reports log p(y) alone; sample_coco writes captions only."""
    from multimodal_vae_amd import coco as M, evaluate as E, train_textonly as TT
    _dev()
    out, res = str(tmp_path / "models"), str(tmp_path / "results")
    hist = TT.main(["--cuda", "--synthetic", "64", "--epochs", "1", "--batch_size", "8", "--n_latents", "20", "--out", out, "--results", res,
                    "--seed", "3"])
    printed = capsys.readouterr().out
    assert len(hist["train"]) == 1 and np.isfinite(hist["train"][0]) and np.isfinite(hist["test"][0]) and hist["kl_lambda"] == [1e-3]
    assert "Train Epoch: 1 [0/64 (0%)]\tLoss: " in printed and "====> Epoch: 1 Average loss: " in printed and "====> Test set loss: " in printed
    ck_path = os.path.join(out, "checkpoint.pth.tar")
    assert os.path.exists(os.path.join(out, "model_best.pth.tar"))
    ck = torch.load(ck_path, map_location="cpu", weights_only=False)
    assert sorted(ck) == ["best_loss", "n_latents", "optimizer", "state_dict"] and ck["n_latents"] == 20
    assert list(ck["state_dict"]) == TR.state_dict_keys(20) and ck["best_loss"] == hist["test"][0]
    assert float(ck["optimizer"]["state"][0]["step"]) == 8 and len(ck["optimizer"]["state"]) == len(ck["state_dict"])
    s = torch.load(os.path.join(res, "sample_text_epoch1.pt"))
    assert s.shape == (64, 102, 300) and bool(torch.isfinite(s).all())
    loss = E.main(["test_textonly", ck_path, "--synthetic", "16", "--batch_size", "8", "--seed", "4"])
    assert np.isfinite(loss) and loss > 0
    assert "====> Test set loss: {:.4f}".format(loss) in capsys.readouterr().out
    table = E.main(["loglik_coco", ck_path, "--synthetic", "4", "--batch_size", "4", "--n_samples", "3", "--seed", "1", "--text_sigma", "0.5"])
    assert list(table) == ["text"] and np.isfinite(table["text"]["log_py"]) and math.isnan(table["text"]["log_px"]) and math.isnan(table["text"]["log_pxy"])
    sdir = str(tmp_path / "samples")
    caps = E.main(["sample_coco", ck_path, "--synthetic_words", "40", "--n_samples", "3", "--out", sdir, "--seed", "2"])
    assert len(caps) == 3 and all(len(c.split(' ')) == 102 for c in caps)
    assert os.path.exists(os.path.join(sdir, "sample_text.txt")) and not os.path.exists(os.path.join(sdir, "sample_image.pt"))
    # with a word table the driver writes words
    TT.main(["--cuda", "--synthetic", "16", "--epochs", "1", "--batch_size", "8", "--n_latents", "20", "--out", out, "--results", res,
             "--synthetic_words", "40"])
    lines = open(os.path.join(res, "sample_text_epoch1.txt")).read().splitlines()
    assert len(lines) == 64 and all(len(l.split(' ')) == 102 for l in lines)


# ====================================================================================================== the scorer
def test_iw_score_text_equals_the_caption_half_of_iw_score():
    """mmvae_coco_iw_score_text at B = 2, K = 3, T = 4, D = 20: sse_y is mmvae_coco_iw_score's on the same z, text and sos bit for bit;
    parameters and buffers are untouched; log_marginal of a text-only model is finite and moves with text_sigma as in loglik_coco."""
    from multimodal_vae_amd import coco as M
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd._ops import stream
    from multimodal_vae_amd.evaluate import coco_text_constant, iw_estimate, log_marginal
    dev = _dev()
    B, K, T, D = 2, 3, 4, 20
    rows = B * K
    st = _state(D, T, dev)
    st.pack_weights()
    g = torch.Generator().manual_seed(5)
    z = torch.randn(rows, D, generator=g).to(dev)
    text = (0.4 * torch.randn(B, T, 300, generator=g)).to(dev)
    image = torch.rand(B, 3, 32, 32, generator=g).to(dev)
    sos = R.formula_sos().to(dev)
    for plan_rows in (rows, rows + 2):              # the plan's rows exactly, and a plan with spare rows
        h = st.plan(plan_rows)
        wsb = call("mmvae_coco_iw_workspace_bytes", h)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        lx, sse_a, sse_b = (torch.full((rows,), 7.0, device=dev) for _ in range(3))
        p0, bn0, nbt0, g0 = st.params.clone(), st.bn_stats.clone(), st.bn_nbt.clone(), st.grads.clone()
        call("mmvae_coco_iw_score", h, ptr(ws), wsb, ptr(z), ptr(image), ptr(text), ptr(sos), B, K, ptr(lx), ptr(sse_a), stream())
        call("mmvae_coco_iw_score_text", h, ptr(ws), wsb, ptr(z), ptr(text), ptr(sos), B, K, ptr(sse_b), stream())
        torch.cuda.synchronize()
        print("iw_score_text (plan of %d rows): sse_y %s" % (plan_rows, sse_b.tolist()))
        assert torch.equal(sse_a, sse_b) and bool(torch.isfinite(sse_b).all()) and float(sse_b.min()) > 0
        assert torch.equal(st.params, p0) and torch.equal(st.bn_stats, bn0) and torch.equal(st.bn_nbt, nbt0) and torch.equal(st.grads, g0)
    # the estimator on a TextVAE
    vae = M.TextVAE(D, sos=R.formula_sos(), steps=T)
    vae.load_state_dict({k[len("text_"):]: v.clone() for k, v in CT.text_params(D).items()}, strict=True)
    vae.cuda().eval()
    r1 = log_marginal(vae, [(None, text)], n_particles=K, posterior="text", seed=3, text_sigma=1.0)
    r2 = log_marginal(vae, [(None, text)], n_particles=K, posterior="text", seed=3, text_sigma=2.0)
    print("TextVAE log p(y): sigma 1: %.4f, sigma 2: %.4f" % (r1["log_py"], r2["log_py"]))
    assert np.isfinite(r1["log_py"]) and np.isfinite(r2["log_py"]) and r1["n"] == B
    assert math.isnan(r1["log_px"]) and math.isnan(r1["log_pxy"]) and math.isnan(r1["image_nll"]) and np.isfinite(r1["text_nll"])
    with pytest.raises(ValueError, match="text posterior alone"):
        log_marginal(vae, [(None, text)], n_particles=2, posterior="joint")
    # sigma enters as -sse / (2 sigma^2) and through the constant: check one example against the scorer's own sse
    with torch.no_grad():
        mu, lv = vae.encoder(text)
    e = iw_estimate(vae, None, text, mu, lv, K, seed=3, return_log_w=True, text_sigma=2.0)
    e1 = iw_estimate(vae, None, text, mu, lv, K, seed=3, return_log_w=True, text_sigma=1.0)
    assert torch.equal(e["sse"], e1["sse"])
    d = (e["log_w"][..., 1] - e1["log_w"][..., 1]).double().cpu()
    want = (-e["sse"].double().cpu() * (0.125 - 0.5)) + (coco_text_constant(T, 2.0) - coco_text_constant(T, 1.0))
    np.testing.assert_allclose(d.numpy(), want.numpy(), rtol=1e-4)
    assert bool(torch.isnan(e["log_w"][..., 0]).all()) and bool(torch.isnan(e["log_w"][..., 2]).all())
