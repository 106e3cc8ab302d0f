"""CPU tests of the text-only VAE baseline (COCO): state_dict keys against the recorded and the live reference, the refusals of the
latent size, the train_textonly driver's command line, KL schedule and checkpoint dict, the ctypes layout of mmvae_text_step_io, and
the test instrument tests/textonly_ref.py itself: its agreement with the live reference, the room the gates of
tests/test_gpu_textonly.py leave to bf16 operands, and that those gates see faults."""
import ctypes as C
import functools
import json
import os
import re
import shutil
import subprocess

import pytest
import torch

from oracle import mmvae_ref as R
import coco_text_ref as CT
import textonly_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "coco_textvae_keys.json")


def _live_reference():
    """(model module, train module) of the reference's coco folder with its GloVe stubbed, or None where it is absent."""
    from oracle import make_golden as G
    if not os.path.isdir(os.path.join(G.REF, "coco")):
        return None
    return G.import_reference("coco")


# ====================================================================================================== the Python face
@pytest.mark.parametrize("D", [8, 20, 100])
def test_state_dict_keys_are_the_references(D):
    """TextVAE(D).state_dict(): the reference's names and shapes (recorded from the live reference TextVAE into
    tests/golden/coco_textvae_keys.json; compared with the live one too where it is present) -- no image key, no experts."""
    from multimodal_vae_amd import coco as M
    vae = M.TextVAE(D, sos=R.formula_sos())
    sd = vae.state_dict()
    recorded = json.load(open(GOLDEN))[str(D)]
    assert [[k, list(v.shape)] for k, v in sd.items()] == recorded
    assert list(sd) == TR.state_dict_keys(D)
    assert all(k.startswith(("encoder.gru.", "encoder.h2p.", "decoder.z2h.", "decoder.gru.", "decoder.h2o.")) for k in sd)
    assert [n for n, _ in vae.named_children()] == ["encoder", "decoder"]
    assert isinstance(vae.encoder, M.TextEncoder) and isinstance(vae.decoder, M.TextDecoder)
    for meth in ("encode", "decode", "reparametrize", "forward"):
        assert callable(getattr(vae, meth))
    assert vae._core.prefix == "text_" and vae.encoder._mmvae_root() is vae and vae.decoder._mmvae_root() is vae
    live = _live_reference()
    if live is not None:
        ref = live[0].TextVAE(D)
        assert [[k, list(v.shape)] for k, v in ref.state_dict().items()] == recorded


@pytest.mark.parametrize("D", [200, 6, 0, 128])
def test_latent_sizes_outside_the_plan_are_refused_on_the_host(D):
    from multimodal_vae_amd import coco as M
    with pytest.raises(M.MMVAEError, match=r"4\.\.124, a multiple of 4"):
        M.TextVAE(D, sos=R.formula_sos())
    for ok in (4, 20, 100, 124):
        assert M.check_text_latents(ok) == ok


def test_refusal_reaches_the_driver_before_any_device_work(monkeypatch):
    from multimodal_vae_amd import train_textonly as T
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    with pytest.raises(SystemExit, match=r"n_latents=200 .*4\.\.124"):
        T.main(["--cuda", "--n_latents", "200", "--synthetic", "64"])


def test_driver_flags_and_defaults():
    from multimodal_vae_amd import train_textonly as T
    a = T.build_parser().parse_args([])
    assert (a.n_latents, a.batch_size, a.epochs, a.lr, a.log_interval, a.anneal_kl, a.cuda) == (100, 64, 20, 1e-4, 10, False, False)
    assert (a.synthetic, a.out, a.results, a.seed) == (0, './trained_models/text_only', './results/text_only', 1234)
    assert (a.sos, a.words, a.synthetic_words) == ('', '', 0)
    assert isinstance(a.data, str)
    help_text = T.build_parser().format_help()
    assert "200" in help_text and "100" in help_text            # the departure from the reference's default is stated
    with pytest.raises(SystemExit):                              # no CPU fallback
        T.main([])


def test_driver_kl_schedule():
    from multimodal_vae_amd import train_textonly as T
    assert T.kl_lambdas(12) == [1e-3] * 12
    # coco/train_textonly.py:145-153: next(schedule) at epochs 1, 6, 11, ...; an exhausted schedule keeps the last value
    assert T.kl_lambdas(33, anneal_kl=True) == [1e-5] * 5 + [1e-4] * 5 + [1e-3] * 5 + [1e-2] * 5 + [1e-1] * 5 + [1.0] * 8


def test_driver_checkpoint_dict():
    """state_dict / best_loss / n_latents / optimizer, the optimizer state over the TextVAE's own (caption) parameters only."""
    from multimodal_vae_amd import coco as M, train_textonly as T

    class Engine:       # the fields the optimizer state reads of a FusedTextStep
        pass
    D = 8
    vae = M.TextVAE(D, sos=R.formula_sos())
    table, off = [], 0
    for n, shape in R.param_table("coco", D):
        numel = 1
        for s in shape:
            numel *= s
        table.append((n, tuple(shape), off))
        off += numel
    eng = Engine()
    eng.state = type("S", (), {"table": table})()
    eng.adam_state = torch.tensor([3, 0])
    eng.exp_avg = torch.arange(off, dtype=torch.float32)
    eng.exp_avg_sq = torch.arange(off, dtype=torch.float32) * 2
    eng.lr, eng.betas, eng.eps = 1e-4, (0.9, 0.999), 1e-8
    ck = T.checkpoint_dict(vae, eng, 0.5, D)
    assert sorted(ck) == ["best_loss", "n_latents", "optimizer", "state_dict"]
    assert list(ck["state_dict"]) == TR.state_dict_keys(D) and ck["n_latents"] == D and ck["best_loss"] == 0.5
    names = ["text_" + k for k in TR.state_dict_keys(D)]
    opt = ck["optimizer"]
    assert len(opt["state"]) == len(names) == len(list(vae.parameters())) and opt["param_groups"][0]["params"] == list(range(len(names)))
    assert set(torch.optim.Adam(vae.parameters(), lr=1e-4).state_dict()["param_groups"][0]) <= set(opt["param_groups"][0])
    offs = {n: o for n, _, o in table}
    shapes = TR.state_dict_shapes(D)
    for i, n in enumerate(names):
        st = opt["state"][i]
        assert tuple(st["exp_avg"].shape) == shapes[n[len("text_"):]] and float(st["step"]) == 3.0
        assert float(st["exp_avg"].reshape(-1)[0]) == float(offs[n]) and float(st["exp_avg_sq"].reshape(-1)[0]) == 2.0 * offs[n]
    assert off > sum(p.numel() for p in vae.parameters())       # the image half of the plan is in no entry


def test_ctypes_text_step_io_layout_matches_the_header(tmp_path):
    from multimodal_vae_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    exe = str(tmp_path / "text_step_layout")
    subprocess.run([cc, "-std=c99", "-pedantic-errors", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "text_step_layout.c"), "-o", exe], check=True)
    line = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip()
    cls_name, size, *fields = line.split()
    cls = getattr(_lib, cls_name)
    assert cls.__doc__.split()[-1] == "mmvae_text_step_io"
    assert C.sizeof(cls) == int(size)
    assert [f.split(":")[0] for f in fields] == [n for n, _ in cls._fields_]
    for f in fields:
        n, o = f.split(":")
        assert getattr(cls, n).offset == int(o), n
    hdr = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    body = re.search(r"\{([^{}]*)\}\s*mmvae_text_step_io;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)(?:\[\d+\])?\s*[;,]", body) == [n for n, _ in cls._fields_]
    # every new entry point of the header has a ctypes prototype
    found = re.findall(r"\b(mmvae_coco_text_step\w*|mmvae_coco_iw_score_text|mmvae_latent1_bwd_f32)\(", hdr)
    assert sorted(set(found)) == ["mmvae_coco_iw_score_text", "mmvae_coco_text_step", "mmvae_coco_text_step_workspace_bytes", "mmvae_latent1_bwd_f32"]
    for fn in found:
        assert fn in _lib.SIGNATURES, fn


def test_evaluate_commands_know_the_text_only_checkpoint(tmp_path):
    from multimodal_vae_amd import coco as M, evaluate as E
    p = E._parser()
    a = p.parse_args(["test_textonly", "ck.pth.tar", "--synthetic", "64"])
    assert (a.cmd, a.batch_size, a.synthetic) == ("test_textonly", 64, 64)
    tv, iv = str(tmp_path / "t.pth.tar"), str(tmp_path / "i.pth.tar")
    torch.save({"state_dict": M.TextVAE(8, sos=R.formula_sos()).state_dict(), "n_latents": 8}, tv)
    torch.save({"state_dict": M.ImageVAE(8).state_dict(), "n_latents": 8}, iv)
    assert E.is_textonly_checkpoint(tv) and not E.is_textonly_checkpoint(iv)
    assert E.is_imageonly_checkpoint(iv)
    vae = M.load_checkpoint_textonly(tv, sos=R.formula_sos())
    assert isinstance(vae, M.TextVAE) and vae.n_latents == 8


# ====================================================================================================== the instrument
def test_step64_agrees_with_autograd_through_the_live_reference():
    """textonly_ref.step64 against the reference's own TextVAE + loss_function in float64 at B = 3, T = 4, D = 8 (stubbed GloVe whose
    '<s>' is formula_sos, dropout off, the eps the reference draws replayed from the same seed): 1e-10 relative."""
    live = _live_reference()
    if live is None:
        pytest.skip("the reference checkout is absent")
    model, train = live
    B, T, D = 3, 4, 8
    P32 = CT.text_params(D)
    inp = TR.make_inputs(T, B, D, False)
    model.MAX_WORDS = T
    vae = model.TextVAE(D).double()
    vae.load_state_dict({k[len("text_"):]: v.double() for k, v in P32.items()}, strict=True)
    vae.decoder.glove.glove.vectors = vae.decoder.glove.glove.vectors.double()
    vae.decoder.gru.dropout = 0.0
    vae.train()
    torch.manual_seed(77)
    inp["eps"] = torch.empty(B, D, dtype=torch.float64).normal_()
    torch.manual_seed(77)
    text = inp["text"].double()
    recon, mu, logvar = vae(text)
    loss = train.loss_function(mu, logvar, recon_text=recon, text=text, kl_lambda=1e-3, lambda_yx=1.)
    loss.backward()
    ref = TR.step64(P32, inp, kl_lambda=1e-3)

    def rel(a, b):
        return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-300)
    assert abs(ref["loss"] - loss.item()) <= 1e-10 * abs(loss.item())
    assert rel(ref["mu"], mu.detach()) <= 1e-10 and rel(ref["logvar"], logvar.detach()) <= 1e-10 and rel(ref["sentence"], recon.detach()) <= 1e-10
    named = dict(vae.named_parameters())
    assert sorted("text_" + k for k in named) == sorted(ref["grads"])
    for k, g in ref["grads"].items():
        lg = named[k[len("text_"):]].grad
        if lg is None or float(lg.abs().max()) == 0.0:
            assert float(g.abs().max()) == 0.0, k
        else:
            assert rel(g, lg) <= 1e-10, (k, rel(g, lg))


def _runs():
    """(case, knobs) of every step comparison of tests/test_gpu_textonly.py"""
    out = [(c, {}) for c in TR.CASES]
    out += [((7, 17, 100, True), k) for k in TR.KNOB_RUNS]
    return out


@functools.lru_cache(maxsize=None)
def _case(T, B, D, keep):
    P32 = CT.text_params(D)
    inp = TR.make_inputs(T, B, D, keep)
    return P32, inp, TR.step64(P32, inp)


@functools.lru_cache(maxsize=None)
def _emulated(T, B, D, keep, enc_form, dec_form):
    P32, inp, ref = _case(T, B, D, keep)
    return TR.measure(TR.emulate(P32, inp, enc_form, dec_form), ref)


def test_case_table_takes_every_path():
    forms = {TR.case_id(c): TR.forms_of(c[1], c[2]) for c in TR.CASES}
    assert forms == {"T1-B3-D20": ("streamed", "composed"), "T2-B1-D4": ("streamed", "composed"), "T7-B17-D100-keep": ("streamed", "composed"),
                     "T5-B23-D120": ("streamed", "composed"), "T5-B20-D124": ("resident", "three"), "T102-B4-D100": ("resident", "composed")}
    assert [TR.forms_of(17, 100, k) for k in TR.KNOB_RUNS] == [("streamed", "three"), ("streamed", "three"), ("streamed", "composed")]


@pytest.mark.parametrize("case,knobs", _runs(), ids=lambda v: TR.case_id(v) if isinstance(v, tuple) else ",".join("%s=%d" % kv for kv in v.items()) or "default")
def test_gates_leave_room_for_bf16_operands(case, knobs):
    """The float64 reference with the bf16 operands of the form that runs, and nothing else, stays within a quarter of every gate in
    force at the GPU case (the caption output's gate is 4x this very distance)."""
    m = _emulated(*case, *TR.forms_of(case[1], case[2], knobs))
    print("%s %s: emulation vs float64: %s" % (TR.case_id(case), knobs, TR.describe(m)))
    for k, v in sorted(m["tensors"].items()):
        print("    %-44s %.3e" % (k, v))
    for k in ("loss", "mu", "logvar", "total"):
        assert m[k] <= TR.GATES[k] / 4, (k, m[k])
    assert m["tensor"] <= TR.GATES["tensor"] / 4, (m["tensor_worst"], m["tensor"])
    assert m["sentence"] <= TR.sentence_gate(m["sentence"]) / 4 or TR.sentence_gate(m["sentence"]) == TR.SENTENCE_FLOOR
    assert all(v == 0.0 for v in m["small"].values()), m["small"]
    assert TR.violations(m, TR.sentence_gate(m["sentence"])) == []


# (ignoring a keep mask is a defect only where masks are given)
FAULT_RUNS = [(c, f) for c in TR.CASES for f in TR.FAULTS if f != "keep_ignored" or c[3]]


@pytest.mark.parametrize("case,fault", FAULT_RUNS, ids=lambda v: TR.case_id(v) if isinstance(v, tuple) else v)
def test_gates_see_faults(case, fault):
    """Each stand-in fault, put into the emulation of the case, misses at least one gate of the case."""
    T, B, D, keep = case
    P32, inp, ref = _case(*case)
    forms = TR.forms_of(B, D)
    yard = _emulated(*case, *forms)["sentence"]
    m = TR.measure(TR.emulate(P32, inp, *forms, fault=fault), ref)
    bad = TR.violations(m, TR.sentence_gate(yard))
    print("%s with %s: %s\n    misses: %s" % (TR.case_id(case), fault, TR.describe(m), bad[:4]))
    assert bad, (fault, TR.describe(m))


def test_latent1_bwd_f32_terms_are_the_latent_blocks_formula():
    import imageonly_ref as IR
    g = torch.Generator().manual_seed(3)
    mu, lv, eps, dz = (torch.randn(5, 7, generator=g) for _ in range(4))
    for training in (True, False):
        val, mag = TR.latent1_bwd_f32_terms(mu, lv, eps, dz, 2.5e-4, training)
        assert torch.allclose(val, IR.latent1_bwd(mu, lv, eps, dz, 2.5e-4, training), rtol=1e-14, atol=0)
        assert bool((mag >= val.abs()).all())
