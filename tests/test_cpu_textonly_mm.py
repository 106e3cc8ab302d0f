"""CPU tests of the MultiMNIST text-only VAE baseline: the float64 restatement of tests/textonly_mm_ref.py against live torch modules,
TextVAE's state_dict against the recorded reference names and shapes, the refusals of the host and of mmvae_mmtext_create, the
train_textonly_multimnist driver's command line, KL schedule and checkpoint dict, the ctypes layout of mmvae_mm_text_step_io, and
the yardsticks of tests/test_gpu_textonly_mm.py: the gates are printed, and every comparison is shown to see the faults it is for."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn as nn

from oracle import mmvae_ref as R
import textonly_mm_ref as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "multimnist_textvae_keys.json")


# ====================================================================================================== the restatement
class _Enc(nn.Module):
    def __init__(self, D, H):
        super().__init__()
        self.embed, self.gru, self.h2p = nn.Embedding(12, H), nn.GRU(H, H, 1, bidirectional=True), nn.Linear(H, 2 * D)


class _Dec(nn.Module):
    def __init__(self, D, H):
        super().__init__()
        self.embed, self.z2h = nn.Embedding(12, H), nn.Linear(D, H)
        self.gru, self.h2o = nn.GRU(H + D, H, 2, dropout=0.0), nn.Linear(H + D, 12)


class _Live(nn.Module):
    """TextVAE's forward (multimnist/model.py:123-147, 237-247, 268-288) on live torch layers, p = 0, float64"""

    def __init__(self, D, H):
        super().__init__()
        self.encoder, self.decoder, self.H = _Enc(D, H), _Dec(D, H), H

    def encode(self, x):
        e = self.encoder
        y, _ = e.gru(e.embed(x).transpose(0, 1), None)
        y = y[-1]
        return e.h2p(y[:, :self.H] + y[:, self.H:])

    def decode(self, z, force):
        d = self.decoder
        n = z.shape[0]
        c_in = torch.full((n,), R.SOS, dtype=torch.long)
        h = d.z2h(z).unsqueeze(0).repeat(2, 1, 1)
        words = []
        for i in range(4):
            c = R.swish(d.embed(c_in))
            o, h = d.gru(torch.cat((c, z), dim=1).unsqueeze(0), h)
            lp = torch.log_softmax(d.h2o(torch.cat((o.squeeze(0), z), dim=1)), dim=1)
            words.append(lp)
            c_in = lp.argmax(1) if force is None else force[:, i]
        return torch.stack(words, 1)


@pytest.mark.parametrize("H", [50, 100])
def test_restatement_equals_live_torch_modules(H):
    D, B = 20, 7
    torch.manual_seed(3 + H)
    live = _Live(D, H).double()
    P = {k: v.detach().clone() for k, v in live.state_dict().items()}
    assert [(k, tuple(v.shape)) for k, v in P.items()] == TM.param_shapes(D, H)
    c = TM.make_inputs(D, H, B)
    text, eps, force = c["text"], c["z"].double(), c["force"]
    out = live.encode(text)
    mu, lv = out[:, :D], out[:, D:]
    z = eps * torch.exp(0.5 * lv) + mu
    words = live.decode(z, force)
    loss = -words.reshape(B * 4, 12).gather(1, text.reshape(-1, 1)).sum() / (B * 4) - 1e-3 * 0.5 * torch.sum(1 + lv - mu ** 2 - lv.exp()) / B
    live.zero_grad()
    loss.backward()
    ref = TM.run_step(P, text, eps, None, force)
    assert abs(ref["loss"] - float(loss)) <= 1e-12 * abs(float(loss))
    assert float((ref["words"] - words.detach()).abs().max()) <= 1e-12
    for n, p in live.named_parameters():
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        assert float((ref["grads"][n] - g).abs().max()) <= 1e-12 * max(1.0, float(g.abs().max())), n
    assert float(ref["grads"]["encoder.gru.weight_hh_l0_reverse"].abs().max()) == 0.0      # one step from h = 0
    # free-running (the decoder's own tokens fed back)
    w2, _ = TM.decoder(TM.f64(P), z.detach())
    assert float((w2 - live.decode(z.detach(), None).detach()).abs().max()) <= 1e-12


# ====================================================================================================== the Python face
@pytest.mark.parametrize("D", [20, 100])
def test_state_dict_keys_are_the_references(D):
    from multimodal_vae_amd import multimnist as M
    vae = M.TextVAE(D)
    sd = vae.state_dict()
    recorded = json.load(open(GOLDEN))[str(D)]
    assert [[k, list(v.shape)] for k, v in sd.items()] == recorded
    assert [[k, list(s)] for k, s in TM.param_shapes(D, 50)] == recorded
    assert [n for n, _ in vae.named_children()] == ["encoder", "decoder"]
    assert isinstance(vae.encoder, M.TextEncoder) and isinstance(vae.decoder, M.TextDecoder)
    for meth in ("encode", "decode", "reparametrize", "forward"):
        assert callable(getattr(vae, meth))
    assert vae.encoder._mmvae_root() is vae and vae.decoder._mmvae_root() is vae
    assert M.TextVAE().n_latents == 20


def test_refusals():
    from multimodal_vae_amd import _lib, multimnist as M
    with pytest.raises(M.MMVAEError, match="n_hiddens=100"):
        M.TextEncoder(20, 12)                                    # stand-alone: today's behaviour and text
    with pytest.raises(M.MMVAEError, match="n_hiddens=100"):
        M.TextDecoder(20, 12)
    M.MultimodalVAE(20)                                          # the MMVAE still builds its 100-wide pair
    lib = _lib.load()
    assert not lib.mmvae_mmtext_create(20, 64, 8)
    msg = lib.mmvae_last_error().decode()
    assert "50" in msg and "100" in msg and "64" in msg
    for D in (0, 128):
        assert not lib.mmvae_mmtext_create(D, 50, 8)
        assert "n_latents" in lib.mmvae_last_error().decode()
    for Hh in (50, 100):
        h = lib.mmvae_mmtext_create(20, Hh, 8)
        assert h and lib.mmvae_mmtext_hidden(h) == Hh
        assert lib.mmvae_mmtext_num_bn(h) == 0 and lib.mmvae_mmtext_bn_floats(h) == 0
        name = C.create_string_buffer(128)
        nd, off, shape = C.c_int(), C.c_longlong(), (C.c_int * 4)()
        table = []
        for i in range(lib.mmvae_mmtext_num_params(h)):
            assert lib.mmvae_mmtext_param_info(h, i, name, C.byref(nd), shape, C.byref(off)) == 0
            table.append((name.value.decode(), tuple(shape[k] for k in range(nd.value))))
        assert table == TM.param_shapes(20, Hh)
        assert lib.mmvae_mmtext_module_workspace_bytes(h) == lib.mmvae_mmtext_workspace_bytes(h) > 0
        lib.mmvae_mmtext_destroy(h)


def test_driver_flags_schedule_and_checkpoint(monkeypatch):
    from multimodal_vae_amd import train_textonly_multimnist as T
    from multimodal_vae_amd.train import kl_schedule
    a = T.build_parser().parse_args([])
    assert (a.n_latents, a.batch_size, a.epochs, a.lr, a.log_interval, a.anneal_kl, a.cuda) == (100, 128, 20, 1e-3, 10, False, False)
    assert (a.synthetic, a.out, a.results, a.seed, a.generate) == (0, './trained_models/text_only', './results/text_only', 1234, False)
    assert (a.mnist_train, a.mnist_test, a.epoch_size, a.min_digits, a.max_digits) == ('', '', 60000, 0, 2)
    with pytest.raises(SystemExit):                              # no CPU fallback
        T.main(["--synthetic", "64"])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no CPU fallback"):
        T.main(["--cuda", "--synthetic", "64"])
    # multimnist/train_textonly.py:134-142: the next value every 5 epochs, the last one kept
    kl, sched, seen = 1e-3, kl_schedule(), []
    for epoch in range(1, 41):
        if (epoch - 1) % 5 == 0:
            kl = next(sched, kl)
        seen.append(kl)
    assert seen[0] == 1e-5 and seen[4] == 1e-5 and seen[5] == 1e-4 and seen[25] == 1.0 and seen[39] == 1.0

    class _Eng:                                                   # what adam_state_dict reads of an engine
        lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8

        def __init__(self, vae):
            shapes = [(n, tuple(p.shape)) for n, p in vae.state_dict().items()]
            offs, o = [], 0
            for n, s in shapes:
                offs.append((n, s, o))
                o += int(torch.tensor(s).prod())
            self.state = type("S", (), {"table": offs})()
            self.adam_state = torch.tensor([3, 0])
            self.exp_avg, self.exp_avg_sq = torch.zeros(o), torch.ones(o)

    from multimodal_vae_amd import multimnist as M
    vae = M.TextVAE(20)
    d = T.checkpoint_dict(vae, _Eng(vae), 0.5, 20)
    assert sorted(d) == ["best_loss", "n_latents", "optimizer", "state_dict"]
    opt = torch.optim.Adam(vae.parameters(), lr=1e-3)
    opt.load_state_dict(d["optimizer"])                           # torch.optim.Adam.state_dict() layout
    assert len(d["optimizer"]["state"]) == 24 and float(d["optimizer"]["state"][0]["step"]) == 3.0


def test_ctypes_step_io_layout_matches_the_header(tmp_path):
    from multimodal_vae_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    exe = str(tmp_path / "mm_text_step_layout")
    subprocess.run([cc, "-std=c99", "-pedantic-errors", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "mm_text_step_layout.c"), "-o", exe], check=True)
    line = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip()
    cls_name, size, *fields = line.split()
    cls = getattr(_lib, cls_name)
    assert cls.__doc__.split()[-1] == "mmvae_mm_text_step_io"
    assert C.sizeof(cls) == int(size)
    assert [f.split(":")[0] for f in fields] == [n for n, _ in cls._fields_]
    for f in fields:
        n, o = f.split(":")
        assert getattr(cls, n).offset == int(o), n
    hdr = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    body = re.search(r"\{([^{}]*)\}\s*mmvae_mm_text_step_io;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)(?:\[\d+\])?\s*[;,]", body) == [n for n, _ in cls._fields_]
    found = set(re.findall(r"\b(mmvae_mmtext_\w+)\(", hdr))
    assert {"mmvae_mmtext_create", "mmvae_mmtext_step", "mmvae_mmtext_iw_score", "mmvae_mmtext_encoder_fwd", "mmvae_mmtext_decoder_bwd"} <= found
    for fn in found:
        assert fn in _lib.SIGNATURES, fn


def test_evaluate_knows_the_checkpoint(tmp_path):
    from multimodal_vae_amd import evaluate as E, multimnist as M
    p = E._parser()
    a = p.parse_args(["test_textonly", "ck.pth.tar", "--synthetic", "64"])
    assert a.dataset == "coco"                                    # the default stays
    assert p.parse_args(["test_textonly", "ck.pth.tar", "--dataset", "multimnist", "--synthetic", "64"]).dataset == "multimnist"
    tv, mv = str(tmp_path / "t.pth.tar"), str(tmp_path / "m.pth.tar")
    torch.save({"state_dict": M.TextVAE(8).state_dict(), "n_latents": 8}, tv)
    torch.save({"state_dict": M.MultimodalVAE(8).state_dict(), "n_latents": 8}, mv)
    assert E.is_textonly_checkpoint(tv) and not E.is_textonly_checkpoint(mv)
    assert E._family(M.TextVAE(8)).text_only and E._family(M.TextVAE(8)).T == 4 and E._family(M.TextVAE(8)).V == 12
    assert E._family(M.MultimodalVAE(8)).name == "multimnist" and not E._family(M.MultimodalVAE(8)).text_only


# ====================================================================================================== the yardsticks
_G = {}


def _setup(D, H=50):
    if (D, H) not in _G:
        P, inp = TM.make_params(D, H), TM.make_inputs(D, H)
        _G[(D, H)] = (P, inp) + TM.gates(P, inp)
    return _G[(D, H)]


@pytest.mark.parametrize("D", [1, 20, 127])
def test_gates_see_the_faults(D, capsys):
    """the gates at H = 50 (printed), and: an ignored last latent column, row 16 answered with another row's result, ignored keep
    masks and hidden unit 49 left out each miss at least one comparison; the emulation itself passes"""
    P, inp, gate, ref, emu = _setup(D)
    with capsys.disabled():
        print("\ngates H=50 D=%d: words %.3e, encoder output %.3e, dz %.3e, gradients %.3e (4 x emulation)"
              % (D, gate["words"], gate["encout"], gate["dz"], gate["grads"]))
    assert all(0 < gate[k] < 0.1 for k in gate)
    bad, _ = TM.violations(TM.run_full(P, inp, rounded=True), ref, gate)
    assert not bad, bad
    for fault in TM.FAULTS:
        bad, _ = TM.violations(TM.run_full(P, inp, fault=fault), ref, gate, fault)
        assert bad, "the comparisons do not see the fault %r at D=%d" % (fault, D)
    # each quantity on its own: words see the mask, the column and the unit; the encoder output sees the unit and the row
    e = {f: TM.errors(TM.run_full(P, inp, fault=f), ref) for f in TM.FAULTS}
    assert e["mask"]["words"] > gate["words"] and e["last_column"]["words"] > gate["words"] and e["unit"]["words"] > gate["words"]
    assert e["unit"]["encout"] > gate["encout"] and e["row16"]["encout"] > gate["encout"] and e["row16"]["words"] > gate["words"]
    assert e["last_column"]["dz"] > gate["dz"] and e["unit"]["grads"] > gate["grads"]


@pytest.mark.parametrize("D", [1, 20, 100, 127])
def test_free_running_inputs_have_wide_margins(D, capsys):
    """the inputs of the free-running token comparison: the float64 top-two margin at every (row, step) is at least 10 x the words
    gate, so the engine's tokens must equal float64's on every row; a stand-in engine with a fault gets a token wrong"""
    P, inp, ref, margin, g_words = TM.free_running_case(D, 50)
    with capsys.disabled():
        print("\nfree-running H=50 D=%d: smallest margin %.3e, words gate %.3e" % (D, margin, g_words))
    assert margin >= 10 * g_words
    assert inp["z"].shape[0] == 23
    emu = TM.run_forward(P, inp, rounded=True, free_running=True)
    assert torch.equal(emu["tokens"], ref["tokens"])
    assert not torch.equal(TM.run_forward(P, inp, fault="unit", free_running=True)["words"], ref["words"])


def test_row_independence_check_sees_a_leak():
    P, inp, _, _, _ = _setup(20)

    def by_row(i, fault=None):       # every row evaluated alone: independent of its batch by construction
        rows = [TM.run_forward(P, TM.take_rows(i, [r])) for r in range(i["z"].shape[0])]
        out = {k: torch.cat([r[k] for r in rows]) for k in rows[0]}
        return {k: TM._row16(v, fault) for k, v in out.items()}

    ok = TM.row_independence_violations(by_row, inp)
    assert not ok, ok
    assert TM.row_independence_violations(lambda i: by_row(i, "row16"), inp)


def test_zero_embedding_is_the_same_function():
    """H = 50 parameters inside an H = 100 model with every added entry zero: the same outputs, the same gradients on the kept
    entries, exactly zero gradients on the added ones -- in float64 this holds to rounding, which is what the GPU cross-check builds on"""
    D = 20
    P, inp, _, ref, _ = _setup(D)
    Q, M = TM.embed_into(P, D)
    assert [(k, tuple(v.shape)) for k, v in Q.items()] == TM.param_shapes(D, 100)
    inp100 = dict(inp, keep=torch.cat((inp["keep"], torch.ones_like(inp["keep"])), dim=2))
    big = TM.run_full(Q, inp100)
    assert float((big["words"] - ref["words"]).abs().max()) <= 1e-12 and float((big["encout"] - ref["encout"]).abs().max()) <= 1e-12
    kept = TM.extract_from(big["grads"], M)
    for n, m in M.items():
        if bool(m.any()):
            assert float(big["grads"][n][m].abs().max()) == 0.0, n
        assert float((kept[n] - ref["grads"][n].reshape(-1)).abs().max()) <= 1e-12, n
