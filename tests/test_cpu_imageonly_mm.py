"""CPU tests of MultiMNIST's image-only VAE baseline: ImageVAE's state_dict against the recorded reference names and shapes, the
refusals of the host, the train_imageonly driver's command line, KL schedule and checkpoint dict for this data set, what evaluate
makes of such a checkpoint, and the yardsticks of tests/test_gpu_imageonly_mm.py's waist comparison (tests/imageonly_mm_ref.py): the
float64 reference's own stand-in stays within every one of them, and each fault the GPU test is there for exceeds at least one."""
import ctypes as C
import json
import os

import pytest
import torch

from oracle import mmvae_ref as R
import imageonly_mm_ref as IM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "multimnist_imagevae_keys.json")


# ====================================================================================================== the Python face
@pytest.mark.parametrize("D", [20, 100])
def test_state_dict_keys_are_the_references(D):
    from multimodal_vae_amd import multimnist as M
    vae = M.ImageVAE(D)
    sd = vae.state_dict()
    recorded = json.load(open(GOLDEN))[str(D)]
    assert [[k, list(v.shape)] for k, v in sd.items()] == recorded
    assert IM.state_dict_shapes(D) == recorded
    assert recorded[0][0] == "encoder.features.0.weight" and recorded[-1][0] == "decoder.hallucinate.9.weight" and len(recorded) == 46
    assert [n for n, _ in vae.named_children()] == ["encoder", "decoder"]
    assert isinstance(vae.encoder, M.ImageEncoder) and isinstance(vae.decoder, M.ImageDecoder)
    for meth in ("encode", "decode", "reparametrize", "forward"):
        assert callable(getattr(vae, meth))
    assert vae.encoder._mmvae_root() is vae and vae.decoder._mmvae_root() is vae and vae._core.prefix == "image_"
    assert M.ImageVAE().n_latents == 20
    # a reference checkpoint loads strict: the recorded names with the recorded shapes
    ref_sd = {k: (torch.zeros(s) if s else torch.zeros((), dtype=torch.long)) for k, s in recorded}
    M.ImageVAE(D).load_state_dict(ref_sd, strict=True)
    with pytest.raises(RuntimeError):
        M.ImageVAE(D).load_state_dict({"image_" + k: v for k, v in ref_sd.items()}, strict=True)      # the MMVAE's keys are not ImageVAE's


def test_refusals():
    from multimodal_vae_amd import _lib, core, evaluate as E, multimnist as M
    # a family without an image-only step
    for api in ("mnist", "mmtext"):
        with pytest.raises(M.MMVAEError, match="CelebA, COCO and MultiMNIST"):
            core.FusedImageStep(type("S", (), {"API": api})(), 8)
    assert core.FusedImageStep.SIDE["mm"] == 50 and core.FusedImageStep.CHANNELS["mm"] == 1

    # a wrong image shape: refused by the engine before anything is enqueued
    class _Eng(core.FusedImageStep):
        def __init__(self):
            self.B, self.side, self.channels = 4, 50, 1
    for shape in ((4, 3, 50, 50), (4, 1, 64, 64), (5, 1, 50, 50), (4, 2500)):
        with pytest.raises(M.MMVAEError, match=r"expected images of shape \(4, 1, 50, 50\)"):
            _Eng().forward_backward(torch.zeros(shape))
    # no CPU fallback behind the modules
    with pytest.raises(M.MMVAEError, match="no CPU fallback"):
        M.ImageVAE(20)(torch.zeros(2, 1, 50, 50))
    # the posterior
    iv = M.ImageVAE(8)
    fam = E._family(iv)
    assert fam.image_only and not fam.text_only and fam.name == "multimnist" and fam.image_shape == (1, 50, 50) and (fam.T, fam.V) == (1, 1)
    for post in ("joint", "text", "attrs", "nonsense"):
        with pytest.raises(ValueError, match="image posterior alone|must be one of"):
            E.log_marginal(iv, [(torch.zeros(2, 1, 50, 50), None)], n_particles=2, posterior=post)
    with pytest.raises(ValueError, match="image posterior alone"):
        E._proposal(iv, torch.zeros(2, 1, 50, 50), None, "joint")
    # the C entry points exist, under the shared io struct
    lib = _lib.load()
    for fn in ("mmvae_mm_image_step", "mmvae_mm_image_step_workspace_bytes", "mmvae_mm_iw_score_image"):
        assert fn in _lib.SIGNATURES and hasattr(lib, fn)
    hdr = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    assert "int mmvae_mm_image_step(mmvae_mm_t*, const mmvae_image_step_io*, int training, int do_backward, void* stream);" in hdr
    for D in (1, 20, 100, 127):
        h = lib.mmvae_mm_create(D, 16)
        assert h
        assert lib.mmvae_mm_image_step_workspace_bytes(h) == lib.mmvae_mm_module_workspace_bytes(h) > 0
        assert lib.mmvae_mm_image_step_workspace_bytes(h) < lib.mmvae_mm_workspace_bytes(h)
        off = lib.mmvae_mm_debug_offset(h, b"image_step:z_bf")
        assert 0 < off < lib.mmvae_mm_debug_offset(h, b"z_bf") and lib.mmvae_mm_debug_offset(h, b"image_step:nothing") == -1
        io = _lib.ImageStepIO()
        assert lib.mmvae_mm_image_step(h, C.byref(io), 1, 1, None) != 0          # an unbound plan: refused before any GPU call
        assert "bound" in lib.mmvae_last_error().decode()
        lib.mmvae_mm_destroy(h)


def test_driver_flags_schedule_and_checkpoint(monkeypatch):
    from multimodal_vae_amd import multimnist as M, train_imageonly as T
    assert T.dataset_of(["--dataset", "multimnist", "--cuda"]) == "multimnist"
    a = T.build_parser("multimnist").parse_args(["--dataset", "multimnist"])
    # multimnist/train_imageonly.py:46-60
    assert (a.n_latents, a.batch_size, a.epochs, a.lr, a.log_interval, a.anneal_kl, a.cuda) == (20, 128, 10, 1e-3, 10, False, False)
    assert (a.data, a.synthetic, a.out, a.results, a.seed, a.generate) == ('./data', 0, './trained_models/image_only', './results/image_only', 1234, False)
    assert (a.mnist_train, a.mnist_test, a.epoch_size, a.min_digits, a.max_digits) == ('', '', 60000, 0, 2)
    assert not hasattr(T.build_parser("celeba").parse_args([]), "generate")
    # multimnist/train_imageonly.py:131-139: 1e-3, or with --anneal_kl the next value every 5 epochs, the last one kept
    assert T.kl_lambdas("multimnist", 12) == [1e-3] * 12
    seen = T.kl_lambdas("multimnist", 40, anneal_kl=True)
    assert seen[:5] == [1e-5] * 5 and seen[5] == 1e-4 and seen[10] == 1e-3 and seen[15] == 1e-2 and seen[20] == 1e-1 and seen[25:] == [1.0] * 15
    assert T.kl_lambdas("celeba", 7, anneal_kl=True) == [1e-3] * 7 and T.kl_lambdas("coco", 12) == [5e-4] * 12      # the others keep theirs
    with pytest.raises(SystemExit):                              # no CPU fallback
        T.main(["--dataset", "multimnist", "--synthetic", "64"])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no CPU fallback"):
        T.main(["--dataset", "multimnist", "--cuda", "--synthetic", "64"])

    class _Eng:                                                   # what image_adam_state_dict reads of an engine
        lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8

        def __init__(self, D):
            offs, o = [], 0
            for n, s in R.param_table("multimnist", D):
                offs.append((n, s, o))
                o += int(torch.tensor(s).prod())
            self.state = type("S", (), {"table": offs})()
            self.adam_state = torch.tensor([3, 0])
            self.exp_avg, self.exp_avg_sq = torch.zeros(o), torch.ones(o)

    vae = M.ImageVAE(20)
    d = T.checkpoint_dict(vae, _Eng(20), 0.5, 20)
    assert sorted(d) == ["best_loss", "n_latents", "optimizer", "state_dict"] and d["n_latents"] == 20 and d["best_loss"] == 0.5
    assert list(d["state_dict"]) == IM.state_dict_keys(20)
    opt = torch.optim.Adam(vae.parameters(), lr=1e-3)
    opt.load_state_dict(d["optimizer"])                           # torch.optim.Adam.state_dict() layout, the image parameters alone
    assert len(d["optimizer"]["state"]) == len(list(vae.parameters())) == 28 and float(d["optimizer"]["state"][0]["step"]) == 3.0


def test_evaluate_knows_the_checkpoint(tmp_path):
    from multimodal_vae_amd import evaluate as E, multimnist as M
    p = E._parser()
    assert p.parse_args(["test_imageonly", "ck.pth.tar", "--synthetic", "64"]).dataset == "celeba"          # the default stays
    assert p.parse_args(["test_imageonly", "ck.pth.tar", "--dataset", "multimnist", "--synthetic", "64"]).dataset == "multimnist"
    iv, tv, mv = (str(tmp_path / n) for n in ("i.pth.tar", "t.pth.tar", "m.pth.tar"))
    torch.save({"state_dict": M.ImageVAE(8).state_dict(), "n_latents": 8}, iv)
    torch.save({"state_dict": M.TextVAE(8).state_dict(), "n_latents": 8}, tv)
    torch.save({"state_dict": M.MultimodalVAE(8).state_dict(), "n_latents": 8}, mv)
    assert E.is_imageonly_checkpoint(iv) and not E.is_textonly_checkpoint(iv)
    assert E.is_textonly_checkpoint(tv) and not E.is_imageonly_checkpoint(mv) and not E.is_textonly_checkpoint(mv)
    vae = M.load_checkpoint_imageonly(iv)
    assert isinstance(vae, M.ImageVAE) and vae.n_latents == 8
    assert E._family(M.MultimodalVAE(8)).name == "multimnist" and not E._family(M.MultimodalVAE(8)).image_only


# ====================================================================================================== the yardsticks
CASES = [(5, 20), (16, 20), (23, 20), (33, 20), (23, 100)]          # the (B, D) of the GPU test's waist comparison


@pytest.mark.parametrize("B,D", CASES)
def test_waist_gates_see_the_faults(B, D, capsys):
    """The stand-in for the kernel pair in the kernel's arithmetic stays within every yardstick (worst ratios printed); with each of
    the faults it exceeds at least one, at the shapes the GPU test uses."""
    c = IM.waist_inputs(B, D)
    ldz, lde = (D + 1 + 7) // 8 * 8, (2 * D + 7) // 8 * 8
    fails, ratios = IM.check_waist(c, IM.emulate(c, ldz, lde))
    with capsys.disabled():
        print("\nwaist yardsticks B=%d D=%d, stand-in's worst error / yardstick: %s" % (B, D, " ".join("%s %.2f" % kv for kv in ratios.items())))
    assert not fails, fails
    # the float64 reference itself (stored the way the kernel stores: bf16 where it stores bf16) never trips a gate
    fref, _ = IM.waist_forward(c)
    bref, _ = IM.waist_backward(c, dict(mu=fref["mu"], logvar=fref["logvar"], y2=IM.bf(fref["y2"])))
    exact = dict(fref, **bref)
    for k in ("y2", "ay2", "dy2", "dy1"):
        exact[k] = IM.bf(exact[k])
    exact["d_enc_out"] = IM.bf(bref["d_enc_out"])
    zf = torch.zeros(B, ldz, dtype=torch.float64)
    zf[:, :D], zf[:, D] = IM.bf(fref["z"]), 1.0
    df = torch.zeros(B, lde, dtype=torch.float64)
    df[:, :2 * D] = exact["d_enc_out"]
    exact.update(z_bf=zf[:, :D], z_bf_full=zf, d_enc_out_full=df)
    fails, _ = IM.check_waist(c, exact)
    assert not fails, fails
    for fault in IM.FAULTS:
        if fault == "last_block" and B % IM.TR == 0:
            continue                                             # (an exact block count has no partial block to leave out)
        fails, _ = IM.check_waist(c, IM.emulate(c, ldz, lde, fault))
        assert fails, "the comparisons do not see the fault %r at B=%d D=%d" % (fault, B, D)
    # which comparison sees which fault
    seen = {f: " ".join(IM.check_waist(c, IM.emulate(c, ldz, lde, f))[0]) for f in IM.FAULTS}
    assert "z " in seen["eps"] and "d_enc_out" in seen["eps"]
    assert "d_enc_out" in seen["kl_coef"] and "d_bias" in seen["kl_coef"] and "z " not in seen["kl_coef"]
    assert "ay2" in seen["mask2"] and "dy2" in seen["mask2"]
    assert seen["z_bf_one"] == "z_bf[:, D] != 1"
    if B % IM.TR:
        assert "d_bias" in seen["last_block"] and "mu" in seen["last_block"] and "z_bf[:, D] != 1" in seen["last_block"]


def test_eval_mode_and_no_dropout_have_their_own_references():
    """eval mode: z == mu and no eps term in the gradient; without dropout the masks are not read"""
    c = dict(IM.waist_inputs(23, 20), training=False, drop=False)
    f, _ = IM.waist_forward(c)
    assert torch.equal(f["z"], f["mu"])
    fails, _ = IM.check_waist(c, IM.emulate(c, 24, 40))
    assert not fails, fails
    c2 = dict(c, m2=torch.zeros_like(c["m2"]), eps=torch.zeros_like(c["eps"]))
    assert torch.equal(IM.waist_forward(c2)[0]["encout"], f["encout"])


def test_step_reference_is_the_oracles():
    """tests/imageonly_mm_ref.py's model: the oracle's image pass without the experts' 1e-8, and multimnist_loss without text"""
    B, D = 3, 20
    P = IM.params64(D)
    image = R.formula_inputs("multimnist", B)[0]
    eps = R.formula_eps(B, D, 1)
    with torch.no_grad():
        loss, (recon, mu, lv) = IM.step_loss(P, image, True, eps, None, 0.0, 1e-3)
        P2 = IM.params64(D)
        o = R.multimnist_image_encoder(P2, image.double(), True, None, drop_p=0.0)
        assert torch.equal(o[:, :D], mu) and torch.equal(o[:, D:], lv)
        pm, pl = R.product_of_experts(mu.unsqueeze(0), lv.unsqueeze(0))
        assert not torch.equal(pl, lv)                           # what the 3-pass route with passes=(False, True, False) would use
        bce = torch.nn.functional.binary_cross_entropy(recon.reshape(-1, 2500), image.double().reshape(-1, 2500))
        assert abs(float(loss) - float(bce + 1e-3 * R.kl_sum(mu, lv) / B)) <= 1e-15
    assert recon.shape == (B, 1, 50, 50) and IM.MASK_WIDTHS == (400, 200)
