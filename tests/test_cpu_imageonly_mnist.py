"""MNIST's uni-modal image VAE (mnist/model.py:188-232, mnist/imageonly/*) without a GPU: the module's keys against the recorded ones
(and the live reference class where a checkout is at hand), the loss against the float64 restatement, the checkpoint dict, the
driver's flags, and the gates of the GPU test seeing each kind of fault."""
import ctypes as C
import importlib.util
import os

import pytest
import torch

import imageonly_mnist_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("MMVAE_REFERENCE", "/root/reference")


def test_keys_equal_the_reference():
    from multimodal_vae_amd import mnist as M
    recorded = IR.recorded_keys()
    vae = M.VAE(20)
    assert M.ImageVAE is M.VAE and vae.n_latents == 20
    sd = vae.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == recorded
    assert len(recorded) == 32 and recorded[0] == ("encoder.0.weight", (400, 784)) and recorded[-1] == ("decoder.6.bias", (784,))
    assert not any(".net." in k for k, _ in recorded)
    for pre in ("encoder.1", "encoder.4", "decoder.1", "decoder.4"):
        assert {pre + ".running_mean", pre + ".running_var", pre + ".num_batches_tracked"} <= set(sd)
    # a reference checkpoint loads strict; the MMVAE's keys do not
    ref_sd = {k: (torch.zeros(s) if s else torch.zeros((), dtype=torch.long)) for k, s in recorded}
    M.VAE(20).load_state_dict(ref_sd, strict=True)
    with pytest.raises(RuntimeError):
        M.VAE(20).load_state_dict({IR.plan_name(k): v for k, v in ref_sd.items()}, strict=True)
    # every key has the plan's name of the same shape, and the image parameters lead the plan's table
    names = IR.image_names(20)
    own = [M.VAE.plan_name(k) for k, _ in vae.named_parameters()]
    assert own == names and [n for n, _ in IR.R.param_table("mnist", 20)][:len(names)] == names
    assert [n for n, _ in vae._twin.named_parameters()] == names
    # other latent sizes keep the layout
    assert [k for k in M.VAE(8).state_dict()] == [k for k, _ in recorded]
    path = os.path.join(REFERENCE, "mnist", "model.py")
    if os.path.exists(path):                        # the live class, where a checkout of the reference is present
        spec = importlib.util.spec_from_file_location("reference_mnist_model", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        live = mod.VAE(20).state_dict()
        assert [(k, tuple(v.shape)) for k, v in live.items()] == recorded
        M.VAE(20).load_state_dict(live, strict=True)


def test_loss_equals_the_restatement():
    from multimodal_vae_amd import mnist as M
    B, D = 5, 20
    image, eps = IR.inputs(B, D)
    with torch.no_grad():
        recon, mu, lv = IR.forward(IR.params(D), image, True, eps)
    want = IR.loss_function(recon, image, mu, lv)
    got = M.imageonly_loss(recon, image.double().view(B, 1, 28, 28), mu, lv)
    assert got.dtype == torch.float64 and abs(float(got) - float(want)) <= 1e-15 * abs(float(want))
    # (mean BCE + KLD / 784) / B, term by term
    bce = torch.nn.functional.binary_cross_entropy(recon, image.double())
    assert abs(float(want) - float((bce + IR.kl_sum(mu, lv) / 784) / B)) <= 1e-15
    # ... which is what the engine forms from its sums with lambda_x = 1 / B, kl_lambda = 1 / 784
    bce_sum = float(bce) * B * 784
    assert abs((1.0 / B) * bce_sum / (B * 784) + (1.0 / 784) * float(IR.kl_sum(mu, lv)) / B - float(want)) <= 1e-15
    # eval mode: z == mu, the running statistics are read and stay
    p = IR.params(D)
    before = {k: v.clone() for k, v in p.items()}
    with torch.no_grad():
        r2, mu2, _ = IR.forward(p, image, False, eps)
    assert all(torch.equal(before[k], p[k]) for k in p) and not torch.equal(r2, recon)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        IR.forward(IR.params(D), image[:1], True, eps[:1])


def test_checkpoint_round_trip_and_driver_defaults(tmp_path, monkeypatch):
    import json
    from multimodal_vae_amd import evaluate as E, mnist as M, train_imageonly as T
    a = T.build_parser(T.dataset_of(["--dataset", "mnist"])).parse_args(["--dataset", "mnist"])
    with open(IR.GOLDEN) as fp:
        want = json.load(fp)["train_defaults"]                     # mnist/imageonly/train_imageonly.py:77-88
    assert {k: getattr(a, k) for k in want} == want
    assert (a.data, a.test_data, a.synthetic, a.out, a.results, a.seed) == ('./data', '', 0, './trained_models', './results', 1234)
    assert not hasattr(a, "anneal_kl") and T.kl_lambdas("mnist", 3) == [1.0 / 784] * 3
    assert T.build_parser("celeba").parse_args([]).epochs == 10 and T.build_parser("celeba").parse_args([]).out == './trained_models/image_only'
    with pytest.raises(SystemExit):                                # no CPU fallback
        T.main(["--dataset", "mnist", "--synthetic", "64"])

    class _Eng:                                                    # what image_adam_state_dict reads of an engine
        lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8

        def __init__(self, D):
            offs, o = [], 0
            for n, s in IR.R.param_table("mnist", D):
                offs.append((n, s, o))
                o += int(torch.tensor(s).prod())
            self.state = type("S", (), {"table": offs})()
            self.adam_state = torch.tensor([3, 0])
            self.exp_avg, self.exp_avg_sq = torch.arange(o, dtype=torch.float32), torch.ones(o)

    vae = M.VAE(20)
    d = T.checkpoint_dict(vae, _Eng(20), 0.5, 20)
    assert sorted(d) == ["best_loss", "n_latents", "optimizer", "state_dict"] and d["n_latents"] == 20 and d["best_loss"] == 0.5
    assert [(k, tuple(v.shape)) for k, v in d["state_dict"].items()] == IR.recorded_keys()
    opt = torch.optim.Adam(vae.parameters(), lr=1e-3)
    opt.load_state_dict(d["optimizer"])                            # torch.optim.Adam.state_dict() layout, the image parameters alone
    assert len(d["optimizer"]["state"]) == len(list(vae.parameters())) == 20 and float(d["optimizer"]["state"][0]["step"]) == 3.0
    assert d["optimizer"]["state"][1]["exp_avg"][0] == 400 * 784   # the flat offset of encoder.0.bias
    path = str(tmp_path / "ck.pth.tar")
    with torch.no_grad():
        vae.encoder[0].weight.fill_(0.25)
        vae.decoder[4].running_var.fill_(3.0)
    torch.save(T.checkpoint_dict(vae, _Eng(20), 0.5, 20), path)
    back = M.load_checkpoint_imageonly(path)
    assert isinstance(back, M.VAE) and back.n_latents == 20
    assert all(torch.equal(v, back.state_dict()[k]) for k, v in vae.state_dict().items())
    assert E.is_imageonly_checkpoint(path) and not E.is_textonly_checkpoint(path)
    fam = E._family(back)
    assert fam.image_only and fam.name == "mnist" and fam.image_shape == (784,) and (fam.T, fam.V) == (1, 1)
    assert not E._family(M.MultimodalVAE(8)).image_only
    for post in ("joint", "text"):
        with pytest.raises(ValueError, match="image posterior alone"):
            E.log_marginal(back, [(torch.zeros(2, 784), None)], n_particles=2, posterior=post)
    p = E._parser()
    assert p.parse_args(["test_imageonly", "ck", "--dataset", "mnist", "--synthetic", "64"]).dataset == "mnist"
    assert p.parse_args(["sample", "ck", "--dataset", "mnist", "--condition_on_image", "3", "--data", "f.pt"]).condition_on_image == "3"
    assert p.parse_args(["sample", "ck"]).dataset == "multimnist"                      # the default stays


def test_refusals_and_exports():
    from multimodal_vae_amd import _lib, core, mnist as M
    assert core.FusedImageStep.SIDE["mnist"] == 28 and core.FusedImageStep.CHANNELS["mnist"] == 1
    with pytest.raises(M.MMVAEError, match="MNIST has one on its fp32 plan"):
        core.FusedImageStep(type("S", (), {"API": "mmtext"})(), 8)
    with pytest.raises(M.MMVAEError, match="precision 'bf16'"):
        core.FusedImageStep(type("S", (), {"API": "mnist", "precision": "bf16"})(), 8)

    class _Eng(core.FusedImageStep):
        def __init__(self):
            self.B, self.side, self.channels, self.flat_images = 4, 28, 1, True
    for shape in ((4, 3, 28, 28), (4, 28, 28), (5, 784), (4, 783)):
        with pytest.raises(M.MMVAEError, match=r"expected images of shape \(4, 1, 28, 28\)"):
            _Eng().forward_backward(torch.zeros(shape))
    with pytest.raises(M.MMVAEError, match="no CPU fallback"):
        M.VAE(20)(torch.zeros(2, 1, 28, 28))
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    for fn in ("mmvae_mnist_image_step", "mmvae_mnist_image_step_workspace_bytes", "mmvae_mnist_iw_score_image", "mmvae_mnist_strip_max_rows",
               "mmvae_mnist_strip_route", "mmvae_mnist_lin_bn_act_fwd", "mmvae_mnist_lin_dgrad_bn_bwd"):
        assert fn in _lib.SIGNATURES and hasattr(lib, fn) and fn + "(" in hdr
    # the strip kernels' row cap and switch: the default is on, up to the cap; the strip route refuses more rows on the host
    cap = lib.mmvae_mnist_strip_max_rows()
    assert cap == 512 and lib.mmvae_mnist_strip_route(cap) == 1 and lib.mmvae_mnist_strip_route(cap + 1) == 0
    assert lib.mmvae_debug_set(b"mnist_strip", 0) == 0 and lib.mmvae_mnist_strip_route(2) == 0
    assert lib.mmvae_debug_set(b"mnist_strip", -1) == 0 and lib.mmvae_mnist_strip_route(2) == 1
    assert lib.mmvae_mnist_lin_bn_act_fwd(1, None, 784, *([None] * 7), cap + 1, 400, 784, 1, *([None] * 4)) != 0       # before any GPU call
    assert "null argument" in lib.mmvae_last_error().decode()
    assert "int mmvae_mnist_image_step(mmvae_mnist_t*, const mmvae_image_step_io*, int training, int do_backward, void* stream);" in hdr
    # plans exist without a GPU: the one-pass carve is smaller than the 3-pass one; a bf16 plan has none; n_latents 6 is no plan
    h = lib.mmvae_mnist_create_p(20, 128, 0)
    assert h and 0 < lib.mmvae_mnist_image_step_workspace_bytes(h) < lib.mmvae_mnist_workspace_bytes(h)
    io = _lib.ImageStepIO()
    assert lib.mmvae_mnist_image_step(h, C.byref(io), 1, 1, None) != 0             # an unbound plan: refused before any GPU call
    assert "bound" in lib.mmvae_last_error().decode()
    lib.mmvae_mnist_destroy(h)
    hb = lib.mmvae_mnist_create_p(20, 128, 1)
    assert hb and lib.mmvae_mnist_image_step_workspace_bytes(hb) == 0
    lib.mmvae_mnist_destroy(hb)
    assert not lib.mmvae_mnist_create_p(6, 8, 0) and "multiple of 4" in lib.mmvae_last_error().decode()


# ====================================================================================================== the yardsticks
@pytest.mark.parametrize("B,D", IR.CASES)
def test_gates_see_the_faults(B, D, capsys):
    """At the (B, D) of the GPU test: a float32 evaluation of the same formulas stays within every gate (worst ratios printed); a dropped loss
    term, a dropped 1 / B, a dropped or biased BatchNorm update each trip at least one."""
    ref = IR.run(D, B, True)
    fails, ratios = IR.check(ref, IR.run(D, B, True, dtype=torch.float32))
    worst = sorted(ratios.items(), key=lambda kv: -kv[1])[:4]
    with capsys.disabled():
        print("\nmnist image step gates B=%d D=%d, float32 restatement's worst error / gate: %s" % (B, D, "; ".join("%s %.2f" % kv for kv in worst)))
    assert not fails, fails
    assert IR.relu_margin(D, B) >= IR.RELU_MARGIN                 # what makes (B, D) a case (eval mode has no gradient: ReLU itself is continuous)
    assert IR.check(ref, ref)[0] == []
    seen = {}
    for fault in ("no_kl", "no_bce", "no_1_over_B", "no_bn_update", "biased_running_var"):
        seen[fault] = " | ".join(IR.check(ref, IR.run(D, B, True, fault=fault))[0])
        assert seen[fault], "the gates do not see the fault %r at B=%d D=%d" % (fault, B, D)
    assert "loss" in seen["no_kl"] and "gradient image_encoder.net.6" in seen["no_kl"]
    assert "loss" in seen["no_bce"] and "gradient image_decoder.net.6.weight" in seen["no_bce"]
    assert "loss" in seen["no_1_over_B"] and "gradient" in seen["no_1_over_B"]
    assert "running_mean" in seen["no_bn_update"] and "num_batches_tracked" in seen["no_bn_update"] and "loss" not in seen["no_bn_update"]
    assert "running_var" in seen["biased_running_var"] and "running_mean" not in seen["biased_running_var"]
    # eval mode: the running statistics stay, z = mu
    ev = IR.run(D, B, False)
    assert IR.check(ev, IR.run(D, B, False, dtype=torch.float32), training=False)[0] == []
    assert all(v == 0 for v in ev["nbt"].values()) and "recon" in " ".join(IR.check(ev, IR.run(D, B, False, fault="eval_draws_eps"), training=False)[0])
