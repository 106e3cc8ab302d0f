"""GPU tests of the uni-modal image VAE baselines (CelebA, COCO): the one-expert latent block alone, the one-pass fused step against the
float64 oracle (tests/imageonly_ref.py), the nn.Module / trainer / driver face and the log p(x) estimator.

Gates of the step are the project's own for these kernels (tests/test_gpu_celeba.py, tests/test_gpu_coco.py): loss rel 1e-3 | mu / logvar
abs 1e-2 | per-tensor gradient rel-L2 CelebA 6e-2 (B = 4, 5) / 4e-2 (B = 32), COCO 4.5e-2 | total gradient norm 2e-3 | running mean abs
2e-3, running variance rel 2e-2 + 1e-4.  No gate is widened.  Every test prints what it measured (run with -s).
"""
import math
import os

import numpy as np
import pytest
import torch

from oracle import mmvae_ref as R
from gradcheck import check_gradients
import imageonly_ref as IR

pytestmark = pytest.mark.gpu

IMG = ("image_encoder.", "image_decoder.")
COCO_T = 4          # caption length of the COCO plans built here: no caption runs in an image-only step


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _state(family, D, dev):
    """The MMVAE's plan state of the family with the formula parameters of EVERY tensor, the second modality's included."""
    from multimodal_vae_amd import core
    st = core.CelebaState(D, dev) if family == "celeba" else core.CocoState(D, dev, COCO_T)
    P = R.formula_params(family, D)
    assert [t[0] for t in st.table] == [n for n, _ in R.param_table(family, D)]
    for n, shape, off in st.table:
        st.params[off:off + P[n].numel()] = P[n].detach().reshape(-1).to(dev)
    return st


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


# ====================================================================================================== latent1 alone
def _latent_inputs(B, D, seed):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(B, D, generator=g)
    lv = torch.linspace(-20.0, 2.0, B * D).view(B, D) if B * D > 1 else torch.full((1, 1), -20.0)
    lv = lv.flatten()[torch.randperm(B * D, generator=g)].view(B, D).contiguous()
    eps = torch.randn(B, D, generator=g)
    dz = torch.randn(B, D, generator=g)
    return torch.cat((mu, lv), dim=1).contiguous(), eps, dz


@pytest.mark.parametrize("B,D", [(1, 1), (3, 4), (5, 20), (7, 100), (4, 124)])
def test_latent1_alone(B, D):
    """mmvae_latent1_fwd / _bwd on their own operands.  mu / logvar are the input halves bit for bit (a copy through the experts' 1e-8
    would read -18.2 at logvar = -20), z is mmvae_reparam_fwd's bit for bit, eval mode gives z == mu, the pads of z_bf (column D is the
    1.0 of upsample.0's folded bias, as in latent3) and of d_enc_out are exact, two calls give equal bits.
    KL sum against float64: at most 4x the error of mmvae_kl_fwd on the same inputs, and below 1e-4 relative (a bf16-sized error
    would be 4e-3).  d_enc_out within one bf16 ulp (2^-8 relative) of the float64 formula, the bias sums within 2 B 2^-24 sum|terms|.
    Measured on MI355X, KL relative error latent1 | mmvae_kl_fwd (whose atomics make it vary from run to run; two runs):
    (1,1) 2.72e-8 | 2.72e-8;  (3,4) 8.44e-9 | 8.44e-9;  (5,20) 3.27e-8 | 3.27e-8;  (7,100) 1.25e-8 | 8.75e-8 and 1.25e-8;
    (4,124) 2.27e-8 | 2.27e-8.  d_enc_out worst 3.9e-3 (gate 3.9e-3 = 2^-8: bf16 rounding is at most 2^-9 of the value, the figure
    is relative to the float64 value); bias sums worst 1.05e-7 of sum|terms| at B = 4 (gate 4.77e-7), 8.3e-8 at B = 1 (gate 1.19e-7)."""
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd._ops import stream
    dev = _dev()
    enc_out, eps, dz = _latent_inputs(B, D, 100 * B + D)
    assert float(enc_out[:, D:].min()) == -20.0
    e_d, eps_d, dz_d = enc_out.to(dev), eps.to(dev), dz.to(dev)
    ldz = (D + 1 + 7) // 8 * 8 + 8            # more than one pad column behind the 1.0
    ld = 2 * D + 5
    nscr = call("mmvae_latent1_scratch_floats", B, D)
    assert nscr >= 128

    def fwd(training):
        f32 = dict(dtype=torch.float32, device=dev)
        mu, lv, z = torch.full((B, D), 7.0, **f32), torch.full((B, D), 7.0, **f32), torch.full((B, D), 7.0, **f32)
        zb = torch.full((B, ldz), 7.0, dtype=torch.bfloat16, device=dev)
        kl = torch.zeros(1, **f32)
        scr = torch.full((nscr,), float("nan"), **f32)
        call("mmvae_latent1_fwd", ptr(e_d), ptr(eps_d) if training else None, B, D, int(training), ptr(mu), ptr(lv), ptr(z), ptr(zb), ldz,
             ptr(kl), ptr(scr), stream())
        return mu, lv, z, zb, kl

    mu, lv, z, zb, kl = fwd(True)
    assert torch.equal(mu.cpu(), enc_out[:, :D]) and torch.equal(lv.cpu(), enc_out[:, D:])
    z_ref = torch.empty(B, D, dtype=torch.float32, device=dev)
    call("mmvae_reparam_fwd", ptr(mu.contiguous()), ptr(lv.contiguous()), ptr(eps_d), B * D, ptr(z_ref), stream())
    assert torch.equal(z, z_ref)
    assert torch.equal(zb[:, :D], z.to(torch.bfloat16))
    assert torch.equal(zb[:, D].float().cpu(), torch.ones(B)) and float(zb[:, D + 1:].float().abs().max()) == 0.0
    mu2, lv2, z2, zb2, kl2 = fwd(True)
    assert torch.equal(z, z2) and torch.equal(zb, zb2) and torch.equal(kl, kl2) and torch.equal(mu, mu2) and torch.equal(lv, lv2)
    mu_e, lv_e, z_e, zb_e, kl_e = fwd(False)
    assert torch.equal(z_e, mu_e) and torch.equal(mu_e, mu) and torch.equal(kl_e, kl)
    assert float(zb_e[:, D + 1:].float().abs().max()) == 0.0
    # KL sum: fixed order, and as accurate as the stand-alone op
    _, _, _, kl64 = IR.latent1_fwd(enc_out, eps, True)
    kl64 = float(kl64)
    kl_old = torch.zeros(1, dtype=torch.float32, device=dev)
    call("mmvae_kl_fwd", ptr(mu.contiguous()), ptr(lv.contiguous()), B * D, ptr(kl_old), stream())
    err_new, err_old = abs(float(kl.double()) - kl64) / abs(kl64), abs(float(kl_old.double()) - kl64) / abs(kl64)
    print("latent1 (B=%d, D=%d): KL sum %.9g, relative error %.3e; mmvae_kl_fwd %.3e" % (B, D, kl64, err_new, err_old))
    assert err_new <= 4 * err_old, (err_new, err_old)
    assert err_new < 1e-4
    kl_acc = torch.full((1,), 3.0, dtype=torch.float32, device=dev)                   # "+="
    scr = torch.zeros(nscr, dtype=torch.float32, device=dev)
    call("mmvae_latent1_fwd", ptr(e_d), ptr(eps_d), B, D, 1, ptr(mu2), ptr(lv2), ptr(z2), ptr(zb2), ldz, ptr(kl_acc), ptr(scr), stream())
    assert torch.equal(kl_acc, kl + 3.0)

    # ---- backward
    kl_coef = 1e-3 / B
    for training in (True, False):
        d_out = torch.full((B, ld), 7.0, dtype=torch.bfloat16, device=dev)
        bias = torch.zeros(2 * D, dtype=torch.float32, device=dev)
        slots = torch.arange(32 * 16, dtype=torch.float32, device=dev).view(32, 16).contiguous()
        loss_out = torch.zeros(16, dtype=torch.float32, device=dev)
        scr = torch.full((nscr,), float("nan"), dtype=torch.float32, device=dev)
        args = (ptr(mu), ptr(lv), ptr(eps_d) if training else None, ptr(dz_d), B, D, int(training), kl_coef, ptr(d_out), ld)
        call("mmvae_latent1_bwd", *args, ptr(bias), ptr(slots), ptr(loss_out), ptr(scr), stream())
        g64 = IR.latent1_bwd(enc_out[:, :D], enc_out[:, D:], eps, dz, kl_coef, training)
        got = d_out[:, :2 * D].double().cpu()
        rel = ((got - g64).abs() / g64.abs().clamp_min(1e-300)).max().item()
        assert rel <= 2.0 ** -8, rel
        assert float(d_out[:, 2 * D:].float().abs().max()) == 0.0
        s64, sabs = g64.sum(0), g64.abs().sum(0)
        berr = ((bias.double().cpu() - s64).abs() / sabs).max().item()
        print("latent1_bwd (B=%d, D=%d, training=%d): d_enc_out worst rel %.3e (gate 2^-8), bias sums worst err / sum|terms| %.3e (gate %.3e)"
              % (B, D, training, rel, berr, 2 * B * 2.0 ** -24))
        assert berr <= 2 * B * 2.0 ** -24, berr
        assert torch.equal(loss_out, slots.sum(0))
        bias2 = torch.full((2 * D,), 0.25, dtype=torch.float32, device=dev)            # "+=", fixed order: equal bits
        d_out2 = torch.empty_like(d_out)
        call("mmvae_latent1_bwd", *args[:8], ptr(d_out2), ld, ptr(bias2), None, None, ptr(scr), stream())
        assert torch.equal(bias2, bias + 0.25) and torch.equal(d_out2, d_out)


# ====================================================================================================== the step
CASES = [   # family, B, D, masks, per-tensor gate, running-variance note
    ("celeba", 4, 100, False, 6e-2), ("celeba", 4, 100, True, 6e-2), ("celeba", 5, 100, False, 6e-2), ("celeba", 5, 20, True, 6e-2),
    ("celeba", 32, 100, False, 4e-2),
    ("coco", 4, 100, False, 4.5e-2), ("coco", 4, 100, True, 4.5e-2), ("coco", 6, 100, False, 4.5e-2), ("coco", 6, 20, True, 4.5e-2),
]


@pytest.mark.parametrize("family,B,D,with_masks,tensor_tol", CASES)
def test_step_matches_oracle(family, B, D, with_masks, tensor_tol):
    """One training step of FusedImageStep (given eps, given or no dropout masks) against the float64 oracle without a product of
    experts.  Measured on MI355X (gates in brackets): loss rel <= 3.2e-5 (1e-3); mu / logvar abs <= 6.2e-3 CelebA, 1.8e-3 COCO (1e-2);
    worst gradient tensor CelebA B = 4: 2.3e-2, B = 5: 2.5e-2 (6e-2), B = 32: 2.0e-2 (4e-2), COCO 1.6e-2 .. 2.0e-2 (4.5e-2); total
    gradient norm <= 4.1e-4 (2e-3); running mean abs <= 2.1e-4 (2e-3), running variance rel <= 1.8e-4 (2e-2).  No gate is widened.  Every second-modality gradient is exactly 0 and its parameters keep their bits through optimizer steps;
    num_batches_tracked grows by 1 per step in the encoder and in the decoder, and not at all in the second modality."""
    from multimodal_vae_amd.core import FusedImageStep
    dev = _dev()
    st = _state(family, D, dev)
    P = IR.params64(family, D, requires_grad=True)
    image = R.formula_inputs(family, B)[0]
    eps = R.formula_eps(B, D, 1)
    masks, kw = None, {}
    if with_masks:
        g = torch.Generator().manual_seed(7 * B + D)
        ms = [(torch.rand(B, w, generator=g) >= 0.1).to(torch.uint8) for w in IR.MASK_WIDTHS[family]]
        masks = ms[0].float() if family == "celeba" else tuple(m.float() for m in ms)
        kw = {"enc_mask%d" % (i + 1): m.to(dev).contiguous() for i, m in enumerate(ms)}
    eng = FusedImageStep(st, B, kl_lambda=1e-3)
    eng.enc_dropout = with_masks
    assert eng.ws.numel() == st.module_workspace_bytes(B) < st.workspace_bytes(B)
    side = IR.SIDE[family]
    mu, lv = torch.zeros(B, D, device=dev), torch.zeros(B, D, device=dev)
    recon = torch.zeros(B, 3, side, side, device=dev)
    p0, nbt0, bn0 = st.params.clone(), st.bn_nbt.clone(), st.bn_stats.clone()
    img_d, eps_d = image.to(dev).contiguous(), eps.to(dev).contiguous()
    out = eng.forward_backward(img_d, True, True, eps=eps_d, mu=mu, logvar=lv, recon_image=recon, **kw)
    o_loss, (o_recon, o_mu, o_lv) = IR.step_loss(family, P, image, True, eps, masks, 0.1 if with_masks else 0.0, 1e-3)
    o_loss.backward()
    losses = out.losses().cpu()
    sums = eng.sums.cpu()
    l_err = abs(losses[0].item() - o_loss.item()) / abs(o_loss.item())
    mu_err, lv_err = (mu.cpu().double() - o_mu.detach()).abs().max().item(), (lv.cpu().double() - o_lv.detach()).abs().max().item()
    r_err = (recon.cpu().double() - o_recon.detach()).abs().max().item()
    assert l_err <= 1e-3, l_err
    assert losses[1].item() == 0.0 and losses[2].item() == 0.0
    assert all(float(sums[i]) == 0.0 for i in range(16) if i not in (0, 8)), sums
    assert mu_err <= 1e-2 and lv_err <= 1e-2, (mu_err, lv_err)
    assert r_err <= 2e-2, r_err
    g = st.grads.cpu()
    pairs, second = [], []
    for n, shape, off in st.table:
        (pairs if n.startswith(IMG) else second).append((n, g[off:off + _numel(shape)], P[n].grad))
    assert len(second) > 0
    for n, gh, gr in second:
        assert gr is None and float(gh.abs().max()) == 0.0, n
    worst, tot = check_gradients(pairs, tensor_tol, 2e-3, "%s image step B=%d D=%d masks=%d" % (family, B, D, with_masks))
    rm_err = rv_err = 0.0
    for i, (pre, c, off) in enumerate(st.bn_table):
        rm, rv = st.bn_stats[off:off + c].cpu(), st.bn_stats[off + c:off + 2 * c].cpu()
        if pre.startswith(IMG):
            np.testing.assert_allclose(rm.numpy(), P[pre + ".running_mean"].float().numpy(), atol=2e-3)
            np.testing.assert_allclose(rv.numpy(), P[pre + ".running_var"].float().numpy(), rtol=2e-2, atol=1e-4)
            rm_err = max(rm_err, (rm.double() - P[pre + ".running_mean"]).abs().max().item())
            rv_err = max(rv_err, ((rv.double() - P[pre + ".running_var"]).abs() / P[pre + ".running_var"]).max().item())
            assert int(st.bn_nbt[i]) == int(nbt0[i]) + 1, pre
        else:
            assert torch.equal(st.bn_stats[off:off + 2 * c], bn0[off:off + 2 * c]) and int(st.bn_nbt[i]) == int(nbt0[i]), pre
    print("image step %s B=%d D=%d masks=%d: loss rel %.2e | mu %.2e logvar %.2e recon %.2e abs | grad worst tensor %.3e (gate %.1e) total %.2e"
          " | running mean abs %.2e var rel %.2e" % (family, B, D, with_masks, l_err, mu_err, lv_err, r_err, worst, tensor_tol, tot, rm_err, rv_err))
    # optimizer: plain Adam on the flat buffers, then one whole step through the packed-gradient Adam over the image range
    eng.optimizer_step()
    eng(img_d, eps=eps_d, **kw)
    torch.cuda.synchronize()
    for n, shape, off in st.table:
        same = torch.equal(st.params[off:off + _numel(shape)], p0[off:off + _numel(shape)])
        assert same == (not n.startswith(IMG)), n
    for i, (pre, c, off) in enumerate(st.bn_table):
        assert int(st.bn_nbt[i]) == int(nbt0[i]) + (2 if pre.startswith(IMG) else 0), pre
    assert int(eng.adam_state[0]) == 2


def test_step_draws_its_own_noise_and_masks():
    """No eps, no masks given: the step draws them (Philox keyed by seed and step counter): the same seed and counter give the same
    step -- up to the order of the fp32 atomics in the BatchNorm statistics and weight gradients, whose bf16 consequences stay inside
    the per-tensor budget of the oracle comparison (6e-2 rel-L2, here on the whole gradient) --, another seed gives another one;
    eval mode ignores eps and masks and leaves the BatchNorm buffers alone."""
    from multimodal_vae_amd.core import FusedImageStep
    dev = _dev()
    B, D = 6, 20
    for family in ("celeba", "coco"):
        st = _state(family, D, dev)
        image = R.formula_inputs(family, B)[0].to(dev).contiguous()
        eng = FusedImageStep(st, B, seed=11)
        bn0, nbt0 = st.bn_stats.clone(), st.bn_nbt.clone()
        a = eng.forward_backward(image, True, True).sums.clone()
        ga = st.grads.clone()
        st.bn_stats.copy_(bn0); st.bn_nbt.copy_(nbt0)
        b = eng.forward_backward(image, True, True).sums.clone()
        assert bool(torch.isfinite(a).all())
        np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), rtol=1e-4)
        assert float((st.grads - ga).double().norm() / ga.double().norm()) <= 6e-2
        eng.seed = 12
        d = eng.forward_backward(image, True, True).sums.clone()
        assert abs(float(d[8]) - float(a[8])) > 1e-4 * abs(float(a[8])) or abs(float(d[0]) - float(a[0])) > 1e-4 * abs(float(a[0]))
        eng.seed = 11
        eng.enc_dropout = False
        c = eng.forward_backward(image, True, True).sums.clone()
        assert not torch.equal(a[0], c[0])
        st.bn_stats.copy_(bn0); st.bn_nbt.copy_(nbt0)
        mu, lv = torch.zeros(B, D, device=dev), torch.zeros(B, D, device=dev)
        e1 = eng.forward_backward(image, False, False, mu=mu, logvar=lv).sums.clone()
        e2 = eng.forward_backward(image, False, False, eps=torch.ones(B, D, device=dev)).sums.clone()
        np.testing.assert_allclose(e2.cpu().numpy(), e1.cpu().numpy(), rtol=1e-5)        # (the BCE slots are fp32 atomics)
        assert torch.equal(st.bn_nbt, nbt0) and torch.equal(st.bn_stats, bn0)


# ====================================================================================================== module face
def _mmvae(family, D):
    import importlib
    M = importlib.import_module("multimodal_vae_amd." + family)
    P = R.formula_params(family, D)
    vae = M.MultimodalVAE(D) if family == "celeba" else M.MultimodalVAE(D, sos=R.formula_sos(), steps=COCO_T)
    vae.load_state_dict({k: v.detach().clone() for k, v in P.items()}, strict=True)
    return M, vae.cuda().eval()


def _image_vae_of(M, mm, D):
    iv = M.ImageVAE(D)
    sd = {k[len("image_"):]: v.detach().clone() for k, v in mm.state_dict().items() if k.startswith("image_")}
    iv.load_state_dict(sd, strict=True)
    return iv.cuda().eval()


@pytest.mark.parametrize("family,kind", [("celeba", "FusedTrainer"), ("coco", "ImageVAETrainer")])
def test_trainer_takes_kl_lambda_per_call(family, kind):
    """``trainer(x, ..., kl_lambda=0.5)`` is the step of a trainer constructed with kl_lambda = 0.5: same seed, same inputs, same step
    counter, so the same drawn noise and masks; the losses agree as two runs of one step do (test_step_draws_its_own_noise_and_masks:
    rtol 1e-4, the order of the fp32 atomics).  ``evaluate`` takes the keyword too."""
    dev = _dev()
    B, D = 8, 20
    image, second = (t.to(dev).contiguous() for t in R.formula_inputs(family, B))
    inputs = (image, second) if kind == "FusedTrainer" else (image,)

    def trainer(**kw):
        M, vae = _mmvae(family, D)
        if kind == "ImageVAETrainer":
            vae = _image_vae_of(M, vae, D)
        return getattr(M, kind)(vae, B, seed=11, **kw)
    per_call, built = trainer(), trainer(kl_lambda=0.5)
    out = per_call(*inputs, kl_lambda=0.5)
    got = out.losses().cpu().numpy()
    assert per_call.engine.kl_lambda == 0.5 and out.kl_scale == 0.5 / B
    want = built(*inputs).losses().cpu().numpy()
    print("%s %s: kl_lambda=0.5 per call %s, at construction %s" % (family, kind, got, want))
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=1e-4)
    assert per_call.evaluate(*inputs, kl_lambda=0.25).kl_scale == 0.25 / B and per_call.engine.kl_lambda == 0.25


@pytest.mark.parametrize("family", ["celeba", "coco"])
def test_module_face_equals_the_mmvaes_image_modules(family):
    D, B = 20, 5
    dev = _dev()
    M, mm = _mmvae(family, D)
    iv = _image_vae_of(M, mm, D)
    assert list(iv.state_dict().keys()) == IR.state_dict_keys(family, D)
    x = R.formula_inputs(family, B)[0].to(dev)
    with torch.no_grad():
        recon, mu, lv = iv(x)
        mu2, lv2 = mm.image_encoder(x)
        recon2 = mm.image_decoder(mu2.contiguous())
    assert torch.equal(mu, mu2) and torch.equal(lv, lv2) and torch.equal(recon, recon2)
    assert recon.shape == (B, 3, IR.SIDE[family], IR.SIDE[family]) and mu.shape == (B, D)
    # the second modality's slots of the flat buffers are at their initial value and in no state_dict
    st = iv._core.state
    for n, shape, off in st.table:
        if not n.startswith(IMG):
            assert float(st.params[off:off + _numel(shape)].abs().max()) == 0.0, n
    # training mode through autograd: reparametrize with a given eps, gradients reach both children
    iv.train()
    recon, mu, lv = iv(x, eps=torch.zeros(B, D, device=dev))
    loss = M.imageonly_loss_function(recon, x, mu, lv) if family == "celeba" else M.loss_function(mu, lv, recon_image=recon, image=x)
    loss.backward()
    assert all(p.grad is not None for p in iv.parameters())


@pytest.mark.parametrize("family", ["celeba", "coco"])
def test_trainer_lowers_the_loss_and_evaluate_matches_oracle(family):
    import importlib
    M = importlib.import_module("multimodal_vae_amd." + family)
    dev = _dev()
    B, D = 32, 20
    rng = np.random.default_rng(2)
    side = IR.SIDE[family]
    base = rng.random((1, 3, side, side), dtype=np.float32)
    shift = (rng.random((B, 3, 1, 1), dtype=np.float32) - 0.5) * 0.6
    img = torch.from_numpy(np.clip(base + shift, 0, 1).astype(np.float32))
    torch.manual_seed(0)
    vae = M.ImageVAE(D).cuda()
    tr = M.ImageVAETrainer(vae, B, lr=1e-3, kl_lambda=1e-3)
    x = img.to(dev)
    first = tr(x).losses()[0].item()
    for _ in range(40):
        last = tr(x).losses()[0].item()
    print("%s ImageVAETrainer: loss %.5f -> %.5f after 40 steps" % (family, first, last))
    assert np.isfinite(last) and last < 0.95 * first, (first, last)
    sd = vae.state_dict()
    assert int(sd["encoder.features.3.num_batches_tracked"].item()) == 41
    assert int(sd["decoder.hallucinate.7.num_batches_tracked"].item()) == 41
    ev = tr.evaluate(x).losses()[0].item()
    Pe = {"image_" + k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in sd.items()}
    with torch.no_grad():
        o_loss, _ = IR.step_loss(family, Pe, img, False, kl_lambda=1e-3)
    print("%s evaluate: %.6f, oracle %.6f (rel %.2e)" % (family, ev, o_loss.item(), abs(ev - o_loss.item()) / o_loss.item()))
    np.testing.assert_allclose(ev, o_loss.item(), rtol=2e-3)
    assert int(vae.state_dict()["encoder.features.3.num_batches_tracked"].item()) == 41          # eval mode: untouched


@pytest.mark.parametrize("family", ["celeba", "coco"])
def test_driver_checkpoint_round_trip(family, tmp_path, capsys):
    import importlib
    from multimodal_vae_amd import evaluate as E, train_imageonly as T
    M = importlib.import_module("multimodal_vae_amd." + family)
    _dev()
    out, res = str(tmp_path / "models"), str(tmp_path / "results")
    argv = ["--dataset", family, "--cuda", "--epochs", "2", "--synthetic", "256", "--batch_size", "64", "--n_latents", "20",
            "--out", out, "--results", res, "--seed", "3"]
    if family == "coco":
        argv.append("--anneal_kl")
    hist = T.main(argv)
    printed = capsys.readouterr().out
    assert len(hist["train"]) == 2 and all(np.isfinite(hist["train"] + hist["test"]))
    assert "Train Epoch: 1 [0/256 (0%)]\tLoss: " in printed and "====> Epoch: 2 Average loss: " in printed and "====> Test set loss: " in printed
    assert ("Using KL Lambda: 1e-05" in printed) == (family == "coco")
    ck_path = os.path.join(out, "checkpoint.pth.tar")
    assert os.path.exists(os.path.join(out, "model_best.pth.tar"))
    ck = torch.load(ck_path, map_location="cpu", weights_only=False)
    assert sorted(ck) == ["best_loss", "n_latents", "optimizer", "state_dict"] and ck["n_latents"] == 20
    assert list(ck["state_dict"]) == IR.state_dict_keys(family, 20) and ck["best_loss"] == min(hist["test"])
    assert float(ck["optimizer"]["state"][0]["step"]) == 2 * (256 // 64)
    side = IR.SIDE[family]
    for e in (1, 2):
        s = torch.load(os.path.join(res, "sample_image_epoch%d.pt" % e))
        assert s.shape == (64, 3, side, side) and bool(((s >= 0) & (s <= 1)).all())
    assert E.is_imageonly_checkpoint(ck_path)
    vae = M.load_checkpoint_imageonly(ck_path, use_cuda=True)
    assert isinstance(vae, M.ImageVAE)
    for k, v in vae.state_dict().items():
        assert torch.equal(v.cpu(), ck["state_dict"][k]), k
    loss = E.main(["test_imageonly", ck_path, "--dataset", family, "--synthetic", "128", "--batch_size", "64", "--seed", "4"])
    assert np.isfinite(loss) and loss > 0
    # log p(x) alone from the checkpoint
    cmd = "loglik_" + family
    table = E.main([cmd, ck_path, "--synthetic", "8", "--batch_size", "8", "--n_samples", "4", "--seed", "1"])
    assert list(table) == ["image"] and np.isfinite(table["image"]["log_px"]) and math.isnan(table["image"]["log_py"])


# ====================================================================================================== estimator
@pytest.mark.parametrize("family", ["celeba", "coco"])
@pytest.mark.parametrize("K,per_call", [(5, None), (40, 16)])
def test_estimator_column_x_equals_the_mmvaes(family, K, per_call):
    """An ImageVAE and a MultimodalVAE with the same image tower, the same mu, logvar and eps: column x of log_p, ess and nll is the
    same number bit for bit (the same decoder body and scoring tail on the same particle rows), y and xy are NaN."""
    from multimodal_vae_amd.evaluate import iw_estimate, log_marginal
    dev = _dev()
    D, B = 20, 3
    M, mm = _mmvae(family, D)
    iv = _image_vae_of(M, mm, D)
    image, second = R.formula_inputs(family, B)
    image = image.to(dev)
    second = second[:, :COCO_T].contiguous().to(dev) if family == "coco" else second.to(dev)
    g = torch.Generator().manual_seed(K)
    mu, lv = 0.3 * torch.randn(B, D, generator=g), -1.0 + 0.2 * torch.randn(B, D, generator=g)
    eps = torch.randn(B, K, D, generator=g)
    kw = dict(eps=eps.to(dev), particles_per_call=per_call, return_log_w=True)
    a = iw_estimate(iv, image, None, mu.to(dev), lv.to(dev), K, **kw)
    b = iw_estimate(mm, image, second, mu.to(dev), lv.to(dev), K, **kw)
    for key in ("log_p", "ess", "nll"):
        assert torch.equal(a[key][:, 0], b[key][:, 0]), key
        assert bool(torch.isfinite(a[key][:, 0]).all())
        assert bool(torch.isnan(a[key][:, 1:]).all()), key
    assert torch.equal(a["log_w"][..., 0], b["log_w"][..., 0]) and bool(torch.isnan(a["log_w"][..., 1:]).all())
    print("%s K=%d: log p(x) %s" % (family, K, a["log_p"][:, 0].tolist()))
    for post in ("joint", "text", "attrs"):
        with pytest.raises(ValueError, match="image posterior alone"):
            log_marginal(iv, [(image, None)], n_particles=2, posterior=post)
    r = log_marginal(iv, [(image, None)], n_particles=K, posterior="image", seed=3)
    assert np.isfinite(r["log_px"]) and math.isnan(r["log_py"]) and math.isnan(r["log_pxy"]) and r["n"] == B
