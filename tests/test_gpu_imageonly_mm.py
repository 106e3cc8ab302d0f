"""GPU tests of MultiMNIST's uni-modal image VAE baseline: the one-pass fused step against the float64 oracle without a product of
experts (tests/imageonly_mm_ref.py), the one-expert waist kernels of csrc/mlp_tail.hip alone (read back through the step's
workspace), the nn.Module / trainer / driver face and the log p(x) estimator.

Gates of the step are the project's own for this tower (tests/test_gpu_latent_sizes.py, tests/test_gpu_imageonly.py): loss rel 1e-3 |
mu / logvar abs 1e-2 | recon abs 2e-2 | per-tensor gradient rel-L2 4e-2 | total gradient norm 2e-3 | running mean abs 2e-3, running
variance rel 2e-2.  No gate is widened.  Every test prints what it measured (run with -s).
"""
import math
import os

import numpy as np
import pytest
import torch

from oracle import mmvae_ref as R
from gradcheck import check_gradients
import imageonly_mm_ref as IM

pytestmark = pytest.mark.gpu

IMG = ("image_encoder.", "image_decoder.")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _state(D, dev):
    """The MMVAE's plan state with the formula parameters of EVERY tensor, the text half's included."""
    from multimodal_vae_amd import core
    st = core.MultimnistState(D, dev)
    P = R.formula_params("multimnist", D)
    assert [t[0] for t in st.table] == [n for n, _ in R.param_table("multimnist", D)]
    for n, shape, off in st.table:
        st.params[off:off + P[n].numel()] = P[n].detach().reshape(-1).to(dev)
    return st


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _knob(value):
    """mm_image_waist for the length of a block: 1 / 0, and back to the default (the size's own)"""
    from multimodal_vae_amd._lib import knobs
    return knobs(mm_image_waist=value)


def _ws(eng, name, shape, dtype):
    """a named buffer of the step's one-pass workspace"""
    from multimodal_vae_amd._lib import call
    off = call("mmvae_mm_debug_offset", eng.h, ("image_step:" + name).encode())
    assert off >= 0, name
    nbytes = _numel(shape) * torch.empty((), dtype=dtype).element_size()
    return eng.ws[off:off + nbytes].view(dtype).view(shape).clone()


def _masks(B, D, dev):
    g = torch.Generator().manual_seed(7 * B + D)
    ms = [(torch.rand(B, w, generator=g) >= 0.1).to(torch.uint8) for w in IM.MASK_WIDTHS]
    return ms, {"enc_mask%d" % (i + 1): m.to(dev).contiguous() for i, m in enumerate(ms)}


# ====================================================================================================== the step
SHAPES = [(5, 20), (16, 20), (23, 20), (33, 20), (23, 100), (16, 1), (23, 127), (5, 32)]
CASES = [(B, D, m, -1) for B, D in SHAPES for m in (False, True)] + [(23, D, m, k) for D in (20, 100) for m in (False, True) for k in (1, 0)]


@pytest.mark.parametrize("B,D,with_masks,knob", CASES)
def test_step_matches_oracle(B, D, with_masks, knob):
    """One training step of FusedImageStep on a MultimnistState (given eps, given or no dropout masks; the waist at its default, forced
    on and forced off) against the float64 oracle without a product of experts.  (5,20) one partial 16-row block, (16,20) one exact
    block, (23,20) a second partial one, (33,20) three blocks; (16,1), (23,127), (5,32): the sizes without a waist, with lde / ldz
    padding.  Every text gradient is exactly 0 and the text parameters keep their bits through two optimizer steps;
    num_batches_tracked grows by 1 per step in the image BatchNorms only; loss slots other than 0 and 8 are 0.
    Measured on MI355X over all 24 cases (gates in brackets): loss rel <= 4.9e-5 (1e-3); mu abs <= 1.2e-3, logvar abs <= 1.4e-3 (1e-2);
    recon abs <= 1.5e-2 (2e-2); worst gradient tensor 1.37e-2 .. 1.99e-2 (4e-2); total gradient norm <= 2.7e-4 (2e-3); running mean
    abs <= 1.5e-4 (2e-3), running variance rel <= 1.2e-4 (2e-2).  Waist on / off at (23,20): worst tensor 1.62e-2 / 1.61e-2 with
    masks, 1.62e-2 / 1.54e-2 without; at (23,100): 1.39e-2 / 1.37e-2 and 1.46e-2 / 1.37e-2.  No gate is widened."""
    from multimodal_vae_amd.core import FusedImageStep
    dev = _dev()
    st = _state(D, dev)
    P = IM.params64(D, requires_grad=True)
    image = R.formula_inputs("multimnist", B)[0]
    eps = R.formula_eps(B, D, 1)
    masks, kw = None, {}
    if with_masks:
        ms, kw = _masks(B, D, dev)
        masks = tuple(m.float() for m in ms)
    eng = FusedImageStep(st, B, kl_lambda=1e-3)
    eng.enc_dropout = with_masks
    assert eng.ws.numel() == st.module_workspace_bytes(B) < st.workspace_bytes(B)
    mu, lv = torch.zeros(B, D, device=dev), torch.zeros(B, D, device=dev)
    recon = torch.zeros(B, 1, 50, 50, device=dev)
    p0, nbt0, bn0 = st.params.clone(), st.bn_nbt.clone(), st.bn_stats.clone()
    img_d, eps_d = image.to(dev).contiguous(), eps.to(dev).contiguous()
    with _knob(knob):
        out = eng.forward_backward(img_d, True, True, eps=eps_d, mu=mu, logvar=lv, recon_image=recon, **kw)
        o_loss, (o_recon, o_mu, o_lv) = IM.step_loss(P, image, True, eps, masks, 0.1 if with_masks else 0.0, 1e-3)
        o_loss.backward()
        losses = out.losses().cpu()
        sums = eng.sums.cpu()
        l_err = abs(losses[0].item() - o_loss.item()) / abs(o_loss.item())
        mu_err, lv_err = (mu.cpu().double() - o_mu.detach()).abs().max().item(), (lv.cpu().double() - o_lv.detach()).abs().max().item()
        r_err = (recon.cpu().double() - o_recon.detach()).abs().max().item()
        g = st.grads.cpu()
        pairs, second = [], []
        for n, shape, off in st.table:
            (pairs if n.startswith(IMG) else second).append((n, g[off:off + _numel(shape)], P[n].grad))
        rm_err = rv_err = 0.0
        for i, (pre, c, off) in enumerate(st.bn_table):
            if pre.startswith(IMG):
                rm, rv = st.bn_stats[off:off + c].cpu(), st.bn_stats[off + c:off + 2 * c].cpu()
                rm_err = max(rm_err, (rm.double() - P[pre + ".running_mean"]).abs().max().item())
                rv_err = max(rv_err, ((rv.double() - P[pre + ".running_var"]).abs() / P[pre + ".running_var"]).max().item())
        head = "mm image step B=%d D=%d masks=%d knob=%d" % (B, D, with_masks, knob)
        print("%s: loss rel %.2e (1e-3) | mu %.2e logvar %.2e (1e-2) recon %.2e (2e-2) abs | running mean abs %.2e (2e-3) var rel %.2e (2e-2)"
              % (head, l_err, mu_err, lv_err, r_err, rm_err, rv_err))
        assert l_err <= 1e-3, l_err
        assert losses[1].item() == 0.0 and losses[2].item() == 0.0
        assert all(float(sums[i]) == 0.0 for i in range(16) if i not in (0, 8)), sums
        assert mu_err <= 1e-2 and lv_err <= 1e-2, (mu_err, lv_err)
        assert r_err <= 2e-2, r_err
        assert len(second) > 0
        for n, gh, gr in second:
            assert gr is None and float(gh.abs().max()) == 0.0, n
        worst, tot = check_gradients(pairs, 4e-2, 2e-3, head)
        print("%s: grad worst tensor %.3e (4e-2) total %.2e (2e-3)" % (head, worst, tot))
        assert rm_err <= 2e-3 and rv_err <= 2e-2, (rm_err, rv_err)
        for i, (pre, c, off) in enumerate(st.bn_table):
            assert pre.startswith(IMG)                             # (this family's BatchNorms are all in the image half)
            assert int(st.bn_nbt[i]) == int(nbt0[i]) + 1, pre
        # optimizer: plain Adam on the flat buffers, then one whole step through the packed-gradient Adam over the image range
        eng.optimizer_step()
        eng(img_d, eps=eps_d, **kw)
        torch.cuda.synchronize()
    for n, shape, off in st.table:
        same = torch.equal(st.params[off:off + _numel(shape)], p0[off:off + _numel(shape)])
        assert same == (not n.startswith(IMG)), n
    for i, (pre, c, off) in enumerate(st.bn_table):
        assert int(st.bn_nbt[i]) == int(nbt0[i]) + 2, pre
    assert int(eng.adam_state[0]) == 2


def test_step_draws_its_own_noise_and_masks():
    """No eps, no masks given: the step draws them (Philox keyed by seed and step counter): the same seed and counter give the same
    step -- up to the order of the fp32 atomics in the BatchNorm statistics and weight gradients, whose bf16 consequences stay inside
    the per-tensor budget of the oracle comparison (4e-2 rel-L2, here on the whole gradient) --, another seed gives another one;
    eval mode ignores eps and masks and leaves the BatchNorm buffers alone.  With the waist (D = 20) and without (D = 32)."""
    from multimodal_vae_amd.core import FusedImageStep
    dev = _dev()
    B = 6
    for D in (20, 32):
        st = _state(D, dev)
        image = R.formula_inputs("multimnist", B)[0].to(dev).contiguous()
        eng = FusedImageStep(st, B, seed=11)
        bn0, nbt0 = st.bn_stats.clone(), st.bn_nbt.clone()
        a = eng.forward_backward(image, True, True).sums.clone()
        ga = st.grads.clone()
        st.bn_stats.copy_(bn0); st.bn_nbt.copy_(nbt0)
        b = eng.forward_backward(image, True, True).sums.clone()
        assert bool(torch.isfinite(a).all())
        np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), rtol=1e-4)
        assert float((st.grads - ga).double().norm() / ga.double().norm()) <= 4e-2
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
        assert all(float(e1[i]) == 0.0 for i in range(16) if i not in (0, 8)) and float(e1[8]) > 0


# ====================================================================================================== the waist alone
def _waist_step(B, D):
    """One training step that draws its own eps and masks: what it leaves in the one-pass workspace are the operands of the replays
    below (mmvae_mm_bench_layer "image_step:..."), which run the middle of the step again, with the waist or with the unfused chain,
    on the SAME bits.  (Two steps do not hand the middle the same bits: the conv towers' BatchNorm sums are fp32 atomics.)"""
    from multimodal_vae_amd.core import FusedImageStep
    dev = _dev()
    st = _state(D, dev)
    image = R.formula_inputs("multimnist", B)[0].to(dev).contiguous()
    eng = FusedImageStep(st, B, kl_lambda=1e-3, seed=5)
    eng.forward_backward(image, True, True)
    torch.cuda.synchronize()
    return st, eng


def _replay(st, eng, B, D, mode):
    """mode "waist" | "chain": forward then backward replay -> every tensor around the middle, and the float64 operands"""
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd._ops import stream
    ldz, lde = (D + 1 + 7) // 8 * 8, (2 * D + 7) // 8 * 8
    bf, f32, u8 = torch.bfloat16, torch.float32, torch.uint8
    off = call("mmvae_mm_debug_offset", eng.h, b"image_step:sums")
    eng.ws[off:off + 32 * 16 * 4].zero_()                         # the loss slots: the KL of this replay alone ends up in loss_out[8]
    for name, shape, dt in (("y2", (B, 200), bf), ("ay2", (B, 200), bf), ("encout", (B, 2 * D), f32), ("mu", (B, D), f32), ("logvar", (B, D), f32),
                            ("z_f32", (B, D), f32), ("z_bf", (B, ldz), bf), ("d_encout", (B, lde), bf), ("dy2", (B, 200), bf), ("dy1", (B, 400), bf)):
        o = call("mmvae_mm_debug_offset", eng.h, ("image_step:" + name).encode())
        eng.ws[o:o + _numel(shape) * torch.empty((), dtype=dt).element_size()].fill_(0x7f)      # (what a kernel leaves out shows)
    st.grads.zero_()
    call("mmvae_mm_bench_layer", eng.h, ptr(eng.ws), eng.ws.numel(), ("image_step:%s_fwd" % mode).encode(), 1, stream())
    call("mmvae_mm_bench_layer", eng.h, ptr(eng.ws), eng.ws.numel(), ("image_step:%s_bwd" % mode).encode(), 1, stream())
    torch.cuda.synchronize()
    t = dict(y1=_ws(eng, "y1", (B, 400), bf), ay1=_ws(eng, "ay1", (B, 400), bf), y2=_ws(eng, "y2", (B, 200), bf), ay2=_ws(eng, "ay2", (B, 200), bf),
             encout=_ws(eng, "encout", (B, 2 * D), f32), mu=_ws(eng, "mu", (B, D), f32), logvar=_ws(eng, "logvar", (B, D), f32),
             z=_ws(eng, "z_f32", (B, D), f32), z_bf_full=_ws(eng, "z_bf", (B, ldz), bf), dz=_ws(eng, "dz_img", (B, D), f32),
             d_enc_out_full=_ws(eng, "d_encout", (B, lde), bf), dy2=_ws(eng, "dy2", (B, 200), bf), dy1=_ws(eng, "dy1", (B, 400), bf),
             eps=_ws(eng, "eps", (B, D), f32), m1=_ws(eng, "m1", (B, 400), u8), m2=_ws(eng, "m2", (B, 200), u8))
    o = call("mmvae_mm_debug_offset", eng.h, b"image_step:tmp_f32")
    t["kl"] = eng.ws[o + (B * 2500 - 16) * 4:o + B * 2500 * 4].view(f32).clone()[8]
    t["z_bf"], t["d_enc_out"] = t["z_bf_full"][:, :D], t["d_enc_out_full"][:, :2 * D]
    for name, key in (("image_encoder.classifier.6.bias", "d_bias"), ("image_encoder.classifier.3.bias", "db2"), ("image_encoder.classifier.0.bias", "db1"),
                      ("image_encoder.classifier.3.weight", "w2"), ("image_encoder.classifier.6.weight", "w3"),
                      ("image_encoder.classifier.3.bias", "b2"), ("image_encoder.classifier.6.bias", "b3")):
        for n, shape, off_ in st.table:
            if n == name:
                t[key] = (st.grads if key[0] == "d" else st.params)[off_:off_ + _numel(shape)].view(shape).clone()
    assert set(t["m1"].unique().tolist()) <= {0, 1} and 0.5 < float(t["m2"].float().mean()) < 1.0
    c = dict(y1=t["y1"].double().cpu(), ay1=t["ay1"].double().cpu(), m1=t["m1"].double().cpu(), m2=t["m2"].double().cpu(), w2=IM.bf(t["w2"].cpu()),
             w3=IM.bf(t["w3"].cpu()), b2=t["b2"].double().cpu(), b3=t["b3"].double().cpu(), eps=t["eps"].double().cpu(), dz=t["dz"].double().cpu(),
             kl_coef=float(np.float32(1e-3) / np.float32(B)), training=True, drop=True)
    return t, c


@pytest.mark.parametrize("B", [5, 23, 33])
def test_waist_equals_the_unfused_chain_at_d100(B):
    """n_latents = 100, the waist against the unfused chain (what mm_image_waist 1 / 0 select) on the same operands: the waist runs the
    stream_gemm instantiations of mlp2_fwd / mlp2_bwd and latent1's expressions, so y2, ay2, mu, logvar, z_f32, z_bf, d_encout, dy2
    and dy1 are the same bits (recon, behind z_bf, with them).  KL sum and classifier.6's bias gradient under test_latent1_alone's
    gates (KL: relative 1e-4 and at most 4x mmvae_kl_fwd's own error; bias: 2 B 2^-24 of sum|terms|); whether they come out bit-equal
    is printed.
    Measured on MI355X: every listed tensor bit-equal; KL sum and bias gradient ALSO bit-equal at B = 5, 23, 33.  KL relative error
    waist = chain 1.3e-6 / 6.6e-7 / 8.3e-8 (mmvae_kl_fwd 1.3e-6 / 5.2e-7 / 1.8e-7); bias error / sum|terms| 5.3e-8 / 3.5e-8 / 3.5e-8
    (gates 6.0e-7 / 2.7e-6 / 3.9e-6)."""
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd._ops import stream
    D = 100
    st, eng = _waist_step(B, D)
    a, c = _replay(st, eng, B, D, "waist")
    b, _ = _replay(st, eng, B, D, "chain")
    for k in ("ay1", "dz", "eps", "m2"):
        assert torch.equal(a[k], b[k]), k                           # the same operands
    for k in ("y2", "ay2", "mu", "logvar", "encout", "z", "z_bf_full", "d_enc_out_full", "dy2", "dy1"):
        assert torch.equal(a[k], b[k]), k
    mu64, lv64 = a["mu"].double().cpu(), a["logvar"].double().cpu()
    kl64 = float(R.kl_sum(mu64, lv64))
    kl_old = torch.zeros(1, dtype=torch.float32, device=a["mu"].device)
    call("mmvae_kl_fwd", ptr(a["mu"].contiguous()), ptr(a["logvar"].contiguous()), B * D, ptr(kl_old), stream())
    e_w, e_u, e_old = (abs(float(x) - kl64) / abs(kl64) for x in (a["kl"], b["kl"], kl_old))
    g64 = IM.IR.latent1_bwd(mu64, lv64, c["eps"], c["dz"], c["kl_coef"], True)
    sabs = g64.abs().sum(0)
    be_w, be_u = (((x["d_bias"].double().cpu() - g64.sum(0)).abs() / sabs).max().item() for x in (a, b))
    print("waist D=100 B=%d: KL rel err waist %.3e chain %.3e mmvae_kl_fwd %.3e, bit-equal %s | bias err / sum|terms| waist %.3e chain %.3e "
          "(gate %.3e), bit-equal %s" % (B, e_w, e_u, e_old, bool(torch.equal(a["kl"], b["kl"])), be_w, be_u, 2 * B * 2.0 ** -24,
                                       bool(torch.equal(a["d_bias"], b["d_bias"]))))
    assert e_w < 1e-4 and e_w <= 4 * max(e_old, 2.0 ** -24), (e_w, e_old)
    assert be_w <= 2 * B * 2.0 ** -24, be_w


@pytest.mark.parametrize("B,D", [(5, 20), (16, 20), (23, 20), (33, 20), (23, 100)])
def test_waist_against_float64(B, D):
    """The waist pair against the float64 waist evaluated from the bf16 operands the kernels read, under the yardsticks derived in
    tests/imageonly_mm_ref.py (worst error / yardstick per quantity printed).  Pad columns of z_bf and d_encout exactly 0, column D of
    z_bf exactly 1; two calls give equal bits (the bias gradients of classifier.3 / .0 excepted: mlp2_bwd's fp32 atomics across
    workgroups).  Eval mode gives z == mu, in a step of its own.
    Measured on MI355X, worst error / yardstick over the five shapes: y2 <= 0.93, ay2 <= 0.90, enc_out (mu, logvar) <= 0.17, z <= 0.13,
    z_bf <= 0.68, KL <= 0.001, d_enc_out <= 0.99, d_bias <= 0.08, dy2 <= 0.99, dy1 <= 0.97, db2 <= 0.009, db1 <= 0.001 (a bf16-stored
    quantity sits at one bf16 rounding of an exact operand, so a ratio just below 1 is what a correct kernel gives)."""
    from multimodal_vae_amd.core import FusedImageStep
    st, eng = _waist_step(B, D)
    t, c = _replay(st, eng, B, D, "waist")
    fails, ratios = IM.check_waist(c, {k: v.cpu() for k, v in t.items()})
    print("waist B=%d D=%d, worst error / yardstick: %s" % (B, D, " ".join("%s %.3f" % kv for kv in ratios.items())))
    assert not fails, fails
    t2, _ = _replay(st, eng, B, D, "waist")
    for k in ("y2", "ay2", "encout", "mu", "logvar", "z", "z_bf_full", "kl", "d_enc_out_full", "d_bias", "dy2", "dy1"):
        assert torch.equal(t[k], t2[k]), k                          # fixed fold orders, no float atomics
    # eval mode, no backward: z == mu, the pads as in training, the KL folded behind the decoder
    with _knob(1):
        out = eng.forward_backward(R.formula_inputs("multimnist", B)[0].to(t["mu"].device).contiguous(), False, False)
    torch.cuda.synchronize()
    ldz = (D + 1 + 7) // 8 * 8
    mu_e, z_e, zb_e = _ws(eng, "mu", (B, D), torch.float32), _ws(eng, "z_f32", (B, D), torch.float32), _ws(eng, "z_bf", (B, ldz), torch.bfloat16)
    assert torch.equal(z_e, mu_e) and torch.equal(zb_e[:, :D], mu_e.to(torch.bfloat16))
    assert bool((zb_e[:, D] == 1).all()) and (ldz == D + 1 or float(zb_e[:, D + 1:].float().abs().max()) == 0.0)
    kl64 = float(R.kl_sum(mu_e.double().cpu(), _ws(eng, "logvar", (B, D), torch.float32).double().cpu()))
    assert abs(float(eng.sums[8]) - kl64) <= 1e-4 * abs(kl64)


# ====================================================================================================== module face
def _mmvae(D):
    from multimodal_vae_amd import multimnist as M
    P = R.formula_params("multimnist", D)
    vae = M.MultimodalVAE(D)
    vae.load_state_dict({k: v.detach().clone() for k, v in P.items()}, strict=True)
    return M, vae.cuda().eval()


def _image_vae_of(M, mm, D):
    iv = M.ImageVAE(D)
    sd = {k[len("image_"):]: v.detach().clone() for k, v in mm.state_dict().items() if k.startswith("image_")}
    iv.load_state_dict(sd, strict=True)
    return iv.cuda().eval()


def test_module_face_equals_the_mmvaes_image_modules():
    D, B = 20, 5
    dev = _dev()
    M, mm = _mmvae(D)
    iv = _image_vae_of(M, mm, D)
    assert list(iv.state_dict().keys()) == IM.state_dict_keys(D)
    x = R.formula_inputs("multimnist", B)[0].to(dev)
    with torch.no_grad():
        recon, mu, lv = iv(x)
        mu2, lv2 = mm.image_encoder(x)
        recon2 = mm.image_decoder(mu2.contiguous())
    assert torch.equal(mu, mu2) and torch.equal(lv, lv2) and torch.equal(recon, recon2)
    assert recon.shape == (B, 1, 50, 50) and mu.shape == (B, D)
    # the text half's slots of the flat buffers are at their initial value and in no state_dict
    st = iv._core.state
    for n, shape, off in st.table:
        if not n.startswith(IMG):
            assert float(st.params[off:off + _numel(shape)].abs().max()) == 0.0, n
    # training mode through autograd: reparametrize with a given eps, given masks, gradients reach both children
    iv.train()
    ms, _ = _masks(B, D, dev)
    recon, mu, lv = iv(x, eps=torch.zeros(B, D, device=dev), enc_masks=tuple(m.to(dev) for m in ms))
    M.imageonly_loss_function(recon, x, mu, lv).backward()
    assert all(p.grad is not None for p in iv.parameters())


# ====================================================================================================== estimator
@pytest.mark.parametrize("K,per_call", [(5, None), (40, 16)])
def test_estimator_column_x_equals_the_mmvaes(K, per_call):
    """An ImageVAE and a MultimodalVAE with the same image tower, the same mu, logvar and eps: column x of log_p, ess and nll is the
    same number bit for bit (mmvae_mm_iw_score_image is the image half of mmvae_mm_iw_score on the same particle rows), y and xy are NaN."""
    from multimodal_vae_amd.evaluate import iw_estimate, log_marginal
    dev = _dev()
    D, B = 20, 3
    M, mm = _mmvae(D)
    iv = _image_vae_of(M, mm, D)
    image, text = R.formula_inputs("multimnist", B)
    image, text = image.to(dev), text.to(dev)
    g = torch.Generator().manual_seed(K)
    mu, lv = 0.3 * torch.randn(B, D, generator=g), -1.0 + 0.2 * torch.randn(B, D, generator=g)
    eps = torch.randn(B, K, D, generator=g)
    kw = dict(eps=eps.to(dev), particles_per_call=per_call, return_log_w=True)
    a = iw_estimate(iv, image, None, mu.to(dev), lv.to(dev), K, **kw)
    b = iw_estimate(mm, image, text, mu.to(dev), lv.to(dev), K, **kw)
    for key in ("log_p", "ess", "nll"):
        assert torch.equal(a[key][:, 0], b[key][:, 0]), key
        assert bool(torch.isfinite(a[key][:, 0]).all())
        assert bool(torch.isnan(a[key][:, 1:]).all()), key
    assert torch.equal(a["log_w"][..., 0], b["log_w"][..., 0]) and bool(torch.isnan(a["log_w"][..., 1:]).all())
    print("multimnist K=%d: log p(x) %s" % (K, a["log_p"][:, 0].tolist()))
    for post in ("joint", "text"):
        with pytest.raises(ValueError, match="image posterior alone"):
            log_marginal(iv, [(image, None)], n_particles=2, posterior=post)
    r = log_marginal(iv, [(image, None)], n_particles=K, posterior="image", seed=3)
    assert np.isfinite(r["log_px"]) and math.isnan(r["log_py"]) and math.isnan(r["log_pxy"]) and r["n"] == B


# ====================================================================================================== trainer, evaluation, driver
def test_trainer_lowers_the_loss_and_evaluate_matches_oracle():
    from multimodal_vae_amd import evaluate as E, multimnist as M
    dev = _dev()
    B, D = 16, 20
    img = R.formula_inputs("multimnist", B, seed=2)[0]
    torch.manual_seed(0)
    vae = M.ImageVAE(D).cuda()
    tr = M.ImageVAETrainer(vae, B, lr=1e-3, kl_lambda=1e-3)
    x = img.to(dev)
    first = tr(x).losses()[0].item()
    for _ in range(20):
        last = tr(x).losses()[0].item()
    print("multimnist ImageVAETrainer: loss %.5f -> %.5f after 20 steps" % (first, last))
    assert np.isfinite(last) and last < 0.95 * first, (first, last)
    sd = vae.state_dict()
    assert int(sd["encoder.features.3.num_batches_tracked"].item()) == 21
    assert int(sd["decoder.hallucinate.7.num_batches_tracked"].item()) == 21
    ev = E.test_imageonly(vae, [(x, None)], kl_lambda=1.0, verbose=False)
    Pe = {"image_" + k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in sd.items()}
    with torch.no_grad():
        o_loss, _ = IM.step_loss(Pe, img, False, kl_lambda=1.0)
    print("multimnist test_imageonly: %.6f, oracle %.6f (rel %.2e)" % (ev, o_loss.item(), abs(ev - o_loss.item()) / o_loss.item()))
    np.testing.assert_allclose(ev, o_loss.item(), rtol=2e-3)
    assert int(vae.state_dict()["encoder.features.3.num_batches_tracked"].item()) == 21          # eval mode: untouched


def test_driver_checkpoint_round_trip(tmp_path, capsys):
    from multimodal_vae_amd import evaluate as E, multimnist as M, train_imageonly as T
    _dev()
    out, res = str(tmp_path / "models"), str(tmp_path / "results")
    hist = T.main(["--dataset", "multimnist", "--cuda", "--epochs", "1", "--synthetic", "64", "--batch_size", "16", "--out", out, "--results", res,
                   "--seed", "3", "--anneal_kl"])
    printed = capsys.readouterr().out
    assert len(hist["train"]) == 1 and all(np.isfinite(hist["train"] + hist["test"])) and hist["kl_lambda"] == [1e-5]
    assert "Train Epoch: 1 [0/64 (0%)]\tLoss: " in printed and "====> Epoch: 1 Average loss: " in printed and "====> Test set loss: " in printed
    assert "Using KL Lambda: 1e-05" in printed
    ck_path = os.path.join(out, "checkpoint.pth.tar")
    assert os.path.exists(os.path.join(out, "model_best.pth.tar"))
    ck = torch.load(ck_path, map_location="cpu", weights_only=False)
    assert sorted(ck) == ["best_loss", "n_latents", "optimizer", "state_dict"] and ck["n_latents"] == 20
    assert list(ck["state_dict"]) == IM.state_dict_keys(20) and ck["best_loss"] == min(hist["test"])
    assert float(ck["optimizer"]["state"][0]["step"]) == 64 // 16 and len(ck["optimizer"]["state"]) == 28
    s = torch.load(os.path.join(res, "sample_image_epoch1.pt"))
    assert s.shape == (64, 1, 50, 50) and bool(((s >= 0) & (s <= 1)).all())
    assert E.is_imageonly_checkpoint(ck_path) and not E.is_textonly_checkpoint(ck_path)
    vae = M.load_checkpoint_imageonly(ck_path, use_cuda=True)
    assert isinstance(vae, M.ImageVAE)
    for k, v in vae.state_dict().items():
        assert torch.equal(v.cpu(), ck["state_dict"][k]), k
    loss = E.main(["test_imageonly", ck_path, "--dataset", "multimnist", "--synthetic", "32", "--batch_size", "16", "--seed", "4"])
    assert np.isfinite(loss) and loss > 0
    # log p(x) alone from the checkpoint, and samples from the prior
    table = E.main(["loglik", ck_path, "--synthetic", "8", "--batch_size", "8", "--n_samples", "4", "--seed", "1"])
    assert list(table) == ["image"] and np.isfinite(table["image"]["log_px"]) and math.isnan(table["image"]["log_py"])
    sdir = str(tmp_path / "samples")
    E.main(["sample", ck_path, "--n_samples", "4", "--out", sdir])
    s = torch.load(os.path.join(sdir, "sample_image.pt"))
    assert s.shape == (4, 1, 50, 50) and bool(((s >= 0) & (s <= 1)).all()) and not os.path.exists(os.path.join(sdir, "sample_text.txt"))
    torch.save((R.formula_inputs("multimnist", 1)[0][0, 0] * 255).to(torch.uint8), str(tmp_path / "x.pt"))
    E.main(["sample", ck_path, "--n_samples", "3", "--out", sdir, "--condition_on_image", str(tmp_path / "x.pt")])
    assert torch.load(os.path.join(sdir, "sample_image.pt")).shape == (3, 1, 50, 50)
