"""GPU tests of the fused COCO InfoVAE step (mmvae_coco_infovae_step, core.FusedInfoVAEStep, coco.FusedInfoVAE / InfoVAETrainer,
train_infovae --fused) and of the y-only form of the MMD sweep it runs (mmvae_mmd_dy), against the float64 instrument
tests/infovae_step_ref.py (whose faults tests/test_cpu_infovae_step.py shows these gates to catch).

Gates of the step: those of tests/test_gpu_imageonly.py::test_step_matches_oracle for COCO, unchanged -- the backward chain is the
same: loss rel 1e-3 | mu / logvar abs 1e-2 | recon abs 2e-2 | per-tensor gradient 4.5e-2, total 2e-3 (gradcheck.check_gradients) |
running mean abs 2e-3, running variance rel 2e-2.  The four MMD values: mmd_ref.GATE_FACTOR x the error of the fp32 formulation on the
CPU for the step's own (true_samples, z), as tests/test_gpu_mmd.py gates them.  Every test prints what it measured (run with -s).
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import mmvae_ref as R  # noqa: E402
from gradcheck import check_gradients  # noqa: E402
import imageonly_ref as IR  # noqa: E402
import infovae_step_ref as IV  # noqa: E402
import mmd_ref as MR  # noqa: E402

pytestmark = pytest.mark.gpu

IMG = ("image_encoder.", "image_decoder.")
ENC, DEC = "image_encoder.", "image_decoder."
COCO_T = 4          # caption length of the COCO plans built here: no caption runs in this step
STEP_LAMBDAS = dict(lambda_x=1.0, lambda_mmd=2.0, kl_lambda=1e-3)       # (tests/test_cpu_infovae_step.py: lambda_mmd != 1 on purpose)
MMD_SLOTS = slice(12, 16)
# z against mu + eps * exp(logvar / 2) in float64, in fp32 ulps of L = the larger of |mu| and |eps exp(logvar / 2)|.  The issue asks for
# 1 ulp; no fp32 evaluation on this hardware can promise that, and the bound asserted instead is the one the number format and the
# exp give: the kernel forms z = fma(eps, E', mu) with E' = exp(logvar / 2) (1 + d).  An exp that is good to k ulp has |d| <= k 2^-23, and
# since ulp(x) > 2^-24 |x| the term's error |eps E d| is below 2 k ulp(L); the one rounding of the fma is 0.5 ulp(z) <= 1 ulp(L) (|z| <= 2 L).
# So |z - exact| <= (2 k + 1) ulp(L).  k: the hardware exp2 is specified to 1 ulp, the reduced argument of the kernels' exp is rounded
# once more (at most 2^-25 absolute, times ln 2: 0.17 ulp), k <= 1.5 with room -> 4 ulp.  (A correctly rounded exp, k = 0.5, gives 2.)
Z64_GATE_ULPS = 4.0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _state(D, dev):
    """A COCO plan state with the formula parameters of EVERY tensor, the caption half included."""
    from multimodal_vae_amd import core
    st = core.CocoState(D, dev, COCO_T)
    P = R.formula_params("coco", D)
    assert [t[0] for t in st.table] == [n for n, _ in R.param_table("coco", D)]
    for n, shape, off in st.table:
        st.params[off:off + P[n].numel()] = P[n].detach().reshape(-1).to(dev)
    return st


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _ws_floats(eng, name, B, D):
    """the [B][D] fp32 buffer `infovae_step:<name>` of the engine's workspace"""
    from multimodal_vae_amd._lib import call
    off = call("mmvae_coco_debug_offset", eng.h, ("infovae_step:" + name).encode())
    assert off > 0 and off % 16 == 0
    return eng.ws[off:off + 4 * B * D].view(torch.float32).view(B, D)


def _check_mmd_slots(sums, true_samples, z, label):
    """the four values against mmd64 on the step's own z, gated as tests/test_gpu_mmd.py gates them; -> (error, yardstick)"""
    ts, z = true_samples.detach().float().cpu(), z.detach().float().cpu()
    ref = MR.mmd64(ts, z)
    yard = MR.value_error(MR.formulation(ts, z)[0], ref["terms"])
    err = MR.value_error(sums[MMD_SLOTS].cpu(), ref["terms"])
    print("%s: MMD slots %s, error %.3e, yardstick %.3e (gate %.0f x)" % (label, [float(v) for v in sums[MMD_SLOTS]], err, yard, MR.GATE_FACTOR))
    assert err <= MR.GATE_FACTOR * yard, (err, yard)
    return err, yard


def _ulp(x):
    """spacing of fp32 at |x| (x float64 tensor)"""
    return torch.pow(2.0, torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 23)


# ====================================================================================================== the step against the oracle
@pytest.mark.parametrize("B,D,with_masks", [(4, 100, False), (6, 20, True), (4, 124, False), (5, 4, True), (65, 100, False)])
def test_step_matches_oracle(B, D, with_masks):
    """One training step (given eps, true_samples, given or no dropout masks) at lambda_x = 1, lambda_mmd = 2, kl_lambda = 1e-3 against the
    float64 instrument.  Measured on MI355X (gates in brackets): loss rel <= 3.2e-5 (1e-3); mu / logvar abs <= 1.7e-3 (1e-2); recon abs
    <= 8.8e-3 (2e-2); worst gradient tensor 1.2e-2 .. 2.0e-2 (4.5e-2), total <= 5.4e-4 (2e-3); running mean abs <= 2.1e-4 (2e-3), variance
    rel <= 1.7e-4 (2e-2); MMD values 1.7e-9 .. 1.8e-8 against gates of 5.8e-8 .. 3.2e-7.  B = 65 crosses the sweep's 64-row tile and its 32-row column tile; D = 124 and D = 4 are the ends of the plan's
    range (M = 8 and M = 1 of the sweep).  z = mu + eps * exp(logvar / 2) of the returned mu / logvar within 1 ulp of that formula in
    fp32 as the library's reparametrize evaluates it (mmvae_reparam_fwd: measured 0 ulp, the bits are equal, as
    tests/test_gpu_imageonly.py::test_latent1_alone finds for the latent block alone).  Against the formula in float64 the same z is up to
    1.85 ulp of the larger operand off (B = 65, D = 100; 1.07 .. 1.74 at the other shapes): the hardware exp2 of the kernels' exp is good to about 1 ulp and eps multiplies
    it, so no fp32 evaluation without a correctly rounded exp is within 1 ulp of float64.  That independent comparison is gated at 4 ulp,
    the bound that the fp32 format and an exp good to 1.5 ulp give (Z64_GATE_ULPS above, with its derivation): a deviation from the 1 ulp
    the task sets, for that reason.
    The caption half: gradients exactly 0, parameters,
    BatchNorm buffers and counters keep their bits through two optimizer steps."""
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd._ops import stream
    from multimodal_vae_amd.core import FusedInfoVAEStep
    dev = _dev()
    st = _state(D, dev)
    P = IV.params(D, requires_grad=True)
    image, eps, ts = IV.inputs(B, D)
    masks, kw = None, {}
    if with_masks:
        masks = IV.masks_of(B, D)
        kw = {"enc_mask%d" % (i + 1): m.to(dev).contiguous() for i, m in enumerate(masks)}
    eng = FusedInfoVAEStep(st, B, **STEP_LAMBDAS)
    eng.enc_dropout = with_masks
    assert eng.ws.numel() > st.module_workspace_bytes(B)
    f32 = dict(dtype=torch.float32, device=dev)
    mu, lv, z = torch.zeros(B, D, **f32), torch.zeros(B, D, **f32), torch.zeros(B, D, **f32)
    recon = torch.zeros(B, 3, 32, 32, **f32)
    p0, nbt0, bn0 = st.params.clone(), st.bn_nbt.clone(), st.bn_stats.clone()
    img_d, eps_d, ts_d = image.to(dev).contiguous(), eps.to(dev).contiguous(), ts.to(dev).contiguous()
    out = eng.forward_backward(img_d, True, True, eps=eps_d, true_samples=ts_d, mu=mu, logvar=lv, z=z, recon_image=recon, **kw)
    o_loss, parts, (o_recon, o_mu, o_lv, o_z) = IV.step_loss(P, image, True, eps, ts, masks, 0.1 if with_masks else 0.0, **STEP_LAMBDAS)
    o_loss.backward()
    losses = out.losses().cpu()
    sums = eng.sums.cpu()
    l_err = abs(losses[0].item() - o_loss.item()) / abs(o_loss.item())
    mu_err, lv_err = (mu.cpu().double() - o_mu.detach()).abs().max().item(), (lv.cpu().double() - o_lv.detach()).abs().max().item()
    r_err = (recon.cpu().double() - o_recon.detach()).abs().max().item()
    assert l_err <= 1e-3, l_err
    assert abs(float(out.total()) - losses[0].item()) <= 1e-6 * abs(losses[0].item()) and losses[1].item() == 0.0 and losses[2].item() == 0.0
    assert all(float(sums[i]) == 0.0 for i in range(16) if i not in (0, 8, 12, 13, 14, 15)), sums
    assert mu_err <= 1e-2 and lv_err <= 1e-2, (mu_err, lv_err)
    assert r_err <= 2e-2, r_err
    m_err, m_yard = _check_mmd_slots(sums, ts, z, "step B=%d D=%d" % (B, D))
    # z of the returned mu / logvar: the formula as the library's own reparametrize evaluates it in fp32 (one fused multiply-add of eps,
    # the kernels' exp and mu), in fp32 ulps of z; and, printed, against the formula in float64
    z_lib = torch.empty(B, D, **f32)
    call("mmvae_reparam_fwd", ptr(mu), ptr(lv), ptr(eps_d), B * D, ptr(z_lib), stream())
    z_ulps = ((z.double() - z_lib.double()).abs().cpu() / _ulp(z_lib.double().cpu())).max().item()
    mu64, term = mu.cpu().double(), eps.double() * torch.exp(0.5 * lv.cpu().double())
    z64_ulps = ((z.cpu().double() - (mu64 + term)).abs() / _ulp(torch.maximum(mu64.abs(), term.abs()))).max().item()
    assert z_ulps <= 1.0, z_ulps
    assert z64_ulps <= Z64_GATE_ULPS, z64_ulps
    g = st.grads.cpu()
    pairs, second = [], []
    for n, shape, off in st.table:
        (pairs if n.startswith(IMG) else second).append((n, g[off:off + _numel(shape)], P[n].grad))
    assert len(second) > 0
    for n, gh, gr in second:
        assert gr is None and float(gh.abs().max()) == 0.0, n
    worst, tot = check_gradients(pairs, 4.5e-2, 2e-3, "infovae step B=%d D=%d masks=%d" % (B, D, with_masks))
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
    print("infovae step B=%d D=%d masks=%d: loss rel %.2e (1e-3) | mu %.2e logvar %.2e (1e-2) recon %.2e (2e-2) abs | z %.2f ulp (1) float64 %.2f ulp (4) | grad worst "
          "tensor %.3e (4.5e-2) total %.2e (2e-3) | running mean abs %.2e (2e-3) var rel %.2e (2e-2) | MMD values %.2e (gate %.2e)"
          % (B, D, with_masks, l_err, mu_err, lv_err, r_err, z_ulps, z64_ulps, worst, tot, rm_err, rv_err, m_err, MR.GATE_FACTOR * m_yard))
    # optimizer: plain Adam on the flat buffers, then one whole step through the packed-gradient Adam over the image range
    eng.optimizer_step()
    eng(img_d, eps=eps_d, true_samples=ts_d, **kw)
    torch.cuda.synchronize()
    for n, shape, off in st.table:
        same = torch.equal(st.params[off:off + _numel(shape)], p0[off:off + _numel(shape)])
        assert same == (not n.startswith(IMG)), n
    for i, (pre, c, off) in enumerate(st.bn_table):
        assert int(st.bn_nbt[i]) == int(nbt0[i]) + (2 if pre.startswith(IMG) else 0), pre
        if not pre.startswith(IMG):
            assert torch.equal(st.bn_stats[off:off + 2 * c], bn0[off:off + 2 * c]), pre
    assert int(eng.adam_state[0]) == 2


# ====================================================================================================== the MMD alone drives the encoder
def _module_route_errors(B, D, image, eps, ts, ref_grads, dev):
    """The existing module route (coco.InfoVAE + infovae_loss, the BCE term scaled by 0 -- ``lambda`` applied by scaling -- through
    autograd) on the same inputs against the same float64 gradients: {encoder tensor: rel-L2 error}."""
    from multimodal_vae_amd import coco as M
    P = R.formula_params("coco", D)
    sd = {}
    for k, v in P.items():
        if k.startswith(ENC):
            sd["encoder." + k[len(ENC):]] = v.detach().clone()
        elif k.startswith(DEC):
            sd["decoder." + k[len(DEC):]] = v.detach().clone()
    vae = M.InfoVAE(n_latents=D)
    vae.load_state_dict(sd, strict=True)
    vae = vae.cuda().train()
    for m in vae.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    mu, logvar = vae.encode(image.to(dev))
    z = vae.reparametrize(mu, logvar, eps.to(dev))
    loss = M.compute_mmd(ts.to(dev), z)
    loss.backward()
    errs = {}
    for n, p in vae.named_parameters():
        if n.startswith("encoder."):
            gr = ref_grads[ENC + n[len("encoder."):]]
            if gr is not None and float(gr.norm()) > 0:
                errs[ENC + n[len("encoder."):]] = float((p.grad.cpu().double().reshape(-1) - gr.reshape(-1)).norm() / gr.norm())
    return errs


@pytest.mark.parametrize("B,D", IV.MMD_ONLY_SHAPES)
def test_mmd_alone_drives_the_encoder(B, D):
    """lambda_x = 0, lambda_mmd = 1, kl_lambda = 0: the decoder's backward is skipped (every decoder gradient exactly 0) and
    lambda_mmd * dMMD/dz is the only dz.  The encoder gradients against the float64 instrument under the step's own per-tensor gate,
    4.5e-2, and total 2e-3.  The existing module route (coco.InfoVAE, compute_mmd through autograd) on the same inputs against the same
    oracle is printed beside it as the yardstick of what the bf16 chain does at these magnitudes.  Measured on MI355X, worst encoder
    tensor fused | module route: (6, 20) 1.547e-2 | 1.547e-2, (65, 100) 9.63e-3 | 9.66e-3: the bf16 chain holds the 4.5e-2 gate, so
    that gate stands and the module route is only printed."""
    from multimodal_vae_amd.core import FusedInfoVAEStep
    dev = _dev()
    st = _state(D, dev)
    P = IV.params(D, requires_grad=True)
    image, eps, ts = IV.inputs(B, D)
    eng = FusedInfoVAEStep(st, B, lambda_x=0.0, lambda_mmd=1.0, kl_lambda=0.0)
    eng.enc_dropout = False
    z = torch.zeros(B, D, device=dev)
    out = eng.forward_backward(image.to(dev).contiguous(), True, True, eps=eps.to(dev).contiguous(), true_samples=ts.to(dev).contiguous(), z=z)
    o_loss, parts, _ = IV.step_loss(P, image, True, eps, ts, lambda_x=0.0, lambda_mmd=1.0, kl_lambda=0.0)
    o_loss.backward()
    sums = eng.sums.cpu()
    _check_mmd_slots(sums, ts, z, "MMD alone B=%d D=%d" % (B, D))
    assert abs(float(out.total()) - float(sums[15])) <= 1e-7
    g = st.grads.cpu()
    pairs = []
    for n, shape, off in st.table:
        gh = g[off:off + _numel(shape)]
        if n.startswith(ENC):
            pairs.append((n, gh, P[n].grad))
        else:
            assert float(gh.abs().max()) == 0.0, n               # decoder and caption half: exactly 0
            assert P[n].grad is None or float(P[n].grad.abs().max()) == 0.0, n
    ref = {n: P[n].grad for n, _, _ in st.table if n.startswith(ENC)}
    route = _module_route_errors(B, D, image, eps, ts, ref, dev)
    tot_ref = math.sqrt(sum(float(gr.pow(2).sum()) for gr in ref.values() if gr is not None))
    fused = {n: float((gh.double() - gr.reshape(-1)).norm() / gr.norm()) for n, gh, gr in pairs if gr is not None and float(gr.norm()) >= 1e-6 * tot_ref}
    w_f = max(fused.items(), key=lambda kv: kv[1])
    w_r = max(((n, e) for n, e in route.items() if n in fused), key=lambda kv: kv[1])
    print("MMD alone B=%d D=%d: fused step worst encoder tensor %.3e (%s) | module route worst %.3e (%s) | gate 4.5e-2" % (B, D, w_f[1], w_f[0], w_r[1], w_r[0]))
    worst, tot = check_gradients(pairs, 4.5e-2, 2e-3, "infovae MMD alone B=%d D=%d" % (B, D))
    print("    total gradient norm rel %.2e (2e-3)" % tot)


# ====================================================================================================== lambda_mmd = 0
def test_lambda_mmd_zero_is_the_image_only_step():
    """The same inputs, seed and counter as mmvae_coco_image_step at kl_lambda = 0, noise and masks drawn by the step: inside the
    run-to-run budget tests/test_gpu_imageonly.py::test_step_draws_its_own_noise_and_masks documents (6e-2 rel-L2 on the whole gradient,
    losses rel 1e-3: the image step's BatchNorm statistics are fp32 atomics, so bit equality is not asked).  The MMD slots still hold
    the value, for the prior samples the step drew."""
    from multimodal_vae_amd.core import FusedImageStep, FusedInfoVAEStep
    dev = _dev()
    B, D = 6, 20
    image = R.formula_inputs("coco", B)[0].to(dev).contiguous()
    st_a, st_b = _state(D, dev), _state(D, dev)
    a = FusedImageStep(st_a, B, lr=1e-4, kl_lambda=0.0, lambda_x=1.0, seed=11)
    b = FusedInfoVAEStep(st_b, B, lambda_x=1.0, lambda_mmd=0.0, kl_lambda=0.0, seed=11)
    mu_a, mu_b, z = (torch.zeros(B, D, device=dev) for _ in range(3))
    _ws_floats(b, "dz_mmd", B, D).fill_(-7.0)                      # a sentinel where the MMD gradient would go
    sa = a.forward_backward(image, True, True, mu=mu_a).sums.clone().cpu()
    sb = b.forward_backward(image, True, True, mu=mu_b, z=z).sums.clone().cpu()
    assert bool(torch.isfinite(sb).all())
    for i in (0, 8):
        assert abs(float(sb[i]) - float(sa[i])) <= 1e-3 * abs(float(sa[i])), (i, sa, sb)
    assert all(float(sa[i]) == 0.0 for i in range(12, 16))
    g_err = float((st_b.grads - st_a.grads).double().norm() / st_a.grads.double().norm())
    mu_err = float((mu_a - mu_b).abs().max())
    print("lambda_mmd = 0 against the image-only step: whole gradient rel-L2 %.3e (6e-2), mu abs %.2e, BCE sums %.6g / %.6g"
          % (g_err, mu_err, float(sa[0]), float(sb[0])))
    assert g_err <= 6e-2
    assert torch.equal(st_a.bn_nbt, st_b.bn_nbt)
    drawn = _ws_floats(b, "true_samples", B, D).clone()
    _check_mmd_slots(sb, drawn, z, "lambda_mmd = 0")
    assert 0.0 < float(sb[15]) < 2.0
    dzm = _ws_floats(b, "dz_mmd", B, D)
    assert float(dzm.min()) == -7.0 and float(dzm.max()) == -7.0    # no gradient is formed at a zero weight: the sentinel is still there


# ====================================================================================================== the new kernels alone
def _mmd_dy(xd, yd, dev, scale=1.0, grad=True, ws=None):
    from multimodal_vae_amd._lib import call, ptr
    nx, ny, D = xd.shape[0], yd.shape[0], xd.shape[1]
    need = call("mmvae_mmd_dy_workspace_bytes", nx, ny, D)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(4, device=dev)
    dy = torch.full_like(yd, float("nan")) if grad else None
    call("mmvae_mmd_dy", ptr(xd), nx, ptr(yd), ny, D, ptr(ws), ws.numel(), scale, ptr(out), ptr(dy), 1,
         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return out, dy, ws


@pytest.mark.parametrize("nx,ny,D", [(65, 65, 100), (7, 130, 20)])
def test_y_only_sweep_is_deterministic_and_is_mmvae_mmd(nx, ny, D):
    """mmvae_mmd_dy twice on the same (x, y), the workspace filled with NaN in between: values and dy bit-identical.  Against mmvae_mmd
    on the same inputs: the fold order is kept (per pair, per 8 columns, per split, the same float64 sums), so the four values and dy
    are BIT-IDENTICAL, not merely within 1 ulp.  dx does not exist for this entry; the workspace holds gradient partials for y's rows
    alone.  scale = 0.5 halves dy exactly; the value-only form (dy NULL) gives the same four values."""
    from multimodal_vae_amd._lib import call, ptr
    dev = _dev()
    x, y = MR.real_inputs(nx, ny, D)
    xd, yd = x.to(dev).contiguous(), y.to(dev).contiguous()
    out1, dy1, ws = _mmd_dy(xd, yd, dev)
    ws.fill_(0xFF)                                                 # NaN in every float64 of the workspace
    out2, dy2, _ = _mmd_dy(xd, yd, dev, ws=ws)
    bits = lambda t: t.view(torch.int32)
    assert bool(torch.isfinite(out2).all()) and bool(torch.isfinite(dy2).all())
    assert torch.equal(bits(out1), bits(out2)) and torch.equal(bits(dy1), bits(dy2))
    need = call("mmvae_mmd_workspace_bytes", nx, ny, D)
    assert ws.numel() < need
    ws_full = torch.empty(need, dtype=torch.uint8, device=dev)
    out_ref, dx_ref, dy_ref = torch.empty(4, device=dev), torch.empty_like(xd), torch.empty_like(yd)
    call("mmvae_mmd", ptr(xd), nx, ptr(yd), ny, D, ptr(ws_full), need, ptr(out_ref), ptr(dx_ref), ptr(dy_ref),
         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    ulps = float(((dy1.double() - dy_ref.double()).abs() / _ulp(dy_ref.double().cpu()).to(dev)).max())
    print("mmd_dy (%d, %d, %d): dy against mmvae_mmd %.2f ulp, values equal %s" % (nx, ny, D, ulps, torch.equal(bits(out1), bits(out_ref))))
    assert torch.equal(bits(out1), bits(out_ref)) and torch.equal(bits(dy1), bits(dy_ref))
    out3, dy3, _ = _mmd_dy(xd, yd, dev, scale=0.5)
    assert torch.equal(bits(out3), bits(out1)) and torch.equal(dy3, 0.5 * dy1)
    out4, _, _ = _mmd_dy(xd, yd, dev, grad=False)
    assert torch.equal(bits(out4), bits(out1))
    # and against float64, under the gates of tests/test_gpu_mmd.py
    c = MR.real_case(nx, ny, D)
    assert MR.value_error(out1, c["ref"]["terms"]) <= MR.GATE_FACTOR * c["yardstick"]["value"]
    assert MR.grad_error(dy1, c["ref"]["dy"]) <= MR.GATE_FACTOR * c["yardstick"]["dy"]


# ====================================================================================================== drawn prior samples, eval mode
def test_drawn_prior_samples_and_eval_mode():
    """true_samples = NULL: the step's prologue draws them on Philox stream 5 keyed by seed and step counter -- the values of
    mmvae_normal for that stream, read back through mmvae_coco_debug_offset.  Eval mode (training = 0, do_backward = 0): z == mu bit for
    bit, nothing of the parameters, gradients or BatchNorm buffers written, the same seed and counter give the same MMD slots for the
    same z, another seed gives others; BCE and MMD inside the gates of the training step."""
    from multimodal_vae_amd import coco as M
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd._ops import stream
    from multimodal_vae_amd.core import FusedInfoVAEStep
    dev = _dev()
    B, D = 6, 20
    st = _state(D, dev)
    image = R.formula_inputs("coco", B)[0]
    img_d = image.to(dev).contiguous()
    eng = FusedInfoVAEStep(st, B, seed=11)
    eng.adam_state[0] = 3                                           # a step counter other than 0
    st.grads.fill_(7.0)
    p0, bn0, nbt0, g0 = st.params.clone(), st.bn_stats.clone(), st.bn_nbt.clone(), st.grads.clone()
    mu, z = torch.zeros(B, D, device=dev), torch.zeros(B, D, device=dev)
    out = eng.evaluate(img_d, mu=mu, z=z)
    s1 = eng.sums.clone()
    drawn = _ws_floats(eng, "true_samples", B, D).clone()
    want = torch.empty(B, D, device=dev)
    call("mmvae_normal", ptr(want), B * D, 11, ptr(eng.adam_state), M.TRUE_SAMPLES_STREAM, stream())
    assert torch.equal(drawn, want) and 0.5 < float(drawn.std()) < 1.5
    assert torch.equal(z, mu)
    assert torch.equal(st.params, p0) and torch.equal(st.bn_stats, bn0) and torch.equal(st.bn_nbt, nbt0) and torch.equal(st.grads, g0)
    P = IV.params(D)
    with torch.no_grad():
        o_loss, parts, (_, o_mu, _, _) = IV.step_loss(P, image, False, None, drawn.cpu())
    assert (mu.cpu().double() - o_mu).abs().max().item() <= 1e-2
    l_err = abs(float(out.total()) - float(o_loss)) / abs(float(o_loss))
    print("eval mode: BCE + MMD %.6f, oracle %.6f, rel %.2e (1e-3)" % (float(out.total()), float(o_loss), l_err))
    assert l_err <= 1e-3
    assert all(float(s1[i]) == 0.0 for i in range(16) if i not in (0, 8, 12, 13, 14, 15))
    _check_mmd_slots(s1.cpu(), drawn, z, "eval mode")
    z2 = torch.zeros(B, D, device=dev)
    eng.evaluate(img_d, z=z2)
    assert torch.equal(z2, z) and torch.equal(eng.sums[MMD_SLOTS].view(torch.int32), s1[MMD_SLOTS].view(torch.int32))
    eng.seed = 12
    eng.evaluate(img_d, z=z2)
    assert torch.equal(z2, z) and not torch.equal(eng.sums[MMD_SLOTS], s1[MMD_SLOTS])
    assert not torch.equal(_ws_floats(eng, "true_samples", B, D), drawn)
    eng.seed = 11
    eng.adam_state[0] = 4                                           # ... and another counter
    eng.evaluate(img_d, z=z2)
    assert not torch.equal(_ws_floats(eng, "true_samples", B, D), drawn)
    # given samples win over the draw; a training forward without backward reports the MMD too
    eng.forward_backward(img_d, True, False, true_samples=drawn, z=z2)
    assert not torch.equal(z2, z) and float(eng.sums[15]) != 0.0
    assert torch.equal(st.grads, g0) and torch.equal(st.params, p0)


def test_step_takes_one_row():
    """B = 1 through the step in eval mode (training = 0, do_backward = 0): z == mu, MMD of 1 x 1 = {1, 1, k, 2 - 2 k} for the given prior
    sample, BCE against the float64 instrument under the loss gate, nothing written.  (A training step at B = 1 is not exercised here.)"""
    from multimodal_vae_amd.core import FusedInfoVAEStep
    dev = _dev()
    B, D = 1, 20
    st = _state(D, dev)
    image, _, ts = IV.inputs(B, D)
    eng = FusedInfoVAEStep(st, B)
    p0, bn0 = st.params.clone(), st.bn_stats.clone()
    mu, z = torch.zeros(B, D, device=dev), torch.zeros(B, D, device=dev)
    out = eng.evaluate(image.to(dev).contiguous(), true_samples=ts.to(dev).contiguous(), mu=mu, z=z)
    s = eng.sums.cpu()
    assert torch.equal(z, mu) and torch.equal(st.params, p0) and torch.equal(st.bn_stats, bn0)
    k = math.exp(-float(((ts.double() - z.cpu().double()) ** 2).sum()) / D / D)
    with torch.no_grad():
        o_loss, _, (_, o_mu, _, _) = IV.step_loss(IV.params(D), image, False, None, ts)
    l_err = abs(float(out.total()) - float(o_loss)) / abs(float(o_loss))
    print("step at B = 1: slots %s, k = %.8f, BCE + MMD rel %.2e (1e-3), mu abs %.2e (1e-2)"
          % ([float(v) for v in s[MMD_SLOTS]], k, l_err, float((mu.cpu().double() - o_mu).abs().max())))
    assert float(s[12]) == 1.0 and float(s[13]) == 1.0 and abs(float(s[14]) - k) <= 2e-7 and abs(float(s[15]) - (2 - 2 * k)) <= 5e-7
    assert l_err <= 1e-3 and float((mu.cpu().double() - o_mu).abs().max()) <= 1e-2


def test_one_by_one():
    """MMD of 1 x 1 (a batch of one row) through the y-only entry: {1, 1, k, 2 - 2 k} and dy, the bits of mmvae_mmd."""
    from multimodal_vae_amd._lib import call, ptr
    dev = _dev()
    D = 4
    x, y = MR.real_inputs(1, 1, D)
    xd, yd = x.to(dev).contiguous(), y.to(dev).contiguous()
    out, dy, _ = _mmd_dy(xd, yd, dev)
    k = math.exp(-float(((x.double() - y.double()) ** 2).sum()) / D / D)
    s = out.cpu()
    print("1 x 1: values %s, k = %.8f" % ([float(v) for v in s], k))
    assert float(s[0]) == 1.0 and float(s[1]) == 1.0 and abs(float(s[2]) - k) <= 2e-7 and abs(float(s[3]) - (2 - 2 * k)) <= 5e-7
    need = call("mmvae_mmd_workspace_bytes", 1, 1, D)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    o2, dx2, dy2 = torch.empty(4, device=dev), torch.empty_like(xd), torch.empty_like(yd)
    call("mmvae_mmd", ptr(xd), 1, ptr(yd), 1, D, ptr(ws), need, ptr(o2), ptr(dx2), ptr(dy2), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert torch.equal(out.view(torch.int32), o2.view(torch.int32)) and torch.equal(dy.view(torch.int32), dy2.view(torch.int32))
    assert float(dy.abs().max()) > 0.0


# ====================================================================================================== refusals
def test_refusals_happen_on_the_host():
    from multimodal_vae_amd import _lib, core
    from multimodal_vae_amd._lib import MMVAEError, call
    from multimodal_vae_amd._ops import stream
    dev = _dev()
    B, D = 4, 20
    st = _state(D, dev)
    eng = core.FusedInfoVAEStep(st, B)
    image = R.formula_inputs("coco", B)[0].to(dev).contiguous()
    st.grads.fill_(7.0)
    eng.sums.fill_(5.0)
    io = eng._io(_lib.InfoVAEStepIO, (("image", image),), dict(eps=None, enc_mask1=None, enc_mask2=None, true_samples=None,
                                                                recon_image=None, mu=None, logvar=None, z=None))
    need = call("mmvae_coco_infovae_step_workspace_bytes", eng.h)
    assert eng.ws.numel() == need
    io.ws_bytes = need - 1
    with pytest.raises(MMVAEError, match="workspace too small"):
        call("mmvae_coco_infovae_step", eng.h, C.byref(io), 1, 1, stream())
    io.ws_bytes = need
    m1 = torch.ones(B, 1024, dtype=torch.uint8, device=dev)
    io.enc_mask1 = m1.data_ptr()
    with pytest.raises(MMVAEError, match="enc_mask1 / enc_mask2 go together"):
        call("mmvae_coco_infovae_step", eng.h, C.byref(io), 1, 1, stream())
    with pytest.raises(MMVAEError, match="expected images"):
        eng.forward_backward(torch.zeros(B, 3, 64, 64, device=dev))
    torch.cuda.synchronize()
    assert float(st.grads.min()) == 7.0 and float(st.grads.max()) == 7.0 and float(eng.sums.min()) == 5.0       # nothing was launched
    for bad in (2, 126, 128):
        with pytest.raises(MMVAEError, match="4..124"):
            core.FusedInfoVAEStep(core.CocoState(bad, dev, COCO_T), B)
    # ... and the engine still works
    io.enc_mask1 = None
    call("mmvae_coco_infovae_step", eng.h, C.byref(io), 1, 1, stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(eng.sums).all()) and float(eng.sums[15]) > 0.0


# ====================================================================================================== trainer and driver
def _batch(B, seed=5):
    """B images in [0, 1] with structure a decoder can learn: one smooth pattern, dimmed per example (tests/test_gpu_infovae.py)"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(32.0), torch.arange(32.0), indexing="ij")
    base = torch.stack([0.5 + 0.5 * torch.sin(0.3 * xx + c) * torch.cos(0.2 * yy - c) for c in range(3)])
    level = 0.15 + 0.5 * torch.rand(B, 1, 1, 1, generator=g)
    return (base[None] * level + 0.03 * torch.rand(B, 3, 32, 32, generator=g)).clamp(0, 1).contiguous()


def test_trainer_reduces_the_loss():
    from multimodal_vae_amd import coco as M
    dev = _dev()
    torch.manual_seed(0)
    vae = M.FusedInfoVAE(n_latents=20).cuda().train()
    trainer = M.InfoVAETrainer(vae, 32, lr=1e-3, seed=3)
    assert trainer.engine.kl_lambda == 0.0 and trainer.engine.lambda_mmd == 1.0 and trainer.engine.lambda_x == 1.0
    img = _batch(32).to(dev)
    losses, parts = [], []
    for _ in range(31):                                            # the first loss, then 30 Adam steps
        out = trainer(img)
        losses.append(out.total().clone())
        parts.append(torch.stack((out.bce(), out.mmd())))
    losses, parts = torch.stack(losses).cpu().tolist(), torch.stack(parts).cpu()
    first, last = losses[0], losses[-1]
    print("InfoVAETrainer: BCE + MMD %.5f -> %.5f over 30 steps (BCE %.5f -> %.5f, MMD %.5f -> %.5f)"
          % (first, last, float(parts[0, 0]), float(parts[-1, 0]), float(parts[0, 1]), float(parts[-1, 1])))
    assert np.isfinite(last) and last < 0.95 * first, (first, last)
    assert abs(losses[-1] - float(parts[-1].sum())) < 1e-5
    assert int(trainer.engine.adam_state[0]) == 31
    ev = trainer.evaluate(img)
    assert np.isfinite(float(ev.total()))
    vae.eval()
    with torch.no_grad():
        recon, z = vae(img)
    assert recon.shape == (32, 3, 32, 32) and z.shape == (32, 20)


def test_command_lines(tmp_path, capsys):
    from multimodal_vae_amd import coco as M, evaluate as E, train_infovae as T
    from multimodal_vae_amd.train_coco import synthetic_coco
    dev = _dev()
    out, results = str(tmp_path / "models"), str(tmp_path / "results")
    hist = T.main(["--fused", "--synthetic", "256", "--epochs", "1", "--batch_size", "32", "--n_latents", "20", "--cuda", "--out", out,
                   "--results", results, "--log_interval", "4", "--seed", "3"])
    printed = capsys.readouterr().out
    assert "Train Epoch: 1 [0/256 (0%)]\tLoss: " in printed and "====> Epoch: 1 Average loss: " in printed
    assert "====> Test set loss: " in printed
    assert len(hist["train"]) == 1 and len(hist["test"]) == 1 and all(np.isfinite(v) for v in hist["train"] + hist["test"])
    ckpt = os.path.join(out, "infovae", "checkpoint.pth.tar")
    assert hist["checkpoint"] == ckpt and os.path.exists(os.path.join(out, "infovae", "model_best.pth.tar"))
    state = torch.load(ckpt, weights_only=False)
    assert sorted(state) == ["best_loss", "n_latents", "optimizer", "state_dict"] and state["n_latents"] == 20
    assert state["best_loss"] == min(hist["test"])
    plain, fused = M.InfoVAE(20), M.FusedInfoVAE(20)
    plain.load_state_dict(state["state_dict"], strict=True)
    fused.load_state_dict(state["state_dict"], strict=True)
    opt = torch.optim.Adam(plain.parameters(), lr=1e-4)
    opt.load_state_dict(state["optimizer"])                       # saved as the other fused drivers save theirs
    assert len(state["optimizer"]["state"]) == len(list(plain.parameters()))
    assert int(state["state_dict"]["encoder.features.3.num_batches_tracked"]) == 8
    a, b = T.load_checkpoint(ckpt, use_cuda=True), T.load_checkpoint(ckpt, use_cuda=True, fused=True)
    assert type(a) is M.InfoVAE and type(b) is M.FusedInfoVAE and next(b.parameters()).is_cuda
    img = _batch(8).to(dev)
    a.eval(); b.eval()
    with torch.no_grad():
        (ra, za), (rb, zb) = a(img), b(img)
    assert torch.equal(za, zb) and torch.equal(ra, rb)             # the same kernels on the same parameters
    assert tuple(torch.load(os.path.join(results, "sample_epoch1.pt")).shape) == (64, 3, 32, 32)
    r = E._main(["latent_mmd", ckpt, "--synthetic", "512"])
    printed = capsys.readouterr().out
    assert "Latent MMD over 512 examples" in printed
    assert r["n"] == 512 and all(np.isfinite(r[k]) for k in ("k_prior", "k_posterior", "k_cross", "mmd"))

    # without --fused the driver is what it was: the first logged loss is the module route's, called directly in the same order
    T.main(["--synthetic", "256", "--epochs", "1", "--batch_size", "32", "--n_latents", "20", "--cuda", "--out", str(tmp_path / "m2"),
            "--log_interval", "100", "--seed", "3"])
    printed = capsys.readouterr().out
    line = [l for l in printed.splitlines() if l.startswith("Train Epoch: 1 [0/256 (0%)]")][0]
    logged = float(line.split("Loss: ")[1])
    torch.manual_seed(3)
    tr_x = synthetic_coco(256, seed=3)[0]
    synthetic_coco(max(32, 256 // 6), seed=4)
    loader = T._DeviceImages(tr_x, 32, dev, shuffle=True, seed=3)
    T._DeviceImages(tr_x[:32], 32, dev, shuffle=True, seed=10)
    vae = M.InfoVAE(n_latents=20).cuda()
    torch.optim.Adam(vae.parameters(), lr=1e-4)
    vae.train()
    data = next(iter(loader))
    recon, z = vae(data)
    direct = float(M.infovae_loss(recon, data, z))
    print("train_infovae without --fused: first logged loss %.6f, the module route called directly %.6f" % (logged, direct))
    assert abs(logged - direct) <= 1e-3 * abs(direct)
