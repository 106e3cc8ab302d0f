"""MNIST's uni-modal image VAE (mnist/model.py:188-232, mnist/imageonly/*) on the GPU: the one-pass step mmvae_mnist_image_step
against the float64 restatement of tests/imageonly_mnist_ref.py under the gates tests/test_gpu_mnist.py applies to the fp32 plan
(with the column-strip Linear + BatchNorm kernels of csrc/mnist_strip.hip and with the unfused launches), the strip kernels alone next
to the launches they replace, determinism and row independence, the untouched label half, the module face, the scorer, trainer,
driver and refusals.
Measured on MI355X, worst error / gate of the step over the five cases: strip 0.54, unfused 0.87 (both recon atol 1e-5 at B = 2; every
other case <= 0.18).  Strip kernels alone: r error 3.0e-7 against gemm_f32's 3.3e-7 at 2 rows, K = 784."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from oracle import mmvae_ref as R
import imageonly_mnist_ref as IR

pytestmark = pytest.mark.gpu

IMG = ("image_encoder.", "image_decoder.")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _strip(v):
    """``with _strip(v):`` the switch "mnist_strip" at v, back at the library's default afterwards"""
    from multimodal_vae_amd._lib import knobs
    return knobs(mnist_strip=v)


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _state(D, dev, precision="fp32"):
    """An MnistState with the formula parameters of the WHOLE MMVAE table (the label half too: it has to come out untouched)"""
    from multimodal_vae_amd.core import MnistState
    P = R.formula_params("mnist", D)
    st = MnistState(D, dev, precision=precision)
    assert [t[0] for t in st.table] == [n for n, _ in R.param_table("mnist", D)]
    for n, shape, off in st.table:
        st.params[off:off + P[n].numel()] = P[n].detach().reshape(-1).to(dev)
    return st


def _engine(st, B, **kw):
    from multimodal_vae_amd.core import FusedImageStep
    return FusedImageStep(st, B, kl_lambda=1.0 / 784, lambda_x=1.0 / B, **kw)


def _collect(st, eng, out, mu, lv, recon, training, params_before=None):
    """The step's results in the layout of imageonly_mnist_ref.run"""
    got = dict(loss=float(out.losses()[0]), kl=float(out.parts()[2][0]), mu=mu.cpu(), logvar=lv.cpu(), recon=recon.cpu())
    got["running"], got["nbt"] = {}, {}
    for i, (pre, c, off) in enumerate(st.bn_table):
        if pre.startswith(IMG):
            got["running"][pre + ".running_mean"] = st.bn_stats[off:off + c].cpu()
            got["running"][pre + ".running_var"] = st.bn_stats[off + c:off + 2 * c].cpu()
            got["nbt"][pre] = int(st.bn_nbt[i])
    if training:
        g, p = st.grads.cpu(), st.params.cpu()
        got["grads"] = {n: g[off:off + _numel(s)].view(s) for n, s, off in st.table if n.startswith(IMG)}
        got["params_after"] = {n: p[off:off + _numel(s)].view(s) for n, s, off in st.table if n.startswith(IMG)}
    return got


# ====================================================================================================== the step against float64
@pytest.mark.parametrize("strip", [0, 1])
@pytest.mark.parametrize("B,D", IR.CASES)
def test_step_matches_float64(B, D, strip):
    with _strip(strip):
        _step_matches_float64(B, D, strip)


def _step_matches_float64(B, D, strip):
    """One training step (given eps; zero_grad, forward, loss, backward, Adam over the image parameters) and one eval-mode forward
    against the float64 restatement: loss rtol 2e-5, KL sum rtol 2e-5, mu / logvar atol 1e-4, recon atol 1e-5, every gradient tensor
    |g - g_ref| <= 1e-3 |g_ref| + 1e-6 |g|_total (the Linear biases in front of a BatchNorm: |g| <= 1e-5), running_mean atol 1e-5,
    running_var rtol 1e-4 atol 1e-6, num_batches_tracked + 1, parameters after Adam as tests/test_gpu_mnist.py (norm rtol 1e-4).
    What was measured is printed (worst error / gate).  Both settings of the switch "mnist_strip": the column-strip fused layers, and
    gemm_f32 + the BatchNorm kernels."""
    from multimodal_vae_amd._lib import call
    dev = _dev()
    assert call("mmvae_mnist_strip_route", B) == strip
    image, eps = IR.inputs(B, D)
    st = _state(D, dev)
    eng = _engine(st, B)
    before = st.params.clone()
    mu, lv, recon = (torch.zeros(B, D, device=dev), torch.zeros(B, D, device=dev), torch.zeros(B, 784, device=dev))
    x = image.to(dev).contiguous()
    out = eng(x, eps=eps.to(dev).contiguous(), mu=mu, logvar=lv, recon_image=recon)
    got = _collect(st, eng, out, mu, lv, recon, True)
    ref = IR.run(D, B, True)
    fails, ratios = IR.check(ref, got, True)
    worst = sorted(ratios.items(), key=lambda kv: -kv[1])[:5]
    print("mnist image step strip=%d B=%d D=%d train: loss %.8f (ref %.8f); worst error / gate: %s"
          % (strip, B, D, got["loss"], ref["loss"], "; ".join("%s %.3f" % kv for kv in worst)))
    assert not fails, fails
    sums = out.sums.cpu()
    assert all(float(sums[i]) == 0.0 for i in range(16) if i not in (0, 8)) and float(sums[8]) > 0
    # the label half: never launched.  Gradient exactly 0, parameters and buffers keep their bits
    for n, shape, off in st.table:
        if not n.startswith(IMG):
            assert float(st.grads[off:off + _numel(shape)].abs().max()) == 0.0, n
            assert torch.equal(st.params[off:off + _numel(shape)], before[off:off + _numel(shape)]), n
    assert int(eng.adam_state[0]) == 1
    # the same images as (B, 1, 28, 28): the same step
    st2 = _state(D, dev)
    out2 = _engine(st2, B)(x.view(B, 1, 28, 28), eps=eps.to(dev).contiguous())
    np.testing.assert_allclose(out2.sums.cpu().numpy(), sums.numpy(), rtol=1e-5)
    # eval mode on the updated model: z = mu, running statistics read and left alone
    bn0, nbt0 = st.bn_stats.clone(), st.bn_nbt.clone()
    oute = eng.forward_backward(x, False, False, mu=mu, logvar=lv, recon_image=recon)
    gote = _collect(st, eng, oute, mu, lv, recon, False)
    assert torch.equal(st.bn_stats, bn0) and torch.equal(st.bn_nbt, nbt0)
    # (the float64 eval forward of the model the GPU now holds: its parameters and running statistics, read back)
    p64 = {}
    for n, shape, off in st.table:
        if n.startswith(IMG):
            p64[n] = st.params[off:off + _numel(shape)].view(shape).double().cpu()
    for i, (pre, c, off) in enumerate(st.bn_table):
        if pre.startswith(IMG):
            p64[pre + ".running_mean"] = st.bn_stats[off:off + c].double().cpu()
            p64[pre + ".running_var"] = st.bn_stats[off + c:off + 2 * c].double().cpu()
            p64[pre + ".num_batches_tracked"] = st.bn_nbt[i].cpu().clone()
    with torch.no_grad():
        r64, mu64, lv64 = IR.forward(p64, image, False, eps)
        refe = dict(loss=float(IR.loss_function(r64, image, mu64, lv64)), kl=float(IR.kl_sum(mu64, lv64)), mu=mu64, logvar=lv64, recon=r64,
                    running={k: v for k, v in p64.items() if k.endswith(("running_mean", "running_var"))}, nbt=gote["nbt"])
    fails, ratios = IR.check(refe, gote, False)
    print("mnist image step strip=%d B=%d D=%d eval: loss %.8f (ref %.8f); worst error / gate: %s"
          % (strip, B, D, gote["loss"], refe["loss"], "; ".join("%s %.3f" % kv for kv in sorted(ratios.items(), key=lambda kv: -kv[1])[:3])))
    assert not fails, fails


@pytest.mark.parametrize("strip", [0, 1])
def test_step_is_deterministic_and_rows_are_independent(strip):
    with _strip(strip):
        _step_is_deterministic_and_rows_are_independent()


def _step_is_deterministic_and_rows_are_independent():
    """Two runs on the same inputs: mu, logvar, recon, the KL sum, every gradient and running statistic bit-equal (the fp32 plan's GEMMs,
    BatchNorms and the latent block have no float atomics); the BCE sum goes through fp32 atomic slots: rtol.  Drawn noise: the same
    seed and counter give the same step, another seed another.  Eval mode: permuting the rows permutes the outputs bit for bit."""
    dev = _dev()
    B, D = 23, 20
    image, eps = IR.inputs(B, D)
    x, e = image.to(dev).contiguous(), eps.to(dev).contiguous()
    runs = []
    for _ in range(2):
        st = _state(D, dev)
        eng = _engine(st, B, seed=11)
        mu, lv, recon = torch.zeros(B, D, device=dev), torch.zeros(B, D, device=dev), torch.zeros(B, 784, device=dev)
        out = eng.forward_backward(x, True, True, eps=e, mu=mu, logvar=lv, recon_image=recon)
        runs.append((mu, lv, recon, out.sums.clone(), st.grads.clone(), st.bn_stats.clone(), st.bn_nbt.clone()))
    a, b = runs
    for k, name in enumerate(("mu", "logvar", "recon")):
        assert torch.equal(a[k], b[k]), name
    assert torch.equal(a[3][8], b[3][8])
    np.testing.assert_allclose(a[3].cpu().numpy(), b[3].cpu().numpy(), rtol=1e-5)        # (the BCE slots are fp32 atomics)
    assert torch.equal(a[4], b[4]) and torch.equal(a[5], b[5]) and torch.equal(a[6], b[6])
    # drawn noise
    bn0, nbt0 = st.bn_stats.clone(), st.bn_nbt.clone()
    d1 = eng.forward_backward(x, True, True).sums.clone()
    st.bn_stats.copy_(bn0); st.bn_nbt.copy_(nbt0)
    d2 = eng.forward_backward(x, True, True).sums.clone()
    assert torch.equal(d1[8], d2[8]) and bool(torch.isfinite(d1).all())
    eng.seed = 12
    d3 = eng.forward_backward(x, True, True).sums.clone()
    assert not torch.equal(d3[0], d1[0])
    # eval mode: rows do not see each other
    st.bn_stats.copy_(bn0); st.bn_nbt.copy_(nbt0)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).to(dev)
    outs = []
    for xx in (x, x[perm].contiguous()):
        mu, lv, recon = torch.zeros(B, D, device=dev), torch.zeros(B, D, device=dev), torch.zeros(B, 784, device=dev)
        eng.forward_backward(xx, False, False, eps=torch.ones(B, D, device=dev), mu=mu, logvar=lv, recon_image=recon)
        outs.append((mu, lv, recon))
    for k, name in enumerate(("mu", "logvar", "recon")):
        assert torch.equal(outs[0][k][perm], outs[1][k]), name
    assert torch.equal(st.bn_stats, bn0) and torch.equal(st.bn_nbt, nbt0)


@pytest.mark.parametrize("strip", [0, 1])
def test_label_half_is_untouched_by_the_trainer(strip):
    with _strip(strip):
        _label_half_is_untouched_by_the_trainer()


def _label_half_is_untouched_by_the_trainer():
    """3 trainer steps: label-half parameters, BatchNorm buffers, exp_avg and exp_avg_sq bit-equal to before, its gradient exactly 0;
    the four image BatchNorms counted 3 batches."""
    from multimodal_vae_amd import mnist as M
    dev = _dev()
    B, D = 16, 20
    torch.manual_seed(0)
    vae = M.VAE(D).cuda()
    tr = M.ImageVAETrainer(vae, B)
    st, eng = tr.engine.state, tr.engine
    with torch.no_grad():                 # give the label half values to lose
        for n, shape, off in st.table:
            if not n.startswith(IMG):
                st.params[off:off + _numel(shape)] = torch.linspace(-1, 1, _numel(shape), device=dev)
    lab = [(i, pre, c, off) for i, (pre, c, off) in enumerate(st.bn_table) if not pre.startswith(IMG)]
    assert len(lab) == 2 and len(st.bn_table) == 6
    p0, bn0, nbt0 = st.params.clone(), st.bn_stats.clone(), st.bn_nbt.clone()
    x = IR.inputs(B, D)[0].to(dev).view(B, 1, 28, 28)
    for _ in range(3):
        tr(x)
    n_img = eng.n_image_params
    assert n_img == sum(_numel(s) for n, s, _ in st.table if n.startswith(IMG)) < st.nparams
    assert torch.equal(st.params[n_img:], p0[n_img:]) and not torch.equal(st.params[:n_img], p0[:n_img])
    assert float(st.grads[n_img:].abs().max()) == 0.0
    assert float(eng.exp_avg[n_img:].abs().max()) == 0.0 and float(eng.exp_avg_sq[n_img:].abs().max()) == 0.0
    assert float(eng.exp_avg[:n_img].abs().max()) > 0.0
    for i, pre, c, off in lab:
        assert torch.equal(st.bn_stats[off:off + 2 * c], bn0[off:off + 2 * c]) and int(st.bn_nbt[i]) == int(nbt0[i]) == 0, pre
    sd = vae.state_dict()
    for pre in ("encoder.1", "encoder.4", "decoder.1", "decoder.4"):
        assert int(sd[pre + ".num_batches_tracked"]) == 3, pre
    assert int(eng.adam_state[0]) == 3


# ====================================================================================================== the strip kernels alone
U32 = 2.0 ** -24
LAYERS = (("image_encoder.net.0+1", 400, 784, 200), ("image_encoder.net.3+4", 200, 400, 40),        # name, N, K, Nn (the next Linear's width)
          ("image_decoder.net.0+1", 200, 20, 400), ("image_decoder.net.3+4", 400, 200, 784))


def _layer_fwd(route, t, rows, N, K, training):
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd._ops import stream
    dev = t["x"].device
    o = dict(r=torch.full((rows, N), 7.0, device=dev), a=torch.full((rows, N), 7.0, device=dev), mr=torch.full((N, 2), 7.0, device=dev),
             rm=t["rm"].clone(), rv=t["rv"].clone(), nbt=torch.zeros(1, dtype=torch.int64, device=dev))
    call("mmvae_mnist_lin_bn_act_fwd", route, ptr(t["x"]), K, ptr(t["w"]), ptr(t["b"]), ptr(t["gamma"]), ptr(t["beta"]), ptr(o["rm"]), ptr(o["rv"]),
         ptr(o["nbt"]), rows, N, K, int(training), ptr(o["r"]), ptr(o["a"]), ptr(o["mr"]), stream())
    return o


def _layer_bwd(route, t, rows, N, Nn):
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd._ops import stream
    dev = t["dy"].device
    o = dict(d_r=torch.full((rows, N), 7.0, device=dev), dgamma=torch.zeros(N, device=dev), dbeta=torch.zeros(N, device=dev))
    call("mmvae_mnist_lin_dgrad_bn_bwd", route, ptr(t["dy"]), Nn, ptr(t["wn"]), ptr(t["r"]), ptr(t["mr"]), ptr(t["gamma"]), ptr(t["beta"]), rows, N,
         ptr(o["d_r"]), ptr(o["dgamma"]), ptr(o["dbeta"]), stream())
    return o


def _yardstick(name, strip, unf, ref, floor, report):
    """|strip - ref| <= 2 max|unfused - ref| + floor, elementwise (the yardstick is the existing kernels' own error on the same operands)"""
    es, eu = (strip.double().cpu() - ref).abs(), (unf.double().cpu() - ref).abs()
    allowed = 2.0 * float(eu.max()) + floor
    ratio = float((es / allowed.clamp(min=1e-300)).max())
    report.append("%s %.2f (strip %.1e, unfused %.1e)" % (name, ratio, float(es.max()), float(eu.max())))
    assert ratio <= 1.0, (name, ratio, float(es.max()), float(eu.max()))


@pytest.mark.parametrize("rows", [2, 15, 16, 17, 33, "cap", "cap+1"])
def test_strip_layers_against_float64_next_to_the_unfused_launches(rows):
    """Forward and backward of each of the four fused layers (the real widths: 400 = 25 strips, 200 = 12 strips + a ragged one of 8)
    through mmvae_mnist_lin_bn_act_fwd / mmvae_mnist_lin_dgrad_bn_bwd, the strip kernel next to the launches it replaces, both against
    float64 on the same fp32 operands.  The strip form's error may be at most 2 x the unfused chain's on the same inputs plus a floor
    of 2 K 2^-24 sum|terms| (propagated to the quantities behind the GEMM as written below).  Rows: 2, the ragged row tiles 15 / 16 /
    17 / 33, the cap, and cap + 1, which takes the unfused route (the strip kernel refuses it).  Two strip calls give equal bits."""
    from multimodal_vae_amd._lib import MMVAEError, call
    dev = _dev()
    cap = call("mmvae_mnist_strip_max_rows")
    assert cap == 512
    over = rows == "cap+1"
    rows = cap if rows == "cap" else cap + 1 if over else rows
    with _strip(1):
        assert call("mmvae_mnist_strip_route", cap) == 1 and call("mmvae_mnist_strip_route", cap + 1) == 0 and call("mmvae_mnist_strip_route", rows) == (0 if over else 1)
    with _strip(0):
        assert call("mmvae_mnist_strip_route", 2) == 0
    assert call("mmvae_mnist_strip_route", 128) == 1          # the library's default: on (profiles/imageonly_mnist_bench.txt)
    g = torch.Generator().manual_seed(rows)
    rnd = lambda *s: torch.randn(*s, generator=g)
    report = []
    for name, N, K, Nn in LAYERS:
        t = dict(x=rnd(rows, K).abs() * 0.5, w=rnd(N, K) / math.sqrt(K), b=0.05 * rnd(N), gamma=1 + 0.1 * rnd(N), beta=0.1 * rnd(N),
                 rm=0.1 * rnd(N), rv=1 + 0.1 * rnd(N).abs())
        t = {k: v.to(dev).contiguous() for k, v in t.items()}
        d = {k: v.double().cpu() for k, v in t.items()}
        for training in (True, False):
            if over:
                with pytest.raises(MMVAEError, match="a workgroup carries"):
                    _layer_fwd(1, t, rows, N, K, training)
                with _strip(1):
                    s_ = _layer_fwd(-1, t, rows, N, K, training)           # what the step takes above the cap: the unfused launches
            else:
                s_ = _layer_fwd(1, t, rows, N, K, training)
                s2 = _layer_fwd(1, t, rows, N, K, training)
                assert all(torch.equal(s_[k], s2[k]) for k in s_), name     # fixed fold orders, no atomics
            u_ = _layer_fwd(0, t, rows, N, K, training)
            r64 = d["x"] @ d["w"].t() + d["b"]
            fl_r = 2 * K * U32 * (d["x"].abs() @ d["w"].abs().t() + d["b"].abs())
            if training:
                mean, var = r64.mean(0), ((r64 - r64.mean(0)) ** 2).mean(0)
                rm64 = 0.9 * d["rm"] + 0.1 * mean
                rv64 = 0.9 * d["rv"] + 0.1 * var * rows / (rows - 1)
            else:
                mean, var, rm64, rv64 = d["rm"], d["rv"], d["rm"], d["rv"]
            rstd = 1 / torch.sqrt(var + 1e-5)
            a64 = torch.relu((r64 - mean) * rstd * d["gamma"] + d["beta"])
            fl_m = fl_r.mean(0) if training else torch.zeros(N, dtype=torch.float64)
            # d rstd = rstd^3 / 2 d var, |d var| <= 2 sqrt(var) max_rows(fl_r + fl_m): the floor of everything behind rstd
            fl_s = (rstd ** 3 * var.sqrt() * (fl_r.max(0)[0] + fl_m) if training else torch.zeros(N, dtype=torch.float64)) + 4 * U32 * rstd
            tag = "%s %s" % (name, "train" if training else "eval")
            _yardstick(tag + " r", s_["r"], u_["r"], r64, fl_r, report)
            _yardstick(tag + " mean", s_["mr"][:, 0], u_["mr"][:, 0], mean, fl_m + 2 * U32 * mean.abs(), report)
            _yardstick(tag + " rstd", s_["mr"][:, 1], u_["mr"][:, 1], rstd, fl_s, report)
            _yardstick(tag + " a", s_["a"], u_["a"], a64, d["gamma"].abs() * (rstd * (fl_r + fl_m) + (r64 - mean).abs() * fl_s) + 8 * U32 * (a64.abs() + d["beta"].abs()), report)
            _yardstick(tag + " running_mean", s_["rm"], u_["rm"], rm64, 0.1 * fl_m + 4 * U32 * rm64.abs(), report)
            _yardstick(tag + " running_var", s_["rv"], u_["rv"], rv64, 0.2 * var.sqrt() * (fl_r.max(0)[0] + fl_m) * rows / max(rows - 1, 1) + 4 * U32 * rv64.abs(), report)
            assert int(s_["nbt"]) == int(u_["nbt"]) == (1 if training else 0)
            if not training:
                assert torch.equal(s_["rm"], t["rm"]) and torch.equal(s_["rv"], t["rv"])        # eval mode touches no buffer
        # ---- backward: the layer's saved r / (mean, rstd) as operands; a ReLU input within 1e-4 of 0 is moved off the threshold
        r32 = (d["x"] @ d["w"].t() + d["b"]).float()
        mr32 = torch.stack((r32.double().mean(0), 1 / torch.sqrt(r32.double().var(0, unbiased=False) + 1e-5)), 1).float()
        pre = (r32.double() - mr32[:, 0].double()) * mr32[:, 1].double() * d["gamma"] + d["beta"]
        r32 = torch.where(pre.abs() < 1e-4, r32 + (0.01 / (mr32[:, 1].double() * d["gamma"])).float(), r32)
        tb = dict(dy=(rnd(rows, Nn) / rows).to(dev).contiguous(), wn=(rnd(Nn, N) / math.sqrt(N)).to(dev).contiguous(), r=r32.to(dev).contiguous(),
                  mr=mr32.to(dev).contiguous(), gamma=t["gamma"], beta=t["beta"])
        if over:
            with pytest.raises(MMVAEError, match="a workgroup carries"):
                _layer_bwd(1, tb, rows, N, Nn)
            with _strip(1):
                sb = _layer_bwd(-1, tb, rows, N, Nn)
        else:
            sb = _layer_bwd(1, tb, rows, N, Nn)
            sb2 = _layer_bwd(1, tb, rows, N, Nn)
            assert all(torch.equal(sb[k], sb2[k]) for k in sb), name
        ub = _layer_bwd(0, tb, rows, N, Nn)
        db = {k: v.double().cpu() for k, v in tb.items()}
        xh = (db["r"] - db["mr"][:, 0]) * db["mr"][:, 1]
        assert float((xh * db["gamma"] + db["beta"]).abs().min()) >= 5e-5
        da = db["dy"] @ db["wn"]
        fl_d = 2 * Nn * U32 * (db["dy"].abs() @ db["wn"].abs())
        dm = torch.where(xh * db["gamma"] + db["beta"] > 0, da, torch.zeros_like(da))
        s1, s2 = dm.sum(0), (dm * xh).sum(0)
        fl_1 = fl_d.sum(0) + 2 * rows * U32 * dm.abs().sum(0)
        fl_2 = (fl_d * xh.abs()).sum(0) + 2 * rows * U32 * (dm * xh).abs().sum(0)
        gr = (db["gamma"] * db["mr"][:, 1]).abs()
        dr64 = db["gamma"] * db["mr"][:, 1] * (dm - s1 / rows - xh * s2 / rows)
        _yardstick(name + " dbeta", sb["dbeta"], ub["dbeta"], s1, fl_1, report)
        _yardstick(name + " dgamma", sb["dgamma"], ub["dgamma"], s2, fl_2, report)
        _yardstick(name + " d_r", sb["d_r"], ub["d_r"], dr64, gr * (fl_d + (fl_1 + xh.abs() * fl_2) / rows) + 8 * U32 * gr * (dm.abs() + s1.abs() / rows + (xh * s2).abs() / rows), report)
    torch.cuda.synchronize()
    print("strip layers rows=%d, worst strip error / (2 x unfused error + floor): %s" % (rows, "; ".join(report)))


# ====================================================================================================== module face
def _mmvae(D):
    from multimodal_vae_amd import mnist as M
    P = R.formula_params("mnist", D)
    vae = M.MultimodalVAE(D)
    vae.load_state_dict({k: v.detach().clone() for k, v in P.items()}, strict=True)
    return M, vae.cuda().eval()


def _image_vae_of(M, mm, D):
    iv = M.VAE(D)
    sd = {}
    for k, v in mm.state_dict().items():
        if k.startswith("image_"):
            half, _, rest = k[len("image_"):].split(".", 2)          # image_encoder.net.0.weight -> encoder.0.weight
            sd[half + "." + rest] = v.detach().clone()
    iv.load_state_dict(sd, strict=True)
    return iv.cuda().eval()


def test_module_face_equals_the_mmvaes_image_modules():
    D, B = 20, 5
    dev = _dev()
    M, mm = _mmvae(D)
    iv = _image_vae_of(M, mm, D)
    assert [(k, tuple(v.shape)) for k, v in iv.state_dict().items()] == IR.recorded_keys()
    x = IR.inputs(B, D)[0].to(dev)
    with torch.no_grad():
        recon, mu, lv = iv(x.view(B, 1, 28, 28))
        mu1, lv1 = iv.encode(x)
        mu2, lv2 = mm.encode_image(x)
        recon2 = mm.decode_image(mu2.contiguous())
        recon1 = iv.decode(mu1.contiguous())
    assert torch.equal(mu, mu2) and torch.equal(lv, lv2) and torch.equal(recon, recon2)
    assert torch.equal(mu1, mu2) and torch.equal(lv1, lv2) and torch.equal(recon1, recon2)
    assert recon.shape == (B, 784) and mu.shape == (B, D) and torch.equal(iv.reparameterize(mu, lv), mu)
    # the label half's slots of the flat buffers are at their initial value and in no state_dict
    st = iv._core.state
    for n, shape, off in st.table:
        if not n.startswith(IMG):
            assert float(st.params[off:off + _numel(shape)].abs().max()) == 0.0, n
    # training mode through autograd: reparameterize with a given eps, gradients reach both halves
    iv.train()
    recon, mu, lv = iv(x, eps=torch.zeros(B, D, device=dev))
    M.imageonly_loss(recon, x, mu, lv).backward()
    assert all(p.grad is not None for p in iv.parameters())
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        iv(x[:1])


# ====================================================================================================== estimator
@pytest.mark.parametrize("K,per_call", [(5, None), (40, 16)])
def test_estimator_column_x_equals_the_mmvaes(K, per_call):
    """A VAE and a MultimodalVAE with the same image half, the same mu, logvar and eps: column x of log_p, ess and nll is the same
    number bit for bit (mmvae_mnist_iw_score_image is mmvae_mnist_iw_score compiled without the label decoder), y and xy are NaN."""
    from multimodal_vae_amd.evaluate import iw_estimate, log_marginal
    dev = _dev()
    D, B = 20, 3
    M, mm = _mmvae(D)
    iv = _image_vae_of(M, mm, D)
    image, text = R.formula_inputs("mnist", B)
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
    print("mnist K=%d: log p(x) %s" % (K, a["log_p"][:, 0].tolist()))
    r = log_marginal(iv, [(image, None)], n_particles=K, posterior="image", seed=3)
    assert np.isfinite(r["log_px"]) and math.isnan(r["log_py"]) and math.isnan(r["log_pxy"]) and r["n"] == B


# ====================================================================================================== trainer, evaluation, driver
def test_trainer_lowers_the_loss_and_evaluate_matches_float64():
    from multimodal_vae_amd import data as Dt, evaluate as E, mnist as M
    dev = _dev()
    B, D = 32, 20
    img = Dt.synthetic_mnist(B, seed=2)[0].float().div(255.0).view(B, 1, 28, 28)       # the driver's --synthetic data
    torch.manual_seed(0)
    vae = M.VAE(D).cuda()
    tr = M.ImageVAETrainer(vae, B, lr=1e-3)
    x = img.to(dev)
    first = tr(x).losses()[0].item()
    for _ in range(29):
        last = tr(x).losses()[0].item()
    print("mnist ImageVAETrainer: loss %.6f -> %.6f after 30 steps" % (first, last))
    assert np.isfinite(last) and last < 0.95 * first, (first, last)
    sd = vae.state_dict()
    assert int(sd["encoder.1.num_batches_tracked"]) == 30 and int(sd["decoder.4.num_batches_tracked"]) == 30
    ev = E.test_imageonly(vae, [(x, None)], kl_lambda=1.0 / 784, verbose=False)
    ev2 = float(tr.evaluate(x).losses()[0])
    p64 = {IR.plan_name(k): (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in sd.items()}
    with torch.no_grad():
        r64, mu64, lv64 = IR.forward(p64, img, False)
        want = float(IR.loss_function(r64, img, mu64, lv64))
    print("mnist test_imageonly: %.8f, float64 %.8f (rel %.2e)" % (ev, want, abs(ev - want) / want))
    np.testing.assert_allclose(ev, want, rtol=1e-4)
    np.testing.assert_allclose(ev2, want, rtol=1e-4)
    assert int(vae.state_dict()["encoder.1.num_batches_tracked"]) == 30          # eval mode: untouched
    # the reference's own likelihood script on the model (one particle set per batch), against the same sum in float64
    torch.manual_seed(5)
    nll = E.compute_nll_mnist_imageonly(vae, [(x, None)], n_samples=3)
    torch.manual_seed(5)
    smp = torch.randn(3, D).double()
    z = smp.unsqueeze(0) * lv64.mul(0.5).exp().unsqueeze(1) + mu64.unsqueeze(1)
    with torch.no_grad():
        want_nll = sum(float(IR.bce_mean(torch.sigmoid(IR._stack(p64, z[:, i], "image_decoder.net.", False)), img)) * B * 784 for i in range(3)) / 3 / B
    print("mnist compute_nll_mnist_imageonly: %.5f, float64 %.5f" % (nll, want_nll))
    np.testing.assert_allclose(nll, want_nll, rtol=1e-4)


def test_driver_checkpoint_round_trip(tmp_path, capsys):
    from multimodal_vae_amd import data as Dt, evaluate as E, mnist as M, train_imageonly as T
    _dev()
    out, res = str(tmp_path / "models"), str(tmp_path / "results")
    hist = T.main(["--dataset", "mnist", "--cuda", "--epochs", "1", "--synthetic", "256", "--batch_size", "32", "--out", out, "--results", res,
                   "--seed", "3"])
    printed = capsys.readouterr().out
    assert len(hist["train"]) == 1 and all(np.isfinite(hist["train"] + hist["test"])) and hist["kl_lambda"] == [1.0 / 784]
    # the reference's lines (mnist/imageonly/train_imageonly.py:129-133,147)
    assert "Train Epoch: 1 [0/256 (0%)]\tLoss: " in printed and "====> Epoch: 1 Average loss: " in printed and "====> Test set loss: " in printed
    assert "Using KL Lambda" not in printed
    ck_path = os.path.join(out, "checkpoint.pth.tar")
    assert os.path.exists(os.path.join(out, "model_best.pth.tar"))
    ck = torch.load(ck_path, map_location="cpu", weights_only=False)
    assert sorted(ck) == ["best_loss", "n_latents", "optimizer", "state_dict"] and ck["n_latents"] == 20
    assert [(k, tuple(v.shape)) for k, v in ck["state_dict"].items()] == IR.recorded_keys() and ck["best_loss"] == min(hist["test"])
    assert float(ck["optimizer"]["state"][0]["step"]) == 256 // 32 and len(ck["optimizer"]["state"]) == 20
    s = torch.load(os.path.join(res, "sample_image.pt"))             # written on a new best: the first epoch is one
    assert s.shape == (64, 1, 28, 28) and bool(((s >= 0) & (s <= 1)).all())
    assert E.is_imageonly_checkpoint(ck_path) and not E.is_textonly_checkpoint(ck_path)
    vae = M.load_checkpoint_imageonly(ck_path, use_cuda=True)
    assert isinstance(vae, M.VAE)
    for k, v in vae.state_dict().items():
        assert torch.equal(v.cpu(), ck["state_dict"][k]), k
    loss = E.main(["test_imageonly", ck_path, "--dataset", "mnist", "--synthetic", "64", "--batch_size", "32", "--seed", "4"])
    assert np.isfinite(loss) and loss > 0
    # log p(x) alone from the checkpoint, from the file the driver reads
    data = str(tmp_path / "mnist.pt")
    torch.save(Dt.synthetic_mnist(16, seed=9), data)
    table = E.main(["loglik", ck_path, "--dataset", "mnist", "--data", data, "--batch_size", "8", "--n_samples", "4", "--seed", "1"])
    assert list(table) == ["image"] and np.isfinite(table["image"]["log_px"]) and math.isnan(table["image"]["log_py"])
    assert "log p(x) >= " in capsys.readouterr().out
    sdir = str(tmp_path / "samples")
    E.main(["sample", ck_path, "--dataset", "mnist", "--n_samples", "4", "--out", sdir])
    s = torch.load(os.path.join(sdir, "sample_image.pt"))
    assert s.shape == (4, 1, 28, 28) and bool(((s >= 0) & (s <= 1)).all())
    label = int(Dt.synthetic_mnist(16, seed=9)[1][0])
    E.main(["sample", ck_path, "--dataset", "mnist", "--n_samples", "3", "--out", sdir, "--condition_on_image", str(label), "--data", data])
    assert torch.load(os.path.join(sdir, "sample_image.pt")).shape == (3, 1, 28, 28)
    m = E.main(["manifold", ck_path, "--data", data, "--pca_only", "--batch_size", "8", "--out", sdir])
    assert m["latents"].shape == (16, 20) and m["embedding"].shape == (16, 2) and bool(torch.isfinite(m["embedding"]).all())
    with pytest.raises(SystemExit, match="padded-latent"):
        E.main(["latent_viz", ck_path, "--out", sdir])


# ====================================================================================================== refusals
def test_refusals():
    from multimodal_vae_amd import _lib, mnist as M
    from multimodal_vae_amd._ops import stream
    from multimodal_vae_amd.core import FusedImageStep, MnistState
    dev = _dev()
    B, D = 4, 20
    st = _state(D, dev)
    eng = _engine(st, B)
    x = torch.rand(B, 784, device=dev)
    # a wrong image shape, before anything is enqueued
    for shape in ((B, 3, 28, 28), (B, 783), (B + 1, 784)):
        with pytest.raises(M.MMVAEError, match=r"expected images of shape \(4, 1, 28, 28\)"):
            eng.forward_backward(torch.zeros(shape, device=dev))
    # the model has no Dropout: a mask is refused by the host code
    with pytest.raises(M.MMVAEError, match="no Dropout"):
        eng.forward_backward(x, enc_mask1=torch.ones(B, 400, dtype=torch.uint8, device=dev))
    with pytest.raises(M.MMVAEError, match="no Dropout"):
        eng.forward_backward(x, enc_mask2=torch.ones(B, 200, dtype=torch.uint8, device=dev))
    # B = 1 in training: BatchNorm's own message; in eval mode it runs
    e1 = _engine(st, 1)
    with pytest.raises(M.MMVAEError, match="Expected more than 1 value per channel when training"):
        e1.forward_backward(x[:1].contiguous(), True, True)
    assert bool(torch.isfinite(e1.forward_backward(x[:1].contiguous(), False, False).sums).all())
    # a bf16 plan: refused by the engine, and by the C entry point itself
    sb = MnistState(D, dev, precision="bf16")
    with pytest.raises(M.MMVAEError, match="precision 'bf16'"):
        FusedImageStep(sb, B)
    io = _lib.ImageStepIO()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    sums = torch.zeros(16, device=dev)
    io.ws, io.ws_bytes, io.image, io.sums = ws.data_ptr(), ws.numel(), x.data_ptr(), sums.data_ptr()
    with pytest.raises(M.MMVAEError, match="fp32 plan only.*bf16"):
        _lib.call("mmvae_mnist_image_step", sb.plan(B), C.byref(io), 1, 1, stream())
    # a short workspace
    io.ws_bytes = 64
    with pytest.raises(M.MMVAEError, match="workspace too small"):
        _lib.call("mmvae_mnist_image_step", st.plan(B), C.byref(io), 1, 1, stream())
    # n_latents the plan does not take
    with pytest.raises(M.MMVAEError, match="multiple of 4"):
        M.ImageVAETrainer(M.VAE(6).cuda(), B)
    torch.cuda.synchronize()
