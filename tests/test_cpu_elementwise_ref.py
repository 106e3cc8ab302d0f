"""CPU checks of tests/elementwise_ref.py: every reference backward equals float64 autograd, the float32 evaluation of every
reference passes the gates the GPU test uses, and every entry of FAULTS fails one of them -- on the GPU test's own inputs."""
import pytest
import torch
import torch.nn.functional as F

import elementwise_ref as E
from oracle import mmvae_ref as R

F64 = torch.float64


def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ---------------------------------------------------------------------------------------------- backward formulas vs autograd
@pytest.mark.parametrize("M", [1, 2, 3])
def test_poe_bwd_is_autograd(M):
    g = torch.Generator().manual_seed(M)
    mu, lv = torch.randn(M, 37, generator=g, dtype=F64), (22 * torch.rand(M, 37, generator=g, dtype=F64) - 20)
    gm, gl = torch.randn(37, generator=g, dtype=F64), torch.randn(37, generator=g, dtype=F64)
    a, b = mu.clone().requires_grad_(True), lv.clone().requires_grad_(True)
    pm, plv = R.product_of_experts(a, b)
    ((pm * gm).sum() + (plv * gl).sum()).backward()
    dm, dl, _, _ = E.poe_bwd(mu, lv, gm, gl)
    assert _close(dm, a.grad) and _close(dl, b.grad)
    pm2, plv2, _, _ = E.poe(mu, lv)
    assert torch.equal(pm2, pm.detach()) and torch.equal(plv2, plv.detach())


def test_reparam_kl_bwd_are_autograd():
    g = torch.Generator().manual_seed(3)
    mu, lv, eps, dz = (torch.randn(41, generator=g, dtype=F64) for _ in range(4))
    a, b = mu.clone().requires_grad_(True), lv.clone().requires_grad_(True)
    ((R.reparametrize(a, b, True, eps) * dz).sum() + 0.37 * R.kl_sum(a, b)).backward()
    dm, dl, _, _ = E.reparam_bwd(lv, eps, dz)
    km, kl, _, _ = E.kl_bwd(mu, lv, 0.37)
    assert _close(dm + km, a.grad) and _close(dl + kl, b.grad)


@pytest.mark.parametrize("training,use_a,use_b", [(True, True, True), (False, True, False), (True, False, True), (True, False, False)])
def test_latent3_bwd_is_autograd(training, use_a, use_b):
    inp = E.latent3_inputs(*E.L3_BWD_CROSS)
    kc = (E.KL_COEF[0], 0.0, E.KL_COEF[2])
    loss, leaves, f = E.latent3_loss64(inp, kc, training, use_a, use_b)
    loss.backward()
    r = E.latent3_bwd(inp, f["mu"].detach(), f["logvar"].detach(), kc, training, use_a, use_b)
    for n, leaf in (("d_im0", "img0"), ("d_im1", "img1"), ("d_txt", "txt")):
        assert _close(r[n], leaves[leaf].grad, 1e-10), n
        assert bool((r[n + "_mag"] >= r[n].abs() * (1 - 1e-12)).all())


def test_bce_is_torch_and_autograd():
    for (B, C, H, W, ldl) in E.BCE_CASES:
        logits, target = E.bce_inputs(3, B, C, H, W, ldl)
        ordinary = logits.clamp(-8, 8)
        l = ordinary.double().requires_grad_(True)
        p = torch.sigmoid(E._nchw(l, C))
        per = F.binary_cross_entropy(p, target.double().repeat(3, 1, 1, 1), reduction="none").view(3, -1).sum(1)
        (per * torch.tensor(E.BCE_COEF[:3], dtype=F64)).sum().backward()
        r = E.bce(ordinary, target, 3, C, E.BCE_COEF)
        assert _close(r["loss"], per.detach()) and _close(r["dlogit"], E._nchw(l.grad, C), 1e-9)
        # saturated logits: the written-out float32 expression is torch's float32 BCE, clamps included
        r32, t32 = E.bce(logits, target, 3, C, E.BCE_COEF, torch.float32), E.bce_torch32(logits, target, 3, C, E.BCE_COEF)
        assert float((r32["loss"] - t32["loss"]).abs().max()) <= 1e-5 * float(t32["loss"].abs().max())
        assert float((r32["dlogit"] - t32["dlogit"]).abs().max()) <= 1e-6
    big, _ = E.bce_inputs(1, 2, 1, 28, 28, 1)
    for s in E.SATURATED:
        assert int((big == s).sum()) >= 5


def test_nll_is_autograd():
    logits, target = E.nll_inputs(3, 5, 10)
    l = logits.double().requires_grad_(True)
    lp = torch.log_softmax(l, 1)
    tg = target.repeat(3)
    per = torch.stack([F.nll_loss(lp[5 * g:5 * g + 5], tg[5 * g:5 * g + 5], reduction="sum") for g in range(3)])
    (per * torch.tensor(E.NLL_COEF[:3], dtype=F64)).sum().backward()
    r = E.logsoftmax_nll(logits, target, 5, E.NLL_COEF)
    assert _close(r["nll"], per.detach()) and _close(r["dlogits"], l.grad) and _close(r["words"], lp.detach())


@pytest.mark.parametrize("use_db2", [False, True])
def test_bn_is_torch_and_autograd(use_db2):
    inp = E.bn_inputs(10, 16, 3, 5)
    C, G, n = 10, 3, 5
    x = inp["r"][:, :C].double().requires_grad_(True)
    gamma, beta = inp["gamma"].double().requires_grad_(True), inp["beta"].double().requires_grad_(True)
    rm, rv = inp["running_mean"].double().clone(), inp["running_var"].double().clone()
    ys = []
    for g in range(G):
        for u in range(2 if g != 1 else 0):          # skip mask 0b010, two calls per group
            y = F.batch_norm(x[g * n:(g + 1) * n], rm, rv, gamma, beta, True, E.BN_MOM, E.BN_EPS)
        ys.append(F.batch_norm(x[g * n:(g + 1) * n], None, None, gamma, beta, True, E.BN_MOM, E.BN_EPS))
    y = torch.cat(ys)
    d = inp["db"][:, :C].double() + (inp["db2"][:, :C].double() if use_db2 else 0.0)
    (y * d).sum().backward()
    t = E.bn_tables(inp, updates=2, skip_mask=0b010)
    assert _close(t["running_mean"], rm) and _close(t["running_var"], rv) and t["nbt"] == 4
    assert float(t["var"][:, 0].abs().max()) == 0.0                                       # the constant channel
    assert float((t["mean"][:, C - 1].abs() / t["var"][:, C - 1].sqrt()).min()) > 4.0     # the |mean| >> std channel
    a, _ = E.bn_act(inp, 0)
    assert _close(a, y.detach())
    b = E.bn_bwd(inp, use_db2)
    assert _close(b["dr"], x.grad, 1e-9) and _close(b["dgamma"], gamma.grad, 1e-9) and _close(b["dbeta"], beta.grad)
    # the slot tables fold to the sums they stand for
    st = E.bn_stats(inp).double().sum(1)
    assert _close(st[..., 0] / n, t["mean"], 1e-6)
    assert int((E.bn_stats(inp)[0, :, 1, 0] == 0).sum()) >= 1          # some slots stay empty
    red = E.bn_red(inp, use_db2).double().sum((0, 1))
    assert _close(red[:, 0], b["dbeta"], 1e-6) and _close(red[:, 1], b["dgamma"], 1e-5)


def test_standalone_loss_refs_are_autograd():
    g = torch.Generator().manual_seed(11)
    p, t = torch.rand(257, generator=g, dtype=F64).clamp(1e-3, 1 - 1e-3), torch.rand(257, generator=g, dtype=F64)
    a = p.clone().requires_grad_(True)
    F.binary_cross_entropy(a, t, reduction="sum").backward()
    s, _, _, dp, _ = E.bce_probs(p, t)
    assert _close(dp, a.grad, 1e-10) and abs(float(s) - float(F.binary_cross_entropy(p, t, reduction="sum"))) < 1e-9
    a, b = torch.randn(257, generator=g, dtype=F64), torch.randn(257, generator=g, dtype=F64)
    x = a.clone().requires_grad_(True)
    F.mse_loss(x, b, reduction="sum").backward()
    assert _close(E.mse(a, b)[3], x.grad)


# ---------------------------------------------------------------------------------------------- faults vs the GPU test's gates
def test_every_fault_is_placed():
    assert set(sum(E.FAULTS_OF.values(), ())) == set(E.FAULTS)


@pytest.mark.parametrize("B,D", [E.L3_BWD_CROSS, (1, 1), (3, 4)])
def test_latent3_fwd_gate_notices(B, D):
    inp, ldz = E.latent3_inputs(B, D), E.ldz_of(D)
    for training in (True, False):
        assert not E.violations(E.gate_latent3_fwd(E.emulate_latent3_fwd(inp, ldz, training), inp, ldz, training))
    for fault in E.FAULTS_OF["latent3_fwd"]:
        bad = E.violations(E.gate_latent3_fwd(E.emulate_latent3_fwd(inp, ldz, True, fault), inp, ldz, True))
        assert bad, fault
    # a one-expert pass is NOT its input: the reference decides
    f = E.latent3_fwd(inp)
    assert float((f["logvar"][1] - inp["img1"][:, D:].double()).abs().max()) > 1.0


@pytest.mark.parametrize("form", E.IMG_FORMS)
def test_latent3_bwd_gate_notices(form):
    B, D = E.L3_BWD_CROSS
    inp = E.latent3_inputs(B, D)
    mu, lv = E.fwd_mu_logvar32(inp)
    args = (inp, mu, lv, E.KL_COEF, form)
    assert not E.violations(E.gate_latent3_bwd(E.emulate_latent3_bwd(*args), *args))
    for fault in E.FAULTS_OF["latent3_bwd"]:
        if fault == "pad_nonzero" and form != "bf16_two_padded":
            continue
        assert E.violations(E.gate_latent3_bwd(E.emulate_latent3_bwd(*args, fault=fault), *args)), fault


@pytest.mark.parametrize("case", E.BCE_CASES[:2])
def test_bce_gate_notices(case):
    B, C, H, W, ldl = case
    logits, target = E.bce_inputs(3, B, C, H, W, ldl)
    args = (logits, target, 3, C, E.BCE_COEF)
    assert not E.violations(E.gate_bce(E.emulate_bce(*args), *args))
    assert not E.violations(E.gate_bce(E.bce_torch32(*args), *args))
    assert E.violations(E.gate_bce(E.emulate_bce(*args, fault="no_bce_clamp"), *args))


def test_nll_gate_notices():
    for classes in E.NLL_CLASSES[1:]:
        logits, target = E.nll_inputs(3, 37, classes)
        ld_d = (classes + 7) // 8 * 8 + 8
        assert not E.violations(E.gate_nll(E.emulate_nll(logits, target, 37, E.NLL_COEF, ld_d), logits, target, 37, E.NLL_COEF))
        for fault in E.FAULTS_OF["nll"]:
            assert E.violations(E.gate_nll(E.emulate_nll(logits, target, 37, E.NLL_COEF, ld_d, fault), logits, target, 37, E.NLL_COEF)), fault


def test_bn_gate_notices():
    inp = E.bn_inputs(10, 16, 3, 5)
    kw = dict(training=True, updates=2, skip_mask=0b010)
    assert not E.violations(E.gate_bn_tables(E.emulate_bn_finalize(inp, **kw), inp, **kw))
    for fault in ("biased_running_var", "skip_mask_ignored", "updates_once"):
        assert E.violations(E.gate_bn_tables(E.emulate_bn_finalize(inp, fault=fault, **kw), inp, **kw)), fault
    a, _ = E.bn_act(inp, 1, dtype=torch.float32)
    buf = torch.zeros(15, 16, dtype=torch.bfloat16)
    buf[:, :10] = a.to(torch.bfloat16)
    assert not E.violations(E.gate_bn_act(buf, inp, 1))
    buf[14, 15] = 2.0 ** -20                                           # "pad_nonzero"
    assert E.violations(E.gate_bn_act(buf, inp, 1))
    b = E.bn_bwd(inp, True, torch.float32)
    dr = torch.zeros(15, 16, dtype=torch.bfloat16)
    dr[:, :10] = b["dr"].to(torch.bfloat16)
    assert not E.violations(E.gate_bn_bwd(dict(dr=dr, dgamma=b["dgamma"], dbeta=b["dbeta"]), inp, True))
    assert E.violations(E.gate_bn_bwd(dict(dr=dr, dgamma=b["dgamma"], dbeta=b["dbeta"]), inp, False))
