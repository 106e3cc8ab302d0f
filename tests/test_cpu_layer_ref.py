"""CPU companion of tests/test_gpu_layers.py and tests/test_gpu_celeba_layers.py: the float64 layer reference (tests/layer_ref.py) the GPU test trusts is tied to the
model definition in oracle/mmvae_ref.py, and its operand generator stays inside the regime where bf16 operands with fp32
accumulation reproduce float64 bit for bit."""
import pytest
import torch
import torch.nn.functional as F

import layer_ref as LR
from oracle import mmvae_ref as R

BMAX = max(LR.BATCHES)


@pytest.mark.parametrize("name", list(LR.LAYERS))
def test_operands_stay_in_the_exact_regime(name):
    """largest batch of the matrix: forward on gf * B images, both gradients on gb * B images"""
    L = LR.LAYERS[name]
    ws, xs = [], []
    for seed in LR.SEEDS:
        x, w, _ = LR.layer_operands(name, L.gf * BMAX, seed)
        out = LR.ref_forward(L, x, w)
        LR.assert_exact_regime(out=out, groups=L.gf, what="%s forward seed %d" % (name, seed))
        assert float(out.abs().max()) > 0
        xb, wb, dy = LR.layer_operands(name, L.gb * BMAX, seed)
        LR.assert_exact_regime(dw=LR.ref_wgrad(L, xb, dy), what="%s wgrad seed %d" % (name, seed))
        acc = LR.ref_dgrad_acc(L, dy, wb)
        assert bool((acc == acc.round()).all()) and float(acc.abs().max()) <= 256, (name, float(acc.abs().max()))
        ws.append(w)
        xs.append(x)
    LR.assert_operand_coverage(ws, xs)


class _Recorder:
    """stands in for torch.nn.functional inside the oracle module: records every conv / transposed conv call"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return getattr(F, name)

    def _rec(self, fn, transposed, x, w, b, stride, pad):
        x.retain_grad()
        out = fn(x, w, b, stride, pad)
        out.retain_grad()
        self.calls.append(dict(transposed=transposed, x=x, w=w, out=out, stride=stride, pad=pad))
        return out

    def conv2d(self, x, w, b, stride, pad):
        return self._rec(F.conv2d, False, x, w, b, stride, pad)

    def conv_transpose2d(self, x, w, b, stride, pad):
        return self._rec(F.conv_transpose2d, True, x, w, b, stride, pad)


def test_reference_agrees_with_autograd_on_the_oracle_modules(monkeypatch):
    """every conv of oracle.mmvae_ref's MultiMNIST image encoder / decoder, run in float64 with autograd: the layer table's
    geometry (kernel, stride, padding, transposed, sizes, parameter name) reproduces the module's output, weight gradient and
    input gradient from the recorded operands"""
    torch.manual_seed(0)
    B = 3
    P = {k: (v.double().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.double() if v.is_floating_point() else v)
         for k, v in R.formula_params("multimnist", 100).items()}
    rec = _Recorder()
    monkeypatch.setattr(R, "F", rec)
    image = torch.rand(B, 1, 50, 50, dtype=torch.float64).requires_grad_(True)
    z = torch.randn(B, 100, dtype=torch.float64)
    enc = R.multimnist_image_encoder(P, image * 1.0, True, None, drop_p=0.0)
    dec = R.multimnist_image_decoder_logits(P, z, True)
    ((enc * torch.randn_like(enc)).sum() + (dec * torch.randn_like(dec)).sum()).backward()
    monkeypatch.undo()
    assert len(rec.calls) == 8
    by_weight = {id(c["w"]): c for c in rec.calls}
    for name, L in LR.LAYERS.items():
        c = by_weight[id(P[L.param])]
        assert c["transposed"] == L.transposed and c["stride"] == L.stride and c["pad"] == L.pad, name
        assert tuple(c["w"].shape) == LR.weight_shape(L), name
        x, dy = LR._nhwc(c["x"].detach()), LR._nhwc(c["out"].grad)
        assert tuple(x.shape) == (B, L.ih, L.ih, L.cin) and tuple(dy.shape) == (B, L.oh, L.oh, L.cout), name
        w = c["w"].detach()
        torch.testing.assert_close(LR.ref_forward(L, x, w), LR._nhwc(c["out"].detach()), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(LR.ref_wgrad(L, x, dy), c["w"].grad, rtol=1e-10, atol=1e-12)
        torch.testing.assert_close(LR.ref_dgrad_acc(L, dy, w), LR._nhwc(c["x"].grad), rtol=1e-10, atol=1e-12)


def test_epilogue_reference_is_swish_batchnorm_backward():
    """ref_dgrad_epilogue == autograd of Swish(scale * r + shift) times the incoming gradient, and its sums are the two reductions
    of the BatchNorm backward: sum dy_bn and sum dy_bn * xhat"""
    g = LR.gen(5, 1)
    groups, n, C = 2, 4, 8
    acc = LR.ternary((groups * n, 3, 3, C), 0.7, g) * torch.randint(1, 40, (groups * n, 3, 3, C), generator=g)
    r = LR.eighths((groups * n, 3, 3, C), g)
    aff, mr = LR.dyadic_tables(groups, C, g)
    v, red, red_abs = LR.ref_dgrad_epilogue(acc, r, aff, mr, groups)
    rr = r.clone().reshape(groups, -1, C).requires_grad_(True)
    pre = rr * aff[:, None, :, 0] + aff[:, None, :, 1]
    y = pre * torch.sigmoid(pre)
    # d/d(pre) of sum(acc * Swish(pre)): the gradient w.r.t. the BatchNorm output
    (gpre,) = torch.autograd.grad((y * acc.reshape(groups, -1, C)).sum(), pre)
    torch.testing.assert_close(v.reshape(groups, -1, C), gpre, rtol=1e-13, atol=1e-13)
    xhat = (rr.detach() - mr[:, None, :, 0]) * mr[:, None, :, 1]
    torch.testing.assert_close(red[..., 0], gpre.sum(1), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(red[..., 1], (gpre * xhat).sum(1), rtol=1e-13, atol=1e-13)
    assert bool((red_abs >= red.abs() - 1e-12).all())
    # no tables: plain Swish'(r), no sums
    v0, red0, _ = LR.ref_dgrad_epilogue(acc, r, None, None, groups)
    r0 = r.clone().requires_grad_(True)
    (g0,) = torch.autograd.grad((r0 * torch.sigmoid(r0) * acc).sum(), r0)
    torch.testing.assert_close(v0, g0, rtol=1e-13, atol=1e-13)
    assert red0 is None


def test_epilogue_inputs_are_exact_in_their_formats():
    g = LR.gen(6, 2)
    r = LR.eighths((1000,), g)
    assert torch.equal(r.to(torch.bfloat16).double(), r) and float(r.abs().max()) <= 4
    aff, mr = LR.dyadic_tables(3, 64, g)
    for t in (aff, mr):
        assert torch.equal(t.float().double(), t)
    pre32 = r.float()[:, None, None] * aff[..., 0].float() + aff[..., 1].float()
    assert torch.equal(pre32.double(), r[:, None, None] * aff[..., 0] + aff[..., 1])
    xh32 = (r.float()[:, None, None] - mr[..., 0].float()) * mr[..., 1].float()
    assert torch.equal(xh32.double(), (r[:, None, None] - mr[..., 0]) * mr[..., 1])


# ------------------------------------------------------------------------------------------------ CelebA
def _celeba_cases():
    """every (batch, seed) tests/test_gpu_celeba_layers.py uses: both seeds at the small batches, the first at the large one"""
    return [(B, seed) for B in LR.BATCHES_CELEBA for seed in (LR.SEEDS if B <= 8 else LR.SEEDS[:1])]


@pytest.mark.parametrize("name", list(LR.LAYERS_CELEBA))
def test_celeba_operands_stay_in_the_exact_regime(name):
    """forward on gf * B images, both gradients on gb * B images, for every (batch, seed) of the GPU module"""
    L = LR.LAYERS_CELEBA[name]
    for B, seed in _celeba_cases():
        x, w, dy = LR.layer_operands(name, L.gf * B, seed, LR.LAYERS_CELEBA)
        assert L.gf == L.gb
        out = LR.ref_forward(L, x, w)
        LR.assert_exact_regime(out=out, groups=L.gf, what="%s forward B=%d seed %d" % (name, B, seed))
        assert float(out.abs().max()) > 0
        LR.assert_exact_regime(dw=LR.ref_wgrad(L, x, dy), what="%s wgrad B=%d seed %d" % (name, B, seed))
        acc = LR.ref_dgrad_acc(L, dy, w)
        assert bool((acc == acc.round()).all()) and float(acc.abs().max()) <= 256, (name, B, seed, float(acc.abs().max()))
    ws, xs = zip(*[LR.layer_operands(name, L.gf * 8, seed, LR.LAYERS_CELEBA)[1::-1] for seed in LR.SEEDS])
    LR.assert_operand_coverage(list(ws), list(xs))


def test_celeba_reference_agrees_with_autograd_on_the_oracle_modules(monkeypatch):
    """every conv of oracle.mmvae_ref's CelebA image encoder / decoder in float64 with autograd: LAYERS_CELEBA's geometry
    reproduces the module's output, weight gradient and input gradient from the recorded operands"""
    torch.manual_seed(0)
    B = 2
    P = {k: (v.double().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.double() if v.is_floating_point() else v)
         for k, v in R.formula_params("celeba", 100).items()}
    rec = _Recorder()
    monkeypatch.setattr(R, "F", rec)
    image = torch.rand(B, 3, 64, 64, dtype=torch.float64).requires_grad_(True)
    z = torch.randn(B, 100, dtype=torch.float64)
    enc = R.celeba_image_encoder(P, image * 1.0, True, None, drop_p=0.0)
    dec = R.celeba_image_decoder(P, z, True)
    ((enc * torch.randn_like(enc)).sum() + (dec * torch.randn_like(dec)).sum()).backward()
    monkeypatch.undo()
    assert len(rec.calls) == 8
    by_weight = {id(c["w"]): c for c in rec.calls}
    for name, L in LR.LAYERS_CELEBA.items():
        c = by_weight[id(P[L.param])]
        assert c["transposed"] == L.transposed and c["stride"] == L.stride and c["pad"] == L.pad, name
        assert tuple(c["w"].shape) == LR.weight_shape(L), name
        x, dy = LR._nhwc(c["x"].detach()), LR._nhwc(c["out"].grad)
        assert tuple(x.shape) == (B, L.ih, L.ih, L.cin) and tuple(dy.shape) == (B, L.oh, L.oh, L.cout), name
        w = c["w"].detach()
        torch.testing.assert_close(LR.ref_forward(L, x, w), LR._nhwc(c["out"].detach()), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(LR.ref_wgrad(L, x, dy), c["w"].grad, rtol=1e-10, atol=1e-12)
        torch.testing.assert_close(LR.ref_dgrad_acc(L, dy, w), LR._nhwc(c["x"].grad), rtol=1e-10, atol=1e-12)


# ------------------------------------------------------------------------------------------------ sensitivity of the gates
class _SimHarness:
    """Stands in for LR.LayerHarness without a GPU: a 'kernel' that is the float64 reference itself, stored the way the engine
    stores (bf16 results, fp32 sums in slot 0 of the table), optionally with one injected fault:
      "tap"   : the engine ignores tap (ky, kx) = (1, 2) of the weights
      "image" : the engine drops the middle image of the launch (its operand reads as zero)
      "tile"  : 16 result columns (channels 16..31) land shifted by one channel
    LR.check_forward / check_wgrad / check_dgrad run against it unchanged: they must pass without a fault and fail with each."""

    class _Gpk:
        def __init__(self, sim):
            self.sim = sim

        def zero_(self):
            self.sim.grads = {}

    class _St:
        pass

    def __init__(self, layers, fault=None):
        self.layers, self.fault = layers, fault
        self.bufs, self.weights, self.grads = {}, {}, {}
        self.st = self._St()
        self.st.gpk = self._Gpk(self)

    def set_weight(self, pname, w):
        self.weights[pname] = w.double().clone()

    def put(self, name, t, dtype=torch.bfloat16):
        src = t.to(dtype)
        assert torch.equal(src.double(), t.double()), name
        self.bufs[name] = src.reshape(-1).clone()

    def zero(self, name, numel, dtype):
        self.bufs[name] = torch.zeros(numel, dtype=dtype)

    def get(self, name, shape, dtype=torch.bfloat16):
        n = 1
        for s in shape:
            n *= s
        assert self.bufs[name].dtype == dtype
        return self.bufs[name][:n].clone().reshape(shape)

    def stats(self, name, groups, C):
        return self.bufs[name].reshape(groups, LR.STAT_SLOTS, C, 2).double().sum(1)

    def packed_grad(self, pname, also=()):
        others = [v.abs().max() for n, v in self.grads.items() if n != pname and n not in also]
        return self.grads[pname].clone(), float(max(others)) if others else 0.0

    def set_knobs(self, **kn):
        pass

    def restore_knobs(self):
        pass

    def _operand(self, name, L, pix, ch):
        t = self.bufs[name].double()
        return t.reshape(-1, pix, pix, ch)

    def _table(self, name, sums):
        """[groups][C][2] sums into slot 0 of a zeroed [groups][STAT_SLOTS][C] float2 table"""
        t = torch.zeros(sums.shape[0], LR.STAT_SLOTS, sums.shape[1], 2, dtype=torch.float32)
        t[:, 0] = sums.float()
        self.bufs[name] = t.reshape(-1)

    def _shift(self, t, dim):
        if self.fault == "tile":
            idx = [slice(None)] * t.dim()
            idx[dim] = slice(16, 32)
            t = t.clone()
            t[tuple(idx)] = torch.roll(t[tuple(idx)], 1, dim)
        return t

    def run(self, layer, **knobs):
        base = layer.rsplit("_", 1)[0] if layer.endswith(("_dgrad", "_wgrad")) else layer
        L = self.layers[base]
        w = self.weights.get(L.param)
        if w is not None and self.fault == "tap":
            w = w.clone()
            w[:, :, 1, 2] = 0
        drop = self.fault == "image"
        if layer == base:
            x = self._operand(L.x, L, L.ih, L.cin).clone()
            if drop:
                x[x.shape[0] // 2] = 0
            out = self._shift(LR.ref_forward(L, x, w), 3)
            self.bufs[L.out] = out.to(torch.bfloat16).reshape(-1)
            self._table(L.stats, LR.ref_colstats(out, L.gf))
        elif layer.endswith("_wgrad"):
            x, dy = self._operand(L.x, L, L.ih, L.cin).clone(), self._operand(L.dy, L, L.oh, L.cout)
            if drop:
                x[x.shape[0] // 2] = 0
            dw = LR.ref_wgrad(L, x, dy)
            if self.fault == "tap":
                dw[:, :, 1, 2] = 0
            self.grads[L.param] = self._shift(dw, 1 if L.transposed else 0)
        else:
            dy = self._operand(L.dy, L, L.oh, L.cout).clone()
            if drop:
                dy[dy.shape[0] // 2] = 0
            acc = self._shift(LR.ref_dgrad_acc(L, dy, w), 3)
            r = self._operand(L.r, L, L.ih, L.cin)
            aff = self.bufs[L.aff].double().reshape(L.gb, L.cin, 2) if L.aff else None
            mr = self.bufs[L.mr].double().reshape(L.gb, L.cin, 2) if L.mr else None
            v, red, _ = LR.ref_dgrad_epilogue(acc, r, aff, mr, L.gb)
            self.bufs[L.dx] = v.to(torch.bfloat16).reshape(-1)
            if L.red:
                self._table(L.red, red)
        return [("sim", layer)]


FAULTS = ("tap", "image", "tile")
_FAMILIES = {"multimnist": LR.LAYERS, "celeba": LR.LAYERS_CELEBA}


def _run_checks(h, layers, name, B, seed=0):
    """the three comparisons of the GPU modules on one layer; returns which of them raised"""
    L = layers[name]
    x, w, dy = LR.layer_operands(name, L.gf * B, seed, layers)
    failed = set()
    try:
        LR.check_forward(h, L, name, x, w, ({},), name)
    except AssertionError:
        failed.add("forward")
    xb, wb, dyb = LR.layer_operands(name, L.gb * B, seed, layers)
    h.put(L.x, xb)
    h.put(L.dy, dyb)
    try:
        LR.check_wgrad(h, name + "_wgrad", L.param, LR.ref_wgrad(L, xb, dyb), ({},), name)
    except AssertionError:
        failed.add("wgrad")
    try:
        LR.check_dgrad(h, L, name, dyb, wb, LR.gen(seed, 4, 4), ({},), name)
    except AssertionError:
        failed.add("dgrad")
    return failed


@pytest.mark.parametrize("family", sorted(_FAMILIES))
def test_checks_pass_on_the_reference_and_see_every_fault(family):
    """The Tier A and Tier B gates are tight enough for the faults the whole-step tests cannot see (a dropped
    image, tap or column tile moves a gradient tensor by 1/B to 1/(3B) of its norm): on every layer the three comparisons pass on
    a fault-free stand-in for the engine and every one of them fails with each fault injected."""
    layers = _FAMILIES[family]
    for name in layers:
        assert _run_checks(_SimHarness(layers), layers, name, 4) == set(), name
        for fault in FAULTS:
            assert _run_checks(_SimHarness(layers, fault), layers, name, 4) == {"forward", "wgrad", "dgrad"}, (name, fault)


@pytest.mark.parametrize("fault", FAULTS)
def test_sum_gates_see_every_fault(fault):
    """The 2^-16 gate of the BatchNorm-backward sums alone (check_dgrad stops at the per-element gate first), on the data gradient of
    every CelebA layer geometry (with tables, whether or not the step's layer has a BatchNorm below it): the sums of a faulty
    launch fall outside, those of the reference inside."""
    layers = LR.LAYERS_CELEBA
    for name, L in layers.items():
        _, w, dy = LR.layer_operands(name, L.gb * 4, 0, layers)
        g = LR.gen(0, 4, 4)
        r = LR.eighths((L.gb * 4, L.ih, L.ih, L.cin), g)
        aff, mr = LR.dyadic_tables(L.gb, L.cin, g)
        _, red, red_abs = LR.ref_dgrad_epilogue(LR.ref_dgrad_acc(L, dy, w), r, aff, mr, L.gb)
        sim = _SimHarness(layers, fault)
        sim.set_weight(L.param, w)
        sim.put(L.dy, dy)
        sim.put(L.r, r)
        sim.bufs["aff"], sim.bufs["mr"] = aff.reshape(-1), mr.reshape(-1)
        Lt = L._replace(aff="aff", mr="mr", red="red")
        sim.layers = {name: Lt}
        sim.run(name + "_dgrad")
        LR.gate_sums(red, red, red_abs, name)
        with pytest.raises(AssertionError):
            LR.gate_sums(sim.stats("red", L.gb, L.cin), red, red_abs, name)


# ------------------------------------------------------------------------------------------------ staged forms
def _faulty_forward(L, x, w, fault):
    """the float64 forward with one of FAULTS injected (as _SimHarness.run)"""
    x, w = x.clone(), w.clone()
    if fault == "tap":
        w[:, :, 1, 2] = 0
    if fault == "image":
        x[x.shape[0] // 2] = 0
    out = LR.ref_forward(L, x, w)
    if fault == "tile":
        out[..., 16:32] = torch.roll(out[..., 16:32], 1, -1)
    return out


@pytest.mark.parametrize("name", ["enc_conv3", "dec_convT2", "dec_convT3"])
def test_staged_forward_reference_and_gates(name):
    """Kind 1 on the CPU: the tables of ref_bn_tables are torch's batch_norm (training) on a hand-checkable case, the by-product is
    Swish of it, the written statistics are exact in fp32 at the largest batch, and the output / column-statistics gates of the
    staged conv see a dropped tap, a dropped image and a shifted column tile on every staged layer."""
    L = LR.LAYERS_CELEBA[name]
    G, B = L.gf, 4
    g = LR.gen(0, 7, B)
    r = LR.eighths((G * B, L.ih, L.ih, L.cin), g)
    gamma = torch.tensor([1.0, 2.0, -1.0])[torch.randint(0, 3, (L.cin,), generator=g)].double()
    beta = torch.randint(-1, 2, (L.cin,), generator=g).double()
    stats = LR.slot_stats(r, G)
    assert torch.equal(stats.float().double(), stats)
    scale, shift, mean, rstd = LR.ref_bn_tables(stats, B * L.ih * L.ih, gamma, beta)
    a, y = LR.ref_stage_fwd(r, scale, shift, G)
    for k in range(G):
        rk = LR._nchw(r[k * B:(k + 1) * B])
        want = F.batch_norm(rk, None, None, gamma, beta, True, 0.1, LR.BN_EPS)
        torch.testing.assert_close(LR._nchw(y[k * B:(k + 1) * B]), want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(a, y * torch.sigmoid(y), rtol=0, atol=0)
    # one image, one channel, by hand: r = (1, -1) -> mean 0, var 1, y = gamma * r / sqrt(1 + eps) + beta
    st1 = torch.zeros(1, LR.STAT_SLOTS, 1, 2, dtype=torch.float64)
    st1[0, 0, 0] = torch.tensor([0.0, 2.0])
    s1, sh1, m1, rs1 = LR.ref_bn_tables(st1, 2, torch.tensor([2.0]), torch.tensor([1.0]))
    assert float(m1) == 0.0 and abs(float(rs1) - (1 + LR.BN_EPS) ** -0.5) < 1e-15 and float(s1) == 2 * float(rs1) and float(sh1) == 1.0
    # the largest batch: every slot entry of the statistics is exact in fp32
    big = LR.slot_stats(LR.eighths((G * 256, L.ih, L.ih, 8), g), G)
    assert torch.equal(big.float().double(), big)
    # (b) gates against faults, on the bf16 values a launch would leave behind
    a_rb = a.to(torch.bfloat16).double()
    w = LR.ternary(LR.weight_shape(L), LR.W_DENSITY, g)
    ref, absterms = LR.ref_forward(L, a_rb, w), LR.ref_abs_terms(L, a_rb, w)
    gate, sgate = LR.gate_stage_conv(L, ref, absterms), LR.gate_stage_colstats(L, ref, absterms, G)
    assert bool(((ref.to(torch.bfloat16).double() - ref).abs() <= gate).all())
    for fault in FAULTS:
        bad = _faulty_forward(L, a_rb, w, fault)
        assert bool(((bad - ref).abs() > gate).any()), (name, fault)
        assert bool(((LR.ref_colstats(bad, G) - LR.ref_colstats(ref, G)).abs() > sgate).any()), (name, fault)


@pytest.mark.parametrize("name", ["enc_conv2", "enc_conv3", "dec_convT2", "dec_convT3"])
def test_staged_backward_reference_and_gates(name):
    """Kind 2 on the CPU: ref_bn_backward is autograd's BatchNorm backward when the sums are the true ones; the operands of
    staged_bwd_operands keep dr on the grid fp32 holds exactly, at the smallest and the largest batch; the data gradient of the
    stored dr stays an exact fp32 accumulation and its gate sees every fault."""
    L = LR.LAYERS_CELEBA[name]
    G = L.gb
    # autograd: y = gamma * xhat + beta per group, loss = sum(y * db)
    g = LR.gen(1, 8)
    n, C = 2, L.cout
    db = LR.ternary((G * n, 3, 3, C), 0.7, g)
    r = LR.eighths((G * n, 3, 3, C), g).requires_grad_(True)
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    rr = r.reshape(G, -1, C)
    mean, var = rr.mean(1), rr.var(1, unbiased=False)
    rstd = 1 / torch.sqrt(var + LR.BN_EPS)
    xhat = (rr - mean[:, None]) * rstd[:, None]
    (xhat * gamma * db.reshape(G, -1, C)).sum().backward()
    d = db.reshape(G, -1, C)
    red = torch.zeros(G, LR.STAT_SLOTS, C, 2, dtype=torch.float64)
    red[:, 0] = torch.stack([d.sum(1), (d * xhat.detach()).sum(1)], -1)
    dr, dgamma, dbeta, _, _ = LR.ref_bn_backward(db, r.detach(), red, torch.stack([mean, rstd], -1).detach(), gamma, n * 9, G)
    torch.testing.assert_close(dr, r.grad, rtol=1e-9, atol=1e-11)
    torch.testing.assert_close(dgamma, (d * xhat.detach()).sum((0, 1)), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dbeta, d.sum((0, 1)), rtol=1e-12, atol=1e-12)
    # the GPU module's operands
    for B in (4, 256):
        if B == 256 and name != "enc_conv3":
            continue                # (one layer at the large batch: the grid argument does not depend on the geometry)
        gg = LR.gen(0, list(LR.LAYERS_CELEBA).index(name), 6, G * B)
        w = LR.ternary(LR.weight_shape(L), LR.W_DENSITY, gg)
        count = B * L.oh * L.oh
        db, r, red, mr, gamma = LR.staged_bwd_operands(L, G * B, G, count, gg)
        for t in (red, mr):
            assert torch.equal(t.float().double(), t)
        dr, _, _, _, _ = LR.ref_bn_backward(db, r, red, mr, gamma, count, G)
        assert bool((dr * 128 == (dr * 128).round()).all()) and float(dr.abs().max()) < 64
        dr_rb = dr.to(torch.bfloat16).double()
        assert bool(((dr_rb - dr).abs() <= 2.0 ** -8 * dr.abs()).all())
        acc = LR.ref_dgrad_acc(L, dr_rb, w)
        assert bool((acc * 256 == (acc * 256).round()).all()) and float(acc.abs().max()) * 256 < 2 ** 24
        if B > 4:
            continue
        r_in = LR.eighths(acc.shape, gg)
        aff, mri = LR.dyadic_tables(G, L.cin, gg)
        v, red_in, red_abs = LR.ref_dgrad_epilogue(acc, r_in, aff, mri, G)
        LR.gate_elements(v.to(torch.bfloat16), v, acc, name)
        for fault in FAULTS:
            wf, dyf = w.clone(), dr_rb.clone()
            if fault == "tap":
                wf[:, :, 1, 2] = 0
            if fault == "image":
                dyf[dyf.shape[0] // 2] = 0
            accf = LR.ref_dgrad_acc(L, dyf, wf)
            if fault == "tile":
                accf[..., 16:32] = torch.roll(accf[..., 16:32], 1, -1)
            vf, redf, _ = LR.ref_dgrad_epilogue(accf, r_in, aff, mri, G)
            with pytest.raises(AssertionError):
                LR.gate_elements(vf.to(torch.bfloat16), v, acc, name)
            with pytest.raises(AssertionError):
                LR.gate_sums(redf, red_in, red_abs, name)


def test_bn_backward_reference_by_hand():
    """one image, one channel, four pixels r = (1, -1, 1, -1) with mean 0, rstd 1, gamma 2 and db = (1, 0, 0, 0): the sums are
    sum db = 1 and sum db xhat = 1, so m1 = m2 = 1/4 and dr = 2 (db - 1/4 - xhat / 4) = (1, 0, -1, 0); dgamma = dbeta = 1"""
    r = torch.tensor([1.0, -1.0, 1.0, -1.0], dtype=torch.float64).reshape(1, 2, 2, 1)
    db = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64).reshape(1, 2, 2, 1)
    red = torch.zeros(1, LR.STAT_SLOTS, 1, 2, dtype=torch.float64)
    red[0, 3, 0] = torch.tensor([1.0, 1.0])
    mr = torch.tensor([[[0.0, 1.0]]], dtype=torch.float64)
    dr, dgamma, dbeta, mag_g, mag_b = LR.ref_bn_backward(db, r, red, mr, torch.tensor([2.0]), 4, 1)
    assert dr.reshape(-1).tolist() == [1.0, 0.0, -1.0, 0.0]
    assert dgamma.tolist() == [1.0] and dbeta.tolist() == [1.0] and mag_g.tolist() == [1.0] and mag_b.tolist() == [1.0]


@pytest.mark.parametrize("fault", ["column", "row", "tile"])
def test_dense_gates_see_every_fault(fault):
    """The comparisons tests/test_gpu_celeba_layers.py makes on classifier.0, classifier.3's data gradient and upsample.0, at its
    densities and B = 4, against the float64 reference with one input column ignored (the dense layers' 'tap'), one row (image)
    dropped or one tile of 16 output columns shifted: the exact comparison, the per-element gate and the 2^-16 gate of the column
    sums all fail; on the unharmed reference they pass."""
    B, D, HID, FEAT = 4, 100, 1024, 6400
    g = LR.gen(0, 13, B)
    tern = lambda shape, d: LR.ternary(shape, d, g)

    def linear(x, W, b=None):
        x, W = x.clone(), W.clone()
        if fault == "column":
            W[:, int(torch.nonzero(x.abs().sum(0))[0])] = 0        # (the first input column some row of this batch uses)
        if fault == "row":
            x[x.shape[0] // 2] = 0
        y = F.linear(x, W, b)
        if fault == "tile":
            y[:, 16:32] = torch.roll(y[:, 16:32], 1, 1)
        return y

    # classifier.0 forward (exact pre-activation, gated Swish copy) and upsample.0 forward
    for x, W, b in ((tern((2 * B, FEAT), 0.25), tern((HID, FEAT), 0.25), torch.randint(-2, 3, (HID,), generator=g).double()),
                    (tern((3 * B, D), 0.5), tern((FEAT, D), 0.25), torch.randint(-2, 3, (FEAT,), generator=g).double())):
        y = F.linear(x, W, b)
        LR.check_exact(y.to(torch.bfloat16), y, "dense")
        sw = y * torch.sigmoid(y)
        LR.gate_elements(sw.to(torch.bfloat16), sw, y, "dense")
        yf = linear(x, W, b)
        with pytest.raises(AssertionError):
            LR.check_exact(yf.to(torch.bfloat16), y, "dense")
        with pytest.raises(AssertionError):
            LR.gate_elements((yf * torch.sigmoid(yf)).to(torch.bfloat16), sw, y, "dense")
    # classifier.3 data gradient: (d_encout W3) * Swish'(y1), column sums
    de, W3, r1 = tern((2 * B, 2 * D), 0.5), tern((2 * D, HID), 0.25), LR.eighths((2 * B, HID), g)
    acc = de @ W3
    v = acc * LR.dswish(r1)
    LR.gate_elements(v.to(torch.bfloat16), v, acc, "fc2_dgrad")
    LR.gate_sums(v.float().sum(0), v.sum(0), v.abs().sum(0), "fc2_dgrad")
    vf = linear(de, W3.t().contiguous()) * LR.dswish(r1)
    with pytest.raises(AssertionError):
        LR.gate_elements(vf.to(torch.bfloat16), v, acc, "fc2_dgrad")
    with pytest.raises(AssertionError):
        LR.gate_sums(vf.sum(0), v.sum(0), v.abs().sum(0), "fc2_dgrad")
