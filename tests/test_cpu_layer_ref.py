"""CPU companion of tests/test_gpu_layers.py, tests/test_gpu_celeba_layers.py and tests/test_gpu_coco_layers.py: the float64 layer reference (tests/layer_ref.py) the GPU test trusts is tied to the
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
        self.calls = []             # conv / transposed conv calls
        self.order = []             # ... and the Linear calls, in call order

    def __getattr__(self, name):
        return getattr(F, name)

    def _rec(self, fn, transposed, x, w, b, stride, pad):
        x.retain_grad()
        out = fn(x, w, b, stride, pad)
        out.retain_grad()
        self.calls.append(dict(transposed=transposed, x=x, w=w, out=out, stride=stride, pad=pad))
        self.order.append(self.calls[-1])
        return out

    def conv2d(self, x, w, b, stride, pad):
        return self._rec(F.conv2d, False, x, w, b, stride, pad)

    def conv_transpose2d(self, x, w, b, stride, pad):
        return self._rec(F.conv_transpose2d, True, x, w, b, stride, pad)

    def linear(self, x, w, b=None):
        if x.requires_grad:
            x.retain_grad()
        out = F.linear(x, w, b)
        out.retain_grad()
        self.order.append(dict(linear=True, x=x, w=w, out=out))
        return out


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
      "border": the border mask is wrong at one pixel: the top right pixel of the last image's operand reads as zero
      "slice" : the first two channel slices of the weights (dimension 0 of the parameter) sit in each other's place
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
        if w is not None and self.fault == "slice":
            w = w.clone()
            w[[0, 1]] = w[[1, 0]]
        drop, border = self.fault == "image", self.fault == "border"
        if layer == base:
            x = self._operand(L.x, L, L.ih, L.cin).clone()
            if drop:
                x[x.shape[0] // 2] = 0
            if border:
                x[-1, 0, -1] = 0
            out = self._shift(LR.ref_forward(L, x, w), 3)
            self.bufs[L.out] = out.to(torch.bfloat16).reshape(-1)
            self._table(L.stats, LR.ref_colstats(out, L.gf))
        elif layer.endswith("_wgrad"):
            x, dy = self._operand(L.x, L, L.ih, L.cin).clone(), self._operand(L.dy, L, L.oh, L.cout)
            if drop:
                x[x.shape[0] // 2] = 0
            if border:
                x[-1, 0, -1] = 0
            dw = LR.ref_wgrad(L, x, dy)
            if self.fault == "tap":
                dw[:, :, 1, 2] = 0
            if self.fault == "slice":
                dw[[0, 1]] = dw[[1, 0]]
            self.grads[L.param] = self._shift(dw, 1 if L.transposed else 0)
        else:
            dy = self._operand(L.dy, L, L.oh, L.cout).clone()
            if drop:
                dy[dy.shape[0] // 2] = 0
            if border:
                dy[-1, 0, -1] = 0
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
FAULTS_COCO = FAULTS + ("border", "slice")
_FAMILIES = {"multimnist": LR.LAYERS, "celeba": LR.LAYERS_CELEBA, "coco": LR.LAYERS_COCO}
_FAMILY_FAULTS = {"multimnist": FAULTS, "celeba": FAULTS, "coco": FAULTS_COCO}


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
        for fault in _FAMILY_FAULTS[family]:
            assert _run_checks(_SimHarness(layers, fault), layers, name, 4) == {"forward", "wgrad", "dgrad"}, (name, fault)


@pytest.mark.parametrize("fault", FAULTS)
def test_sum_gates_see_every_fault(fault):
    """The 2^-16 gate of the BatchNorm-backward sums alone (check_dgrad stops at the per-element gate first), on the data gradient of
    every CelebA layer geometry (with tables, whether or not the step's layer has a BatchNorm below it): the sums of a faulty
    launch fall outside, those of the reference inside."""
    _sum_gates(LR.LAYERS_CELEBA, fault)


@pytest.mark.parametrize("fault", FAULTS_COCO)
def test_coco_sum_gates_see_every_fault(fault):
    """the same on every COCO layer geometry, with the two faults of the small maps (border pixel, channel slice) on top"""
    _sum_gates(LR.LAYERS_COCO, fault)


def _sum_gates(layers, fault):
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


# ------------------------------------------------------------------------------------------------ COCO
def _coco_cases():
    """every (batch, seed) tests/test_gpu_coco_layers.py uses: both seeds at the small batches, the first at the large ones"""
    return [(B, seed) for B in LR.BATCHES_COCO for seed in (LR.SEEDS if B <= 8 else LR.SEEDS[:1])]


@pytest.mark.parametrize("name", list(LR.LAYERS_COCO))
def test_coco_operands_stay_in_the_exact_regime(name):
    """forward on gf * B images, both gradients on gb * B images, for every (batch, seed) of the GPU module"""
    L = LR.LAYERS_COCO[name]
    assert L.gf == L.gb
    for B, seed in _coco_cases():
        x, w, dy = LR.layer_operands(name, L.gf * B, seed, LR.LAYERS_COCO)
        out = LR.ref_forward(L, x, w)
        LR.assert_exact_regime(out=out, groups=L.gf, what="%s forward B=%d seed %d" % (name, B, seed))
        assert float(out.abs().max()) > 0
        LR.assert_exact_regime(dw=LR.ref_wgrad(L, x, dy), what="%s wgrad B=%d seed %d" % (name, B, seed))
        acc = LR.ref_dgrad_acc(L, dy, w)
        assert bool((acc == acc.round()).all()) and float(acc.abs().max()) <= 256, (name, B, seed, float(acc.abs().max()))
    ws, xs = zip(*[LR.layer_operands(name, L.gf * 8, seed, LR.LAYERS_COCO)[1::-1] for seed in LR.SEEDS])
    LR.assert_operand_coverage(list(ws), list(xs))


def test_coco_pass_operands_stay_in_their_regimes():
    """the operands of the stand-alone passes and of the last layer at the smallest and the largest batch of the GPU module: the
    written statistics are exact in fp32, and the last layer's logits are integers with at least 90 % in |l| <= 8, none beyond 14"""
    for B in (min(LR.BATCHES_COCO), max(LR.BATCHES_COCO)):
        for name, L in LR.LAYERS_COCO.items():
            g = LR.gen(0, 1, 16, L.gf * B)
            stats = LR.slot_stats_any(LR.eighths((L.gf * B, L.oh, L.oh, 8), g), L.gf)
            assert torch.equal(stats.float().double(), stats), (name, B)
            red = LR.staged_bwd_operands(L._replace(cout=8), L.gb * B, L.gb, B * L.oh * L.oh, g, integer_slots=False)[2]
            assert torch.equal(red.float().double(), red), (name, B)
        for seed in LR.SEEDS:
            g = LR.gen(seed, 21, B)
            a3 = LR.ternary((3 * B, 16, 16, 64), LR.LAST_X_DENSITY, g)
            w9 = LR.ternary((64, 3, 4, 4), LR.LAST_W_DENSITY, g)
            LR.assert_last_layer_regime(F.conv_transpose2d(LR._nchw(a3), w9, None, 2, 1))
    # slot_stats_any is slot_stats where the rows divide evenly
    r = LR.eighths((3 * 4, 8, 8, 16), LR.gen(0, 2))
    assert torch.equal(LR.slot_stats_any(r, 3), LR.slot_stats(r, 3))


def test_coco_references_agree_with_autograd_on_the_oracle_modules(monkeypatch):
    """oracle.mmvae_ref's COCO image encoder and decoder in float64 with autograd, every conv and Linear call recorded:
    LAYERS_COCO's geometry reproduces each conv's output, weight gradient and input gradient; ref_bn_tables + ref_stage_fwd
    reproduce the tensor the next module reads (for features.9 through the NCHW flatten c * 4 + y * 2 + x, for upsample.0 through
    the NHWC map the engine writes); ref_dgrad_epilogue + ref_bn_backward reproduce the gradient at the conv's raw output and the
    BatchNorm parameter gradients from the gradient at that next module's input; ref_dec_last reproduces the decoder's output."""
    from test_gpu_coco_layers import BN_PASSES, _flat_nchw, _map_nhwc
    torch.manual_seed(0)
    B = 3
    P = {k: (v.double().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.double() if v.is_floating_point() else v)
         for k, v in R.formula_params("coco", 100).items()}
    rec = _Recorder()
    monkeypatch.setattr(R, "F", rec)
    image = torch.rand(B, 3, 32, 32, dtype=torch.float64).requires_grad_(True)
    z = torch.randn(B, 100, dtype=torch.float64)
    enc = R.coco_image_encoder(P, image * 1.0, True, None, drop_p=0.0)
    dec = R.coco_image_decoder(P, z, True)
    ((enc * torch.randn_like(enc)).sum() + (dec * torch.randn_like(dec)).sum()).backward()
    monkeypatch.undo()
    assert len(rec.calls) == 8 and len(rec.order) == 12
    by_weight = {id(c["w"]): c for c in rec.order}
    after = {id(c["w"]): rec.order[i + 1] for i, c in enumerate(rec.order[:-1])}       # the module that reads a call's result
    # (float64 through two different formulas of the BatchNorm backward: cancellation leaves 1e-10 absolute)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-7, atol=1e-9)
    for name, L in LR.LAYERS_COCO.items():
        c = by_weight[id(P[L.param])]
        assert c["transposed"] == L.transposed and c["stride"] == L.stride and c["pad"] == L.pad, name
        assert tuple(c["w"].shape) == LR.weight_shape(L), name
        x, dy = LR._nhwc(c["x"].detach()), LR._nhwc(c["out"].grad)
        assert tuple(x.shape) == (B, L.ih, L.ih, L.cin) and tuple(dy.shape) == (B, L.oh, L.oh, L.cout), name
        w = c["w"].detach()
        torch.testing.assert_close(LR.ref_forward(L, x, w), LR._nhwc(c["out"].detach()), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(LR.ref_wgrad(L, x, dy), c["w"].grad, rtol=1e-10, atol=1e-12)
        torch.testing.assert_close(LR.ref_dgrad_acc(L, dy, w), LR._nhwc(c["x"].grad), rtol=1e-10, atol=1e-12)
        # the BatchNorm + Swish behind it, forward and backward (one group: the oracle runs one pass)
        bn = [v[1] for v in BN_PASSES.values() if v[0] == name][0]
        gamma, beta = P[bn + ".weight"].detach(), P[bn + ".bias"].detach()
        r, count = LR._nhwc(c["out"].detach()), B * L.oh * L.oh
        scale, shift, mean, rstd = LR.ref_bn_tables(LR.slot_stats_any(r, 1), count, gamma, beta)
        a, _ = LR.ref_stage_fwd(r, scale, shift, 1)
        nxt = after[id(c["w"])]
        if "linear" in nxt:                              # features.9 -> classifier.0: torch's flatten of (512, 2, 2)
            close(_flat_nchw(a), nxt["x"].detach())
            da = LR._nhwc(nxt["x"].grad.reshape(B, 512, 2, 2))
        else:
            close(a, LR._nhwc(nxt["x"].detach()))
            da = LR._nhwc(nxt["x"].grad)
        aff, mr = torch.stack([scale, shift], -1), torch.stack([mean, rstd], -1)
        db, red, _ = LR.ref_dgrad_epilogue(da, r, aff, mr, 1)
        table = torch.zeros(1, LR.STAT_SLOTS, L.cout, 2, dtype=torch.float64)
        table[:, 5] = red
        dr, dgamma, dbeta, _, _ = LR.ref_bn_backward(db, r, table, mr, gamma, count, 1)
        close(dr, dy)
        close(dgamma, P[bn + ".weight"].grad)
        close(dbeta, P[bn + ".bias"].grad)
    # upsample.0: the engine's NHWC columns s * 512 + c of Linear(D, 2048) are what hallucinate.0 reads
    up = by_weight[id(P["image_decoder.upsample.0.weight"])]
    u = _map_nhwc(up["out"].detach())
    close(u * torch.sigmoid(u), LR._nhwc(after[id(up["w"])]["x"].detach()))
    # last layer: logits -> sigmoid is the decoder's output; dlogit is autograd's gradient of sum_g coef[g] * BCE_g
    last = by_weight[id(P["image_decoder.hallucinate.9.weight"])]
    a3 = LR._nhwc(last["x"].detach()).repeat(3, 1, 1, 1)
    target = torch.rand(B, 3, 32, 32, dtype=torch.float64)
    coef = torch.tensor([0.7, 0.2, 0.0], dtype=torch.float64)
    logits, recon, dlogit, sums, mags = LR.ref_dec_last(a3, last["w"].detach(), target, coef)
    close(recon[:B], dec.detach())
    lg = logits.clone().requires_grad_(True)
    per = F.binary_cross_entropy(torch.sigmoid(lg), target.repeat(3, 1, 1, 1), reduction="none").reshape(3, -1).sum(1)
    close(per.detach(), sums)
    (per * coef).sum().backward()
    close(lg.grad, dlogit)


def test_coco_pass_gates_pass_on_the_reference_and_see_every_fault():
    """The gates of the stand-alone passes and of the last layer, on values stored the way the engine stores them (bf16 / fp32):
    they pass on the reference and fail on a reference with one group's table used for another, db2 ignored, one border pixel of
    the im2col wrong, and -- last layer -- one tap dropped, one channel slice swapped, one border logit off by one, one group's
    loss weight used for another."""
    from test_gpu_coco_layers import _within
    B = 4
    # ---- BatchNorm forward (3 groups): tables of group g + 1 used for group g
    L = LR.LAYERS_COCO["dec_convT2"]
    G, C, count = 3, L.cout, B * L.oh * L.oh
    g = LR.gen(0, 31)
    r = LR.eighths((G * B, L.oh, L.oh, C), g)
    r[B:2 * B] = (r[B:2 * B] / 2 + 1).mul(8).round() / 8          # the groups differ in mean and variance, as passes do
    gamma = torch.tensor([1.0, 2.0, -1.0])[torch.randint(0, 3, (C,), generator=g)].double()
    beta = torch.randint(-1, 2, (C,), generator=g).double()
    scale, shift, mean, rstd = LR.ref_bn_tables(LR.slot_stats_any(r, G), count, gamma, beta)
    a, _ = LR.ref_stage_fwd(r, scale, shift, G)
    gate = LR.gate_stage_fwd(r, scale, shift, mean, beta, a, G)
    _within(a.to(torch.bfloat16), a, gate, "bn forward")
    wrong, _ = LR.ref_stage_fwd(r, scale.roll(1, 0), shift.roll(1, 0), G)
    with pytest.raises(AssertionError):
        _within(wrong.to(torch.bfloat16), a, gate, "bn forward, tables of another group")
    rm, rv, unb = LR.ref_bn_running(LR.slot_stats_any(r, G), count, torch.zeros(C), torch.ones(C), 1)
    rm1, rv1, _ = LR.ref_bn_running(LR.slot_stats_any(r, G)[:2], count, torch.zeros(C), torch.ones(C), 1)
    gm, gv = (16 + 15) * LR.EPS32 * 4 * torch.ones_like(rm), (22 + 15) * LR.EPS32 * torch.maximum(unb, torch.ones(C).double())
    _within(rm.float(), rm, gm, "running mean")
    _within(rv.float(), rv, gv, "running variance")
    with pytest.raises(AssertionError):
        _within(rm1.float(), rm, gm, "running mean, one group's update missing")
    with pytest.raises(AssertionError):
        _within(rv1.float(), rv, gv, "running variance, one group's update missing")
    # ---- BatchNorm backward: another group's (mean, rstd); enc_bn4_bwd with db2 ignored; at a power-of-two count and at count 12
    for Ln, Bn in (("dec_convT2", 4), ("enc_conv4", 4), ("enc_conv4", 3)):
        L = LR.LAYERS_COCO[Ln]
        G, count = L.gb, Bn * L.oh * L.oh
        db, r, red, mr, gamma = LR.staged_bwd_operands(L, G * Bn, G, count, g, integer_slots=False)
        db2 = LR.ternary(db.shape, LR.G_DENSITY, g) if G == 1 else torch.zeros_like(db)
        dr, dgamma, dbeta, mag_g, mag_b = LR.ref_bn_backward(db + db2, r, red, mr, gamma, count, G)
        gate = LR.gate_bn_backward(db + db2, r, red, mr, gamma, count, G, dr)
        _within(dr.to(torch.bfloat16), dr, gate, "bn backward")
        if G == 1:
            bad = LR.ref_bn_backward(db, r, red, mr, gamma, count, G)[0]
        else:
            bad = LR.ref_bn_backward(db, r, red.roll(1, 0), mr.roll(1, 0), gamma, count, G)[0]
        with pytest.raises(AssertionError):
            _within(bad.to(torch.bfloat16), dr, gate, "bn backward, db2 ignored / another group's tables")
        LR.gate_sums(dgamma.float(), dgamma, mag_g, "dgamma")
        with pytest.raises(AssertionError):
            LR.gate_sums(LR.ref_bn_backward(db, r, red[:, 1:], mr, gamma, count, G)[1], dgamma, mag_g, "dgamma, one slot missing")
    # ---- im2col: the comparison is equality; a border pixel that is not zeroed differs
    dl = LR.eighths((2, 3, 32, 32), g)
    dl[dl == 0] = 0.125
    want = LR.patches_k4s2(dl)
    assert float(want[0, 0]) == 0.0 and float(want[0, 5 * 3]) == float(dl[0, 0, 0, 0])      # row (0, 0): tap (0, 0) outside, tap (1, 1) = pixel (0, 0)
    assert tuple(want.shape) == (2 * 256, 48)
    # ---- last layer
    a3 = LR.ternary((3 * B, 16, 16, 64), LR.LAST_X_DENSITY, g)
    w9 = LR.ternary((64, 3, 4, 4), LR.LAST_W_DENSITY, g)
    target = torch.tensor(LR.LAST_TARGETS, dtype=torch.float64)[torch.randint(0, 4, (B, 3, 32, 32), generator=g)]
    coef = LR.last_layer_coef(B)
    logits, recon, dlogit, sums, mags = LR.ref_dec_last(a3, w9, target, coef)
    LR.check_exact(logits.float(), logits, "logits")
    LR.gate_last_layer(recon.float(), recon, LR.LAST_RECON_MULT, "recon")
    LR.gate_last_layer(dlogit.float(), dlogit, LR.LAST_DLOGIT_MULT, "dlogit")
    LR.gate_last_sums(sums.float(), sums, mags, "BCE sums")
    w_tap, w_slice, a_border = w9.clone(), w9.clone(), a3.clone()
    w_tap[:, :, 1, 2] = 0
    w_slice[[0, 1]] = w_slice[[1, 0]]
    a_border[0, 0, -1] = 0               # (an image of the first group: the last group's loss weight is 0)
    for what, args in (("tap", (a3, w_tap, target, coef)), ("slice", (a3, w_slice, target, coef)), ("border", (a_border, w9, target, coef)),
                       ("coef", (a3, w9, target, coef.roll(1)))):
        lo, re_, dl_, su, _ = LR.ref_dec_last(*args)
        if what != "coef":
            with pytest.raises(AssertionError):
                LR.check_exact(lo.float(), logits, "logits " + what)
            with pytest.raises(AssertionError):
                LR.gate_last_layer(re_.float(), recon, LR.LAST_RECON_MULT, "recon " + what)
        with pytest.raises(AssertionError):
            LR.gate_last_layer(dl_.float(), dlogit, LR.LAST_DLOGIT_MULT, "dlogit " + what)
        if what in ("tap", "slice"):
            with pytest.raises(AssertionError):
                LR.gate_last_sums(su.float(), sums, mags, "BCE sums " + what)
    # one logit off by one: the elementwise gates see it, and so does the sum of its group
    off = logits.clone()
    off[0, 0, 0, 31] += 1
    p_off = torch.sigmoid(off)
    assert float((p_off - recon).abs().max()) > 3e-4 or float(logits[0, 0, 0, 31].abs()) > 8
    with pytest.raises(AssertionError):
        LR.gate_last_layer(p_off.float(), recon, LR.LAST_RECON_MULT, "recon, one logit off by one")


@pytest.mark.parametrize("fault", ["column", "row", "tile"])
def test_coco_dense_gates_see_every_fault(fault):
    """The comparisons tests/test_gpu_coco_layers.py makes on the dense layers, at its densities and B = 4, against the float64
    reference with one input column ignored, one row dropped or one tile of 16 output columns shifted: classifier.0 / .3 / .6 and
    upsample.0 forward (exact pre-activation, gated Swish copy), classifier.6's and classifier.3's data gradients with their column
    sums.  Every comparison fails on the fault and passes on the unharmed reference."""
    B, D, HID1, HID2, FEAT = 4, 100, 1024, 256, 2048
    g = LR.gen(0, 13, B)
    tern = lambda shape, d: LR.ternary(shape, d, g)
    ib = lambda n: torch.randint(-2, 3, (n,), generator=g).double()

    def linear(x, W, b=None):
        x, W = x.clone(), W.clone()
        if fault == "column":
            W[:, int(torch.nonzero(x.abs().sum(0))[0])] = 0
        if fault == "row":
            x[x.shape[0] // 2] = 0
        y = F.linear(x, W, b)
        if fault == "tile":
            y[:, 16:32] = torch.roll(y[:, 16:32], 1, 1)
        return y

    for x, W, b, limit in ((tern((2 * B, FEAT), 0.25), tern((HID1, FEAT), 0.25), ib(HID1), 256), (tern((2 * B, HID1), 0.25), tern((HID2, HID1), 0.25), ib(HID2), 256),
                           (tern((2 * B, HID2), 0.5), tern((2 * D, HID2), 0.25), ib(2 * D), 2 ** 24), (tern((3 * B, D), 0.5), tern((FEAT, D), 0.25), ib(FEAT), 256)):
        y = F.linear(x, W, b)
        LR.check_exact(y.to(torch.bfloat16) if limit == 256 else y.float(), y, "dense", limit)
        sw = y * torch.sigmoid(y)
        LR.gate_elements(sw.to(torch.bfloat16), sw, y, "dense")
        yf = linear(x, W, b)
        with pytest.raises(AssertionError):
            LR.check_exact(yf.to(torch.bfloat16) if limit == 256 else yf.float(), y, "dense", limit)
        with pytest.raises(AssertionError):
            LR.gate_elements((yf * torch.sigmoid(yf)).to(torch.bfloat16), sw, y, "dense")
    for de, W, r in ((tern((2 * B, 2 * D), 0.5), tern((2 * D, HID2), 0.25), LR.eighths((2 * B, HID2), g)),
                     (tern((2 * B, HID2), 0.5), tern((HID2, HID1), 0.25), LR.eighths((2 * B, HID1), g))):
        acc = de @ W
        v = acc * LR.dswish(r)
        LR.gate_elements(v.to(torch.bfloat16), v, acc, "dgrad")
        LR.gate_sums(v.float().sum(0), v.sum(0), v.abs().sum(0), "dgrad")
        vf = linear(de, W.t().contiguous()) * LR.dswish(r)
        with pytest.raises(AssertionError):
            LR.gate_elements(vf.to(torch.bfloat16), v, acc, "dgrad")
        with pytest.raises(AssertionError):
            LR.gate_sums(vf.sum(0), v.sum(0), v.abs().sum(0), "dgrad")
