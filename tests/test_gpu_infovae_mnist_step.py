"""GPU tests of the MNIST InfoVAE's fp32 Linear kernels (mmvae_lin_act_*), its one-enqueue step (mmvae_mnist_infovae_step) and
``mnist.InfoVAETrainer``, against tests/infovae_mnist_step_ref.py.

Layer level, every shape of ``R.LAYER_SHAPES`` x every activation: y, dx, dW, db against float64 under
gate = LAYER_FACTOR x max(E_f32, 2^-23 max |ref|), E_f32 the error of the same layer in torch float32 on the CPU.  MEASURED on the
MI355X: the worst ratio E_hip / max(E_f32, 2^-23 max |ref|) is 2.22 (db of (65, 1024, 6272, perm), relu; y, dx and dW stay within
1.23), so LAYER_FACTOR = 8 leaves 3.6 x; a kernel beyond 8 x is wrong.  Rows permuted and sub-batches give bit-equal forward rows;
two calls are bit-equal, also with the workspace filled with NaN in between.

Whole step, formula weights at ``R.STEP_SHAPES`` with lambda_x, lambda_mmd = ``R.STEP_LAMBDAS`` and given ``true_samples``:
E_hip <= 2 E_emu + C_STEP E_f32 per tensor for recon, z, loss and all 12 gradients (E_emu: the float64 model with bf16-rounded
convolution operands against pure float64, E_f32: the CPU torch-float32 model against float64).  MEASURED: no tensor needs the
float32 term, (E_hip - 2 E_emu) / E_f32 is negative everywhere (worst E_hip / (2 E_emu) = 0.59, z at B = 1; worst E_hip / gate 0.50);
C_STEP = 4.  The four MMD sums equal ``mmvae_mmd`` on the returned z bit for bit.

`pytest -s` prints every figure.
"""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv4s2_ref as C  # noqa: E402
import infovae_mnist_step_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _lib():
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd._ops import stream
    return call, ptr, stream


def _ws(dev, rows, N, K, which, fill=None):
    call, _, _ = _lib()
    need = int(call("mmvae_lin_act_workspace_bytes", rows, N, K, which))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    if fill is not None:
        ws.view(torch.float32).fill_(fill)
    return ws


def _layer(dev, shape, kind, x, w, b, g, y_saved=None, fill=None):
    """the three kernels on one layer (operands in the weight's feature order; the permuted side is laid out channels-last here)
    -> {"y", "dx", "dw", "db"} back in the weight's order, on the CPU"""
    call, ptr, stream = _lib()
    rows, N, K, perm = shape
    code, slope = R.ACTS.index(kind), 0.1
    k_side = perm and K == 6272
    xd = (R.to_cl(x) if k_side else x).contiguous().to(dev)
    wd, bd = w.contiguous().to(dev), b.contiguous().to(dev)
    gd = (R.to_cl(g) if perm and not k_side else g).contiguous().to(dev)
    y = torch.empty(rows, N, device=dev)
    ws = _ws(dev, rows, N, K, 0, fill)
    call("mmvae_lin_act_fwd", ptr(xd), ptr(wd), ptr(bd), ptr(y), rows, N, K, code, slope, perm, ptr(ws), ws.numel(), stream())
    ys = y if y_saved is None else (R.to_cl(y_saved) if perm and not k_side else y_saved).contiguous().to(dev)
    dx, dw, db = torch.empty(rows, K, device=dev), torch.empty(N, K, device=dev), torch.empty(N, device=dev)
    ws = _ws(dev, rows, N, K, 1, fill)
    call("mmvae_lin_act_dgrad", ptr(gd), ptr(ys) if code else None, ptr(wd), ptr(dx), rows, N, K, code, slope, perm, ptr(ws), ws.numel(), stream())
    call("mmvae_lin_act_wgrad", ptr(gd), ptr(ys) if code else None, ptr(xd), ptr(dw), ptr(db), rows, N, K, code, slope, perm, stream())
    torch.cuda.synchronize()
    y, dx = y.cpu(), dx.cpu()
    return {"y": R.from_cl(y) if perm and not k_side else y, "dx": R.from_cl(dx) if k_side else dx, "dw": dw.cpu(), "db": db.cpu()}


def _sid(s):
    return "rows%d-N%d-K%d%s" % (s[0], s[1], s[2], "-perm" if s[3] else "")


@pytest.mark.parametrize("kind", R.ACTS)
@pytest.mark.parametrize("shape", R.LAYER_SHAPES, ids=_sid)
def test_layer_against_float64(shape, kind):
    dev = _dev()
    x, w, b, g = R.lin_operands(shape)
    got = _layer(dev, shape, kind, x, w, b, g)
    ref, yard, gates = R.lin_reference(x, w, b, g, kind, 0.1, y=got["y"])
    worst = 0.0
    for k in ("y", "dx", "dw", "db"):
        err = float((got[k].double() - ref[k]).abs().max())
        unit = gates[k] / R.LAYER_FACTOR
        worst = max(worst, err / unit)
        print("%s %-5s %-2s E_hip %.3e  E_f32 %.3e  max|ref| %.3e  E_hip / max(E_f32, floor) %.2f" %
              (_sid(shape), kind, k, err, yard[k], float(ref[k].abs().max()), err / unit))
    for k in ("y", "dx", "dw", "db"):
        assert float((got[k].double() - ref[k]).abs().max()) <= gates[k], (k, worst)
    assert worst <= 8.0


@pytest.mark.parametrize("shape", R.LAYER_SHAPES, ids=_sid)
def test_layer_rows_and_repeats_are_bit_equal(shape):
    dev = _dev()
    rows, N, K, perm = shape
    x, w, b, g = R.lin_operands(shape, seed=1)
    a = _layer(dev, shape, "leaky", x, w, b, g)
    again = _layer(dev, shape, "leaky", x, w, b, g, fill=float("nan"))
    for k in a:
        assert torch.equal(a[k], again[k]), k
    order = torch.randperm(rows, generator=torch.Generator().manual_seed(3))
    p = _layer(dev, shape, "leaky", x[order], w, b, g[order])
    assert torch.equal(p["y"], a["y"][order])
    for n in sorted({1, max(1, rows // 2)}):
        sub = _layer(dev, (n, N, K, perm), "leaky", x[:n], w, b, g[:n])
        assert torch.equal(sub["y"], a["y"][:n]), n


def test_layer_refusals():
    from multimodal_vae_amd._lib import MMVAEError
    dev = _dev()
    call, ptr, stream = _lib()
    t = torch.zeros(1 << 16, device=dev)
    with pytest.raises(MMVAEError, match="6272"):
        call("mmvae_lin_act_fwd", ptr(t), ptr(t), ptr(t), ptr(t), 2, 8, 8, 0, 0.1, 1, None, 0, stream())
    with pytest.raises(MMVAEError, match="act"):
        call("mmvae_lin_act_fwd", ptr(t), ptr(t), ptr(t), ptr(t), 2, 8, 8, 3, 0.1, 0, None, 0, stream())
    with pytest.raises(MMVAEError, match="aligned"):
        call("mmvae_lin_act_fwd", ptr(t[1:]), ptr(t), ptr(t), ptr(t), 2, 8, 8, 0, 0.1, 0, None, 0, stream())
    with pytest.raises(MMVAEError, match="rows"):
        call("mmvae_lin_act_wgrad", ptr(t), None, ptr(t), ptr(t), ptr(t), 0, 8, 8, 0, 0.1, 0, stream())
    with pytest.raises(MMVAEError, match="workspace"):
        call("mmvae_lin_act_fwd", ptr(t), ptr(t), ptr(t), ptr(t), 2, 20, 1024, 0, 0.1, 0, None, 0, stream())


# ------------------------------------------------------------------------------------------------------ the whole step
class _Engine:
    def __init__(self, dev, B, D, lambda_x, lambda_mmd):
        from multimodal_vae_amd import core
        self.st = core.MnistInfoVAEState(D, dev)
        self.sd = {k: v.float() for k, v in R.formula_weights(D).items()}
        assert [n for n, _, _ in self.st.table] == list(R.NAMES)
        for k, v in self.sd.items():
            self.st.view(k).copy_(v)
        self.eng = core.FusedInfoVAEStep(self.st, B, lr=1e-3, lambda_x=lambda_x, lambda_mmd=lambda_mmd)
        self.B, self.D, self.dev = B, D, dev

    def grads(self):
        out = {}
        for n, shape, off in self.st.table:
            numel = 1
            for s in shape:
                numel *= s
            out[n] = self.st.grads[off:off + numel].view(shape).clone().cpu()
        return out

    def run(self, x, ts, backward=True):
        recon = torch.empty(self.B, 784, device=self.dev)
        z = torch.empty(self.B, self.D, device=self.dev)
        out = self.eng.forward_backward(x.to(self.dev).contiguous(), True, backward, true_samples=None if ts is None else ts.to(self.dev),
                                        recon_image=recon, z=z)
        torch.cuda.synchronize()
        return recon.cpu().view(self.B, 1, 28, 28), z.cpu(), out.sums.clone().cpu(), float(out.total())


@functools.lru_cache(maxsize=None)
def _case(B, D):
    x = C.formula_input(B).float()
    ts = torch.randn(B, D, generator=torch.Generator().manual_seed(5))
    sd = {k: v.float() for k, v in R.formula_weights(D).items()}
    return (x, ts, sd) + R.step_yardsticks(sd, x, ts, *R.STEP_LAMBDAS)


@pytest.mark.parametrize("B,D", R.STEP_SHAPES)
def test_whole_step(B, D):
    from multimodal_vae_amd.mmd import mmd_terms
    dev = _dev()
    x, ts, sd, ref, e_emu, e_f32, gates = _case(B, D)
    e = _Engine(dev, B, D, *R.STEP_LAMBDAS)
    recon, z, sums, loss = e.run(x, ts)
    got = {"recon": recon.double(), "z": z.double(), "loss": torch.tensor([loss], dtype=torch.float64)}
    got.update({k: v.double() for k, v in e.grads().items()})
    want = R.tensors(ref)
    over = []
    for k in want:
        err = float((got[k] - want[k]).abs().max())
        c = (err - 2 * e_emu[k]) / e_f32[k] if e_f32[k] > 0 else 0.0
        print("B=%d D=%d %-24s E_hip %.3e  E_emu %.3e  E_f32 %.3e  max|ref| %.3e  (E_hip - 2 E_emu) / E_f32 %.2f  E_hip / gate %.3f"
              % (B, D, k, err, e_emu[k], e_f32[k], float(want[k].abs().max()), c, err / gates[k] if gates[k] > 0 else 0.0))
        if not err <= gates[k]:
            over.append((k, err, gates[k]))
    assert not over, over
    # the loss slots: SSE in slot 0, the four MMD values what mmvae_mmd returns for (true_samples, z), every other slot 0
    terms = mmd_terms(ts.to(dev), z.to(dev)).cpu()
    assert torch.equal(sums[12:16], terms), (sums[12:16], terms)
    assert float(sums[1:12].abs().max()) == 0.0
    sse = float(ref["sums"][0])
    assert abs(float(sums[0]) - sse) <= 784 * B / R.STEP_LAMBDAS[0] * gates["loss"] + 2.0 ** -20 * sse
    lx, lm = R.STEP_LAMBDAS
    assert abs(loss - (lx * float(sums[0]) / (B * 784) + lm * float(sums[15]))) <= 2.0 ** -21 * abs(loss)


def test_step_special_cases():
    dev = _dev()
    B, D = 4, 2
    x, ts, sd, ref, e_emu, e_f32, gates = _case(B, D)
    # lambda_x = 0: the decoder's gradients are exactly 0, the encoder's come from the MMD term alone
    e = _Engine(dev, B, D, 0.0, R.STEP_LAMBDAS[1])
    e.st.grads.fill_(7.0)
    e.run(x, ts)
    g = e.grads()
    assert all(float(g[k].abs().max()) == 0.0 for k in R.DECODER)
    only = R.step(sd, x, ts, 0.0, R.STEP_LAMBDAS[1])["grads"]
    assert float(only["encoder_fc.2.bias"].abs().max()) > 0
    emu0 = R.step(sd, x, ts, 0.0, R.STEP_LAMBDAS[1], emulate=True)["grads"]
    f320 = R.torch_step(sd, x, ts, 0.0, R.STEP_LAMBDAS[1], torch.float32)["grads"]
    for k in R.NAMES[:6]:
        gate = 2 * float((emu0[k] - only[k]).abs().max()) + R.C_STEP * float((f320[k] - only[k]).abs().max())
        assert float((g[k].double() - only[k]).abs().max()) <= gate, k
    # lambda_mmd = 0: the MSE-only gradient under the same gate, the MMD value still reported
    e = _Engine(dev, B, D, R.STEP_LAMBDAS[0], 0.0)
    _, _, sums, _ = e.run(x, ts)
    g = e.grads()
    mse = R.step(sd, x, ts, R.STEP_LAMBDAS[0], 0.0)
    emu = R.step(sd, x, ts, R.STEP_LAMBDAS[0], 0.0, emulate=True)["grads"]
    f32 = R.torch_step(sd, x, ts, R.STEP_LAMBDAS[0], 0.0, torch.float32)["grads"]
    for k in R.NAMES:
        gate = 2 * float((emu[k] - mse["grads"][k]).abs().max()) + R.C_STEP * float((f32[k] - mse["grads"][k]).abs().max())
        assert float((g[k].double() - mse["grads"][k]).abs().max()) <= gate, k
    assert abs(float(sums[15]) - float(mse["sums"][15])) <= gates["loss"] and float(sums[15]) != 0.0
    # do_backward = 0 leaves grads untouched
    e.st.grads.fill_(3.0)
    e.run(x, ts, backward=False)
    assert bool((e.st.grads == 3.0).all())
    # true_samples drawn on the device: the values of mmvae_normal on that stream; two calls with one counter are bit-equal
    from multimodal_vae_amd.mmd import mmd_terms
    call, ptr, stream = _lib()
    r1, z1, s1, _ = e.run(x, None, backward=False)
    drawn = torch.empty(B, D, device=dev)
    call("mmvae_normal", ptr(drawn), B * D, ctypes.c_ulonglong(e.eng.seed), ptr(e.eng.adam_state), 5, stream())
    torch.cuda.synchronize()
    assert torch.equal(s1[12:16], mmd_terms(drawn, z1.to(dev)).cpu())
    r2, z2, s2, _ = e.run(x, None, backward=False)
    assert torch.equal(r1, r2) and torch.equal(z1, z2) and torch.equal(s1, s2)


def test_step_twice_is_bit_equal_and_serial_agrees():
    dev = _dev()
    B, D = 9, 20
    x, ts, *_ = _case(B, D)
    e = _Engine(dev, B, D, *R.STEP_LAMBDAS)
    a = e.run(x, ts)
    ga = e.grads()
    e.eng.ws.view(torch.float32).fill_(float("nan"))
    b = e.run(x, ts)
    gb = e.grads()
    assert all(torch.equal(p, q) for p, q in zip(a[:3], b[:3])) and all(torch.equal(ga[k], gb[k]) for k in ga)


# ------------------------------------------------------------------------------------------------------ training
def test_training_and_checkpoint(tmp_path):
    import multimodal_vae_amd.data as D
    import multimodal_vae_amd.evaluate as E
    import multimodal_vae_amd.mnist as M
    import multimodal_vae_amd.train_infovae_mnist as T
    from multimodal_vae_amd.train_common import adam_state_dict
    dev = _dev()
    B = 32
    images = D.synthetic_mnist(B, seed=3)[0]
    data = images.float().div(255.0).unsqueeze(1)
    torch.manual_seed(21)
    ref_vae = M.InfoVAE(n_latents=20)
    sd = {k: v.detach().clone() for k, v in ref_vae.state_dict().items()}
    ts = torch.randn(B, 20, generator=torch.Generator().manual_seed(6))
    l64 = R.step(sd, data, ts)["loss"]
    lem = R.step(sd, data, ts, emulate=True)["loss"]
    # the module route under conv_backend = "hip" from equal weights and samples
    mod = M.set_infovae_backend(M.InfoVAE(n_latents=20), "hip")
    mod.load_state_dict(sd)
    mod.to(dev)
    with torch.no_grad():
        r_mod, z_mod = mod(data.to(dev))
        loss_mod = float(M.infovae_loss(r_mod, data.to(dev), z_mod, ts.to(dev)))
    vae = M.FusedInfoVAE(n_latents=20)
    assert list(vae.state_dict()) == list(sd)
    vae.load_state_dict(sd, strict=True)
    vae.to(dev)
    trainer = M.InfoVAETrainer(vae, B, lr=1e-3)
    xd = data.to(dev)
    losses = [float(trainer(xd, **({"true_samples": ts.to(dev)} if k == 0 else {})).total()) for k in range(20)]
    bound = 2 * abs(lem - l64) + 8 * 2.0 ** -23 * abs(l64)          # the bound of test_gpu_infovae_mnist.py
    print("step 0 %.8f (module route, hip backend %.8f, |difference| %.3e; float64 %.8f, emulated %.8f, bound %.3e), last five %.6f, "
          "first five %.6f" % (losses[0], loss_mod, abs(losses[0] - loss_mod), l64, lem, bound, sum(losses[-5:]) / 5, sum(losses[:5]) / 5))
    assert all(torch.isfinite(torch.tensor(losses)))
    assert sum(losses[-5:]) / 5 < sum(losses[:5]) / 5
    assert abs(losses[0] - loss_mod) <= bound
    # the parameters are views of the plan's flat buffer, and the module's own forward sees the trained weights
    st = vae._core.state
    assert vae.encoder_fc[0].weight.data_ptr() == st.view("encoder_fc.0.weight").data_ptr()
    r_f, z_f = vae(xd[:4])
    assert r_f.shape == (4, 1, 28, 28) and z_f.shape == (4, 20)
    # the checkpoint loads into a CPU InfoVAE, and evaluate latent_mmd runs on it
    T.save_checkpoint({"state_dict": vae.state_dict(), "best_loss": losses[-1], "n_latents": 20,
                       "optimizer": adam_state_dict(vae, trainer.engine)}, False, folder=str(tmp_path))
    path = os.path.join(str(tmp_path), "checkpoint.pth.tar")
    cpu = M.load_infovae_checkpoint(path)
    assert isinstance(cpu, M.InfoVAE) and next(cpu.parameters()).device.type == "cpu"
    with torch.no_grad():
        r_cpu, z_cpu = cpu.eval()(data[:4])
    assert float((r_f.cpu() - r_cpu).abs().max()) < 5e-2 and float((z_f.cpu() - z_cpu).abs().max()) < 5e-2
    torch.optim.Adam(cpu.parameters(), lr=1e-3).load_state_dict(torch.load(path, weights_only=False)["optimizer"])
    torch.save((images, torch.zeros(B, dtype=torch.int64)), os.path.join(str(tmp_path), "images.pt"))
    out = E.main(["latent_mmd", path, "--dataset", "mnist", "--data", os.path.join(str(tmp_path), "images.pt")])
    assert set(out) == {"n", "k_prior", "k_posterior", "k_cross", "mmd"} and out["n"] == B
    assert all(torch.isfinite(torch.tensor([float(v) for v in out.values()])))
