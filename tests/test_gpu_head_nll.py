"""GPU tests of the fused PixelCNN head ``pixelcnn.head_nll`` (csrc/head_nll.hip) and of everything that runs on it: ``pixelcnn.nll``
with ``head="hip"``, ``train_step(..., head="hip")`` and ``evaluate nll_pixelcnn --head hip``.

The gates are functions of tests/head_nll_ref.py (tests/test_cpu_head_nll.py shows that each catches the faults it is meant to catch):

forward, tight    nll (autograd op) and lse (C entry) against float64 on bf16-rounded operands; the gate is GATE_FACTOR (8) x
                  max(error of the same computation in float32 on the CPU, 2^-23 max |reference|).  Also at logits of magnitude 100 and
                  more (weights x 30, one level with a bias of -200 that is the target at one position), where everything must be finite.
db, tight         g non-zero at a single position: db is d there, one summand, no bf16 rounding of d involved.
dh, dw, tight     on separated supports (h non-zero in one half of the channels, w in the other, bias constant per data channel, g signed
                  powers of two, V a power of two): d is exact in bf16, the other halves of dh / dw are exactly 0.
dh, dw, db, loose on the general cases against PURE float64: the kernel error must be <= 2 x the emulation's own error, per tensor.  d is
                  rounded to bf16 from values computed in fp32, so rounding boundaries flip between correct realisations and a gate on
                  |kernel - emulation| would be wrong (the rule and the reason of tests/test_gpu_pixelcnn_train.py).
exactness         identical bits over two calls with the workspace filled with NaN in between; sample 0 alone = sample 0 in a batch;
                  g = 0 rows give dh exactly 0; gradients nobody asked for stay None; a target of V gives NaN there and only there.
whole model       the four MODELS of tests/test_gpu_pixelcnn_train.py under ``set_conv_backend("hip")`` and ``head="hip"``: loss and every
                  parameter's gradient against pure float64 within 2 x the emulated model's error; ``nll(head="hip")`` against the float64
                  head on the bf16-rounded features brought back from the device, tight.
training          30 steps of ``train_step(..., head="hip")``; step 0 within 2 x the loss yardstick of the torch head, step 29 below step 0.
evaluation        ``evaluate nll_pixelcnn --head hip --cuda --synthetic 20 --batch_size 8`` against ``--head torch`` per image, within the
                  sum of the tight per-element gates.  That bound is an fp32 one, so the checkpoint is built for it: conv2 has zero
                  weights and bf16-representable biases and conv4 bf16-representable weights, which makes the head's operands exact in
                  bf16 and leaves fp32 rounding as the only difference between the two heads.

MEASURED (largest ratio per tensor over the cases; `pytest -s` prints every one):

gate                                   tensor: largest ratio over the cases (MI355X)               must stay <=
forward, tight (11 cases)              nll 1.00   lse 1.00                                          8
forward at large logits (3 cases)      nll 0.55   lse 1.07   (all finite)                           8
db, one position (4 cases)             db 1.37                                                      8
dh, dw on separated supports (12)      dh 1.85   dw 3.16   (the other halves exactly 0)             8
dh, dw, db, loose (11 cases)           dh 1.00   dw 1.00   db 1.00                                  2
whole model (4 models)                 loss 1.00 / 1.04 / 1.57 / 1.01; worst gradient 1.00 / 1.02 / 1.04 / 1.00             2
  head on the device's features        nll 1.21 / 0.57 / 0.58 / 1.14                                8
training plain: step 0 2.083780 (torch head 2.083790, |difference| 1.05e-05 / loss yardstick 1.07e-05  0.98; gate 2), step 29 2.021025
training gated: step 0 2.114776 (torch head 2.114779, |difference| 2.38e-06 / loss yardstick 2.37e-06  1.01; gate 2), step 29 2.053133
evaluation: per-image |hip - torch| 1.97e-05, sum of the per-element gates 7.15e-04, ratio 0.03 (gate 1)
"""
import copy
import ctypes
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_nll_ref as HR  # noqa: E402
import pixelcnn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# (gated, n_blocks, C, hid, V, B, H, W): the four MODELS of tests/test_gpu_pixelcnn_train.py
MODELS = [(0, 3, 3, 48, 8, 3, 6, 9), (1, 3, 3, 48, 8, 3, 6, 9), (1, 1, 1, 128, 8, 2, 4, 4), (0, 1, 3, 16, 256, 3, 9, 5)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _geometry():
    import multimodal_vae_amd.pixelcnn as P
    tile, _, chunk = P.head_nll_geometry()[:3]
    return tile, chunk


def _c_forward(h, w, b, t, C, want_lse=True):
    """the C entry directly -> (nll, lse) on the device"""
    import multimodal_vae_amd.pixelcnn as P
    from multimodal_vae_amd._lib import call, ptr
    B, hid, H, W = h.shape
    dims = (B, C, H, W, hid, w.shape[0] // C)
    hc = h.contiguous(memory_format=torch.channels_last)
    ws = P._conv_ws(h.device, P.head_nll_workspace_bytes(*dims))
    nll = torch.empty(B, C, H, W, dtype=torch.float32, device=h.device)
    lse = torch.empty_like(nll) if want_lse else None
    call("mmvae_head_nll_forward", ptr(hc), ptr(w.contiguous()), ptr(b), ptr(t), ptr(nll), ptr(lse), *dims, ptr(ws), ws.numel(),
         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return nll, lse


def _run(h, w, b, t, g, C, grads=(True, True, True)):
    """the device op on CPU operands -> CPU results {"nll", "lse", "dh", "dw", "db"}"""
    import multimodal_vae_amd.pixelcnn as P
    dev = _dev()
    hd, wd, bd = (x.to(dev).requires_grad_(r) for x, r in zip((h, w, b), grads))
    td = t.to(dev)
    nll = P.head_nll(hd, wd, bd, td, C)
    nll_c, lse = _c_forward(hd.detach(), wd.detach(), bd.detach(), td, C)
    assert torch.equal(nll_c, nll.detach()) or bool(torch.isnan(nll_c).any())
    out = {"nll": nll.detach().cpu(), "lse": lse.cpu()}
    if g is not None and any(grads):
        nll.backward(g.to(dev))
        out.update({"dh": None if hd.grad is None else hd.grad.cpu(), "dw": None if wd.grad is None else wd.grad.cpu(),
                    "db": None if bd.grad is None else bd.grad.cpu()})
    return out


def _all_cases():
    return HR.CASES + HR.tile_cases(64)


def _report(label, ratios, factor):
    print("%-44s" % label + "  ".join("%s %.4g" % (k, v) for k, v in ratios.items()) + "   (gate %g)" % factor)
    for k, v in ratios.items():
        assert v <= factor, (label, k, v, factor)


def test_geometry_is_what_the_cases_assume():
    _dev()
    tile, chunk = _geometry()
    assert HR.tile_cases(tile) == HR.tile_cases(64) and chunk == 1024
    B, C, hid, V, H, W = HR.CASES[-1]
    assert 2 * chunk < B * H * W < 3 * chunk                         # 2 chunks and a partial third


# ------------------------------------------------------------------------------------------------------ the op
@pytest.mark.parametrize("case", _all_cases(), ids=HR.case_id)
def test_forward_tight(case):
    _report("forward " + HR.case_id(case), HR.check_forward(_run, case), HR.GATE_FACTOR)


@pytest.mark.parametrize("case", HR.CASES[1:4], ids=HR.case_id)
def test_forward_large_logits(case):
    ops, (ref, _) = HR._tight("large", case)
    assert float(ref["lse"].abs().max()) > 100
    got = _run(*ops[:4], None, case[1])
    assert bool(torch.isfinite(got["nll"]).all()) and bool(torch.isfinite(got["lse"]).all())
    _report("large logits " + HR.case_id(case), HR.check_forward(_run, case, "large"), HR.GATE_FACTOR)


@pytest.mark.parametrize("case", HR.DB1_CASES, ids=HR.case_id)
def test_db_single_position(case):
    _report("db, one position " + HR.case_id(case), HR.check_db1(_run, case), HR.GATE_FACTOR)


@pytest.mark.parametrize("h_first", [True, False], ids=["h-first", "w-first"])
@pytest.mark.parametrize("levels", HR.SEPARATED_LEVELS)
@pytest.mark.parametrize("shape", HR.SEPARATED_SHAPES, ids=["multi-chunk", "two-k-blocks"])
def test_separated_supports(shape, levels, h_first):
    case = shape[:3] + (levels,) + shape[4:]
    _report("separated %s %s" % (HR.case_id(case), "h-first" if h_first else "w-first"), HR.check_separated(_run, case, h_first),
            HR.GATE_FACTOR)


@pytest.mark.parametrize("case", _all_cases(), ids=HR.case_id)
def test_gradients_general(case):
    _report("gradients " + HR.case_id(case), HR.check_loose(_run, case), HR.LOOSE_FACTOR)


# ------------------------------------------------------------------------------------------------------ exactness
def _poison_workspace():
    import multimodal_vae_amd.pixelcnn as P
    for ws in P._CONV_WS.values():
        ws.view(torch.float32).fill_(float("nan"))


@pytest.mark.parametrize("case", [HR.CASES[1], HR.CASES[6], HR.CASES[7]], ids=HR.case_id)
def test_two_calls_give_identical_bits(case):
    ops = HR.operands(case)
    a = _run(*ops, case[1])
    _poison_workspace()
    b = _run(*ops, case[1])
    for k in ("nll", "lse", "dh", "dw", "db"):
        assert torch.equal(a[k], b[k]), k
        assert bool(torch.isfinite(a[k]).all()), k


def test_a_sample_does_not_depend_on_its_batch():
    case = (3, 3, 48, 8, 6, 9)
    h, w, b, t, g = HR.operands(case)
    full = _run(h, w, b, t, g, 3)
    alone = _run(h[:1], w, b, t[:1], g[:1], 3)
    assert torch.equal(full["nll"][:1], alone["nll"]) and torch.equal(full["dh"][:1], alone["dh"])


def test_zero_g_rows_and_unasked_gradients():
    case = HR.CASES[2]
    h, w, b, t, g = HR.operands(case)
    g = g.clone()
    g[0, :, 2, 3] = 0.0
    g[0, :, 0, 0] = -0.0
    got = _run(h, w, b, t, g, case[1], grads=(True, False, False))
    assert got["dw"] is None and got["db"] is None                   # weight.grad / bias.grad stay None
    zero = (g == 0).all(dim=1)                                       # (B, H, W)
    assert int(zero.sum()) >= 3
    rows = got["dh"].permute(0, 2, 3, 1)[zero]
    assert torch.equal(rows, torch.zeros_like(rows))
    assert bool((got["dh"].permute(0, 2, 3, 1)[~zero] != 0).any())
    only_w = _run(h, w, b, t, g, case[1], grads=(False, True, False))
    assert only_w["dh"] is None and only_w["db"] is None and only_w["dw"] is not None


def test_target_out_of_range_gives_nan_there_only():
    case = HR.CASES[4]
    h, w, b, t, g = HR.operands(case)
    t = t.clone()
    t[0, 1, 3, 4] = case[3]                                          # V
    t[0, 2, 0, 0] = -1
    got = _run(h, w, b, t, None, case[1])
    nan = torch.isnan(got["nll"])
    want = torch.zeros_like(nan)
    want[0, 1, 3, 4] = want[0, 2, 0, 0] = True
    assert torch.equal(nan, want)
    assert bool(torch.isfinite(got["lse"]).all())
    ref = HR.head(h, w, b, t, None, case[1])
    assert HR.error(got["nll"], ref["nll"]) < 1e-4


def test_limits_raise_before_any_launch():
    import multimodal_vae_amd.pixelcnn as P
    dev = _dev()
    h, w, b, t, _ = (x.to(dev) for x in HR.operands((1, 1, 16, 4, 2, 2)))
    for bad_h, bad_w in ((h[:, :12], w[:, :12]), (torch.zeros(1, 264, 2, 2, device=dev), torch.zeros(4, 264, 1, 1, device=dev))):
        with pytest.raises(P.MMVAEError):
            P.head_nll(bad_h.contiguous(), bad_w.contiguous(), b, t, 1)
    with pytest.raises(P.MMVAEError):
        P.head_nll(h, w, b, t.int(), 1)
    with pytest.raises(P.MMVAEError):
        P.head_nll(h, torch.zeros(8, 16, 1, 1, device=dev), torch.zeros(8, device=dev), t.expand(1, 2, 2, 2).contiguous(), 2)     # C = 2


# ------------------------------------------------------------------------------------------------------ whole model
def _loss_and_grads(sd, cfg, x, target, emulated):
    leaves = {k: v.double().clone().requires_grad_(k.endswith(("weight", "bias"))) for k, v in sd.items()}
    loss = HR.model_nll(leaves, cfg, x, target, emulated).mean()
    names = [k for k, v in leaves.items() if v.requires_grad]
    grads = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    return float(loss.detach()), {k: g for k, g in zip(names, grads) if g is not None}


@pytest.mark.parametrize("spec", MODELS, ids=lambda s: "%s-b%d-c%d-h%d-v%d-B%d-%dx%d" % (("gated" if s[0] else "plain",) + tuple(s[1:])))
def test_whole_model(spec):
    import multimodal_vae_amd.pixelcnn as P
    dev = _dev()
    c = R.case(*spec)
    cfg, sd, target = c["cfg"], c["sd"], c["given"]
    x32 = target.float() / (cfg["out_dims"] - 1)
    loss64, g64 = _loss_and_grads(sd, cfg, x32.double(), target, False)
    lossem, gem = _loss_and_grads(sd, cfg, x32.double(), target, True)

    model = P.set_conv_backend(copy.deepcopy(c["model"]), "hip").to(dev)
    nll = P.nll(model, x32.to(dev), target.to(dev), head="hip")
    loss = nll.mean()
    loss.backward()
    rows = [("loss", abs(float(loss.detach()) - loss64), abs(lossem - loss64))]
    for name, p in model.named_parameters():
        assert (p.grad is not None) == (name in g64), name
        if p.grad is not None:
            rows.append((name, float((p.grad.cpu().double() - g64[name]).abs().max()), float((gem[name] - g64[name]).abs().max())))
    worst = max(rows[1:], key=lambda r: r[1] / r[2] if r[2] > 0 else float("inf"))
    for label, (n, e, yd) in (("loss", rows[0]), ("worst gradient: " + worst[0], worst)):
        print("%-60s %.3e / %.3e  %5.2f" % (label, e, yd, e / yd if yd > 0 else float("inf")))
    for n, e, yd in rows:
        assert e <= HR.LOOSE_FACTOR * yd, (n, e, yd)

    # the head alone: against float64 on the (bf16-rounded) features the device computed
    with torch.no_grad():
        f = model.features(x32.to(dev)).cpu()
    w, b = model.conv4.weight.detach().cpu(), model.conv4.bias.detach().cpu()
    ref, yard = HR.reference(f, w, b, target, None, cfg["data_channels"], keys=("nll",))
    _report("head on the device's features", {"nll": HR.tight_ratio(nll.detach().cpu(), ref["nll"], yard["nll"])}, HR.GATE_FACTOR)


# ------------------------------------------------------------------------------------------------------ training
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_training(gated):
    import multimodal_vae_amd.pixelcnn as P
    import multimodal_vae_amd.train_pixelcnn as T
    dev = _dev()
    V = 8
    data = T.preprocess(T.synthetic_images(16, 1, 8, seed=3), V)
    torch.manual_seed(21)
    model = (P.GatedPixelCNN if gated else P.PixelCNN)(n_blocks=1, data_channels=1, hid_dims=16, out_dims=V)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    cfg = R.make_cfg(gated, 1, 1, 16, V)
    target = (data * (V - 1)).long()
    with torch.no_grad():
        yard = abs(float(HR.model_nll(sd, cfg, data.double(), target, True).mean()) - float(HR.model_nll(sd, cfg, data.double(), target, False).mean()))
        loss_torch = float(P.cross_entropy_by_dim(copy.deepcopy(model).to(dev)(data.to(dev)), target.to(dev)))
    model = P.set_conv_backend(model, "hip").to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    losses = [T.train_step(model, opt, data.to(dev), V, head="hip")[0] for _ in range(30)]
    ratio = abs(losses[0] - loss_torch) / yard if yard > 0 else float("inf")
    print("%s: step 0 %.6f (torch head %.6f, |difference| %.2e / loss yardstick %.2e  %.2f; gate 2), step 29 %.6f"
          % ("gated" if gated else "plain", losses[0], loss_torch, abs(losses[0] - loss_torch), yard, ratio, losses[-1]))
    assert abs(losses[0] - loss_torch) <= HR.LOOSE_FACTOR * yard
    assert losses[-1] < losses[0]


# ------------------------------------------------------------------------------------------------------ evaluation
def test_evaluate_nll_pixelcnn(tmp_path):
    import multimodal_vae_amd.evaluate as E
    import multimodal_vae_amd.pixelcnn as P
    import multimodal_vae_amd.train_pixelcnn as T
    _dev()
    C, H, W, V, hid = 3, 6, 9, 8, 16
    torch.manual_seed(5)
    model = R.scale_weights(P.GatedPixelCNN(n_blocks=1, data_channels=C, hid_dims=hid, out_dims=V), True, 5)
    with torch.no_grad():                                            # the head's operands exact in bf16 (see the docstring)
        model.conv2.weight.zero_()
        model.conv2.bias.copy_(HR.round_bf16(model.conv2.bias * 4))
        model.conv4.weight.copy_(HR.round_bf16(model.conv4.weight))
    path = str(tmp_path / "checkpoint.pth.tar")
    torch.save({"state_dict": model.state_dict(), "gated": True, "n_blocks": 1, "data_channels": C, "hid_dims": hid, "out_dims": V,
                "height": H, "width": W}, path)
    common = ["nll_pixelcnn", path, "--synthetic", "20", "--batch_size", "8"]
    hip = E.main(common + ["--head", "hip", "--cuda", "--json", str(tmp_path / "hip.json")])
    ref = E.main(common + ["--head", "torch", "--json", str(tmp_path / "torch.json")])
    assert json.load(open(str(tmp_path / "hip.json"))) == hip and hip["head"] == "hip" and ref["head"] == "torch"

    # the tight per-element gate of this head, summed over an image
    images = T.synthetic_images(20, C, max(H, W), 0)[:, :, :H, :W].contiguous()
    x = T.preprocess(images, V)
    target = (x * (V - 1)).long()
    with torch.no_grad():
        f = model.features(x)
    assert torch.equal(HR.round_bf16(f), f) and float(f.max()) > 0
    _, yard = HR.reference(f, model.conv4.weight.detach(), model.conv4.bias.detach(), target, None, C, keys=("nll",))
    gate = C * H * W * HR.GATE_FACTOR * yard["nll"]
    a, b = torch.tensor(hip["per_image_nll"], dtype=torch.float64), torch.tensor(ref["per_image_nll"], dtype=torch.float64)
    err = float((a - b).abs().max())
    print("evaluation: per-image |hip - torch| %.3e, sum of the per-element gates %.3e, ratio %.3g (gate 1)" % (err, gate, err / gate))
    assert a.shape == (20,) and err <= gate
    dims = C * H * W
    for out in (hip, ref):
        assert out["n"] == 20
        assert abs(out["nll_mean"] - float(torch.tensor(out["per_image_nll"], dtype=torch.float64).mean())) <= 1e-9 * abs(out["nll_mean"])
        assert abs(out["loss"] - out["nll_mean"] / dims) <= 1e-12 and abs(out["bits_per_dim"] - out["nll_mean"] / (dims * HR.LN2)) <= 1e-12
        assert out["nll_se"] > 0
