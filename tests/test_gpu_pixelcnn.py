"""GPU tests of the one-launch incremental PixelCNN sampler (csrc/pixelcnn.hip) against float64 (tests/pixelcnn_ref.py).

The networks are causal (tests/test_cpu_pixelcnn.py: difference exactly 0), so ONE float64 forward over a finished sample gives the
logits every sampling step saw; no trajectory has to be followed.

Logits gate: 8 x the yardstick, the yardstick being max |fp32 torch CPU forward - float64 forward| on the same image.  The margin
covers another summation order over taps and MFMA blocks and the device's tanhf / expf against the host's.
Draws: each level must equal the inverse-CDF draw from the float64 softmax and the same uniform, except where the uniform lies within
delta = 4 x gate of a float64 CDF boundary (a logit error e moves a CDF value by less than e^{2e} - 1 ~ 2e: twice that).  The share
left out is computed from the reference alone and must be <= 3 %.  Integer levels are compared, never image floats.
tests/test_cpu_pixelcnn.py shows that the logits gate sees a dropped tap, a shifted column, a shifted ring row, a missing mask, a
bias dropped at a border, a swapped channel interleave, a dropped residual and a dropped x_to_h.

MEASURED (error of the kernel's logits / yardstick per case; `pytest -s` prints them): see the table below.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pixelcnn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

MEASURED = """
error of the kernel's logits / yardstick (= error of the fp32 torch forward on the CPU), both against float64, and their ratio; the
gate is 8 x the yardstick.  MI355X:
forced plain-b0-c1-h16-v2-B1-1x1               3.109e-08 / 5.831e-08   0.53
forced plain-b1-c3-h48-v8-B15-1x6              1.861e-07 / 2.940e-07   0.63
forced plain-b3-c1-h16-v256-B16-5x1            2.120e-07 / 2.330e-07   0.91
forced plain-b3-c3-h48-v256-B17-6x9            3.298e-07 / 4.225e-07   0.78
forced plain-b1-c3-h16-v8-B17-9x5              2.691e-07 / 2.782e-07   0.97
forced plain-b1-c1-h128-v8-B16-4x4             5.141e-07 / 4.854e-07   1.06
forced gated-b0-c1-h16-v2-B1-1x1               4.029e-08 / 7.153e-08   0.56
forced gated-b1-c3-h48-v8-B15-1x6              1.242e-06 / 1.180e-06   1.05
forced gated-b3-c3-h16-v256-B16-5x1            9.679e-07 / 9.596e-07   1.01
forced gated-b3-c1-h48-v2-B17-6x9              4.319e-06 / 3.430e-06   1.26
forced gated-b1-c3-h16-v8-B17-9x5              3.037e-06 / 2.141e-06   1.42
forced gated-b1-c1-h128-v8-B16-4x4             1.981e-06 / 1.628e-06   1.22
free plain-b0-c1-h16-v2-B1-1x1                 3.109e-08 / 5.831e-08   0.53
free plain-b1-c3-h48-v8-B15-1x6                2.555e-07 / 2.961e-07   0.86
free plain-b3-c1-h16-v256-B16-5x1              2.219e-07 / 2.355e-07   0.94
free plain-b3-c3-h48-v256-B17-6x9              3.235e-07 / 4.525e-07   0.71
free plain-b1-c3-h16-v8-B17-9x5                2.589e-07 / 2.702e-07   0.96
free plain-b1-c1-h128-v8-B16-4x4               4.202e-07 / 5.053e-07   0.83
free gated-b0-c1-h16-v2-B1-1x1                 4.029e-08 / 7.153e-08   0.56
free gated-b1-c3-h48-v8-B15-1x6                1.180e-06 / 1.478e-06   0.80
free gated-b3-c3-h16-v256-B16-5x1              8.068e-07 / 1.038e-06   0.78
free gated-b3-c1-h48-v2-B17-6x9                3.537e-06 / 2.550e-06   1.39
free gated-b1-c3-h16-v8-B17-9x5                2.727e-06 / 2.567e-06   1.06
free gated-b1-c1-h128-v8-B16-4x4               1.857e-06 / 2.229e-06   0.83
complete W plain-b3-c3-h48-v256-B17-6x9        3.363e-07 / 5.039e-07   0.67
complete W plain-b1-c3-h16-v8-B17-9x5          2.608e-07 / 2.301e-07   1.13
complete W plain-b1-c1-h128-v8-B16-4x4         4.244e-07 / 4.605e-07   0.92
complete W gated-b3-c1-h48-v2-B17-6x9          3.915e-06 / 2.919e-06   1.34
complete W gated-b1-c3-h16-v8-B17-9x5          3.145e-06 / 2.481e-06   1.27
complete W gated-b1-c1-h128-v8-B16-4x4         2.031e-06 / 2.136e-06   0.95
complete 2W+3 plain-b3-c3-h48-v256-B17-6x9     3.375e-07 / 5.139e-07   0.66
complete 2W+3 plain-b1-c3-h16-v8-B17-9x5       2.384e-07 / 3.282e-07   0.73
complete 2W+3 plain-b1-c1-h128-v8-B16-4x4      4.989e-07 / 4.854e-07   1.03
complete 2W+3 gated-b3-c1-h48-v2-B17-6x9       2.904e-06 / 2.730e-06   1.06
complete 2W+3 gated-b1-c3-h16-v8-B17-9x5       2.355e-06 / 3.360e-06   0.70
complete 2W+3 gated-b1-c1-h128-v8-B16-4x4      2.583e-06 / 2.507e-06   1.03
fresh plain                                    3.158e-07 / 2.488e-07   1.27
fresh gated                                    2.203e-06 / 3.156e-06   0.70
The largest ratio is 1.42.  Share of draws left out (uniform within 4 x gate of a float64 CDF boundary): at most 2.08 % (the gated
model at 256 levels); every compared level equalled the float64 draw.
"""

TILE = 16                                                          # checked against mmvae_pixelcnn_geometry in a test
# (n_blocks, channels, hid, levels, B, H, W): per model every (H, W) of {(1, 1), (1, 6), (5, 1), (6, 9), (9, 5)}, C of {1, 3}, V of
# {2, 8, 256}, hid of {16, 48}, n_blocks of {0, 1, 3} and B of {1, TILE - 1, TILE, TILE + 1} appears; and one 4 x 4 case at hid 128.
# The share of draws left out is about 2 delta (V - 1) = 64 x 8 x yardstick x (V - 1): with 256 levels it stays below 3 % only while
# the yardstick is below 1.8e-6, which the gated model (larger logits) meets on the one-column image and not on the 6 x 9 one.
# A consequence: the completion cases (LARGE) leave the 5 x 1 image out, so the gated model's draws at 256 levels, and the gated
# model at 3 channels with 3 blocks, are never checked on an image wider than one column or with 0 < n_given < H W.
PLAIN = [(0, 1, 16, 2, 1, 1, 1), (1, 3, 48, 8, TILE - 1, 1, 6), (3, 1, 16, 256, TILE, 5, 1), (3, 3, 48, 256, TILE + 1, 6, 9),
         (1, 3, 16, 8, TILE + 1, 9, 5), (1, 1, 128, 8, TILE, 4, 4)]
GATED = [(0, 1, 16, 2, 1, 1, 1), (1, 3, 48, 8, TILE - 1, 1, 6), (3, 3, 16, 256, TILE, 5, 1, 1), (3, 1, 48, 2, TILE + 1, 6, 9),
         (1, 3, 16, 8, TILE + 1, 9, 5), (1, 1, 128, 8, TILE, 4, 4)]                           # (a trailing 8th entry: the seed)
CASES = [(False,) + s for s in PLAIN] + [(True,) + s for s in GATED]
LARGE = [c for c in CASES if c[6] * c[7] >= 2 * c[7] + 3 + 1]      # room for n_given = 2 W + 3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _ids(c):
    return "%s-b%d-c%d-h%d-v%d-B%d-%dx%d" % (("gated" if c[0] else "plain",) + tuple(c[1:8]))


def _model(c, dev):
    """the case's model on the device: a copy, so that the shared one stays as constructed (no forward ever ran on it)"""
    import copy
    return copy.deepcopy(c["model"]).to(dev)


def _generate(c, dev, **kw):
    from multimodal_vae_amd.pixelcnn import generate
    B, _, H, W = c["uniforms"].shape
    kw.setdefault("uniforms", c["uniforms"].to(dev))
    if "given" in kw:
        kw["given"] = kw["given"].to(dev)
    out = generate(_model(c, dev), B, H, W, return_logits=True, **kw)
    assert out.levels.dtype == torch.int64 and out.image.dtype == torch.float32 and out.logits.dtype == torch.float32
    assert out.levels.shape == c["uniforms"].shape and out.logits.shape == (B, c["cfg"]["out_dims"], c["cfg"]["data_channels"], H, W)
    # (integer levels are what is compared: v / (V - 1) differs in the last bit between a division and a multiply by the reciprocal)
    scale = c["cfg"]["out_dims"] - 1
    assert torch.equal((out.image * scale).round().long(), out.levels) and float((out.image - out.levels.float() / scale).abs().max()) < 2e-7
    return out


def _check_logits(label, c, levels, logits):
    """-> (float64 logits on `levels`, gate); asserts the kernel's logits are within the gate"""
    l64 = R.forward64(c["sd"], c["cfg"], levels)
    yard = R.yardstick(c["sd"], c["cfg"], levels, l64)
    err = float((logits.double().cpu() - l64).abs().max())
    print("PIXELCNN %-44s error %.3e  yardstick %.3e  ratio %.2f  logit std %.2f" % (label, err, yard, err / yard, float(l64.std())))
    assert err <= R.GATE_FACTOR * yard, (label, err, yard)
    return l64, R.GATE_FACTOR * yard


def _check_draws(label, c, out, n_given, given=None):
    levels = out.levels.cpu()
    B, C, H, W = levels.shape
    l64, gate = _check_logits(label, c, levels, out.logits)
    drawn = torch.arange(H * W).view(1, 1, H, W).expand(B, C, H, W) >= n_given
    if given is not None:
        assert torch.equal(levels[~drawn], given[~drawn])
    far = R.boundary_distance(l64, c["uniforms"]) > R.DELTA_FACTOR * gate
    left_out = 1.0 - float(far[drawn].double().mean())
    print("PIXELCNN %-44s left out %.3f %%" % (label, 100 * left_out))
    assert left_out <= 0.03, (label, left_out)
    want = R.draw(l64, c["uniforms"])
    keep = drawn & far
    assert torch.equal(levels[keep], want[keep]), (label, int((levels[keep] != want[keep]).sum()))


def test_geometry():
    from multimodal_vae_amd.pixelcnn import pixelcnn_geometry
    assert pixelcnn_geometry() == (TILE, 128, 64)


@pytest.mark.parametrize("c", CASES, ids=_ids)
def test_teacher_forced(c):
    dev = _dev()
    k = R.case(*c)
    H, W = c[6], c[7]
    out = _generate(k, dev, given=k["given"], n_given=H * W)
    assert torch.equal(out.levels.cpu(), k["given"])
    _check_logits("forced " + _ids(c), k, k["given"], out.logits)


@pytest.mark.parametrize("c", CASES, ids=_ids)
def test_free_sampling(c):
    k = R.case(*c)
    _check_draws("free " + _ids(c), k, _generate(k, _dev()), 0)


@pytest.mark.parametrize("c", LARGE, ids=_ids)
@pytest.mark.parametrize("rule", ["W", "2W+3"])
def test_completion(c, rule):
    k = R.case(*c)
    W = c[7]
    n_given = W if rule == "W" else 2 * W + 3
    out = _generate(k, _dev(), given=k["given"], n_given=n_given)
    _check_draws("complete %s %s" % (rule, _ids(c)), k, out, n_given, k["given"])


@pytest.mark.parametrize("gated", [False, True])
def test_bitwise(gated):
    """two calls give identical bits; a batch of 19 equals the same rows run as batches of 16 and 3"""
    from multimodal_vae_amd.pixelcnn import generate
    dev = _dev()
    k = R.case(gated, 1, 3, 48, 8, 19, 6, 9)
    model, u, g = _model(k, dev), k["uniforms"].to(dev), k["given"].to(dev)
    a = generate(model, 19, 6, 9, uniforms=u, given=g, n_given=5, return_logits=True)
    b = generate(model, 19, 6, 9, uniforms=u, given=g, n_given=5, return_logits=True)
    assert torch.equal(a.levels, b.levels) and torch.equal(a.logits.view(torch.int32), b.logits.view(torch.int32))
    for lo, hi in ((0, 16), (16, 19)):
        p = generate(model, hi - lo, 6, 9, uniforms=u[lo:hi].contiguous(), given=g[lo:hi].contiguous(), n_given=5, return_logits=True)
        assert torch.equal(p.levels, a.levels[lo:hi])
        assert torch.equal(p.logits.view(torch.int32), a.logits[lo:hi].view(torch.int32))


@pytest.mark.parametrize("gated", [False, True])
def test_masks_are_honoured_without_a_forward(gated):
    """a freshly constructed model: no forward has zeroed the masked weights, the packing must"""
    dev = _dev()
    k = R.case(gated, 1, 3, 16, 8, 3, 6, 9, 5)
    model = _model(k, dev)
    if not gated:
        assert not torch.equal(model.conv1.weight, model.conv1.weight * model.conv1.mask)
    from multimodal_vae_amd.pixelcnn import generate
    out = generate(model, 3, 6, 9, uniforms=k["uniforms"].to(dev), given=k["given"].to(dev), n_given=54, return_logits=True)
    if not gated:
        assert not torch.equal(model.conv1.weight, model.conv1.weight * model.conv1.mask)      # and generate leaves them alone
    assert torch.equal(out.levels.cpu(), k["given"])
    _check_logits("fresh %s" % ("gated" if gated else "plain"), k, k["given"], out.logits)


def test_refusals_do_not_launch():
    import multimodal_vae_amd.pixelcnn as P
    from multimodal_vae_amd import MMVAEError
    dev = _dev()
    good = P.PixelCNN(1, 1, 16, 8).to(dev)
    u = torch.rand(2, 1, 4, 4, device=dev)
    g = torch.zeros(2, 1, 4, 4, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for cls in (P.PixelCNN, P.GatedPixelCNN):
        with pytest.raises(MMVAEError):
            P.generate(cls(1, 1, 24, 8).to(dev), 2, 4, 4)
        with pytest.raises(MMVAEError):
            P.generate(cls(1, 2, 16, 8).to(dev), 2, 4, 4)
        with pytest.raises(MMVAEError):
            P.generate(cls(1, 1, 16, 8).to(dev), 2, 65, 4)
        with pytest.raises(MMVAEError):
            P.generate(cls(1, 1, 16, 8), 2, 4, 4)                  # a CPU model
    for bad in (u.cpu(), u.double(), torch.rand(2, 1, 4, 5, device=dev), torch.rand(3, 1, 4, 4, device=dev)):
        with pytest.raises(MMVAEError):
            P.generate(good, 2, 4, 4, uniforms=bad)
    with pytest.raises(MMVAEError):
        P.generate(good, 2, 4, 4, uniforms=u, given=g, n_given=17)
    with pytest.raises(MMVAEError):
        P.generate(good, 2, 4, 4, uniforms=u, given=g.cpu(), n_given=3)
    with pytest.raises(MMVAEError):
        P.generate(good, 2, 4, 4, uniforms=u, given=g.float(), n_given=3)
    # the C boundary refuses the same before it launches: the outputs stay as they were
    from multimodal_vae_amd._lib import call, ptr
    import ctypes as C
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lev = torch.full((2, 1, 4, 4), 7, dtype=torch.int32, device=dev)
    img = torch.full((2, 1, 4, 4), 7.0, device=dev)
    packed = P.pack_weights(good)
    need = call("mmvae_pixelcnn_workspace_bytes", 0, 1, 1, 16, 8, 2, 4, 4)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    for cfg, shape, n_given, ws_bytes in (((0, 1, 1, 24, 8), (2, 4, 4), 0, need), ((0, 1, 2, 16, 8), (2, 4, 4), 0, need),
                                          ((0, 1, 1, 16, 8), (2, 65, 4), 0, need), ((0, 1, 1, 16, 8), (2, 4, 4), 17, need),
                                          ((0, 1, 1, 16, 8), (2, 4, 4), 0, need - 1), ((0, 16, 1, 16, 8), (2, 4, 4), 0, need),
                                          ((0, 1, 1, 16, 257), (2, 4, 4), 0, need), ((0, 1, 1, 16, 8), (0, 4, 4), 0, need)):
        with pytest.raises(MMVAEError):
            call("mmvae_pixelcnn_sample", *cfg, ptr(packed), ptr(ws), ws_bytes, *shape, ptr(u), ptr(lev), n_given, ptr(lev), ptr(img), None, s)
    torch.cuda.synchronize()
    assert bool((lev == 7).all()) and bool((img == 7.0).all())


def test_sample_pixelcnn_round_trip(tmp_path):
    import multimodal_vae_amd.pixelcnn as P
    from multimodal_vae_amd import evaluate
    _dev()
    k = R.case(True, 1, 3, 16, 8, 4, 6, 9)
    P.save_checkpoint(dict(k["cfg"], state_dict=k["model"].state_dict(), best_loss=0.0, optimizer={}, height=6, width=9), False,
                      folder=str(tmp_path))
    im = torch.randint(0, 256, (3, 6, 9), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    torch.save(im, str(tmp_path / "im.pt"))
    evaluate._main(["sample_pixelcnn", str(tmp_path / "checkpoint.pth.tar"), "--n_samples", "4", "--complete", str(tmp_path / "im.pt"),
                    "--rows", "2", "--seed", "1", "--out", str(tmp_path / "out")])
    got = torch.load(str(tmp_path / "out" / "sample_image.pt"))
    assert got.shape == (4, 3, 6, 9) and got.dtype == torch.float32
    lev = (got * 7).round().long()
    assert torch.equal(lev.float() / 7, got) and int(lev.min()) >= 0 and int(lev.max()) <= 7
    kept = torch.from_numpy(P.quantisize(im.float().div(255.0).numpy(), 8)).long()
    assert torch.equal(lev[:, :, :2], kept[:, :2].expand(4, -1, -1, -1))
    assert not torch.equal(lev[0, :, 2:], lev[1, :, 2:])           # the rest is drawn per sample
