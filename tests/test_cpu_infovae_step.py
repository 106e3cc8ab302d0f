"""CPU tests of the fused COCO InfoVAE step's Python side and of its test instrument (no GPU):

  * tests/infovae_step_ref.py equals the reference's ``loss_function`` (coco/train_infovae.py:44-55) on a tiny case;
  * each fault the instrument can inject breaks the gates tests/test_gpu_infovae_step.py applies, at every shape that file runs, while
    the instrument's own fp32-vs-float64 error -- the size of an honest deviation -- stays far inside them;
  * the ctypes layout of mmvae_infovae_step_io against the header (as tests/test_cpu_imageonly.py does for mmvae_image_step_io);
  * ``FusedInfoVAE`` has ``InfoVAE``'s state-dict keys, in both directions;
  * ``train_infovae --help`` lists ``--fused`` and the defaults are the reference's.
"""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import pytest
import torch

import imageonly_ref as IR
import infovae_step_ref as IV
import mmd_ref as MR
from gradcheck import check_gradients

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the weights of the GPU test of the step (tests/test_gpu_infovae_step.py STEP_LAMBDAS): lambda_mmd != 1 so that a step that ignores it shows
STEP_LAMBDAS = dict(lambda_x=1.0, lambda_mmd=2.0, kl_lambda=1e-3)
MMD_ONLY_LAMBDAS = dict(lambda_x=0.0, lambda_mmd=1.0, kl_lambda=0.0)
LOSS_TOL, TENSOR_TOL, TOTAL_TOL = 1e-3, 4.5e-2, 2e-3


def test_oracle_is_the_references_loss_function():
    """lambda_x = lambda_mmd = 1, kl_lambda = 0 is BCE + MMD of coco/train_infovae.py:44-55, x = the prior samples, y = z."""
    B, D = 3, 8
    p = IV.params(D)
    image, eps, ts = IV.inputs(B, D)
    with torch.no_grad():
        loss, parts, (recon, mu, logvar, z) = IV.step_loss(p, image, True, eps, ts)
        want = IV.reference_loss_function(recon, image.double(), z, ts.double())
        assert float(loss) == float(want)
        assert torch.equal(z, mu + eps.double() * torch.exp(0.5 * logvar))
        # compute_kernel / compute_mmd as written (coco/model.py:385-402), against the float64 formula with analytic gradient
        ref = MR.mmd64(ts, z)
        assert abs(float(parts["mmd"]) - float(ref["terms"][3])) < 1e-14
        # eval mode: z = mu
        _, _, (_, mu_e, _, z_e) = IV.step_loss(p, image, False, None, ts)
        assert torch.equal(z_e, mu_e)
        # the weights
        l2, parts2, _ = IV.step_loss(p, image, True, eps, ts, lambda_x=0.5, lambda_mmd=3.0, kl_lambda=0.25)
        assert abs(float(l2) - (0.5 * float(parts2["bce"]) + 3.0 * float(parts2["mmd"]) + 0.25 * float(parts2["kl"]) / B)) < 1e-14
    # autograd of the formulation gives the analytic dMMD/dz
    zl = z.clone().requires_grad_(True)
    MR.formulation_mmd(ts.double(), zl).backward()
    assert float((zl.grad - ref["dy"]).abs().max()) <= 1e-12 * float(ref["dy"].abs().max()) + 1e-18


@functools.lru_cache(maxsize=None)
def _case(B, D, mmd_only, fault, fp32=False):
    """loss, MMD and the image half's gradients of one training step of the instrument"""
    lam = MMD_ONLY_LAMBDAS if mmd_only else STEP_LAMBDAS
    p = IV.params(D, torch.float32 if fp32 else torch.float64, requires_grad=True)
    image, eps, ts = IV.inputs(B, D)
    loss, parts, _ = IV.step_loss(p, image, True, eps, ts, fault=fault, **lam)
    loss.backward()
    grads = {n: (None if p[n].grad is None else p[n].grad.double()) for n in IR.image_names("coco", D)}
    return float(loss.detach()), float(parts["mmd"].detach()), grads


def _deviation(B, D, mmd_only, fault, fp32=False):
    """(loss rel, MMD value error on the scale of test_gpu_mmd's value gate, worst gradient tensor, total gradient norm rel)"""
    l0, m0, g0 = _case(B, D, mmd_only, None)
    l1, m1, g1 = _case(B, D, mmd_only, fault, fp32)
    live = [n for n in g0 if g0[n] is not None]          # (lambda_x = 0: the decoder has no gradient at all)
    assert all(g1[n] is None for n in g0 if g0[n] is None)
    worst, tot = check_gradients([(n, g1[n], g0[n]) for n in live], float("inf"), None)
    return abs(l1 - l0) / abs(l0), abs(m1 - m0), worst, tot


SHAPES = [(B, D, False) for B, D in IV.STEP_SHAPES] + [(B, D, True) for B, D in IV.MMD_ONLY_SHAPES]


@pytest.mark.parametrize("B,D,mmd_only", SHAPES)
def test_every_fault_breaks_the_gpu_gates(B, D, mmd_only):
    """The honest deviation (the instrument at fp32 against itself at float64) is below 1 % of every gate.  Every fault is beyond twice
    the per-tensor gradient gate at every shape -- the gate that is there for it (the total-norm gate is dominated by the decoder's
    gradients, and a misdirected gradient can have the right norm: it is printed, not asserted).  The sign of the cross term is also beyond the loss gate and
    moves the MMD slot by more than 1e-4 (the value gate of the slots is a few 1e-8, tests/test_gpu_mmd.py); a dropped or misdirected
    gradient leaves every value as it is, only the gradient gates can see it.  ``lambda_ignored`` cannot show where lambda_mmd = 1
    (the MMD-alone cases): it is checked at the step's weights."""
    l, m, worst, tot = _deviation(B, D, mmd_only, None, fp32=True)
    print("(%d, %d, mmd_only=%d): honest fp32 deviation loss %.2e mmd %.2e worst tensor %.2e total %.2e" % (B, D, mmd_only, l, m, worst, tot))
    assert worst <= 1e-2 * TENSOR_TOL and tot <= 1e-2 * TOTAL_TOL and m <= 1e-6
    # (with the MMD alone the loss IS the MMD, 4e-4 at (65, 100): a difference of three means near 1, whose fp32 rounding is 5e-4 of it.
    #  The GPU test has no relative loss gate there; the four values are gated on the scale of the means, as tests/test_gpu_mmd.py does)
    assert mmd_only or l <= 1e-2 * LOSS_TOL
    for fault in IV.FAULTS:
        if fault == "lambda_ignored" and mmd_only:
            continue
        l, m, worst, tot = _deviation(B, D, mmd_only, fault)
        print("    %-17s loss %.2e mmd %.2e worst tensor %.2e total %.2e" % (fault, l, m, worst, tot))
        assert worst > 2 * TENSOR_TOL, (fault, worst)
        if fault == "cross_sign":
            assert l > 2 * LOSS_TOL and m > 1e-4, (l, m)
        if fault in ("no_mmd_grad", "grad_for_samples"):
            assert l == 0.0 and m == 0.0          # (only the gradient gates can see these)


def test_ctypes_infovae_step_io_layout_matches_the_header(tmp_path):
    from multimodal_vae_amd import _lib, coco
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    exe = str(tmp_path / "infovae_step_layout")
    subprocess.run([cc, "-std=c99", "-pedantic-errors", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "infovae_step_layout.c"), "-o", exe], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    cls_name, size, *fields = lines[0].split()
    cls = getattr(_lib, cls_name)
    assert cls is _lib.InfoVAEStepIO and cls.__doc__.split()[-1] == "mmvae_infovae_step_io"
    assert C.sizeof(cls) == int(size)
    assert [f.split(":")[0] for f in fields] == [n for n, _ in cls._fields_]
    for f in fields:
        n, o = f.split(":")
        assert getattr(cls, n).offset == int(o), n
    # every field of mmvae_image_step_io leads the struct, at the same offsets
    _, _, *img_fields = lines[1].split()
    assert img_fields == fields[:len(img_fields)] and len(fields) == len(img_fields) + 3
    assert [n for n, _ in cls._fields_[-3:]] == ["true_samples", "lambda_mmd", "z"]
    hdr = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    body = re.search(r"\{([^{}]*)\}\s*mmvae_infovae_step_io;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)(?:\[\d+\])?\s*[;,]", body) == [n for n, _ in cls._fields_]
    # the named loss slots and the Philox stream of the prior samples
    assert lines[2].split() == ["slots", "12", "13", "14", "15", "stream", str(coco.TRUE_SAMPLES_STREAM)]
    from multimodal_vae_amd.core import InfoVAEStepOutputs
    assert (InfoVAEStepOutputs.MMD_SLOTS.start, InfoVAEStepOutputs.MMD_SLOTS.stop) == (12, 16)
    # every new entry point of the header has a ctypes prototype of the right length
    for fn in re.findall(r"\b(mmvae_coco_infovae_step\w*|mmvae_mmd_dy\w*)\(", hdr):
        assert fn in _lib.SIGNATURES, fn
    assert len(_lib.SIGNATURES["mmvae_mmd_dy"][1]) == 12 and len(_lib.SIGNATURES["mmvae_coco_infovae_step"][1]) == 5
    # the shared filler takes lambda_mmd from the engine, as lambda_x
    scalars, per_call, lambdas = __import__("multimodal_vae_amd.core", fromlist=["_io_layout"])._io_layout(cls)
    assert [n for n, _ in scalars] == ["enc_dropout", "kl_lambda", "lambda_x", "lambda_mmd"] and per_call == ("defer_unpack",) and lambdas == ()


def test_the_library_refuses_on_the_host():
    """No GPU call is reached: an unbound plan, a latent size outside the plan's range, a null argument."""
    from multimodal_vae_amd import _lib
    lib = _lib.load()
    h = lib.mmvae_coco_create_t(20, 4, 1)
    assert h
    try:
        need = lib.mmvae_coco_infovae_step_workspace_bytes(h)
        assert need > lib.mmvae_coco_image_step_workspace_bytes(h) and need % 16 == 0
        extra = need - (lib.mmvae_coco_image_step_workspace_bytes(h) + 15) // 16 * 16
        assert extra == (lib.mmvae_mmd_dy_workspace_bytes(4, 4, 20) + 15) // 16 * 16 + 2 * ((4 * 20 * 4 + 15) // 16 * 16)
        for name in (b"infovae_step:mmd_ws", b"infovae_step:dz_mmd", b"infovae_step:true_samples"):
            off = lib.mmvae_coco_debug_offset(h, name)
            assert lib.mmvae_coco_image_step_workspace_bytes(h) <= off < need and off % 16 == 0, name
        assert lib.mmvae_coco_debug_offset(h, b"infovae_step:nothing") == -1
        io = _lib.InfoVAEStepIO()
        assert lib.mmvae_coco_infovae_step(h, C.byref(io), 1, 1, None) != 0          # an unbound plan
        assert b"bind" in lib.mmvae_last_error()
        assert lib.mmvae_coco_infovae_step(h, None, 1, 1, None) != 0 and b"null" in lib.mmvae_last_error()
    finally:
        lib.mmvae_coco_destroy(h)
    for D in (0, 2, 126, 128, 200):
        assert not lib.mmvae_coco_create_t(D, 4, 1), D
        assert b"4..124" in lib.mmvae_last_error()
    # the y-only sweep's workspace: the kernel sums of mmvae_mmd, and gradient partials for y's rows alone
    rt = 64
    for nx, ny, D in ((65, 65, 100), (7, 130, 20), (128, 128, 100), (1, 1, 4)):
        rtx, rty, tx, ty, sx, sy = MR.split_rule(nx, ny, rt, 32)
        assert lib.mmvae_mmd_dy_workspace_bytes(nx, ny, D) == (sx + sy) * ((rtx + rty) * rt + rty * rt * D) * 8
        assert lib.mmvae_mmd_dy_workspace_bytes(nx, ny, D) < lib.mmvae_mmd_workspace_bytes(nx, ny, D)
    assert lib.mmvae_mmd_dy_workspace_bytes(0, 4, 4) == 0 and lib.mmvae_mmd_dy_workspace_bytes(4, 4, 257) == 0
    p = C.c_void_p(64)
    for args, msg in (([None, 2, p, 2, 3, p, 1 << 20, 1.0, p, None, 1, None], b"null"),
                      ([p, 2, p, 2, 3, p, 1 << 20, 1.0, p, None, 0, None], b"grad_y_only"),
                      ([p, 0, p, 2, 3, p, 1 << 20, 1.0, p, None, 1, None], b"n_x = 0"),
                      ([p, 2, p, 2, 3, p, lib.mmvae_mmd_dy_workspace_bytes(2, 2, 3) - 1, 1.0, p, None, 1, None], b"workspace too small")):
        assert lib.mmvae_mmd_dy(*args) != 0 and msg in lib.mmvae_last_error(), (msg, lib.mmvae_last_error())


@pytest.mark.parametrize("D", [20, 100])
def test_fused_infovae_has_infovaes_keys(D):
    """Key lists without a device, as tests/test_cpu_imageonly.py builds them for ImageVAE: the same keys in the same order, each way
    loads strict, one core under the plan's image_ names."""
    from multimodal_vae_amd import coco as M
    fused, plain = M.FusedInfoVAE(D), M.InfoVAE(D)
    keys = list(fused.state_dict().keys())
    assert keys == list(plain.state_dict().keys()) == IR.state_dict_keys("coco", D)
    assert all(k.startswith(("encoder.", "decoder.")) for k in keys)
    sd = {k: torch.full_like(v, 0.5) if v.is_floating_point() else v + 3 for k, v in plain.state_dict().items()}
    fused.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in fused.state_dict().items())
    plain2 = M.InfoVAE(D)
    plain2.load_state_dict(fused.state_dict(), strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in plain2.state_dict().items())
    assert fused._core.prefix == "image_" and fused.encoder._mmvae_root() is fused and fused.decoder._mmvae_root() is fused
    assert [n for n, _ in fused.named_children()] == ["encoder", "decoder"] and fused.n_latents == D
    for meth in ("encode", "reparametrize", "decode", "forward"):
        assert callable(getattr(fused, meth))
    assert not isinstance(plain, M.FusedInfoVAE) and type(plain).__mro__[1] is not M.ImageVAE       # coco.InfoVAE itself is not touched
    assert M.InfoVAETrainer.ENGINE.__name__ == "FusedInfoVAEStep" and (M.InfoVAETrainer.LR, M.InfoVAETrainer.KL_LAMBDA) == (1e-4, 0.0)


def test_driver_lists_fused_and_keeps_the_references_defaults(capsys):
    from multimodal_vae_amd import train_infovae as T
    a = T.build_parser().parse_args([])
    assert (a.n_latents, a.batch_size, a.epochs, a.lr, a.log_interval, a.cuda, a.fused) == (100, 128, 10, 1e-4, 10, False, False)
    assert T.build_parser().parse_args(["--fused"]).fused is True
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--help"])
    assert "--fused" in capsys.readouterr().out
    with pytest.raises(SystemExit):                          # no CPU fallback, on either route
        T.main(["--fused", "--synthetic", "64"])
    import inspect
    assert list(inspect.signature(T.load_checkpoint).parameters) == ["file_path", "use_cuda", "fused"]
    assert inspect.signature(T.load_checkpoint).parameters["fused"].default is False


def test_engine_refuses_other_families_and_capture():
    from multimodal_vae_amd import core
    with pytest.raises(core.MMVAEError, match="COCO has one"):
        core.FusedInfoVAEStep(type("S", (), {"API": "celeba"})(), 8)
    eng = object.__new__(core.FusedInfoVAEStep)
    with pytest.raises(core.MMVAEError, match="capture"):
        eng.capture(torch.zeros(1))
    sums = torch.arange(16.0)
    out = core.InfoVAEStepOutputs(sums, 4.0, 0.0, 1.0, 2.0)
    assert float(out.bce()) == 0.0 and float(out.mmd()) == 15.0 and out.mmd_terms().tolist() == [12.0, 13.0, 14.0, 15.0]
    assert out.lambda_mmd == 2.0 and out.passes == (True, False, False)
