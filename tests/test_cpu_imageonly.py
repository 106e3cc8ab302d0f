"""CPU tests of the uni-modal image VAE baselines (CelebA, COCO): state_dict keys, the train_imageonly driver's command line, KL
schedules and checkpoint dict, the ctypes layout of mmvae_image_step_io, and the test instrument tests/imageonly_ref.py itself."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from oracle import mmvae_ref as R
import imageonly_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("family,D", [("celeba", 100), ("celeba", 20), ("coco", 20), ("coco", 100)])
def test_state_dict_keys_are_the_references(family, D):
    """ImageVAE().state_dict() == the image half of R.param_table / R.bn_layers under encoder. / decoder. -- nothing of the second
    modality, no experts, no extra buffer."""
    import importlib
    M = importlib.import_module("multimodal_vae_amd." + family)
    vae = M.ImageVAE(D)
    keys = list(vae.state_dict().keys())
    assert keys == IR.state_dict_keys(family, D)
    assert all(k.startswith(("encoder.", "decoder.")) for k in keys)
    shapes = dict(R.param_table(family, D))
    for n, p in vae.named_parameters():
        assert tuple(p.shape) == tuple(shapes["image_" + n]), n
    assert [n for n, _ in vae.named_children()] == ["encoder", "decoder"]
    for meth in ("encode", "decode", "reparametrize", "forward"):
        assert callable(getattr(vae, meth))
    assert hasattr(vae, "weight_init") == (family == "celeba")
    # the shared core names the plan's parameters
    assert vae._core.prefix == "image_" and vae.encoder._mmvae_root() is vae and vae.decoder._mmvae_root() is vae


def test_driver_flags_and_defaults():
    from multimodal_vae_amd import train_imageonly as T
    a = T.build_parser("celeba").parse_args([])
    assert (a.n_latents, a.batch_size, a.epochs, a.lr, a.log_interval, a.cuda) == (100, 128, 10, 1e-3, 10, False)
    assert not hasattr(a, "anneal_kl")                      # celeba/train_imageonly.py has no such flag
    c = T.build_parser("coco").parse_args([])
    assert (c.n_latents, c.batch_size, c.epochs, c.lr, c.log_interval, c.cuda, c.anneal_kl) == (20, 128, 10, 1e-4, 10, False, False)
    for ns in (a, c):
        assert (ns.data, ns.synthetic, ns.out, ns.results, ns.seed) == ('./data', 0, './trained_models/image_only', './results/image_only', 1234)
    assert T.dataset_of(["--dataset", "coco", "--cuda"]) == "coco" and T.dataset_of(["--cuda"]) == "celeba"
    assert T.build_parser("coco").parse_args(["--dataset", "coco", "--anneal_kl", "--n_latents", "8"]).anneal_kl
    with pytest.raises(SystemExit):                          # no CPU fallback
        T.main(["--dataset", "celeba"])


def test_driver_kl_schedules():
    from multimodal_vae_amd import train_imageonly as T
    assert T.kl_lambdas("celeba", 12) == [1e-3] * 12
    assert T.kl_lambdas("celeba", 7, anneal_kl=True) == [1e-3] * 7
    assert T.kl_lambdas("coco", 12) == [5e-4] * 12
    # coco/train_imageonly.py:141-149: next(schedule) at epochs 1, 6, 11; an exhausted schedule keeps the last value
    assert T.kl_lambdas("coco", 17, anneal_kl=True) == [1e-5] * 5 + [1e-4] * 5 + [1e-3] * 7


def test_driver_checkpoint_dict():
    """state_dict / best_loss / n_latents / optimizer, the optimizer state over the ImageVAE's own parameters only."""
    from multimodal_vae_amd import celeba as M, train_imageonly as T

    class Engine:       # the fields image_adam_state_dict reads of a FusedImageStep
        pass
    vae = M.ImageVAE(8)
    table, off = [], 0
    for n, shape in R.param_table("celeba", 8):
        numel = 1
        for s in shape:
            numel *= s
        table.append((n, tuple(shape), off))
        off += numel
    eng = Engine()
    eng.state = type("S", (), {"table": table})()
    eng.adam_state = torch.tensor([3, 0])
    eng.exp_avg = torch.arange(off, dtype=torch.float32)
    eng.exp_avg_sq = torch.arange(off, dtype=torch.float32) * 2
    eng.lr, eng.betas, eng.eps = 1e-3, (0.9, 0.999), 1e-8
    ck = T.checkpoint_dict(vae, eng, 0.5, 8)
    assert sorted(ck) == ["best_loss", "n_latents", "optimizer", "state_dict"]
    assert list(ck["state_dict"]) == IR.state_dict_keys("celeba", 8) and ck["n_latents"] == 8 and ck["best_loss"] == 0.5
    names = IR.image_names("celeba", 8)
    opt = ck["optimizer"]
    assert len(opt["state"]) == len(names) == len(list(vae.parameters())) and opt["param_groups"][0]["params"] == list(range(len(names)))
    ref = torch.optim.Adam(vae.parameters(), lr=1e-3).state_dict()["param_groups"][0]
    assert set(ref) <= set(opt["param_groups"][0])
    offs = {n: o for n, _, o in table}
    for i, (n, p) in enumerate(zip(names, vae.parameters())):
        st = opt["state"][i]
        assert st["exp_avg"].shape == p.shape and float(st["step"]) == 3.0
        assert float(st["exp_avg"].reshape(-1)[0]) == float(offs[n]) and float(st["exp_avg_sq"].reshape(-1)[0]) == 2.0 * offs[n]
    # the attribute half of the plan is in no entry
    assert off > sum(p.numel() for p in vae.parameters())


def test_ctypes_image_step_io_layout_matches_the_header(tmp_path):
    from multimodal_vae_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    exe = str(tmp_path / "image_step_layout")
    subprocess.run([cc, "-std=c99", "-pedantic-errors", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "image_step_layout.c"), "-o", exe], check=True)
    line = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip()
    cls_name, size, *fields = line.split()
    cls = getattr(_lib, cls_name)
    assert cls.__doc__.split()[-1] == "mmvae_image_step_io"
    assert C.sizeof(cls) == int(size)
    assert [f.split(":")[0] for f in fields] == [n for n, _ in cls._fields_]
    for f in fields:
        n, o = f.split(":")
        assert getattr(cls, n).offset == int(o), n
    hdr = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    body = re.search(r"\{([^{}]*)\}\s*mmvae_image_step_io;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)(?:\[\d+\])?\s*[;,]", body) == [n for n, _ in cls._fields_]
    # every new entry point of the header has a ctypes prototype
    for fn in re.findall(r"\b(mmvae_(?:celeba|coco)_(?:image_step\w*|iw_score_image)|mmvae_latent1_\w+)\(", hdr):
        assert fn in _lib.SIGNATURES, fn


def test_instrument_is_the_image_pass_without_the_experts_epsilon():
    """tests/imageonly_ref.py against the oracle's own image-only pass, celeba_forward(image, None): the same numbers except for the
    1e-8 that ProductOfExperts adds to exp(logvar) -- invisible at ordinary log-variances, and about 1.8 at logvar = -20."""
    torch.manual_seed(0)
    D, B = 20, 3
    p = IR.params64("celeba", D)
    image = torch.rand(B, 3, 64, 64, dtype=torch.float64)
    with torch.no_grad():
        recon, mu, lv = IR.forward("celeba", dict(p), image, False)
        o = R.celeba_forward(dict(p), image, None, False)
    assert torch.equal(mu, R.celeba_image_encoder(p, image, False)[:, :D].detach())
    # eval mode: z = mu, and one expert's variance-weighted mean is mu itself (up to rounding): same reconstruction
    assert (recon - o[0]).abs().max().item() < 1e-9 and (mu - o[2]).abs().max().item() < 1e-12
    d = (lv - o[3]).abs()
    assert 0 < d.max().item() < 1e-6                  # exp(lv) ~ 1: log(exp(lv) + 1e-8) - lv ~ 1e-8 / exp(lv)
    # at logvar = -20 the experts' epsilon is larger than the variance: log(e^-20 + 1e-8) = -18.23
    p2 = dict(p)
    p2["image_encoder.classifier.3.weight"] = torch.zeros_like(p["image_encoder.classifier.3.weight"])
    b = torch.zeros(2 * D, dtype=torch.float64)
    b[D:] = -20.0
    p2["image_encoder.classifier.3.bias"] = b
    with torch.no_grad():
        _, mu2, lv2 = IR.forward("celeba", dict(p2), image, False)
        o2 = R.celeba_forward(dict(p2), image, None, False)
    assert torch.equal(lv2, torch.full_like(lv2, -20.0)) and torch.equal(mu2, torch.zeros_like(mu2))
    import math
    assert (o2[3] - math.log(math.exp(-20.0) + 1e-8)).abs().max().item() < 1e-12 and (o2[3] - lv2).min().item() > 1.7
    # and the latent formulas used by the GPU test
    eo = torch.cat((mu2, lv2), dim=1)
    m, l, z, kl = IR.latent1_fwd(eo, torch.ones(B, D), True)
    assert torch.equal(m, mu2) and torch.equal(l, lv2)
    assert torch.allclose(z, torch.full_like(z, float(torch.exp(torch.tensor(-10.0, dtype=torch.float64)))))
    assert abs(kl.item() - R.kl_sum(mu2, lv2).item()) == 0.0
