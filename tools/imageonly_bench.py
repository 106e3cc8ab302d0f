"""Step time of the uni-modal image VAE baselines (CelebA, COCO) on the one-pass fused step against the two routes a user had before it.

    python tools/imageonly_bench.py [--steps 30] [--repeats 5] [--out profiles/imageonly_bench.txt] [--small]

Per family and batch size (B = 128 for both; B = 512 for CelebA, B = 1024 for COCO) ONE training step (forward, backward, Adam) is
timed between device events on three routes, warmed up and ALTERNATED in one process (``--repeats`` rounds of ``--steps`` steps each):
  * one-pass:  ``ImageVAETrainer`` (core.FusedImageStep: B rows, no product of experts, packed-gradient Adam over the image range);
  * 3-pass:    the MMVAE's ``FusedTrainer`` called with ``passes=(False, True, False)`` -- it still computes all 3 B rows and the whole
               second modality;
  * modules:   the stand-alone ``ImageEncoder`` / ``ImageDecoder`` modules glued by autograd (``ImageVAE.forward`` + ``loss_function``
               + ``loss.backward()``) and ``torch.optim.Adam``.
Reported per route: the median of the rounds and their spread (max - min), in ms per step; the verdict line says whether the
one-pass step is faster than the 3-pass route by more than the larger of the two spreads.  Also: the workspace bytes of the
one-pass carve against the 3-pass one, and the particle rate of the image-only scorer (``iw_estimate`` on an ``ImageVAE``) against the
full scorer (on the ``MultimodalVAE``) at B = 64, K = 64.  Inputs are synthetic; the models are freshly initialised.
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def bench_family(family, B, D, args):
    M = importlib.import_module("multimodal_vae_amd." + family)
    from oracle import mmvae_ref as R
    dev = torch.device("cuda:0")
    side = 64 if family == "celeba" else 32
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, 3, side, side, generator=g).to(dev)
    torch.manual_seed(0)
    # one-pass
    iv = M.ImageVAE(D).cuda()
    one = M.ImageVAETrainer(iv, B, lr=1e-4)
    # 3-pass with only the image pass present
    if family == "celeba":
        mm = M.MultimodalVAE(D).cuda()
        second = (torch.rand(B, 18, generator=g) < 0.3).float().to(dev)
    else:
        mm = M.MultimodalVAE(D, sos=R.formula_sos()).cuda()
        second = (0.4 * torch.randn(B, M.MAX_WORDS, 300, generator=g)).to(dev)
    three = M.FusedTrainer(mm, B, lr=1e-4)
    # stand-alone modules + autograd + torch.optim.Adam
    mv = M.ImageVAE(D).cuda().train()
    opt = torch.optim.Adam(mv.parameters(), lr=1e-4)

    def step_modules():
        opt.zero_grad()
        recon, mu, lv = mv(x)
        loss = M.loss_function(mu, lv, recon, x) if family == "celeba" else M.loss_function(mu, lv, recon_image=recon, image=x)
        loss.backward()
        opt.step()

    routes = [("one-pass", lambda: one(x)), ("3-pass (F,T,F)", lambda: three(x, second, passes=(False, True, False))),
              ("modules+Adam", step_modules)]
    for _, fn in routes:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n, _ in routes}
    for _ in range(args.repeats):
        for n, fn in routes:
            ms[n].append(timed(fn, args.steps))
    say("%s  B = %d  n_latents = %d  (%d rounds of %d steps)" % (family, B, D, args.repeats, args.steps))
    med, spread = {}, {}
    for n, _ in routes:
        med[n], spread[n] = statistics.median(ms[n]), max(ms[n]) - min(ms[n])
        say("    %-16s %8.3f ms / step   spread %.3f ms   rounds: %s" % (n, med[n], spread[n], " ".join("%.3f" % v for v in ms[n])))
    a, b = med["one-pass"], med["3-pass (F,T,F)"]
    noise = max(spread["one-pass"], spread["3-pass (F,T,F)"])
    say("    one-pass vs 3-pass: %.2fx (%.3f ms less; run-to-run spread %.3f ms) -> %s;  vs modules+Adam: %.2fx"
        % (b / a, b - a, noise, "FASTER than the spread" if b - a > noise else "NOT faster than the spread", med["modules+Adam"] / a))
    say("    workspace: one-pass carve %d bytes (%.1f MiB), 3-pass carve %d bytes (%.1f MiB)"
        % (one.engine.ws.numel(), one.engine.ws.numel() / 2 ** 20, three.engine.ws.numel(), three.engine.ws.numel() / 2 ** 20))


def bench_scorer(family, D, args):
    M = importlib.import_module("multimodal_vae_amd." + family)
    from multimodal_vae_amd.evaluate import iw_estimate
    from oracle import mmvae_ref as R
    dev = torch.device("cuda:0")
    B, K = 64, 64
    side = 64 if family == "celeba" else 32
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 3, side, side, generator=g).to(dev)
    iv = M.ImageVAE(D).cuda().eval()
    if family == "celeba":
        mm = M.MultimodalVAE(D).cuda().eval()
        second = (torch.rand(B, 18, generator=g) < 0.3).float().to(dev)
    else:
        mm = M.MultimodalVAE(D, sos=R.formula_sos()).cuda().eval()
        second = (0.4 * torch.randn(B, M.MAX_WORDS, 300, generator=g)).to(dev)
    mu, lv = torch.zeros(B, D, device=dev), torch.zeros(B, D, device=dev)
    rates = {}
    for name, model, sec in (("image-only scorer", iv, None), ("full scorer", mm, second)):
        iw_estimate(model, x, sec, mu, lv, K, seed=1)
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            iw_estimate(model, x, sec, mu, lv, K, seed=1)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        rates[name] = B * K / statistics.median(ts)
        say("    %-18s %10.0f particles / s   (B = %d, K = %d, median of %d)" % (name, rates[name], B, K, args.repeats))
    say("    %s: image-only / full = %.2fx" % (family, rates["image-only scorer"] / rates["full scorer"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "imageonly_bench.txt"))
    ap.add_argument("--small", action="store_true", help="B = 128 only")
    args = ap.parse_args()
    say("imageonly_bench: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    shapes = [("celeba", 128, 100), ("coco", 128, 20)]
    if not args.small:
        shapes += [("celeba", 512, 100), ("coco", 1024, 20)]
    for family, B, D in shapes:
        bench_family(family, B, D, args)
        torch.cuda.empty_cache()
    say("log p(x) scorer")
    for family, D in (("celeba", 100), ("coco", 20)):
        bench_scorer(family, D, args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
