"""Step time of MultiMNIST's image-only VAE baseline: the one-pass fused step with the one-expert waist kernels on and off, the MMVAE's
3-pass step restricted to its image pass, the module route, and the image-only scorer against the MMVAE's.

    python tools/imageonly_mm_bench.py [--steps 50] [--repeats 5] [--out profiles/imageonly_mm_bench.txt] [--small]

Per batch size (B = 128, the reference script's default, and 256) and latent size (20, the baseline's default, and 100) ONE training
step (forward, backward, Adam) is timed between device events on four routes, warmed up and ALTERNATED in one process (``--repeats``
rounds of ``--steps`` steps):
  * (a) one-pass, waist:   ``ImageVAETrainer`` on ``ImageVAE`` (core.FusedImageStep -> mmvae_mm_image_step) with mm_image_waist = 1:
                           classifier.3 + classifier.6 + the latent block as one row-block launch per direction (csrc/mlp_tail.hip);
  * (b) one-pass, chain:   the same step with mm_image_waist = 0: mlp2_fwd (D = 100) or two GEMMs (D = 20), latent1 + finish, and back;
  * (c) 3-pass (F,T,F):    the MMVAE's ``FusedTrainer`` with ``passes=(False, True, False)`` -- what a user had before: 3 B decoder rows,
                           both dropout variants, the whole text half, the experts' 1e-8; its launches are not changed here;
  * (d) modules+Adam:      ``ImageVAE.forward`` + ``imageonly_loss_function`` + ``loss.backward()`` + ``torch.optim.Adam``.
Reported per route: the median of the rounds and their spread (max - min), in ms per step.  A difference inside the larger of two
routes' spreads is called a tie.  Then the scorer: particles per second of mmvae_mm_iw_score_image against mmvae_mm_iw_score on 4096
particle rows.  Inputs are synthetic; models freshly initialised.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINES = []
A, B_, C_, D_ = "(a) one-pass, waist", "(b) one-pass, chain", "(c) 3-pass (F,T,F)", "(d) modules+Adam"


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


def verdict(name_x, name_y, med, spread):
    """x against y: faster / slower by more than the larger spread, or a tie"""
    d, noise = med[name_y] - med[name_x], max(spread[name_x], spread[name_y])
    word = "a TIE (inside the spread)" if abs(d) <= noise else ("FASTER" if d > 0 else "SLOWER")
    return "%s vs %s: %.3f ms %s, %.2fx (spread %.3f ms) -> %s" % (name_x, name_y, abs(d), "less" if d > 0 else "more", med[name_y] / med[name_x], noise, word)


def bench_step(B, D, args):
    from multimodal_vae_amd import multimnist as M
    from multimodal_vae_amd._lib import call
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    text = torch.randint(0, 12, (B, 4), generator=g).to(dev)
    image = torch.rand(B, 1, 50, 50, generator=g).to(dev)
    torch.manual_seed(0)
    one_w = M.ImageVAETrainer(M.ImageVAE(D).cuda(), B, lr=1e-3)
    one_c = M.ImageVAETrainer(M.ImageVAE(D).cuda(), B, lr=1e-3)
    three = M.FusedTrainer(M.MultimodalVAE(D, use_cuda=True).cuda(), B, lr=1e-3)
    mv = M.ImageVAE(D).cuda().train()
    opt = torch.optim.Adam(mv.parameters(), lr=1e-3)

    def knob(v):
        call("mmvae_debug_set", b"mm_image_waist", v)

    def step_modules():
        opt.zero_grad()
        recon, mu, lv = mv(image)
        M.imageonly_loss_function(recon, image, mu, lv).backward()
        opt.step()

    routes = [(A, 1, lambda: one_w(image)), (B_, 0, lambda: one_c(image)), (C_, -1, lambda: three(image, text, passes=(False, True, False))),
              (D_, -1, step_modules)]
    for _, k, fn in routes:
        knob(k)
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n, _, _ in routes}
    for _ in range(args.repeats):
        for n, k, fn in routes:
            knob(k)
            ms[n].append(timed(fn, args.steps))
    knob(-1)
    say("multimnist image-only  B = %d  n_latents = %d  (%d rounds of %d steps)" % (B, D, args.repeats, args.steps))
    med, spread = {}, {}
    for n, _, _ in routes:
        med[n], spread[n] = statistics.median(ms[n]), max(ms[n]) - min(ms[n])
        say("    %-20s %8.3f ms / step   spread %.3f ms   rounds: %s" % (n, med[n], spread[n], " ".join("%.3f" % v for v in ms[n])))
    say("    " + verdict(A, B_, med, spread))
    say("    " + verdict(A, C_, med, spread))
    say("    " + verdict(B_, C_, med, spread))
    say("    " + verdict(A, D_, med, spread))
    say("    workspace: one-pass %.1f MiB (waist and chain alike), 3-pass %.1f MiB" % (one_w.engine.ws.numel() / 2 ** 20, three.engine.ws.numel() / 2 ** 20))


def bench_scorer(D, args):
    from multimodal_vae_amd import evaluate as E, multimnist as M
    from multimodal_vae_amd import _ops
    dev = torch.device("cuda:0")
    rows, K = E.IW_ROWS, 64
    nr = rows // K
    iv, mm = M.ImageVAE(D).cuda().eval(), M.MultimodalVAE(D, use_cuda=True).cuda().eval()
    z = torch.randn(rows, D, device=dev)
    image = torch.rand(nr, 2500, device=dev)
    lx, words = torch.empty(rows, device=dev), torch.empty(rows * 4 * 12, device=dev)
    ms = {}
    runs = []
    for name, model in (("mmvae_mm_iw_score_image", iv), ("mmvae_mm_iw_score", mm)):
        fam, st = E._family(model), model._core.sync(dev)
        nb = fam.workspace_bytes(st, rows)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        fn = (lambda fam=fam, st=st, ws=ws, nb=nb: fam.score(st, rows, ws, nb, z, image, nr, K, lx, words, _ops.stream()))
        for _ in range(3):
            fn()
        runs.append((name, fn))
        ms[name] = []
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for name, fn in runs:
            ms[name].append(timed(fn, max(args.steps // 5, 2)))
    say("multimnist scorer  n_latents = %d  %d particle rows per call (%d examples x %d particles)" % (D, rows, nr, K))
    for name, _ in runs:
        med = statistics.median(ms[name])
        say("    %-26s %8.3f ms / call   spread %.3f ms   %.2f M particles/s" % (name, med, max(ms[name]) - min(ms[name]), rows / med / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "imageonly_mm_bench.txt"))
    ap.add_argument("--small", action="store_true", help="B = 128, n_latents = 20 only")
    args = ap.parse_args()
    say("imageonly_mm_bench: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for D in ((20,) if args.small else (20, 100)):
        for B in ((128,) if args.small else (128, 256)):
            bench_step(B, D, args)
            torch.cuda.empty_cache()
        bench_scorer(D, args)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
