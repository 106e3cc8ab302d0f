"""Step time of MNIST's image-only VAE baseline: the one-pass fused step with the column-strip fused layers on and off, the MMVAE's
3-pass step restricted to its image pass, the module route, the two strip kernels alone against the launches they replace, and the
image-only scorer against the two-modality one.

    python tools/imageonly_mnist_bench.py [--steps 50] [--repeats 5] [--out profiles/imageonly_mnist_bench.txt]

At B = 128 (the reference script's default) and 256, n_latents = 20, ONE training step (forward, backward, Adam) is timed between
device events on four routes, warmed up and ALTERNATED in one process (``--repeats`` rounds of ``--steps`` steps):
  * (a) one-pass, strip:   ``ImageVAETrainer`` on ``mnist.VAE`` (core.FusedImageStep -> mmvae_mnist_image_step) with mnist_strip = 1: each
                           Linear + BatchNorm1d + ReLU one column-strip launch per direction (csrc/mnist_strip.hip);
  * (b) one-pass, unfused: the same step with mnist_strip = 0: gemm_f32 + bn1d_fwd32, gemm_f32 + bn1d_bwd32;
  * (c) 3-pass (F,T,F):    the MMVAE's ``FusedTrainer`` with ``passes=(False, True, False)`` -- what a user had before: 3 B decoder rows,
                           the whole label half, the experts' 1e-8; its launches are not changed here;
  * (d) modules+Adam:      ``VAE.forward`` + ``imageonly_loss`` + ``loss.backward()`` + ``torch.optim.Adam``.
Reported per route: the median of the rounds and their spread (max - min), in ms per step.  A difference inside the larger of two
routes' spreads is called a tie.  Then each of the four fused layers alone, forward and backward, strip against unfused launches
(mmvae_mnist_lin_bn_act_fwd / mmvae_mnist_lin_dgrad_bn_bwd, route 1 against route 0), the scorer in particles per second
(mmvae_mnist_iw_score_image against mmvae_mnist_iw_score on 4096 particle rows), and the workspace sizes.  Inputs are synthetic;
models freshly initialised.
"""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINES = []
A, B_, C_, D_ = "(a) one-pass, strip", "(b) one-pass, unfused", "(c) 3-pass (F,T,F)", "(d) modules+Adam"
LAYERS = (("image_encoder.net.0+1", 400, 784, 200), ("image_encoder.net.3+4", 200, 400, 40),        # name, N, K, Nn
          ("image_decoder.net.0+1", 200, 20, 400), ("image_decoder.net.3+4", 400, 200, 784))


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
    return "%s vs %s: %.4f ms %s, %.2fx (spread %.4f ms) -> %s" % (name_x, name_y, abs(d), "less" if d > 0 else "more", med[name_y] / med[name_x], noise, word)


def alternate(routes, args, steps, before=None):
    for n, k, fn in routes:
        if before:
            before(k)
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n, _, _ in routes}
    for _ in range(args.repeats):
        for n, k, fn in routes:
            if before:
                before(k)
            ms[n].append(timed(fn, steps))
    return ({n: statistics.median(v) for n, v in ms.items()}, {n: max(v) - min(v) for n, v in ms.items()}, ms)


def bench_step(B, D, args):
    from multimodal_vae_amd import mnist as M
    from multimodal_vae_amd._lib import call
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    label = torch.randint(0, 10, (B,), generator=g).to(dev)
    image = torch.rand(B, 784, generator=g).to(dev)
    torch.manual_seed(0)
    one_s = M.ImageVAETrainer(M.VAE(D).cuda(), B, lr=1e-3)
    one_u = M.ImageVAETrainer(M.VAE(D).cuda(), B, lr=1e-3)
    three = M.FusedTrainer(M.MultimodalVAE(D).cuda(), B, lr=1e-3)
    mv = M.VAE(D).cuda().train()
    opt = torch.optim.Adam(mv.parameters(), lr=1e-3)

    def knob(v):
        if v >= 0:
            call("mmvae_debug_set", b"mnist_strip", v)

    def step_modules():
        opt.zero_grad()
        recon, mu, lv = mv(image)
        M.imageonly_loss(recon, image, mu, lv).backward()
        opt.step()

    routes = [(A, 1, lambda: one_s(image)), (B_, 0, lambda: one_u(image)), (C_, -1, lambda: three(image, label, passes=(False, True, False))),
              (D_, -1, step_modules)]
    med, spread, ms = alternate(routes, args, args.steps, knob)
    call("mmvae_debug_reset", b"mnist_strip")
    say("mnist image-only  B = %d  n_latents = %d  (%d rounds of %d steps)" % (B, D, args.repeats, args.steps))
    for n, _, _ in routes:
        say("    %-22s %8.4f ms / step   spread %.4f ms   rounds: %s" % (n, med[n], spread[n], " ".join("%.4f" % v for v in ms[n])))
    say("    " + verdict(A, B_, med, spread))
    say("    " + verdict(A, C_, med, spread))
    say("    " + verdict(B_, C_, med, spread))
    say("    " + verdict(B_, D_, med, spread))
    say("    workspace: one-pass %.2f MiB (strip and unfused alike), 3-pass %.2f MiB" % (one_s.engine.ws.numel() / 2 ** 20, three.engine.ws.numel() / 2 ** 20))


def bench_layers(B, args):
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd._ops import stream
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev).contiguous()
    say("mnist fused layers alone  B = %d  (%d rounds of %d calls; strip = 1 launch, unfused = gemm_f32 + BatchNorm kernel)" % (B, args.repeats, args.steps))
    for name, N, K, Nn in LAYERS:
        x, w, b, gamma, beta = rnd(B, K).abs(), rnd(N, K) / math.sqrt(K), 0.05 * rnd(N), 1 + 0.1 * rnd(N), 0.1 * rnd(N)
        rm, rv, nbt = torch.zeros(N, device=dev), torch.ones(N, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        r, a, mr = torch.empty(B, N, device=dev), torch.empty(B, N, device=dev), torch.empty(N, 2, device=dev)
        dy, wn = rnd(B, Nn) / B, rnd(Nn, N) / math.sqrt(N)
        d_r, dg, dbt = torch.empty(B, N, device=dev), torch.zeros(N, device=dev), torch.zeros(N, device=dev)

        def fwd(route):
            call("mmvae_mnist_lin_bn_act_fwd", route, ptr(x), K, ptr(w), ptr(b), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt), B, N, K, 1,
                 ptr(r), ptr(a), ptr(mr), stream())

        def bwd(route):
            call("mmvae_mnist_lin_dgrad_bn_bwd", route, ptr(dy), Nn, ptr(wn), ptr(r), ptr(mr), ptr(gamma), ptr(beta), B, N, ptr(d_r), ptr(dg), ptr(dbt), stream())

        for what, fn in (("fwd", fwd), ("bwd", bwd)):
            routes = [("strip", 1, lambda fn=fn: fn(1)), ("unfused", 0, lambda fn=fn: fn(0))]
            med, spread, _ = alternate(routes, args, args.steps)
            say("    %-22s %s  strip %7.2f us (spread %.2f)   unfused %7.2f us (spread %.2f)   %s"
                % (name, what, 1e3 * med["strip"], 1e3 * spread["strip"], 1e3 * med["unfused"], 1e3 * spread["unfused"],
                   verdict("strip", "unfused", med, spread).split("-> ")[1]))


def bench_scorer(D, args):
    from multimodal_vae_amd import evaluate as E, mnist as M
    from multimodal_vae_amd import _ops
    dev = torch.device("cuda:0")
    rows, K = 4096, 64
    nr = rows // K
    iv, mm = M.VAE(D).cuda().eval(), M.MultimodalVAE(D).cuda().eval()
    z = torch.randn(rows, D, device=dev)
    image = torch.rand(nr, 784, device=dev)
    lx, words = torch.empty(rows, device=dev), torch.empty(rows * 10, device=dev)
    routes = []
    for name, model in (("mmvae_mnist_iw_score_image", iv), ("mmvae_mnist_iw_score", mm)):
        fam, st = E._family(model), model._core.sync(dev)
        ws = torch.empty(0, dtype=torch.uint8, device=dev)
        routes.append((name, -1, (lambda fam=fam, st=st, ws=ws: fam.score(st, rows, ws, 0, z, image, nr, K, lx, words, _ops.stream()))))
    med, spread, _ = alternate(routes, args, max(args.steps // 5, 2))
    say("mnist scorer  n_latents = %d  %d particle rows per call (%d examples x %d particles)" % (D, rows, nr, K))
    for name, _, _ in routes:
        say("    %-28s %8.4f ms / call   spread %.4f ms   %.2f M particles/s" % (name, med[name], spread[name], rows / med[name] / 1e3))
    say("    " + verdict(routes[0][0], routes[1][0], med, spread))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "imageonly_mnist_bench.txt"))
    args = ap.parse_args()
    from multimodal_vae_amd._lib import call
    say("imageonly_mnist_bench: %s, torch %s; strip row cap %d" % (torch.cuda.get_device_name(0), torch.__version__, call("mmvae_mnist_strip_max_rows")))
    for B in (128, 256):
        bench_step(B, 20, args)
        torch.cuda.empty_cache()
    for B in (128, 256):
        bench_layers(B, args)
    bench_scorer(20, args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
