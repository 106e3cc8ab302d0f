"""Step time of the COCO InfoVAE on the one-enqueue fused step against the module route and against the image-only step.

    python tools/infovae_bench.py [--steps 50] [--repeats 5] [--out profiles/infovae_bench.txt] [--small]

At B = 128 and B = 1024, n_latents = 100, ONE training step (forward, backward, Adam) is timed between device events on three arms,
warmed up and ALTERNATED in one process (``--repeats`` rounds of ``--steps`` steps each):
  * (a) fused:      ``InfoVAETrainer`` on a ``FusedInfoVAE`` (core.FusedInfoVAEStep -> mmvae_coco_infovae_step: one pass over B rows, the
                    MMD sweep on a side stream beside the decoder, packed-gradient Adam over the image range);
  * (b) modules:    the route of ``train_infovae`` without ``--fused``: ``InfoVAE`` (two stand-alone cores, autograd between them),
                    ``infovae_loss`` (BCE kernel + the two-launch ``mmvae_mmd`` op) and ``torch.optim.Adam``.  The baseline;
  * (c) image-only: ``FusedImageStep`` at kl_lambda = 0 on the same batch: the floor, (a) - (c) is what the MMD term costs inside the step.
Reported per arm: the median of the rounds and their spread (max - min), in ms per step.
Also, alone: the y-only sweep + fold (mmvae_mmd_dy) against mmvae_mmd with both gradients at (128, 128, 100) and (1024, 1024, 100).
Inputs are synthetic; the models are freshly initialised.
"""
import argparse
import ctypes as C
import gc
import os
import statistics
import sys

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


def alternate(arms, args, warmup=5, steps=None):
    steps = args.steps if steps is None else steps
    for _, fn in arms:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n, _ in arms}
    for _ in range(args.repeats):
        for n, fn in arms:
            gc.collect()            # (outside the timed region: see MODULE_ROUTE_BYTES)
            ms[n].append(timed(fn, steps))
    med = {n: statistics.median(v) for n, v in ms.items()}
    spread = {n: max(v) - min(v) for n, v in ms.items()}
    return ms, med, spread


# The module route's decoder keeps its output for the backward, which forms a reference cycle through the autograd node: the node's
# one-pass workspace (5.06 GiB at B = 1024 on the default 102-step plan) is released by Python's cycle collector, not by the backward.
# A round of the module arm is kept below this many bytes of such workspaces, and the collector runs between rounds.
MODULE_ROUTE_BYTES = 96 << 30


def bench_step(B, D, args):
    from multimodal_vae_amd import coco as M
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, 3, 32, 32, generator=g).to(dev)
    torch.manual_seed(0)
    fused = M.InfoVAETrainer(M.FusedInfoVAE(D).cuda().train(), B, lr=1e-4)
    mv = M.InfoVAE(D).cuda().train()
    opt = torch.optim.Adam(mv.parameters(), lr=1e-4)
    floor = M.ImageVAETrainer(M.ImageVAE(D).cuda().train(), B, lr=1e-4, kl_lambda=0.0)       # (core.FusedImageStep)

    def step_modules():                         # train_infovae.main's batch loop body without --fused
        opt.zero_grad()
        recon, z = mv(x)
        loss = M.infovae_loss(recon, x, z)
        loss.backward()
        opt.step()

    arms = [("(a) fused", lambda: fused(x)), ("(b) modules+Adam", step_modules), ("(c) image-only", lambda: floor(x))]
    step_modules()                              # (the stand-alone modules build their plans at their first forward)
    ws_mod = mv.decoder._core.sync(dev).module_workspace_bytes(B)
    steps = max(5, min(args.steps, MODULE_ROUTE_BYTES // ws_mod))
    ms, med, spread = alternate(arms, args, steps=steps)
    say("coco InfoVAE  B = %d  n_latents = %d  (%d rounds of %d steps, arms alternated; the module route's workspace is %.2f GiB per module call)"
        % (B, D, args.repeats, steps, ws_mod / 2 ** 30))
    for n, _ in arms:
        say("    %-18s %8.3f ms / step   spread %.3f ms   rounds: %s" % (n, med[n], spread[n], " ".join("%.3f" % v for v in ms[n])))
    a, b, c = med["(a) fused"], med["(b) modules+Adam"], med["(c) image-only"]
    noise = max(spread["(a) fused"], spread["(b) modules+Adam"])
    say("    (b) / (a) = %.2fx (%.3f ms less; spread %.3f ms) -> %s" % (b / a, b - a, noise, "FASTER than the spread" if b - a > noise else "NOT faster than the spread"))
    noise = max(spread["(a) fused"], spread["(c) image-only"])
    say("    (a) - (c) = %+.3f ms (%.1f %% of (c); spread %.3f ms): the MMD term inside the step -> %s"
        % (a - c, 100.0 * (a - c) / c, noise, "hidden within the spread" if a - c <= noise else "NOT hidden: it shows on the main chain"))
    say("    workspace: fused %d bytes (%.1f MiB), image-only %d bytes" % (fused.engine.ws.numel(), fused.engine.ws.numel() / 2 ** 20, floor.engine.ws.numel()))
    return med


def bench_sweep(n, D, args):
    from multimodal_vae_amd._lib import call, ptr
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(n, D, generator=g).to(dev), (1.5 * torch.randn(n, D, generator=g) + 0.3).to(dev)
    need_xy, need_y = call("mmvae_mmd_workspace_bytes", n, n, D), call("mmvae_mmd_dy_workspace_bytes", n, n, D)
    ws_xy, ws_y = torch.empty(need_xy, dtype=torch.uint8, device=dev), torch.empty(need_y, dtype=torch.uint8, device=dev)
    out, dx, dy = torch.empty(4, device=dev), torch.empty_like(x), torch.empty_like(y)

    def stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    arms = [("mmvae_mmd (dx, dy)", lambda: call("mmvae_mmd", ptr(x), n, ptr(y), n, D, ptr(ws_xy), need_xy, ptr(out), ptr(dx), ptr(dy), stream())),
            ("mmvae_mmd_dy", lambda: call("mmvae_mmd_dy", ptr(x), n, ptr(y), n, D, ptr(ws_y), need_y, 1.0, ptr(out), ptr(dy), 1, stream())),
            ("mmvae_mmd (value)", lambda: call("mmvae_mmd", ptr(x), n, ptr(y), n, D, ptr(ws_xy), need_xy, ptr(out), None, None, stream()))]
    ms, med, spread = alternate(arms, args)
    say("MMD alone  (%d, %d, %d): sweep + fold, us per call" % (n, n, D))
    for nm, _ in arms:
        say("    %-20s %8.1f us   spread %.1f us   rounds: %s" % (nm, 1e3 * med[nm], 1e3 * spread[nm], " ".join("%.1f" % (1e3 * v) for v in ms[nm])))
    a, b = med["mmvae_mmd (dx, dy)"], med["mmvae_mmd_dy"]
    noise = max(spread["mmvae_mmd (dx, dy)"], spread["mmvae_mmd_dy"])
    say("    both gradients / y only = %.2fx -> %s;  workspace %d -> %d bytes"
        % (a / b, "FASTER than the spread" if a - b > noise else "NOT faster than the spread", need_xy, need_y))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "infovae_bench.txt"))
    ap.add_argument("--small", action="store_true", help="B = 128 only")
    args = ap.parse_args()
    say("infovae_bench: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for B in (128,) if args.small else (128, 1024):
        bench_step(B, 100, args)
        torch.cuda.empty_cache()
        bench_sweep(B, 100, args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
