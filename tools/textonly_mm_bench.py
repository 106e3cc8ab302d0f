"""Step time of the MultiMNIST text-only VAE baseline: the one-pass fused step at hidden size 50 against the same step at 100, the
module route, and (for orientation) the MMVAE's 3-pass step restricted to its text pass.

    python tools/textonly_mm_bench.py [--steps 50] [--repeats 5] [--out profiles/textonly_mm_bench.txt] [--small]

Per batch size (B = 128, the reference script's default, and 256; n_latents = 100) ONE training step (forward, backward, Adam) is
timed between device events on four routes, warmed up and ALTERNATED in one process (``--repeats`` rounds of ``--steps`` steps):
  * (a) one-pass H=50:   ``TextVAETrainer`` on ``TextVAE`` (core.FusedMMTextStep on the text kernels' hidden-size-50 instantiation);
  * (b) one-pass H=100:  the same step on a plan created with n_hiddens = 100 -- isolates what the smaller instantiation buys;
  * (c) modules+Adam:    ``TextVAE.forward`` + ``textonly_loss_function`` + ``loss.backward()`` + ``torch.optim.Adam``;
  * (d) 3-pass (F,F,T):  the MMVAE's ``FusedTrainer`` with ``passes=(False, False, True)`` -- ANOTHER model (hidden size 100, image
                         decoder forward, text decoder on 3 B rows): orientation only.
Reported per route: the median of the rounds and their spread (max - min), in ms per step.  A difference inside the larger of two
routes' spreads is called a tie.  At 8-16 workgroups the text path is latency-bound.  Inputs are synthetic; models freshly initialised.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINES = []
A, B_, C_, D_ = "(a) one-pass H=50", "(b) one-pass H=100", "(c) modules+Adam", "(d) 3-pass (F,F,T)"


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
    from multimodal_vae_amd import core, multimnist as M
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    text = torch.randint(0, 12, (B, 4), generator=g).to(dev)
    image = torch.rand(B, 1, 50, 50, generator=g).to(dev)
    torch.manual_seed(0)
    one50 = M.TextVAETrainer(M.TextVAE(D, use_cuda=True).cuda(), B, lr=1e-3)
    st100 = core.MultimnistTextState(D, dev, 100)
    st100.params.uniform_(-0.1, 0.1)
    one100 = core.FusedMMTextStep(st100, B, lr=1e-3)
    three = M.FusedTrainer(M.MultimodalVAE(D, use_cuda=True).cuda(), B, lr=1e-3)
    mv = M.TextVAE(D, use_cuda=True).cuda().train()
    opt = torch.optim.Adam(mv.parameters(), lr=1e-3)

    def step_modules():
        opt.zero_grad()
        recon, mu, lv = mv(text)
        M.textonly_loss_function(mu, lv, recon, text).backward()
        opt.step()

    routes = [(A, lambda: one50(text)), (B_, lambda: one100(text)), (C_, step_modules),
              (D_, lambda: three(image, text, passes=(False, False, True)))]
    for _, fn in routes:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n, _ in routes}
    for _ in range(args.repeats):
        for n, fn in routes:
            ms[n].append(timed(fn, args.steps))
    say("multimnist text-only  B = %d  n_latents = %d  (%d rounds of %d steps)" % (B, D, args.repeats, args.steps))
    med, spread = {}, {}
    for n, _ in routes:
        med[n], spread[n] = statistics.median(ms[n]), max(ms[n]) - min(ms[n])
        say("    %-20s %8.3f ms / step   spread %.3f ms   rounds: %s" % (n, med[n], spread[n], " ".join("%.3f" % v for v in ms[n])))
    say("    " + verdict(A, B_, med, spread))
    say("    " + verdict(A, C_, med, spread))
    say("    " + verdict(A, D_, med, spread) + "   [another model: orientation only]")
    say("    workspace: one-pass H=50 %.1f MiB, H=100 %.1f MiB, 3-pass %.1f MiB"
        % (one50.engine.ws.numel() / 2 ** 20, one100.ws.numel() / 2 ** 20, three.engine.ws.numel() / 2 ** 20))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "textonly_mm_bench.txt"))
    ap.add_argument("--small", action="store_true", help="B = 128 only")
    args = ap.parse_args()
    say("textonly_mm_bench: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for B in ((128,) if args.small else (128, 256)):
        bench_step(B, 100, args)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
