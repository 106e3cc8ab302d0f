"""Step time of the text-only VAE baseline (COCO captions) on the one-pass fused step against the two routes a user had before it.

    python tools/textonly_bench.py [--steps 20] [--repeats 5] [--out profiles/textonly_bench.txt] [--small]

Per batch size (B = 64, the reference script's default, 128 and 1024; 102 caption positions, n_latents = 100) ONE training step
(forward, backward, Adam) is timed between device events on three routes, warmed up and ALTERNATED in one process (``--repeats``
rounds of ``--steps`` steps each):
  * one-pass:  ``TextVAETrainer`` (core.FusedTextStep: B rows, no product of experts, no image half, packed-gradient Adam over the
               caption range);
  * 3-pass:    the MMVAE's ``FusedTrainer`` called with ``passes=(False, False, True)`` -- it still runs the caption decoder on 3 B
               rows and the image decoder forward;
  * modules:   the ``TextEncoder`` / ``TextDecoder`` modules glued by autograd (``TextVAE.forward`` + ``loss_function`` +
               ``loss.backward()``) and ``torch.optim.Adam``.
Reported per route: the median of the rounds and their spread (max - min), in ms per step; the verdict line says whether the
one-pass step is faster than the 3-pass route by more than the larger of the two spreads.  Also: the workspace bytes of each route
(the modules' is one module call's), and the particle rate of the text-only scorer (``iw_estimate`` on a ``TextVAE``:
mmvae_coco_iw_score_text) against the full scorer (on the ``MultimodalVAE``: mmvae_coco_iw_score) at B = 64, K = 16.  Inputs are
synthetic; the models are freshly initialised.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINES = []
THREE = "3-pass (F,F,T)"


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


def bench_step(B, D, args):
    from multimodal_vae_amd import coco as M
    from oracle import mmvae_ref as R
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    text = (0.4 * torch.randn(B, M.MAX_WORDS, 300, generator=g)).to(dev)
    image = torch.rand(B, 3, 32, 32, generator=g).to(dev)
    sos = R.formula_sos()
    torch.manual_seed(0)
    one = M.TextVAETrainer(M.TextVAE(D, sos=sos).cuda(), B, lr=1e-4)
    three = M.FusedTrainer(M.MultimodalVAE(D, sos=sos).cuda(), B, lr=1e-4)
    mv = M.TextVAE(D, sos=sos).cuda().train()
    opt = torch.optim.Adam(mv.parameters(), lr=1e-4)

    def step_modules():
        opt.zero_grad()
        recon, mu, lv = mv(text)
        M.loss_function(mu, lv, recon_text=recon, text=text).backward()
        opt.step()

    routes = [("one-pass", lambda: one(text)), (THREE, lambda: three(image, text, passes=(False, False, True))), ("modules+Adam", step_modules)]
    for _, fn in routes:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n, _ in routes}
    for _ in range(args.repeats):
        for n, fn in routes:
            ms[n].append(timed(fn, args.steps))
    one(text).check()
    say("coco captions  B = %d  n_latents = %d  T = %d  (%d rounds of %d steps)" % (B, D, M.MAX_WORDS, args.repeats, args.steps))
    med, spread = {}, {}
    for n, _ in routes:
        med[n], spread[n] = statistics.median(ms[n]), max(ms[n]) - min(ms[n])
        say("    %-16s %8.3f ms / step   spread %.3f ms   rounds: %s" % (n, med[n], spread[n], " ".join("%.3f" % v for v in ms[n])))
    a, b = med["one-pass"], med[THREE]
    noise = max(spread["one-pass"], spread[THREE])
    say("    one-pass vs 3-pass: %.2fx (%.3f ms less; run-to-run spread %.3f ms) -> %s;  vs modules+Adam: %.2fx"
        % (b / a, b - a, noise, "FASTER than the spread" if b - a > noise else "NOT faster than the spread", med["modules+Adam"] / a))
    st = one.engine.state
    say("    workspace: one-pass carve %d bytes (%.1f MiB), 3-pass carve %d bytes (%.1f MiB), one module call %d bytes (%.1f MiB)"
        % (one.engine.ws.numel(), one.engine.ws.numel() / 2 ** 20, three.engine.ws.numel(), three.engine.ws.numel() / 2 ** 20,
           st.module_workspace_bytes(B), st.module_workspace_bytes(B) / 2 ** 20))


def bench_scorer(D, args):
    from multimodal_vae_amd import coco as M
    from multimodal_vae_amd.evaluate import iw_estimate
    from oracle import mmvae_ref as R
    dev = torch.device("cuda:0")
    B, K = 64, 16
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 3, 32, 32, generator=g).to(dev)
    text = (0.4 * torch.randn(B, M.MAX_WORDS, 300, generator=g)).to(dev)
    tv = M.TextVAE(D, sos=R.formula_sos()).cuda().eval()
    mm = M.MultimodalVAE(D, sos=R.formula_sos()).cuda().eval()
    mu, lv = torch.zeros(B, D, device=dev), torch.zeros(B, D, device=dev)
    rates = {}
    for name, model, image in (("text-only scorer", tv, None), ("full scorer", mm, x)):
        iw_estimate(model, image, text, mu, lv, K, seed=1)
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            iw_estimate(model, image, text, mu, lv, K, seed=1)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        rates[name] = B * K / statistics.median(ts)
        say("    %-18s %10.0f particles / s   (B = %d, K = %d, median of %d)" % (name, rates[name], B, K, args.repeats))
    say("    text-only / full = %.2fx" % (rates["text-only scorer"] / rates["full scorer"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "textonly_bench.txt"))
    ap.add_argument("--small", action="store_true", help="B = 64 only")
    args = ap.parse_args()
    say("textonly_bench: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for B in ((64,) if args.small else (64, 128, 1024)):
        bench_step(B, 100, args)
        torch.cuda.empty_cache()
    say("log p(y) scorer")
    bench_scorer(100, args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
