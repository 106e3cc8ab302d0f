"""MNIST InfoVAE: the one-enqueue fused step against the module route, and each fp32 Linear kernel against torch, on the same GPU.

    python tools/infovae_mnist_step_bench.py [--out profiles/infovae_mnist_step_bench.txt] [--batches 128 512] [--iters 50] [--reps 5]

1. One training step at B in ``--batches``, D = 20.  Arms, alternated in one process: (a) ``InfoVAETrainer`` (mmvae_mnist_infovae_step
   + mmvae_adam_step); (b) the module route with ``conv_backend="hip"`` + ``torch.optim.Adam``; (c) the module route with the torch
   backend + ``torch.optim.Adam``.
2. Each of the four Linear layers alone through the C ABI (forward, data gradient, weight gradient) against
   ``torch.nn.functional.linear`` + activation and its autograd, and against its byte bound: the weight (or its gradient) once over
   the HBM rate.  The permuted layers run on channels-last operands; torch gets them in the weight's own order (no transposing pass is
   charged to it).
Device events around ``--iters`` calls, ``--reps`` rounds per arm after ``--warmup`` calls of every arm; median and spread.  Run it alone."""
import argparse
import copy
import ctypes
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_vae_amd.data as D  # noqa: E402
import multimodal_vae_amd.mnist as M  # noqa: E402
import multimodal_vae_amd.train_infovae_mnist as T  # noqa: E402
from multimodal_vae_amd._lib import call, ptr  # noqa: E402

HBM_BW = 6.3e12              # achievable HBM bytes/s
# (name, N, K, act, perm)
LAYERS = [("encoder_fc.0  Linear(6272,1024)+LeakyReLU, perm", 1024, 6272, "leaky", 1), ("encoder_fc.2  Linear(1024,20)", 20, 1024, "none", 0),
          ("decoder_fc.0  Linear(20,1024)+ReLU", 1024, 20, "relu", 0), ("decoder_fc.2  Linear(1024,6272)+ReLU, perm", 6272, 1024, "relu", 1)]
ACTS = ("none", "relu", "leaky")


def _events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n * 1e3          # us per call


def _interleaved(arms, args):
    """arms: [(label, fn)] -> {label: (median, fastest, slowest)} in us"""
    for _, fn in arms:
        for _ in range(args.warmup):
            fn()
    times = {label: [] for label, _ in arms}
    for _ in range(args.reps):
        for label, fn in arms:
            times[label].append(_events(fn, args.iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def _steps(say, args, dev, B):
    torch.manual_seed(0)
    base = M.InfoVAE(n_latents=20)
    data = D.synthetic_mnist(B, seed=1)[0].float().div(255.0).unsqueeze(1).to(dev)
    ts = torch.randn(B, 20, generator=torch.Generator().manual_seed(2)).to(dev)
    losses, arms = {}, []
    fused = M.FusedInfoVAE(n_latents=20)
    fused.load_state_dict(base.state_dict())
    fused.to(dev)
    trainer = M.InfoVAETrainer(fused, B, lr=1e-3)

    def fused_step():
        losses["(a)"] = trainer(data, true_samples=ts)
    arms.append(("(a) fused step + mmvae_adam_step", fused_step))
    for tag, label, backend in (("(b)", "(b) module route, conv_backend hip + torch.optim.Adam", "hip"),
                                ("(c)", "(c) module route, conv_backend torch + torch.optim.Adam", "torch")):
        vae = M.set_infovae_backend(copy.deepcopy(base), backend).to(dev)
        opt = torch.optim.Adam(vae.parameters(), lr=1e-3)

        def step(vae=vae, opt=opt, tag=tag):
            losses[tag] = T.train_step(vae, opt, data, ts)
        arms.append((label, step))
    first = {}
    for label, fn in arms:
        fn()
        v = losses[label[:3]]
        first[label] = float(v.total()) if hasattr(v, "total") else float(v)
    r = _interleaved(arms, args)
    n = 1 + args.warmup + args.reps * args.iters
    say("1. one training step at B = %d, D = 20 (forward, MSE + MMD, backward, Adam over 12.9 M parameters): us per step, median "
        "(fastest .. slowest) of %d x %d" % (B, args.reps, args.iters))
    for label, _ in arms:
        v = losses[label[:3]]
        last = float(v.total()) if hasattr(v, "total") else float(v)
        say("  %-58s %9.1f (%.1f .. %.1f)   loss at step 0 %.6f, after %d steps %.6f" % ((label,) + r[label] + (first[label], n, last)))
    a, b, c = (r[label][0] for label, _ in arms)
    say("  (a) takes %.2f x the time of (b) and %.2f x the time of (c)" % (a / b, a / c))


def _layers(say, args, dev, B):
    say("2. Linear layers alone at B = %d: us per call, median (fastest .. slowest); bound = 4 N K bytes / %.1f TB/s" % (B, HBM_BW / 1e12))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, N, K, act, perm in LAYERS:
        gen = torch.Generator().manual_seed(0)
        x = torch.randn(B, K, generator=gen).to(dev).requires_grad_()
        w = (torch.randn(N, K, generator=gen) / K ** 0.5).to(dev).requires_grad_()
        b = torch.randn(N, generator=gen).to(dev).requires_grad_()
        g = torch.randn(B, N, generator=gen).to(dev)
        y, dx, dw, db = torch.empty(B, N, device=dev), torch.empty(B, K, device=dev), torch.empty(N, K, device=dev), torch.empty(N, device=dev)
        wsf = torch.empty(max(16, int(call("mmvae_lin_act_workspace_bytes", B, N, K, 0))), dtype=torch.uint8, device=dev)
        wsd = torch.empty(max(16, int(call("mmvae_lin_act_workspace_bytes", B, N, K, 1))), dtype=torch.uint8, device=dev)
        code = ACTS.index(act)
        tact = {"none": lambda t: t, "relu": torch.relu, "leaky": lambda t: F.leaky_relu(t, 0.1)}[act]
        xd, wd, bd = x.detach(), w.detach(), b.detach()
        yp = ptr(y) if code else None

        def t_fwd():
            with torch.no_grad():
                tact(F.linear(xd, wd, bd))

        def t_all():
            x.grad = w.grad = b.grad = None
            tact(F.linear(x, w, b)).backward(g)

        arms = [("torch fwd", t_fwd), ("torch fwd + autograd (dx, dW, db)", t_all),
                ("hip fwd", lambda: call("mmvae_lin_act_fwd", ptr(xd), ptr(wd), ptr(bd), ptr(y), B, N, K, code, 0.1, perm, ptr(wsf), wsf.numel(), stream)),
                ("hip dgrad", lambda: call("mmvae_lin_act_dgrad", ptr(g), yp, ptr(wd), ptr(dx), B, N, K, code, 0.1, perm, ptr(wsd), wsd.numel(), stream)),
                ("hip wgrad (dW, db)", lambda: call("mmvae_lin_act_wgrad", ptr(g), yp, ptr(xd), ptr(dw), ptr(db), B, N, K, code, 0.1, perm, stream))]
        arms[2][1]()                                          # y before the backward kernels read it
        r = _interleaved(arms, args)
        bound = 4.0 * N * K / HBM_BW * 1e6
        say("  %s: weight %.1f MB, bound %.2f us per pass" % (name, 4.0 * N * K / 1e6, bound))
        for label, _ in arms:
            t = r[label]
            extra = "" if label.startswith("torch") else "   %5.1f%% of the bound, %7.1f GB/s of weight traffic" % (100.0 * bound / t[0], 4.0 * N * K / t[0] / 1e3)
            say("    %-36s %8.1f (%.1f .. %.1f)%s" % (label, t[0], t[1], t[2], extra))
        hip3 = r["hip fwd"][0] + r["hip dgrad"][0] + r["hip wgrad (dW, db)"][0]
        say("    hip fwd + dgrad + wgrad %.1f us = %.2f x torch fwd + autograd" % (hip3, hip3 / r["torch fwd + autograd (dx, dW, db)"][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a gfx950 GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("MNIST InfoVAE fused step on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for B in args.batches:
        _steps(say, args, dev, B)
    for B in args.batches:
        _layers(say, args, dev, B)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
