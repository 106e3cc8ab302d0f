"""MNIST InfoVAE: the four 4 x 4 stride-2 layers and the whole training step, torch ops against the HIP op, on the same GPU.

    python tools/infovae_mnist_bench.py [--out profiles/infovae_mnist_bench.txt] [--batch 128] [--iters 50] [--reps 7] [--warmup 5]

1. Each of the four layers (convolution + activation) at B = ``--batch``, forward alone and forward + backward (dx and dw; the first
   layer's input is the image: dw only).  Arms: (a) torch ops, fp32; (b) torch ops under ``torch.autocast(dtype=torch.bfloat16)`` (for
   information); (c) ``down4s2`` / ``up4s2``.  Channels-last inputs for every arm.
2. The three kernels of the op alone through the C ABI (each call packs its weights / folds its partials, as in training), with the
   FLOPs and bytes they need computed from shapes, against their own bound: the larger of FLOPs / bf16 MFMA peak and bytes / HBM rate.
3. One ``train_infovae_mnist.train_step`` (forward, loss, backward, Adam) at B = ``--batch`` under both backends.
Device events around ``--iters`` calls, ``--reps`` repetitions per arm, interleaved (a, b, c, a, b, c, ...) in one process after
``--warmup`` calls of every arm; median and spread.  Run it alone."""
import argparse
import contextlib
import copy
import ctypes
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_vae_amd.conv4s2 as K  # noqa: E402
import multimodal_vae_amd.data as D  # noqa: E402
import multimodal_vae_amd.mnist as M  # noqa: E402
import multimodal_vae_amd.train_infovae_mnist as T  # noqa: E402
from multimodal_vae_amd._lib import call, ptr  # noqa: E402

BF16_PEAK = 2.5e15           # dense bf16 MFMA, FLOP/s (16 x the 157 TFLOP/s fp32 matrix rate)
HBM_BW = 6.3e12              # achievable HBM bytes/s
# (name, direction, Cs, Cl, Hs, Ws, act, needs dx)
LAYERS = [("encoder_conv.0  Conv2d(1,64)+LeakyReLU", "down", 1, 64, 28, 28, "leaky", False),
          ("encoder_conv.2  Conv2d(64,128)+LeakyReLU", "down", 64, 128, 14, 14, "leaky", True),
          ("decoder_conv.0  ConvT2d(128,64)+ReLU", "up", 64, 128, 14, 14, "relu", True),
          ("decoder_conv.2  ConvT2d(64,1)+sigmoid", "up", 1, 64, 28, 28, "sigmoid", True)]


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


def _torch_layer(direction, act, x, w):
    pre = F.conv2d(x, w, stride=2, padding=1) if direction == "down" else F.conv_transpose2d(x, w, stride=2, padding=1)
    return {"leaky": lambda t: F.leaky_relu(t, 0.1), "relu": torch.relu, "sigmoid": torch.sigmoid}[act](pre)


def _layers(say, args, dev):
    B = args.batch
    say("1. layers at B = %d: us per call, median (fastest .. slowest) of %d x %d calls; fwd+bwd = forward, dx and dw" % (B, args.reps, args.iters))
    for name, direction, Cs, Cl, Hs, Ws, act, need_dx in LAYERS:
        gen = torch.Generator().manual_seed(0)
        xs = (B, Cs, Hs, Ws) if direction == "down" else (B, Cl, Hs // 2, Ws // 2)
        ys = (B, Cl, Hs // 2, Ws // 2) if direction == "down" else (B, Cs, Hs, Ws)
        x = torch.randn(xs, generator=gen).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(need_dx)
        w = (torch.randn(Cl, Cs, 4, 4, generator=gen) / (16 * Cs) ** 0.5).to(dev).requires_grad_()
        g = torch.randn(ys, generator=gen).to(dev).contiguous(memory_format=torch.channels_last)
        op = K.down4s2 if direction == "down" else K.up4s2
        cast = lambda: torch.autocast("cuda", dtype=torch.bfloat16)          # noqa: E731

        def fwd(f, ctx=contextlib.nullcontext):
            def run():
                with torch.no_grad(), ctx():
                    f()
            return run

        def both(f, ctx=contextlib.nullcontext):
            def run():
                x.grad = w.grad = None
                with ctx():
                    y = f()
                y.backward(g.to(y.dtype))
            return run

        t_ = lambda: _torch_layer(direction, act, x, w)                      # noqa: E731
        h_ = lambda: op(x, w, act, 0.1)                                      # noqa: E731
        arms = [("(a) fwd", fwd(t_)), ("(b) fwd", fwd(t_, cast)), ("(c) fwd", fwd(h_)),
                ("(a) fwd+bwd", both(t_)), ("(b) fwd+bwd", both(t_, cast)), ("(c) fwd+bwd", both(h_))]
        r = _interleaved(arms, args)
        say("  %s%s" % (name, "" if need_dx else "   (no dx: the input is the image)"))
        for what in ("fwd", "fwd+bwd"):
            say("    %-8s (a) torch fp32 %8.1f (%.1f .. %.1f)   (b) torch autocast bf16 %8.1f (%.1f .. %.1f)   (c) hip %8.1f (%.1f .. %.1f)   (c)/(a) %.2f"
                % ((what,) + r["(a) " + what] + r["(b) " + what] + r["(c) " + what] + (r["(c) " + what][0] / r["(a) " + what][0],)))


def _kernels(say, args, dev):
    B = args.batch
    say("2. kernels alone at B = %d (C ABI; down / up include the weight-pack launch, wgrad the fold launch): us per call, median" % B)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, direction, Cs, Cl, Hs, Ws, act, _ in LAYERS[:2]:
        dims = (B, Cs, Cl, Hs, Ws)
        ws = torch.empty(K.conv4s2_workspace_bytes(*dims), dtype=torch.uint8, device=dev)
        s = torch.randn(B, Hs, Ws, Cs, device=dev)
        l = torch.randn(B, Hs // 2, Ws // 2, Cl, device=dev)
        w = torch.randn(Cl, Cs, 4, 4, device=dev)
        so, lo, dw = torch.empty_like(s), torch.empty_like(l), torch.empty_like(w)
        tail = dims + (ptr(ws), ws.numel(), stream)
        arms = [("down", lambda: call("mmvae_conv4s2_down", ptr(s), None, ptr(w), ptr(lo), 0, 2, 0.1, *tail)),
                ("up", lambda: call("mmvae_conv4s2_up", ptr(l), None, ptr(w), ptr(so), 0, 1, 0.1, *tail)),
                ("up (g, y) -> dx", lambda: call("mmvae_conv4s2_up", ptr(l), ptr(l), ptr(w), ptr(so), 2, 0, 0.1, *tail)),
                ("wgrad", lambda: call("mmvae_conv4s2_wgrad", ptr(s), ptr(l), None, ptr(l), 2, 0.1, ptr(dw), *tail))]
        r = _interleaved(arms, args)
        flops = 2.0 * B * (Hs // 2) * (Ws // 2) * Cl * Cs * 16
        io = 4.0 * (s.numel() + l.numel() + w.numel())
        say("  Cs = %d, Cl = %d, S %d x %d: %.3f GFLOP, %.1f MB of fp32 operands and results (one pass each)" % (Cs, Cl, Hs, Ws, flops / 1e9, io / 1e6))
        for label, _ in arms:
            bytes_ = io + (4.0 * l.numel() if "(g, y)" in label or label == "wgrad" else 0.0)      # the saved output is read too
            bound = max(flops / BF16_PEAK, bytes_ / HBM_BW) * 1e6
            t = r[label][0]
            say("    %-16s %8.1f us (%.1f .. %.1f)   %7.2f TFLOP/s   %7.1f GB/s   bound %.2f us (%s)   %.1f%% of it"
                % (label, t, r[label][1], r[label][2], flops / t / 1e6, bytes_ / t / 1e3, bound,
                   "FLOPs" if flops / BF16_PEAK > bytes_ / HBM_BW else "bytes", 100.0 * bound / t))


def _steps(say, args, dev):
    B = args.batch
    torch.manual_seed(0)
    base = M.InfoVAE(n_latents=20)
    data = D.synthetic_mnist(B, seed=1)[0].float().div(255.0).unsqueeze(1).to(dev)
    ts = torch.randn(B, 20, generator=torch.Generator().manual_seed(2)).to(dev)
    arms, losses = [], {}
    for label, backend, cast in (("(a) torch backend, fp32", "torch", False), ("(b) torch backend, autocast bf16 (information)", "torch", True),
                                 ("(c) hip backend (bf16 MFMA, fp32 accumulate)", "hip", False)):
        vae = M.set_infovae_backend(copy.deepcopy(base), backend).to(dev)
        opt = torch.optim.Adam(vae.parameters(), lr=1e-3)
        ctx = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if cast else contextlib.nullcontext

        def step(vae=vae, opt=opt, ctx=ctx, label=label, cast=cast):
            if not cast:
                losses[label] = T.train_step(vae, opt, data, ts)
                return
            opt.zero_grad()                                 # train_step with the model alone under autocast: the loss wants fp32
            with ctx():
                recon, z = vae(data)
            loss = M.infovae_loss(recon.float(), data, z.float(), ts)
            loss.backward()
            opt.step()
            losses[label] = loss.detach()
        arms.append((label, step))
    first = {}
    for label, fn in arms:
        fn()
        first[label] = float(losses[label])
    r = _interleaved(arms, args)
    n = 1 + args.warmup + args.reps * args.iters
    say("3. train_step at B = %d (forward, MSE + MMD, backward, Adam over 12.9 M parameters): us per step, median (fastest .. slowest)" % B)
    for label, _ in arms:
        say("  %-50s %9.1f (%.1f .. %.1f)   loss at step 0 %.6f, after %d steps %.6f" % ((label,) + r[label] + (first[label], n, float(losses[label]))))
    say("  (c) takes %.2f x the time of (a)" % (r[arms[2][0]][0] / r[arms[0][0]][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a gfx950 GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("MNIST InfoVAE on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    _layers(say, args, dev)
    _kernels(say, args, dev)
    _steps(say, args, dev)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
