"""PixelCNN / GatedPixelCNN training step: the torch backend against the HIP causal convolution, on the same GPU.

    python tools/pixelcnn_train_bench.py [--out profiles/pixelcnn_train_bench.txt] [--steps 20] [--reps 5] [--warmup 3]

What is timed is ``train_pixelcnn.train_step`` (forward, loss, backward, clip, Adam) at the reference's default shapes:
GatedPixelCNN B = 32, 3 x 32 x 32, 15 blocks, hid 128, 256 levels and PixelCNN B = 32, 1 x 28 x 28, 15 blocks, hid 128, 8 levels.
Arms: (a) torch backend, fp32; (b) torch backend under ``torch.autocast(dtype=torch.bfloat16)`` (for information); (c) hip backend.
Device events around ``--steps`` steps, ``--reps`` repetitions per arm, interleaved (a, b, c, a, b, c, ...) in one process; median and
spread.  Then the three kernels alone (each call packs its weights / folds its partials, as in training) at the 3 x 3 block layer and
the 2 x 3 vertical layer of the 32 x 3 x 32 x 32 shape, with the FLOPs and bytes they need computed from shapes.  Run it alone."""
import argparse
import contextlib
import copy
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_vae_amd.pixelcnn as P  # noqa: E402
import multimodal_vae_amd.train_pixelcnn as T  # noqa: E402
from multimodal_vae_amd._lib import call, ptr  # noqa: E402

BF16_PEAK = 2.5e15           # dense bf16 MFMA, FLOP/s (16 x the 157 TFLOP/s fp32 matrix rate)
HBM_BW = 6.3e12              # achievable HBM bytes/s


def _events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n          # ms per call


def _steps(lines, say, cls, B, C, S, V, args, dev):
    torch.manual_seed(0)
    base = cls(n_blocks=args.n_blocks, data_channels=C, hid_dims=128, out_dims=V)
    data = T.preprocess(T.synthetic_images(B, C, S, seed=1), V).to(dev)
    arms = []
    for label, backend, cast in (("(a) torch backend, fp32", "torch", False), ("(b) torch backend, autocast bf16 (information)", "torch", True),
                                 ("(c) hip backend (bf16 MFMA, fp32 accumulate)", "hip", False)):
        model = P.set_conv_backend(copy.deepcopy(base), backend).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
        ctx = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if cast else contextlib.nullcontext

        def step(model=model, opt=opt, ctx=ctx):
            with ctx():
                return T.train_step(model, opt, data, V)
        arms.append([label, step, [], None])
    say("%s B = %d, %d x %d x %d, %d blocks, hid 128, %d levels:" % (cls.__name__, B, C, S, S, args.n_blocks, V))
    for arm in arms:
        try:
            for _ in range(args.warmup):
                arm[3] = arm[1]()[0]
        except RuntimeError as e:
            arm[1] = None
            say("  %-50s unusable here: %s" % (arm[0], str(e).splitlines()[0][:120]))
    for _ in range(args.reps):
        for arm in arms:
            if arm[1] is not None:
                arm[2].append(_events(arm[1], args.steps))
    med = {}
    for label, fn, ts, loss in arms:
        if fn is None:
            continue
        med[label[:3]] = statistics.median(ts)
        say("  %-50s %9.2f ms per step (fastest %.2f, slowest %.2f over %d x %d steps)   loss after warm-up %.4f"
            % (label, med[label[:3]], min(ts), max(ts), args.reps, args.steps, loss))
    if "(a)" in med and "(c)" in med:
        say("  (c) takes %.2f x the time of (a)" % (med["(c)"] / med["(a)"]))


def _kernels(say, name, kind_taps, Cin, Cout, kh, kw, args, dev):
    B, H, W = 32, 32, 32
    P_ = B * H * W
    n = len(kind_taps)
    x = torch.randn(B, Cin, H, W, device=dev).contiguous(memory_format=torch.channels_last)
    g = torch.randn(B, Cout, H, W, device=dev).contiguous(memory_format=torch.channels_last)
    w = torch.randn(Cout, Cin, kh, kw, device=dev) / (Cin * n) ** 0.5
    b = torch.zeros(Cout, device=dev)
    y, dx, dw, db = torch.empty_like(g), torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
    dims = (B, H, W, Cin, Cout, kh, kw)
    ws = torch.empty(call("mmvae_causal_conv_workspace_bytes", *dims, n), dtype=torch.uint8, device=dev)
    taps = (ctypes.c_int * (4 * n))(*[v for t in kind_taps for v in t])
    tail = (taps, n) + dims + (ptr(ws), ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    chunk = P.causal_conv_geometry()[2]
    flops = 2.0 * P_ * Cin * Cout * n
    wbytes = 4 * Cout * Cin * kh * kw
    runs = (("forward", lambda: call("mmvae_causal_conv_forward", ptr(x), ptr(w), ptr(b), ptr(y), *tail), 4 * P_ * (Cin + Cout) + wbytes),
            ("data gradient", lambda: call("mmvae_causal_conv_backward_data", ptr(g), ptr(w), ptr(dx), *tail), 4 * P_ * (Cin + Cout) + wbytes),
            ("weight gradient", lambda: call("mmvae_causal_conv_backward_weight", ptr(g), ptr(x), ptr(dw), ptr(db), *tail),
             4 * P_ * (Cin + 2 * Cout) + wbytes + 2 * 4 * ((P_ + chunk - 1) // chunk) * n * Cout * Cin))
    say("%s: %d taps, Cin %d, Cout %d, %d positions; %.2f GFLOP per kernel" % (name, n, Cin, Cout, P_, flops / 1e9))
    for label, fn, nbytes in runs:
        for _ in range(3):
            fn()
        ts = [_events(fn, args.steps) for _ in range(args.reps)]
        t = statistics.median(ts) * 1e-3
        t_mfma, t_hbm = flops / BF16_PEAK, nbytes / HBM_BW
        bound = "bf16 MFMA rate" if t_mfma > t_hbm else "HBM bandwidth"
        say("  %-16s %8.1f us (fastest %.1f, slowest %.1f)   %7.1f TFLOP/s   %6.1f MB needed, %6.2f TB/s   bound: %s, %.1f us -> %.1f %% of it"
            % (label, 1e6 * t, 1e3 * min(ts), 1e3 * max(ts), flops / t / 1e12, nbytes / 1e6, nbytes / t / 1e12, bound,
               1e6 * max(t_mfma, t_hbm), 100 * max(t_mfma, t_hbm) / t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n_blocks", type=int, default=15)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    say("pixelcnn_train_bench: %s, torch %s; tile %d positions x %d channels, weight-gradient chunk %d; device events around %d steps, "
        "%d repetitions per arm, interleaved, medians" % ((torch.cuda.get_device_name(0), torch.__version__) + P.causal_conv_geometry()[:3]
                                                          + (args.steps, args.reps)))
    say("this tool ran alone in its process and started nothing else; the machine itself is shared")
    _steps(lines, say, P.GatedPixelCNN, 32, 3, 32, 256, args, dev)
    _steps(lines, say, P.PixelCNN, 32, 1, 28, 8, args, dev)
    say("kernels alone (each call packs its weights or folds its partials); bounds: bf16 MFMA %.1f PFLOP/s, HBM %.1f TB/s achievable; bytes = "
        "activations and weights once, fp32, plus the weight gradient's partials written and read" % (BF16_PEAK / 1e15, HBM_BW / 1e12))
    mB = P.MaskedConv2d("B", 128, 128, 3, 1, 1)
    blk = P.GatedResidualBlock("B", 128, 128, 3)
    _kernels(say, "3 x 3 block layer (mask B)", P.taps_of(mB), 128, 128, 3, 3, args, dev)
    _kernels(say, "2 x 3 vertical layer", P.taps_of(blk.vertical_conv), 128, 256, 2, 3, args, dev)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
