"""PixelCNN output head (conv4 + cross entropy): torch ops against the fused HIP head ``pixelcnn.head_nll``, on the same GPU.

    python tools/pixelcnn_head_bench.py [--out profiles/pixelcnn_head_bench.txt] [--steps 20] [--reps 5] [--warmup 3]

Shapes: GatedPixelCNN coco B = 32, 3 x 32 x 32, hid 128, 256 levels and PixelCNN mnist B = 32, 1 x 28 x 28, hid 128, 8 levels.
The head alone, forward + backward from ``features`` to the gradients of h, w and b of the mean NLL:
(a) torch ``conv4`` + ``cross_entropy_by_dim`` in fp32; (b) ``causal_conv2d`` for ``conv4`` + torch cross entropy (what
``--conv_backend hip`` runs); (c) the fused op.  For each arm also ``torch.cuda.max_memory_allocated`` over one forward + backward,
above what was allocated before it.  Then the whole ``train_step`` under ``--conv_backend hip`` with ``--head torch`` against
``--head hip``, and the images per second of ``evaluate.nll_pixelcnn`` with either head.  Device events around ``--steps`` iterations,
``--reps`` repetitions per arm, interleaved in one process, after a warm-up; median with fastest and slowest.  Run it alone."""
import argparse
import contextlib
import copy
import io
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_vae_amd.evaluate as E  # noqa: E402
import multimodal_vae_amd.pixelcnn as P  # noqa: E402
import multimodal_vae_amd.train_pixelcnn as T  # noqa: E402


def _events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n          # ms per call


def _interleaved(say, arms, args, unit="ms", scale=1.0, fmt="%9.3f"):
    """arms: [label, fn] -> {label[:3]: median}"""
    for arm in arms:
        for _ in range(args.warmup):
            arm[1]()
    ts = {arm[0]: [] for arm in arms}
    for _ in range(args.reps):
        for label, fn in arms:
            ts[label].append(_events(fn, args.steps))
    med = {}
    for label, _ in arms:
        v = [scale(t) if callable(scale) else t * scale for t in ts[label]]
        med[label[:3]] = statistics.median(v)
        say(("  %-62s " + fmt + " %s (fastest %.3f, slowest %.3f over %d x %d)") % (label, med[label[:3]], unit, min(v), max(v), args.reps,
                                                                                  args.steps))
    return med


def _head(say, name, B, C, S, V, args, dev):
    hid = 128
    torch.manual_seed(0)
    conv4 = P.MaskedConv2d("B", hid, V * C, 1).to(dev)
    h0 = torch.relu(torch.randn(B, hid, S, S, device=dev)).contiguous(memory_format=torch.channels_last)
    target = torch.randint(0, V, (B, C, S, S), device=dev)
    taps = P.taps_of(conv4)

    def run(kind):
        h = h0.detach().requires_grad_()
        conv4.weight.grad = conv4.bias.grad = None
        if kind == "fused":
            loss = P.head_nll(h, conv4.weight, conv4.bias, target, C).mean()
        else:
            y = P.causal_conv2d(h, conv4.weight, conv4.bias, taps) if kind == "conv" else conv4(h)
            loss = P.cross_entropy_by_dim(y.view(B, V, C, S, S), target)
        loss.backward()
        return loss

    arms = [["(a) torch conv4 + cross_entropy_by_dim, fp32", lambda: run("torch")],
            ["(b) causal_conv2d conv4 + torch cross entropy", lambda: run("conv")],
            ["(c) fused head_nll (bf16 MFMA, fp32 accumulate, no logits)", lambda: run("fused")]]
    say("%s head alone, B = %d, %d x %d x %d, hid %d, %d levels (fp32 logits %.1f MB): forward + backward to dh, dw, db" %
        (name, B, C, S, S, hid, V, 4e-6 * B * V * C * S * S))
    med = _interleaved(say, arms, args)
    say("  (c) takes %.2f x the time of (a) and %.2f x the time of (b)" % (med["(c)"] / med["(a)"], med["(c)"] / med["(b)"]))
    for label, fn in arms:
        torch.cuda.synchronize()
        conv4.weight.grad = conv4.bias.grad = None
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        loss = float(fn().detach())
        torch.cuda.synchronize()
        say("  %-62s peak memory above the %.1f MB held before: %8.1f MB   loss %.5f"
            % (label, before / 1e6, (torch.cuda.max_memory_allocated() - before) / 1e6, loss))
    say("  workspace of the fused op at this shape: %.2f MB (held in the cached buffer, part of 'held before')"
        % (P.head_nll_workspace_bytes(B, C, S, S, hid, V) / 1e6))


def _steps(say, cls, B, C, S, V, args, dev):
    torch.manual_seed(0)
    base = cls(n_blocks=args.n_blocks, data_channels=C, hid_dims=128, out_dims=V)
    data = T.preprocess(T.synthetic_images(B, C, S, seed=1), V).to(dev)
    arms = []
    for label, head in (("(a) --conv_backend hip --head torch", "torch"), ("(c) --conv_backend hip --head hip", "hip")):
        model = P.set_conv_backend(copy.deepcopy(base), "hip").to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
        arms.append([label, lambda model=model, opt=opt, head=head: T.train_step(model, opt, data, V, head=head)])
    say("%s train_step, B = %d, %d x %d x %d, %d blocks, hid 128, %d levels:" % (cls.__name__, B, C, S, S, args.n_blocks, V))
    med = _interleaved(say, arms, args, fmt="%9.2f")
    say("  (c) takes %.2f x the time of (a)" % (med["(c)"] / med["(a)"]))

    images = T.synthetic_images(4 * B, C, S, seed=2)
    model = copy.deepcopy(base).to(dev)

    def evaluate(head):
        with contextlib.redirect_stdout(io.StringIO()):
            E.nll_pixelcnn(model, images, B, head)
    say("%s evaluate.nll_pixelcnn, %d images in batches of %d (torch convolutions):" % (cls.__name__, 4 * B, B))
    keep, args.steps = args.steps, max(1, args.steps // 4)
    med = _interleaved(say, [["(a) --head torch", lambda: evaluate("torch")], ["(c) --head hip", lambda: evaluate("hip")]], args, unit="images/s",
                       scale=lambda ms: 4 * B / (ms * 1e-3), fmt="%9.0f")
    args.steps = keep
    say("  (c) evaluates %.2f x the images per second of (a)" % (med["(c)"] / med["(a)"]))


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

    say("pixelcnn_head_bench: %s, torch %s; head tile %d positions x %d levels, dw / db chunk %d; device events around %d iterations, "
        "%d repetitions per arm, interleaved, medians" % ((torch.cuda.get_device_name(0), torch.__version__) + P.head_nll_geometry()[:3]
                                                          + (args.steps, args.reps)))
    say("this tool ran alone in its process and started nothing else; the machine itself is shared")
    _head(say, "GatedPixelCNN coco", 32, 3, 32, 256, args, dev)
    _head(say, "PixelCNN mnist", 32, 1, 28, 8, args, dev)
    _steps(say, P.GatedPixelCNN, 32, 3, 32, 256, args, dev)
    _steps(say, P.PixelCNN, 32, 1, 28, 8, args, dev)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
