"""One-launch incremental PixelCNN sampler against the reference's own sampling loop, on the same GPU.

    python tools/pixelcnn_sample_bench.py [--out profiles/pixelcnn_sample_bench.txt] [--ref_pixels 4] [--reps 3]

The reference loop (``coco/train_pixelcnn.py:185-197``) runs one full forward per pixel AND channel through torch ops and keeps one
column of the result.  It is timed over ``--ref_pixels`` pixels (x data_channels forwards each) and SCALED to the H x W image; the
sampler is timed whole.  Shapes: 64 x 1 x 28 x 28 with PixelCNN and 64 x 3 x 32 x 32 with GatedPixelCNN, 15 blocks, hid_dims 128,
out_dims 256.  Run it alone in its process."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_vae_amd.pixelcnn as P  # noqa: E402


def _time(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def _reference_pixels(model, sample, pixels, levels):
    """the reference's loop body for the first `pixels` pixels of the image"""
    _, C, _, W = sample.shape
    with torch.no_grad():
        for p in range(pixels):
            i, j = divmod(p, W)
            for k in range(C):
                probs = torch.exp(P.log_softmax_by_dim(model(sample), dim=1))[:, :, k, i, j]
                sample[:, k, i, j] = torch.multinomial(probs, 1).float().view(-1) / (levels - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ref_pixels", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n_blocks", type=int, default=15)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["pixelcnn_sample_bench: %s, torch %s; samples per workgroup %d; %d repetitions per arm, medians"
             % (torch.cuda.get_device_name(0), torch.__version__, P.pixelcnn_geometry()[0], args.reps),
             "this tool ran alone in its process and started nothing else; the machine itself is shared",
             "the reference loop is timed over its first %d pixels (x data_channels forwards each) and scaled to H x W" % args.ref_pixels]
    for cls, B, C, S in ((P.PixelCNN, 64, 1, 28), (P.GatedPixelCNN, 64, 3, 32)):
        torch.manual_seed(0)
        model = cls(n_blocks=args.n_blocks, data_channels=C, hid_dims=128, out_dims=256).to(dev).eval()
        u = torch.rand(B, C, S, S, device=dev)
        P.generate(model, B, S, S, uniforms=u)                     # warm-up: workspace, code load
        ts = _time(lambda: P.generate(model, B, S, S, uniforms=u), args.reps)
        t = statistics.median(ts)
        lines.append("%s %d x %d x %d x %d, %d blocks:" % (cls.__name__, B, C, S, S, args.n_blocks))
        lines.append("  sampler   one launch (+ packing)     %9.2f ms (fastest %.2f, slowest %.2f)   %8.1f samples/s   %7.2f us per pixel step"
                     % (1e3 * t, 1e3 * min(ts), 1e3 * max(ts), B / t, 1e6 * t / (S * S)))
        try:
            sample = torch.zeros(B, C, S, S, device=dev)
            _reference_pixels(model, sample, 1, 256)               # warm-up
            rs = _time(lambda: _reference_pixels(model, sample, args.ref_pixels, 256), args.reps)
            r = statistics.median(rs) * (S * S) / args.ref_pixels
            lines.append("  reference one forward per pixel and channel, SCALED from %d pixels   %9.2f ms   %8.2f samples/s   %7.2f us per pixel step"
                         "   %.1fx the sampler's time" % (args.ref_pixels, 1e3 * r, B / r, 1e6 * r / (S * S), r / t))
        except RuntimeError as e:                                  # torch's convolution unusable here: the sampler alone
            lines.append("  reference loop: torch's convolution is unusable on this machine (%s); the sampler alone is reported"
                         % str(e).splitlines()[0][:120])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(text)


if __name__ == "__main__":
    main()
