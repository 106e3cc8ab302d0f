"""MultiMNIST generator on the device: what it costs, measured on the GPU.

    python tools/multimnist_gen_bench.py [--out profiles/multimnist_gen_bench.txt] [--digits 60000] [--host_canvases 20000] [--steps 300] [--reps 5]

1. The bulk call: 60,000 canvases (random mode, 0..2 digits, the reference's defaults) in one ``generate`` call, device events around
   it and, separately, the wall time including the read-back of the pixels; against the reference's host loop (``datasets.py:93-145``:
   per digit one Pillow BILINEAR resize + ``np.pad`` + add, redraw above 255) over ``--host_canvases`` canvases on one core.  Where
   Pillow does not import the host loop resizes with the numpy restatement of tests/multimnist_gen_ref.py, and the report says so.
2. One B = 256 ``out="f32"`` call between device events: median and spread of ``--reps`` windows of 200 calls, and the bytes it moves.
3. The fused MultiMNIST training step at B = 256 fed three ways, alternated in one process (a, b, c, a, b, c, ...), ``--steps`` steps per
   window: (a) resident inputs, (b) ``MultiMNISTStream`` (one generator kernel in front of every step, same stream), (c)
   ``data.DeviceBatcher`` over a host dataset of the same canvases.  Wall time per step around a final synchronise.
The MNIST digits are ``data.synthetic_mnist`` (no MNIST files are needed; the work per digit does not depend on its pixels, the
retry rate does: it is printed).  Run it alone."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import multimodal_vae_amd.data as D  # noqa: E402
import multimodal_vae_amd.multimnist_gen as G  # noqa: E402


def host_loop(digits, n, seed):
    """the reference's mk_dataset for n canvases -> (seconds, retries, which resize)"""
    try:
        from PIL import Image
        which = "Pillow %s" % __import__("PIL").__version__

        def resize(img, s):
            return np.asarray(Image.fromarray(img, "L").resize((s, s), Image.BILINEAR))
    except ImportError:
        import multimnist_gen_ref as R
        which, resize = "numpy restatement (Pillow does not import)", R.resize
    rng = np.random.RandomState(seed)
    retries = 0
    t0 = time.perf_counter()
    for _ in range(n):
        k = rng.randint(0, 3)
        while True:
            canvas = np.zeros((50, 50))
            for _ in range(k):
                digit = digits[rng.randint(len(digits))]
                s = int(28 * (1.0 / (0.1 * rng.randn() + 1.3)))
                r = resize(digit, s)
                pad = 50 - s
                t, l = rng.randint(0, pad), rng.randint(0, pad)
                canvas += np.pad(r, ((t, pad - t), (l, pad - l)), "constant")
            if canvas.max() <= 255:
                break
            retries += 1
        canvas.astype(np.uint8)
    return time.perf_counter() - t0, retries, which


def events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n * 1e3           # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--digits", type=int, default=60000)
    ap.add_argument("--host_canvases", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a gfx950 GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("MultiMNIST generator on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    say("command: python tools/multimnist_gen_bench.py --out profiles/multimnist_gen_bench.txt --digits %d --host_canvases %d --steps %d --reps %d"
        % (args.digits, args.host_canvases, args.steps, args.reps))
    digits_h, labels_h = D.synthetic_mnist(args.digits, seed=0)
    digits, labels = digits_h.to(dev), labels_h.to(dev)
    mode = dict(min_digits=0, max_digits=2)

    # ---- 1. bulk
    N = 60000
    for _ in range(2):
        G.generate(digits, labels, N, seed=1, **mode)
    dev_us = [events(lambda: G._launch(digits, labels, N, 0, 0, 2, 1, 0, "u8", None, None, None), 1) for _ in range(args.reps)]
    walls = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        images, text, params, attempts = G.generate(digits, labels, N, seed=1, return_params=True, **mode)
        images_h = images.cpu()
        walls.append(time.perf_counter() - t0)
    att = attempts.cpu().numpy()
    sec, retries, which = host_loop(digits_h.numpy(), args.host_canvases, 1)
    say("1. bulk: %d canvases in one call, random mode, 0..2 digits, %d resident digits" % (N, args.digits))
    say("   kernel (device events)      median %.3f ms (%.3f .. %.3f)   %.1f M canvases/s" % (
        statistics.median(dev_us) / 1e3, min(dev_us) / 1e3, max(dev_us) / 1e3, N / statistics.median(dev_us)))
    say("   call + 150 MB read-back     median %.1f ms (%.1f .. %.1f)   %.2f M canvases/s (wall)" % (
        1e3 * statistics.median(walls), 1e3 * min(walls), 1e3 * max(walls), N / statistics.median(walls) / 1e6))
    say("   attempts: %.1f %% of the canvases were redrawn, at most %d attempts" % (100.0 * (att >= 2).mean(), att.max()))
    say("   host loop (%s, one core), %d canvases: %.2f s, %.0f canvases/s, %d redraws -> 60,000 would take %.0f s" % (
        which, args.host_canvases, sec, args.host_canvases / sec, retries, 60000.0 * sec / args.host_canvases))
    say("   device kernel / host loop: %.0f x" % ((N / statistics.median(dev_us) * 1e6) / (args.host_canvases / sec)))
    del images, images_h, text, params, attempts

    # ---- 2. one batch
    B = 256
    stream = G.MultiMNISTStream(digits, labels, B, dev, epoch_size=1 << 30, seed=3, **mode)
    counter = [0]

    def one():
        counter[0] += 1
        stream.batch(counter[0])
    events(one, 50)
    us = [events(one, 200) for _ in range(args.reps)]
    bytes_ = B * (2500 * 4 + 32) + B * 1.0 * 784          # outputs + on average one digit read per canvas
    say("2. one B = %d call (float32 out, includes the two output allocations): median %.1f us (%.1f .. %.1f); it moves about %.1f MB"
        % (B, statistics.median(us), min(us), max(us), bytes_ / 1e6))
    say("   (%.0f GB/s: far below any memory bound -- the call is launch- and latency-bound, one workgroup per CU)" % (bytes_ / statistics.median(us) / 1e3))
    stream.check()

    # ---- 3. the fused step, fed three ways
    from multimodal_vae_amd import core
    from multimodal_vae_amd.init import default_init_
    st = core.MultimnistState(100, dev)
    default_init_(st, 1)
    eng = core.FusedELBOStep(st, B)
    n_ds = 32 * B
    ds_u8, ds_text = G.generate(digits, labels, n_ds, seed=5, **mode)
    ds_u8_h, ds_text_h = ds_u8.cpu(), ds_text.cpu()
    res_x, res_t = (ds_u8[:B].float() / 255).unsqueeze(1).contiguous(), ds_text[:B].contiguous()
    loader = D.DeviceBatcher(ds_u8_h, ds_text_h, B, dev, shuffle=True, seed=1)
    gen = G.MultiMNISTStream(digits, labels, B, dev, epoch_size=args.steps * B, seed=7, **mode)

    def resident(n):
        for _ in range(n):
            eng(res_x, res_t)

    def streamed(n):
        done = 0
        while done < n:
            for x, t in gen:
                eng(x, t)
                done += 1
                if done == n:
                    break

    def loaded(n):
        done = 0
        while done < n:
            for x, t in loader:
                eng(x, t)
                done += 1
                if done == n:
                    break
    arms = [("(a) resident inputs", resident), ("(b) MultiMNISTStream", streamed), ("(c) DeviceBatcher", loaded)]
    for _, fn in arms:
        fn(100)
    torch.cuda.synchronize()
    times = {k: [] for k, _ in arms}
    for _ in range(args.reps):
        for k, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(args.steps)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / args.steps * 1e3)
    say("3. fused MultiMNIST step at B = %d, %d steps per window, %d windows per arm, alternated: ms per step, median (fastest .. slowest)" % (B, args.steps, args.reps))
    base = statistics.median(times[arms[0][0]])
    for k, _ in arms:
        m = statistics.median(times[k])
        say("   %-24s %.3f (%.3f .. %.3f)   %.0f steps/s   resident / this = %.3f" % (k, m, min(times[k]), max(times[k]), 1e3 / m, base / m))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
