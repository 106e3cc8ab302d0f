"""Measures the Scale + CenterCrop op (multimodal_vae_amd.imgprep) and what surrounds it in a dataset build, and writes
profiles/imgprep_bench.txt.  Needs a gfx950 GPU (no fallback: without one it fails).

    python tools/imgprep_bench.py [--images 4096] [--reps 20] [--builder 19867] [--out profiles/imgprep_bench.txt]

What is recorded, each named for what it is:
  * the op's time between device events, inputs resident on the device, for --images synthetic 218 x 178 images at S = 64 and the same
    number of 480 (wide) x 640 images at S = 32; the implied input rate = packed input bytes / time, against the 8.0 TB/s HBM3E
    specification (6.29 TB/s is the measured float4 copy);
  * the host-to-device copy of the same packed, pinned buffer, between device events;
  * the same arrays through Pillow ``resize`` + crop on 16 host threads (wall clock), where Pillow imports; otherwise that is said
    and no ratio is recorded;
  * ``make_celeba --synthetic N`` for one partition of --builder images (wall clock; 19867 = CelebA's val partition), 0 skips it.
"""
import argparse
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC = 8.0e12
HBM_COPY = 6.29e12


def event_ms(fn, reps, warmup=3):
    """median and spread of ``fn`` between device events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def pillow_scale_crop(img, size):
    from PIL import Image
    from multimodal_vae_amd import imgprep as I
    h, w = img.shape[:2]
    ow, oh = I.scaled_size(w, h, size)
    x1, y1 = I.crop_offset(ow - size), I.crop_offset(oh - size)
    return np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR).crop((x1, y1, x1 + size, y1 + size)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--builder', type=int, default=19867)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'imgprep_bench.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("imgprep_bench: no GPU; nothing is measured on a CPU")
    from multimodal_vae_amd import data as D, imgprep as I, make_celeba as M
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd._ops import stream
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = ["imgprep_bench: %d images per shape, %d timed repetitions (median [min .. max]), device %s"
             % (args.images, args.reps, torch.cuda.get_device_name(dev))]
    try:
        import PIL
        pillow = PIL.__version__
    except ImportError:
        pillow = None
    rng = np.random.default_rng(0)
    celeba, _ = D.synthetic_celeba_raw(min(args.images, 256), seed=0)
    shapes = (("218 x 178 -> 64 (CelebA)", [celeba[i % len(celeba)] for i in range(args.images)], 64),
              ("480 x 640 (w x h) -> 32 (COCO-like)", [rng.integers(0, 256, size=(640, 480, 3), dtype=np.uint8) for _ in range(64)] * (args.images // 64), 32))
    for name, arrays, S in shapes:
        n = len(arrays)
        t0 = time.perf_counter()
        packed = I.pack_images(arrays)
        pack_s = time.perf_counter() - t0
        pixels = packed[0]
        in_bytes = sum(a.size for a in arrays)
        d = [t.to(dev) for t in packed]
        out = torch.empty((n, 3, S, S), dtype=torch.uint8, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)

        def op():
            call("mmvae_imgprep_scale_crop", ptr(d[0]), d[0].numel(), ptr(d[1]), ptr(d[2]), ptr(d[3]), n, S, ptr(out), None, ptr(status), stream())
        med, lo, hi = event_ms(op, args.reps)
        assert int(status.abs().sum()) == 0
        lines.append("")
        lines.append("%s, n = %d, %.1f MB of packed input" % (name, n, in_bytes / 1e6))
        lines.append("  op (device events, inputs resident):   %8.3f ms [%.3f .. %.3f]  %.2f us / image" % (med, lo, hi, 1e3 * med / n))
        rate = in_bytes / (med * 1e-3)
        lines.append("  implied input rate:                    %8.2f TB/s = %.1f %% of the 8.0 TB/s HBM3E specification (%.1f %% of the 6.29 TB/s "
                     "measured copy rate)" % (rate / 1e12, 100 * rate / HBM_SPEC, 100 * rate / HBM_COPY))
        dst = torch.empty_like(d[0])
        cmed, clo, chi = event_ms(lambda: dst.copy_(pixels, non_blocking=True), args.reps)
        lines.append("  host-to-device copy of the pinned buffer: %6.3f ms [%.3f .. %.3f]  %.1f GB/s" % (cmed, clo, chi, pixels.numel() / cmed / 1e6))
        lines.append("  packing on the host (one thread):      %8.1f ms" % (1e3 * pack_s))
        if pillow is None:
            lines.append("  Pillow baseline: Pillow does not import on this machine; no ratio recorded")
        else:
            with ThreadPoolExecutor(max_workers=16) as pool:
                list(pool.map(lambda a: pillow_scale_crop(a, S), arrays[:64]))
                t0 = time.perf_counter()
                res = list(pool.map(lambda a: pillow_scale_crop(a, S), arrays))
                wall = time.perf_counter() - t0
            same = all((r.transpose(2, 0, 1) == o).all() for r, o in zip(res[:32], out[:32].cpu().numpy()))
            lines.append("  Pillow %s resize + crop, 16 host threads: %6.1f ms wall  (%.0f x the op; first 32 outputs %s)"
                         % (pillow, 1e3 * wall, 1e3 * wall / med, "equal the op's" if same else "DIFFER from the op's"))
    if args.builder > 0:
        with tempfile.TemporaryDirectory() as tmp:
            t0 = time.perf_counter()
            M.main(['--synthetic', str(args.builder), '--out', tmp, '--partitions', 'val'])
            wall = time.perf_counter() - t0
        lines.append("")
        lines.append("make_celeba --synthetic %d --partitions val (synthesis on the host, pack, copy, op, read-back, torch.save): %.2f s wall"
                     % (args.builder, wall))
        lines.append("  (no file is decoded in this run: a real build adds the JPEG decoding of every image on the host thread pool)")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fp:
        fp.write(text)
    print(text)


if __name__ == "__main__":
    main()
