"""Records Pillow's 8-bit BILINEAR resize of a few 28 x 28 images to every side the MultiMNIST generator uses, as the fixture of
tests/test_cpu_multimnist_gen.py (which restates the resample in numpy and compares bit for bit).

    python tools/record_pillow_resize.py [--out tests/golden/pillow_bilinear_28.npz]

Contents: ``images`` uint8 (6,28,28) (two random, all-255, two sparse, one digit-like blob), ``sides`` (14..41), ``side_<s>`` uint8
(6,s,s) = ``Image.fromarray(img, "L").resize((s, s), Image.BILINEAR)``, ``pillow_version``.  Needs Pillow."""
import argparse
import os

import numpy as np


def images() -> np.ndarray:
    rng = np.random.RandomState(28)
    out = np.zeros((6, 28, 28), dtype=np.uint8)
    out[0] = rng.randint(0, 256, (28, 28))
    out[1] = rng.randint(0, 256, (28, 28))
    out[2] = 255
    out[3] = np.where(rng.rand(28, 28) < 0.1, rng.randint(1, 256, (28, 28)), 0)
    out[4] = np.where(rng.rand(28, 28) < 0.03, 255, 0)
    yy, xx = np.mgrid[:28, :28]
    out[5] = np.clip(255.0 * np.exp(-((yy - 13.5) ** 2 + (xx - 12.0) ** 2) / 30.0) * 1.3, 0, 255)
    return out


def main():
    import PIL
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "pillow_bilinear_28.npz"))
    args = ap.parse_args()
    imgs = images()
    sides = np.arange(14, 42)
    rec = {"images": imgs, "sides": sides, "pillow_version": np.array(PIL.__version__)}
    for s in sides:
        rec["side_%d" % s] = np.stack([np.asarray(Image.fromarray(im, "L").resize((int(s), int(s)), Image.BILINEAR)) for im in imgs])
    np.savez_compressed(args.out, **rec)
    print("wrote %s (%d bytes), Pillow %s" % (args.out, os.path.getsize(args.out), PIL.__version__))


if __name__ == "__main__":
    main()
