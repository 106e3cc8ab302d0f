"""Records tests/golden/pillow_scale_crop.npz: what Pillow's ``Image.resize((ow, oh), BILINEAR)`` followed by the centre crop gives for
the case list of tests/imgprep_ref.py.  The file holds OUTPUTS only (one (3,S,S) uint8 array per case, the case list and the Pillow
version); the inputs are regenerated from ``numpy.random.default_rng(seed)`` by ``imgprep_ref.case_images``.  Needs Pillow; run it
again only when the case list changes:

    python tools/record_pillow_scale_crop.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import imgprep_ref as R  # noqa: E402

SEED = 0


def pillow_scale_crop(img, size):
    from PIL import Image
    h, w = img.shape[:2]
    ow, oh = R.scaled_size(w, h, size)
    full = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
    x1, y1 = R.crop_offset(ow - size), R.crop_offset(oh - size)
    return np.ascontiguousarray(full[y1:y1 + size, x1:x1 + size].transpose(2, 0, 1))


def main():
    import PIL
    images = R.case_images(SEED)
    arrays = {"cases": np.asarray(R.CASES, dtype=np.int32), "seed": np.asarray(SEED), "pillow_version": np.asarray(PIL.__version__)}
    for k, ((w, h, S), im) in enumerate(zip(R.CASES, images)):
        arrays["out_%03d" % k] = pillow_scale_crop(im, S)
    path = os.path.join(ROOT, "tests", "golden", "pillow_scale_crop.npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s: %d cases, %d bytes, Pillow %s" % (path, len(R.CASES), os.path.getsize(path), PIL.__version__))


if __name__ == "__main__":
    main()
