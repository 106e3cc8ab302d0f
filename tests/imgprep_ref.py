"""numpy restatement of multimodal-vae_amd/csrc/imgprep_core.h: torchvision's ``Scale(S)`` + ``CenterCrop(S)`` over Pillow's 8-bit
BILINEAR resample, in integers.  The tables are built with Python floats (IEEE double, no fused multiply-add), the sums are int64.

``scale_crop`` computes only the crop window, from the input rows and columns it depends on; ``resize_full`` is the whole resize, what
``Image.resize((ow, oh), BILINEAR)`` returns -- the CPU tests compare both with live Pillow.  The keyword arguments of ``scale_crop``
that break it on purpose (``drop_last_tap``, ``vertical_first``, ``crop``) exist so that a test can show that the case list sees
such a mistake."""
import numpy as np

PRECISION_BITS = 22
HALF = 1 << (PRECISION_BITS - 1)

# (w, h, S) of tests/test_gpu_imgprep.py and of the CPU tests
NAMED_CASES = [(178, 218, 64), (640, 480, 32), (480, 640, 32), (20, 30, 32), (64, 80, 64), (64, 64, 64), (65, 64, 64), (97, 64, 64),
               (500, 33, 32), (33, 500, 32), (1, 1, 32), (3, 1000, 64), (1300, 2000, 64), (127, 95, 32), (31, 31, 32), (100, 37, 32)]
GRID_CASES = [(w, h, 32) for w in range(30, 80, 7) for h in range(30, 80, 5)]
CASES = NAMED_CASES + GRID_CASES


def scaled_size(w, h, size):
    """torchvision's Scale of that era -> (ow, oh)"""
    if w <= h:
        return size, int(size * h / w)
    return int(size * w / h), size


def crop_offset(d):
    """int(round(d / 2.)) under Python 2 rounding (half away from zero), d >= 0"""
    return (d + 1) // 2


def coeffs(n_in, n_out, first=0, count=None, drop_last_tap=False):
    """-> [(xmin, [int coefficient, ...]), ...] for the output indices first .. first + count - 1"""
    count = n_out - first if count is None else count
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ss = 1.0 / fs
    rows = []
    for xx in range(first, first + count):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5))
        w = []
        ww = 0.0
        for x in range(xmax - xmin):
            a = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - a if a < 1.0 else 0.0)
            ww += w[-1]
        k = [int(0.5 + (v / ww if ww != 0.0 else v) * (1 << PRECISION_BITS)) for v in w]
        if drop_last_tap and len(k) > 1:
            k = k[:-1]
        rows.append((xmin, k))
    return rows


def _pass(a, axis, rows):
    """one resample pass of the uint8 array ``a`` along ``axis`` with the coefficient rows -> uint8, len(rows) along that axis"""
    a = np.moveaxis(a, axis, 0)
    out = np.empty((len(rows),) + a.shape[1:], dtype=np.uint8)
    for j, (xmin, k) in enumerate(rows):
        kk = np.asarray(k, dtype=np.int64).reshape((-1,) + (1,) * (a.ndim - 1))
        acc = HALF + (a[xmin:xmin + len(k)].astype(np.int64) * kk).sum(axis=0)
        out[j] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_full(img, ow, oh):
    """``Image.fromarray(img).resize((ow, oh), BILINEAR)`` as an (oh, ow, 3) uint8 array"""
    h, w = img.shape[:2]
    if ow != w:
        img = _pass(img, 1, coeffs(w, ow))
    if oh != h:
        img = _pass(img, 0, coeffs(h, oh))
    return img


def scale_crop(img, size, drop_last_tap=False, vertical_first=False, crop=crop_offset):
    """(h, w, 3) uint8 -> (3, size, size) uint8: Scale(size), CenterCrop(size), planar"""
    h, w = img.shape[:2]
    ow, oh = scaled_size(w, h, size)
    x1, y1 = crop(ow - size), crop(oh - size)
    hrows = coeffs(w, ow, x1, size, drop_last_tap) if ow != w else None
    vrows = coeffs(h, oh, y1, size, drop_last_tap) if oh != h else None

    def horizontal(a):
        return a[:, x1:x1 + size] if hrows is None else _pass(a, 1, hrows)

    def vertical(a):
        if vrows is None:
            return a[y1:y1 + size]
        # only the rows the window depends on
        r0, r1 = vrows[0][0], vrows[-1][0] + len(vrows[-1][1])
        return _pass(a[r0:r1], 0, [(xmin - r0, k) for xmin, k in vrows])

    out = horizontal(vertical(img)) if vertical_first else vertical(horizontal(img))
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def random_image(rng, w, h):
    return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def case_images(seed=0, cases=None):
    """the random inputs of the case list: one ``default_rng(seed)`` stream, drawn in list order"""
    rng = np.random.default_rng(seed)
    return [random_image(rng, w, h) for (w, h, _) in (CASES if cases is None else cases)]
