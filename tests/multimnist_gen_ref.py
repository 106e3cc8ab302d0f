"""numpy restatement of multimodal-vae_amd/csrc/mmgen_core.h: Philox4x32-10 with common.h's keying, the resize tables, the draws, the
render and the rejection loop of the MultiMNIST generator.  Everything is integer arithmetic (the tables: IEEE double), so the
device result is compared with ``==``."""
import math

import numpy as np

CANVAS, DIGIT, SIDE_MIN, SIDE_MAX, MAX_TAPS, MAX_DIGITS, MAX_ATTEMPTS, MAX_REDRAWS, FIXED_SIDE, FILL = 50, 28, 14, 41, 5, 4, 64, 64, 21, 11
N_SIDES = SIDE_MAX - SIDE_MIN + 1
COEF_WORDS = 2 + MAX_TAPS
SIDE_WORDS = SIDE_MAX * COEF_WORDS
T_OFFSET = N_SIDES * SIDE_WORDS
TABLE_WORDS = T_OFFSET + N_SIDES
F_FIXED, F_NO_RESIZE, F_NO_TRANSLATE, F_REVERSE, F_SCRAMBLE, F_NO_REPEAT = 1, 2, 4, 8, 16, 32
FIXED_PADS = [(4, 4), (4, 23), (23, 4), (23, 23)]
M32 = np.uint64(0xffffffff)


def philox(seed, ctr, stream):
    """Philox::gen(seed, ctr, stream) of csrc/common.h; ``ctr`` and ``stream`` may be arrays -> uint32 (..., 4)"""
    ctr = np.asarray(ctr, dtype=np.uint64)
    stream = np.asarray(stream, dtype=np.uint64)
    ctr, stream = np.broadcast_arrays(ctr, stream)
    c = [ctr & M32, ctr >> np.uint64(32), stream & M32, np.full(ctr.shape, 0x5bd1e995, dtype=np.uint64)]
    k0, k1 = np.uint64(int(seed) & 0xffffffff), np.uint64((int(seed) >> 32) & 0xffffffff)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, axis=-1).astype(np.uint32)


def mulhi(a, b):
    return ((np.asarray(a, dtype=np.uint64) * np.uint64(b)) >> np.uint64(32)).astype(np.int64)


def coefficients(side, n_in=DIGIT):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for BILINEAR, n_in -> side: [(xmin, [int taps])] per output index"""
    scale = n_in / side
    fs = max(scale, 1.0)
    support, ss = fs, 1.0 / fs
    rows = []
    for xx in range(side):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        rows.append((xmin, [int((v / ww if ww != 0.0 else v) * (1 << 22) + 0.5) for v in w]))
    return rows


def side_thresholds():
    T = np.zeros(N_SIDES, dtype=np.uint32)
    for s in range(SIDE_MIN, SIDE_MAX + 1):
        z = (DIGIT / (s + 1) - 1.3) / 0.1
        p = 0.5 * math.erfc(z / math.sqrt(2.0)) * 4294967296.0
        T[s - SIDE_MIN] = 0xffffffff if s == SIDE_MAX or p >= 4294967295.0 else int(p)
    return T


def tables():
    """the int32 words mmvae_mmgen_build_tables writes"""
    buf = np.zeros(TABLE_WORDS, dtype=np.int32)
    for s in range(SIDE_MIN, SIDE_MAX + 1):
        for xx, (xmin, taps) in enumerate(coefficients(s)):
            assert 1 <= len(taps) <= MAX_TAPS
            o = (s - SIDE_MIN) * SIDE_WORDS + xx * COEF_WORDS
            buf[o], buf[o + 1] = xmin, len(taps)
            buf[o + 2:o + 2 + len(taps)] = taps
    buf[T_OFFSET:] = side_thresholds().view(np.int32)
    return buf


_DENSE = {}


def dense(side, n_in=DIGIT):
    """the coefficient rows as an int64 (side, n_in) matrix"""
    if (side, n_in) not in _DENSE:
        K = np.zeros((side, n_in), dtype=np.int64)
        for xx, (xmin, taps) in enumerate(coefficients(side, n_in)):
            K[xx, xmin:xmin + len(taps)] = taps
        _DENSE[(side, n_in)] = K
    return _DENSE[(side, n_in)]


def _pass(x, K):
    return np.clip(((1 << 21) + x.astype(np.int64) @ K.T) >> 22, 0, 255).astype(np.uint8)


def resize(img, side):
    """Pillow's Image.resize((side, side), BILINEAR) of an 8-bit square image: horizontal pass, 8-bit intermediate, vertical pass"""
    K = dense(side, img.shape[0])
    return _pass(_pass(img, K).T, K).T


_T = side_thresholds()


def side_of(u):
    """the smallest s with u < T[s], SIDE_MAX when there is none (arrays allowed)"""
    return SIDE_MIN + np.minimum((np.asarray(u, dtype=np.uint32)[..., None] >= _T[:-1]).sum(-1), N_SIDES - 1)


def flags_of(fixed=False, resize=True, translate=True, reverse=False, scramble=False, no_repeat=False):
    if reverse and scramble:
        reverse = False
    return (F_FIXED if fixed else 0) | (0 if resize else F_NO_RESIZE) | (0 if translate else F_NO_TRANSLATE) | (F_REVERSE if reverse else 0) \
        | (F_SCRAMBLE if scramble else 0) | (F_NO_REPEAT if no_repeat else 0)


def draw_digit(seed, c, a, j, t, flags, M):
    r = philox(seed, c, 1 + ((a * 4 + j) * MAX_REDRAWS + t))
    index = int(mulhi(r[0], M))
    if flags & F_FIXED:
        return index, FIXED_SIDE, FIXED_PADS[j][0], FIXED_PADS[j][1]
    side = DIGIT if flags & F_NO_RESIZE else int(side_of(r[1]))
    pad = CANVAS - side
    if flags & F_NO_TRANSLATE:
        return index, side, pad // 2, pad // 2
    return index, side, int(mulhi(r[2], pad)), int(mulhi(r[3], pad))


def label_order(k, reverse_bit, scramble_value, flags):
    order = list(range(k))
    if flags & F_SCRAMBLE:
        left, v, order = list(range(MAX_DIGITS)), int(scramble_value), []
        for i in range(k):
            f = math.factorial(k - 1 - i)
            order.append(left.pop(v // f))
            v %= f
    elif flags & F_REVERSE and reverse_bit:
        order = order[::-1]
    return order


def render_sum(digits, slots):
    """int64 (50,50) sum of the resized digits; slots: (index, side, top, left)"""
    canvas = np.zeros((CANVAS, CANVAS), dtype=np.int64)
    for index, side, top, left in slots:
        canvas[top:top + side, left:left + side] += resize(digits[index], side)
    return canvas


def render(digits, params):
    """mmvae_mmgen_render: params (n,4,4) -> (uint8 (n,50,50), overflow (n,))"""
    images = np.zeros((len(params), CANVAS, CANVAS), dtype=np.uint8)
    overflow = np.zeros(len(params), dtype=np.int32)
    for i, p in enumerate(params):
        canvas = render_sum(digits, [tuple(int(v) for v in s) for s in p if s[0] >= 0])
        overflow[i] = int(canvas.max() > 255)
        images[i] = np.minimum(canvas, 255)
    return images, overflow


def generate(digits, labels, n, seed=0, first=0, flags=0, min_digits=0, max_digits=2):
    """mmvae_mmgen_generate -> (images uint8 (n,50,50), text int64 (n,4), params int32 (n,4,4), attempts int32 (n,))"""
    M = len(digits)
    images = np.zeros((n, CANVAS, CANVAS), dtype=np.uint8)
    text = np.full((n, MAX_DIGITS), FILL, dtype=np.int64)
    params = np.zeros((n, MAX_DIGITS, 4), dtype=np.int32)
    params[:, :, 0] = -1
    attempts = np.zeros(n, dtype=np.int32)
    for i in range(n):
        c = first + i
        r = philox(seed, c, 0)
        k = min_digits + int(mulhi(r[0], max_digits - min_digits + 1))
        order = label_order(k, int(r[1]) >> 31, mulhi(r[2], math.factorial(k)), flags)
        for a in range(MAX_ATTEMPTS):
            slots, labs, drawn = [], [], True
            for j in range(k):
                found = False
                for t in range(MAX_REDRAWS if flags & F_NO_REPEAT else 1):
                    d = draw_digit(seed, c, a, j, t, flags, M)
                    lab = int(labels[d[0]])
                    if not (flags & F_NO_REPEAT) or lab not in labs:
                        found = True
                        break
                if not found:
                    drawn = False
                    break
                slots.append(d)
                labs.append(lab)
            if not drawn:
                continue
            canvas = render_sum(digits, slots)
            if canvas.max() <= 255:
                images[i] = canvas
                attempts[i] = a + 1
                for j in range(k):
                    params[i, j] = slots[j]
                    text[i, j] = labs[order[j]]
                break
    return images, text, params, attempts


# ---- the inputs the CPU and the GPU tests share
def crafted_digits():
    """16 digits, every second one with bright left and right borders: two of those side by side in fixed mode (slots 0 and 1 share
    columns 23 and 24) pass 255, so canvases do retry"""
    d = np.zeros((16, DIGIT, DIGIT), dtype=np.uint8)
    d[:, 8:20, 8:20] = 90
    d[::2, :, :3] = 200
    d[::2, :, -3:] = 200
    return d, (np.arange(16) % 10).astype(np.int64)


# name -> (digit set, canvases, seed, mode arguments of multimnist_gen.generate)
CASES = {
    "random_0_4": ("synthetic", 257, 0, dict(min_digits=0, max_digits=4)),
    "no_resize": ("synthetic", 40, 1, dict(resize=False, min_digits=0, max_digits=4)),
    "no_translate": ("synthetic", 40, 1, dict(translate=False, min_digits=0, max_digits=2)),
    "empty": ("synthetic", 9, 1, dict(min_digits=0, max_digits=0)),
    "four": ("synthetic", 40, 1, dict(min_digits=4, max_digits=4)),
    "fixed_reverse": ("synthetic", 40, 1, dict(fixed=True, reverse=True, min_digits=0, max_digits=4)),
    "fixed_scramble": ("synthetic", 40, 1, dict(fixed=True, scramble=True, min_digits=0, max_digits=4)),
    "fixed_no_repeat": ("synthetic", 40, 1, dict(fixed=True, no_repeat=True, min_digits=0, max_digits=4)),
    "fixed_crafted": ("crafted", 40, 1, dict(fixed=True, no_repeat=True, scramble=True, min_digits=0, max_digits=4)),
}
_CASE_CACHE = {}


def case(name):
    """-> (digits uint8 (M,28,28), labels int64 (M,), n, seed, mode, (images, text, params, attempts) of the reference), computed once"""
    if name not in _CASE_CACHE:
        which, n, seed, mode = CASES[name]
        if which == "synthetic":
            from multimodal_vae_amd import data as D
            d, l = D.synthetic_mnist(64, 0)
            d, l = d.numpy(), l.numpy()
        else:
            d, l = crafted_digits()
        flags = flags_of(**{k: v for k, v in mode.items() if k not in ("min_digits", "max_digits")})
        _CASE_CACHE[name] = (d, l, n, seed, mode, generate(d, l, n, seed=seed, flags=flags, min_digits=mode["min_digits"], max_digits=mode["max_digits"]))
    return _CASE_CACHE[name]
