// MultiMNIST synthesis (multimnist/datasets.py): what a canvas is made of, stated once.  Pure C++17 (no HIP-only construct; the
// one qualifier macro below is empty for a host compiler): the kernels of multimnist_gen.hip, the host table builder behind
// mmvae_mmgen_build_tables and the stand-alone host program tests/host/mmgen_core_check.cpp all compile THIS text, and
// tests/multimnist_gen_ref.py restates it in numpy.
//
// Resize.  The reference resizes a 28 x 28 digit with scipy.misc.imresize(digit, 1 / scale) = Pillow's 8-bit BILINEAR resample to
// (s, s), s = int(28 * (1 / scale)): a horizontal pass 28 -> s, then a vertical pass 28 -> s, with an 8-bit intermediate.  Both
// passes use the same coefficients.  Per output index xx, with scale = 28 / s, fs = max(scale, 1), support = fs, ss = 1 / fs:
//   center = (xx + 0.5) scale;  xmin = max(int(center - support + 0.5), 0);  xmax = min(int(center + support + 0.5), 28)
//   w_x = max(0, 1 - |(x + xmin - center + 0.5) ss|), x < xmax - xmin, divided by their sum (double)
//   k_x = int(w_x 2^22 + 0.5);   out = clamp((2^21 + sum_x pixel[xmin + x] k_x) >> 22, 0, 255)
// Sides SIDE_MIN .. SIDE_MAX need at most MAX_TAPS taps (build_tables checks it); side 28 is the identity.
//
// Draws.  gen(seed, ctr, stream) is Philox4x32-10 with the keying of common.h's Philox::gen; mulhi(a, b) = (a b) >> 32.
//   canvas c (64-bit, global: first_canvas + local index):  R = gen(seed, c, 0)
//     k = min_digits + mulhi(R[0], max_digits - min_digits + 1);  reverse bit = R[1] >> 31 (labels reversed when set);
//     scramble: v = mulhi(R[2], k!), Lehmer code: for i = 0 .. k-1: d = v / (k-1-i)!, v %= (k-1-i)!, label i of the result is the
//     d-th of the labels not yet taken (in slot order)
//   digit of attempt a, slot j, redraw t:  D = gen(seed, c, 1 + ((a 4 + j) MAX_REDRAWS + t))
//     index = mulhi(D[0], M);  side = the smallest s with D[1] < T[s], SIDE_MAX when there is none;
//     top = mulhi(D[2], 50 - side);  left = mulhi(D[3], 50 - side)
//   T[s] = floor(2^32 P(side <= s)), P(side <= s) = 1 - Phi((28 / (s + 1) - 1.3) / 0.1) = erfc(z / sqrt 2) / 2 in double: the side
//   int(28 / N(1.3, 0.1)) of the reference.  T[SIDE_MAX] = 2^32 - 1 and is never compared.
// Modes.  no_resize: side = 28.  no_translate: top = left = (50 - side) / 2.  fixed: side = 21 = int(28 / 1.3), slot j sits at
// (4,4), (4,23), (23,4), (23,23); no_repeat (fixed only) redraws a slot (t = 1, 2, ...) until its label differs from the labels of
// the slots before it.  reverse and scramble are drawn once per canvas, not once per attempt: they do not depend on the pixels.
// Rejection.  The digits of an attempt are summed; a sum above 255 anywhere rejects the attempt and a + 1 is drawn with the same k.
// A slot that is still a repeat after MAX_REDRAWS draws rejects the attempt too.  After MAX_ATTEMPTS rejected attempts the canvas is
// reported as failed: zeros, FILL text, attempts = 0 (the reference would recurse for ever).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MMGEN_HD __host__ __device__
#else
#define MMGEN_HD
#endif

namespace mmgen {

enum {
    CANVAS = 50,
    DIGIT = 28,
    SIDE_MIN = 14,
    SIDE_MAX = 41,
    N_SIDES = SIDE_MAX - SIDE_MIN + 1,
    MAX_TAPS = 5,
    MAX_DIGITS = 4,
    MAX_ATTEMPTS = 64,
    MAX_REDRAWS = 64,
    FIXED_SIDE = 21,
    FILL = 11,                               // utils.FILL
    PRECISION_BITS = 22,
    // table layout, int32 words: [N_SIDES][SIDE_MAX][COEF_WORDS] = (xmin, tap count, MAX_TAPS taps) per output index (rows past the
    // side are zero), then the N_SIDES thresholds T as uint32
    COEF_WORDS = 2 + MAX_TAPS,
    SIDE_WORDS = SIDE_MAX * COEF_WORDS,
    T_OFFSET = N_SIDES * SIDE_WORDS,
    TABLE_WORDS = T_OFFSET + N_SIDES,
};
enum { F_FIXED = 1, F_NO_RESIZE = 2, F_NO_TRANSLATE = 4, F_REVERSE = 8, F_SCRAMBLE = 16, F_NO_REPEAT = 32, F_ALL = 63 };

MMGEN_HD inline uint32_t mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

MMGEN_HD inline void philox(uint64_t seed, uint64_t ctr, uint32_t stream, uint32_t (&out)[4]) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = stream, c3 = 0x5bd1e995u;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int i = 0; i < 10; ++i) {
        const uint32_t hi0 = mulhi(M0, c0), lo0 = M0 * c0, hi1 = mulhi(M1, c2), lo1 = M1 * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

MMGEN_HD inline bool flags_ok(int flags, int min_digits, int max_digits) {
    if (flags & ~F_ALL) return false;
    if ((flags & (F_REVERSE | F_SCRAMBLE | F_NO_REPEAT)) && !(flags & F_FIXED)) return false;
    return 0 <= min_digits && min_digits <= max_digits && max_digits <= MAX_DIGITS;
}

struct CanvasDraw { int k; int reverse; uint32_t scramble; };

MMGEN_HD inline uint32_t factorial(int n) { return n < 2 ? 1u : n == 2 ? 2u : n == 3 ? 6u : 24u; }

MMGEN_HD inline CanvasDraw draw_canvas(uint64_t seed, uint64_t c, int min_digits, int max_digits) {
    uint32_t r[4];
    philox(seed, c, 0u, r);
    CanvasDraw d;
    d.k = min_digits + (int)mulhi(r[0], (uint32_t)(max_digits - min_digits + 1));
    d.reverse = (int)(r[1] >> 31);
    d.scramble = mulhi(r[2], factorial(d.k));
    return d;
}

// order[i] = the slot whose label becomes label i of the text.  (Fixed-bound loops and no array indexed by a run-time value: on the
// device everything here stays in registers.)
MMGEN_HD inline void label_order(const CanvasDraw& d, int flags, int (&order)[MAX_DIGITS]) {
    const int k = d.k;
    for (int i = 0; i < MAX_DIGITS; ++i) order[i] = i;
    if (flags & F_SCRAMBLE) {
        uint32_t v = d.scramble, taken = 0;
        for (int i = 0; i < MAX_DIGITS; ++i) {
            if (i >= k) continue;
            const uint32_t f = factorial(k - 1 - i);
            const int q = (int)(v / f);
            v %= f;
            int seen = 0, pick = 0;
            for (int j = 0; j < MAX_DIGITS; ++j)
                if (!((taken >> j) & 1u)) {
                    if (seen == q) pick = j;
                    ++seen;
                }
            taken |= 1u << pick;
            order[i] = pick;
        }
    } else if ((flags & F_REVERSE) && d.reverse) {
        for (int i = 0; i < MAX_DIGITS; ++i)
            if (i < k) order[i] = k - 1 - i;
    }
}

MMGEN_HD inline int side_of(uint32_t u, const uint32_t* T) {
    for (int s = SIDE_MIN; s < SIDE_MAX; ++s)
        if (u < T[s - SIDE_MIN]) return s;
    return SIDE_MAX;
}

struct DigitDraw { int index, side, top, left; };

MMGEN_HD inline uint32_t digit_stream(int attempt, int slot, int redraw) {
    return 1u + (uint32_t)((attempt * MAX_DIGITS + slot) * MAX_REDRAWS + redraw);
}

MMGEN_HD inline DigitDraw draw_digit(uint64_t seed, uint64_t c, int attempt, int slot, int redraw, int flags, uint32_t M, const uint32_t* T) {
    uint32_t r[4];
    philox(seed, c, digit_stream(attempt, slot, redraw), r);
    DigitDraw d;
    d.index = (int)mulhi(r[0], M);
    if (flags & F_FIXED) {
        d.side = FIXED_SIDE;
        d.top = slot < 2 ? 4 : 23;
        d.left = (slot & 1) ? 23 : 4;
        return d;
    }
    d.side = (flags & F_NO_RESIZE) ? (int)DIGIT : side_of(r[1], T);
    const uint32_t pad = (uint32_t)(CANVAS - d.side);
    d.top = (flags & F_NO_TRANSLATE) ? (int)(pad / 2) : (int)mulhi(r[2], pad);
    d.left = (flags & F_NO_TRANSLATE) ? (int)(pad / 2) : (int)mulhi(r[3], pad);
    return d;
}

// ---- host side: the tables.  Returns the largest tap count met, or -1 when a side needs more than MAX_TAPS (nothing is then valid).
inline int build_tables(int32_t* buf) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int i = 0; i < TABLE_WORDS; ++i) buf[i] = 0;
    int most = 0;
    for (int s = SIDE_MIN; s <= SIDE_MAX; ++s) {
        const double scale = (double)DIGIT / s;
        const double fs = scale < 1.0 ? 1.0 : scale;
        const double support = fs, ss = 1.0 / fs;
        for (int xx = 0; xx < s; ++xx) {
            const double center = (xx + 0.5) * scale;
            int xmin = (int)(center - support + 0.5);
            if (xmin < 0) xmin = 0;
            int xmax = (int)(center + support + 0.5);
            if (xmax > DIGIT) xmax = DIGIT;
            const int n = xmax - xmin;
            if (n < 1 || n > MAX_TAPS) return -1;
            double w[MAX_TAPS], ww = 0.0;
            for (int x = 0; x < n; ++x) {
                double a = (x + xmin - center + 0.5) * ss;
                if (a < 0.0) a = -a;
                w[x] = a < 1.0 ? 1.0 - a : 0.0;
                ww += w[x];
            }
            int32_t* row = buf + (s - SIDE_MIN) * SIDE_WORDS + xx * COEF_WORDS;
            row[0] = xmin;
            row[1] = n;
            for (int x = 0; x < n; ++x) {
                const double v = ww != 0.0 ? w[x] / ww : w[x];
                row[2 + x] = (int32_t)(v * (double)(1 << PRECISION_BITS) + 0.5);
            }
            if (n > most) most = n;
        }
    }
    uint32_t* T = reinterpret_cast<uint32_t*>(buf + T_OFFSET);
    for (int s = SIDE_MIN; s <= SIDE_MAX; ++s) {
        const double z = ((double)DIGIT / (s + 1) - 1.3) / 0.1;
        const double p = 0.5 * erfc(z / sqrt(2.0)) * 4294967296.0;
        T[s - SIDE_MIN] = s == SIDE_MAX || p >= 4294967295.0 ? 0xffffffffu : (uint32_t)p;
    }
    return most;
}

// one pass over a line of DIGIT 8-bit pixels read with `stride`: the output at index xx of the side whose coefficient rows are `rows`
MMGEN_HD inline int resample_at(const uint8_t* line, int stride, const int32_t* rows, int xx) {
    const int32_t* row = rows + xx * COEF_WORDS;
    int n = row[1] < MAX_TAPS ? row[1] : (int)MAX_TAPS;
    int x0 = row[0] < 0 ? 0 : row[0];
    if (x0 > DIGIT - n) x0 = DIGIT - n;                       // (a table that is not build_tables' own cannot leave the line)
    int acc = 1 << (PRECISION_BITS - 1);
    for (int x = 0; x < n; ++x) acc += (int)line[(x0 + x) * stride] * row[2 + x];
    acc >>= PRECISION_BITS;
    return acc < 0 ? 0 : acc > 255 ? 255 : acc;
}

}  // namespace mmgen
