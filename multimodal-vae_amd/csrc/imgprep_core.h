// Scale(S) + CenterCrop(S) + ToTensor of the reference's image pipelines (celeba/train.py:102-104, coco/train.py:107-112; torchvision's
// transforms over Pillow's 8-bit BILINEAR resample), stated once in integers.  Pure C++17 (the one qualifier macro below is empty for a
// host compiler): the kernel of imgprep.hip, the host functions behind mmvae_imgprep_layout / mmvae_imgprep_coeffs and the stand-alone
// host program tests/host/imgprep_core_check.cpp all compile THIS text, and tests/imgprep_ref.py restates it in numpy.
//
// One decoded image: height h, width w, 3 interleaved 8-bit channels (HWC), output side S.
// Scaled size (torchvision's Scale of that era): w <= h: ow = S, oh = int(S h / w); else oh = S, ow = int(S w / h).  Python divides
//   the exact integer S h by w in float64 and truncates.  The quotient of two integers below 2^53 is correctly rounded, and a
//   non-integer S h / w lies at least 1 / w >= 2^-13 from the next integer while the rounding error is below 2^-32: the truncated
//   float quotient IS the integer quotient, and scaled_size uses integer division.  ow >= S and oh >= S follow.
// Resample to (ow, oh) as Image.resize((ow, oh), BILINEAR): a horizontal pass, then a vertical pass over its 8-bit result.  Per axis
//   (n_in -> n_out), output index xx, in float64, NO fused multiply-add anywhere (span_of / coef_at turn contraction off: an FMA changes
//   center - support + 0.5 and the weights in the last bit, and with them xmin and the coefficients):
//     scale = n_in / n_out;  fs = max(scale, 1);  support = fs;  ss = 1 / fs;  center = (xx + 0.5) scale
//     xmin = max(0, int(center - support + 0.5));  xmax = min(n_in, int(center + support + 0.5));  n = xmax - xmin
//     w_t = max(0, 1 - |(t + xmin - center + 0.5) ss|), t < n;  ww = their sum from t = 0 upwards;  k_t = int(0.5 + (w_t / ww) 2^22)
//     out = clip8((2^21 + sum_t pixel[xmin + t] k_t) >> 22), int32 sums
//   (Pillow multiplies by ss = 1 / fs; it does not divide by fs.)  Pillow skips a pass whose size does not change; with n_in == n_out
//   the formulas give xmin = xx and k = (2^22, 0), the identity, so the kernel needs no special case.
// Centre crop to S x S: x1 = (ow - S + 1) / 2, y1 = (oh - S + 1) / 2 -- the reference's int(round(d / 2.)) under Python 2 rounding.
//   Only output columns x1 .. x1 + S - 1 and rows y1 .. y1 + S - 1 are ever computed, from the input rows and columns they depend on.
// Output, planar [3][S][S]: uint8 and / or float32 = u8 / 255 (IEEE division).
//
// Limits.  Input sides 1 .. MAX_SIDE, S 1 .. MAX_OUT.  Both n_out are >= S, so scale <= MAX_SIDE / S, and an output index has
// n = floor(y + 2 scale) - floor(y) <= 2 scale + 1 <= 2 MAX_SIDE / S + 1 taps.  The 8-bit intermediate holds floor(LDS_BUDGET / 3 S)
// rows of 3 S bytes, which is at least n when LDS_BUDGET >= 3 (2 MAX_SIDE + 2 MAX_OUT) (static_assert): the input rows of ONE output
// row always fit, so a band of output rows always exists.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IMGPREP_HD __host__ __device__
#else
#define IMGPREP_HD
#endif

namespace imgprep {

enum {
    MAX_SIDE = 8192,
    MAX_OUT = 128,
    PRECISION_BITS = 22,
    LDS_BUDGET = 50176,                      // bytes of 8-bit intermediate a workgroup keeps: rows x S x 3; more rows -> bands of output rows
    STAGE_BYTES = 32768,                     // input rows staged per round (one row of MAX_SIDE pixels is 24 KB)
    COEF_CAP = 2048,                         // int32 coefficients kept per axis (S x most taps); beyond it they are computed where used
};
static_assert(LDS_BUDGET >= 3 * (2 * MAX_SIDE + 2 * MAX_OUT), "one output row's input rows must fit the intermediate");
static_assert(STAGE_BYTES >= 3 * MAX_SIDE + 8, "one input row must fit the stage");

IMGPREP_HD inline void scaled_size(int w, int h, int S, int* ow, int* oh) {
    if (w <= h) {
        *ow = S;
        *oh = (int)((long long)S * h / w);
    } else {
        *oh = S;
        *ow = (int)((long long)S * w / h);
    }
}

IMGPREP_HD inline int crop_offset(int d) { return (d + 1) / 2; }

IMGPREP_HD inline bool sides_ok(int h, int w) { return h >= 1 && h <= MAX_SIDE && w >= 1 && w <= MAX_SIDE; }

struct Span { int xmin, n; double ww; };

// the taps of output index xx of an axis n_in -> n_out: first input index, count, and the sum of the raw weights
IMGPREP_HD inline Span span_of(int n_in, int n_out, int xx) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double scale = (double)n_in / (double)n_out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = fs, ss = 1.0 / fs;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > n_in) xmax = n_in;
    Span s;
    s.xmin = xmin;
    s.n = xmax > xmin ? xmax - xmin : 0;
    s.ww = 0.0;
    for (int t = 0; t < s.n; ++t) {
        double a = (t + xmin - center + 0.5) * ss;
        if (a < 0.0) a = -a;
        s.ww += a < 1.0 ? 1.0 - a : 0.0;
    }
    return s;
}

// coefficient t of that span (xmin, ww as span_of gave them)
IMGPREP_HD inline int coef_at(int n_in, int n_out, int xx, int xmin, double ww, int t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double scale = (double)n_in / (double)n_out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double ss = 1.0 / fs;
    const double center = (xx + 0.5) * scale;
    double a = (t + xmin - center + 0.5) * ss;
    if (a < 0.0) a = -a;
    double v = a < 1.0 ? 1.0 - a : 0.0;
    if (ww != 0.0) v = v / ww;
    return (int)(0.5 + v * (double)(1 << PRECISION_BITS));
}

IMGPREP_HD inline int clip8(int acc) {
    acc >>= PRECISION_BITS;
    return acc < 0 ? 0 : acc > 255 ? 255 : acc;
}

}  // namespace imgprep
