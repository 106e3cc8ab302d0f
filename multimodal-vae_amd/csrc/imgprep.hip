// Scale + CenterCrop + ToTensor of a ragged image batch on the device: see imgprep.h (kernel) and imgprep_core.h (arithmetic, limits).
#include "imgprep.h"

using namespace imgprep;

namespace {

struct Lds {
    double ww[2][MAX_OUT];                       // per axis (0 horizontal, 1 vertical) and window index: weight sum,
    int xmin[2][MAX_OUT];                        //   first tap,
    int n[2][MAX_OUT];                           //   tap count
    int coef[2][COEF_CAP];                       // [index][most taps] when the axis is cached
    uint32_t stage[STAGE_BYTES / 4];             // input rows, each from its 4-byte aligned address on
    uint8_t tmp[LDS_BUDGET];                     // after the horizontal pass: [row][S][3]
};
static_assert(sizeof(Lds) <= 160 * 1024, "LDS of a gfx950 workgroup");

constexpr int HALF = 1 << (PRECISION_BITS - 1);
constexpr int STAGE_U = STAGE_BYTES / 4 / IMGPREP_THREADS;   // dwords of a stage round per lane
static_assert(STAGE_U * IMGPREP_THREADS * 4 == STAGE_BYTES, "a round is a whole number of dwords per lane");

__global__ __launch_bounds__(IMGPREP_THREADS) void imgprep_kernel(const uint8_t* __restrict__ pixels, long long pixels_bytes,
                                                                 const long long* __restrict__ offsets, const int* __restrict__ heights,
                                                                 const int* __restrict__ widths, int S, uint8_t* __restrict__ out_u8,
                                                                 float* __restrict__ out_f32, int* __restrict__ status) {
    extern __shared__ __align__(16) unsigned char smem[];
    Lds& s = *reinterpret_cast<Lds*>(smem);
    const int img = blockIdx.x, tid = threadIdx.x;
    const int h = heights[img], w = widths[img];
    const long long off = offsets[img];
    const long long obase = (long long)img * 3 * S * S;
    // (uniform: the whole workgroup leaves, or none of it)
    if (!sides_ok(h, w) || off < 0 || off > pixels_bytes || 3ll * h * w > pixels_bytes - off) {
        for (int i = tid; i < 3 * S * S; i += IMGPREP_THREADS) {
            if (out_u8) out_u8[obase + i] = 0;
            if (out_f32) out_f32[obase + i] = 0.0f;
        }
        if (tid == 0) status[img] = -1;
        return;
    }
    int ow, oh;
    scaled_size(w, h, S, &ow, &oh);
    const int first[2] = {crop_offset(ow - S), crop_offset(oh - S)};
    const int n_in[2] = {w, h}, n_out[2] = {ow, oh};

    for (int i = tid; i < 2 * S; i += IMGPREP_THREADS) {
        const int ax = i >= S ? 1 : 0, j = i - ax * S;
        const Span sp = span_of(ax ? h : w, ax ? oh : ow, (ax ? first[1] : first[0]) + j);
        s.xmin[ax][j] = sp.xmin;
        s.n[ax][j] = sp.n;
        s.ww[ax][j] = sp.ww;
    }
    __syncthreads();
    int T[2] = {1, 1};
    for (int j = 0; j < S; ++j) {
        T[0] = max(T[0], s.n[0][j]);
        T[1] = max(T[1], s.n[1][j]);
    }
    const bool cached[2] = {S * T[0] <= COEF_CAP, S * T[1] <= COEF_CAP};
#pragma unroll
    for (int ax = 0; ax < 2; ++ax) {
        if (!cached[ax]) continue;
        for (int i = tid; i < S * T[ax]; i += IMGPREP_THREADS) {
            const int j = i / T[ax], t = i - j * T[ax];
            s.coef[ax][i] = t < s.n[ax][j] ? coef_at(n_in[ax], n_out[ax], first[ax] + j, s.xmin[ax][j], s.ww[ax][j], t) : 0;
        }
    }
    // the input columns the window depends on (xmin and xmin + n do not decrease with the index), and the stage's geometry
    const int cx0 = s.xmin[0][0], cx1 = s.xmin[0][S - 1] + s.n[0][S - 1];
    const int SD = ((cx1 - cx0) * 3 + 6) >> 2;                   // dwords per staged row: up to 3 bytes of lead, rounded up
    const int stage_rows = (STAGE_BYTES / 4) / SD;
    const int band_rows = LDS_BUDGET / (3 * S);
    const uintptr_t P = reinterpret_cast<uintptr_t>(pixels), Pend = P + (uintptr_t)pixels_bytes;
    const uintptr_t base = P + (uintptr_t)off;

    // the dwords of input rows rc .. rc + nr - 1 (nr <= stage_rows), STAGE_U per lane, dword j of the round = (row j / SD, dword j % SD
    // from the row's 4-byte aligned address); loads only, so that they are all in flight before the first is waited for
    auto fetch = [&](int rc, int nr, uint32_t (&v)[STAGE_U]) {
#pragma unroll
        for (int u = 0; u < STAGE_U; ++u) {
            const int j = tid + u * IMGPREP_THREADS;
            v[u] = 0;
            if (j < nr * SD) {
                const int r = j / SD, d = j - r * SD;
                const uintptr_t q = ((base + ((uintptr_t)(rc + r) * w + cx0) * 3) & ~(uintptr_t)3) + 4 * (uintptr_t)d;
                if (q >= P && q + 4 <= Pend) {
                    v[u] = *reinterpret_cast<const uint32_t*>(q);
                } else {                         // a dword that leaves the buffer: only the bytes inside it
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (q + b >= P && q + b < Pend) v[u] |= (uint32_t)*reinterpret_cast<const uint8_t*>(q + b) << (8 * b);
                }
            }
        }
    };

    int yy0 = 0;
    while (yy0 < S) {
        // the band: output rows yy0 .. ye - 1, as many as their input rows ra .. rb - 1 fit
        const int ra = s.xmin[1][yy0];
        int ye = yy0 + 1;
        while (ye < S && s.xmin[1][ye] + s.n[1][ye] - ra <= band_rows) ++ye;
        const int rb = min(s.xmin[1][ye - 1] + s.n[1][ye - 1], ra + band_rows);      // (the min never binds: imgprep_core.h, Limits)
        // rounds of stage_rows input rows; the dwords of round k + 1 are in flight, in registers, while round k is resampled
        int rc = ra, nr = min(stage_rows, rb - ra);
        uint32_t v[STAGE_U];
        fetch(rc, nr, v);
        while (nr > 0) {
            __syncthreads();                     // the stage and tmp are free: the passes that read them are done (and coef is written)
#pragma unroll
            for (int u = 0; u < STAGE_U; ++u) {
                const int j = tid + u * IMGPREP_THREADS;
                if (j < nr * SD) s.stage[j] = v[u];
            }
            __syncthreads();
            const int rc_next = rc + nr, nr_next = min(stage_rows, rb - rc_next);
            if (nr_next > 0) fetch(rc_next, nr_next, v);
            for (int i = tid; i < nr * S; i += IMGPREP_THREADS) {
                const int r = i / S, xx = i - r * S;
                const int lead = (int)((base + ((uintptr_t)(rc + r) * w + cx0) * 3) & 3);
                const int xmin = s.xmin[0][xx], n = s.n[0][xx];
                const uint8_t* src = reinterpret_cast<const uint8_t*>(s.stage) + r * SD * 4 + lead + (xmin - cx0) * 3;
                int a0 = HALF, a1 = HALF, a2 = HALF;
                if (cached[0]) {
                    const int* k = s.coef[0] + xx * T[0];
#pragma unroll 4
                    for (int t = 0; t < n; ++t) {
                        a0 += (int)src[3 * t] * k[t];
                        a1 += (int)src[3 * t + 1] * k[t];
                        a2 += (int)src[3 * t + 2] * k[t];
                    }
                } else {
                    const double ww = s.ww[0][xx];
                    for (int t = 0; t < n; ++t) {
                        const int k = coef_at(w, ow, first[0] + xx, xmin, ww, t);
                        a0 += (int)src[3 * t] * k;
                        a1 += (int)src[3 * t + 1] * k;
                        a2 += (int)src[3 * t + 2] * k;
                    }
                }
                uint8_t* dst = s.tmp + ((rc + r - ra) * S + xx) * 3;
                dst[0] = (uint8_t)clip8(a0);
                dst[1] = (uint8_t)clip8(a1);
                dst[2] = (uint8_t)clip8(a2);
            }
            rc = rc_next;
            nr = nr_next;
        }
        __syncthreads();
        const int nb = ye - yy0;
        for (int i = tid; i < 3 * nb * S; i += IMGPREP_THREADS) {
            const int c = i / (nb * S), rem = i - c * nb * S, yl = rem / S, xx = rem - yl * S, yy = yy0 + yl;
            const int xmin = s.xmin[1][yy], n = min(s.n[1][yy], rb - xmin);
            const uint8_t* src = s.tmp + ((xmin - ra) * S + xx) * 3 + c;
            int acc = HALF;
            if (cached[1]) {
                const int* k = s.coef[1] + yy * T[1];
#pragma unroll 8
                for (int t = 0; t < n; ++t) acc += (int)src[t * S * 3] * k[t];
            } else {
                const double ww = s.ww[1][yy];
                for (int t = 0; t < n; ++t) acc += (int)src[t * S * 3] * coef_at(h, oh, first[1] + yy, xmin, ww, t);
            }
            const int v = clip8(acc);
            const long long o = obase + ((long long)c * S + yy) * S + xx;
            if (out_u8) out_u8[o] = (uint8_t)v;
            if (out_f32) out_f32[o] = __fdiv_rn((float)v, 255.0f);
        }
        yy0 = ye;
    }
    if (tid == 0) status[img] = 0;
}

}  // namespace

int launch_imgprep_scale_crop(const uint8_t* pixels, long long pixels_bytes, const long long* offsets, const int* heights, const int* widths,
                              int n, int S, uint8_t* out_u8, float* out_f32, int* status, hipStream_t st) {
    if (n == 0) return MMVAE_OK;
    static std::atomic<unsigned> attr_set{0};
    if (mmvae_first_use_on_device(attr_set))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&imgprep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Lds));
    MMVAE_LAUNCH(imgprep_kernel, dim3((unsigned)n), dim3(IMGPREP_THREADS), sizeof(Lds), st, pixels, pixels_bytes, offsets, heights, widths, S,
                 out_u8, out_f32, status);
    return mmvae_check_launch("imgprep_scale_crop");
}
