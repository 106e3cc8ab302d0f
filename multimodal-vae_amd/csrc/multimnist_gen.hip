// MultiMNIST canvases on the device: see multimnist_gen.h (kernels) and mmgen_core.h (resize, draws, bounds).
#include "multimnist_gen.h"

using namespace mmgen;

namespace {

struct Lds {
    uint32_t digit[DIGIT * DIGIT / 4];           // the 28 x 28 source, loaded as dwords
    uint8_t tmp[DIGIT * SIDE_MAX + 4];           // after the horizontal pass: [28][side]
    int32_t coef[SIDE_WORDS];                    // the side's coefficient rows
    int32_t canvas[CANVAS * CANVAS];             // sums of the attempt
    int32_t red[MMGEN_THREADS / 64];
};

// adds digit `index`, resized to side x side, at (top, left).  The arguments are workgroup-uniform and in range (the callers see to
// that).  Ends with a barrier: the canvas is complete and the staging buffers are free again.
__device__ __forceinline__ void add_digit(Lds& s, const uint8_t* __restrict__ digits, const int32_t* __restrict__ tables, int index,
                                          int side, int top, int left) {
    const int tid = threadIdx.x;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(digits + (size_t)index * (DIGIT * DIGIT));
    if (tid < DIGIT * DIGIT / 4) s.digit[tid] = src[tid];
    const int32_t* rows = tables + (side - SIDE_MIN) * SIDE_WORDS;
    for (int i = tid; i < side * COEF_WORDS; i += MMGEN_THREADS) s.coef[i] = rows[i];
    __syncthreads();
    const uint8_t* dig = reinterpret_cast<const uint8_t*>(s.digit);
    for (int i = tid; i < DIGIT * side; i += MMGEN_THREADS) {
        const int y = i / side, xx = i - y * side;
        s.tmp[i] = (uint8_t)resample_at(dig + y * DIGIT, 1, s.coef, xx);
    }
    __syncthreads();
    for (int i = tid; i < side * side; i += MMGEN_THREADS) {
        const int yy = i / side, xx = i - yy * side;
        s.canvas[(top + yy) * CANVAS + left + xx] += resample_at(s.tmp + xx, side, s.coef, yy);
    }
    __syncthreads();
}

__device__ __forceinline__ void clear_canvas(Lds& s) {
    for (int i = threadIdx.x; i < CANVAS * CANVAS; i += MMGEN_THREADS) s.canvas[i] = 0;
    __syncthreads();
}

// max over the canvas, the same value in every lane of the workgroup
__device__ __forceinline__ int canvas_max(Lds& s) {
    int m = 0;
    for (int i = threadIdx.x; i < CANVAS * CANVAS; i += MMGEN_THREADS) m = max(m, s.canvas[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) s.red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = s.red[0];
#pragma unroll
    for (int w = 1; w < MMGEN_THREADS / 64; ++w) m = max(m, s.red[w]);
    __syncthreads();                             // (red is written again by the next attempt)
    return m;
}

// the canvas, clamped to 255 (zeros when !keep), as 625 dwords and / or 625 float4
__device__ __forceinline__ void store_canvas(const Lds& s, bool keep, long long canvas, uint8_t* __restrict__ images_u8,
                                             float* __restrict__ images_f32) {
    for (int i = threadIdx.x; i < CANVAS * CANVAS / 4; i += MMGEN_THREADS) {
        uint32_t px[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) px[q] = keep ? (uint32_t)min(s.canvas[4 * i + q], 255) : 0u;
        if (images_u8)
            reinterpret_cast<uint32_t*>(images_u8 + canvas * (CANVAS * CANVAS))[i] = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
        if (images_f32) {
            f32x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = __fdiv_rn((float)px[q], 255.0f);
            reinterpret_cast<f32x4*>(images_f32 + canvas * (CANVAS * CANVAS))[i] = o;
        }
    }
}

__global__ __launch_bounds__(MMGEN_THREADS) void mmgen_kernel(const uint8_t* __restrict__ digits, const long long* __restrict__ labels,
                                                             uint32_t M, const int32_t* __restrict__ tables, int flags, int min_digits,
                                                             int max_digits, uint64_t seed, uint64_t first, uint8_t* __restrict__ images_u8,
                                                             float* __restrict__ images_f32, long long* __restrict__ text,
                                                             int* __restrict__ params, int* __restrict__ attempts_out,
                                                             int* __restrict__ fail_count) {
    __shared__ Lds s;
    const long long local = blockIdx.x;
    const uint64_t c = first + (uint64_t)local;
    const uint32_t* T = reinterpret_cast<const uint32_t*>(tables + T_OFFSET);
    const CanvasDraw cd = draw_canvas(seed, c, min_digits, max_digits);
    const int k = cd.k;
    DigitDraw dd[MAX_DIGITS] = {};
    long long lab[MAX_DIGITS] = {};
    int used = 0;                                // attempts used by the accepted one, 0 = none accepted
    for (int a = 0; a < MAX_ATTEMPTS && !used; ++a) {
        // every draw of the attempt first (uniform: no lane renders a digit of an attempt another lane has rejected)
        bool drawn = true;
        const int redraws = (flags & F_NO_REPEAT) ? (int)MAX_REDRAWS : 1;
#pragma unroll
        for (int j = 0; j < MAX_DIGITS; ++j) {   // (unrolled: dd and lab stay in registers)
            if (j >= k || !drawn) continue;
            bool found = false;
            for (int t = 0; t < redraws && !found; ++t) {
                dd[j] = draw_digit(seed, c, a, j, t, flags, M, T);
                lab[j] = labels[dd[j].index];
                found = true;
                if (flags & F_NO_REPEAT) {
#pragma unroll
                    for (int q = 0; q < j; ++q) found = found && lab[q] != lab[j];
                }
            }
            drawn = found;
        }
        if (!drawn) continue;
        clear_canvas(s);
#pragma unroll
        for (int j = 0; j < MAX_DIGITS; ++j)
            if (j < k) add_digit(s, digits, tables, dd[j].index, dd[j].side, dd[j].top, dd[j].left);
        if (canvas_max(s) <= 255) used = a + 1;  // (k = 0 is accepted at once, with nothing added)
    }
    store_canvas(s, used != 0, local, images_u8, images_f32);
    const int tid = threadIdx.x;
    int order[MAX_DIGITS];
    label_order(cd, flags, order);
    if (tid < MAX_DIGITS) {
        long long v = FILL;
#pragma unroll
        for (int i = 0; i < MAX_DIGITS; ++i)     // (a register array indexed by a lane-dependent value would go to scratch)
#pragma unroll
            for (int j = 0; j < MAX_DIGITS; ++j)
                if (used && tid == i && i < k && order[i] == j) v = lab[j];
        text[local * MAX_DIGITS + tid] = v;
    }
    if (params && tid < MAX_DIGITS * 4) {
        const int j = tid >> 2, f = tid & 3;
        int v = f == 0 ? -1 : 0;
#pragma unroll
        for (int q = 0; q < MAX_DIGITS; ++q)
            if (used && q < k && q == j) v = f == 0 ? dd[q].index : f == 1 ? dd[q].side : f == 2 ? dd[q].top : dd[q].left;
        params[local * (MAX_DIGITS * 4) + tid] = v;
    }
    if (tid == 0) {
        if (attempts_out) attempts_out[local] = used;
        if (!used && fail_count) atomicAdd(fail_count, 1);
    }
}

__global__ __launch_bounds__(MMGEN_THREADS) void mmgen_render_kernel(const uint8_t* __restrict__ digits, int M,
                                                                    const int32_t* __restrict__ tables, const int* __restrict__ params,
                                                                    uint8_t* __restrict__ images_u8, float* __restrict__ images_f32,
                                                                    int* __restrict__ overflow) {
    __shared__ Lds s;
    const long long local = blockIdx.x;
    int p[MAX_DIGITS][4];
    bool ok = true;
    for (int j = 0; j < MAX_DIGITS; ++j) {
        for (int f = 0; f < 4; ++f) p[j][f] = params[local * (MAX_DIGITS * 4) + j * 4 + f];
        if (p[j][0] < 0) continue;                                           // absent slot
        ok = ok && p[j][0] < M && p[j][1] >= SIDE_MIN && p[j][1] <= SIDE_MAX && p[j][2] >= 0 && p[j][3] >= 0 &&
             p[j][2] + p[j][1] <= CANVAS && p[j][3] + p[j][1] <= CANVAS;
    }
    clear_canvas(s);
    if (ok)
        for (int j = 0; j < MAX_DIGITS; ++j)
            if (p[j][0] >= 0) add_digit(s, digits, tables, p[j][0], p[j][1], p[j][2], p[j][3]);
    const int m = canvas_max(s);
    store_canvas(s, ok, local, images_u8, images_f32);
    if (threadIdx.x == 0) overflow[local] = ok ? (m > 255 ? 1 : 0) : -1;
}

}  // namespace

int launch_mmgen_generate(const uint8_t* digits, const long long* labels, int M, const int32_t* tables, int flags, int min_digits,
                          int max_digits, unsigned long long seed, unsigned long long first, int n, uint8_t* images_u8, float* images_f32,
                          long long* text, int* params, int* attempts, int* fail_count, hipStream_t st) {
    if (n == 0) return MMVAE_OK;
    MMVAE_LAUNCH(mmgen_kernel, dim3((unsigned)n), dim3(MMGEN_THREADS), 0, st, digits, labels, (uint32_t)M, tables, flags, min_digits,
                 max_digits, (uint64_t)seed, (uint64_t)first, images_u8, images_f32, text, params, attempts, fail_count);
    return mmvae_check_launch("mmgen_generate");
}

int launch_mmgen_render(const uint8_t* digits, int M, const int32_t* tables, const int* params, int n, uint8_t* images_u8,
                        float* images_f32, int* overflow, hipStream_t st) {
    if (n == 0) return MMVAE_OK;
    MMVAE_LAUNCH(mmgen_render_kernel, dim3((unsigned)n), dim3(MMGEN_THREADS), 0, st, digits, M, tables, params, images_u8, images_f32,
                 overflow);
    return mmvae_check_launch("mmgen_render");
}
