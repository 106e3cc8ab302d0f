// See mnist_strip.h.
//
// Workgroup = 16 output features (blockIdx.x) x all rows, 8 waves.  Wave w owns the 16-row tiles w, w + 8, ... (T of them, a
// template parameter: 1 up to 128 rows, 2 up to 256, 4 up to 512), f32x4 accumulators per tile: lane -> feature lane % 16, rows
// 4 (lane / 16) .. + 3 of the tile (the accumulator layout of v_mfma_f32_16x16x4_f32, as gemm_f32.hip).  Within a 16-deep step MFMA q
// of lane group fq consumes k = k0 + 4 fq + q on both operands, so an operand that is contiguous along k is one 16-byte load per lane
// per step.  Operands go through buffer descriptors of exactly their size; a row past the batch, a feature past N or a k past K is
// the offset 0xFFFFFFFF, which the hardware range check turns into 0.  U steps of loads are issued before their MFMAs, and each of
// the U steps accumulates into a partial of its own.
//
// The sums over the rows: every lane adds its T x 4 values in tile order, the 32 (wave, lane group) partials of a feature meet in
// LDS and every lane of that feature adds them in the same fixed order.  No atomics; the result does not depend on scheduling.
#include "mnist_strip.h"
#include "plan_base.h"

namespace {

constexpr int SW = MNIST_STRIP_WAVES, TPB = SW * 64;

// sum over all rows of the workgroup of the per-lane partial `v` of feature `fr`; every lane returns the same bits
__device__ __forceinline__ float strip_fold(float v, float (*part)[16], int wave, int fq, int fr) {
    __syncthreads();
    part[wave * 4 + fq][fr] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < SW * 4; ++i) s += part[i][fr];
    return s;
}

template <int T>
__global__ __launch_bounds__(TPB) void lin_bn_act_fwd32_kernel(const StripFwdArgs a) {
    __shared__ float part[SW * 4][16];
    constexpr int U = T == 1 ? 8 : 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
    const int n = blockIdx.x * 16 + fr;
    const bool nok = n < a.N;
    // U partial accumulators per tile (8 up to 128 rows, else 4), step st of the K loop into partial st % U, added pairwise at the
    // end: independent MFMA chains 1 / U as long (the dependent latency of one chain is hidden behind the others, and the rounding
    // error of a sum of K products grows with the length of the longest chain: at K = 784 one chain gave twice gemm_f32's error in r,
    // which a 2-row BatchNorm amplifies past the step's gates; gemm_f32 splits that K over its 8 waves)
    f32x4 pacc[U][T];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int t = 0; t < T; ++t) pacc[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (wave * 16 < a.rows) {                                   // (uniform per wave: a wave without rows skips the K loop)
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, ((a.rows - 1) * a.ldx + a.K) * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, a.N * a.K * 4, 0x00020000);
        unsigned xrow[T];
        bool rok[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int row = (wave + t * SW) * 16 + fr;
            rok[t] = row < a.rows;
            xrow[t] = (unsigned)row * (unsigned)a.ldx * 4u;
        }
        const unsigned wrow = (unsigned)n * (unsigned)a.K * 4u;
        const int nst = (a.K + 15) >> 4;
        for (int st = 0; st < nst; st += U) {
            f32x4 av[U][T], bv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int kb = (st + u) * 16 + fq * 4;          // K % 4 == 0: the 4 k are all inside or all outside
                const bool kok = kb < a.K;
                bv[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wr, (nok && kok) ? wrow + (unsigned)kb * 4u : 0xFFFFFFFFu, 0, 0));
#pragma unroll
                for (int t = 0; t < T; ++t)
                    av[u][t] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, (rok[t] && kok) ? xrow[t] + (unsigned)kb * 4u : 0xFFFFFFFFu, 0, 0));
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int t = 0; t < T; ++t) pacc[u][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][t][q], bv[u][q], pacc[u][t], 0, 0, 0);
        }
    }
    f32x4 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int w = 1; w < U; w *= 2)                           // pairwise: (0 + 1) + (2 + 3), ...
#pragma unroll
            for (int u = 0; u + w < U; u += 2 * w) pacc[u][t] += pacc[u + w][t];
        acc[t] = pacc[0][t];
    }
    const float bias = nok ? a.bias[n] : 0.f;
    float y[T][4];
    bool ok[T][4];
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ok[t][r] = (wave + t * SW) * 16 + fq * 4 + r < a.rows;
            y[t][r] = acc[t][r] + bias;
            if (ok[t][r]) s += y[t][r];
        }
    float mean, rstd;
    if (a.training) {                                           // two-pass: the mean first, then the centred squares
        mean = strip_fold(s, part, wave, fq, fr) / (float)a.rows;
        float v = 0.f;
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (ok[t][r]) { const float d = y[t][r] - mean; v += d * d; }
        const float var = strip_fold(v, part, wave, fq, fr) / (float)a.rows;         // biased, like nn.BatchNorm1d's normalisation
        rstd = rsqrtf(var + BN_EPS);
        if (wave == 0 && fq == 0 && nok) {
            float rm = a.running_mean[n], rv = a.running_var[n];
            const float unbiased = var * (float)a.rows / (float)(a.rows - 1);
            for (int u = 0; u < a.updates; ++u) {
                rm = (1.f - BN_MOM) * rm + BN_MOM * mean;
                rv = (1.f - BN_MOM) * rv + BN_MOM * unbiased;
            }
            a.running_mean[n] = rm; a.running_var[n] = rv;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) *a.nbt += (long long)a.updates;
    } else {
        mean = nok ? a.running_mean[n] : 0.f;
        rstd = rsqrtf((nok ? a.running_var[n] : 1.f) + BN_EPS);
    }
    if (!nok) return;
    if (wave == 0 && fq == 0) a.mr[n] = make_float2(mean, rstd);
    const float gamma = a.gamma[n], beta = a.beta[n];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (!ok[t][r]) continue;
            const size_t i = (size_t)((wave + t * SW) * 16 + fq * 4 + r) * a.N + n;
            a.r[i] = y[t][r];
            a.a[i] = fmaxf((y[t][r] - mean) * rstd * gamma + beta, 0.f);
        }
}

template <int T>
__global__ __launch_bounds__(TPB) void lin_dgrad_bn_bwd32_kernel(const StripBwdArgs a) {
    __shared__ float part[SW * 4][16];
    constexpr int U = T == 1 ? 8 : 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
    const int n = blockIdx.x * 16 + fr;
    const bool nok = n < a.N;
    // U partial accumulators per tile (8 up to 128 rows, else 4), step st of the K loop into partial st % U, added pairwise at the
    // end: independent MFMA chains 1 / U as long (the dependent latency of one chain is hidden behind the others, and the rounding
    // error of a sum of K products grows with the length of the longest chain: at K = 784 one chain gave twice gemm_f32's error in r,
    // which a 2-row BatchNorm amplifies past the step's gates; gemm_f32 splits that K over its 8 waves)
    f32x4 pacc[U][T];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int t = 0; t < T; ++t) pacc[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (wave * 16 < a.rows) {
        const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dy), 0, a.rows * a.Nn * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w_next), 0, a.Nn * a.N * 4, 0x00020000);
        unsigned drow[T];
        bool rok[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int row = (wave + t * SW) * 16 + fr;
            rok[t] = row < a.rows;
            drow[t] = (unsigned)row * (unsigned)a.Nn * 4u;
        }
        const unsigned wcol = (unsigned)n * 4u, wrs = (unsigned)a.N * 4u;
        const int nst = (a.Nn + 15) >> 4;
        for (int st = 0; st < nst; st += U) {
            f32x4 av[U][T];
            float bv[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int kb = (st + u) * 16 + fq * 4;          // Nn % 4 == 0: the 4 k are all inside or all outside
                const bool kok = kb < a.Nn;
#pragma unroll
                for (int q = 0; q < 4; ++q)                      // W_next(k, n): k strides by N, the 16 lanes of a group read 16 neighbours
                    bv[u][q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wr, (nok && kok) ? (unsigned)(kb + q) * wrs + wcol : 0xFFFFFFFFu, 0, 0));
#pragma unroll
                for (int t = 0; t < T; ++t)
                    av[u][t] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dr, (rok[t] && kok) ? drow[t] + (unsigned)kb * 4u : 0xFFFFFFFFu, 0, 0));
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int t = 0; t < T; ++t) pacc[u][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][t][q], bv[u][q], pacc[u][t], 0, 0, 0);
        }
    }
    f32x4 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int w = 1; w < U; w *= 2)                           // pairwise: (0 + 1) + (2 + 3), ...
#pragma unroll
            for (int u = 0; u + w < U; u += 2 * w) pacc[u][t] += pacc[u + w][t];
        acc[t] = pacc[0][t];
    }
    const float2 m = nok ? a.mr[n] : make_float2(0.f, 0.f);
    const float gamma = nok ? a.gamma[n] : 0.f, beta = nok ? a.beta[n] : 0.f;
    float d[T][4], xh[T][4];
    bool ok[T][4];
    float p1 = 0.f, p2 = 0.f;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = (wave + t * SW) * 16 + fq * 4 + r;
            ok[t][r] = nok && row < a.rows;
            xh[t][r] = ok[t][r] ? (a.r[(size_t)row * a.N + n] - m.x) * m.y : 0.f;
            d[t][r] = (ok[t][r] && xh[t][r] * gamma + beta > 0.f) ? acc[t][r] : 0.f;      // ReLU backward
            p1 += d[t][r]; p2 += d[t][r] * xh[t][r];
        }
    const float s1 = strip_fold(p1, part, wave, fq, fr);
    const float s2 = strip_fold(p2, part, wave, fq, fr);
    if (!nok) return;
    if (wave == 0 && fq == 0) { a.dgamma[n] += s2; a.dbeta[n] += s1; }
    const float inv = 1.f / (float)a.rows;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (!ok[t][r]) continue;
            const int row = (wave + t * SW) * 16 + fq * 4 + r;
            a.d_r[(size_t)row * a.N + n] = gamma * m.y * (d[t][r] - s1 * inv - xh[t][r] * s2 * inv);
        }
}

int tiles_per_wave(int rows) {
    const int t = ceil_div(ceil_div(rows, 16), SW);
    return t <= 1 ? 1 : t <= 2 ? 2 : 4;
}

}  // namespace

int launch_lin_bn_act_fwd32(const StripFwdArgs& a, hipStream_t s) {
    MMVAE_REQUIRE(a.x && a.w && a.bias && a.gamma && a.beta && a.running_mean && a.running_var && a.r && a.a && a.mr && (a.nbt || !a.training),
                  "lin_bn_act_fwd32: null argument");
    MMVAE_REQUIRE(a.rows >= 1 && a.rows <= MNIST_STRIP_MAX_ROWS, "lin_bn_act_fwd32: %d rows (a workgroup carries 1 .. %d)", a.rows, MNIST_STRIP_MAX_ROWS);
    MMVAE_REQUIRE(!a.training || a.rows > 1, "Expected more than 1 value per channel when training");
    MMVAE_REQUIRE(a.N >= 1 && a.K >= 4 && a.K % 4 == 0 && a.ldx >= a.K && a.ldx % 4 == 0 && aligned16(a.x) && aligned16(a.w),
                  "lin_bn_act_fwd32: N=%d K=%d ldx=%d: K and ldx must be multiples of 4, x and W 16-byte aligned", a.N, a.K, a.ldx);
    MMVAE_REQUIRE((long long)a.rows * a.ldx * 4 < 0x7FFFFFFFll && (long long)a.N * a.K * 4 < 0x7FFFFFFFll && a.updates >= 0,
                  "lin_bn_act_fwd32: operand spans more than 2 GiB");
    const dim3 grid(ceil_div(a.N, 16)), block(TPB);
    switch (tiles_per_wave(a.rows)) {
        case 1: MMVAE_LAUNCH(lin_bn_act_fwd32_kernel<1>, grid, block, 0, s, a); break;
        case 2: MMVAE_LAUNCH(lin_bn_act_fwd32_kernel<2>, grid, block, 0, s, a); break;
        default: MMVAE_LAUNCH(lin_bn_act_fwd32_kernel<4>, grid, block, 0, s, a); break;
    }
    return mmvae_check_launch("lin_bn_act_fwd32");
}

int launch_lin_dgrad_bn_bwd32(const StripBwdArgs& a, hipStream_t s) {
    MMVAE_REQUIRE(a.dy && a.w_next && a.r && a.mr && a.gamma && a.beta && a.d_r && a.dgamma && a.dbeta, "lin_dgrad_bn_bwd32: null argument");
    MMVAE_REQUIRE(a.rows >= 1 && a.rows <= MNIST_STRIP_MAX_ROWS, "lin_dgrad_bn_bwd32: %d rows (a workgroup carries 1 .. %d)", a.rows, MNIST_STRIP_MAX_ROWS);
    MMVAE_REQUIRE(a.N >= 1 && a.Nn >= 4 && a.Nn % 4 == 0 && aligned16(a.dy),
                  "lin_dgrad_bn_bwd32: N=%d Nn=%d: Nn must be a multiple of 4, dy 16-byte aligned", a.N, a.Nn);
    MMVAE_REQUIRE((long long)a.rows * a.Nn * 4 < 0x7FFFFFFFll && (long long)a.N * a.Nn * 4 < 0x7FFFFFFFll, "lin_dgrad_bn_bwd32: operand spans more than 2 GiB");
    const dim3 grid(ceil_div(a.N, 16)), block(TPB);
    switch (tiles_per_wave(a.rows)) {
        case 1: MMVAE_LAUNCH(lin_dgrad_bn_bwd32_kernel<1>, grid, block, 0, s, a); break;
        case 2: MMVAE_LAUNCH(lin_dgrad_bn_bwd32_kernel<2>, grid, block, 0, s, a); break;
        default: MMVAE_LAUNCH(lin_dgrad_bn_bwd32_kernel<4>, grid, block, 0, s, a); break;
    }
    return mmvae_check_launch("lin_dgrad_bn_bwd32");
}
