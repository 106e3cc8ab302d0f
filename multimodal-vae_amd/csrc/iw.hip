// Importance-sampled marginal log-likelihood: particles, accumulator, finalize (iw.h).
//
//   log w_k = log-likelihood(z_k) + log p(z_k) - log q(z_k),   log p^ = logsumexp_k(log w_k) - log K,
//   ESS = (sum_k w_k)^2 / sum_k w_k^2.
// log w is around -1e3 nats and spreads over tens to hundreds between particles, so the sums carry a running maximum.
// Every example has ONE owner (a wave) in the accumulator: the chunk's merge into the caller's state needs no atomics and the
// result does not depend on scheduling.
#include "iw.h"
#include <cfloat>

namespace {

constexpr int TPB = 256;
constexpr unsigned IW_STREAM = 0x49570000u;      // Philox stream ids of the particles (+ the dimension quad)

// particles: 8 rows per workgroup, lane j of a 32-lane half-wave owns dimensions 4j .. 4j+3 (D <= 128)
__global__ __launch_bounds__(TPB) void iw_particles_kernel(const float* mu, const float* lv, int B, int D, int K, long long first_row,
                                                           long long first_particle, unsigned long long seed, const float* eps,
                                                           float* z, float* log_ratio) {
    const int j = threadIdx.x & 31;
    const long long row = (long long)blockIdx.x * (TPB / 32) + (threadIdx.x >> 5);
    const bool live = row < (long long)B * K;
    float acc = 0.f;
    if (live && 4 * j < D) {
        const int b = (int)(row / K), k = (int)(row - (long long)b * K);
        float e[4];
        if (eps) {
#pragma unroll
            for (int q = 0; q < 4; ++q) e[q] = 4 * j + q < D ? eps[row * D + 4 * j + q] : 0.f;
        } else {
            uint32_t r[4];
            const uint64_t ctr = ((uint64_t)(uint32_t)(first_row + b) << 32) | (uint32_t)(first_particle + k);
            Philox::gen(seed, ctr, IW_STREAM + (unsigned)j, r);
            const float u0 = u01(r[0]), u1 = u01(r[1]), u2 = u01(r[2]), u3 = u01(r[3]);
            const float m0 = sqrtf(-2.0f * logf(u0)), m1 = sqrtf(-2.0f * logf(u2));
            e[0] = m0 * cosf(6.28318530718f * u1); e[1] = m0 * sinf(6.28318530718f * u1);
            e[2] = m1 * cosf(6.28318530718f * u3); e[3] = m1 * sinf(6.28318530718f * u3);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d = 4 * j + q;
            if (d < D) {
                const float l = lv[(long long)b * D + d];
                const float zz = mu[(long long)b * D + d] + expf(0.5f * l) * e[q];
                z[row * D + d] = zz;
                acc += 0.5f * (e[q] * e[q] - zz * zz + l);          // log N(z; 0, 1) - log N(z; mu, exp(l)), the 2 pi terms cancel
            }
        }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);    // within the 32-lane half
    if (live && j == 0) log_ratio[row] = acc;
}

__device__ __forceinline__ void lse_add(float& m, float& s1, float& s2, float v) {
    if (v > m) {
        const float c = expf(m - v);
        s1 = s1 * c + 1.f; s2 = s2 * c * c + 1.f; m = v;
    } else {
        const float e = expf(v - m);
        s1 += e; s2 += e * e;
    }
}
// (an empty state has m = -FLT_MAX and zero sums: merging it changes nothing)
__device__ __forceinline__ void lse_merge(float& m, float& s1, float& s2, float m2, float t1, float t2) {
    const float mm = fmaxf(m, m2), ca = expf(m - mm), cb = expf(m2 - mm);
    s1 = s1 * ca + t1 * cb; s2 = s2 * ca * ca + t2 * cb * cb; m = mm;
}

// one wave per example
__global__ __launch_bounds__(TPB) void iw_accumulate_kernel(const float* lx, const float* words, const long long* tgt, int T, int V,
                                                            const float* lr, int B, int K, float* state, float* log_w) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (b >= B) return;                                      // (uniform over the wave)
    float m[IW_TARGETS], s1[IW_TARGETS], s2[IW_TARGETS], sl[IW_TARGETS];
#pragma unroll
    for (int i = 0; i < IW_TARGETS; ++i) { m[i] = -FLT_MAX; s1[i] = s2[i] = sl[i] = 0.f; }
    for (int k = lane; k < K; k += 64) {
        const long long row = (long long)b * K + k;
        const float x = lx[row], r = lr[row];
        float y = 0.f;
        for (int t = 0; t < T; ++t) {                        // the target log-probabilities of the text decoder's greedy pass
            const long long c = min(max(tgt[(long long)b * T + t], 0ll), (long long)V - 1);
            y += words[(row * T + t) * V + c];
        }
        const float v[IW_TARGETS] = {x + r, y + r, x + y + r}, l[IW_TARGETS] = {x, y, x + y};
#pragma unroll
        for (int i = 0; i < IW_TARGETS; ++i) { lse_add(m[i], s1[i], s2[i], v[i]); sl[i] += l[i]; }
        if (log_w) {
#pragma unroll
            for (int i = 0; i < IW_TARGETS; ++i) log_w[row * IW_TARGETS + i] = v[i];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int i = 0; i < IW_TARGETS; ++i) {
            const float m2 = __shfl_xor(m[i], o, 64), t1 = __shfl_xor(s1[i], o, 64), t2 = __shfl_xor(s2[i], o, 64);
            lse_merge(m[i], s1[i], s2[i], m2, t1, t2);
            sl[i] += __shfl_xor(sl[i], o, 64);
        }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < IW_TARGETS; ++i) {
            float* st = state + ((long long)b * IW_TARGETS + i) * IW_STATE;
            float M = st[0], S1 = st[1], S2 = st[2];
            lse_merge(M, S1, S2, m[i], s1[i], s2[i]);
            st[0] = M; st[1] = S1; st[2] = S2; st[3] += sl[i];
        }
    }
}

__global__ __launch_bounds__(TPB) void iw_init_kernel(float* state, int B) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < B * IW_TARGETS * IW_STATE) state[i] = (i % IW_STATE) == 0 ? -FLT_MAX : 0.f;
}

__global__ __launch_bounds__(TPB) void iw_finalize_kernel(const float* state, int B, float K, float* out) {
    const int b = blockIdx.x * TPB + threadIdx.x;
    if (b >= B) return;
    const float* st = state + (long long)b * IW_TARGETS * IW_STATE;
    float* o = out + (long long)b * IW_OUT;
#pragma unroll
    for (int i = 0; i < IW_TARGETS; ++i) {
        const float m = st[i * IW_STATE], s1 = st[i * IW_STATE + 1], s2 = st[i * IW_STATE + 2];
        o[i] = m + (logf(s1) - logf(K));
        o[IW_TARGETS + i] = s1 * s1 / s2;
    }
    o[6] = -st[0 * IW_STATE + 3] / K;
    o[7] = -st[1 * IW_STATE + 3] / K;
}

}  // namespace

int launch_iw_particles(const float* mu, const float* logvar, int B, int D, int K, long long first_row, long long first_particle,
                        unsigned long long seed, const float* eps, float* z, float* log_ratio, hipStream_t s) {
    MMVAE_REQUIRE(mu && logvar && z && log_ratio, "iw_particles: null argument");
    MMVAE_REQUIRE(B >= 1 && K >= 1 && D >= 1 && D <= 128 && (long long)B * K * D < (1ll << 31),
                  "iw_particles: B=%d K=%d D=%d out of range (1 <= D <= 128, B*K*D < 2^31)", B, K, D);
    MMVAE_REQUIRE(first_row >= 0 && first_particle >= 0 && first_row + B <= (1ll << 32) && first_particle + K <= (1ll << 32),
                  "iw_particles: row / particle indices must stay below 2^32");
    const long long rows = (long long)B * K;
    hipLaunchKernelGGL(iw_particles_kernel, dim3((unsigned)((rows + TPB / 32 - 1) / (TPB / 32))), dim3(TPB), 0, s,
                       mu, logvar, B, D, K, first_row, first_particle, seed, eps, z, log_ratio);
    return mmvae_check_launch("iw_particles");
}

int launch_iw_init(float* state, int B, hipStream_t s) {
    MMVAE_REQUIRE(state && B >= 1, "iw_init: null state or B < 1");
    hipLaunchKernelGGL(iw_init_kernel, dim3(ceil_div(B * IW_TARGETS * IW_STATE, TPB)), dim3(TPB), 0, s, state, B);
    return mmvae_check_launch("iw_init");
}

int launch_iw_accumulate(const float* loglik_x, const float* words, const long long* targets, int T, int V, const float* log_ratio,
                         int B, int K, float* state, float* log_w, hipStream_t s) {
    MMVAE_REQUIRE(loglik_x && words && targets && log_ratio && state, "iw_accumulate: null argument");
    MMVAE_REQUIRE(B >= 1 && K >= 1 && T >= 1 && V >= 1 && (long long)B * K * T * V < (1ll << 40), "iw_accumulate: B=%d K=%d T=%d V=%d", B, K, T, V);
    hipLaunchKernelGGL(iw_accumulate_kernel, dim3(ceil_div(B, TPB / 64)), dim3(TPB), 0, s, loglik_x, words, targets, T, V, log_ratio,
                       B, K, state, log_w);
    return mmvae_check_launch("iw_accumulate");
}

int launch_iw_finalize(const float* state, int B, long long K_total, float* out, hipStream_t s) {
    MMVAE_REQUIRE(state && out && B >= 1 && K_total >= 1, "iw_finalize: null argument or empty");
    hipLaunchKernelGGL(iw_finalize_kernel, dim3(ceil_div(B, TPB)), dim3(TPB), 0, s, state, B, (float)K_total, out);
    return mmvae_check_launch("iw_finalize");
}
