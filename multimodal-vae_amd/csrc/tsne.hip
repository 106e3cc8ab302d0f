// See tsne.h.
#include "tsne.h"
#include <math.h>
#include <algorithm>

namespace {

constexpr int RT = TSNE_RT, CT = TSNE_CT, ST = TSNE_ST, AT = TSNE_AT, NTHR = 256, SUB = 8, WCOLS = CT / 4, DCH = 16;
static_assert(NTHR == 4 * RT && AT == NTHR, "lane = row, 4 waves");
static_assert(2 * CT == NTHR, "one float of a column tile of y per thread");
static_assert(WCOLS % SUB == 0, "a wave's columns of a tile are whole groups of 8");
static_assert(NTHR == 8 * ST, "8 rows of a symmetrisation tile per pass");

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// v[0..K) summed over the workgroup in a fixed order (butterfly per wave, then the 4 waves ascending), the result in every thread
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double (*red)[4]) {
#pragma unroll
    for (int c = 0; c < K; ++c) v[c] = wave_sum_d(v[c]);
    __syncthreads();                                              // the previous call's readers are done with red
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) red[c][threadIdx.x >> 6] = v[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < K; ++c) v[c] = ((red[c][0] + red[c][1]) + red[c][2]) + red[c][3];
}

// ---------------------------------------------------------------------------------------------- conditional affinities
// One workgroup per row i.  The row of P holds d_ij while beta_i is searched and p_{j|i} afterwards; thread t reads back only the
// columns it wrote itself.
__global__ __launch_bounds__(AT) void tsne_cond_kernel(const float* __restrict__ x, int n, int dim, double log_perp, float* __restrict__ P,
                                                       float* __restrict__ beta_out) {
    __shared__ float xi[TSNE_MAX_DIM + DCH];
    __shared__ double red[2][4];
    __shared__ float mins[4];
    const int tid = threadIdx.x, i = blockIdx.x;
    float* row = P + (size_t)i * n;
    for (int k = tid; k < dim; k += AT) xi[k] = x[(size_t)i * dim + k];
    __syncthreads();
    float dmin = INFINITY;
    for (int j = tid; j < n; j += AT) {
        const float* xj = x + (size_t)j * dim;
        float c[DCH];                                             // coordinate k goes to chain k % DCH, ascending
#pragma unroll
        for (int u = 0; u < DCH; ++u) c[u] = 0.f;
        for (int k0 = 0; k0 < dim; k0 += DCH) {
#pragma unroll
            for (int u = 0; u < DCH; ++u) {
                const float d = k0 + u < dim ? xi[k0 + u] - xj[k0 + u] : 0.f;
                c[u] = fmaf(d, d, c[u]);
            }
        }
#pragma unroll
        for (int o = 1; o < DCH; o <<= 1) {                       // a fixed tree: (c0 + c1) + (c2 + c3), ...
#pragma unroll
            for (int u = 0; u < DCH; u += 2 * o) c[u] += c[u + o];
        }
        const float acc = c[0];
        row[j] = acc;
        if (j != i) dmin = fminf(dmin, acc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dmin = fminf(dmin, __shfl_xor(dmin, o, 64));
    if ((tid & 63) == 0) mins[tid >> 6] = dmin;
    __syncthreads();
    dmin = fminf(fminf(mins[0], mins[1]), fminf(mins[2], mins[3]));   // n >= 3: some j != i exists, the minimum is finite

    // sklearn's _binary_search_perplexity on d - dmin: the nearest neighbour's term is exp(0), the sum is never below 1
    float beta = 1.f, bmin = -INFINITY, bmax = INFINITY, beta_used = 1.f;
    double sum_p = 1.0;
    for (int step = 0; step < TSNE_SEARCH_STEPS; ++step) {
        double a[2] = {0.0, 0.0};
        for (int j = tid; j < n; j += AT) {
            if (j == i) continue;
            const float d = row[j] - dmin;
            const float p = expf(-beta * d);
            a[0] += (double)p;
            a[1] += (double)(d * p);
        }
        block_sum<2>(a, red);                                     // the same bits in every thread: the branches below are uniform
        sum_p = a[0];
        beta_used = beta;
        const double diff = (log(a[0]) + (double)beta * a[1] / a[0]) - log_perp;
        if (fabs(diff) <= 1e-5) break;
        if (diff > 0.0) {
            bmin = beta;
            beta = bmax == INFINITY ? beta * 2.f : (beta + bmax) * 0.5f;
        } else {
            bmax = beta;
            beta = bmin == -INFINITY ? beta * 0.5f : (beta + bmin) * 0.5f;
        }
    }
    for (int j = tid; j < n; j += AT) row[j] = j == i ? 0.f : (float)((double)expf(-beta_used * (row[j] - dmin)) / sum_p);
    if (tid == 0) beta_out[i] = beta_used;
}

// ---------------------------------------------------------------------------------------------- symmetrisation
// grid (column tile b, row tile a); the workgroups with a > b only write their (zero) partial sums
__global__ __launch_bounds__(NTHR) void tsne_sym_kernel(float* __restrict__ P, int n, double* __restrict__ part) {
    __shared__ float A[ST][ST + 1], B[ST][ST + 1];
    __shared__ double red[2][4];
    const int a = blockIdx.y, b = blockIdx.x;
    const int tid = threadIdx.x, tx = tid & (ST - 1), ty = tid / ST;
    double acc[2] = {0.0, 0.0};                                   // sum P log P, sum P
    if (a <= b) {
        const int a0 = a * ST, b0 = b * ST;
        for (int r = ty; r < ST; r += NTHR / ST) {
            A[r][tx] = (a0 + r < n && b0 + tx < n) ? P[(size_t)(a0 + r) * n + b0 + tx] : 0.f;
            B[r][tx] = (b0 + r < n && a0 + tx < n) ? P[(size_t)(b0 + r) * n + a0 + tx] : 0.f;
        }
        __syncthreads();
        const float den = 2.f * (float)n;
        for (int r = ty; r < ST; r += NTHR / ST) {
            int i = a0 + r, j = b0 + tx;
            if (i < n && j < n) {
                const float v = i == j ? 0.f : fmaxf((A[r][tx] + B[tx][r]) / den, 1e-12f);
                P[(size_t)i * n + j] = v;
                if (v > 0.f) { acc[0] += (double)v * log((double)v); acc[1] += (double)v; }
            }
            i = b0 + r; j = a0 + tx;
            if (a != b && i < n && j < n) {
                const float v = fmaxf((B[r][tx] + A[tx][r]) / den, 1e-12f);
                P[(size_t)i * n + j] = v;
                acc[0] += (double)v * log((double)v); acc[1] += (double)v;
            }
        }
    }
    block_sum<2>(acc, red);
    if (tid == 0) {
        const size_t k = (size_t)a * gridDim.x + b;
        part[2 * k] = acc[0]; part[2 * k + 1] = acc[1];
    }
}

__global__ __launch_bounds__(NTHR) void tsne_stats_kernel(const double* __restrict__ part, long long count, float* __restrict__ out2) {
    __shared__ double red[2][4];
    double acc[2] = {0.0, 0.0};
    for (long long k = threadIdx.x; k < count; k += NTHR) { acc[0] += part[2 * k]; acc[1] += part[2 * k + 1]; }
    block_sum<2>(acc, red);
    if (threadIdx.x == 0) { out2[0] = (float)acc[0]; out2[1] = (float)acc[1]; }
}

// ---------------------------------------------------------------------------------------------- the sweep
// log q for a float64 q >= 1 to about 2e-13: q = 2^e m, m in [1, 2), m = c (1 + r) with c the centre of m's bin of 1 / 128;
// tab[bin] = {log c, 1 / c}, log(1 + r) = r - r^2 / 2 + r^3 / 3 - r^4 / 4 (|r| < 2^-8).  logf is not enough here: its error has
// a bias of a third of an ulp, which the sum over the pairs does not average away (3e-7 of KL measured).
__device__ __forceinline__ double log_q(double q, const double2* __restrict__ tab) {
    const long long b = __double_as_longlong(q);
    const int e = (int)((b >> 52) & 0x7ff) - 1023;
    const double2 t = tab[(int)((b >> 45) & 127)];
    const double m = __longlong_as_double((b & 0x000fffffffffffffLL) | 0x3ff0000000000000LL);
    const double r = fma(m, t.y, -1.0);
    double s = fma(r, -0.25, 1.0 / 3.0);
    s = fma(s, r, -0.5);
    s = fma(s, r, 1.0);
    return fma((double)e, 0.69314718055994530942, t.x) + r * s;
}

// sums per thread: P w dy (2) and w^2 dy (2) from fp32 terms; w (j != i), P log(1 + |dy|^2) = -P log w and P log P from float64
// terms (1 + |dy|^2 is exact in float64; w there is the fp32 reciprocal after one Newton step)
template <bool PLOGP>
__global__ __launch_bounds__(NTHR) void tsne_pairs_kernel(const float* __restrict__ P, const float* __restrict__ Y, int n, int T,
                                                          long long rpad, double* __restrict__ Gp, double* __restrict__ Wp) {
    __shared__ __attribute__((aligned(16))) float ys[2][CT][2];
    __shared__ double2 ltab[128];
    __shared__ double red[7][NTHR];
    const int tid = threadIdx.x, il = tid & 63, w = tid >> 6;
    const int rt = blockIdx.x, sp = blockIdx.y, S = gridDim.y;
    const int t0 = (int)((long long)T * sp / S), t1 = (int)((long long)T * (sp + 1) / S);
    const int row = rt * RT + il;
    const bool rok = row < n;                                     // rows past the end compute a copy of the last row, unwritten
    const int rr = rok ? row : n - 1;
    const float yi0 = Y[2 * (size_t)rr], yi1 = Y[2 * (size_t)rr + 1];
    const float* Pc = P + rr;                                     // P_ji for P_ij: 64 consecutive floats per wave and column
    double acc[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) acc[c] = 0.0;
    if (tid < 128) {
        const double c = 1.0 + ((double)tid + 0.5) / 128.0;
        ltab[tid] = make_double2(log(c), 1.0 / c);
    }

    auto stage = [&](int t, int buf) {                            // columns past n are staged as zeros and never counted
        const int j = t * CT + (tid >> 1);
        ys[buf][tid >> 1][tid & 1] = j < n ? Y[2 * (size_t)j + (tid & 1)] : 0.f;
    };
    stage(t0, 0);
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
        const int cur = (t - t0) & 1;
        if (t + 1 < t1) stage(t + 1, cur ^ 1);
        const int jbeg = t * CT + w * WCOLS;
        for (int jb = jbeg; jb < jbeg + WCOLS && jb < n; jb += SUB) {
            float p[SUB];
#pragma unroll
            for (int u = 0; u < SUB; ++u) p[u] = jb + u < n ? Pc[(size_t)(jb + u) * n] : 0.f;
            float f[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < SUB; ++u) {
                const int j = jb + u;
                const float d0 = yi0 - ys[cur][j - t * CT][0], d1 = yi1 - ys[cur][j - t * CT][1];
                const double qd = fma((double)d0, (double)d0, fma((double)d1, (double)d1, 1.0));
                const float wv = j < n ? 1.f / (float)qd : 0.f;
                const float pw = p[u] * wv, w2 = wv * wv;
                f[0] = fmaf(pw, d0, f[0]); f[1] = fmaf(pw, d1, f[1]);
                f[2] = fmaf(w2, d0, f[2]); f[3] = fmaf(w2, d1, f[3]);
                const double w0 = (double)wv;
                acc[4] += j == row ? 0.0 : fma(w0, fma(-qd, w0, 1.0), w0);
                acc[5] = fma((double)p[u], log_q(qd, ltab), acc[5]);
                if (PLOGP) acc[6] += p[u] > 0.f ? (double)p[u] * log((double)p[u]) : 0.0;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] += (double)f[c];
        }
        __syncthreads();
    }

#pragma unroll
    for (int c = 0; c < 7; ++c) red[c][tid] = rok ? acc[c] : 0.0;
    __syncthreads();
    if (tid < RT) {                                               // wave 0, lane = row: the 4 waves in ascending order
        double v[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) v[c] = ((red[c][il] + red[c][RT + il]) + red[c][2 * RT + il]) + red[c][3 * RT + il];
        if (rok) {
            const size_t slot = (size_t)sp * (size_t)rpad + (size_t)row;       // < S * rpad
#pragma unroll
            for (int c = 0; c < 4; ++c) Gp[4 * slot + c] = v[c];
        }
        const double sw = wave_sum_d(v[4]), sl = wave_sum_d(v[5]), sq = wave_sum_d(v[6]);
        if (il == 0) {
            const size_t k = (size_t)sp * gridDim.x + rt;                      // < S * row tiles
            Wp[3 * k] = sw; Wp[3 * k + 1] = sl; Wp[3 * k + 2] = sq;
        }
    }
}

// ---------------------------------------------------------------------------------------------- the fold and the update
// Every workgroup adds the sweep's workgroup partials in the same order (Z has the same bits everywhere), then one thread per row
// adds the row's splits in ascending order.  keep[0] carries sum P log P from the call's first iteration to the later ones.
template <bool UPDATE>
__global__ __launch_bounds__(NTHR) void tsne_fold_kernel(const double* __restrict__ Gp, const double* __restrict__ Wp, int n, int S, int RTn,
                                                         long long rpad, float exaggeration, bool fresh_plogp, double* __restrict__ keep,
                                                         float* __restrict__ y, float* __restrict__ update, float* __restrict__ gains,
                                                         float momentum, float lr, float* __restrict__ grad, float* __restrict__ out) {
    __shared__ double red[3][4];
    const int tid = threadIdx.x;
    double a[3] = {0.0, 0.0, 0.0};
    for (int k = tid; k < S * RTn; k += NTHR) { a[0] += Wp[3 * (size_t)k]; a[1] += Wp[3 * (size_t)k + 1]; a[2] += Wp[3 * (size_t)k + 2]; }
    block_sum<3>(a, red);
    const double Z = a[0];
    if (blockIdx.x == 0 && tid == 0) {
        const double plogp = fresh_plogp ? a[2] : keep[0];
        if (fresh_plogp) keep[0] = a[2];
        const double kl = plogp + a[1] + log(Z);
        out[0] = (float)kl;
        if (!UPDATE) { out[1] = (float)Z; out[2] = (float)plogp; }
    }
    const int row = blockIdx.x * NTHR + tid;
    if (row >= n) return;
    double g[4] = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < S; ++s) {
        const size_t slot = (size_t)s * (size_t)rpad + (size_t)row;
#pragma unroll
        for (int c = 0; c < 4; ++c) g[c] += Gp[4 * slot + c];
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float gr = (float)(4.0 * ((double)exaggeration * g[c] - g[2 + c] / Z));
        const size_t e = 2 * (size_t)row + c;
        if (UPDATE) {                                             // sklearn's _gradient_descent: min_gain 0.01
            float u = update[e], gn = gains[e];
            gn = u * gr < 0.f ? gn + 0.2f : gn * 0.8f;
            gn = fmaxf(gn, 0.01f);
            u = momentum * u - lr * (gn * gr);
            gains[e] = gn; update[e] = u; y[e] += u;
        } else {
            grad[e] = gr;
        }
    }
}

struct Ws {
    double *Gp, *Wp, *keep;
};
Ws carve(void* ws, const TsneShape& g) {
    Ws o;
    o.Gp = reinterpret_cast<double*>(ws);
    o.Wp = o.Gp + (size_t)g.s * (size_t)g.rpad * 4;
    o.keep = o.Wp + (size_t)g.s * (size_t)g.rt * 3;
    return o;
}

int sweep(const float* P, const float* y, int n, const TsneShape& g, const Ws& o, bool plogp, hipStream_t s) {
    if (plogp) MMVAE_LAUNCH((tsne_pairs_kernel<true>), dim3(g.rt, g.s), dim3(NTHR), 0, s, P, y, n, g.ct, g.rpad, o.Gp, o.Wp);
    else MMVAE_LAUNCH((tsne_pairs_kernel<false>), dim3(g.rt, g.s), dim3(NTHR), 0, s, P, y, n, g.ct, g.rpad, o.Gp, o.Wp);
    return mmvae_check_launch("tsne_pairs");
}

}  // namespace

TsneShape tsne_shape(int n) {
    TsneShape g;
    g.rt = ceil_div(n, RT); g.ct = ceil_div(n, CT); g.st = ceil_div(n, ST);
    g.s = std::max(1, std::min(std::min(g.ct, (int)TSNE_MAX_SPLITS), (int)TSNE_GRID_TARGET / g.rt));
    g.rpad = (long long)g.rt * RT;
    return g;
}

size_t tsne_workspace_bytes(int n) {
    const TsneShape g = tsne_shape(n);
    const size_t sweep_d = (size_t)g.s * (size_t)g.rpad * 4 + (size_t)g.s * (size_t)g.rt * 3 + 4;
    const size_t sym_d = (size_t)g.st * (size_t)g.st * 2;
    return std::max(sweep_d, sym_d) * sizeof(double);
}

int launch_tsne_affinities(const float* x, int n, int dim, float perplexity, float* P, float* beta, float* out2, void* ws, hipStream_t s) {
    MMVAE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "tsne: the workspace must be 8-byte aligned");
    const TsneShape g = tsne_shape(n);
    double* part = reinterpret_cast<double*>(ws);
    MMVAE_LAUNCH(tsne_cond_kernel, dim3(n), dim3(AT), 0, s, x, n, dim, log((double)perplexity), P, beta);
    MMVAE_TRY(mmvae_check_launch("tsne_cond"));
    MMVAE_LAUNCH(tsne_sym_kernel, dim3(g.st, g.st), dim3(NTHR), 0, s, P, n, part);
    MMVAE_TRY(mmvae_check_launch("tsne_sym"));
    MMVAE_LAUNCH(tsne_stats_kernel, dim3(1), dim3(NTHR), 0, s, (const double*)part, (long long)g.st * g.st, out2);
    return mmvae_check_launch("tsne_stats");
}

int launch_tsne_grad(const float* P, float exaggeration, const float* y, int n, void* ws, float* grad, float* out3, hipStream_t s) {
    MMVAE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "tsne: the workspace must be 8-byte aligned");
    const TsneShape g = tsne_shape(n);
    const Ws o = carve(ws, g);
    MMVAE_TRY(sweep(P, y, n, g, o, true, s));
    MMVAE_LAUNCH((tsne_fold_kernel<false>), dim3(ceil_div(n, NTHR)), dim3(NTHR), 0, s, (const double*)o.Gp, (const double*)o.Wp, n, g.s, g.rt,
                 g.rpad, exaggeration, true, o.keep, (float*)nullptr, (float*)nullptr, (float*)nullptr, 0.f, 0.f, grad, out3);
    return mmvae_check_launch("tsne_fold");
}

int launch_tsne_run(const float* P, int n, float* y, float* update, float* gains, int first_iter, int n_iter, float learning_rate,
                    float early_exaggeration, int exaggeration_iters, float* kl_trace, void* ws, hipStream_t s) {
    MMVAE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "tsne: the workspace must be 8-byte aligned");
    const TsneShape g = tsne_shape(n);
    const Ws o = carve(ws, g);
    for (int k = 0; k < n_iter; ++k) {
        const bool early = (long long)first_iter + k < exaggeration_iters;
        MMVAE_TRY(sweep(P, y, n, g, o, k == 0, s));
        MMVAE_LAUNCH((tsne_fold_kernel<true>), dim3(ceil_div(n, NTHR)), dim3(NTHR), 0, s, (const double*)o.Gp, (const double*)o.Wp, n, g.s,
                     g.rt, g.rpad, early ? early_exaggeration : 1.f, k == 0, o.keep, y, update, gains, early ? 0.5f : 0.8f, learning_rate,
                     (float*)nullptr, kl_trace + k);
        MMVAE_TRY(mmvae_check_launch("tsne_fold"));
    }
    return MMVAE_OK;
}
