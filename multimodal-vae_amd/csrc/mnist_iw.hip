// MNIST importance-weighted evaluation: ONE kernel decodes and scores a tile of particles (mnist.h: mnist_iw_score).
//
//   image decoder (eval): Linear(D,200) -> BN -> ReLU -> Linear(200,400) -> BN -> ReLU -> Linear(400,784)   mnist/model.py:121-133
//   text decoder  (eval): Linear(D,10)  -> BN -> ReLU -> Linear(10,10) -> log_softmax                       mnist/model.py:156-170
//   loglik_x[r] = sum over the 784 pixels of x*l - softplus(l) on the pre-sigmoid logit l (not clamped), words[r][0..9] = the log-softmax.
//
// A workgroup of 8 waves carries IW_R = 32 particle rows (two 16-row MFMA tiles) through the three layers.  The activations stay
// in LDS (z, 200-wide, 400-wide), the weights are the plan's bound fp32 parameters streamed from L2 straight into the B operand
// of v_mfma_f32_16x16x4_f32 (a weight row is contiguous along k: one 16-byte load per lane per 16-deep step), and a wave owns
// whole 16-column output tiles, so the 784 logits only ever exist as accumulator registers: the last layer's epilogue turns a
// tile into its 16 columns' share of the per-row sum.  BatchNorm is the affine map of the running statistics.
// Within a 16-deep step MFMA s of lane group q consumes k = k0 + 4q + s on both operands (as gemm_f32.hip).
#include "mnist_plan.h"

namespace {

constexpr int IW_R = 32, IW_WAVES = 8, IW_TPB = IW_WAVES * 64;
constexpr int H1 = 200, H2 = 400, NPIX = 784, NCLS = 10;
// LDS row strides in floats, all = 8 mod 16: the four 16-lane groups of a ds_read_b128 (16 rows x 4 consecutive floats,
// the lane group q at +4q) then cover 16 distinct 16-byte slots of the 256-byte bank row
constexpr int S1 = 216, S2 = 408;
constexpr int TS = 16;                                  // text hidden layer: [IW_R][TS]
__host__ __device__ constexpr int z_stride(int D) { return (D + 15) / 16 * 16 + 8; }

struct MnistIwArgs {
    const float* params; const float* bn_stats;
    const float* z; const float* image; float* loglik_x; float* words;
    long long rows; int B, K, D;
    long long w[3], b[3];                               // image_decoder.net.{0,3,6}
    long long tw[2], tb[2];                             // text_decoder.net.{0,3}
    long long bn_g[3], bn_b[3], bn_s[3];                // BatchNorm of image layer 1, image layer 2, text layer 1: gamma, beta, running stats
};

__device__ __forceinline__ float softplus_(float l) { return fmaxf(l, 0.f) + __logf(1.f + __expf(-fabsf(l))); }

// acc[t] (t = 0, 1: rows 16t .. 16t+15) += A[rows][0..K) W[n0 + lane%16][0..K)^T;  A: LDS image, stride S, zero beyond K up to
// the next multiple of 16; W: row-major [N][K] behind a buffer descriptor of exactly N*K floats (a column past N or a k past K
// reads 0 through the range check)
// KC: the compile-time K (0: K is the run-time `Kr`, the first layer's n_latents: 2.5 % of the work at D = 20, a plain loop).
// The weight fragments are fetched a group of G 16-deep steps ahead of the MFMAs that consume them (the loads of group g + 1 are
// in flight while group g multiplies): an L2 round trip is several steps long, and hipcc waits for each load where it is written.
template <int KC>
__device__ __forceinline__ void tile_gemm(const float* A, int S, const __amdgpu_buffer_rsrc_t wr, int N, int Kr, int n0, int fr, int fq,
                                          f32x4 (&acc)[2]) {
    const int K = KC > 0 ? KC : Kr;
    const int n = n0 + fr;
    const unsigned wrow = (unsigned)n * (unsigned)K * 4u;
    const bool nok = n < N;
    const float* a0 = A + fr * S + fq * 4;
    const float* a1 = a0 + 16 * S;
    auto wload = [&](int st) {
        const int kb = st * 16 + fq * 4;
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wr, (nok && kb < K) ? wrow + (unsigned)kb * 4u : 0xFFFFFFFFu, 0, 0));
    };
    auto step = [&](int st, const f32x4 bv) {
        const f32x4 av0 = *reinterpret_cast<const f32x4*>(a0 + st * 16);
        const f32x4 av1 = *reinterpret_cast<const f32x4*>(a1 + st * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av0[q], bv[q], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av1[q], bv[q], acc[1], 0, 0, 0);
        }
    };
    if constexpr (KC > 0) {
        constexpr int NST = (KC + 15) / 16, G = 5, NG = (NST + G - 1) / G;
        f32x4 cur[G], nxt[G];
#pragma unroll
        for (int u = 0; u < G; ++u) cur[u] = wload(u);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
#pragma unroll
            for (int u = 0; u < G; ++u)
                if ((g + 1) * G + u < NST) nxt[u] = wload((g + 1) * G + u);
            __builtin_amdgcn_sched_barrier(0);          // (the scheduler otherwise sinks each load to just above its first use)
#pragma unroll
            for (int u = 0; u < G; ++u)
                if (g * G + u < NST) step(g * G + u, cur[u]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < G; ++u) cur[u] = nxt[u];
        }
    } else {
        const int nst = (K + 15) >> 4;
        for (int st = 0; st < nst; ++st) step(st, wload(st));
    }
}

// Linear -> BatchNorm (running statistics) -> ReLU epilogue of one output tile into an LDS image (columns past N: 0)
__device__ __forceinline__ void bn_relu_store(const MnistIwArgs& a, const f32x4 (&acc)[2], long long b_off, int bi, int C, int n, int fq,
                                              float* out, int S) {
    float bias = 0.f, mean = 0.f, g = 0.f, beta = 0.f;
    if (n < C) {
        bias = a.params[b_off + n];
        mean = a.bn_stats[a.bn_s[bi] + n];
        g = a.params[a.bn_g[bi] + n] / sqrtf(a.bn_stats[a.bn_s[bi] + C + n] + BN_EPS);
        beta = a.params[a.bn_b[bi] + n];
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = (acc[t][r] + bias - mean) * g + beta;
            out[(t * 16 + fq * 4 + r) * S + n] = n < C ? fmaxf(v, 0.f) : 0.f;
        }
}

// TEXT = false (mnist_iw_score_image): the image decoder alone -- no 14th tile in layer 1, no text tail, `words` is not touched.  The image
// half runs the same instructions on the same operands either way: loglik_x is the same bits.
template <bool TEXT>
__global__ __launch_bounds__(IW_TPB) void mnist_iw_score_kernel(const MnistIwArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int D = a.D, ZS = z_stride(D);
    float* zs = lds;                                    // [IW_R][ZS]
    float* h1 = zs + IW_R * ZS;                         // [IW_R][S1]
    float* h2 = h1 + IW_R * S1;                         // [IW_R][S2]
    float* th = h2 + IW_R * S2;                         // [IW_R][TS]
    float* part = th + IW_R * TS;                       // [IW_WAVES][IW_R]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const long long row0 = (long long)blockIdx.x * IW_R;

    for (int i = tid; i < IW_R * ZS; i += IW_TPB) {
        const int m = i / ZS, d = i - m * ZS;
        zs[i] = (d < D && row0 + m < a.rows) ? a.z[(row0 + m) * D + d] : 0.f;
    }
    __syncthreads();

    // ---- layer 1: 13 image tiles (200 padded to 208) + the text decoder's first Linear as tile 13
    {
        const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.params + a.w[0]), 0, H1 * D * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t tr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.params + a.tw[0]), 0, NCLS * D * 4, 0x00020000);
        for (int nt = wave; nt < (TEXT ? 14 : 13); nt += IW_WAVES) {
            f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
            if (nt < 13) {
                tile_gemm<0>(zs, ZS, wr, H1, D, nt * 16, fr, fq, acc);
                bn_relu_store(a, acc, a.b[0], 0, H1, nt * 16 + fr, fq, h1, S1);
            } else {
                tile_gemm<0>(zs, ZS, tr, NCLS, D, 0, fr, fq, acc);
                bn_relu_store(a, acc, a.tb[0], 2, NCLS, fr, fq, th, TS);
            }
        }
    }
    __syncthreads();

    // ---- text tail (the last wave has the fewest tiles of layer 2): Linear(10,10) + log_softmax, one lane per row
    if (TEXT && wave == IW_WAVES - 1 && lane < IW_R && row0 + lane < a.rows) {
        const float* W = a.params + a.tw[1];
        const float* bb = a.params + a.tb[1];
        float lg[NCLS], mx = -3.0e38f;
#pragma unroll
        for (int j = 0; j < NCLS; ++j) {
            float s = bb[j];
#pragma unroll
            for (int i = 0; i < NCLS; ++i) s = fmaf(W[j * NCLS + i], th[lane * TS + i], s);
            lg[j] = s; mx = fmaxf(mx, s);
        }
        float se = 0.f;
#pragma unroll
        for (int j = 0; j < NCLS; ++j) se += expf(lg[j] - mx);
        const float lse = mx + logf(se);
        float* o = a.words + (row0 + lane) * NCLS;
#pragma unroll
        for (int j = 0; j < NCLS; ++j) o[j] = lg[j] - lse;
    }

    // ---- layer 2: 25 tiles
    {
        const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.params + a.w[1]), 0, H2 * H1 * 4, 0x00020000);
        for (int nt = wave; nt < H2 / 16; nt += IW_WAVES) {
            f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
            tile_gemm<H1>(h1, S1, wr, H2, H1, nt * 16, fr, fq, acc);
            bn_relu_store(a, acc, a.b[1], 1, H2, nt * 16 + fr, fq, h2, S2);
        }
    }
    __syncthreads();

    // ---- layer 3: 49 tiles, each reduced into the per-row sums.  Rows are example-major: a tile with K >= IW_R touches one or
    // two examples, whose pixels are then loaded once per example (two coalesced loads per tile), not once per row
    {
        const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.params + a.w[2]), 0, NPIX * H2 * 4, 0x00020000);
        const long long last = a.rows - 1;
        const int b_first = (int)(row0 / a.K);
        const int b_last = (int)((row0 + IW_R - 1 < last ? row0 + IW_R - 1 : last) / a.K);
        const bool two = b_last - b_first <= 1;                          // (uniform over the workgroup)
        int be[2][4];                                                    // example of this lane's 8 rows (rows past the end: the last row's)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long row = row0 + t * 16 + fq * 4 + r;
                be[t][r] = (int)((row < last ? row : last) / a.K);
            }
        float sum[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        for (int nt = wave; nt < NPIX / 16; nt += IW_WAVES) {
            f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
            const int n = nt * 16 + fr;
            const float bias = a.params[a.b[2] + n];
            float x0 = 0.f, x1 = 0.f;
            if (two) { x0 = a.image[(long long)b_first * NPIX + n]; x1 = a.image[(long long)b_last * NPIX + n]; }
            tile_gemm<H2>(h2, S2, wr, NPIX, H2, nt * 16, fr, fq, acc);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float l = acc[t][r] + bias;
                    const float x = two ? (be[t][r] == b_first ? x0 : x1) : a.image[(long long)be[t][r] * NPIX + n];
                    sum[t][r] += x * l - softplus_(l);
                }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = sum[t][r];
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);      // over the 16 columns of the lane group
                if (fr == 0) part[wave * IW_R + t * 16 + fq * 4 + r] = v;
            }
    }
    __syncthreads();
    if (tid < IW_R && row0 + tid < a.rows) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < IW_WAVES; ++w) v += part[w * IW_R + tid];          // fixed order: the result does not depend on scheduling
        a.loglik_x[row0 + tid] = v;
    }
}

size_t iw_lds_bytes(int D) { return sizeof(float) * (size_t)(IW_R * (z_stride(D) + S1 + S2 + TS) + IW_WAVES * IW_R); }

}  // namespace

static int iw_score(MnistPlan* Pp, const float* z, const float* image, int B, int K, float* loglik_x, float* words, bool text, hipStream_t s) {
    MMVAE_TRY(check_bound(Pp));
    MnistPlan& P = *Pp;
    MMVAE_REQUIRE(z && image && loglik_x && (words || !text), "mnist_iw_score: null argument");
    const long long rows = (long long)B * K;
    // row, pixel and tile indices are 32-bit in the kernel (rows + IW_R and B * 784 must fit)
    MMVAE_REQUIRE(B >= 1 && K >= 1 && rows <= 0x7FFFFFFFll - IW_R && (long long)B * NPIX <= 0x7FFFFFFFll,
                  "mnist_iw_score: B=%d K=%d out of range (B*K and B*784 must stay below 2^31)", B, K);
    MnistIwArgs a{};
    a.params = P.buf.params; a.bn_stats = P.buf.bn_stats;
    a.z = z; a.image = image; a.loglik_x = loglik_x; a.words = words;
    a.rows = rows; a.B = B; a.K = K; a.D = P.D;
    for (int i = 0; i < 3; ++i) { a.w[i] = P.id[i].w_off; a.b[i] = P.id[i].b_off; }
    for (int i = 0; i < 2; ++i) { a.tw[i] = P.td[i].w_off; a.tb[i] = P.td[i].b_off; }
    const int bi[3] = {2, 3, 5};
    for (int i = 0; i < 3; ++i) { a.bn_g[i] = P.bn[bi[i]].w_off; a.bn_b[i] = P.bn[bi[i]].b_off; a.bn_s[i] = P.bn[bi[i]].stat_off; }
    // the 16-byte weight loads: every matrix streamed through the MFMA starts 16-byte aligned and has rows of a multiple of 4 floats
    MMVAE_REQUIRE((reinterpret_cast<uintptr_t>(a.params) & 15) == 0 && a.w[0] % 4 == 0 && a.w[1] % 4 == 0 && a.w[2] % 4 == 0 &&
                  a.tw[0] % 4 == 0 && P.D % 4 == 0, "mnist_iw_score: parameter buffer is not 16-byte aligned");
    const size_t lds = iw_lds_bytes(P.D);
    static std::atomic<unsigned> attr_set{0}, attr_set_image{0};
    if (text) {
        if (mmvae_first_use_on_device(attr_set))
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mnist_iw_score_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)iw_lds_bytes(124));
        MMVAE_LAUNCH(mnist_iw_score_kernel<true>, dim3((unsigned)((rows + IW_R - 1) / IW_R)), dim3(IW_TPB), lds, s, a);
        return mmvae_check_launch("mnist_iw_score");
    }
    if (mmvae_first_use_on_device(attr_set_image))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mnist_iw_score_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)iw_lds_bytes(124));
    MMVAE_LAUNCH(mnist_iw_score_kernel<false>, dim3((unsigned)((rows + IW_R - 1) / IW_R)), dim3(IW_TPB), lds, s, a);
    return mmvae_check_launch("mnist_iw_score_image");
}
int mnist_iw_score(MnistPlan* P, const float* z, const float* image, int B, int K, float* loglik_x, float* words, hipStream_t s) {
    return iw_score(P, z, image, B, K, loglik_x, words, true, s);
}
int mnist_iw_score_image(MnistPlan* P, const float* z, const float* image, int B, int K, float* loglik_x, hipStream_t s) {
    return iw_score(P, z, image, B, K, loglik_x, nullptr, false, s);
}
