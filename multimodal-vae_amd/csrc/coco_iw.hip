// COCO importance-weighted evaluation: the two scoring kernels behind mmvae_coco_iw_score (coco.h).
//
// (a) coco_iw_tail_kernel: the forward-only tail of the image decoder (coco/model.py:205-216).  Per particle row
//       raw bf16 NHWC [16][16][64] (hallucinate.6) -> BatchNorm affine + activation -> ConvTranspose2d(64, 3, 4, 2, 1) -> 3x32x32
//       logits l -> loglik[row] = sum of x*l - softplus(l) against the image of example row / K (softplus not clamped).
//     The matrix-core formulation is the one of celeba_iw_tail_kernel (celeba_iw.hip) at another geometry: P[pixel][j = tap*3 + co]
//     = A[pixel][64 ch] . W[64 ch][j] (48 of 64 columns used), then every logit is the overlap-add of 4 entries of P out of LDS.
//     The image is small enough that the strip / ring schedule of the CelebA kernel is not needed:
//       * a wave owns 32 pixels (two 16-pixel input rows) and reads its MFMA A operand straight from the raw tensor: lane
//         (pixel r, half h) loads the 8 channels 16 ks + 8 h .. of its pixel as one 16-byte vector per k-step, applies the affine
//         and the activation in registers and rounds to bf16 -- every activated value is made exactly once and never staged in LDS;
//       * P of the WHOLE image (256 pixels x 49 floats, 50 KB) sits in LDS, so a row costs two barriers; two workgroups are
//         resident on a CU (126 VGPRs x 8 waves; the LDS alone would take three);
//       * a workgroup walks rows blockIdx.x, + gridDim.x, ...: the raw vectors of its next row are fetched into registers while
//         the current row is computed.
//     The sum has a fixed order (thread in fp32 -> wave shuffle tree and the 8 wave partials in double): no float atomics,
//     equal inputs give bit-equal outputs whatever the grid.  Nothing but loglik (and the tests' optional logits dump) is written.
// (b) coco_iw_text_sse_kernel: sse[row] = sum over (t, e) of (sentence[row][t][e] - text[row / K][t][e])^2, one workgroup per
//     row: differences and a thread's partial sum in fp32 (16-byte vectors, elements i = 4 (tid + 256 n) ..), then the same
//     double-precision fold.  A row's result depends on nothing but that row.
#include "coco.h"
#include "convres_epi.h"

namespace {

constexpr int T_IH = 16, T_IW = 16, T_OH = 32, T_OW = 32, T_C = 64, T_CO = 3, T_J = 48, T_NPIX = T_IH * T_IW;
constexpr int T_KS = T_C / 16;         // k-steps of the 32x32x16 MFMA
constexpr int T_PF = 49;               // P: floats per pixel (48 + 1: the overlap-add reads a column across pixels)
constexpr int T_WAVES = 8, T_NTHR = T_WAVES * 64;
constexpr int T_NOUT = T_CO * T_OH * T_OW;
static_assert(T_WAVES * 32 == T_NPIX, "32 pixels of the image per wave");
static_assert(T_NOUT % T_NTHR == 0, "every thread sums the same number of logits");
static_assert((T_NPIX * T_PF + 2 * T_C) * 4 + T_WAVES * 8 <= 64 * 1024, "static LDS budget");

__device__ __forceinline__ float tail_act(int act, float v) {
    if (act == ACT_SWISH) return swish_fast(v);
    if (act == ACT_RELU) return fmaxf(v, 0.f);
    return v;
}

__global__ __launch_bounds__(T_NTHR) void coco_iw_tail_kernel(const IwTailArgs a) {
    __shared__ float P_s[T_NPIX * T_PF];
    __shared__ float2 aff_s[T_C];
    __shared__ double part[T_WAVES];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;

    if (tid < T_C) {
        float2 aff;
        if (a.affine) {
            aff = a.affine[tid];
        } else {                                             // eval-mode BatchNorm: as bn_channel_tables (bn_dev.h)
            const float sc = a.gamma[tid] * rsqrtf(a.rvar[tid] + a.eps);
            aff = make_float2(sc, a.beta[tid] - a.rmean[tid] * sc);
        }
        aff_s[tid] = aff;
    }
    // weight fragments, fp32 (64, 3, 4, 4) -> bf16, column j = tap*3 + co: B[k = ch][j] for the four k-steps and the two column tiles
    bf16x8 wf[T_KS][2];
#pragma unroll
    for (int ks = 0; ks < T_KS; ++ks)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int j = nt * 32 + r, tap = j / T_CO, co = j - tap * T_CO;
#pragma unroll
            for (int e = 0; e < 8; ++e) wf[ks][nt][e] = j < T_J ? (bf16)a.w[((ks * 16 + 8 * h + e) * T_CO + co) * 16 + tap] : (bf16)0.f;
        }
    // the lane's A operand of k-step ks: pixel 32 wave + r, channels 16 ks + 8 h .. + 7
    i32x4c rv[T_KS];
    auto fetch = [&](int row) {
        const bf16* src = a.q3 + ((size_t)row * T_NPIX + wave * 32 + r) * T_C + 8 * h;
#pragma unroll
        for (int ks = 0; ks < T_KS; ++ks) rv[ks] = *reinterpret_cast<const i32x4c*>(src + ks * 16);
    };
    int row = blockIdx.x;
    if (row < a.rows) fetch(row);
    __syncthreads();

    for (; row < a.rows; row += gridDim.x) {
        // ---- affine + activation in registers -> bf16 A fragments
        bf16x8 af[T_KS];
#pragma unroll
        for (int ks = 0; ks < T_KS; ++ks) {
            const bf16x8 x = __builtin_bit_cast(bf16x8, rv[ks]);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float2 t = aff_s[ks * 16 + 8 * h + e];
                af[ks][e] = (bf16)tail_act(a.act, (float)x[e] * t.x + t.y);
            }
        }
        if (row + (int)gridDim.x < a.rows) fetch(row + (int)gridDim.x);      // in flight through the rest of this row
        // ---- P[pixel][j] of the wave's 32 pixels (every reader of the previous row's P passed the barrier behind its sum)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
            for (int ks = 0; ks < T_KS; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ks], wf[ks][nt], acc, 0, 0, 0);
            const int j = nt * 32 + r;
            if (j < T_J) {                                   // lane = column j, register e = pixel (e&3) + 8*(e>>2) + 4h of the wave's 32
#pragma unroll
                for (int e = 0; e < 16; ++e) P_s[(wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * h) * T_PF + j] = acc[e];
            }
        }
        __syncthreads();
        // ---- the 3x32x32 logits by overlap-add, and their terms of the sum
        const float* const timg = a.image + (size_t)(row / a.K) * T_NOUT;
        float* const lg = a.logits ? a.logits + (size_t)row * T_NOUT : nullptr;
        float ll = 0.f;
#pragma unroll
        for (int it = 0; it < T_NOUT / T_NTHR; ++it) {
            const int o = tid + it * T_NTHR;                 // NCHW index (co, oy, ox)
            const int ox = o & (T_OW - 1), oy = (o >> 5) & (T_OH - 1), co = o >> 10;
            const int kh0 = (oy + 1) & 1, kw0 = (ox + 1) & 1;
            const int iy0 = (oy + 1 - kh0) >> 1, ix0 = (ox + 1 - kw0) >> 1;
            float acc = 0.f;
#pragma unroll
            for (int ty = 0; ty < 2; ++ty)
#pragma unroll
                for (int tx = 0; tx < 2; ++tx) {
                    // a row / column outside the image is masked, not branched on (the clamped pixel is one of the image)
                    const int iy = iy0 - ty, ix = ix0 - tx;
                    const int iyc = min(max(iy, 0), T_IH - 1), ixc = min(max(ix, 0), T_IW - 1);
                    const float pv = P_s[(iyc * T_IW + ixc) * T_PF + ((kh0 + 2 * ty) * 4 + kw0 + 2 * tx) * T_CO + co];
                    acc += (iy == iyc && ix == ixc) ? pv : 0.f;
                }
            if (lg) lg[o] = acc;
            ll += timg[o] * acc - (fmaxf(acc, 0.f) + log1pf(expf(-fabsf(acc))));
        }
        // a thread's 6 terms in fp32, the 512 thread sums in double (once per row): the sum of 3072 terms of one sign is rounded to
        // fp32 once
        double dl = (double)ll;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dl += __shfl_xor(dl, o, 64);
        if (lane == 0) part[wave] = dl;
        __syncthreads();                                     // also: the next row overwrites the P read above
        if (tid == 0) {
            double s = 0.0;
            for (int w = 0; w < T_WAVES; ++w) s += part[w];
            a.loglik[row] = (float)s;
        }
        // (part is rewritten only behind the next row's P barrier, which thread 0 reaches after this read)
    }
}

// ---------------------------------------------------------------------------------------------------------------------
constexpr int S_WAVES = 4, S_NTHR = S_WAVES * 64;

__global__ __launch_bounds__(S_NTHR) void coco_iw_text_sse_kernel(const float* __restrict__ sentence, const float* __restrict__ text, int K,
                                                                  long long n4, float* __restrict__ sse) {
    __shared__ double part[S_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row = blockIdx.x;
    const float4* const y = reinterpret_cast<const float4*>(sentence) + row * n4;
    const float4* const t = reinterpret_cast<const float4*>(text) + (row / K) * n4;
    float acc = 0.f;
    for (long long i = tid; i < n4; i += S_NTHR) {
        const float4 u = y[i], v = t[i];
        const float d0 = u.x - v.x, d1 = u.y - v.y, d2 = u.z - v.z, d3 = u.w - v.w;
        acc = fmaf(d0, d0, acc); acc = fmaf(d1, d1, acc); acc = fmaf(d2, d2, acc); acc = fmaf(d3, d3, acc);
    }
    double ds = (double)acc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ds += __shfl_xor(ds, o, 64);
    if (lane == 0) part[wave] = ds;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < S_WAVES; ++w) s += part[w];
        sse[row] = (float)s;
    }
}

}  // namespace

int launch_coco_iw_tail(const IwTailArgs& a, hipStream_t s) {
    MMVAE_REQUIRE(a.q3 && a.w && a.image && a.loglik, "coco_iw_tail: null argument");
    MMVAE_REQUIRE(a.affine || (a.gamma && a.beta && a.rmean && a.rvar), "coco_iw_tail: neither an affine table nor BatchNorm buffers");
    MMVAE_REQUIRE(a.act == ACT_NONE || a.act == ACT_SWISH || a.act == ACT_RELU, "coco_iw_tail: unknown activation %d", a.act);
    // (row indices are 32-bit in the kernel; the byte offsets are 64-bit)
    MMVAE_REQUIRE(a.rows >= 1 && a.K >= 1 && a.rows % a.K == 0 && a.rows <= 0x3FFFFFFF, "coco_iw_tail: rows=%d K=%d", a.rows, a.K);
    MMVAE_REQUIRE((reinterpret_cast<uintptr_t>(a.q3) & 15) == 0, "coco_iw_tail: the raw tensor is not 16-byte aligned");
    const int cap = 2 * mmvae_cu_count();                    // two resident workgroups per CU (registers); more rows: each walks several
    const int grid = a.rows < cap ? a.rows : cap;
    MMVAE_LAUNCH(coco_iw_tail_kernel, dim3(grid), dim3(T_NTHR), 0, s, a);
    return mmvae_check_launch("coco_iw_tail");
}

int launch_coco_iw_text_sse(const float* sentence, const float* text, int B, int K, int steps, float* sse, hipStream_t s) {
    MMVAE_REQUIRE(sentence && text && sse, "coco_iw_text_sse: null argument");
    MMVAE_REQUIRE(B >= 1 && K >= 1 && (long long)B * K <= 0x3FFFFFFF && steps >= 1 && steps <= 1024,
                  "coco_iw_text_sse: B=%d K=%d steps=%d out of range", B, K, steps);
    // (a caption row is steps * 1200 bytes, a multiple of 16: aligned bases keep every row aligned)
    MMVAE_REQUIRE(((reinterpret_cast<uintptr_t>(sentence) | reinterpret_cast<uintptr_t>(text)) & 15) == 0,
                  "coco_iw_text_sse: sentence / text are not 16-byte aligned");
    const long long n4 = (long long)steps * 300 / 4;
    MMVAE_LAUNCH(coco_iw_text_sse_kernel, dim3((unsigned)(B * K)), dim3(S_NTHR), 0, s, sentence, text, K, n4, sse);
    return mmvae_check_launch("coco_iw_text_sse");
}
