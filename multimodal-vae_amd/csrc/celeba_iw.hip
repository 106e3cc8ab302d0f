// CelebA importance-weighted evaluation: the two scoring kernels behind mmvae_celeba_iw_score (celeba.h).
//
// (a) celeba_iw_tail_kernel: the forward-only tail of the image decoder (celeba/model.py:146-150).  Per particle row
//       raw bf16 NHWC [32][32][32] (hallucinate.6) -> BatchNorm affine + activation -> ConvTranspose2d(32, 3, 4, 2, 1) -> 3x64x64
//       logits l -> loglik[row] = sum of x*l - softplus(l) against the image of example row / K (softplus not clamped).
//     The matrix-core formulation is the one of dec_last_ca_kernel (dec_last.hip): P[pixel][j = tap*3 + co] = A[pixel][32 ch] .
//     W[32 ch][j] (48 of 64 columns used), then every logit is the overlap-add of 4 entries of P out of LDS.  Forward only, so:
//       * the whole activated image stays in LDS (1024 pixels x 80 B), staged once per row;
//       * P is made in 4 strips of 8 input rows, one 32-pixel row per wave, into a ring of 9 row slots (row iy -> slot iy % 9):
//         a strip's output rows 2y0-1 .. 2y0+14 read input rows y0-1 .. y0+7, i.e. the 8 new rows and the last row of the strip
//         before -- no halo row is computed twice (the last strip also owns output row 63);
//       * a workgroup walks rows blockIdx.x, + gridDim.x, ...: the raw tensor of its next row is fetched into registers while the
//         current row is computed (one workgroup per CU fits: 135 KB of LDS, 2 waves per SIMD, so nothing else hides the load).
//     The sum has a fixed order (thread in fp32 -> wave shuffle tree and the 8 wave partials in double): no float atomics,
//     equal inputs give bit-equal outputs whatever the grid.  Nothing but loglik (and the tests' optional logits dump) is written.
// (b) celeba_iw_attrs_kernel: the attribute decoder (celeba/model.py:181-196) in fp32 on the bound fp32 parameters, 64 rows per
//     workgroup: z tile in LDS, a wave owns 16 of the 64 hidden units (its weights are wave-uniform loads), BatchNorm1d from the
//     running statistics, Swish, then Linear(64, 18); words[row][t] = (log(1 - p_t), log p_t) = (-softplus(a_t), -softplus(-a_t)),
//     the latter being a_t - softplus(a_t) without the cancellation.
#include "celeba.h"
#include "convres_epi.h"

namespace {

constexpr int T_IH = 32, T_IW = 32, T_OH = 64, T_OW = 64, T_C = 32, T_CO = 3, T_J = 48, T_NPIX = T_IH * T_IW;
constexpr int T_AP = 80;               // A: bytes per pixel (32 bf16 + 16)
constexpr int T_PF = 49;               // P: floats per pixel (48 + 1: the overlap-add reads a column across pixels)
constexpr int T_SR = 8, T_NS = T_IH / T_SR, T_SLOTS = T_SR + 1;
constexpr int T_WAVES = 8, T_NTHR = T_WAVES * 64;
constexpr int T_OFF_A = 0;                                          // [1024][80]
constexpr int T_OFF_P = T_OFF_A + T_NPIX * T_AP;                    // fp32 [9 slots][32][49]
constexpr int T_OFF_TAB = T_OFF_P + T_SLOTS * T_IW * T_PF * 4;      // float2 [32]
constexpr int T_LDS = T_OFF_TAB + T_C * 8;
constexpr int T_IT = T_NPIX * 4 / T_NTHR;                           // 16-byte vectors of a raw row per thread
static_assert(T_SR == T_WAVES, "one input row of a strip per wave");
static_assert(T_OFF_TAB % 16 == 0 && T_LDS <= 160 * 1024 - 64, "LDS budget");
static_assert(T_NPIX * 4 % T_NTHR == 0 && T_NTHR % 4 == 0, "a thread keeps its channel octet");

__device__ __forceinline__ float tail_act(int act, float v) {
    if (act == ACT_SWISH) return swish_fast(v);
    if (act == ACT_RELU) return fmaxf(v, 0.f);
    return v;
}

__global__ __launch_bounds__(T_NTHR) void celeba_iw_tail_kernel(const IwTailArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const A_s = smem + T_OFF_A;
    float* const P_s = reinterpret_cast<float*>(smem + T_OFF_P);
    float2* const aff_s = reinterpret_cast<float2*>(smem + T_OFF_TAB);
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
    // weight fragments, fp32 (32, 3, 4, 4) -> bf16, column j = tap*3 + co: B[k = ch][j] for the two k-steps and the two column tiles
    bf16x8 wf[2][2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int j = nt * 32 + r, tap = j / T_CO, co = j - tap * T_CO;
#pragma unroll
            for (int e = 0; e < 8; ++e) wf[ks][nt][e] = j < T_J ? (bf16)a.w[((ks * 16 + 8 * h + e) * T_CO + co) * 16 + tap] : (bf16)0.f;
        }
    i32x4c rv[T_IT];
    auto fetch = [&](int row) {
        const bf16* src = a.q3 + (size_t)row * T_NPIX * T_C;
#pragma unroll
        for (int it = 0; it < T_IT; ++it) rv[it] = *reinterpret_cast<const i32x4c*>(src + (size_t)(tid + it * T_NTHR) * 8);
    };
    int row = blockIdx.x;
    if (row < a.rows) fetch(row);
    __syncthreads();
    const int cv = tid & 3;
    float sc[8], sh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float2 t = aff_s[cv * 8 + e]; sc[e] = t.x; sh[e] = t.y; }

    for (; row < a.rows; row += gridDim.x) {
        // ---- stage: affine + activation -> A (every reader of the previous row's A passed a barrier of its last strip)
#pragma unroll
        for (int it = 0; it < T_IT; ++it) {
            const int v = tid + it * T_NTHR;
            const bf16x8 x = __builtin_bit_cast(bf16x8, rv[it]);
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (bf16)tail_act(a.act, (float)x[e] * sc[e] + sh[e]);
            *reinterpret_cast<bf16x8*>(A_s + (v >> 2) * T_AP + cv * 16) = o;
        }
        if (row + (int)gridDim.x < a.rows) fetch(row + (int)gridDim.x);      // in flight through the strips below
        __syncthreads();
        const float* const timg = a.image + (size_t)(row / a.K) * (T_CO * T_OH * T_OW);
        float* const lg = a.logits ? a.logits + (size_t)row * (T_CO * T_OH * T_OW) : nullptr;
        float ll = 0.f;
        for (int strip = 0; strip < T_NS; ++strip) {
            const int y0 = strip * T_SR;
            {   // ---- P[pixel][j] of input row y0 + wave
                const int iy = y0 + wave, slot = iy % T_SLOTS;
                const char* ap = A_s + (iy * T_IW + r) * T_AP + h * 16;
                const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(ap), a1 = *reinterpret_cast<const bf16x8*>(ap + 32);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    f32x16 acc;
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, wf[0][nt], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, wf[1][nt], acc, 0, 0, 0);
                    const int j = nt * 32 + r;
                    if (j < T_J) {                           // lane = column j, register e = pixel (e&3) + 8*(e>>2) + 4h of the row
#pragma unroll
                        for (int e = 0; e < 16; ++e) P_s[(slot * T_IW + (e & 3) + 8 * (e >> 2) + 4 * h) * T_PF + j] = acc[e];
                    }
                }
            }
            __syncthreads();
            // ---- logits of output rows 2y0-1 .. 2y0+14 (the last strip: .. 63) by overlap-add, and their terms of the sum
            const int oy_lo = strip == 0 ? 0 : 2 * y0 - 1, oy_hi = strip == T_NS - 1 ? T_OH : 2 * y0 + 2 * T_SR - 1;
            const int no = (oy_hi - oy_lo) * T_CO * T_OW;
            for (int o = tid; o < no; o += T_NTHR) {
                const int q = o >> 6, ox = o & 63, lo = q / T_CO, co = q - lo * T_CO, oy = oy_lo + lo;
                const int kh0 = (oy + 1) & 1, kw0 = (ox + 1) & 1;
                const int iy0 = (oy + 1 - kh0) >> 1, ix0 = (ox + 1 - kw0) >> 1;
                float acc = 0.f;
#pragma unroll
                for (int ty = 0; ty < 2; ++ty)
#pragma unroll
                    for (int tx = 0; tx < 2; ++tx) {
                        // a row / column outside the image is masked, not branched on (its clamped slot holds a row of the image)
                        const int iy = iy0 - ty, ix = ix0 - tx;
                        const int iyc = min(max(iy, 0), T_IH - 1), ixc = min(max(ix, 0), T_IW - 1);
                        const float pv = P_s[((iyc % T_SLOTS) * T_IW + ixc) * T_PF + ((kh0 + 2 * ty) * 4 + kw0 + 2 * tx) * T_CO + co];
                        acc += (iy == iyc && ix == ixc) ? pv : 0.f;
                    }
                const int oi = (co * T_OH + oy) * T_OW + ox;                 // NCHW
                if (lg) lg[oi] = acc;
                ll += timg[oi] * acc - (fmaxf(acc, 0.f) + log1pf(expf(-fabsf(acc))));
            }
            __syncthreads();                                 // the next strip (or row) overwrites slots / A read above
        }
        // a thread's 24-25 terms in fp32, the 512 thread sums in double (once per row): the sum of 12288 terms of one sign is
        // rounded to fp32 once
        double dl = (double)ll;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dl += __shfl_xor(dl, o, 64);
        if (lane == 0) part[wave] = dl;
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int w = 0; w < T_WAVES; ++w) s += part[w];
            a.loglik[row] = (float)s;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
constexpr int AT_R = 64, AT_WAVES = 4, AT_NTHR = AT_WAVES * 64, AT_H = 64, AT_NA = 18, AT_HS = AT_H + 1;
static_assert(AT_H % AT_WAVES == 0, "hidden units per wave");

__global__ __launch_bounds__(AT_NTHR) void celeba_iw_attrs_kernel(const CelebaIwAttrsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int D = a.D, ZS = D + 1;                           // odd strides: a wave's 64 rows hit 64 different banks
    float* const zs = lds;                                   // [AT_R][ZS]
    float* const hs = lds + AT_R * ZS;                       // [AT_R][AT_HS]
    const int tid = threadIdx.x, m = tid & 63;
    const int g = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long row0 = (long long)blockIdx.x * AT_R;
    const int nvalid = (int)(a.rows - row0 < AT_R ? a.rows - row0 : AT_R);

    for (int i = tid; i < AT_R * D; i += AT_NTHR) {
        const int mm = i / D, d = i - mm * D;
        zs[mm * ZS + d] = mm < nvalid ? a.z[row0 * D + i] : 0.f;
    }
    __syncthreads();
    {   // Linear(D, 64) -> BatchNorm1d (running statistics) -> Swish: row m, hidden units 16g .. 16g+15
        constexpr int HU = AT_H / AT_WAVES;
        float acc[HU];
#pragma unroll
        for (int j = 0; j < HU; ++j) acc[j] = a.b0[g * HU + j];
        const float* const w = a.w0 + (size_t)(g * HU) * D;
        for (int d = 0; d < D; ++d) {
            const float zv = zs[m * ZS + d];
#pragma unroll
            for (int j = 0; j < HU; ++j) acc[j] = fmaf(w[j * D + d], zv, acc[j]);
        }
#pragma unroll
        for (int j = 0; j < HU; ++j) {
            const int c = g * HU + j;
            const float v = (acc[j] - a.rmean[c]) / sqrtf(a.rvar[c] + a.eps) * a.gamma[c] + a.beta[c];
            hs[m * AT_HS + c] = v / (1.f + expf(-v));
        }
    }
    __syncthreads();
    for (int t = g; t < AT_NA; t += AT_WAVES) {              // Linear(64, 18): attribute t of row m
        float s = a.b1[t];
        const float* const w = a.w1 + t * AT_H;
#pragma unroll 8
        for (int j = 0; j < AT_H; ++j) s = fmaf(w[j], hs[m * AT_HS + j], s);
        const float e = log1pf(expf(-fabsf(s)));
        if (m < nvalid)
            reinterpret_cast<float2*>(a.words)[(row0 + m) * AT_NA + t] = make_float2(-(fmaxf(s, 0.f) + e), -(fmaxf(-s, 0.f) + e));
    }
}

}  // namespace

int launch_celeba_iw_tail(const IwTailArgs& a, hipStream_t s) {
    MMVAE_REQUIRE(a.q3 && a.w && a.image && a.loglik, "celeba_iw_tail: null argument");
    MMVAE_REQUIRE(a.affine || (a.gamma && a.beta && a.rmean && a.rvar), "celeba_iw_tail: neither an affine table nor BatchNorm buffers");
    MMVAE_REQUIRE(a.act == ACT_NONE || a.act == ACT_SWISH || a.act == ACT_RELU, "celeba_iw_tail: unknown activation %d", a.act);
    // (row indices are 32-bit in the kernel; the byte offsets are 64-bit)
    MMVAE_REQUIRE(a.rows >= 1 && a.K >= 1 && a.rows % a.K == 0 && a.rows <= 0x3FFFFFFF, "celeba_iw_tail: rows=%d K=%d", a.rows, a.K);
    MMVAE_REQUIRE((reinterpret_cast<uintptr_t>(a.q3) & 15) == 0, "celeba_iw_tail: the raw tensor is not 16-byte aligned");
    static std::atomic<unsigned> attr_set{0};
    if (mmvae_first_use_on_device(attr_set))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&celeba_iw_tail_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, T_LDS);
    const int cus = mmvae_cu_count();                        // one resident workgroup per CU: each walks rows / cus rows
    const int grid = a.rows < cus ? a.rows : cus;
    MMVAE_LAUNCH(celeba_iw_tail_kernel, dim3(grid), dim3(T_NTHR), T_LDS, s, a);
    return mmvae_check_launch("celeba_iw_tail");
}

int launch_celeba_iw_attrs(const CelebaIwAttrsArgs& a, hipStream_t s) {
    MMVAE_REQUIRE(a.w0 && a.b0 && a.gamma && a.beta && a.rmean && a.rvar && a.w1 && a.b1 && a.z && a.words, "celeba_iw_attrs: null argument");
    MMVAE_REQUIRE(a.rows >= 1 && a.rows < 0x7FFFFFFFll && a.D >= 1 && a.D <= 128, "celeba_iw_attrs: rows=%lld D=%d out of range (rows below 2^31)",
                  a.rows, a.D);
    MMVAE_REQUIRE((reinterpret_cast<uintptr_t>(a.words) & 7) == 0, "celeba_iw_attrs: words is not 8-byte aligned");
    const size_t lds = sizeof(float) * (size_t)AT_R * (a.D + 1 + AT_HS);
    MMVAE_LAUNCH(celeba_iw_attrs_kernel, dim3((unsigned)((a.rows + AT_R - 1) / AT_R)), dim3(AT_NTHR), lds, s, a);
    return mmvae_check_launch("celeba_iw_attrs");
}
