// The two small dependent Linears at the end of the image encoder's classifier (multimnist/model.py:173-179:
// Linear(400,200) -> Swish -> Dropout -> Linear(200,2D)) as ONE row-block launch, and their data gradients as one more.
//
// As separate launches they were 9.8 + 6.4 us forward and 15.2 + 17.1 us backward plus a launch gap each, all on the
// step's critical chain, for 0.1 GFLOP.  Rows are independent, so a workgroup takes 16 rows through both layers: the
// intermediate stays in LDS, the weights (266 / 272 KB bf16, fragment-major) stream from L2 through the register ring of
// stream_gemm.h, and the epilogues (bias, Swish, dropout, raw + activated copies for the backward pass; d-Swish, dropout,
// bias-gradient column sums) are those of the GEMM epilogue they replace, value for value.
//
// The kernels take the latent size DL as a compile-time parameter.  WAIST = false, DL = 100 is the pair the 3-pass step runs.
// WAIST = true (DL = 20, 100) is the one-expert waist of the image-only VAE step: without a product of experts a row stays
// independent up to z, so the forward goes on from classifier.6's result in LDS to (mu | logvar), z, z_bf and the workgroup's KL
// partial (latent1_fwd_kernel's expressions), and the backward forms the gradient wrt (mu | logvar) itself (latent1_bwd_kernel's
// double expression) while it stages its first operand.
#include "mlp_tail.h"
#include "stream_gemm.h"

namespace {

using namespace mmvae_sg;

constexpr int TR = 16;
constexpr int N1 = 400, N2 = 200;                                  // fc1 / fc2 widths
constexpr int K1P = 416, K2P = 224;                                // padded reduction widths (multiples of 32)
constexpr int LDX1 = K1P + 8, LDX2 = K2P + 8;                      // bf16 LDS row strides (+16 B: conflict-free ds_read_b128)
constexpr int LDO = 404;                                           // fp32 LDS row stride of a GEMM result (<= 400 columns)
constexpr int NQ2 = (N2 + 31) / 32, NQ1 = (N1 + 31) / 32;          // 7, 13
constexpr int RD = 4;                                              // ring depth of both kernels

// what follows from the latent size: classifier.6 is [N3][200]
template <int DL> struct Tail {
    static constexpr int N3 = 2 * DL;                              // (mu | logvar)
    static constexpr int NT3 = (N3 + 15) / 16;                     // its column tiles
    static constexpr int MAXT3 = (NT3 + NW - 1) / NW;              // tile slots per wave of the forward's second GEMM
    static constexpr int K3P = (N3 + 31) / 32 * 32;                // reduction width of the backward's first GEMM
    static constexpr int NQ3 = (N3 + 31) / 32, NQD = (DL + 31) / 32;
    using W2 = WMat<K1P / 32, (N2 + 15) / 16>;                     // classifier.3            [208][416]
    using W3 = WMat<K2P / 32, NT3>;                                // classifier.6            [16 NT3][224]
    using W3T = WMat<K3P / 32, (N2 + 15) / 16>;                    // classifier.6 transposed [208][K3P]: rows = fc2 units, k = fc3 outputs
    using W2T = WMat<K2P / 32, N1 / 16>;                           // classifier.3 transposed [400][224]: rows = fc1 units, k = fc2 units
    // The ring constraint of stream_gemm.h, per instantiation: the slot of every chunk is static, so the first GEMM of a kernel must
    // end on a slot the next one is compiled to start from.
    // forward: classifier.3 walks 2 tile slots x W2::nch chunks from slot 0 and requests classifier.6's first RD chunks behind
    // them; classifier.6 starts from slot 0 again
    static_assert((2 * W2::nch) % RD == 0, "forward: classifier.3's chunk count must be a multiple of the ring depth");
    static_assert(MAXT3 * W3::nch <= RD, "forward: classifier.6's chunks are all requested from inside classifier.3");
    // backward: 2 chunks of the first GEMM in slots 0-1, the second GEMM's 4 start in slot 2
    static_assert(W3T::nch == 1 && W2T::nch == 1 && (2 * W3T::nch) % RD == 2 && (2 * W3T::nch + 4 * W2T::nch) % RD == 2,
                  "backward: the data gradients' chunk lists no longer meet the ring slots they are compiled for");
    static_assert(N3 <= N2 && K3P <= K2P, "the LDS tiles are sized for 2 D <= 200");
    static_assert((size_t)TR * N3 * sizeof(double) <= (size_t)NQ1 * TR * 32 * sizeof(float), "the exact terms alias the column-sum staging");
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int DL, bool WAIST, class Args>
__global__ __launch_bounds__(NTHR) void mlp2_fwd_kernel(const Args a) {
    using T = Tail<DL>;
    constexpr int N3 = T::N3;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* o = reinterpret_cast<float*>(smem);                      // [16][LDO]
    bf16* xb = reinterpret_cast<bf16*>(o + TR * LDO);               // [16][LDX1] fc2 operand (activated fc1 output)
    bf16* hb = xb + TR * LDX1;                                      // [16][LDX2] fc3 operand (activated fc2 output)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = blockIdx.x * TR, rows = a.rows;
    const int grow = tid >> 5, c0 = tid & 31;
    const bool gok = r0 + grow < rows;
    const size_t gr = gok ? r0 + grow : 0;
    constexpr int D = RD;            // the whole of classifier.3's chunk list is requested before the first MFMA
    const typename T::W2 w2(a.w2);
    const typename T::W3 w3(a.w3);
    bf16x8 ring[D][KCH];
#pragma unroll
    for (int q = 0; q < D; ++q) load_chunk(ring[q], w2, q, wave, lane);
    // operand rows -> LDS (16-byte vectors; pad columns and rows past the end are zero)
    for (int i = tid; i < TR * (LDX1 / 8); i += NTHR) {
        const int row = i / (LDX1 / 8), v = i - row * (LDX1 / 8);
        bf16x8 x = {};
        if (r0 + row < rows && v * 8 < N1) x = *reinterpret_cast<const bf16x8*>(a.x + (size_t)(r0 + row) * N1 + v * 8);
        *reinterpret_cast<bf16x8*>(xb + row * LDX1 + v * 8) = x;
    }
    for (int i = tid; i < TR * LDX2; i += NTHR) hb[i] = (bf16)0.f;
    __syncthreads();
    // ---- fc2: 13 column tiles over 8 waves (2 slots), 13 k-steps in 2 chunks = 4 chunks per wave
    uint8_t kp[NQ2];                 // (requested before the GEMM: nothing of the epilogue waits on memory)
    float bb[NQ2];
#pragma unroll
    for (int q = 0; q < NQ2; ++q) {
        const int j = min(c0 + 32 * q, N2 - 1);
        kp[q] = a.mask ? a.mask[gr * N2 + j] : (uint8_t)1;
        bb[q] = a.b2[j];
    }
    stream_gemm<2, D, 0>(xb, LDX1, w2, o, LDO, ring, w3, true, wave, lane);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ2; ++q) {
        const int j = c0 + 32 * q;
        if (j < N2) {
            const float v = o[grow * LDO + j] + bb[q];
            float x = act_fwd(ACT_SWISH, v);
            if (a.mask) x = kp[q] ? x * a.mask_scale : 0.f;
            hb[grow * LDX2 + j] = (bf16)x;
            if (gok) { a.y2[gr * N2 + j] = (bf16)v; a.ay2[gr * N2 + j] = (bf16)x; }
        }
    }
    __syncthreads();
    // ---- fc3: NT3 tiles (13 at D = 100: 2 slots; 3 at D = 20: 1 slot), 7 k-steps = 1 chunk per slot
    stream_gemm<T::MAXT3, D, 0>(hb, LDX2, w3, o, LDO, ring, w3, false, wave, lane);
    __syncthreads();
    if constexpr (!WAIST) {
#pragma unroll
        for (int q = 0; q < T::NQ3; ++q) {
            const int j = c0 + 32 * q;
            if (j < N3 && gok) a.out[gr * N3 + j] = o[grow * LDO + j] + a.b3[j];
        }
    } else {
        // ---- the latent block of the thread's row: columns d = c0 + 32 q of mu and of logvar (latent1_fwd_kernel's expressions)
        double kl = 0.0;
#pragma unroll
        for (int q = 0; q < T::NQD; ++q) {
            const int d = c0 + 32 * q;
            if (d < DL && gok) {
                const float mu = o[grow * LDO + d] + a.b3[d], lv = o[grow * LDO + DL + d] + a.b3[DL + d];
                const size_t e = gr * DL + d;
                a.out[gr * N3 + d] = mu; a.out[gr * N3 + DL + d] = lv;
                if (a.mu) a.mu[e] = mu;
                if (a.logvar) a.logvar[e] = lv;
                const float z = a.training ? a.eps[e] * expf(0.5f * lv) + mu : mu;
                a.z_f32[e] = z;
                a.z_bf[gr * a.ldz + d] = (bf16)z;
                kl += (double)(-0.5f * (1.0f + lv - mu * mu - expf(lv)));
            }
        }
        if (gok)
            for (int c = DL + c0; c < a.ldz; c += 32) a.z_bf[gr * a.ldz + c] = (bf16)(c == DL ? 1.f : 0.f);
        // the workgroup's KL partial: thread (ascending q), wave (xor tree), workgroup (waves in order); a plain store
        double* part = reinterpret_cast<double*>(hb + TR * LDX2);   // [NW]
        kl = wave_sum_f64(kl);
        if (lane == 0) part[wave] = kl;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int w = 0; w < NW; ++w) t += part[w];
            a.scratch[blockIdx.x] = t;
        }
    }
}

// d_y2 = (d_out W3) * swish'(y2) * keep2 ;  d_y1 = (d_y2 W2) * swish'(y1) * keep1 ;  bias gradients = column sums
template <int DL, bool WAIST, class Args>
__global__ __launch_bounds__(NTHR) void mlp2_bwd_kernel(const Args a) {
    using T = Tail<DL>;
    constexpr int N3 = T::N3;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* o = reinterpret_cast<float*>(smem);                      // [16][LDO]
    float* cs = o + TR * LDO;                                       // [NQ1][16][32] column-sum staging (q, row lane, column lane)
    bf16* db = reinterpret_cast<bf16*>(cs + NQ1 * TR * 32);         // [16][LDX2] d_out, then d_y2
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = blockIdx.x * TR, rows = a.rows;
    const int grow = tid >> 5, c0 = tid & 31;
    const bool gok = r0 + grow < rows;
    const size_t gr = gok ? r0 + grow : 0;
    constexpr int D = RD;
    const typename T::W3T w3t(a.w3t);
    const typename T::W2T w2t(a.w2t);
    bf16x8 ring[D][KCH];
    load_chunk(ring[0], w3t, 0, wave, lane); load_chunk(ring[1], w3t, 1, wave, lane);       // the 2 chunks of the first GEMM
    load_chunk(ring[2], w2t, 0, wave, lane); load_chunk(ring[3], w2t, 1, wave, lane);       // and the first 2 of the second
    if constexpr (!WAIST) {
        for (int i = tid; i < TR * (LDX2 / 8); i += NTHR) {
            const int row = i / (LDX2 / 8), v = i - row * (LDX2 / 8);
            bf16x8 x = {};
            if (r0 + row < rows && v * 8 < N3) x = *reinterpret_cast<const bf16x8*>(a.d_out + (size_t)(r0 + row) * N3 + v * 8);
            *reinterpret_cast<bf16x8*>(db + row * LDX2 + v * 8) = x;
        }
    } else {
        // the gradient wrt (mu | logvar) of the thread's row, columns d = c0 + 32 q: latent1_bwd_kernel's doubles, rounded to bf16
        // into the operand tile and into d_enc_out (classifier.6's weight gradient reads it); the exact terms meet in LDS for the
        // column sums (classifier.6's bias gradient).  Rows past the end are zero.
        double* cd = reinterpret_cast<double*>(cs);                 // [16][N3]
#pragma unroll
        for (int q = 0; q < T::NQD; ++q) {
            const int d = c0 + 32 * q;
            if (d >= DL) continue;
            double gmu = 0.0, glv = 0.0;
            if (gok) {
                const size_t e = gr * DL + d;
                const double dz = a.dz ? (double)a.dz[e] : 0.0;
                const double mu = a.mu[e], lv = a.logvar[e], kc = a.kl_coef;
                gmu = dz + kc * mu;
                glv = -0.5 * kc * (1.0 - exp(lv));
                if (a.training) glv += dz * (double)a.eps[e] * 0.5 * exp(0.5 * lv);
                a.d_enc_out[gr * a.lde + d] = (bf16)(float)gmu;
                a.d_enc_out[gr * a.lde + DL + d] = (bf16)(float)glv;
            }
            db[grow * LDX2 + d] = (bf16)(float)gmu; db[grow * LDX2 + DL + d] = (bf16)(float)glv;
            cd[grow * N3 + d] = gmu; cd[grow * N3 + DL + d] = glv;
        }
        for (int c = N3 + c0; c < LDX2; c += 32) db[grow * LDX2 + c] = (bf16)0.f;
        if (gok)
            for (int c = N3 + c0; c < a.lde; c += 32) a.d_enc_out[gr * a.lde + c] = (bf16)0.f;
        __syncthreads();
        for (int col = tid; col < N3; col += NTHR) {                // rows in ascending order; a plain store
            double t = 0.0;
#pragma unroll
            for (int r = 0; r < TR; ++r) t += cd[r * N3 + col];
            a.scratch[gridDim.x + (size_t)blockIdx.x * N3 + col] = t;
        }
    }
    __syncthreads();
    // ---- through fc3: 13 tiles x K3P / 32 k-steps = 2 chunks per wave
    bf16 rr2[NQ2], rr1[NQ1];         // raw pre-activations and keep flags of both layers: requested up front, so that
    uint8_t kp2[NQ2], kp1[NQ1];      // neither epilogue waits on memory
#pragma unroll
    for (int q = 0; q < NQ2; ++q) {
        const int j = min(c0 + 32 * q, N2 - 1);
        rr2[q] = a.y2[gr * N2 + j];
        kp2[q] = a.mask2 ? a.mask2[gr * N2 + j] : (uint8_t)1;
    }
#pragma unroll
    for (int q = 0; q < NQ1; ++q) {
        const int j = min(c0 + 32 * q, N1 - 1);
        rr1[q] = a.y1[gr * N1 + j];
        kp1[q] = a.mask1 ? a.mask1[gr * N1 + j] : (uint8_t)1;
    }
    stream_gemm<2, D, 0>(db, LDX2, w3t, o, LDO, ring, w2t, true, wave, lane);
    __syncthreads();
    // bias gradients = column sums: a thread owns columns c0 + 32 q of ONE row; the 16 rows of a column meet in LDS
    auto colsums = [&](int ncols, float* dst) {
        __syncthreads();
        for (int col = tid; col < ncols; col += NTHR) {
            const float* p = cs + (col >> 5) * TR * 32 + (col & 31);
            float t = 0.f;
#pragma unroll
            for (int r = 0; r < TR; ++r) t += p[r * 32];
            atomicAdd(dst + col, t);
        }
    };
#pragma unroll
    for (int q = 0; q < NQ2; ++q) {
        const int j = c0 + 32 * q;
        float x = 0.f;
        if (j < N2 && gok) {
            x = o[grow * LDO + j] * act_bwd(ACT_SWISH, (float)rr2[q]);
            if (a.mask2) x = kp2[q] ? x * a.mask_scale : 0.f;
            a.dy2[gr * N2 + j] = (bf16)x;
        }
        cs[(q * TR + grow) * 32 + c0] = x;
        if (j < N2) db[grow * LDX2 + j] = (bf16)x;       // d_out is consumed (barrier behind the GEMM): the operand of the next one
    }
    colsums(N2, a.db2);
    __syncthreads();
    // ---- through fc2: 25 tiles (4 slots; the last holds one real tile) x 7 k-steps = 4 chunks per wave
    stream_gemm<4, D, 2>(db, LDX2, w2t, o, LDO, ring, w2t, false, wave, lane);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ1; ++q) {
        const int j = c0 + 32 * q;
        float x = 0.f;
        if (j < N1 && gok) {
            x = o[grow * LDO + j] * act_bwd(ACT_SWISH, (float)rr1[q]);
            if (a.mask1) x = kp1[q] ? x * a.mask_scale : 0.f;
            a.dy1[gr * N1 + j] = (bf16)x;
        }
        cs[(q * TR + grow) * 32 + c0] = x;
    }
    colsums(N1, a.db1);
}

// the partials of both waist kernels, folded in block order by one workgroup (see launch_mlp2_latent1_finish)
__global__ __launch_bounds__(256) void mlp2_latent1_finish_kernel(const double* scratch, int nblk, int D2, float* d_bias, const float* loss_slots,
                                                                  float* loss_out) {
    const int c = threadIdx.x;
    if (c < 16) {
        float t = 0.f;
        for (int q = 0; q < MMVAE_LOSS_SLOTS; ++q) t += loss_slots[q * 16 + c];
        if (c == 8) {
            double s = 0.0;
            for (int p = 0; p < nblk; ++p) s += scratch[p];
            t += (float)s;
        }
        loss_out[c] = t;
    }
    if (!d_bias || c >= D2) return;
    double s = 0.0;
    for (int r = 0; r < nblk; ++r) s += scratch[nblk + (size_t)r * D2 + c];
    d_bias[c] += (float)s;
}

constexpr size_t FWD_LDS = (size_t)TR * LDO * sizeof(float) + (size_t)TR * (LDX1 + LDX2) * sizeof(bf16);
constexpr size_t BWD_LDS = (size_t)(TR * LDO + NQ1 * TR * 32) * sizeof(float) + (size_t)TR * LDX2 * sizeof(bf16);
static_assert(FWD_LDS % sizeof(double) == 0 && ((size_t)TR * LDO * sizeof(float)) % sizeof(double) == 0, "the doubles in LDS are 8-byte aligned");

template <int DL>
int waist_fwd(const Mlp2Latent1FwdArgs& a, hipStream_t s) {
    MMVAE_LAUNCH((mlp2_fwd_kernel<DL, true, Mlp2Latent1FwdArgs>), dim3(ceil_div(a.rows, TR)), dim3(NTHR), FWD_LDS + NW * sizeof(double), s, a);
    return mmvae_check_launch("mlp2_latent1_fwd");
}
template <int DL>
int waist_bwd(const Mlp2Latent1BwdArgs& a, hipStream_t s) {
    MMVAE_LAUNCH((mlp2_bwd_kernel<DL, true, Mlp2Latent1BwdArgs>), dim3(ceil_div(a.rows, TR)), dim3(NTHR), BWD_LDS, s, a);
    return mmvae_check_launch("mlp2_latent1_bwd");
}

}  // namespace

int launch_mlp2_fwd(const Mlp2FwdArgs& a, hipStream_t s) {
    MMVAE_REQUIRE(a.rows > 0 && a.x && a.w2 && a.w3 && a.b2 && a.b3 && a.y2 && a.ay2 && a.out, "mlp2_fwd: null argument");
    MMVAE_LAUNCH((mlp2_fwd_kernel<100, false, Mlp2FwdArgs>), dim3(ceil_div(a.rows, TR)), dim3(NTHR), FWD_LDS, s, a);
    return mmvae_check_launch("mlp2_fwd");
}
int launch_mlp2_bwd(const Mlp2BwdArgs& a, hipStream_t s) {
    MMVAE_REQUIRE(a.rows > 0 && a.d_out && a.w3t && a.w2t && a.y2 && a.y1 && a.dy2 && a.dy1 && a.db2 && a.db1, "mlp2_bwd: null argument");
    MMVAE_LAUNCH((mlp2_bwd_kernel<100, false, Mlp2BwdArgs>), dim3(ceil_div(a.rows, TR)), dim3(NTHR), BWD_LDS, s, a);
    return mmvae_check_launch("mlp2_bwd");
}

bool mlp2_latent1_compiled(int D) { return D == 20 || D == 100; }
size_t mlp2_latent1_scratch_doubles(int rows, int D) { return (size_t)ceil_div(rows, TR) * (1 + 2 * (size_t)D); }
int launch_mlp2_latent1_fwd(const Mlp2Latent1FwdArgs& a, hipStream_t s) {
    MMVAE_REQUIRE(a.rows > 0 && a.x && a.w2 && a.w3 && a.b2 && a.b3 && a.y2 && a.ay2 && a.out && a.z_f32 && a.z_bf && a.scratch &&
                  (!a.training || a.eps), "mlp2_latent1_fwd: null argument");
    MMVAE_REQUIRE(a.ldz > a.D && ((uintptr_t)a.scratch & 7) == 0, "mlp2_latent1_fwd: ldz=%d must exceed D=%d, scratch must be 8-byte aligned", a.ldz, a.D);
    if (a.D == 20) return waist_fwd<20>(a, s);
    if (a.D == 100) return waist_fwd<100>(a, s);
    mmvae_set_error("mlp2_latent1_fwd: not compiled for n_latents = %d (20 and 100 are)", a.D);
    return MMVAE_EINVAL;
}
int launch_mlp2_latent1_bwd(const Mlp2Latent1BwdArgs& a, hipStream_t s) {
    MMVAE_REQUIRE(a.rows > 0 && a.w3t && a.w2t && a.y2 && a.y1 && a.dy2 && a.dy1 && a.db2 && a.db1 && a.mu && a.logvar && a.d_enc_out &&
                  a.scratch && (!a.training || a.eps), "mlp2_latent1_bwd: null argument");
    MMVAE_REQUIRE(a.lde >= 2 * a.D && ((uintptr_t)a.scratch & 7) == 0, "mlp2_latent1_bwd: lde=%d < 2D or scratch not 8-byte aligned", a.lde);
    if (a.D == 20) return waist_bwd<20>(a, s);
    if (a.D == 100) return waist_bwd<100>(a, s);
    mmvae_set_error("mlp2_latent1_bwd: not compiled for n_latents = %d (20 and 100 are)", a.D);
    return MMVAE_EINVAL;
}
int launch_mlp2_latent1_finish(const double* scratch, int rows, int D, float* d_bias, const float* loss_slots, float* loss_out, hipStream_t s) {
    MMVAE_REQUIRE(scratch && loss_slots && loss_out && rows > 0 && D >= 1 && 2 * D <= 256, "mlp2_latent1_finish: bad argument");
    MMVAE_LAUNCH(mlp2_latent1_finish_kernel, dim3(1), dim3(256), 0, s, scratch, ceil_div(rows, TR), 2 * D, d_bias, loss_slots, loss_out);
    return mmvae_check_launch("mlp2_latent1_finish");
}
