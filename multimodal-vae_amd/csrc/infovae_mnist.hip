// See infovae_mnist.h.
#include "infovae_mnist.h"
#include "conv4s2.h"
#include "mmd.h"
#include "plan_base.h"

namespace {

// ------------------------------------------------------------------ device helpers
// v_mfma_f32_16x16x4_f32: A operand lane -> (row lane % 16, k slot lane / 16), B operand lane -> (column lane % 16, k slot lane / 16),
// accumulator lane -> column lane % 16, rows 4 * (lane / 16) .. + 3.
// Every operand goes through a buffer descriptor whose size is the tensor's own: an element that does not exist (row or feature past
// the end, a step past the wave's range) is the offset OOB, which the hardware's range check turns into 0 without a branch.
constexpr unsigned OOB = 0xFFFFFFFFu;
typedef __amdgpu_buffer_rsrc_t rsrc_t;

__device__ __forceinline__ rsrc_t make_rsrc(const float* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float ld1(rsrc_t r, unsigned off) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0)); }
__device__ __forceinline__ f32x4 ld4(rsrc_t r, unsigned off) { return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0)); }

// where feature f = c * 49 + p of a weight lives in a channels-last [49][128] activation row
__device__ __forceinline__ int perm_idx(int f) {
    const int c = f / LIN_PERM_P;
    return (f - c * LIN_PERM_P) * LIN_PERM_C + c;
}
// features f .. f + 3 of the row that starts `row` bytes into the tensor (F features per row).  VEC: one 16-byte load (f and F are
// multiples of 4, so the four exist together); else four 4-byte loads, through the permutation when PERM.
template <bool VEC, bool PERM>
__device__ __forceinline__ f32x4 fetch4(rsrc_t r, unsigned row, bool row_ok, int f, int F) {
    if (VEC) return ld4(r, (row_ok && f < F) ? row + (unsigned)f * 4u : OOB);
    f32x4 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int fq = f + q;
        const bool ok = row_ok && fq < F;
        const int idx = PERM ? perm_idx(ok ? fq : 0) : fq;
        v[q] = ld1(r, ok ? row + (unsigned)idx * 4u : OOB);
    }
    return v;
}
__device__ __forceinline__ float act_of(int act, float slope, float v) {
    if (act == LIN_ACT_RELU) return v > 0.f ? v : 0.f;
    if (act == LIN_ACT_LEAKY) return v > 0.f ? v : slope * v;
    return v;
}
// the gradient in front of the activation from the upstream gradient and the saved output (conv4s2.h's contract)
__device__ __forceinline__ float gp_of(int act, float slope, float g, float y) {
    if (act == LIN_ACT_RELU) return y > 0.f ? g : 0.f;
    if (act == LIN_ACT_LEAKY) return y > 0.f ? g : slope * g;
    return g;
}
__device__ __forceinline__ f32x4 gp4(int act, float slope, f32x4 g, f32x4 y) {
    f32x4 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = gp_of(act, slope, g[q], y[q]);
    return v;
}

struct LinK {
    const float *a, *a2, *w, *bias;     // a: x (forward, weight gradient) or g; a2: the saved output y beside g, or null
    float *out, *out2, *part;           // out2: db of the weight gradient
    int rows, N, K, act, perm_out, nz;
    float slope;
    unsigned a_bytes, a2_bytes, x_bytes, w_bytes;
    const float* x;                     // weight gradient: the layer's input
};

// one element behind the reduction: bias, activation, store (through the permutation when the layer's output side is permuted)
__device__ __forceinline__ void finish(const float* bias, int act, float slope, int perm_out, float* out, int cols, int m, int c, float v) {
    if (bias) v += bias[c];
    out[(size_t)m * cols + (perm_out ? perm_idx(c) : c)] = act_of(act, slope, v);
}

// ------------------------------------------------------------------ forward: y = act(x W^T + b)
// A workgroup owns 64 rows x 16 output columns and chunk blockIdx.z of the reduction; its 4 waves cut the chunk in four and are folded
// through LDS in ascending order.  Within a 16-deep step lane group q holds k = k0 + 4 q .. + 3 of BOTH operands (MFMA s consumes
// k0 + 4 q + s): a weight row is read with one 16-byte load per lane and step, 64 contiguous bytes per step and U steps in flight.
template <bool WV, bool AV, bool PERM>
__global__ __launch_bounds__(256) void lin_fwd_kernel(const LinK g) {
    __shared__ float red[3 * 16 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
    const int n0 = blockIdx.x * 16, m0 = blockIdx.y * 64, z = blockIdx.z;
    const rsrc_t ar = make_rsrc(g.a, g.a_bytes), wr = make_rsrc(g.w, g.w_bytes);
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool nok = n0 + fr < g.N;
    const unsigned wrow = (unsigned)(n0 + fr) * (unsigned)g.K * 4u;
    unsigned arow[4];
    bool aok[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int m = m0 + 16 * t + fr;
        aok[t] = m < g.rows;
        arow[t] = (unsigned)m * (unsigned)g.K * 4u;
    }
    const int nst_all = (g.K + 15) / 16;
    const int zs0 = (int)((long long)nst_all * z / g.nz), zs1 = (int)((long long)nst_all * (z + 1) / g.nz);
    const int nst = zs1 - zs0;
    const int st0 = zs0 + nst * wave / 4, st1 = zs0 + nst * (wave + 1) / 4;
    constexpr int U = (WV && AV) ? 4 : 2;
    for (int st = st0; st < st1; st += U) {
        f32x4 av[U][4], bv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool sin = st + u < st1;
            const int kb = (st + u) * 16 + fq * 4;
            bv[u] = fetch4<WV, false>(wr, wrow, sin && nok, kb, g.K);
#pragma unroll
            for (int t = 0; t < 4; ++t) av[u][t] = fetch4<AV, PERM>(ar, arow[t], sin && aok[t], kb, g.K);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][t][q], bv[u][q], acc[t], 0, 0, 0);
    }
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[((wave - 1) * 16 + t * 4 + r) * 64 + lane] = acc[t][r];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int w = 0; w < 3; ++w)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t][r] += red[(w * 16 + t * 4 + r) * 64 + lane];
    const int n = n0 + fr;
    if (n >= g.N) return;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 16 * t + 4 * fq + r;
            if (m >= g.rows) continue;
            if (g.nz > 1) g.part[((size_t)z * g.rows + m) * g.N + n] = acc[t][r];
            else finish(g.bias, g.act, g.slope, g.perm_out, g.out, g.N, m, n, acc[t][r]);
        }
}

// out[m][c] = act(sum_z part[z][m][c] + bias[c]), z ascending
__global__ __launch_bounds__(256) void lin_fold_kernel(const float* __restrict__ part, int nz, int rows, int cols, const float* bias, int act,
                                                       float slope, int perm_out, float* out) {
    const size_t total = (size_t)rows * cols, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float v = part[i];
    for (int z = 1; z < nz; ++z) v += part[(size_t)z * total + i];
    const int m = (int)(i / cols), c = (int)(i - (size_t)m * cols);
    finish(bias, act, slope, perm_out, out, cols, m, c, v);
}

// ------------------------------------------------------------------ data gradient: dx = (g (.) act'(y)) W
// A workgroup owns 64 rows x 64 columns of dx and chunk blockIdx.z of the reduction over n, cut in four over its waves as above.  Lane
// group q holds n = n0 + 4 q .. + 3 of g and y (one 16-byte load each); a weight row n is read along k, 16 bytes per lane, 256
// contiguous bytes per row: the lane's four values belong to four column tiles, tile t owning the columns k0 + 4 j + t.
template <bool VECA, bool PERM, bool VECB>
__global__ __launch_bounds__(256) void lin_dgrad_kernel(const LinK g) {
    __shared__ float red[3 * 64 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
    const int k0 = blockIdx.x * 64, m0 = blockIdx.y * 64, z = blockIdx.z;
    const rsrc_t gr = make_rsrc(g.a, g.a_bytes), yr = make_rsrc(g.a2, g.a2_bytes), wr = make_rsrc(g.w, g.w_bytes);
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    unsigned arow[4];
    bool aok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + 16 * i + fr;
        aok[i] = m < g.rows;
        arow[i] = (unsigned)m * (unsigned)g.N * 4u;
    }
    const int nst_all = (g.N + 15) / 16;
    const int zs0 = (int)((long long)nst_all * z / g.nz), zs1 = (int)((long long)nst_all * (z + 1) / g.nz);
    const int nst = zs1 - zs0;
    const int st0 = zs0 + nst * wave / 4, st1 = zs0 + nst * (wave + 1) / 4;
    const bool with_y = g.act != LIN_ACT_NONE;
    for (int st = st0; st < st1; ++st) {
        const int nb = st * 16 + fq * 4;
        f32x4 a[4], bv[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) bv[s] = fetch4<VECB, false>(wr, (unsigned)(nb + s) * (unsigned)g.K * 4u, nb + s < g.N, k0 + 4 * fr, g.K);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 gv = fetch4<VECA, PERM>(gr, arow[i], aok[i], nb, g.N);
            f32x4 yv = f32x4{0.f, 0.f, 0.f, 0.f};
            if (with_y) yv = fetch4<VECA, PERM>(yr, arow[i], aok[i], nb, g.N);
            a[i] = gp4(g.act, g.slope, gv, yv);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][s], bv[s][t], acc[i][t], 0, 0, 0);
    }
    if (wave > 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[((wave - 1) * 64 + (i * 4 + t) * 4 + r) * 64 + lane] = acc[i][t][r];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int w = 0; w < 3; ++w)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][t][r] += red[(w * 64 + (i * 4 + t) * 4 + r) * 64 + lane];
    const int kc = k0 + 4 * fr;
    if (kc >= g.K) return;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 16 * i + 4 * fq + r;
            if (m >= g.rows) continue;
            float* dst = g.nz > 1 ? g.part + ((size_t)z * g.rows + m) * g.K : g.out + (size_t)m * g.K;
            if (VECB && (g.nz > 1 || !g.perm_out)) {        // (K % 4 == 0: the four columns exist together, 16-byte aligned)
                *reinterpret_cast<f32x4*>(dst + kc) = f32x4{acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]};
                continue;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (kc + t >= g.K) continue;
                dst[(g.nz > 1 || !g.perm_out) ? kc + t : perm_idx(kc + t)] = acc[i][t][r];
            }
        }
}

// ------------------------------------------------------------------ weight gradient: dW = (g (.) act'(y))^T x, db = its column sums
// A wave owns 64 x 64 of dW (a workgroup 64 x 256); the reduction is the batch, 4 rows per MFMA (row = k slot), so every element has
// one writer and there is nothing to fold.  Both operands are read along their rows, 16 bytes per lane: the lane's four values belong
// to four tiles (n = n0 + 4 j + ti, k = k0 + 4 j + tj), and a dW row segment is stored as 16 lanes x 16 bytes.  The workgroup of the
// first k block also multiplies gp by a column of ones: db.
template <bool NV, bool PERM_N, bool KV, bool PERM_K>
__global__ __launch_bounds__(256) void lin_wgrad_kernel(const LinK g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
    const int k0 = blockIdx.x * 256 + wave * 64, n0 = blockIdx.y * 64;
    if (k0 >= g.K) return;
    const rsrc_t gr = make_rsrc(g.a, g.a_bytes), yr = make_rsrc(g.a2, g.a2_bytes), xr = make_rsrc(g.x, g.x_bytes);
    const bool with_y = g.act != LIN_ACT_NONE, with_db = g.out2 != nullptr && blockIdx.x == 0 && wave == 0;
    f32x4 acc[4][4], accb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    constexpr int U = 2;
    for (int mb = 0; mb < g.rows; mb += 4 * U) {
        f32x4 a[U], xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int m = mb + 4 * u + fq;
            const bool ok = m < g.rows;
            const f32x4 gv = fetch4<NV && !PERM_N, PERM_N>(gr, (unsigned)m * (unsigned)g.N * 4u, ok, n0 + 4 * fr, g.N);
            f32x4 yv = f32x4{0.f, 0.f, 0.f, 0.f};
            if (with_y) yv = fetch4<NV && !PERM_N, PERM_N>(yr, (unsigned)m * (unsigned)g.N * 4u, ok, n0 + 4 * fr, g.N);
            a[u] = gp4(g.act, g.slope, gv, yv);
            xv[u] = fetch4<KV && !PERM_K, PERM_K>(xr, (unsigned)m * (unsigned)g.K * 4u, ok, k0 + 4 * fr, g.K);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][i], xv[u][t], acc[i][t], 0, 0, 0);
            if (with_db) {
#pragma unroll
                for (int i = 0; i < 4; ++i) accb[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][i], 1.0f, accb[i], 0, 0, 0);
            }
        }
    }
    const int kc = k0 + 4 * fr;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + 4 * (4 * fq + r) + i;
            if (n >= g.N) continue;
            if (with_db && fr == 0) g.out2[n] = accb[i][r];
            if (kc >= g.K) continue;
            float* dst = g.out + (size_t)n * g.K + kc;
            if (KV) {
                *reinterpret_cast<f32x4*>(dst) = f32x4{acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]};
                continue;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (kc + t < g.K) dst[t] = acc[i][t][r];
        }
}

// ------------------------------------------------------------------ loss tail
// block q of MMVAE_LOSS_SLOTS: the elements [n q / SLOTS, n (q + 1) / SLOTS), thread-strided sums folded by a fixed tree
__global__ __launch_bounds__(256) void mse_tail_kernel(const float* __restrict__ recon, const float* __restrict__ x, long long n, float coef,
                                                       float* __restrict__ gout, float* __restrict__ slots) {
    __shared__ float red[256];
    const long long i0 = n * blockIdx.x / MMVAE_LOSS_SLOTS, i1 = n * (blockIdx.x + 1) / MMVAE_LOSS_SLOTS;
    float s = 0.f;
    for (long long i = i0 + threadIdx.x; i < i1; i += 256) {
        const float d = recon[i] - x[i];
        s += d * d;
        if (gout) gout[i] = coef * (2.0f * d);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) slots[blockIdx.x * 16] = red[0];
}

// dz = a + b, the sum taken in float64 and rounded once (the two terms' gradients in z)
__global__ __launch_bounds__(256) void add2_kernel(const float* a, const float* b, int n, float* out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)((double)a[i] + (double)b[i]);
}

int perm_side(const LinShape& s) {      // 0 none, 1 the K side, 2 the N side
    const int W = LIN_PERM_P * LIN_PERM_C;
    if (!s.perm) return 0;
    return s.K == W ? 1 : 2;
}
unsigned bytes_of(int rows, int cols) { return (unsigned)((size_t)rows * cols * 4); }

}  // namespace

const char* lin_shape_error(const LinShape& s) {
    const int W = LIN_PERM_P * LIN_PERM_C;
    if (s.rows < 1 || s.rows > LIN_MAX_ROWS) return "rows out of range (1..65536)";
    if (s.N < 1 || s.N > LIN_MAX_DIM || s.K < 1 || s.K > LIN_MAX_DIM) return "N or K out of range (1..65536)";
    if ((long long)s.N * s.K > (1ll << 28)) return "the weight has more than 2^28 elements";
    if ((long long)s.rows * (s.N > s.K ? s.N : s.K) > (1ll << 28)) return "an activation has more than 2^28 elements";
    if (s.act < LIN_ACT_NONE || s.act > LIN_ACT_LEAKY) return "act must be 0 (none), 1 (relu) or 2 (leaky)";
    if (s.perm != 0 && s.perm != 1) return "perm must be 0 or 1";
    if (s.perm && ((s.N == W) == (s.K == W))) return "perm needs exactly one of N, K to be 6272 (49 x 128)";
    return nullptr;
}

// Workgroups wanted: about one per compute unit.  `blocks` = the launch's workgroups per reduction chunk and row block; a chunk is at
// least 8 steps of 16 terms.  A function of the layer's shape alone: the batch never changes how a row's sum is cut.
int lin_ksplit(int blocks, int red) {
    const int nst = (red + 15) / 16;
    int cap = nst / 8;
    if (cap > LIN_MAX_SPLIT) cap = LIN_MAX_SPLIT;
    int want = 256 / (blocks > 0 ? blocks : 1);
    if (want > cap) want = cap;
    return want < 1 ? 1 : want;
}
static int fwd_split(const LinShape& s) { return lin_ksplit(ceil_div(s.N, 16), s.K); }
static int dgrad_split(const LinShape& s) { return lin_ksplit(ceil_div(s.K, 64), s.N); }
size_t lin_fwd_workspace_bytes(const LinShape& s) {
    const int nz = fwd_split(s);
    return nz > 1 ? (size_t)nz * s.rows * s.N * sizeof(float) : 0;
}
size_t lin_dgrad_workspace_bytes(const LinShape& s) {
    const int nz = dgrad_split(s);
    return nz > 1 ? (size_t)nz * s.rows * s.K * sizeof(float) : 0;
}

static int lin_check(const char* what, const LinShape& s, std::initializer_list<const void*> ptrs) {
    const char* e = lin_shape_error(s);
    MMVAE_REQUIRE(e == nullptr, "%s: rows = %d, N = %d, K = %d, act = %d, perm = %d: %s", what, s.rows, s.N, s.K, s.act, s.perm, e);
    for (const void* p : ptrs) MMVAE_REQUIRE(aligned16(p), "%s: every pointer must be 16-byte aligned", what);
    return MMVAE_OK;
}

int launch_lin_fwd(const LinShape& s, const float* x, const float* w, const float* b, float* y, void* ws, hipStream_t st) {
    MMVAE_REQUIRE(x && w && b && y, "lin_act_fwd: null argument");
    MMVAE_TRY(lin_check("lin_act_fwd", s, {x, w, b, y, ws}));
    const int side = perm_side(s), nz = fwd_split(s);
    MMVAE_REQUIRE(nz == 1 || ws != nullptr, "lin_act_fwd: the layer needs its workspace");
    LinK g{};
    g.a = x; g.w = w; g.bias = b; g.out = y; g.part = static_cast<float*>(ws);
    g.rows = s.rows; g.N = s.N; g.K = s.K; g.act = s.act; g.slope = s.slope; g.perm_out = side == 2; g.nz = nz;
    g.a_bytes = bytes_of(s.rows, s.K); g.w_bytes = bytes_of(s.N, s.K);
    const dim3 grid(ceil_div(s.N, 16), ceil_div(s.rows, 64), nz), block(256);
    const bool kv = s.K % 4 == 0;
    if (side == 1) MMVAE_LAUNCH((lin_fwd_kernel<true, false, true>), grid, block, 0, st, g);
    else if (kv) MMVAE_LAUNCH((lin_fwd_kernel<true, true, false>), grid, block, 0, st, g);
    else MMVAE_LAUNCH((lin_fwd_kernel<false, false, false>), grid, block, 0, st, g);
    MMVAE_TRY(mmvae_check_launch("lin_fwd"));
    if (nz == 1) return MMVAE_OK;
    const size_t total = (size_t)s.rows * s.N;
    const float* part = g.part;
    MMVAE_LAUNCH(lin_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part, nz, g.rows, g.N, b, g.act, g.slope,
                 g.perm_out, y);
    return mmvae_check_launch("lin_fwd_fold");
}

int launch_lin_dgrad(const LinShape& s, const float* gu, const float* y, const float* w, float* dx, void* ws, hipStream_t st) {
    MMVAE_REQUIRE(gu && w && dx && (y || s.act == LIN_ACT_NONE), "lin_act_dgrad: null argument");
    MMVAE_TRY(lin_check("lin_act_dgrad", s, {gu, y, w, dx, ws}));
    const int side = perm_side(s), nz = dgrad_split(s);
    MMVAE_REQUIRE(nz == 1 || ws != nullptr, "lin_act_dgrad: the layer needs its workspace");
    LinK g{};
    g.a = gu; g.a2 = y; g.w = w; g.out = dx; g.part = static_cast<float*>(ws);
    g.rows = s.rows; g.N = s.N; g.K = s.K; g.act = s.act; g.slope = s.slope; g.perm_out = side == 1; g.nz = nz;
    g.a_bytes = bytes_of(s.rows, s.N); g.a2_bytes = y ? g.a_bytes : 0; g.w_bytes = bytes_of(s.N, s.K);
    const dim3 grid(ceil_div(s.K, 64), ceil_div(s.rows, 64), nz), block(256);
    const bool nv = s.N % 4 == 0, kv = s.K % 4 == 0;
#define LIN_DG(A, P, B) MMVAE_LAUNCH((lin_dgrad_kernel<A, P, B>), grid, block, 0, st, g)
    if (side == 2) { if (kv) LIN_DG(false, true, true); else LIN_DG(false, true, false); }
    else if (nv) { if (kv) LIN_DG(true, false, true); else LIN_DG(true, false, false); }
    else { if (kv) LIN_DG(false, false, true); else LIN_DG(false, false, false); }
#undef LIN_DG
    MMVAE_TRY(mmvae_check_launch("lin_dgrad"));
    if (nz == 1) return MMVAE_OK;
    const size_t total = (size_t)s.rows * s.K;
    const float *part = g.part, *no_bias = nullptr;
    const int no_act = LIN_ACT_NONE;
    const float no_slope = 0.f;
    MMVAE_LAUNCH(lin_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part, nz, g.rows, g.K, no_bias, no_act, no_slope,
                 g.perm_out, dx);
    return mmvae_check_launch("lin_dgrad_fold");
}

int launch_lin_wgrad(const LinShape& s, const float* gu, const float* y, const float* x, float* dw, float* db, hipStream_t st) {
    MMVAE_REQUIRE(gu && x && dw && (y || s.act == LIN_ACT_NONE), "lin_act_wgrad: null argument");
    MMVAE_TRY(lin_check("lin_act_wgrad", s, {gu, y, x, dw, db}));
    const int side = perm_side(s);
    LinK g{};
    g.a = gu; g.a2 = y; g.x = x; g.out = dw; g.out2 = db;
    g.rows = s.rows; g.N = s.N; g.K = s.K; g.act = s.act; g.slope = s.slope;
    g.a_bytes = bytes_of(s.rows, s.N); g.a2_bytes = y ? g.a_bytes : 0; g.x_bytes = bytes_of(s.rows, s.K);
    const dim3 grid(ceil_div(s.K, 256), ceil_div(s.N, 64)), block(256);
    const bool nv = s.N % 4 == 0, kv = s.K % 4 == 0;
#define LIN_WG(A, B, C, D) MMVAE_LAUNCH((lin_wgrad_kernel<A, B, C, D>), grid, block, 0, st, g)
    if (side == 2) { if (kv) LIN_WG(true, true, true, false); else LIN_WG(true, true, false, false); }
    else if (side == 1) { if (nv) LIN_WG(true, false, true, true); else LIN_WG(false, false, true, true); }
    else if (nv) { if (kv) LIN_WG(true, false, true, false); else LIN_WG(true, false, false, false); }
    else { if (kv) LIN_WG(false, false, true, false); else LIN_WG(false, false, false, false); }
#undef LIN_WG
    return mmvae_check_launch("lin_wgrad");
}

int launch_mse_tail(const float* recon, const float* x, long long n, float coef, float* gout, float* slots, hipStream_t st) {
    MMVAE_REQUIRE(recon && x && slots && n > 0, "mse_tail: bad arguments");
    MMVAE_LAUNCH(mse_tail_kernel, dim3(MMVAE_LOSS_SLOTS), dim3(256), 0, st, recon, x, n, coef, gout, slots);
    return mmvae_check_launch("mse_tail");
}

// ================================================================== the plan and its step
enum { IV_LAT_MAX = MMD_MAX_DIM, IV_C4 = 11, IV_LIN = 8 };
enum { L_EFC0 = 0, L_EFC2 = 1, L_DFC0 = 2, L_DFC2 = 3 };

struct MnistInfoVaePlan : PlanBase {
    struct W {
        float *h1, *h2, *a1, *z, *d1, *d2, *u1, *recon, *g, *du1, *dd2, *dd1, *dz_img, *dz_mmd, *dz, *da1, *dh2, *dh1, *drawn, *sums;
        void* c4[IV_C4];
        void* lin[IV_LIN];          // forward of layer l: [l], its data gradient: [4 + l]
        void* mmd;
    } w;
    long long w_off[4], b_off[4];   // the four Linear layers
    long long cw_off[4];            // encoder_conv.0, encoder_conv.2, decoder_conv.0, decoder_conv.2
    LinShape lin[4];
    C4Shape outer, inner;
};

namespace {

void add_param4(PlanBase& P, const std::string& name, std::initializer_list<int> shape) {      // every tensor starts 16-byte aligned
    P.nparams = (P.nparams + 3) / 4 * 4;
    add_param(P, name, shape);
}

void carve(MnistInfoVaePlan& P, Workspace& ws) {
    MnistInfoVaePlan::W& w = P.w;
    const size_t B = P.B, D = P.D;
    w.sums = ws.take<float>(MMVAE_LOSS_SLOTS * 16);
    w.h1 = ws.take<float>(B * 196 * 64); w.h2 = ws.take<float>(B * 6272); w.a1 = ws.take<float>(B * 1024); w.z = ws.take<float>(B * D);
    w.d1 = ws.take<float>(B * 1024); w.d2 = ws.take<float>(B * 6272); w.u1 = ws.take<float>(B * 196 * 64); w.recon = ws.take<float>(B * 784);
    w.g = ws.take<float>(B * 784); w.du1 = ws.take<float>(B * 196 * 64); w.dd2 = ws.take<float>(B * 6272); w.dd1 = ws.take<float>(B * 1024);
    w.dz_img = ws.take<float>(B * D); w.dz_mmd = ws.take<float>(B * D); w.dz = ws.take<float>(B * D); w.da1 = ws.take<float>(B * 1024);
    w.dh2 = ws.take<float>(B * 6272); w.dh1 = ws.take<float>(B * 196 * 64); w.drawn = ws.take<float>(B * D);
    // every convolution launch packs its weights into (or folds its partials from) a workspace of its own: launches of one step overlap
    const size_t co = c4_workspace_bytes(P.outer), ci = c4_workspace_bytes(P.inner);
    for (int i = 0; i < IV_C4; ++i) w.c4[i] = ws.take<char>(co > ci ? co : ci);
    for (int l = 0; l < 4; ++l) {
        const size_t f = lin_fwd_workspace_bytes(P.lin[l]), d = lin_dgrad_workspace_bytes(P.lin[l]);
        w.lin[l] = ws.take<char>(f ? f : 16);
        w.lin[4 + l] = ws.take<char>(d ? d : 16);
    }
    w.mmd = ws.take<char>(mmd_dy_workspace_bytes(P.B, P.B, P.D));
}

int step_body(MnistInfoVaePlan* Pp, const mmvae_mnist_infovae_step_io& io, int /*training*/, int do_backward, hipStream_t s) {
    MMVAE_TRY(check_bound(Pp));
    MnistInfoVaePlan& P = *Pp;
    MMVAE_REQUIRE(io.image && io.sums, "mmvae_mnist_infovae_step: image / sums must be given");
    MMVAE_REQUIRE(io.ws != nullptr && io.ws_bytes >= P.ws_bytes, "mmvae_mnist_infovae_step: workspace too small (%zu < %zu)", io.ws_bytes, P.ws_bytes);
    MMVAE_REQUIRE(aligned16(io.ws) && aligned16(io.image) && aligned16(io.true_samples) && aligned16(io.recon_image) && aligned16(io.z),
                  "mmvae_mnist_infovae_step: the workspace and every tensor must be 16-byte aligned");
    Workspace wsp(io.ws, io.ws_bytes);
    carve(P, wsp);
    MnistInfoVaePlan::W& w = P.w;
    const int B = P.B, D = P.D;
    float* const par = P.buf.params;
    float* const gr = P.buf.grads;
    float* const z = io.z ? io.z : w.z;
    float* const recon = io.recon_image ? io.recon_image : w.recon;
    const float slope = 0.1f;
    P.side_pending.clear(); P.wgrad_forked = false;
    (void)mmvae_take_stop_event();

    StepBeginArgs sb{};
    sb.zero_ptr[0] = w.sums; sb.zero_bytes[0] = MMVAE_LOSS_SLOTS * 16 * sizeof(float);
    sb.seed = io.seed; sb.step = io.step_counter;
    const float* prior = io.true_samples;
    if (!prior) { sb.normal2 = w.drawn; sb.n_normal2 = (long long)B * D; sb.normal2_stream = MMVAE_TRUE_SAMPLES_STREAM; prior = w.drawn; }
    MMVAE_TRY(launch_step_begin(sb, s));
    MMVAE_TRY(ensure_streams(P));
    // =============================== forward ===============================
    int c4 = 0;
    MMVAE_TRY(launch_c4_down(P.outer, io.image, nullptr, par + P.cw_off[0], w.h1, C4_ACT_NONE, C4_ACT_LEAKY, slope, w.c4[c4++], s));
    MMVAE_TRY(launch_c4_down(P.inner, w.h1, nullptr, par + P.cw_off[1], w.h2, C4_ACT_NONE, C4_ACT_LEAKY, slope, w.c4[c4++], s));
    MMVAE_TRY(launch_lin_fwd(P.lin[L_EFC0], w.h2, par + P.w_off[L_EFC0], par + P.b_off[L_EFC0], w.a1, w.lin[L_EFC0], s));
    MMVAE_TRY(launch_lin_fwd(P.lin[L_EFC2], w.a1, par + P.w_off[L_EFC2], par + P.b_off[L_EFC2], z, w.lin[L_EFC2], s));
    // the MMD sweep and its fold beside the decoder: z is ready, the gradient is wanted in front of encoder_fc.2's backward
    hipStream_t Sm = s;
    const bool mmd_grad = do_backward && io.lambda_mmd != 0.f;        // (a zero weight has exactly no gradient)
    if (!mmvae_serial()) { Sm = P.st_text; MMVAE_TRY(edge(P, s, Sm)); }
    MMVAE_TRY(launch_mmd_dy(prior, B, z, B, D, w.mmd, io.lambda_mmd, w.sums + MMVAE_SUM_MMD_KXX, mmd_grad ? w.dz_mmd : nullptr, Sm));
    MMVAE_TRY(launch_lin_fwd(P.lin[L_DFC0], z, par + P.w_off[L_DFC0], par + P.b_off[L_DFC0], w.d1, w.lin[L_DFC0], s));
    MMVAE_TRY(launch_lin_fwd(P.lin[L_DFC2], w.d1, par + P.w_off[L_DFC2], par + P.b_off[L_DFC2], w.d2, w.lin[L_DFC2], s));
    MMVAE_TRY(launch_c4_up(P.inner, w.d2, nullptr, par + P.cw_off[2], w.u1, C4_ACT_NONE, C4_ACT_RELU, slope, w.c4[c4++], s));
    MMVAE_TRY(launch_c4_up(P.outer, w.u1, nullptr, par + P.cw_off[3], recon, C4_ACT_NONE, C4_ACT_SIGMOID, slope, w.c4[c4++], s));
    const bool img_term = do_backward && io.lambda_x != 0.f;          // (a zero weight has exactly no gradient)
    MMVAE_TRY(launch_mse_tail(recon, io.image, (long long)B * 784, io.lambda_x / (float)((long long)B * 784), img_term ? w.g : nullptr, w.sums, s));
    if (!do_backward) {
        if (Sm != s) MMVAE_TRY(edge(P, Sm, s));
        hipLaunchKernelGGL(sum_slots_kernel, dim3(1), dim3(64), 0, s, w.sums, io.sums);
        return mmvae_check_launch("sum_slots");
    }
    // =============================== backward ===============================
    // Weight gradients only feed the optimizer: each goes to a side stream behind an edge from the kernel that made its operand.
    P.wgrad_forked = true;
    hipStream_t sw = s;
    const float* dz = nullptr;
    if (img_term) {
        // decoder_conv.2 (sigmoid's backward from the saved recon) and decoder_conv.0 (relu's from u1)
        MMVAE_TRY(wgrad_side_stream(P, s, &sw));
        MMVAE_TRY(launch_c4_wgrad(P.outer, w.g, w.u1, recon, nullptr, C4_ACT_SIGMOID, slope, gr + P.cw_off[3], w.c4[c4++], sw));
        MMVAE_TRY(launch_c4_down(P.outer, w.g, recon, par + P.cw_off[3], w.du1, C4_ACT_SIGMOID, C4_ACT_NONE, slope, w.c4[c4++], s));
        MMVAE_TRY(wgrad_side_stream(P, s, &sw));
        MMVAE_TRY(launch_c4_wgrad(P.inner, w.du1, w.d2, w.u1, nullptr, C4_ACT_RELU, slope, gr + P.cw_off[2], w.c4[c4++], sw));
        MMVAE_TRY(launch_c4_down(P.inner, w.du1, w.u1, par + P.cw_off[2], w.dd2, C4_ACT_RELU, C4_ACT_NONE, slope, w.c4[c4++], s));
        MMVAE_TRY(wgrad_side_stream(P, s, &sw));
        MMVAE_TRY(launch_lin_wgrad(P.lin[L_DFC2], w.dd2, w.d2, w.d1, gr + P.w_off[L_DFC2], gr + P.b_off[L_DFC2], sw));
        MMVAE_TRY(launch_lin_dgrad(P.lin[L_DFC2], w.dd2, w.d2, par + P.w_off[L_DFC2], w.dd1, w.lin[4 + L_DFC2], s));
        MMVAE_TRY(wgrad_side_stream(P, s, &sw));
        MMVAE_TRY(launch_lin_wgrad(P.lin[L_DFC0], w.dd1, w.d1, z, gr + P.w_off[L_DFC0], gr + P.b_off[L_DFC0], sw));
        MMVAE_TRY(launch_lin_dgrad(P.lin[L_DFC0], w.dd1, w.d1, par + P.w_off[L_DFC0], w.dz_img, w.lin[4 + L_DFC0], s));
        dz = w.dz_img;
    } else {
        // no reconstruction term: the decoder's six gradients (decoder_fc.0.weight .. decoder_conv.2.weight, one run) are exactly 0
        const long long d0 = P.w_off[L_DFC0], d1 = P.nparams;
        MMVAE_TRY(launch_fill_zero(gr + d0, (size_t)(d1 - d0) * sizeof(float), s));
    }
    if (Sm != s) MMVAE_TRY(edge(P, Sm, s));         // the MMD term's value and gradient
    if (dz && mmd_grad) {
        const float *ta = w.dz_img, *tb = w.dz_mmd;
        const int nd = B * D;
        MMVAE_LAUNCH(add2_kernel, dim3(ceil_div(nd, 256)), dim3(256), 0, s, ta, tb, nd, w.dz);
        MMVAE_TRY(mmvae_check_launch("add2"));
        dz = w.dz;
    } else if (mmd_grad) {
        dz = w.dz_mmd;
    }
    if (!dz) {      // neither term has a gradient: the encoder's six are exactly 0 too
        MMVAE_TRY(launch_fill_zero(gr, (size_t)P.w_off[L_DFC0] * sizeof(float), s));
    } else {
        MMVAE_TRY(wgrad_side_stream(P, s, &sw));
        MMVAE_TRY(launch_lin_wgrad(P.lin[L_EFC2], dz, nullptr, w.a1, gr + P.w_off[L_EFC2], gr + P.b_off[L_EFC2], sw));
        MMVAE_TRY(launch_lin_dgrad(P.lin[L_EFC2], dz, nullptr, par + P.w_off[L_EFC2], w.da1, w.lin[4 + L_EFC2], s));
        MMVAE_TRY(wgrad_side_stream(P, s, &sw));
        MMVAE_TRY(launch_lin_wgrad(P.lin[L_EFC0], w.da1, w.a1, w.h2, gr + P.w_off[L_EFC0], gr + P.b_off[L_EFC0], sw));
        MMVAE_TRY(launch_lin_dgrad(P.lin[L_EFC0], w.da1, w.a1, par + P.w_off[L_EFC0], w.dh2, w.lin[4 + L_EFC0], s));
        MMVAE_TRY(wgrad_side_stream(P, s, &sw));
        MMVAE_TRY(launch_c4_wgrad(P.inner, w.h1, w.dh2, nullptr, w.h2, C4_ACT_LEAKY, slope, gr + P.cw_off[1], w.c4[c4++], sw));
        MMVAE_TRY(launch_c4_up(P.inner, w.dh2, w.h2, par + P.cw_off[1], w.dh1, C4_ACT_LEAKY, C4_ACT_NONE, slope, w.c4[c4++], s));
        MMVAE_TRY(launch_c4_wgrad(P.outer, io.image, w.dh1, nullptr, w.h1, C4_ACT_LEAKY, slope, gr + P.cw_off[0], w.c4[c4++], s));
    }
    P.wgrad_forked = false;
    MMVAE_TRY(join_sides(P, s, s));
    hipLaunchKernelGGL(sum_slots_kernel, dim3(1), dim3(64), 0, s, w.sums, io.sums);
    return mmvae_check_launch("sum_slots");
}

}  // namespace

MnistInfoVaePlan* mnist_infovae_create(int n_latents, int batch) {
    if (n_latents < 1 || n_latents > IV_LAT_MAX) {
        mmvae_set_error("mmvae_mnist_infovae_create: n_latents = %d, need 1..%d", n_latents, (int)IV_LAT_MAX);
        return nullptr;
    }
    if (batch < 1 || batch > LIN_MAX_ROWS || batch > MMD_MAX_N) {
        mmvae_set_error("mmvae_mnist_infovae_create: batch = %d, need 1..%d", batch, (int)LIN_MAX_ROWS);
        return nullptr;
    }
    MnistInfoVaePlan* P = new MnistInfoVaePlan();
    P->D = n_latents; P->B = batch; P->no_pack = true;
    const int D = n_latents, F = LIN_PERM_P * LIN_PERM_C;
    add_param4(*P, "encoder_conv.0.weight", {64, 1, 4, 4});
    add_param4(*P, "encoder_conv.2.weight", {128, 64, 4, 4});
    add_param4(*P, "encoder_fc.0.weight", {1024, F});
    add_param4(*P, "encoder_fc.0.bias", {1024});
    add_param4(*P, "encoder_fc.2.weight", {D, 1024});
    add_param4(*P, "encoder_fc.2.bias", {D});
    add_param4(*P, "decoder_fc.0.weight", {1024, D});
    add_param4(*P, "decoder_fc.0.bias", {1024});
    add_param4(*P, "decoder_fc.2.weight", {F, 1024});
    add_param4(*P, "decoder_fc.2.bias", {F});
    add_param4(*P, "decoder_conv.0.weight", {128, 64, 4, 4});
    add_param4(*P, "decoder_conv.2.weight", {64, 1, 4, 4});
    P->nparams = (P->nparams + 3) / 4 * 4;
    const char* lname[4] = {"encoder_fc.0", "encoder_fc.2", "decoder_fc.0", "decoder_fc.2"};
    for (int l = 0; l < 4; ++l) {
        P->w_off[l] = off(*P, std::string(lname[l]) + ".weight");
        P->b_off[l] = off(*P, std::string(lname[l]) + ".bias");
    }
    const char* cname[4] = {"encoder_conv.0.weight", "encoder_conv.2.weight", "decoder_conv.0.weight", "decoder_conv.2.weight"};
    for (int i = 0; i < 4; ++i) P->cw_off[i] = off(*P, cname[i]);
    P->lin[L_EFC0] = LinShape{batch, 1024, F, LIN_ACT_LEAKY, 1, 0.1f};
    P->lin[L_EFC2] = LinShape{batch, D, 1024, LIN_ACT_NONE, 0, 0.f};
    P->lin[L_DFC0] = LinShape{batch, 1024, D, LIN_ACT_RELU, 0, 0.f};
    P->lin[L_DFC2] = LinShape{batch, F, 1024, LIN_ACT_RELU, 1, 0.f};
    P->outer = C4Shape{batch, 1, 64, 28, 28};
    P->inner = C4Shape{batch, 64, 128, 14, 14};
    for (int l = 0; l < 4; ++l)
        if (const char* e = lin_shape_error(P->lin[l])) {
            mmvae_set_error("mmvae_mnist_infovae_create: batch = %d: %s", batch, e);
            delete P;
            return nullptr;
        }
    if (!c4_shape_ok(P->outer) || !c4_shape_ok(P->inner)) {
        mmvae_set_error("mmvae_mnist_infovae_create: batch = %d is outside what the convolution kernels take", batch);
        delete P;
        return nullptr;
    }
    Workspace ws(nullptr, 0);
    carve(*P, ws);
    P->ws_bytes = P->ws_bytes_module = ws.used();
    return P;
}
void mnist_infovae_destroy(MnistInfoVaePlan* P) {
    if (!P) return;
    for (hipEvent_t e : P->events) (void)hipEventDestroy(e);
    delete P;
}
PlanBase* mnist_infovae_base(MnistInfoVaePlan* P) { return P; }
int mnist_infovae_bind(MnistInfoVaePlan* P, float* params, float* grads) {
    MMVAE_REQUIRE(P && params && grads, "mmvae_mnist_infovae_bind: null argument");
    MMVAE_REQUIRE(aligned16(params) && aligned16(grads), "mmvae_mnist_infovae_bind: params / grads must be 16-byte aligned");
    P->buf.params = params; P->buf.grads = grads;
    P->bound = true;
    return MMVAE_OK;
}
size_t mnist_infovae_step_workspace_bytes(const MnistInfoVaePlan* P) { return P ? P->ws_bytes : 0; }
int mnist_infovae_step(MnistInfoVaePlan* P, const mmvae_mnist_infovae_step_io& io, int training, int do_backward, hipStream_t s) {
    return plan_step(P, io, training, do_backward, s, step_body);
}
