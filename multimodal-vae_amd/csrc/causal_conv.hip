// Causal tap-list convolution: forward / data gradient (one implicit-GEMM kernel) and weight gradient (partials + fold).
// See causal_conv.h for the definition and the decomposition.
#include "causal_conv.h"
#include "conv_tile.h"

namespace {

constexpr int NTHR = 256;
static_assert(CC_KC == CT_KC && CC_KP == CT_KP && CC_TM == 64 && CC_TN == 64, "conv_tile.h is written for these stages and this tile");

// p = q * d + r for 0 <= p < 2^22: the float product is within one of the quotient, fixed up exactly in integers
__device__ __forceinline__ void cc_divmod(int p, int d, float rcp, int& q, int& r) {
    q = (int)((float)p * rcp);
    r = p - q * d;
    if (r < 0) { q -= 1; r += d; }
    if (r >= d) { q += 1; r -= d; }
}

// ---- weights -> bf16 [tap][Np][Kp], taps that exist only.  transposed == 0: row n = co, k = ci (forward);
//      transposed == 1: row n = ci, k = co (data gradient).  Padding is zero.
__global__ __launch_bounds__(NTHR) void cc_pack_kernel(const float* __restrict__ w, bf16* __restrict__ wp, CcTaps taps, int Cin, int Cout,
                                                       int Np, int Kp, int transposed) {
    const int t = blockIdx.y;                      // uniform: the tap table is read with scalar loads
    const int idx = blockIdx.x * NTHR + threadIdx.x;
    if (idx >= Np * Kp) return;
    const int k = idx % Kp, n = idx / Kp;
    const int co = transposed ? k : n, ci = transposed ? n : k;
    float v = 0.f;
    if (co < Cout && ci < Cin) v = w[((long long)co * Cin + ci) * taps.cells + taps.cell[t]];
    wp[(long long)t * Np * Kp + idx] = f2bf(v);
}

// ---- forward (sign = +1) and data gradient (sign = -1, in/out channels exchanged by the caller)
// x [P][Cin] fp32, wp [tap][Np][Kp] bf16, y [P][Cout] fp32.  grid = (ceil(P / CC_TM), Np / CC_TN), 4 waves as 2 x 2 of 32 x 32.
template <bool VEC>
__global__ __launch_bounds__(NTHR) void cc_gemm_kernel(const float* __restrict__ x, const bf16* __restrict__ wp, const float* __restrict__ bias,
                                                       float* __restrict__ y, CcTaps taps, int sign, int P, int H, int W, int Cin, int Cout,
                                                       int Kp, int Np, float rcpW, float rcpHW) {
    __shared__ __attribute__((aligned(16))) bf16 As[CC_TM * A_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fq = lane >> 4;
    const int p0 = blockIdx.x * CC_TM, n0 = blockIdx.y * CC_TN;

    // staging: thread -> float4 column c4 of the CC_KC staged channels, rows r0 + 8 i
    const int c4 = tid & 31, r0 = tid >> 5;
    int pi[8], pj[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int p = p0 + r0 + 8 * i;
        int b, rem, ii, jj;
        cc_divmod(p < P ? p : 0, H * W, rcpHW, b, rem);
        cc_divmod(rem, W, rcpW, ii, jj);
        pi[i] = p < P ? ii : -0x4000;            // a row past the end is outside for every tap
        pj[i] = jj;
    }
    const int spt = (Kp + CC_KC - 1) / CC_KC;    // stages per tap
    const int S = taps.n * spt;

    float4 v[8];
    auto fetch = [&](int s) {
        const int t = s / spt, kc = (s - t * spt) * CC_KC;
        const int dy = sign * taps.dy[t], dx = sign * taps.dx[t];
        const int k = kc + 4 * c4;
        const long long shift = (long long)dy * W + dx;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool ok = (unsigned)(pi[i] + dy) < (unsigned)H && (unsigned)(pj[i] + dx) < (unsigned)W;
            const long long row = (long long)(p0 + r0 + 8 * i) + shift;
            v[i] = ok ? load4<VEC>(x + row * Cin + k, Cin - k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };

    // two-level sum: `acc` runs over one tap's input channels, `tot` over the taps (shorter fp32 chains than one over taps x Cin)
    f32x4 acc[2][2], tot[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = tot[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    fetch(0);
    for (int s = 0; s < S; ++s) {
        // the 8 staged rows -> bf16 LDS tile (written out, not a conv_tile.h helper: through a pointer parameter the LDS addresses come out differently and the kernel measured slower)
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<bf16x4*>(&As[(r0 + 8 * i) * A_LD + 4 * c4]) = round4(v[i]);
        __syncthreads();
        if (s + 1 < S) fetch(s + 1);
        const int t = s / spt, kc = (s - t * spt) * CC_KC;
        const int ksteps = min(CC_KC, Kp - kc) / 32;
        const bf16* wrow = wp + ((long long)t * Np + n0 + wn * 32 + fr) * Kp + kc + 8 * fq;
        for (int ks = 0; ks < ksteps; ++ks) {
            bf16x8 af[2], bfr[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) af[a] = *reinterpret_cast<const bf16x8*>(&As[(wm * 32 + a * 16 + fr) * A_LD + ks * 32 + 8 * fq]);
#pragma unroll
            for (int b = 0; b < 2; ++b) bfr[b] = *reinterpret_cast<const bf16x8*>(wrow + (long long)b * 16 * Kp + ks * 32);
            mma_2x2(af, bfr, acc);
        }
        if (kc + CC_KC >= Kp) {                  // the tap's last stage
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    tot[a][b] += acc[a][b];
                    acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
        }
        __syncthreads();
    }

#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int col = n0 + wn * 32 + b * 16 + fr;
        if (col >= Cout) continue;
        const float bv = bias ? bias[col] : 0.f;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int p = p0 + wm * 32 + a * 16 + 4 * fq + j;
                if (p < P) y[(long long)p * Cout + col] = tot[a][b][j] + bv;
            }
    }
}

// ---- weight gradient, partials: workgroup (chunk, tap, channel tile) -> part[chunk][tap][co][ci] = sum over the chunk's
//      positions of bf16(g[p][co]) * bf16(x[p + offset_t][ci]).  Both operands go through LDS transposed ([channel][position]),
//      so that a lane's 8 MFMA k-elements (positions) are contiguous.
template <bool VEC_G, bool VEC_X>
__global__ __launch_bounds__(NTHR) void cc_wgrad_kernel(const float* __restrict__ g, const float* __restrict__ x, float* __restrict__ part,
                                                        CcTaps taps, int P, int H, int W, int Cin, int Cout, int cit_n, float rcpW,
                                                        float rcpHW) {
    __shared__ __attribute__((aligned(16))) bf16 Gs[64 * T_LD];
    __shared__ __attribute__((aligned(16))) bf16 Xs[64 * T_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fq = lane >> 4;
    const int chunk = blockIdx.x, t = blockIdx.y;
    const int co0 = (blockIdx.z / cit_n) * 64, ci0 = (blockIdx.z % cit_n) * 64;
    const int dy = taps.dy[t], dx = taps.dx[t];
    const long long shift = (long long)dy * W + dx;

    // staging: thread -> 4 channels (cg) of the position pairs pp and pp + 16
    const int cg = tid & 15, pp = tid >> 4;
    float4 vg[2][2], vx[2][2];
    auto fetch = [&](int s) {
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int p = chunk * CC_CHUNK + s * CC_KP + 2 * (it * 16 + pp) + e;
                const bool in = p < P;
                int b, rem, ii, jj;
                cc_divmod(in ? p : 0, H * W, rcpHW, b, rem);
                cc_divmod(rem, W, rcpW, ii, jj);
                const bool ok = in && (unsigned)(ii + dy) < (unsigned)H && (unsigned)(jj + dx) < (unsigned)W;
                const int kg = co0 + 4 * cg, kx = ci0 + 4 * cg;
                vg[it][e] = in ? load4<VEC_G>(g + (long long)p * Cout + kg, Cout - kg) : make_float4(0.f, 0.f, 0.f, 0.f);
                vx[it][e] = ok ? load4<VEC_X>(x + ((long long)p + shift) * Cin + kx, Cin - kx) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
    };

    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    constexpr int S = CC_CHUNK / CC_KP;
    fetch(0);
    for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            put_pair(Gs, vg[it][0], vg[it][1], cg, 2 * (it * 16 + pp));
            put_pair(Xs, vx[it][0], vx[it][1], cg, 2 * (it * 16 + pp));
        }
        __syncthreads();
        if (s + 1 < S) fetch(s + 1);
        // (the k-steps are written out for the same reason as the staging of cc_gemm_kernel: as a helper this kernel ran 1 % slower)
#pragma unroll
        for (int ks = 0; ks < CC_KP / 32; ++ks) {
            bf16x8 af[2], bfr[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) af[a] = *reinterpret_cast<const bf16x8*>(&Gs[(wm * 32 + a * 16 + fr) * T_LD + ks * 32 + 8 * fq]);
#pragma unroll
            for (int b = 0; b < 2; ++b) bfr[b] = *reinterpret_cast<const bf16x8*>(&Xs[(wn * 32 + b * 16 + fr) * T_LD + ks * 32 + 8 * fq]);
            mma_2x2(af, bfr, acc);
        }
        __syncthreads();
    }

    store_partial(part + ((long long)chunk * taps.n + t) * Cout * Cin, acc, co0, Cout, ci0, Cin, Cin, wm, wn, fr, fq);
}

// ---- bias gradient, partials: dbp[chunk][co] = sum over the chunk's positions of g[p][co], fp32, fixed order
__global__ __launch_bounds__(NTHR) void cc_dbias_kernel(const float* __restrict__ g, float* __restrict__ dbp, int P, int Cout) {
    __shared__ float red[4][64];
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int chunk = blockIdx.x, co = blockIdx.y * 64 + c;
    float s = 0.f;
    if (co < Cout)
        for (int lp = q; lp < CC_CHUNK; lp += 4) {
            const int p = chunk * CC_CHUNK + lp;
            if (p < P) s += g[(long long)p * Cout + co];
        }
    red[q][c] = s;
    __syncthreads();
    if (q == 0 && co < Cout) dbp[(long long)chunk * Cout + co] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

// ---- fold: partials in ascending chunk order -> dw (Cout, Cin, kh, kw), cells in no tap 0; dbp -> db
__global__ __launch_bounds__(NTHR) void cc_fold_kernel(const float* __restrict__ part, const float* __restrict__ dbp, float* __restrict__ dw,
                                                       float* __restrict__ db, CcTaps taps, int chunks, int Cin, int Cout) {
    // blockIdx.y < taps.n: that tap's plane (coalesced reads, one scattered write); above: one kernel cell, zeroed if in no tap
    const long long idx = (long long)blockIdx.x * NTHR + threadIdx.x;
    const long long plane = (long long)Cout * Cin;
    const int yy = blockIdx.y;
    if (dw && idx < plane) {
        if (yy < taps.n) {
            float s = 0.f;
            for (int ch = 0; ch < chunks; ++ch) s += part[((long long)ch * taps.n + yy) * plane + idx];
            dw[idx * taps.cells + taps.cell[yy]] = s;
        } else if (taps.tap_of_cell[yy - taps.n] < 0) {
            dw[idx * taps.cells + (yy - taps.n)] = 0.f;
        }
    }
    if (db && yy == 0 && idx < Cout) {
        float s = 0.f;
        for (int ch = 0; ch < chunks; ++ch) s += dbp[(long long)ch * Cout + idx];
        db[idx] = s;
    }
}

inline long long positions(const CcShape& s) { return (long long)s.B * s.H * s.W; }
inline int chunks_of(const CcShape& s) { return (int)((positions(s) + CC_CHUNK - 1) / CC_CHUNK); }
inline size_t pack_bytes(int n_taps, int n, int k) { return (size_t)n_taps * round_up(n, CC_TN) * round_up(k, 32) * sizeof(bf16); }
inline size_t part_bytes(const CcShape& s, int n_taps) { return (size_t)chunks_of(s) * n_taps * s.Cout * s.Cin * sizeof(float); }

// x [P][K] -> y [P][N] through w packed as [tap][N][K]
int run_gemm(const CcShape& s, const CcTaps& t, const float* x, const float* w, const float* bias, float* y, void* ws, int sign, hipStream_t st) {
    const int K = sign > 0 ? s.Cin : s.Cout, N = sign > 0 ? s.Cout : s.Cin;
    const int Kp = round_up(K, 32), Np = round_up(N, CC_TN), P = (int)positions(s);
    bf16* wp = static_cast<bf16*>(ws);
    MMVAE_LAUNCH(cc_pack_kernel, dim3(ceil_div(Np * Kp, NTHR), t.n), dim3(NTHR), 0, st, w, wp, t, s.Cin, s.Cout, Np, Kp, sign > 0 ? 0 : 1);
    MMVAE_TRY(mmvae_check_launch("causal_conv_pack"));
    const dim3 grid(ceil_div(P, CC_TM), Np / CC_TN);
    const float rw = 1.0f / (float)s.W, rhw = 1.0f / (float)(s.H * s.W);
    if (K % 4 == 0 && aligned16(x))
        MMVAE_LAUNCH((cc_gemm_kernel<true>), grid, dim3(NTHR), 0, st, x, wp, bias, y, t, sign, P, s.H, s.W, K, N, Kp, Np, rw, rhw);
    else
        MMVAE_LAUNCH((cc_gemm_kernel<false>), grid, dim3(NTHR), 0, st, x, wp, bias, y, t, sign, P, s.H, s.W, K, N, Kp, Np, rw, rhw);
    mmvae_count_flops(2.0 * P * N * (double)K * t.n);
    return mmvae_check_launch("causal_conv_gemm");
}

}  // namespace

int cc_make_taps(const char* what, const CcShape& s, const int* taps, int n_taps, CcTaps* out) {
    MMVAE_REQUIRE(s.B >= 1 && s.H >= 1 && s.W >= 1 && positions(s) <= CC_MAX_POS, "%s: batch = %d, height = %d, width = %d: need each >= 1 and "
                  "batch * height * width <= %d", what, s.B, s.H, s.W, (int)CC_MAX_POS);
    MMVAE_REQUIRE(s.Cin >= 1 && s.Cin <= CC_MAX_CH && s.Cout >= 1 && s.Cout <= CC_MAX_CH, "%s: Cin = %d, Cout = %d, need 1..%d", what, s.Cin,
                  s.Cout, (int)CC_MAX_CH);
    MMVAE_REQUIRE(s.kh >= 1 && s.kw >= 1 && s.kh * s.kw <= CC_MAX_CELLS, "%s: kernel %d x %d, need 1..%d cells", what, s.kh, s.kw,
                  (int)CC_MAX_CELLS);
    MMVAE_REQUIRE(taps && n_taps >= 1 && n_taps <= CC_MAX_TAPS, "%s: %d taps, need 1..%d", what, n_taps, (int)CC_MAX_TAPS);
    CcTaps t;
    t.n = n_taps; t.cells = s.kh * s.kw;
    for (int c = 0; c < CC_MAX_CELLS; ++c) t.tap_of_cell[c] = -1;
    for (int k = 0; k < CC_MAX_TAPS; ++k) t.dy[k] = t.dx[k] = t.cell[k] = 0;
    for (int k = 0; k < n_taps; ++k) {
        const int r = taps[4 * k], c = taps[4 * k + 1], dy = taps[4 * k + 2], dx = taps[4 * k + 3];
        MMVAE_REQUIRE(r >= 0 && r < s.kh && c >= 0 && c < s.kw, "%s: tap %d names cell (%d, %d) of a %d x %d kernel", what, k, r, c, s.kh, s.kw);
        MMVAE_REQUIRE(dy >= -CC_MAX_OFF && dy <= CC_MAX_OFF && dx >= -CC_MAX_OFF && dx <= CC_MAX_OFF,
                      "%s: tap %d has offset (%d, %d), need |offset| <= %d", what, k, dy, dx, (int)CC_MAX_OFF);
        MMVAE_REQUIRE(t.tap_of_cell[r * s.kw + c] < 0, "%s: cell (%d, %d) appears in two taps", what, r, c);
        t.tap_of_cell[r * s.kw + c] = (signed char)k;
        t.cell[k] = (signed char)(r * s.kw + c); t.dy[k] = (signed char)dy; t.dx[k] = (signed char)dx;
    }
    *out = t;
    return MMVAE_OK;
}

size_t cc_workspace_bytes(const CcShape& s, int n_taps) {
    size_t pack = pack_bytes(n_taps, s.Cout, s.Cin), packT = pack_bytes(n_taps, s.Cin, s.Cout);
    size_t wgrad = part_bytes(s, n_taps) + (size_t)chunks_of(s) * s.Cout * sizeof(float);
    size_t need = pack > packT ? pack : packT;
    return need > wgrad ? need : wgrad;
}

int launch_cc_forward(const CcShape& s, const CcTaps& t, const float* x, const float* w, const float* bias, float* y, void* ws, hipStream_t st) {
    return run_gemm(s, t, x, w, bias, y, ws, +1, st);
}

int launch_cc_backward_data(const CcShape& s, const CcTaps& t, const float* g, const float* w, float* dx, void* ws, hipStream_t st) {
    return run_gemm(s, t, g, w, nullptr, dx, ws, -1, st);
}

int launch_cc_backward_weight(const CcShape& s, const CcTaps& t, const float* g, const float* x, float* dw, float* db, void* ws, hipStream_t st) {
    const int P = (int)positions(s), chunks = chunks_of(s);
    float* part = static_cast<float*>(ws);
    float* dbp = reinterpret_cast<float*>(static_cast<char*>(ws) + part_bytes(s, t.n));
    if (dw) {
        const int cot_n = ceil_div(s.Cout, 64), cit_n = ceil_div(s.Cin, 64);
        const dim3 grid(chunks, t.n, cot_n * cit_n);
        const float rw = 1.0f / (float)s.W, rhw = 1.0f / (float)(s.H * s.W);
        const bool vg = s.Cout % 4 == 0 && aligned16(g), vx = s.Cin % 4 == 0 && aligned16(x);
#define CC_WGRAD(G, X) MMVAE_LAUNCH((cc_wgrad_kernel<G, X>), grid, dim3(NTHR), 0, st, g, x, part, t, P, s.H, s.W, s.Cin, s.Cout, cit_n, rw, rhw)
        if (vg && vx) CC_WGRAD(true, true);
        else if (vg) CC_WGRAD(true, false);
        else if (vx) CC_WGRAD(false, true);
        else CC_WGRAD(false, false);
#undef CC_WGRAD
        mmvae_count_flops(2.0 * P * s.Cout * (double)s.Cin * t.n);
        MMVAE_TRY(mmvae_check_launch("causal_conv_wgrad"));
    }
    if (db) {
        MMVAE_LAUNCH(cc_dbias_kernel, dim3(chunks, ceil_div(s.Cout, 64)), dim3(NTHR), 0, st, g, dbp, P, s.Cout);
        MMVAE_TRY(mmvae_check_launch("causal_conv_dbias"));
    }
    if (!dw && !db) return MMVAE_OK;
    // with dw: one grid row per tap and per kernel cell over the Cout x Cin plane (>= Cout); db alone: Cout threads of row 0
    const long long elems = dw ? (long long)s.Cout * s.Cin : s.Cout;
    MMVAE_LAUNCH(cc_fold_kernel, dim3((unsigned)((elems + NTHR - 1) / NTHR), dw ? t.n + t.cells : 1), dim3(NTHR), 0, st, part, dbp, dw, db, t, chunks, s.Cin, s.Cout);
    return mmvae_check_launch("causal_conv_fold");
}
