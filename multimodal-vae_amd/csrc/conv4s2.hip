// 4 x 4 stride-2 convolution / transposed convolution with a fused activation: down / up (one implicit-GEMM kernel) and the weight
// gradient (partials + fold).  See conv4s2.h for the definition and the decomposition.
#include "conv4s2.h"
#include "conv_tile.h"

namespace {

constexpr int NTHR = 256;
constexpr int KC = C4_MAX_CH;            // channels staged per tap: the whole (padded) K
static_assert(KC == CT_KC && C4_KP == CT_KP && C4_TM == 64 && C4_TN == 64, "conv_tile.h is written for these stages and this tile");

__device__ __forceinline__ float c4_act(int act, float slope, float pre) {
    if (act == C4_ACT_RELU) return pre > 0.f ? pre : 0.f;
    if (act == C4_ACT_LEAKY) return pre > 0.f ? pre : slope * pre;
    if (act == C4_ACT_SIGMOID) return 1.0f / (1.0f + expf(-pre));
    return pre;
}

// the gradient in front of the activation from the upstream gradient g and the saved output y
__device__ __forceinline__ float c4_gp(int act, float slope, float g, float y) {
    if (act == C4_ACT_RELU) return y > 0.f ? g : 0.f;
    if (act == C4_ACT_LEAKY) return y > 0.f ? g : slope * g;
    if (act == C4_ACT_SIGMOID) return (g * y) * (1.0f - y);
    return g;
}

__device__ __forceinline__ float4 c4_gp4(int act, float slope, const float4& g, const float4& y) {
    return make_float4(c4_gp(act, slope, g.x, y.x), c4_gp(act, slope, g.y, y.y), c4_gp(act, slope, g.z, y.z), c4_gp(act, slope, g.w, y.w));
}

// ---- weights (Cl, Cs, 4, 4) fp32 -> bf16 [cell][Np][Kp].  up == 0: row n = l, k = s (down); up == 1: row n = s, k = l.  Padding is zero.
__global__ __launch_bounds__(NTHR) void c4_pack_kernel(const float* __restrict__ w, bf16* __restrict__ wp, int Cs, int Cl, int Np, int Kp, int up) {
    const int cell = blockIdx.y;
    const int idx = blockIdx.x * NTHR + threadIdx.x;
    if (idx >= Np * Kp) return;
    const int k = idx % Kp, n = idx / Kp;
    const int l = up ? k : n, s = up ? n : k;
    float v = 0.f;
    if (l < Cl && s < Cs) v = w[((long long)l * Cs + s) * 16 + cell];
    wp[(long long)cell * Np * Kp + idx] = f2bf(v);
}

// ---- down (UP == false) and up (UP == true).  src [positions][K] fp32, wp [cell][Np][Kp] bf16, dst [positions][N] fp32; H, W are the
//      L side's.  grid = (ceil(P / C4_TM), Np / C4_TN, UP ? 4 parity classes : 1), 4 waves as 2 x 2 of 32 x 32.
template <bool UP, bool VEC>
__global__ __launch_bounds__(NTHR) void c4_gemm_kernel(const float* __restrict__ src, const float* __restrict__ ysrc, const bf16* __restrict__ wp,
                                                       float* __restrict__ dst, int P, int H, int W, int K, int N, int Kp, int Np, int act_in,
                                                       int act_out, float slope) {
    __shared__ __attribute__((aligned(16))) bf16 As[C4_TM * A_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fq = lane >> 4;
    const int p0 = blockIdx.x * C4_TM, n0 = blockIdx.y * C4_TN;
    const int py = UP ? (int)(blockIdx.z >> 1) : 0, px = UP ? (int)(blockIdx.z & 1) : 0;
    const int SH = UP ? H : 2 * H, SW = UP ? W : 2 * W;          // the source side
    constexpr int ST = UP ? 1 : 2;                                // source positions per L position
    constexpr int TAPS = UP ? 4 : 16;

    // staging: thread -> float4 column c4 of the KC staged channels, rows r0 + 8 i
    const int c4 = tid & 31, r0 = tid >> 5;
    int by[8], bx[8], rb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int p = p0 + r0 + 8 * i;
        const int pc = p < P ? p : 0;
        const int b = pc / (H * W), rem = pc - b * (H * W);
        const int qy = rem / W, qx = rem - qy * W;
        by[i] = p < P ? ST * qy : -0x4000;       // a row past the end is outside for every tap
        bx[i] = ST * qx;
        rb[i] = (b * SH + ST * qy) * SW + ST * qx;
    }

    // the source rows of tap t, two taps ahead of their use (va / vb alternate): a tap's MFMAs are far shorter than a load's latency
    float4 va[8], vb[8];
    auto fetch = [&](int t, float4 (&v)[8]) {
        const int oy = UP ? py - (t >> 1) : (t >> 2) - 1, ox = UP ? px - (t & 1) : (t & 3) - 1;
        const int k = 4 * c4;
        const int shift = oy * SW + ox;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool ok = (unsigned)(by[i] + oy) < (unsigned)SH && (unsigned)(bx[i] + ox) < (unsigned)SW;
            const long long off = (long long)(rb[i] + shift) * K + k;
            v[i] = ok ? load4<VEC>(src + off, K - k) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (ysrc != nullptr && ok) v[i] = c4_gp4(act_in, slope, v[i], load4<VEC>(ysrc + off, K - k));
        }
    };

    // two-level sum: `acc` runs over one tap's input channels, `tot` over the taps
    f32x4 acc[2][2], tot[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = tot[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int ksteps = Kp / 32;
    auto stage = [&](int t, float4 (&v)[8]) {
        // the 8 staged rows -> bf16 LDS tile (written out, not a conv_tile.h helper: through a pointer parameter the LDS addresses come out differently and the kernel measured slower)
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<bf16x4*>(&As[(r0 + 8 * i) * A_LD + 4 * c4]) = round4(v[i]);
        // the tap's weight fragments, all k-steps, issued before the barrier so that their latency overlaps it
        const int cell = UP ? (1 - py + 2 * (t >> 1)) * 4 + (1 - px + 2 * (t & 1)) : t;
        const bf16* wrow = wp + ((long long)cell * Np + n0 + wn * 32 + fr) * Kp + 8 * fq;
        bf16x8 bfr[KC / 32][2];
#pragma unroll
        for (int ks = 0; ks < KC / 32; ++ks)
#pragma unroll
            for (int b = 0; b < 2; ++b)
                if (ks < ksteps) bfr[ks][b] = *reinterpret_cast<const bf16x8*>(wrow + (long long)b * 16 * Kp + ks * 32);
        __syncthreads();
        if (t + 2 < TAPS) fetch(t + 2, v);
#pragma unroll
        for (int ks = 0; ks < KC / 32; ++ks) {
            if (ks < ksteps) {
                bf16x8 af[2];
#pragma unroll
                for (int a = 0; a < 2; ++a) af[a] = *reinterpret_cast<const bf16x8*>(&As[(wm * 32 + a * 16 + fr) * A_LD + ks * 32 + 8 * fq]);
                mma_2x2(af, bfr[ks], acc);
            }
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                tot[a][b] += acc[a][b];
                acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        __syncthreads();
    };

    fetch(0, va);
    fetch(1, vb);
    for (int t = 0; t < TAPS; t += 2) {          // (TAPS is even)
        stage(t, va);
        stage(t + 1, vb);
    }

#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = p0 + wm * 32 + a * 16 + 4 * fq + j;
            if (p >= P) continue;
            long long orow = p;
            if (UP) {
                const int b = p / (H * W), rem = p - b * (H * W);
                const int qy = rem / W, qx = rem - qy * W;
                orow = ((long long)b * 2 * H + 2 * qy + py) * (2 * W) + 2 * qx + px;
            }
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int col = n0 + wn * 32 + b * 16 + fr;
                if (col < N) dst[orow * N + col] = c4_act(act_out, slope, tot[a][b][j]);
            }
        }
}

// ---- weight gradient, partials: workgroup (chunk, cell, channel tile) -> part[chunk][cell][l][s] = sum over the chunk's L positions
//      of bf16(L[p][l]) * bf16(S[source of p under the cell][s]).  Both operands go through LDS transposed ([channel][position]), so
//      that a lane's 8 MFMA k-elements (positions) are contiguous.
template <bool VEC_L, bool VEC_S>
__global__ __launch_bounds__(NTHR) void c4_wgrad_kernel(const float* __restrict__ lt, const float* __restrict__ st, const float* __restrict__ yl,
                                                        const float* __restrict__ ys, float* __restrict__ part, int P, int H, int W, int Cs,
                                                        int Cl, int stile_n, int chunk, int act, float slope) {
    __shared__ __attribute__((aligned(16))) bf16 Ls[64 * T_LD];
    __shared__ __attribute__((aligned(16))) bf16 Ss[64 * T_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fq = lane >> 4;
    const int ch = blockIdx.x, cell = blockIdx.y;
    const int l0 = (blockIdx.z / stile_n) * 64, s0 = (blockIdx.z % stile_n) * 64;
    const int ky = cell >> 2, kx = cell & 3;
    const int SH = 2 * H, SW = 2 * W;

    // staging: thread -> 4 channels (cg) of the position pairs pp and pp + 16
    const int cg = tid & 15, pp = tid >> 4;
    float4 vl[2][2], vs[2][2];
    auto fetch = [&](int s) {
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int p = ch * chunk + s * C4_KP + 2 * (it * 16 + pp) + e;
                const bool in = p < P;
                const int pc = in ? p : 0;
                const int b = pc / (H * W), rem = pc - b * (H * W);
                const int qy = rem / W, qx = rem - qy * W;
                const int sy = 2 * qy - 1 + ky, sx = 2 * qx - 1 + kx;
                const bool ok = in && (unsigned)sy < (unsigned)SH && (unsigned)sx < (unsigned)SW;
                const int kl = l0 + 4 * cg, ks = s0 + 4 * cg;
                const long long offl = (long long)pc * Cl + kl, offs = ((long long)(b * SH + sy) * SW + sx) * Cs + ks;
                vl[it][e] = in ? load4<VEC_L>(lt + offl, Cl - kl) : make_float4(0.f, 0.f, 0.f, 0.f);
                if (yl != nullptr && in) vl[it][e] = c4_gp4(act, slope, vl[it][e], load4<VEC_L>(yl + offl, Cl - kl));
                vs[it][e] = ok ? load4<VEC_S>(st + offs, Cs - ks) : make_float4(0.f, 0.f, 0.f, 0.f);
                if (ys != nullptr && ok) vs[it][e] = c4_gp4(act, slope, vs[it][e], load4<VEC_S>(ys + offs, Cs - ks));
            }
    };

    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the stages of this chunk that hold a position (the last chunk may be short)
    const int left = P - ch * chunk;
    const int S = ((left < chunk ? left : chunk) + C4_KP - 1) / C4_KP;
    if (S > 0) fetch(0);
    for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            put_pair(Ls, vl[it][0], vl[it][1], cg, 2 * (it * 16 + pp));
            put_pair(Ss, vs[it][0], vs[it][1], cg, 2 * (it * 16 + pp));
        }
        __syncthreads();
        if (s + 1 < S) fetch(s + 1);
        // (the k-steps are written out for the same reason as the staging of c4_gemm_kernel: as a helper this kernel ran 1 % slower)
#pragma unroll
        for (int ks = 0; ks < C4_KP / 32; ++ks) {
            bf16x8 af[2], bfr[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) af[a] = *reinterpret_cast<const bf16x8*>(&Ls[(wm * 32 + a * 16 + fr) * T_LD + ks * 32 + 8 * fq]);
#pragma unroll
            for (int b = 0; b < 2; ++b) bfr[b] = *reinterpret_cast<const bf16x8*>(&Ss[(wn * 32 + b * 16 + fr) * T_LD + ks * 32 + 8 * fq]);
            mma_2x2(af, bfr, acc);
        }
        __syncthreads();
    }

    store_partial(part + ((long long)ch * 16 + cell) * Cl * Cs, acc, l0, Cl, s0, Cs, Cs, wm, wn, fr, fq);
}

// ---- Cs == 1 on the vector unit.  With one channel on the S side the GEMM has K = 16 (down) or N = 1 (up, weight gradient): a
//      matrix tile would be padding.  The operands are rounded to bf16 as everywhere (the products are then exact in fp32) and the
//      sums run in fp32 in a fixed order per output, so the contract of conv4s2.h holds.
__device__ __forceinline__ float c4_q(float v) { return bf2f(f2bf(v)); }

// down: thread -> L position p and 4 consecutive output channels.  x [B][2H][2W], w (Cl, 1, 4, 4), dst [P][Cl]
__global__ __launch_bounds__(NTHR) void c4_down1_kernel(const float* __restrict__ x, const float* __restrict__ yx, const float* __restrict__ w,
                                                        float* __restrict__ dst, int P, int H, int W, int Cl, int groups, int act_in,
                                                        int act_out, float slope, int vec_out) {
    const long long idx = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (idx >= (long long)P * groups) return;
    const int p = (int)(idx / groups), l0 = 4 * (int)(idx - (long long)p * groups);
    const int b = p / (H * W), rem = p - b * (H * W);
    const int qy = rem / W, qx = rem - qy * W;
    const int SH = 2 * H, SW = 2 * W;
    float xq[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int sy = 2 * qy - 1 + (c >> 2), sx = 2 * qx - 1 + (c & 3);
        const bool ok = (unsigned)sy < (unsigned)SH && (unsigned)sx < (unsigned)SW;
        const long long off = ((long long)b * SH + sy) * SW + sx;
        float v = ok ? x[off] : 0.f;
        if (yx != nullptr && ok) v = c4_gp(act_in, slope, v, yx[off]);
        xq[c] = c4_q(v);
    }
    float out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float acc = 0.f;
        if (l0 + j < Cl) {
            const float* wl = w + (long long)(l0 + j) * 16;
#pragma unroll
            for (int c = 0; c < 16; ++c) acc += xq[c] * c4_q(wl[c]);
        }
        out[j] = c4_act(act_out, slope, acc);
    }
    float* o = dst + (long long)p * Cl + l0;
    if (vec_out) {
        *reinterpret_cast<float4*>(o) = make_float4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (l0 + j < Cl) o[j] = out[j];
    }
}

// up: thread -> one S pixel; its parity class picks 4 cells, each a dot product over Cl; one fp32 chain per tap, the taps summed in a
//     second one.  x [P][Cl], w (Cl, 1, 4, 4) staged through LDS as [cell][l] (rounded), dst [B][2H][2W]
template <bool VEC>
__global__ __launch_bounds__(NTHR) void c4_up1_kernel(const float* __restrict__ x, const float* __restrict__ yx, const float* __restrict__ w,
                                                      float* __restrict__ dst, int B, int H, int W, int Cl, int act_in, int act_out,
                                                      float slope) {
    __shared__ float wq[16 * C4_MAX_CH];
    for (int i = threadIdx.x; i < 16 * Cl; i += NTHR) {
        const int cell = i / Cl, l = i - cell * Cl;
        wq[i] = c4_q(w[(long long)l * 16 + cell]);
    }
    __syncthreads();
    const long long idx = (long long)blockIdx.x * NTHR + threadIdx.x;
    const int SH = 2 * H, SW = 2 * W;
    if (idx >= (long long)B * SH * SW) return;
    const int b = (int)(idx / (SH * SW)), rem = (int)(idx - (long long)b * (SH * SW));
    const int iy = rem / SW, ix = rem - iy * SW;
    const int py = iy & 1, px = ix & 1, qy = iy >> 1, qx = ix >> 1;
    float tot = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int oy = qy + py - (t >> 1), ox = qx + px - (t & 1);
        if ((unsigned)oy >= (unsigned)H || (unsigned)ox >= (unsigned)W) continue;
        const int cell = (1 - py + 2 * (t >> 1)) * 4 + (1 - px + 2 * (t & 1));
        const long long off = (((long long)b * H + oy) * W + ox) * Cl;
        const float* wc = wq + cell * Cl;
        float acc = 0.f;
        for (int l = 0; l < Cl; l += 4) {
            float4 v = load4<VEC>(x + off + l, Cl - l);
            if (yx != nullptr) v = c4_gp4(act_in, slope, v, load4<VEC>(yx + off + l, Cl - l));
            acc += c4_q(v.x) * wc[l];
            if (l + 1 < Cl) acc += c4_q(v.y) * wc[l + 1];
            if (l + 2 < Cl) acc += c4_q(v.z) * wc[l + 2];
            if (l + 3 < Cl) acc += c4_q(v.w) * wc[l + 3];
        }
        tot += acc;
    }
    dst[idx] = c4_act(act_out, slope, tot);
}

// weight gradient, partials: workgroup (chunk, 64-channel tile, kernel row ky), thread -> channel l and one of 16 position slices, the
//     row's 4 cells.  part[chunk][cell][l] as the matrix kernel writes it (Cs == 1): the slices are summed in ascending order, the fold
//     is shared.
constexpr int W1_SLICES = 16;
__global__ __launch_bounds__(64 * W1_SLICES) void c4_wgrad1_kernel(const float* __restrict__ lt, const float* __restrict__ st,
                                                                   const float* __restrict__ yl, const float* __restrict__ ys,
                                                                   float* __restrict__ part, int P, int H, int W, int Cl, int chunk, int act,
                                                                   float slope) {
    __shared__ float red[W1_SLICES][4][64];
    const int lc = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int ch = blockIdx.x, l = blockIdx.y * 64 + lc, ky = blockIdx.z;
    const int SH = 2 * H, SW = 2 * W;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const int end = min(P, (ch + 1) * chunk);
#pragma unroll 2
    for (int p = ch * chunk + q; p < end; p += W1_SLICES) {
        const int b = p / (H * W), rem = p - b * (H * W);
        const int qy = rem / W, qx = rem - qy * W;
        float lv = 0.f;
        if (l < Cl) {
            lv = lt[(long long)p * Cl + l];
            if (yl != nullptr) lv = c4_gp(act, slope, lv, yl[(long long)p * Cl + l]);
        }
        lv = c4_q(lv);
        const int sy = 2 * qy - 1 + ky;
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) {
            const int sx = 2 * qx - 1 + kx;
            const bool ok = (unsigned)sy < (unsigned)SH && (unsigned)sx < (unsigned)SW;
            const long long off = ((long long)b * SH + sy) * SW + sx;
            float sv = ok ? st[off] : 0.f;
            if (ys != nullptr && ok) sv = c4_gp(act, slope, sv, ys[off]);
            acc[kx] += lv * c4_q(sv);
        }
    }
#pragma unroll
    for (int kx = 0; kx < 4; ++kx) red[q][kx][lc] = acc[kx];
    __syncthreads();
    if (q < 4 && l < Cl) {                       // thread -> (cell 4 ky + q, channel l)
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < W1_SLICES; ++k) s += red[k][q][lc];
        part[((long long)ch * 16 + 4 * ky + q) * Cl + l] = s;
    }
}

// ---- fold: partials in ascending chunk order -> dw (Cl, Cs, 4, 4); blockIdx.y = cell (coalesced reads, one scattered write)
__global__ __launch_bounds__(NTHR) void c4_fold_kernel(const float* __restrict__ part, float* __restrict__ dw, int chunks, int plane) {
    const int idx = blockIdx.x * NTHR + threadIdx.x, cell = blockIdx.y;
    if (idx >= plane) return;
    float s = 0.f;
    for (int ch = 0; ch < chunks; ++ch) s += part[((long long)ch * 16 + cell) * plane + idx];
    dw[(long long)idx * 16 + cell] = s;
}

inline int l_positions(const C4Shape& s) { return s.B * (s.Hs / 2) * (s.Ws / 2); }
inline int chunks_of(const C4Shape& s) { return ceil_div(l_positions(s), c4_chunk(s)); }
inline size_t pack_bytes(int n, int k) { return (size_t)16 * round_up(n, C4_TN) * round_up(k, 32) * sizeof(bf16); }
inline size_t part_bytes(const C4Shape& s) { return (size_t)chunks_of(s) * 16 * s.Cl * s.Cs * sizeof(float); }

// src [L or S positions][K] -> dst [S or L positions][N] through w packed as [cell][N][K]
int run_gemm(const C4Shape& s, bool up, const float* src, const float* src_y, const float* w, float* dst, int act_in, int act_out, float slope,
             void* ws, hipStream_t st) {
    const int K = up ? s.Cl : s.Cs, N = up ? s.Cs : s.Cl;
    const int Kp = round_up(K, 32), Np = round_up(N, C4_TN), P = l_positions(s), H = s.Hs / 2, W = s.Ws / 2;
    if (s.Cs == 1) {                                    // the vector unit: reads the fp32 weights themselves, nothing to pack
        mmvae_count_flops(2.0 * P * s.Cl * 16);
        if (!up) {
            const int groups = ceil_div(s.Cl, 4);
            const long long n = (long long)P * groups;
            MMVAE_LAUNCH(c4_down1_kernel, dim3((unsigned)((n + NTHR - 1) / NTHR)), dim3(NTHR), 0, st, src, src_y, w, dst, P, H, W, s.Cl, groups,
                         act_in, act_out, slope, (s.Cl % 4 == 0 && aligned16(dst)) ? 1 : 0);
            return mmvae_check_launch("conv4s2_down1");
        }
        const long long n = (long long)P * 4;
        const dim3 g1((unsigned)((n + NTHR - 1) / NTHR));
        if (s.Cl % 4 == 0 && aligned16(src) && (src_y == nullptr || aligned16(src_y)))
            MMVAE_LAUNCH((c4_up1_kernel<true>), g1, dim3(NTHR), 0, st, src, src_y, w, dst, s.B, H, W, s.Cl, act_in, act_out, slope);
        else
            MMVAE_LAUNCH((c4_up1_kernel<false>), g1, dim3(NTHR), 0, st, src, src_y, w, dst, s.B, H, W, s.Cl, act_in, act_out, slope);
        return mmvae_check_launch("conv4s2_up1");
    }
    bf16* wp = static_cast<bf16*>(ws);
    MMVAE_LAUNCH(c4_pack_kernel, dim3(ceil_div(Np * Kp, NTHR), 16), dim3(NTHR), 0, st, w, wp, s.Cs, s.Cl, Np, Kp, up ? 1 : 0);
    MMVAE_TRY(mmvae_check_launch("conv4s2_pack"));
    const dim3 grid(ceil_div(P, C4_TM), Np / C4_TN, up ? 4 : 1);
    const bool vec = K % 4 == 0 && aligned16(src) && (src_y == nullptr || aligned16(src_y));
#define C4_GEMM(UP, VEC) MMVAE_LAUNCH((c4_gemm_kernel<UP, VEC>), grid, dim3(NTHR), 0, st, src, src_y, wp, dst, P, H, W, K, N, Kp, Np, act_in, act_out, slope)
    if (up && vec) C4_GEMM(true, true);
    else if (up) C4_GEMM(true, false);
    else if (vec) C4_GEMM(false, true);
    else C4_GEMM(false, false);
#undef C4_GEMM
    mmvae_count_flops(2.0 * P * s.Cl * (double)s.Cs * 16);
    return mmvae_check_launch(up ? "conv4s2_up" : "conv4s2_down");
}

}  // namespace

bool c4_shape_ok(const C4Shape& s) {
    return s.B >= 1 && s.Cs >= 1 && s.Cs <= C4_MAX_CH && s.Cl >= 1 && s.Cl <= C4_MAX_CH && s.Hs >= 2 && s.Hs <= C4_MAX_SIDE && s.Hs % 2 == 0 &&
           s.Ws >= 2 && s.Ws <= C4_MAX_SIDE && s.Ws % 2 == 0 && (long long)s.B * s.Hs * s.Ws <= C4_MAX_POS;
}

int c4_chunk(const C4Shape& s) {
    const int per = round_up(ceil_div(l_positions(s), C4_MAX_CHUNKS), C4_KP);
    return per > C4_CHUNK ? per : C4_CHUNK;
}

size_t c4_workspace_bytes(const C4Shape& s) {
    const size_t pack = pack_bytes(s.Cl, s.Cs), packT = pack_bytes(s.Cs, s.Cl), wgrad = part_bytes(s);
    const size_t need = pack > packT ? pack : packT;
    return need > wgrad ? need : wgrad;
}

int launch_c4_down(const C4Shape& s, const float* src, const float* src_y, const float* w, float* dst, int act_in, int act_out, float slope,
                   void* ws, hipStream_t st) {
    return run_gemm(s, false, src, src_y, w, dst, act_in, act_out, slope, ws, st);
}

int launch_c4_up(const C4Shape& s, const float* src, const float* src_y, const float* w, float* dst, int act_in, int act_out, float slope,
                 void* ws, hipStream_t st) {
    return run_gemm(s, true, src, src_y, w, dst, act_in, act_out, slope, ws, st);
}

int launch_c4_wgrad(const C4Shape& s, const float* s_side, const float* l_side, const float* y_s, const float* y_l, int act, float slope,
                    float* dw, void* ws, hipStream_t st) {
    const int P = l_positions(s), H = s.Hs / 2, W = s.Ws / 2, chunk = c4_chunk(s), chunks = chunks_of(s);
    float* part = static_cast<float*>(ws);
    const int ltile_n = ceil_div(s.Cl, 64), stile_n = ceil_div(s.Cs, 64);
    const int plane = s.Cl * s.Cs;
    if (s.Cs == 1) {
        MMVAE_LAUNCH(c4_wgrad1_kernel, dim3(chunks, ltile_n, 4), dim3(64 * W1_SLICES), 0, st, l_side, s_side, y_l, y_s, part, P, H, W, s.Cl, chunk,
                     act, slope);
        mmvae_count_flops(2.0 * P * s.Cl * 16);
        MMVAE_TRY(mmvae_check_launch("conv4s2_wgrad1"));
        MMVAE_LAUNCH(c4_fold_kernel, dim3(ceil_div(plane, NTHR), 16), dim3(NTHR), 0, st, part, dw, chunks, plane);
        return mmvae_check_launch("conv4s2_fold");
    }
    const dim3 grid(chunks, 16, ltile_n * stile_n);
    const bool vl = s.Cl % 4 == 0 && aligned16(l_side) && (y_l == nullptr || aligned16(y_l));
    const bool vs = s.Cs % 4 == 0 && aligned16(s_side) && (y_s == nullptr || aligned16(y_s));
#define C4_WGRAD(L, S) MMVAE_LAUNCH((c4_wgrad_kernel<L, S>), grid, dim3(NTHR), 0, st, l_side, s_side, y_l, y_s, part, P, H, W, s.Cs, s.Cl, stile_n, chunk, act, slope)
    if (vl && vs) C4_WGRAD(true, true);
    else if (vl) C4_WGRAD(true, false);
    else if (vs) C4_WGRAD(false, true);
    else C4_WGRAD(false, false);
#undef C4_WGRAD
    mmvae_count_flops(2.0 * P * s.Cl * (double)s.Cs * 16);
    MMVAE_TRY(mmvae_check_launch("conv4s2_wgrad"));
    MMVAE_LAUNCH(c4_fold_kernel, dim3(ceil_div(plane, NTHR), 16), dim3(NTHR), 0, st, part, dw, chunks, plane);
    return mmvae_check_launch("conv4s2_fold");
}
