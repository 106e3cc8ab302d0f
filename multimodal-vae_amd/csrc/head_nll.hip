// PixelCNN output head fused with its cross entropy: pack, forward / dh (one kernel template), dw / db partials, fold.
// See head_nll.h for the definition and the decomposition.
#include "head_nll.h"
#include <math.h>

namespace {

constexpr int NTHR = 256;
constexpr int T_LD = 64 + 8;             // bf16 per LDS row of a 64-wide tile: 144 B, a multiple of 16 B off the bank period
constexpr float NEG_BIG = -3.0e38f;      // start of the running maximum: finite, so that no inf - inf can arise


struct HnDims {
    int P, HW, C, hid, V;
    int Vp, Kp, Hp, tiles, Np;           // levels padded to HN_TN, hid padded to 32, hid padded to the dh / dw column blocks, Vp / HN_TN, C * Vp
};

// ---- weights -> bf16, channel-major rows n' = c * Vp + v: wp [n'][Kp] and wT [c][Hp][Vp].  Padding is zero.
__global__ __launch_bounds__(NTHR) void hn_pack_kernel(const float* __restrict__ w, bf16* __restrict__ wp, bf16* __restrict__ wT, HnDims d) {
    const int idx = blockIdx.x * NTHR + threadIdx.x;
    if (idx < d.Np * d.Kp) {
        const int k = idx % d.Kp, n = idx / d.Kp;
        const int c = n / d.Vp, v = n - c * d.Vp;
        float val = 0.f;
        if (v < d.V && k < d.hid) val = w[(long long)(v * d.C + c) * d.hid + k];
        wp[idx] = f2bf(val);
    }
    if (idx < d.C * d.Hp * d.Vp) {
        const int v = idx % d.Vp, r = idx / d.Vp;
        const int c = r / d.Hp, k = r - c * d.Hp;
        float val = 0.f;
        if (v < d.V && k < d.hid) val = w[(long long)(v * d.C + c) * d.hid + k];
        wT[idx] = f2bf(val);
    }
}

// 8 consecutive channels k .. k + 7 of position p as an MFMA A fragment; zeros past the end of either (hid is a multiple of 8)
__device__ __forceinline__ bf16x8 hn_afrag(const float* __restrict__ h, long long p, int P, int hid, int k) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (p < P && k < hid) {
        const float4* src = reinterpret_cast<const float4*>(h + p * hid + k);
        a = src[0];
        b = src[1];
    }
    bf16x8 o;
    o[0] = f2bf(a.x); o[1] = f2bf(a.y); o[2] = f2bf(a.z); o[3] = f2bf(a.w);
    o[4] = f2bf(b.x); o[5] = f2bf(b.y); o[6] = f2bf(b.z); o[7] = f2bf(b.w);
    return o;
}

// 16 positions x 64 levels of logits without the bias: wtile = the 64 packed rows of the tile
template <int KS>
__device__ __forceinline__ void hn_logits(const bf16x8 (&af)[KS], const bf16* __restrict__ wtile, int Kp, int fr, int fq, f32x4 (&acc)[4]) {
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ksteps = Kp / 32;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        if (ks < ksteps) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const bf16x8 bfr = *reinterpret_cast<const bf16x8*>(wtile + (long long)(b * 16 + fr) * Kp + ks * 32 + 8 * fq);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], bfr, acc[b], 0, 0, 0);
            }
        }
    }
}

// reductions over the 16 lanes that hold one row of a C fragment
__device__ __forceinline__ float row_max(float v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- forward (BWD = false: nll, lse) and dh (BWD = true: from the saved lse and g).  grid = ceil(P / HN_TM); wave w owns the
//      positions 16 w .. 16 w + 15 of the workgroup's 64.  C fragment: column (level) = lane & 15, row (position) = 4 (lane >> 4) + reg.
template <int KS, int NB, bool BWD>
__global__ __launch_bounds__(NTHR) void hn_rows_kernel(const float* __restrict__ h, const bf16* __restrict__ wp, const bf16* __restrict__ wT,
                                                       const float* __restrict__ bias, const long long* __restrict__ target,
                                                       float* __restrict__ nll, float* __restrict__ lse_out, const float* __restrict__ lse_in,
                                                       const float* __restrict__ g, float* __restrict__ dh, HnDims d) {
    __shared__ __attribute__((aligned(16))) bf16 Ds[BWD ? HN_TM * T_LD : 8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const long long p0 = (long long)blockIdx.x * HN_TM + wave * 16;

    bf16x8 af[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) af[ks] = hn_afrag(h, p0 + fr, d.P, d.hid, ks * 32 + 8 * fq);

    bool valid[4];
    long long base[4];                       // element (b, 0, i, j) of the (B, C, H, W) tensors
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long p = p0 + 4 * fq + j;
        valid[j] = p < d.P;
        const int pp = valid[j] ? (int)p : 0;
        const int b = pp / d.HW, rem = pp - b * d.HW;
        base[j] = (long long)b * d.C * d.HW + rem;
    }

    f32x4 dacc[BWD ? NB : 1];
#pragma unroll
    for (int nb = 0; nb < (BWD ? NB : 1); ++nb) dacc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int c = 0; c < d.C; ++c) {
        long long tg[4];
        float m[4], s[4], tl[4], ls[4], gg[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long e = base[j] + (long long)c * d.HW;
            tg[j] = valid[j] ? target[e] : 0;
            m[j] = NEG_BIG; s[j] = 0.f; tl[j] = 0.f;
            ls[j] = (BWD && valid[j]) ? lse_in[e] : 0.f;
            gg[j] = (BWD && valid[j]) ? g[e] : 0.f;
        }
        for (int t = 0; t < d.tiles; ++t) {
            f32x4 acc[4];
            hn_logits<KS>(af, wp + (long long)(c * d.Vp + t * HN_TN) * d.Kp, d.Kp, fr, fq, acc);
            bool ok[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int v = t * HN_TN + b * 16 + fr;
                ok[b] = v < d.V;
                const float bv = ok[b] ? bias[v * d.C + c] : 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[b][j] += bv;
            }
            if constexpr (!BWD) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float tm = NEG_BIG;
#pragma unroll
                    for (int b = 0; b < 4; ++b) tm = ok[b] ? fmaxf(tm, acc[b][j]) : tm;
                    const float mn = fmaxf(m[j], row_max(tm));
                    float sum = 0.f, hit = 0.f;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int v = t * HN_TN + b * 16 + fr;
                        sum += ok[b] ? expf(acc[b][j] - mn) : 0.f;
                        hit += (ok[b] && (long long)v == tg[j]) ? acc[b][j] : 0.f;
                    }
                    s[j] = s[j] * expf(m[j] - mn) + row_sum(sum);
                    m[j] = mn;
                    tl[j] += row_sum(hit);
                }
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int v = t * HN_TN + b * 16 + fr;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float dv = 0.f;
                        if (ok[b] && valid[j]) dv = gg[j] * (expf(acc[b][j] - ls[j]) - ((long long)v == tg[j] ? 1.f : 0.f));
                        Ds[(wave * 16 + 4 * fq + j) * T_LD + b * 16 + fr] = f2bf(dv);
                    }
                }
                __syncthreads();
#pragma unroll
                for (int ks = 0; ks < HN_TN / 32; ++ks) {
                    const bf16x8 a = *reinterpret_cast<const bf16x8*>(&Ds[(wave * 16 + fr) * T_LD + ks * 32 + 8 * fq]);
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) {
                        if (nb * 16 < d.hid) {
                            const bf16x8 bfr = *reinterpret_cast<const bf16x8*>(wT + (long long)(c * d.Hp + nb * 16 + fr) * d.Vp + t * HN_TN +
                                                                                ks * 32 + 8 * fq);
                            dacc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfr, dacc[nb], 0, 0, 0);
                        }
                    }
                }
                __syncthreads();
            }
        }
        if constexpr (!BWD) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (fr == 0 && valid[j]) {
                    const long long e = base[j] + (long long)c * d.HW;
                    const float lse = m[j] + logf(s[j]);
                    const bool in = tg[j] >= 0 && tg[j] < d.V;
                    nll[e] = in ? lse - tl[j] : __builtin_nanf("");
                    if (lse_out) lse_out[e] = lse;
                }
            }
        }
    }
    if constexpr (BWD) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int ch = nb * 16 + fr;
            if (ch < d.hid) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (valid[j]) dh[(p0 + 4 * fq + j) * d.hid + ch] = dacc[nb][j];
            }
        }
    }
}

// ---- dw / db partials.  grid = (chunks, C * tiles): workgroup (chunk, level tile n0 .. n0 + 63 of channel c) recomputes l and d for its
//      chunk, 64 positions at a time, and accumulates part[chunk][n'][k] = sum_p bf16(d[p][n']) bf16(h[p][k]), dbp[chunk][n'] = sum_p d.
//      Both MFMA operands go through LDS transposed ([level][position], [channel][position]): a lane's 8 k-elements are positions.
template <int KS, int NB>
__global__ __launch_bounds__(NTHR) void hn_dw_kernel(const float* __restrict__ h, const bf16* __restrict__ wp, const float* __restrict__ bias,
                                                     const long long* __restrict__ target, const float* __restrict__ lse_in,
                                                     const float* __restrict__ g, float* __restrict__ part, float* __restrict__ dbp, HnDims d) {
    __shared__ __attribute__((aligned(16))) bf16 HsT[NB * 16 * T_LD];
    __shared__ __attribute__((aligned(16))) bf16 DsT[HN_TN * T_LD];
    __shared__ float red[4][HN_TN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int chunk = blockIdx.x;
    const int c = blockIdx.y / d.tiles, t = blockIdx.y - c * d.tiles;
    const int n0 = c * d.Vp + t * HN_TN;
    const bf16* wtile = wp + (long long)n0 * d.Kp;

    bool ok[4];
    float bv[4], dbs[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int v = t * HN_TN + b * 16 + fr;
        ok[b] = v < d.V;
        bv[b] = ok[b] ? bias[v * d.C + c] : 0.f;
        dbs[b] = 0.f;
    }
    f32x4 dacc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) dacc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

    constexpr int S = HN_CHUNK / 64;
    for (int s = 0; s < S; ++s) {
        const long long pb = (long long)chunk * HN_CHUNK + s * 64;
        // h -> HsT: thread item = 4 channels (cg) of the position pair pp
        for (int it = tid; it < NB * 4 * 32; it += NTHR) {
            const int cg = it % (NB * 4), pp = it / (NB * 4);
            const int k = 4 * cg;
            const long long p = pb + 2 * pp;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b2 = a;
            if (k < d.hid) {
                if (p < d.P) a = *reinterpret_cast<const float4*>(h + p * d.hid + k);
                if (p + 1 < d.P) b2 = *reinterpret_cast<const float4*>(h + (p + 1) * d.hid + k);
            }
            const float av[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b2.x, b2.y, b2.z, b2.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bf16x2 pr;
                pr[0] = f2bf(av[e]); pr[1] = f2bf(bw[e]);
                *reinterpret_cast<bf16x2*>(&HsT[(k + e) * T_LD + 2 * pp]) = pr;
            }
        }
        bf16x8 af[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) af[ks] = hn_afrag(h, pb + wave * 16 + fr, d.P, d.hid, ks * 32 + 8 * fq);
        f32x4 acc[4];
        hn_logits<KS>(af, wtile, d.Kp, fr, fq, acc);

        long long tg[4];
        float ls[4], gg[4];
        bool valid[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long p = pb + wave * 16 + 4 * fq + j;
            valid[j] = p < d.P;
            const int pp = valid[j] ? (int)p : 0;
            const int b = pp / d.HW, rem = pp - b * d.HW;
            const long long e = ((long long)b * d.C + c) * d.HW + rem;
            tg[j] = valid[j] ? target[e] : 0;
            ls[j] = valid[j] ? lse_in[e] : 0.f;
            gg[j] = valid[j] ? g[e] : 0.f;
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int v = t * HN_TN + b * 16 + fr;
            bf16x4 pk;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float dv = 0.f;
                if (ok[b] && valid[j]) dv = gg[j] * (expf(acc[b][j] + bv[b] - ls[j]) - ((long long)v == tg[j] ? 1.f : 0.f));
                dbs[b] += dv;
                pk[j] = f2bf(dv);
            }
            *reinterpret_cast<bf16x4*>(&DsT[(b * 16 + fr) * T_LD + wave * 16 + 4 * fq]) = pk;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(&DsT[(wave * 16 + fr) * T_LD + ks * 32 + 8 * fq]);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                if (nb * 16 < d.hid) {
                    const bf16x8 bfr = *reinterpret_cast<const bf16x8*>(&HsT[(nb * 16 + fr) * T_LD + ks * 32 + 8 * fq]);
                    dacc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfr, dacc[nb], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // dw partial: row (level) = 16 wave + 4 fq + reg, column (channel) = 16 nb + fr
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int ch = nb * 16 + fr;
        if (ch < d.hid) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                part[((long long)chunk * d.Np + n0 + wave * 16 + 4 * fq + j) * d.hid + ch] = dacc[nb][j];
        }
    }
    // db partial: the lanes of one column, then the 4 waves, in a fixed order
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        float v = dbs[b];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (fq == 0) red[wave][b * 16 + fr] = v;
    }
    __syncthreads();
    if (tid < HN_TN) dbp[(long long)chunk * d.Np + n0 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// ---- fold: partials in ascending chunk order -> dw (V * C, hid), db (V * C), rows back in the order v * C + c
__global__ __launch_bounds__(NTHR) void hn_fold_kernel(const float* __restrict__ part, const float* __restrict__ dbp, float* __restrict__ dw,
                                                       float* __restrict__ db, int chunks, HnDims d) {
    const int idx = blockIdx.x * NTHR + threadIdx.x;
    const int N = d.V * d.C;
    if (dw && idx < N * d.hid) {
        const int n = idx / d.hid, k = idx - n * d.hid;
        const int v = n / d.C, c = n - v * d.C;
        const long long row = (long long)c * d.Vp + v;
        float s = 0.f;
        for (int ch = 0; ch < chunks; ++ch) s += part[((long long)ch * d.Np + row) * d.hid + k];
        dw[idx] = s;
    }
    if (db && idx < N) {
        const int v = idx / d.C, c = idx - v * d.C;
        const long long row = (long long)c * d.Vp + v;
        float s = 0.f;
        for (int ch = 0; ch < chunks; ++ch) s += dbp[(long long)ch * d.Np + row];
        db[idx] = s;
    }
}

inline size_t align16(size_t v) { return (v + 15) / 16 * 16; }

HnDims dims_of(const HnShape& s) {
    HnDims d;
    d.P = s.B * s.H * s.W; d.HW = s.H * s.W; d.C = s.C; d.hid = s.hid; d.V = s.V;
    d.Vp = round_up(s.V, HN_TN); d.Kp = round_up(s.hid, 32); d.Hp = s.hid <= 128 ? 128 : 256;
    d.tiles = d.Vp / HN_TN; d.Np = s.C * d.Vp;
    return d;
}
inline int chunks_of(const HnDims& d) { return ceil_div(d.P, HN_CHUNK); }

struct HnWs { bf16 *wp, *wT; float *part, *dbp; size_t bytes; };
HnWs carve(const HnDims& d, void* ws) {
    const uintptr_t base = reinterpret_cast<uintptr_t>(ws);
    size_t o = 0;
    HnWs r;
    r.wp = reinterpret_cast<bf16*>(base + o); o += align16((size_t)d.Np * d.Kp * sizeof(bf16));
    r.wT = reinterpret_cast<bf16*>(base + o); o += align16((size_t)d.C * d.Hp * d.Vp * sizeof(bf16));
    r.part = reinterpret_cast<float*>(base + o); o += align16((size_t)chunks_of(d) * d.Np * d.hid * sizeof(float));
    r.dbp = reinterpret_cast<float*>(base + o); o += align16((size_t)chunks_of(d) * d.Np * sizeof(float));
    r.bytes = o;
    return r;
}

int pack(const HnDims& d, const HnWs& k, const float* w, hipStream_t st) {
    const int elems = max(d.Np * d.Kp, d.C * d.Hp * d.Vp);
    MMVAE_LAUNCH(hn_pack_kernel, dim3(ceil_div(elems, NTHR)), dim3(NTHR), 0, st, w, k.wp, k.wT, d);
    return mmvae_check_launch("head_nll_pack");
}

}  // namespace

bool hn_shape_ok(const HnShape& s) {
    return s.B >= 1 && s.H >= 1 && s.W >= 1 && (long long)s.B * s.H * s.W <= HN_MAX_POS && (s.C == 1 || s.C == 3) && s.hid >= 8 &&
           s.hid <= HN_MAX_HID && s.hid % 8 == 0 && s.V >= 2 && s.V <= HN_MAX_V;
}

size_t hn_workspace_bytes(const HnShape& s) { return carve(dims_of(s), nullptr).bytes; }

int launch_hn_forward(const HnShape& s, const float* h, const float* w, const float* bias, const long long* target, float* nll, float* lse,
                      void* ws, hipStream_t st) {
    const HnDims d = dims_of(s);
    const HnWs k = carve(d, ws);
    MMVAE_TRY(pack(d, k, w, st));
    const dim3 grid(ceil_div(d.P, HN_TM));
    if (d.hid <= 128)
        MMVAE_LAUNCH((hn_rows_kernel<4, 8, false>), grid, dim3(NTHR), 0, st, h, k.wp, k.wT, bias, target, nll, lse, nullptr, nullptr, nullptr, d);
    else
        MMVAE_LAUNCH((hn_rows_kernel<8, 16, false>), grid, dim3(NTHR), 0, st, h, k.wp, k.wT, bias, target, nll, lse, nullptr, nullptr, nullptr, d);
    mmvae_count_flops(2.0 * d.P * (double)d.V * d.C * d.hid);
    return mmvae_check_launch("head_nll_forward");
}

int launch_hn_backward(const HnShape& s, const float* h, const float* w, const float* bias, const long long* target, const float* lse,
                       const float* g, float* dh, float* dw, float* db, void* ws, hipStream_t st) {
    if (!dh && !dw && !db) return MMVAE_OK;
    const HnDims d = dims_of(s);
    const HnWs k = carve(d, ws);
    MMVAE_TRY(pack(d, k, w, st));
    if (dh) {
        const dim3 grid(ceil_div(d.P, HN_TM));
        if (d.hid <= 128)
            MMVAE_LAUNCH((hn_rows_kernel<4, 8, true>), grid, dim3(NTHR), 0, st, h, k.wp, k.wT, bias, target, nullptr, nullptr, lse, g, dh, d);
        else
            MMVAE_LAUNCH((hn_rows_kernel<8, 16, true>), grid, dim3(NTHR), 0, st, h, k.wp, k.wT, bias, target, nullptr, nullptr, lse, g, dh, d);
        mmvae_count_flops(4.0 * d.P * (double)d.V * d.C * d.hid);
        MMVAE_TRY(mmvae_check_launch("head_nll_dh"));
    }
    if (dw || db) {
        const int chunks = chunks_of(d);
        const dim3 grid(chunks, d.C * d.tiles);
        if (d.hid <= 128)
            MMVAE_LAUNCH((hn_dw_kernel<4, 8>), grid, dim3(NTHR), 0, st, h, k.wp, bias, target, lse, g, k.part, k.dbp, d);
        else
            MMVAE_LAUNCH((hn_dw_kernel<8, 16>), grid, dim3(NTHR), 0, st, h, k.wp, bias, target, lse, g, k.part, k.dbp, d);
        mmvae_count_flops(4.0 * d.P * (double)d.V * d.C * d.hid);
        MMVAE_TRY(mmvae_check_launch("head_nll_dw"));
        MMVAE_LAUNCH(hn_fold_kernel, dim3(ceil_div(d.V * d.C * d.hid, NTHR)), dim3(NTHR), 0, st, k.part, k.dbp, dw, db, chunks, d);
        return mmvae_check_launch("head_nll_fold");
    }
    return MMVAE_OK;
}
