// gemm_small_kernel<MT, NT, KS, ...>: implicit GEMMs whose pixel-row count is too small to fill 256 CUs with 128-row
// tiles (classifier / bottleneck / MLP layers and their data gradients: 0.1 .. 5 GFLOP, rows <= ~10k).
//
// The 128-row kernel gives such a problem a handful of workgroups and then needs split-K (two launches, fp32 slabs)
// or the 16-row weight-streaming kernel (a few dozen workgroups, each a serial chain over the whole weight matrix) to
// find parallelism; both run at a few TFLOP/s.  Here ONE WAVE owns one (16*MT) x (16*NT) output tile:
//   * both operands are loaded straight into MFMA fragment registers (the fragment layout of
//     v_mfma_f32_16x16x32_bf16 is a 16-byte load per lane), through buffer descriptors: 32-bit offsets and hardware
//     range checking (padded taps, rows past the end and weight rows past Npad read as zeros) -- no LDS, no barrier;
//   * 2 .. 4 64-deep chunks of fragments are in flight in front of the MFMAs (gemm_small_kernel_v0, the form this replaced and
//     the reference it is tested against: one chunk while the previous one feeds the MFMAs);
//   * the KS waves of a workgroup split the K range of the same tile and are summed through LDS once (in-kernel
//     split-K: one launch, no global slabs);
//   * the product is computed transposed (weights in the A slot), so a lane owns 4 consecutive channels of one of its
//     own gathered pixel rows: the full epilogue (bias, bf16/fp32 stores, activated copy with dropout mask,
//     BatchNorm statistics, d-activation with BatchNorm-backward sums, bias-gradient column sums) runs from registers
//     with 8/16-byte accesses.
#include "gemm.h"
#include <cstdlib>

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;

__device__ __forceinline__ bf16x8 buf_load16(__amdgpu_buffer_rsrc_t rsrc, unsigned off) {
    const i32x4 v = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)off, 0, 0));
    return __builtin_bit_cast(bf16x8, v);
}

// q = r / d, rem = r % d for 0 <= r < 2^23 with inv = 1.0f/d (one correction step each way)
__device__ __forceinline__ int fast_divmod(int r, int d, float inv, int& rem) {
    int q = (int)((float)r * inv);
    rem = r - q * d;
    if (rem < 0) { --q; rem += d; }
    else if (rem >= d) { ++q; rem -= d; }
    return q;
}

template <int MT, int NT, int KS, bool DGRAD>
__global__ __launch_bounds__(KS * 64) void gemm_small_kernel_v0(const GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const GatherCommon& c = p.c;
    const GatherClass& k = p.cls[blockIdx.z];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    constexpr int RW = MT * 16, CW = NT * 16;
    const int tiles_per_group = (k.rows_per_group + RW - 1) / RW;
    if ((int)blockIdx.x >= tiles_per_group * c.groups) return;
    const int g = blockIdx.x / tiles_per_group;
    const int row0 = (blockIdx.x - g * tiles_per_group) * RW;
    const int n_base = blockIdx.y * CW;
    const int K = k.K, Kpad = k.Kpad;
    const int nch_all = (K + 63) / 64;
    const int ch0 = nch_all * wave / KS, ch1 = nch_all * (wave + 1) / KS;

    const int nimg_a = c.a_bcast_n > 0 ? c.a_bcast_n : c.groups * c.group_n;
    const __amdgpu_buffer_rsrc_t arsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<bf16*>(c.A), 0, (int)((size_t)nimg_a * c.AH * c.AW * c.Ald * sizeof(bf16)), 0x00020000);
    const __amdgpu_buffer_rsrc_t brsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<bf16*>(k.Wp), 0, (int)((size_t)p.npad * Kpad * sizeof(bf16)), 0x00020000);

    // ---- this lane's pixel rows (operand fragment layout: row = mt*16 + lane%16)
    const int pix_per_img = k.OY * k.OX;
    const float inv_pix = 1.0f / (float)pix_per_img, inv_ox = 1.0f / (float)k.OX, inv_tw = 1.0f / (float)k.TW;
    int a_off[MT], opix[MT], dpix[MT], grow[MT];
    unsigned mtap[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int r = row0 + mt * 16 + fr;
        a_off[mt] = 0; mtap[mt] = 0; opix[mt] = -1; dpix[mt] = 0; grow[mt] = 0;
        if (r < k.rows_per_group) {
            int rem, ox;
            const int img = fast_divmod(r, pix_per_img, inv_pix, rem);
            const int oy = fast_divmod(rem, k.OX, inv_ox, ox);
            const int nimg = g * c.group_n + img;
            int aimg = nimg;
            if (c.a_bcast_n > 0) aimg %= c.a_bcast_n;
            const int y0 = oy * c.sy + k.offy, x0 = ox * c.sx + k.offx;
            a_off[mt] = (((aimg * c.AH + y0) * c.AW + x0) * c.Ald + fq * 8) * (int)sizeof(bf16);
            unsigned mx = 0, m = 0;
            for (int tx = 0; tx < k.TW; ++tx) mx |= ((unsigned)(x0 + tx * c.dx) < (unsigned)c.AW ? 1u : 0u) << tx;
            for (int ty = 0; ty < k.TH; ++ty)
                if ((unsigned)(y0 + ty * c.dy) < (unsigned)c.AH) m |= mx << (ty * k.TW);
            mtap[mt] = m;
            const int py = oy * c.osy + k.ooy, px = ox * c.osx + k.oox;
            opix[mt] = (nimg * c.OH + py) * c.OW + px;
            dpix[mt] = p.d_bcast_n > 0 ? ((nimg % p.d_bcast_n) * c.OH + py) * c.OW + px : opix[mt];
            grow[mt] = g * k.rows_per_group + r;
        }
    }
    const int ntaps = k.TH * k.TW;
    const int cshift = 31 - __clz(c.C);          // multi-tap operands have a power-of-two channel count >= 32 (launcher)
    int b_off[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) b_off[nt] = ((n_base + nt * 16 + fr) * Kpad + fq * 8) * (int)sizeof(bf16);

    bf16x8 a0[2][MT], a1[2][MT], b0[2][NT], b1[2][NT];
    auto load_chunk = [&](int ch, bf16x8 (&a)[2][MT], bf16x8 (&b)[2][NT]) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int kk0 = ch * 64 + ks * 32;
            int tap = 0, acb = kk0;
            if (ntaps > 1) { tap = kk0 >> cshift; acb = kk0 & (c.C - 1); }    // wave-uniform
            const int ty = (int)(((float)tap + 0.5f) * inv_tw), tx = tap - ty * k.TW;
            const int toff = (((ty * c.dy) * c.AW + tx * c.dx) * c.Ald + acb) * (int)sizeof(bf16);
            const bool kin = kk0 + fq * 8 < K;                               // only the last k-step can be partial
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const unsigned bit = kin ? (mtap[mt] >> tap) & 1u : 0u;
                a[ks][mt] = buf_load16(arsrc, (unsigned)(a_off[mt] + toff) | (bit - 1u));   // invalid -> 0xFFFFFFFF -> zeros
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                b[ks][nt] = buf_load16(brsrc, kk0 < Kpad ? (unsigned)(b_off[nt] + kk0 * (int)sizeof(bf16)) : 0xFFFFFFFFu);
        }
    };
    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto compute_chunk = [&](bf16x8 (&a)[2][MT], bf16x8 (&b)[2][NT]) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)           // transposed product: rows = channels, columns = pixel rows
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[ks][nt], a[ks][mt], acc[mt][nt], 0, 0, 0);
    };

    if (ch0 < ch1) load_chunk(ch0, a0, b0);
    for (int ch = ch0; ch < ch1; ch += 2) {
        if (ch + 1 < ch1) load_chunk(ch + 1, a1, b1);
        compute_chunk(a0, b0);
        if (ch + 1 < ch1) {
            if (ch + 2 < ch1) load_chunk(ch + 2, a0, b0);
            compute_chunk(a1, b1);
        }
    }

    // ---- in-kernel split-K: waves 1.. hand their partial tile to wave 0 through LDS
    if (KS > 1) {
        float* red = reinterpret_cast<float*>(smem);          // [KS-1][MT*NT*4][64]
        if (wave > 0) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        red[((wave - 1) * (MT * NT * 4) + (mt * NT + nt) * 4 + j) * 64 + lane] = acc[mt][nt][j];
        }
        __syncthreads();
        if (wave > 0) return;
#pragma unroll
        for (int w = 0; w < KS - 1; ++w)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[mt][nt][j] += red[(w * (MT * NT * 4) + (mt * NT + nt) * 4 + j) * 64 + lane];
    }

    // ---- epilogue: lane owns channels n_base + nt*16 + fq*4 .. +3 of pixel row mt*16 + fr
    const bool want_stats = !DGRAD && p.colstats != nullptr;
    const bool want_red = DGRAD && (p.d_red != nullptr || p.d_colsum != nullptr);
    const int tn = p.d_cmod > 0 ? p.d_cmod : c.N;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n0 = n_base + nt * 16 + fq * 4;
        if (n0 >= c.N) continue;
        const int nv = min(4, c.N - n0);                      // valid channels of this quad
        float bias4[4], dsc[4], dsh[4], dmean[4], drstd[4], s1[4], s2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = min(n0 + j, c.N - 1);
            const int tcol = p.d_cmod > 0 ? n % p.d_cmod : n;
            bias4[j] = p.bias ? p.bias[n] : 0.f;
            dsc[j] = 1.f; dsh[j] = 0.f; dmean[j] = 0.f; drstd[j] = 0.f; s1[j] = 0.f; s2[j] = 0.f;
            if (DGRAD && p.d_affine) { const float2 a = p.d_affine[g * tn + tcol]; dsc[j] = a.x; dsh[j] = a.y; }
            if (DGRAD && p.d_meanrstd) { const float2 m = p.d_meanrstd[g * tn + tcol]; dmean[j] = m.x; drstd[j] = m.y; }
        }
        const bool vec = nv == 4 && p.ldo % 4 == 0;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            if (opix[mt] < 0) continue;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = acc[mt][nt][j] + bias4[j];
            if (DGRAD) {
                float rr[4];
                const bf16* rp = p.d_r + (size_t)dpix[mt] * p.d_ld + n0;
                if (nv == 4 && p.d_ld % 4 == 0) {
                    const bf16x4 rv = *reinterpret_cast<const bf16x4*>(rp);
#pragma unroll
                    for (int j = 0; j < 4; ++j) rr[j] = (float)rv[j];
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) rr[j] = j < nv ? (float)rp[j] : 0.f;
                }
                unsigned mb = 0x01010101u;
                if (p.d_mask) {
                    const uint8_t* mp = p.d_mask + (size_t)grow[mt] * c.N + n0;
                    if (nv == 4 && c.N % 4 == 0) mb = *reinterpret_cast<const unsigned*>(mp);
                    else { mb = 0; for (int j = 0; j < nv; ++j) mb |= (unsigned)(mp[j] ? 1 : 0) << (8 * j); }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float x = v[j] * act_bwd(p.d_act, rr[j] * dsc[j] + dsh[j]);
                    if (p.d_mask) x = ((mb >> (8 * j)) & 0xff) ? x * p.d_mask_scale : 0.f;
                    v[j] = x;
                    if (want_red && j < nv) { s1[j] += x; s2[j] += x * (rr[j] - dmean[j]) * drstd[j]; }
                }
            }
            if (want_stats) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nv) { s1[j] += v[j]; s2[j] += v[j] * v[j]; }
            }
            float av[4];
            if (!DGRAD && p.out_act_bf) {
                unsigned mb = 0x01010101u;
                if (p.e_mask) {
                    const uint8_t* mp = p.e_mask + (size_t)grow[mt] * c.N + n0;
                    if (nv == 4 && c.N % 4 == 0) mb = *reinterpret_cast<const unsigned*>(mp);
                    else { mb = 0; for (int j = 0; j < nv; ++j) mb |= (unsigned)(mp[j] ? 1 : 0) << (8 * j); }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float x = act_fwd(p.e_act, v[j]);
                    if (p.e_mask) x = ((mb >> (8 * j)) & 0xff) ? x * p.e_mask_scale : 0.f;
                    av[j] = x;
                }
            }
            const size_t o = (size_t)opix[mt] * p.ldo + n0;
            if (vec) {
                if (p.out_bf) {
                    bf16x4 ob;
#pragma unroll
                    for (int j = 0; j < 4; ++j) ob[j] = (bf16)v[j];
                    *reinterpret_cast<bf16x4*>(p.out_bf + o) = ob;
                }
                if (!DGRAD && p.out_act_bf) {
                    bf16x4 ob;
#pragma unroll
                    for (int j = 0; j < 4; ++j) ob[j] = (bf16)av[j];
                    *reinterpret_cast<bf16x4*>(p.out_act_bf + o) = ob;
                }
                if (p.out_f) *reinterpret_cast<f32x4*>(p.out_f + o) = f32x4{v[0], v[1], v[2], v[3]};
            } else {
                for (int j = 0; j < nv; ++j) {
                    if (p.out_bf) p.out_bf[o + j] = (bf16)v[j];
                    if (!DGRAD && p.out_act_bf) p.out_act_bf[o + j] = (bf16)av[j];
                    if (p.out_f) p.out_f[o + j] = v[j];
                }
            }
        }
        if (want_stats || want_red) {
            const int slot = (blockIdx.x + 5 * blockIdx.z) % MMVAE_STAT_SLOTS;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float a = s1[j], b = s2[j];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
                if (fr == 0 && j < nv) {
                    const int n = n0 + j;
                    float2* dst = want_stats ? p.colstats : p.d_red;
                    if (dst) {
                        const bool cm = !want_stats && p.d_cmod > 0;
                        const int tcol = cm ? n % p.d_cmod : n;
                        const int sl = (slot + (cm ? n / p.d_cmod : 0)) % MMVAE_STAT_SLOTS;
                        atomicAdd(&dst[(g * MMVAE_STAT_SLOTS + sl) * (cm ? p.d_cmod : c.N) + tcol].x, a);
                        atomicAdd(&dst[(g * MMVAE_STAT_SLOTS + sl) * (cm ? p.d_cmod : c.N) + tcol].y, b);
                    }
                    if (p.d_colsum) atomicAdd(p.d_colsum + n, a);
                }
            }
        }
    }
}

// ---------------------------------------------------------------- the prefetching form (knob "gemm_small_prefetch" = 2 .. 4, default 2)
// Same grid, LDS, chunk order and arithmetic as gemm_small_kernel_v0 above (knob 0, the A/B and bitwise reference), bit for bit
// on every stored tensor (tests/test_gpu_gemm_small_forms.py); what differs is when things are loaded.  These grids put about one
// wave on each SIMD, so a wave hides its memory latency itself or not at all, and the launch costs its number of DEPENDENT
// round trips:
//   * the launcher flattens GemmParams into SmallArgs: what the host knows (which optional operands exist, the 4-wide path,
//     d_cmod) is settled there.  An absent table is a buffer descriptor of zero bytes -- every read of it returns zero without
//     touching memory -- so the device code has no test on a pointer in front of a load;
//   * the epilogue's operands (bias, BatchNorm tables, saved raw tensor, keep mask) depend only on the lane's rows and
//     columns: the wave that runs the epilogue issues them in one block BEFORE the operand loads and consumes them after the
//     LDS reduce;
//   * up to DEPTH chunks of both operands are in flight before the first MFMA (DEPTH = 4: 128 VGPRs at MT = NT = 2); a longer
//     K range refills the slot just consumed.  A load of the K loop for a chunk past the wave's range is issued with the
//     out-of-range offset instead of being branched around.
struct SmallCls {
    int OY, OX, rows_per_group, TH, TW, offy, offx, ooy, oox, K, Kpad, w_bytes;
    const bf16* Wp;
};
enum { SM_AFFINE = 1, SM_MASK = 2, SM_OUT_BF = 4, SM_OUT_F = 8, SM_OUT_ACT = 16, SM_STATS = 32, SM_COLSUM = 64, SM_CMOD = 128 };
struct SmallArgs {
    const bf16* A; const bf16* d_r;
    const float* bias; const float2* d_affine; const float2* d_meanrstd; const uint8_t* mask;   // never null (stand-in: A, zero bytes)
    bf16* out_bf; float* out_f; bf16* out_act_bf;
    float2* stats;                  // forward: colstats, data gradient: d_red
    float* d_colsum;
    int a_bytes, bias_bytes, aff_bytes, mr_bytes, mask_bytes;
    int groups, group_n, a_bcast_n, d_bcast_n;
    int AH, AW, Ald, C, sy, sx, dy, dx;
    int OH, OW, osy, osx, N, ldo, d_ld;
    int cmod;                       // channels of the BatchNorm tables: d_cmod, or N
    float inv_cmod;
    int act;                        // forward: e_act, data gradient: d_act
    float mask_scale;
    unsigned flags;
    SmallCls cls[MMVAE_MAX_CLASSES];
};

__device__ __forceinline__ float buf_load_f32(__amdgpu_buffer_rsrc_t rsrc, unsigned off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)off, 0, 0));
}
__device__ __forceinline__ float2 buf_load_f32x2(__amdgpu_buffer_rsrc_t rsrc, unsigned off) {
    return __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)off, 0, 0));
}

template <int MT, int NT, int KS, bool DGRAD, bool VEC, int DEPTH>
__global__ __launch_bounds__(KS * 64) void gemm_small_kernel(const SmallArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const SmallCls k = a.cls[blockIdx.z];
    // every scalar the kernel uses is alive here: its kernel-argument loads are issued in this block, behind two waits, and not
    // each in front of its first use behind a wait of its own (an asm statement takes at most 30 operands)
    asm volatile("" ::"s"(a.A), "s"(a.d_r), "s"(a.bias), "s"(a.d_affine), "s"(a.d_meanrstd), "s"(a.mask), "s"(a.out_bf), "s"(a.out_f),
                 "s"(a.out_act_bf), "s"(a.stats), "s"(a.d_colsum), "s"(k.Wp), "s"(a.a_bytes), "s"(a.bias_bytes), "s"(a.aff_bytes),
                 "s"(a.mr_bytes), "s"(a.mask_bytes), "s"(a.groups), "s"(a.group_n), "s"(a.a_bcast_n), "s"(a.d_bcast_n), "s"(a.AH),
                 "s"(a.AW), "s"(a.Ald), "s"(a.C), "s"(a.sy), "s"(a.sx), "s"(a.dy), "s"(a.dx));
    asm volatile("" ::"s"(a.OH), "s"(a.OW), "s"(a.osy), "s"(a.osx), "s"(a.N), "s"(a.ldo), "s"(a.d_ld), "s"(a.cmod), "s"(a.inv_cmod),
                 "s"(a.act), "s"(a.mask_scale), "s"(a.flags), "s"(k.OY), "s"(k.OX), "s"(k.rows_per_group), "s"(k.TH), "s"(k.TW),
                 "s"(k.offy), "s"(k.offx), "s"(k.ooy), "s"(k.oox), "s"(k.K), "s"(k.Kpad), "s"(k.w_bytes));
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // scalar: the branches on it are no exec-mask branches
    const int fr = lane & 15, fq = lane >> 4;
    constexpr int RW = MT * 16, CW = NT * 16;
    const int tiles_per_group = (k.rows_per_group + RW - 1) / RW;
    if ((int)blockIdx.x >= tiles_per_group * a.groups) return;
    const int g = blockIdx.x / tiles_per_group;
    const int row0 = (blockIdx.x - g * tiles_per_group) * RW;
    const int n_base = blockIdx.y * CW;
    const int K = k.K, Kpad = k.Kpad, N = a.N;
    const int nch_all = (K + 63) / 64;
    const int ch0 = nch_all * wave / KS, ch1 = nch_all * (wave + 1) / KS;
    const int nch = ch1 - ch0;
    const unsigned flags = a.flags;

    const __amdgpu_buffer_rsrc_t arsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(a.A), 0, a.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t brsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(k.Wp), 0, k.w_bytes, 0x00020000);

    // ---- this lane's pixel rows (operand fragment layout: row = mt*16 + lane%16)
    const int pix_per_img = k.OY * k.OX;
    const float inv_pix = 1.0f / (float)pix_per_img, inv_ox = 1.0f / (float)k.OX, inv_tw = 1.0f / (float)k.TW;
    int a_off[MT], opix[MT], dpix[MT], grow[MT];
    unsigned mtap[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int r = row0 + mt * 16 + fr;
        a_off[mt] = 0; mtap[mt] = 0; opix[mt] = -1; dpix[mt] = 0; grow[mt] = 0;
        if (r < k.rows_per_group) {
            int rem, ox;
            const int img = fast_divmod(r, pix_per_img, inv_pix, rem);
            const int oy = fast_divmod(rem, k.OX, inv_ox, ox);
            const int nimg = g * a.group_n + img;
            int aimg = nimg;
            if (a.a_bcast_n > 0) aimg %= a.a_bcast_n;
            const int y0 = oy * a.sy + k.offy, x0 = ox * a.sx + k.offx;
            a_off[mt] = (((aimg * a.AH + y0) * a.AW + x0) * a.Ald + fq * 8) * (int)sizeof(bf16);
            unsigned mx = 0, m = 0;
            for (int tx = 0; tx < k.TW; ++tx) mx |= ((unsigned)(x0 + tx * a.dx) < (unsigned)a.AW ? 1u : 0u) << tx;
            for (int ty = 0; ty < k.TH; ++ty)
                if ((unsigned)(y0 + ty * a.dy) < (unsigned)a.AH) m |= mx << (ty * k.TW);
            mtap[mt] = m;
            const int py = oy * a.osy + k.ooy, px = ox * a.osx + k.oox;
            opix[mt] = (nimg * a.OH + py) * a.OW + px;
            dpix[mt] = a.d_bcast_n > 0 ? ((nimg % a.d_bcast_n) * a.OH + py) * a.OW + px : opix[mt];
            grow[mt] = g * k.rows_per_group + r;
        }
    }

    // ---- epilogue operands of the wave that runs the epilogue: issued here, consumed behind the reduce.  A lane owns channels
    // n_base + nt*16 + fq*4 .. +3 of pixel row mt*16 + fr; rows and columns past the end read a valid stand-in element.
    // (left uninitialised on purpose: the other waves never read them, and a default value would be merged with the loaded one
    //  right behind this block -- a copy that waits for the load)
    float bias4[NT][4];
    float2 aff[NT][4], mrs[NT][4];
    int tcol[NT][4], tdiv[NT][4];
    unsigned rbits[MT][NT][VEC ? 2 : 4];          // saved raw tensor as loaded (bf16 pairs / single bf16): unpacked where it is consumed
    unsigned mb[MT][NT];
    if (KS == 1 || wave == 0) {
        const __amdgpu_buffer_rsrc_t bias_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.bias), 0, a.bias_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t aff_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2*>(a.d_affine), 0, a.aff_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t mr_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2*>(a.d_meanrstd), 0, a.mr_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t mask_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.mask), 0, a.mask_bytes, 0x00020000);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int n0 = n_base + nt * 16 + fq * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = min(n0 + j, N - 1);
                tcol[nt][j] = n; tdiv[nt][j] = 0;
                if (flags & SM_CMOD) { int rem; tdiv[nt][j] = fast_divmod(n, a.cmod, a.inv_cmod, rem); tcol[nt][j] = rem; }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bias4[nt][j] = buf_load_f32(bias_rsrc, (unsigned)min(n0 + j, N - 1) * 4u);
                if (DGRAD) {
                    aff[nt][j] = buf_load_f32x2(aff_rsrc, (unsigned)(g * a.cmod + tcol[nt][j]) * 8u);
                    mrs[nt][j] = buf_load_f32x2(mr_rsrc, (unsigned)(g * a.cmod + tcol[nt][j]) * 8u);
                }
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                if (DGRAD) {
                    if (VEC) {
                        const uint2 rv = *reinterpret_cast<const uint2*>(a.d_r + (size_t)dpix[mt] * a.d_ld + min(n0, N - 4));
                        rbits[mt][nt][0] = rv.x; rbits[mt][nt][1] = rv.y;
                    } else {
                        const unsigned short* rp = reinterpret_cast<const unsigned short*>(a.d_r) + (size_t)dpix[mt] * a.d_ld;
#pragma unroll
                        for (int j = 0; j < 4; ++j) rbits[mt][nt][j] = rp[min(n0 + j, N - 1)];
                    }
                }
                const unsigned moff = (unsigned)(grow[mt] * N + n0);
                if (VEC) {
                    mb[mt][nt] = __builtin_amdgcn_raw_buffer_load_b32(mask_rsrc, (int)moff, 0, 0);
                } else {
                    unsigned m = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        m |= (unsigned)(__builtin_amdgcn_raw_buffer_load_b8(mask_rsrc, (int)(moff + j), 0, 0) ? 1 : 0) << (8 * j);
                    mb[mt][nt] = m;
                }
            }
        }
    }

    const int ntaps = k.TH * k.TW;
    const int cshift = 31 - __clz(a.C);          // multi-tap operands have a power-of-two channel count >= 32 (launcher)
    int b_off[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) b_off[nt] = ((n_base + nt * 16 + fr) * Kpad + fq * 8) * (int)sizeof(bf16);

    // chunk ch of this wave's range, or nothing (every offset out of range) when there is no such chunk
    auto load_chunk = [&](int ch, bf16x8 (&fa)[2][MT], bf16x8 (&fb)[2][NT]) {
        const bool live = ch < ch1;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int kk0 = ch * 64 + ks * 32;
            int tap = 0, acb = kk0;
            if (ntaps > 1) { tap = kk0 >> cshift; acb = kk0 & (a.C - 1); }    // wave-uniform
            const int ty = (int)(((float)tap + 0.5f) * inv_tw), tx = tap - ty * k.TW;
            const int toff = (((ty * a.dy) * a.AW + tx * a.dx) * a.Ald + acb) * (int)sizeof(bf16);
            const bool kin = live & (kk0 + fq * 8 < K);                      // only the last k-step can be partial
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const unsigned bit = (mtap[mt] >> (tap & 31)) & (unsigned)kin;     // (no select: it becomes a branch around the load)
                fa[ks][mt] = buf_load16(arsrc, (unsigned)(a_off[mt] + toff) | (bit - 1u));   // invalid -> 0xFFFFFFFF -> zeros
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                fb[ks][nt] = buf_load16(brsrc, (live & (kk0 < Kpad)) ? (unsigned)(b_off[nt] + kk0 * (int)sizeof(bf16)) : 0xFFFFFFFFu);
        }
    };
    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto compute_chunk = [&](bf16x8 (&fa)[2][MT], bf16x8 (&fb)[2][NT]) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)           // transposed product: rows = channels, columns = pixel rows
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[ks][nt], fa[ks][mt], acc[mt][nt], 0, 0, 0);
    };

    // Register ring: DEPTH chunks are in flight before the first MFMA; a range longer than that refills slot i as soon as it has
    // been consumed.  One loop serves both: a range that fits (at depth 4 every MultiMNIST launch, at depth 2 the ones with K <= 512) runs it once and skips the
    // refills.  (As compiled, the wait in front of slot 0 is vmcnt(0): a longer range drains its loads once per round of DEPTH
    // chunks, where gemm_small_kernel_v0 drains them at every chunk.)
    bf16x8 ra[DEPTH][2][MT], rb[DEPTH][2][NT];
#pragma unroll
    for (int i = 0; i < DEPTH; ++i) load_chunk(ch0 + i, ra[i], rb[i]);
#pragma unroll 1
    for (int base = 0; base < nch; base += DEPTH) {
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) {
            if (base + i < nch) compute_chunk(ra[i], rb[i]);
            __builtin_amdgcn_sched_barrier(0);     // the refill stays behind the MFMAs that free its registers: lifted above them
            if (nch > DEPTH) load_chunk(ch0 + base + i + DEPTH, ra[i], rb[i]);      // it would need a second set
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // ---- in-kernel split-K: waves 1.. hand their partial tile to wave 0 through LDS
    if (KS > 1) {
        float* red = reinterpret_cast<float*>(smem);          // [KS-1][MT*NT*4][64]
        if (wave > 0) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        red[((wave - 1) * (MT * NT * 4) + (mt * NT + nt) * 4 + j) * 64 + lane] = acc[mt][nt][j];
        }
        __syncthreads();
        if (wave > 0) return;
#pragma unroll
        for (int w = 0; w < KS - 1; ++w)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[mt][nt][j] += red[(w * (MT * NT * 4) + (mt * NT + nt) * 4 + j) * 64 + lane];
    }

    // ---- epilogue from registers: the arithmetic of gemm_small_kernel_v0, term for term
    const bool has_mask = (flags & SM_MASK) != 0;
    const bool want_stats = !DGRAD && (flags & SM_STATS) != 0;
    const bool want_red = DGRAD && (flags & (SM_STATS | SM_COLSUM)) != 0;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n0 = n_base + nt * 16 + fq * 4;
        if (n0 >= N) continue;
        const int nv = VEC ? 4 : min(4, N - n0);              // valid channels of this quad
        float dsc[4], dsh[4], dmean[4], drstd[4], s1[4], s2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dsc[j] = (flags & SM_AFFINE) ? aff[nt][j].x : 1.f; dsh[j] = (flags & SM_AFFINE) ? aff[nt][j].y : 0.f;
            dmean[j] = mrs[nt][j].x; drstd[j] = mrs[nt][j].y; s1[j] = 0.f; s2[j] = 0.f;
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            if (opix[mt] < 0) continue;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = acc[mt][nt][j] + bias4[nt][j];
            const unsigned mbits = mb[mt][nt];
            if (DGRAD) {
                float rr[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {       // a bf16 is the upper half of its float
                    const unsigned b = VEC ? ((j & 1) ? rbits[mt][nt][j >> 1] & 0xffff0000u : rbits[mt][nt][j >> 1] << 16) : rbits[mt][nt][VEC ? 0 : j] << 16;
                    rr[j] = j < nv ? __builtin_bit_cast(float, b) : 0.f;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float x = v[j] * act_bwd(a.act, rr[j] * dsc[j] + dsh[j]);
                    if (has_mask) x = ((mbits >> (8 * j)) & 0xff) ? x * a.mask_scale : 0.f;
                    v[j] = x;
                    if (want_red && j < nv) { s1[j] += x; s2[j] += x * (rr[j] - dmean[j]) * drstd[j]; }
                }
            }
            if (want_stats) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nv) { s1[j] += v[j]; s2[j] += v[j] * v[j]; }
            }
            float av[4];
            if (!DGRAD && (flags & SM_OUT_ACT)) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float x = act_fwd(a.act, v[j]);
                    if (has_mask) x = ((mbits >> (8 * j)) & 0xff) ? x * a.mask_scale : 0.f;
                    av[j] = x;
                }
            }
            const size_t o = (size_t)opix[mt] * a.ldo + n0;
            if (VEC) {
                if (flags & SM_OUT_BF) {
                    bf16x4 ob;
#pragma unroll
                    for (int j = 0; j < 4; ++j) ob[j] = (bf16)v[j];
                    *reinterpret_cast<bf16x4*>(a.out_bf + o) = ob;
                }
                if (!DGRAD && (flags & SM_OUT_ACT)) {
                    bf16x4 ob;
#pragma unroll
                    for (int j = 0; j < 4; ++j) ob[j] = (bf16)av[j];
                    *reinterpret_cast<bf16x4*>(a.out_act_bf + o) = ob;
                }
                if (flags & SM_OUT_F) *reinterpret_cast<f32x4*>(a.out_f + o) = f32x4{v[0], v[1], v[2], v[3]};
            } else {
                for (int j = 0; j < nv; ++j) {
                    if (flags & SM_OUT_BF) a.out_bf[o + j] = (bf16)v[j];
                    if (!DGRAD && (flags & SM_OUT_ACT)) a.out_act_bf[o + j] = (bf16)av[j];
                    if (flags & SM_OUT_F) a.out_f[o + j] = v[j];
                }
            }
        }
        if (want_stats || want_red) {
            const int slot = (blockIdx.x + 5 * blockIdx.z) % MMVAE_STAT_SLOTS;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float sa = s1[j], sb = s2[j];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) { sa += __shfl_xor(sa, o, 64); sb += __shfl_xor(sb, o, 64); }
                if (fr == 0 && j < nv) {
                    const int n = n0 + j;
                    if (flags & SM_STATS) {       // forward tables have N channels (the launcher: cmod = N, tdiv = 0)
                        const int sl = (slot + tdiv[nt][j]) % MMVAE_STAT_SLOTS;
                        atomicAdd(&a.stats[(g * MMVAE_STAT_SLOTS + sl) * a.cmod + tcol[nt][j]].x, sa);
                        atomicAdd(&a.stats[(g * MMVAE_STAT_SLOTS + sl) * a.cmod + tcol[nt][j]].y, sb);
                    }
                    if (DGRAD && (flags & SM_COLSUM)) atomicAdd(a.d_colsum + n, sa);
                }
            }
        }
    }
}

template <bool DGRAD>
SmallArgs flatten_small(const GemmParams& p) {
    const GatherCommon& c = p.c;
    SmallArgs a{};
    const long long nimg_a = c.a_bcast_n > 0 ? c.a_bcast_n : (long long)c.groups * c.group_n;
    a.A = c.A; a.a_bytes = (int)((size_t)nimg_a * c.AH * c.AW * c.Ald * sizeof(bf16));
    a.groups = c.groups; a.group_n = c.group_n; a.a_bcast_n = c.a_bcast_n; a.d_bcast_n = p.d_bcast_n;
    a.AH = c.AH; a.AW = c.AW; a.Ald = c.Ald; a.C = c.C; a.sy = c.sy; a.sx = c.sx; a.dy = c.dy; a.dx = c.dx;
    a.OH = c.OH; a.OW = c.OW; a.osy = c.osy; a.osx = c.osx; a.N = c.N; a.ldo = p.ldo; a.d_ld = p.d_ld;
    int rows_max = 0;
    for (int i = 0; i < c.nclasses; ++i) {
        const GatherClass& k = p.cls[i];
        SmallCls& s = a.cls[i];
        s.OY = k.OY; s.OX = k.OX; s.rows_per_group = k.rows_per_group; s.TH = k.TH; s.TW = k.TW; s.offy = k.offy; s.offx = k.offx;
        s.ooy = k.ooy; s.oox = k.oox; s.K = k.K; s.Kpad = k.Kpad; s.w_bytes = (int)((size_t)p.npad * k.Kpad * sizeof(bf16)); s.Wp = k.Wp;
        rows_max = max(rows_max, k.rows_per_group);
    }
    const bool cm = DGRAD && p.d_cmod > 0;      // (the forward statistics have N channels whatever d_cmod says)
    a.cmod = cm ? p.d_cmod : c.N; a.inv_cmod = 1.0f / (float)a.cmod;
    const void* none = c.A;                     // stand-in base of a table the launch does not have: a descriptor of zero bytes
    a.bias = p.bias ? p.bias : (const float*)none; a.bias_bytes = p.bias ? c.N * (int)sizeof(float) : 0;
    const bool aff = DGRAD && p.d_affine, mr = DGRAD && p.d_meanrstd;
    const int tab_bytes = c.groups * a.cmod * (int)sizeof(float2);
    a.d_affine = aff ? p.d_affine : (const float2*)none; a.aff_bytes = aff ? tab_bytes : 0;
    a.d_meanrstd = mr ? p.d_meanrstd : (const float2*)none; a.mr_bytes = mr ? tab_bytes : 0;
    const uint8_t* mask = DGRAD ? p.d_mask : (p.out_act_bf ? p.e_mask : nullptr);
    a.mask = mask ? mask : (const uint8_t*)none; a.mask_bytes = mask ? c.groups * rows_max * c.N : 0;
    a.mask_scale = DGRAD ? p.d_mask_scale : p.e_mask_scale;
    a.act = DGRAD ? p.d_act : p.e_act;
    a.d_r = p.d_r; a.out_bf = p.out_bf; a.out_f = p.out_f; a.out_act_bf = DGRAD ? nullptr : p.out_act_bf;
    a.stats = DGRAD ? p.d_red : p.colstats; a.d_colsum = DGRAD ? p.d_colsum : nullptr;
    a.flags = (aff ? SM_AFFINE : 0) | (mask ? SM_MASK : 0) | (a.out_bf ? SM_OUT_BF : 0) | (a.out_f ? SM_OUT_F : 0) |
              (a.out_act_bf ? SM_OUT_ACT : 0) | (a.stats ? SM_STATS : 0) | (a.d_colsum ? SM_COLSUM : 0) | (cm ? SM_CMOD : 0);
    return a;
}

template <int MT, int NT, int KS, bool DGRAD, bool VEC>
void launch_small_depth(const SmallArgs& a, int depth, dim3 grid, size_t lds, hipStream_t stream) {
    if (depth == 2) MMVAE_LAUNCH((gemm_small_kernel<MT, NT, KS, DGRAD, VEC, 2>), grid, dim3(KS * 64), lds, stream, a);
    else if (depth == 3) MMVAE_LAUNCH((gemm_small_kernel<MT, NT, KS, DGRAD, VEC, 3>), grid, dim3(KS * 64), lds, stream, a);
    else MMVAE_LAUNCH((gemm_small_kernel<MT, NT, KS, DGRAD, VEC, 4>), grid, dim3(KS * 64), lds, stream, a);
}

template <int MT, int NT, int KS, bool DGRAD>
int launch_small(const GemmParams& p, hipStream_t stream) {
    const GatherCommon& c = p.c;
    int max_tiles = 0;
    for (int i = 0; i < c.nclasses; ++i) max_tiles = max(max_tiles, ceil_div(p.cls[i].rows_per_group, MT * 16));
    dim3 grid(max_tiles * c.groups, ceil_div(c.N, NT * 16), c.nclasses);
    const size_t lds = KS > 1 ? (size_t)(KS - 1) * MT * NT * 4 * 64 * sizeof(float) : 0;
    if (mmvae_probe_on()) {
        char note[40];
        snprintf(note, sizeof(note), "small<%d,%d,%d,%s>", MT, NT, KS, DGRAD ? "dgrad" : "fwd");
        mmvae_probe_note(note);
    }
    // knob gemm_small_prefetch: 2 .. 4: gemm_small_kernel with that many chunks of both operands in flight per wave (default 2);
    // 0: gemm_small_kernel_v0.  Depth 2 is the one the MultiMNIST step gains from: at depth 4 the launches are as
    // short, with 234 registers per lane instead of 186, and the step is not shorter than with the old form.
    const int depth = mmvae_knob(K_gemm_small_prefetch);
    if (depth <= 0) {
        MMVAE_LAUNCH((gemm_small_kernel_v0<MT, NT, KS, DGRAD>), grid, dim3(KS * 64), lds, stream, p);
    } else {
        const SmallArgs a = flatten_small<DGRAD>(p);
        // the 4-wide accesses of the epilogue: every quad of columns is whole and every row start a multiple of 4 elements
        const bool vec = c.N % 4 == 0 && p.ldo % 4 == 0 && (!DGRAD || p.d_ld % 4 == 0);
        if (vec) launch_small_depth<MT, NT, KS, DGRAD, true>(a, depth, grid, lds, stream);
        else launch_small_depth<MT, NT, KS, DGRAD, false>(a, depth, grid, lds, stream);
    }
    return mmvae_check_launch("gemm_small");
}

template <int MT, int NT, bool DGRAD>
int launch_small_ks(const GemmParams& p, int ks, hipStream_t stream) {
    if (ks >= 4) return launch_small<MT, NT, 4, DGRAD>(p, stream);
    if (ks >= 2) return launch_small<MT, NT, 2, DGRAD>(p, stream);
    return launch_small<MT, NT, 1, DGRAD>(p, stream);
}

}  // namespace

// returns 1 when the problem was launched here, 0 when the caller should use the generic kernels, < 0 on error
int try_launch_gemm_small(const GemmParams& pin, hipStream_t stream) {
    const GatherCommon& c = pin.c;
    int max_tiles128 = 0, min_nch = 1 << 30;
    long long tiles22 = 0, tiles44 = 0, rows_total = 0;
    for (int i = 0; i < c.nclasses; ++i) {
        const GatherClass& k = pin.cls[i];
        if (k.TH * k.TW > 1 && (c.C < 32 || (c.C & (c.C - 1)) != 0)) return 0;   // the tap walk must be wave-uniform
        if (k.TH * k.TW > 32) return 0;                                           // tap-validity bit mask
        max_tiles128 = max(max_tiles128, ceil_div(k.rows_per_group, 128));
        min_nch = min(min_nch, ceil_div(k.K, 64));
        tiles22 += (long long)ceil_div(k.rows_per_group, 32) * c.groups * ceil_div(c.N, 32);
        tiles44 += (long long)ceil_div(k.rows_per_group, 64) * c.groups * ceil_div(c.N, 64);
        rows_total += (long long)k.rows_per_group * c.groups;
    }
    // only problems that leave most of the chip idle under 128-row tiles
    const long long tiles128 = (long long)max_tiles128 * c.groups * c.nclasses * ceil_div(c.N, 128);
    if (tiles128 > 128) return 0;
    {   // ... and not the long-K giants: one wave per 32x32 tile re-reads both operands from L2 with no reuse
        constexpr double cap = 8.0;   // CelebA classifier.0 (13.4 GFLOP): 107 us here, ~35 us tiled + split-K
        double fl = 0.0;
        for (int i = 0; i < c.nclasses; ++i) fl += 2.0 * pin.cls[i].rows_per_group * c.groups * c.N * pin.cls[i].K;
        if (cap > 0.0 && fl > cap * 1e9) return 0;
    }
    const long long nimg_a = c.a_bcast_n > 0 ? c.a_bcast_n : (long long)c.groups * c.group_n;
    if (nimg_a * c.AH * c.AW * c.Ald * 2 >= (1ll << 31)) return 0;                 // 32-bit buffer offsets
    if ((long long)c.groups * c.group_n * c.OH * c.OW >= (1ll << 31) || rows_total >= (1ll << 23)) return 0;
    GemmParams p = pin;
    p.ksplit = 1; p.sk_buf = nullptr;
    // packed rows available (layers.h npad_for); the kernel range-checks weight rows against it
    if (p.npad <= 0) p.npad = c.N <= 16 ? 16 : c.N <= 32 ? 32 : c.N <= 64 ? 64 : round_up(c.N, 128);
    (void)tiles44;
    if (tiles22 > 1536) return 0;                                                  // enough work for the tile kernels
    if (p.d_r == nullptr && (p.d_mask || p.d_red || p.d_colsum)) return 0;
    constexpr long long wave_target = 1024;
    const int ks = (int)min((long long)min(4, max(1, min_nch / 2)), max(1ll, wave_target / max(tiles22, 1ll)));
    const int rc = p.d_r ? launch_small_ks<2, 2, true>(p, ks, stream) : launch_small_ks<2, 2, false>(p, ks, stream);
    return rc == MMVAE_OK ? 1 : rc;
}
