// The tile pieces the two stand-alone convolutions share (causal_conv.hip, conv4s2.hip): 256 threads = 4 waves as 2 x 2 (wm, wn) of
// 32 x 32, each wave a 2 x 2 grid of v_mfma_f32_16x16x32_bf16 tiles; fr = lane & 15, fq = lane >> 4.
//   forward / data gradient: 64 position rows x up to CT_KC channels go through LDS as bf16 (fp32 -> bf16 on the way in, load4 / round4),
//     A_LD bf16 per row: thread -> float4 column c4 = tid & 31 of the rows r0 + 8 i, r0 = tid >> 5.  A fragments come from that tile, B
//     fragments from the packed weights in global memory, on each kernel's own schedule; mma_2x2 is one k-step.
//   weight gradient: both operands go through LDS transposed ([channel][position], CT_KP positions per stage, T_LD bf16 per row), so
//     that a lane's 8 MFMA k-elements (positions) are contiguous: thread -> 4 channels cg = tid & 15 of position pairs (put_pair),
//     then CT_KP / 32 k-steps over the two tiles and a bounds-checked store of the 64 x 64 partial (store_partial).
// C fragment (every accumulator here): column = lane & 15, row = 4 (lane >> 4) + register.
// What is NOT here, on purpose: how a kernel finds its source rows (fetch lambdas, position decomposition, tap / parity geometry), when
// it reads its B fragments, and the forward epilogues: those differ between the two ops for measured reasons stated in their headers.
// Nor the statements that index the LDS tiles in the k-loops (the staging store, the fragment reads): they are the same few lines
// in both files, but behind a pointer parameter the compiler forms their addresses differently, and kernels measured up to 1 %
// slower than with the statements written in the kernel, against the __shared__ array itself.
#pragma once
#include "common.h"

constexpr int CT_KC = 128;               // channels per forward / data-gradient LDS stage
constexpr int CT_KP = 64;                // positions per weight-gradient LDS stage
constexpr int A_LD = CT_KC + 8;          // bf16 per LDS row of the source tile: 272 B, a multiple of 16 B off the bank period
constexpr int T_LD = CT_KP + 8;          // bf16 per LDS row of the transposed weight-gradient tiles: 144 B

// 4 consecutive channels of one position row; `left` = channels from src to the end of the row (<= 0: none)
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* __restrict__ src, int left) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (VEC) {
        if (left > 0) v = *reinterpret_cast<const float4*>(src);
    } else {
        if (left > 0) v.x = src[0];
        if (left > 1) v.y = src[1];
        if (left > 2) v.z = src[2];
        if (left > 3) v.w = src[3];
    }
    return v;
}

__device__ __forceinline__ bf16x4 round4(const float4& v) {
    bf16x4 o;
    o[0] = f2bf(v.x); o[1] = f2bf(v.y); o[2] = f2bf(v.z); o[3] = f2bf(v.w);
    return o;
}

// acc[a][b] += af[a] x bfr[b]: the wave's 2 x 2 grid of 16 x 16 x 32 updates of one k-step
__device__ __forceinline__ void mma_2x2(const bf16x8 (&af)[2], const bf16x8 (&bfr)[2], f32x4 (&acc)[2][2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bfr[b], acc[a][b], 0, 0, 0);
}

// positions lp, lp + 1 of channels 4 cg .. 4 cg + 3 into a transposed tile
__device__ __forceinline__ void put_pair(bf16* dst, const float4& a, const float4& b, int cg, int lp) {
    const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        bf16x2 pr;
        pr[0] = f2bf(av[j]); pr[1] = f2bf(bv[j]);
        *reinterpret_cast<bf16x2*>(&dst[(4 * cg + j) * T_LD + lp]) = pr;
    }
}

// the workgroup's 64 x 64 partial -> out[row][col], row0 + local row < rows, col0 + local column < cols, ld elements per row
__device__ __forceinline__ void store_partial(float* __restrict__ out, const f32x4 (&acc)[2][2], int row0, int rows, int col0, int cols, int ld,
                                              int wm, int wn, int fr, int fq) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int col = col0 + wn * 32 + b * 16 + fr;
        if (col >= cols) continue;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = row0 + wm * 32 + a * 16 + 4 * fq + j;
                if (row < rows) out[(long long)row * ld + col] = acc[a][b][j];
            }
    }
}
