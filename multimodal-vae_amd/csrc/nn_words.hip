// See nn_words.h.
#include "nn_words.h"
#include <math.h>

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) float f32x2;

constexpr int D = NNW_DIM, TQ = NNW_TQ, TV = NNW_TV;
constexpr int NTHR = 512;                       // 8 waves: 2 per SIMD
constexpr int ROW_V4 = D / 4;                   // 75 16-byte pieces per table row
constexpr int TILE_V4 = TV * ROW_V4;            // 2400 per vocabulary tile
constexpr int STAGE = (TILE_V4 + NTHR - 1) / NTHR;   // 5 staged pieces per thread
// LDS row stride in floats.  The B operand of a lane (column j = lane % 32, half h = lane / 32) is an 8-byte read at float
// j * LDW + 4 m + 2 h, and the compiler pairs the reads of m and m + 1 into one ds_read2_b64.  That instruction is served in
// groups of 16 consecutive lanes with banks (address / 4) % 32, two banks per lane: j * LDW % 32 has to be 16 distinct even
// numbers over 16 consecutive j -- LDW = 2 * odd (302: 14 j % 32).  The same stride is conflict-free for a lone ds_read_b64
// (32-lane groups, banks % 64: 46 j % 64 are 32 distinct even numbers).
constexpr int LDW = 302;
constexpr int LDS_BYTES = 2 * TV * LDW * (int)sizeof(float);
static_assert(D % 4 == 0 && (LDW / 2) % 2 == 1 && LDW >= D, "tile layout");

struct NnwPair { float score; int index; };     // index -1: nothing seen (an empty split, or every score NaN)

// (s, i) <- the better of (s, i) and (os, oi): smaller score, lowest index on equal scores.  -1 compares as the largest index.
__device__ __forceinline__ void take_better(float& s, int& i, float os, int oi) {
    if (os < s || (os == s && (unsigned)oi < (unsigned)i)) { s = os; i = oi; }
}

// sum_k (q_k - w_k)^2 (q == nullptr: sum_k w_k^2) by the 16 lanes of a group; every lane of the group returns it.  Lane `sub`
// takes the 16-byte pieces sub, sub + 16, ... of the row as one fmaf chain in that order, then a 4-level xor butterfly: one
// fixed summation order per (q, w) pair, whoever calls.  All 64 lanes of the wave must be here.
__device__ __forceinline__ float group16_sqdist(const float* __restrict__ q, const float* __restrict__ w, int sub) {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < (ROW_V4 + 15) / 16; ++i) {
        const int c = sub + 16 * i;
        if (c < ROW_V4) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(w + 4 * c);
            f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
            if (q) a = *reinterpret_cast<const f32x4*>(q + 4 * c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = q ? a[e] - b[e] : b[e];
                acc = fmaf(d, d, acc);
            }
        }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    return acc;
}

// ---------------------------------------------------------------------------------------------- norms
__global__ __launch_bounds__(NTHR) void nn_words_norms_kernel(const float* __restrict__ W, long long V, float* __restrict__ sqn) {
    const int sub = threadIdx.x & 15;
    const long long v = (long long)blockIdx.x * (NTHR / 16) + (threadIdx.x >> 4);
    const long long vc = v < V ? v : V - 1;
    const float s = group16_sqdist(nullptr, W + (size_t)vc * D, sub);
    if (sub == 0 && v < V) sqn[v] = s;
}

// ---------------------------------------------------------------------------------------------- direct distances
__global__ __launch_bounds__(NTHR) void nn_words_dists_kernel(const float* __restrict__ Q, int n, const float* __restrict__ W, long long V,
                                                              float* __restrict__ dist) {
    const int sub = threadIdx.x & 15;
    const long long v = (long long)blockIdx.x * (NTHR / 16) + (threadIdx.x >> 4);
    const long long vc = v < V ? v : V - 1;
    const float* w = W + (size_t)vc * D;
    for (int qi = 0; qi < n; ++qi) {
        const float s = group16_sqdist(Q + (size_t)qi * D, w, sub);
        if (sub == 0 && v < V) dist[(size_t)qi * (size_t)V + (size_t)v] = sqrtf(s);
    }
}

// ---------------------------------------------------------------------------------------------- nearest: the sweep
// grid (query blocks, splits).  Split sp of S covers the word tiles [T sp / S, T (sp + 1) / S) of T = ceil(V / TV).
// Wave w of the workgroup owns query rows 32 w .. 32 w + 31 of the block: they are its MFMA A operands, loaded once (150
// registers).  The vocabulary tile goes through LDS, double-buffered: the loads of tile t + 1 are issued before the MFMAs of
// tile t and land in LDS after them, one barrier per tile.  Table addresses are a 64-bit tile base plus an in-tile offset.
// k order of the chain of every (query, word) pair: for m = 0..74: 4m, 4m+2, 4m+1, 4m+3 (half h of the wave supplies
// k = 4m + 2h and 4m + 2h + 1 as one 8-byte LDS read; an MFMA consumes one k of each half, the lower half's first).
__global__ __launch_bounds__(NTHR) void nn_words_nearest_kernel(const float* __restrict__ Q, int N, const float* __restrict__ W,
                                                                const float* __restrict__ sqn, long long V, int ntiles,
                                                                NnwPair* __restrict__ ws, int npad) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int S = gridDim.y, sp = blockIdx.y;
    const int t0 = (int)((long long)ntiles * sp / S), t1 = (int)((long long)ntiles * (sp + 1) / S);
    const int q0 = blockIdx.x * TQ + wave * 32;
    const bool wave_on = q0 < N;                                  // uniform per wave

    float a[2 * ROW_V4];
    {
        const int qrow = q0 + j;
        const bool ok = qrow < N;
        const float* qp = Q + (size_t)(ok ? qrow : N - 1) * D + 2 * h;
#pragma unroll
        for (int m = 0; m < ROW_V4; ++m) {
            const f32x2 v = *reinterpret_cast<const f32x2*>(qp + 4 * m);
            a[2 * m] = ok ? v.x : 0.f;
            a[2 * m + 1] = ok ? v.y : 0.f;
        }
    }

    float best[16];
    int bidx[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { best[r] = INFINITY; bidx[r] = -1; }

    f32x4 st[STAGE];
    // rows past the end of the table are loaded as copies of its last row (no predicated loads) and masked in the epilogue
    auto load_tile = [&](int t) {
        const long long v0 = (long long)t * TV;
        const long long left = V - 1 - v0;
        const int last = left < TV - 1 ? (int)left : TV - 1;
        const float* base = W + (size_t)v0 * D;
#pragma unroll
        for (int it = 0; it < STAGE; ++it) {
            const int f = tid + NTHR * it;
            if (it < STAGE - 1 || f < TILE_V4) {
                int jr = f / ROW_V4;
                const int c = f - jr * ROW_V4;
                jr = jr < last ? jr : last;
                st[it] = *reinterpret_cast<const f32x4*>(base + jr * D + 4 * c);
            }
        }
    };
    auto store_tile = [&](float* buf) {
#pragma unroll
        for (int it = 0; it < STAGE; ++it) {
            const int f = tid + NTHR * it;
            if (it < STAGE - 1 || f < TILE_V4) {
                const int jr = f / ROW_V4, c = f - jr * ROW_V4;
                f32x2* p = reinterpret_cast<f32x2*>(buf + jr * LDW + 4 * c);
                p[0] = f32x2{st[it][0], st[it][1]};
                p[1] = f32x2{st[it][2], st[it][3]};
            }
        }
    };

    if (t0 < t1) {                                                // uniform per workgroup
        load_tile(t0);
        store_tile(lds);
        __syncthreads();
        for (int t = t0; t < t1; ++t) {
            float* cur = lds + ((t - t0) & 1) * (TV * LDW);
            float* nxt = lds + (((t - t0) & 1) ^ 1) * (TV * LDW);
            const bool more = t + 1 < t1;
            if (more) load_tile(t + 1);
            if (wave_on) {
                const long long v = (long long)t * TV + j;
                const bool vok = v < V;
                const float sq = sqn[vok ? v : V - 1];
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                const float* bp = cur + j * LDW + 2 * h;
#pragma unroll
                for (int m = 0; m < ROW_V4; ++m) {
                    const f32x2 b = *reinterpret_cast<const f32x2*>(bp + 4 * m);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * m], b.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * m + 1], b.y, acc, 0, 0, 0);
                }
                const int vi = (int)v;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float sc = vok ? fmaf(-2.f, acc[r], sq) : INFINITY;
                    if (sc < best[r]) { best[r] = sc; bidx[r] = vi; }      // tiles ascend: the first of equal scores stays
                }
            }
            if (more) store_tile(nxt);
            __syncthreads();
        }
    }

    // accumulator register r of lane (j, h) is query row (r & 3) + 8 (r >> 2) + 4 h, word column j: reduce over the 32 columns
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float s = best[r];
        int i = bidx[r];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            const float os = __shfl_xor(s, o, 64);
            const int oi = __shfl_xor(i, o, 64);
            take_better(s, i, os, oi);
        }
        if (j == 0) {
            const int row = q0 + (r & 3) + 8 * (r >> 2) + 4 * h;  // < npad: the workspace holds whole query blocks
            ws[(size_t)sp * npad + row] = NnwPair{s, i};
        }
    }
}

// ---------------------------------------------------------------------------------------------- nearest: merge + distance
// 16 lanes per query: lane `sub` folds the splits sub, sub + 16, ... in ascending order, a butterfly folds the 16 partial
// winners (the rule is associative and commutative: any order gives the same pair), then the group recomputes the distance.
__global__ __launch_bounds__(NTHR) void nn_words_merge_kernel(const float* __restrict__ Q, int N, const float* __restrict__ W,
                                                              const NnwPair* __restrict__ ws, int npad, int S,
                                                              long long* __restrict__ index, float* __restrict__ dist) {
    const int sub = threadIdx.x & 15;
    const int qi = blockIdx.x * (NTHR / 16) + (threadIdx.x >> 4);
    const int qc = qi < N ? qi : N - 1;
    float s = INFINITY;
    int i = -1;
    for (int sp = sub; sp < S; sp += 16) {
        const NnwPair p = ws[(size_t)sp * npad + qc];
        take_better(s, i, p.score, p.index);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        const float os = __shfl_xor(s, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        take_better(s, i, os, oi);
    }
    if (i < 0) i = 0;                                             // a query with NaN scores only: word 0, distance NaN
    const float d2 = group16_sqdist(Q + (size_t)qc * D, W + (size_t)i * D, sub);
    if (sub == 0 && qi < N) {
        index[qi] = i;
        dist[qi] = sqrtf(d2);
    }
}

}  // namespace

int nn_words_splits(int n_queries, long long n_words) {
    const long long qblocks = (n_queries + TQ - 1) / TQ, tiles = (n_words + TV - 1) / TV;
    long long s = 1024 / qblocks;                                 // at most 1024 workgroups: 4 full rounds of 256 CUs
    if (s > NNW_MAX_SPLITS) s = NNW_MAX_SPLITS;
    if (s > tiles) s = tiles;
    return s < 1 ? 1 : (int)s;
}

size_t nn_words_workspace_bytes(int n_queries, long long n_words) {
    const size_t qblocks = (size_t)((n_queries + TQ - 1) / TQ);
    return (size_t)nn_words_splits(n_queries, n_words) * qblocks * TQ * sizeof(NnwPair);
}

int launch_nn_words_norms(const float* table, long long n_words, float* sqnorm, hipStream_t s) {
    MMVAE_REQUIRE(aligned16(table), "nn_words_norms: the table must be 16-byte aligned");
    const long long blocks = (n_words + NTHR / 16 - 1) / (NTHR / 16);
    MMVAE_REQUIRE(blocks <= 0x7FFFFFFFll, "nn_words_norms: n_words = %lld is too large", n_words);
    MMVAE_LAUNCH(nn_words_norms_kernel, dim3((unsigned)blocks), dim3(NTHR), 0, s, table, n_words, sqnorm);
    return mmvae_check_launch("nn_words_norms");
}

int launch_nn_words_dists(const float* queries, int n_queries, const float* table, long long n_words, float* dist, hipStream_t s) {
    MMVAE_REQUIRE(aligned16(table) && aligned16(queries), "nn_words_dists: table and queries must be 16-byte aligned");
    const long long blocks = (n_words + NTHR / 16 - 1) / (NTHR / 16);
    MMVAE_REQUIRE(blocks <= 0x7FFFFFFFll, "nn_words_dists: n_words = %lld is too large", n_words);
    MMVAE_LAUNCH(nn_words_dists_kernel, dim3((unsigned)blocks), dim3(NTHR), 0, s, queries, n_queries, table, n_words, dist);
    return mmvae_check_launch("nn_words_dists");
}

int launch_nn_words_nearest(const float* queries, int n_queries, const float* table, const float* sqnorm, long long n_words,
                            void* ws, long long* index, float* dist, hipStream_t s) {
    MMVAE_REQUIRE(aligned16(table) && aligned16(queries) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
                  "nn_words_nearest: table and queries must be 16-byte aligned, the workspace 8-byte aligned");
    // word indices travel as int32 inside the sweep (the table itself is addressed in 64 bits)
    MMVAE_REQUIRE(n_words <= 0x7FFFFFFFll - TV, "nn_words_nearest: n_words = %lld is too large", n_words);
    static std::atomic<unsigned> attr_set{0};
    if (mmvae_first_use_on_device(attr_set))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&nn_words_nearest_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    const int qblocks = ceil_div(n_queries, TQ), npad = qblocks * TQ;
    const int ntiles = (int)((n_words + TV - 1) / TV);
    const int S = nn_words_splits(n_queries, n_words);
    mmvae_count_flops(2.0 * D * (double)n_queries * (double)n_words);
    MMVAE_LAUNCH(nn_words_nearest_kernel, dim3(qblocks, S), dim3(NTHR), LDS_BYTES, s, queries, n_queries, table, sqnorm, n_words, ntiles,
                 reinterpret_cast<NnwPair*>(ws), npad);
    MMVAE_TRY(mmvae_check_launch("nn_words_nearest"));
    MMVAE_LAUNCH(nn_words_merge_kernel, dim3(ceil_div(n_queries, NTHR / 16)), dim3(NTHR), 0, s, queries, n_queries, table,
                 reinterpret_cast<const NnwPair*>(ws), npad, S, index, dist);
    return mmvae_check_launch("nn_words_merge");
}
