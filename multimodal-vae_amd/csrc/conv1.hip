// First layer of the MultiMNIST image encoder on the matrix cores: Conv2d(1, 32, 4, 2, 1) on a 50x50 image + Swish, and its
// weight gradient (multimnist/model.py:160-161).
//
// Before: im2col_small_kernel (fp32 image -> bf16 patches in HBM) + a gather GEMM with K = 16 (10 TFLOP/s: 16 of the 64 k
// columns of a tile are real) forward, and a streamed weight gradient over the same patches as the LAST kernel of the backward
// chain -- 41 us of the main chain for 0.5 GFLOP.  Here the image sits in LDS as bf16 with a zero halo, the patch matrix (625 x 16)
// is built there once, and
//   forward      r1[pixel][32] = patch[pixel][16 taps] . W[16 taps][32]     one 32x32x16 MFMA per 32 pixels; raw and Swish
//                                                                            copies leave through the conv kernels' epilogue;
//                                                                            two workgroups per image (thin_split_geo.h)
//   weight grad  dW[32][16 taps] = d1[pixel][32]^T . patch[pixel][16]       transposed LDS reads, k = 640 pixel rows over the
//                                                                            waves, per-image partial added with float atomics
//                                                                            (256 x 512 adds: no slab, no reduce launch on the tail);
//                                                                            one workgroup per image: the atomics of a second one
//                                                                            per image (3 us) cost what its overlap saves
#include "thin.h"
#include "convres_epi.h"
#include "thin_split_geo.h"

namespace {

constexpr int C1_IMG = 50, C1_OH = 25, C1_NPIX = 625, C1_TILES = 20, C1_ROWS = 640, C1_C = 32;
constexpr int C1_HW = 52;              // image rows / columns with a zero halo
constexpr int C1_PP = 48;              // patches: bytes per pixel (16 bf16 + 16)
constexpr int C1_AP = 80;              // gradient tile: bytes per pixel (32 bf16 + 16)
static_assert(c1s::IMG == C1_IMG && c1s::OH == C1_OH && c1s::NPIX == C1_NPIX && c1s::C == C1_C && c1s::HALVES * c1s::TILES == C1_TILES &&
              c1s::PP == C1_PP, "thin_split_geo.h describes this layer");

typedef __attribute__((address_space(3))) s16x4 lds_s16x4e;
__device__ __forceinline__ bf16x8 tr_pair_e(const char* a0, const char* a1) {
    union { struct { s16x4 a, b; } s; bf16x8 v; } u;
    u.s.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4e*)a0);
    u.s.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4e*)a1);
    return u.v;
}

// image (fp32, global) -> bf16 with halo in LDS; patches[pixel][tap] = image(2oy-1+kh, 2ox-1+kw) (padding rows zero)
template <int NTHR>
__device__ __forceinline__ void c1_patches(const float* img, bf16* img_s, char* pat_s, int tid) {
    for (int i = tid; i < C1_HW * C1_HW; i += NTHR) {
        const int y = i / C1_HW - 1, x = i - (y + 1) * C1_HW - 1;
        img_s[i] = ((unsigned)y < (unsigned)C1_IMG && (unsigned)x < (unsigned)C1_IMG) ? (bf16)img[y * C1_IMG + x] : (bf16)0.f;
    }
    __syncthreads();
    for (int px = tid; px < C1_ROWS; px += NTHR) {
        bf16x8 lo, hi;
        if (px < C1_NPIX) {
            const int oy = px / C1_OH, ox = px - oy * C1_OH;
            const bf16* d0 = img_s + (2 * oy) * C1_HW + 2 * ox;          // (2oy-1+kh) + 1 halo row, (2ox-1+kw) + 1 halo column
#pragma unroll
            for (int kw = 0; kw < 4; ++kw) {
                lo[kw] = d0[kw]; lo[4 + kw] = d0[C1_HW + kw];
                hi[kw] = d0[2 * C1_HW + kw]; hi[4 + kw] = d0[3 * C1_HW + kw];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) { lo[j] = (bf16)0.f; hi[j] = (bf16)0.f; }
        }
        *reinterpret_cast<bf16x8*>(pat_s + px * C1_PP) = lo;
        *reinterpret_cast<bf16x8*>(pat_s + px * C1_PP + 16) = hi;
    }
    __syncthreads();
}

struct Conv1WgradArgs { const float* image; int B; const bf16* d1; float* dWp; int Kpad; };

constexpr int C1W_WAVES = 8, C1W_NTHR = C1W_WAVES * 64;
constexpr int C1W_OFF_D = 0, C1W_OFF_IMG = C1W_OFF_D + C1_ROWS * C1_AP, C1W_OFF_PAT = C1W_OFF_IMG + ((C1_HW * C1_HW * 2 + 15) / 16) * 16,
              C1W_OFF_RED = C1W_OFF_PAT + C1_ROWS * C1_PP, C1W_LDS = C1W_OFF_RED + C1W_WAVES * C1_C * 16 * 4;

__global__ __launch_bounds__(C1W_NTHR) void conv1_wgrad_mfma_kernel(const Conv1WgradArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int n = blockIdx.x;
    char* const D_s = smem + C1W_OFF_D;
    // gradient image [625][32] -> LDS rows of 80 bytes (padding rows zero)
    {
        constexpr int NV = C1_NPIX * 4;
        const bf16* src = a.d1 + (size_t)n * C1_NPIX * C1_C;
        for (int v = tid; v < C1_ROWS * 4; v += C1W_NTHR) {
            i32x4c val = {0, 0, 0, 0};
            if (v < NV) val = *reinterpret_cast<const i32x4c*>(src + (size_t)v * 8);
            *reinterpret_cast<i32x4c*>(D_s + (v >> 2) * C1_AP + (v & 3) * 16) = val;
        }
    }
    c1_patches<C1W_NTHR>(a.image + (size_t)n * (C1_IMG * C1_IMG), reinterpret_cast<bf16*>(smem + C1W_OFF_IMG), smem + C1W_OFF_PAT, tid);
    // dW[ch][tap] = sum over pixel rows: A[i = ch][k = pixel] from the gradient tile, B[k = pixel][j = tap] from the patches
    const int g4 = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    f32x16 acc;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    for (int ks = wave; ks < C1_ROWS / 16; ks += C1W_WAVES) {
        const int row = ks * 16 + 8 * h + q;
        const char* a0 = D_s + row * C1_AP + (16 * (g4 & 1) + 4 * p) * 2;
        const char* b0 = smem + C1W_OFF_PAT + row * C1_PP + (4 * p) * 2;          // taps 0..15 for both column halves (16..31 unused)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_pair_e(a0, a0 + 4 * C1_AP), tr_pair_e(b0, b0 + 4 * C1_PP), acc, 0, 0, 0);
    }
    float* wred = reinterpret_cast<float*>(smem + C1W_OFF_RED) + wave * (C1_C * 16);
    if (r < 16) {                                            // lane = tap, register j = channel (j&3) + 8*(j>>2) + 4h
#pragma unroll
        for (int j = 0; j < 16; ++j) wred[((j & 3) + 8 * (j >> 2) + 4 * h) * 16 + r] = acc[j];
    }
    __syncthreads();
    {
        const float* wr = reinterpret_cast<const float*>(smem + C1W_OFF_RED);
        for (int i = tid; i < C1_C * 16; i += C1W_NTHR) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < C1W_WAVES; ++w) s += wr[w * C1_C * 16 + i];
            atomicAdd(a.dWp + (size_t)(i >> 4) * a.Kpad + (i & 15), s);        // packed gradient [channel][Kpad], k = tap
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Forward on half images (thin_split_geo.h): two workgroups per image, so that at B = 256 every CU holds two independent
// workgroups whose load / barrier stalls overlap.  A workgroup loads the 27 image rows its 320 pixels read as 8-byte vectors, all
// in flight before the first LDS write, and builds its half of the patch matrix with two threads per pixel.
// `vec`: the image pointer is 8-byte aligned (else: two 4-byte loads per pair)
struct Conv1FwdArgs { const float* image; int B; const bf16* Wp; int Kpad; bf16* r1; bf16* a1; };

template <int NTHR>
struct C1sImage {
    static constexpr int IT = (c1s::LD_VEC + NTHR - 1) / NTHR;
    float2 v[IT];
    __device__ __forceinline__ void fetch(const float* img, int z, int tid, bool vec) {
        const float* src = img + c1s::ld_row0(z) * c1s::IMG;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = tid + it * NTHR;
            v[it] = float2{0.f, 0.f};
            if (i < c1s::LD_VEC) {
                if (vec) v[it] = *reinterpret_cast<const float2*>(src + 2 * i);
                else v[it] = float2{src[2 * i], src[2 * i + 1]};
            }
        }
    }
    // -> bf16 rows with the zero halo; then patches[local pixel][tap] = image(2oy-1+kh, 2ox-1+kw); rows past the image's pixels zero
    __device__ __forceinline__ void stage(bf16* img_s, char* pat_s, int z, int tid) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = tid + it * NTHR;
            if (i < c1s::LD_VEC) {
                const int lr = i / (c1s::IMG / 2), c = i - lr * (c1s::IMG / 2);              // (one multiply-shift per 8-byte vector)
                bf16x2 o;
                o[0] = (bf16)v[it].x; o[1] = (bf16)v[it].y;
                *reinterpret_cast<bf16x2*>(img_s + c1s::cell(z, c1s::ld_row0(z) + lr, 2 * c)) = o;
            }
        }
        {   // the halo: cells 0, 1 and 52, 53 of every row, and the one staged row outside the image (cells no load writes)
            unsigned* w = reinterpret_cast<unsigned*>(img_s);
            if (tid < c1s::IROWS) { w[tid * (c1s::IW / 2)] = 0u; w[tid * (c1s::IW / 2) + c1s::IW / 2 - 1] = 0u; }
            if (tid >= 32 && tid < 32 + c1s::IW / 2) w[c1s::pad_row(z) * (c1s::IW / 2) + tid - 32] = 0u;
        }
        __syncthreads();
        const int np = c1s::npix(z);
        for (int i = tid; i < 2 * c1s::PIX; i += NTHR) {
            const int lp = i >> 1, half = i & 1;
            bf16x8 o;
            if (lp < np) {
                const bf16* d0 = img_s + c1s::window(z, lp, half);
#pragma unroll
                for (int kw = 0; kw < 4; ++kw) { o[kw] = d0[kw]; o[4 + kw] = d0[c1s::IW + kw]; }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (bf16)0.f;
            }
            *reinterpret_cast<bf16x8*>(pat_s + lp * c1s::PP + half * 16) = o;
        }
        __syncthreads();
    }
};

__global__ __launch_bounds__(c1s::F_NTHR) void conv1_fwd_half_kernel(const Conv1FwdArgs a, const bool vec) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int n = blockIdx.x, z = blockIdx.y;
    C1sImage<c1s::F_NTHR> im;
    im.fetch(a.image + (size_t)n * (C1_IMG * C1_IMG), z, tid, vec);
    // B[k = tap][j = channel]: packed weights [32][Kpad], k = tap
    const bf16x8 wb = *reinterpret_cast<const bf16x8*>(a.Wp + (size_t)r * a.Kpad + 8 * h);
    im.stage(reinterpret_cast<bf16*>(smem + c1s::F_OFF_IMG), smem + c1s::F_OFF_PAT, z, tid);
    const size_t bytes = (size_t)a.B * C1_NPIX * C1_C * 2;
    const __amdgpu_buffer_rsrc_t rsrc_r = __builtin_amdgcn_make_buffer_rsrc(a.r1, 0, (int)bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(a.a1, 0, (int)bytes, 0x00020000);
    char* const scr = smem + c1s::F_OFF_SCR + wave * 2560;
    float s1 = 0.f, s2 = 0.f;
    for (int tl = wave; tl < c1s::TILES; tl += c1s::F_WAVES) {
        const int t = z * c1s::TILES + tl;                   // tile of the image
        f32x16 acc;
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0.f;
        const bf16x8 pa = *reinterpret_cast<const bf16x8*>(smem + c1s::F_OFF_PAT + (tl * 32 + r) * c1s::PP + h * 16);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa, wb, acc, 0, 0, 0);
        const unsigned base = (unsigned)(((size_t)n * C1_NPIX + t * 32) * (C1_C * 2)) + (unsigned)((lane >> 4) * 16);
        const int p0 = t * 32 + (lane & 15), p1 = p0 + 16;
        const unsigned off0 = p0 < C1_NPIX ? base + (unsigned)((lane & 15) * (C1_C * 2)) : 0x40000000u;
        const unsigned off1 = p1 < C1_NPIX ? base + (unsigned)((16 + (lane & 15)) * (C1_C * 2)) : 0x40000000u;
        f32x16 act;
#pragma unroll
        for (int j = 0; j < 16; ++j) act[j] = swish_fast(acc[j]);
        // (rows past the image carry an out-of-range offset: dropped; the sums of the epilogue are not used here)
        cr_epilogue_tile<0, false>(acc, scr, lane, 32, off0, off1, rsrc_r, rsrc_r, 1.f, 0.f, 0.f, 0.f, s1, s2, true);
        cr_epilogue_tile<0, false>(act, scr, lane, 32, off0, off1, rsrc_a, rsrc_a, 1.f, 0.f, 0.f, 0.f, s1, s2, true);
    }
}

}  // namespace

int launch_conv1_fwd_mfma(const float* image, int B, const bf16* Wp, int Kpad, bf16* r1, bf16* a1, hipStream_t s) {
    MMVAE_REQUIRE(image && Wp && r1 && a1 && Kpad >= 16 && (size_t)B * C1_NPIX * C1_C * 2 < 0x40000000ull, "conv1 fwd: arguments");
    Conv1FwdArgs a{image, B, Wp, Kpad, r1, a1};
    const bool vec = reinterpret_cast<uintptr_t>(image) % 8 == 0;
    MMVAE_LAUNCH(conv1_fwd_half_kernel, dim3(B, c1s::HALVES), dim3(c1s::F_NTHR), c1s::F_LDS, s, a, vec);
    return mmvae_check_launch("conv1_fwd_half");
}
int launch_conv1_wgrad_mfma(const float* image, int B, const bf16* d1, float* dWp, int Kpad, hipStream_t s) {
    MMVAE_REQUIRE(image && d1 && dWp && Kpad >= 16, "conv1 wgrad: arguments");
    static std::atomic<unsigned> attr_set{0};
    if (mmvae_first_use_on_device(attr_set))
        hipFuncSetAttribute(reinterpret_cast<const void*>(&conv1_wgrad_mfma_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, C1W_LDS);
    Conv1WgradArgs a{image, B, d1, dWp, Kpad};
    MMVAE_LAUNCH(conv1_wgrad_mfma_kernel, dim3(B), dim3(C1W_NTHR), C1W_LDS, s, a);
    return mmvae_check_launch("conv1_wgrad_mfma");
}
