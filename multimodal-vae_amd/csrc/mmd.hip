// See mmd.h.
#include "mmd.h"
#include <math.h>
#include <algorithm>

namespace {

constexpr int RT = MMD_RT, CT = MMD_CT, NTHR = 256, SUB = 8;
static_assert(NTHR == 4 * RT, "4 lanes per row");

// Lane q of a row's 4 lanes owns the 16-byte coordinate chunks q, q + 4, ..., q + 4 (M - 1): M = ceil(ceil(D / 4) / 4).
// A tile row in LDS is 16 M floats, coordinates past D are zero on both sides (d = 0 leaves every chain as it is).
template <int M>
__device__ __forceinline__ void load_row(const float* __restrict__ p, int D, int q, float (&r)[M][4]) {
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int e = 4 * (q + 4 * m) + v;
            r[m][v] = e < D ? p[e] : 0.f;
        }
}

// rows [j0, j0 + CT) of C (n rows of D floats) -> buf[CT][16 M], zero-filled past D and past n
template <int M>
__device__ __forceinline__ void stage_tile(const float* __restrict__ C, int n, int D, int j0, float* __restrict__ buf) {
    constexpr int LD = 16 * M;
    for (int idx = threadIdx.x; idx < CT * LD; idx += NTHR) {
        const int j = idx / LD, e = idx - j * LD, col = j0 + j;
        buf[idx] = (e < D && col < n) ? C[(size_t)col * D + e] : 0.f;
    }
}

// d = r - c for this lane's chunks, the squared distance of the pair in every one of the row's 4 lanes (bitwise the same)
template <int M>
__device__ __forceinline__ float pair_sqdist(const float (&r)[M][4], const float* __restrict__ crow, int q, float (&d)[M][4]) {
    const f32x4* cp = reinterpret_cast<const f32x4*>(crow) + q;
    float acc = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const f32x4 c = cp[4 * m];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            d[m][v] = r[m][v] - c[v];
            acc = fmaf(d[m][v], d[m][v], acc);
        }
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    return acc;
}

// coco/model.py:394: exp(-mean(diff^2, dim=2) / dim)
__device__ __forceinline__ float pair_kernel(float sq, float fD) { return expf(-((sq / fD) / fD)); }

// ---------------------------------------------------------------------------------------------- the sweep
// grid (row tiles of x then of y, splits over x's column tiles then over y's).  Split c of a class's Sc covers its tiles
// [T c / Sc, T (c + 1) / Sc).
// GRAD: MMD_VALUE no gradient sums | MMD_GRAD_XY both classes' | MMD_GRAD_Y the y rows' alone (mmd.h launch_mmd_dy): the x row tiles run
// the value form (kernel sums, no k * d work, nothing written to Gp), the y row tiles the gradient form into a Gp of y's rows only.
// The branch is uniform per workgroup; per pair, per 8 columns and per split the arithmetic and its order are the same in every mode.
enum { MMD_VALUE = 0, MMD_GRAD_XY = 1, MMD_GRAD_Y = 2 };
template <int M, int MODE>
__global__ __launch_bounds__(NTHR) void mmd_pairs_kernel(const float* __restrict__ X, int nx, const float* __restrict__ Y, int ny, int D,
                                                         int rtx, int tx, int ty, int sx, long long rpad,
                                                         double* __restrict__ Sp, double* __restrict__ Gp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int LD = 16 * M;
    const int tid = threadIdx.x, q = tid & 3, il = tid >> 2;
    const int rt = blockIdx.x, sp = blockIdx.y, S = gridDim.y;
    const bool rowy = rt >= rtx, coly = sp >= sx;
    const bool GRAD = MODE == MMD_GRAD_XY || (MODE == MMD_GRAD_Y && rowy);
    if (MODE == MMD_VALUE && rowy && !coly) return;                           // k(y_j, x_i) = k(x_i, y_j): only the gradient needs this quarter
    const float* R = rowy ? Y : X;
    const float* C = coly ? Y : X;
    const int nr = rowy ? ny : nx, nc = coly ? ny : nx;
    const int T = coly ? ty : tx, Sc = coly ? S - sx : sx, sc = coly ? sp - sx : sp;
    const int t0 = (int)((long long)T * sc / Sc), t1 = (int)((long long)T * (sc + 1) / Sc);
    const int row = (rowy ? rt - rtx : rt) * RT + il;
    const bool rok = row < nr;                                    // rows past the end compute a copy of the last row, unwritten
    const float fD = (float)D;

    float r[M][4];
    load_row<M>(R + (size_t)(rok ? row : nr - 1) * D, D, q, r);
    double gs[M][4];
    double ss = 0.0;
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int v = 0; v < 4; ++v) gs[m][v] = 0.0;

    stage_tile<M>(C, nc, D, t0 * CT, lds);
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
        const float* cur = lds + ((t - t0) & 1) * (CT * LD);
        float* nxt = lds + (((t - t0) & 1) ^ 1) * (CT * LD);
        if (t + 1 < t1) stage_tile<M>(C, nc, D, (t + 1) * CT, nxt);
        const int jn = min(CT, nc - t * CT);
        for (int jb = 0; jb < jn; jb += SUB) {
            const int je = min(jb + SUB, jn);
            float gb[M][4];
            float sb = 0.f;
#pragma unroll
            for (int m = 0; m < M; ++m)
#pragma unroll
                for (int v = 0; v < 4; ++v) gb[m][v] = 0.f;
            for (int j = jb; j < je; ++j) {
                float d[M][4];
                const float k = pair_kernel(pair_sqdist<M>(r, cur + j * LD, q, d), fD);
                sb += k;
                if (GRAD) {
#pragma unroll
                    for (int m = 0; m < M; ++m)
#pragma unroll
                        for (int v = 0; v < 4; ++v) gb[m][v] = fmaf(k, d[m][v], gb[m][v]);
                }
            }
            ss += (double)sb;
            if (GRAD) {
#pragma unroll
                for (int m = 0; m < M; ++m)
#pragma unroll
                    for (int v = 0; v < 4; ++v) gs[m][v] += (double)gb[m][v];
            }
        }
        __syncthreads();
    }

    if (rok) {
        size_t slot = (size_t)sp * (size_t)rpad + (size_t)rt * RT + il;            // < (sx + sy) * rpad
        if (q == 0) Sp[slot] = ss;
        if (MODE == MMD_GRAD_Y) slot = (size_t)sp * ((size_t)rpad - (size_t)rtx * RT) + (size_t)(rt - rtx) * RT + il;   // y's rows alone
        if (GRAD) {
#pragma unroll
            for (int m = 0; m < M; ++m)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int e = 4 * (q + 4 * m) + v;
                    if (e < D) Gp[slot * D + e] = gs[m][v];
                }
        }
    }
}

// ---------------------------------------------------------------------------------------------- the fold
// block 0: the three means and MMD; blocks 1..: one gradient element per thread.  Everything in float64, splits in ascending order.
// the three means and MMD by one workgroup: out4 = {mean Kxx, mean Kyy, mean Kxy, MMD}
__device__ __forceinline__ void fold_values(const double* __restrict__ Sp, int nx, int ny, int rtx, int sx, int S, long long rpad,
                                            double (&red)[3][NTHR], float* __restrict__ out4) {
    const int tid = threadIdx.x;
    double axx = 0.0, axy = 0.0, ayy = 0.0;
    for (long long i = tid; i < (long long)nx * S; i += NTHR) {
        const int s = (int)(i / nx), row = (int)(i - (long long)s * nx);
        const double v = Sp[(size_t)s * rpad + row];
        if (s < sx) axx += v; else axy += v;
    }
    for (long long i = tid; i < (long long)ny * (S - sx); i += NTHR) {
        const int s = (int)(i / ny), row = (int)(i - (long long)s * ny);
        ayy += Sp[(size_t)(sx + s) * rpad + (size_t)rtx * RT + row];
    }
    red[0][tid] = axx; red[1][tid] = ayy; red[2][tid] = axy;
    __syncthreads();
    for (int o = NTHR / 2; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int c = 0; c < 3; ++c) red[c][tid] += red[c][tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double kxx = red[0][0] / ((double)nx * (double)nx), kyy = red[1][0] / ((double)ny * (double)ny);
        const double kxy = red[2][0] / ((double)nx * (double)ny);
        out4[0] = (float)kxx; out4[1] = (float)kyy; out4[2] = (float)kxy;
        out4[3] = (float)((kxx + kyy) - 2.0 * kxy);
    }
}
// one gradient element of row `row` of class rowy: G = the [S][prows][D] partial sums, prow the row's place in a split's slab
__device__ __forceinline__ double fold_grad(const double* __restrict__ G, size_t prows, size_t prow, int e, bool rowy, int nx, int ny, int D,
                                            int sx, int S) {
    double a = 0.0, b = 0.0;                                      // sums against x's columns, against y's
    for (int s = 0; s < sx; ++s) a += G[((size_t)s * prows + prow) * D + e];
    for (int s = sx; s < S; ++s) b += G[((size_t)s * prows + prow) * D + e];
    const double dd = (double)D * (double)D, na = rowy ? ny : nx;
    const double same = -4.0 / (na * na * dd), cross = 4.0 / ((double)nx * (double)ny * dd);
    return rowy ? cross * a + same * b : same * a + cross * b;
}
__global__ __launch_bounds__(NTHR) void mmd_fold_kernel(const double* __restrict__ Sp, const double* __restrict__ Gp, int nx, int ny, int D,
                                                        int rtx, int sx, int S, long long rpad, bool grad, float* __restrict__ out4,
                                                        float* __restrict__ dx, float* __restrict__ dy) {
    __shared__ double red[3][NTHR];
    if (blockIdx.x == 0) { fold_values(Sp, nx, ny, rtx, sx, S, rpad, red, out4); return; }
    if (!grad) return;
    const long long gid = (long long)(blockIdx.x - 1) * NTHR + threadIdx.x;
    if (gid >= (long long)(nx + ny) * D) return;
    const int z = (int)(gid / D), e = (int)(gid - (long long)z * D);
    const bool rowy = z >= nx;
    const int row = rowy ? z - nx : z;
    const size_t prow = (rowy ? (size_t)rtx * RT : 0) + row;
    const double g = fold_grad(Gp, (size_t)rpad, prow, e, rowy, nx, ny, D, sx, S);
    float* out = rowy ? dy : dx;
    if (out) out[(size_t)row * D + e] = (float)g;
}
// The fold behind the MMD_GRAD_Y sweep (Gy: [S][rty * RT][D], y's rows alone).  Block 0: the values, as above; blocks 1..: dy =
// scale * dMMD/dy, the product taken in float64 and rounded once (scale = 1: the bits of mmd_fold_kernel's dy).  dy may be null.
__global__ __launch_bounds__(NTHR) void mmd_fold_y_kernel(const double* __restrict__ Sp, const double* __restrict__ Gy, int nx, int ny, int D,
                                                          int rtx, int sx, int S, long long rpad, float scale, float* __restrict__ out4,
                                                          float* __restrict__ dy) {
    __shared__ double red[3][NTHR];
    if (blockIdx.x == 0) { fold_values(Sp, nx, ny, rtx, sx, S, rpad, red, out4); return; }
    const long long gid = (long long)(blockIdx.x - 1) * NTHR + threadIdx.x;
    if (!dy || gid >= (long long)ny * D) return;
    const int row = (int)(gid / D), e = (int)(gid - (long long)row * D);
    const double g = fold_grad(Gy, (size_t)rpad - (size_t)rtx * RT, (size_t)row, e, true, nx, ny, D, sx, S);
    dy[gid] = (float)(g * (double)scale);
}

// ---------------------------------------------------------------------------------------------- the kernel matrix
// grid (row tiles of x, column tiles of y): the sweep's arithmetic, one column tile per workgroup, lane 0 of a row stores
template <int M>
__global__ __launch_bounds__(NTHR) void mmd_kernel_matrix_kernel(const float* __restrict__ X, int nx, const float* __restrict__ Y, int ny, int D,
                                                                 float* __restrict__ K) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int LD = 16 * M;
    const int tid = threadIdx.x, q = tid & 3, il = tid >> 2;
    const int row = blockIdx.x * RT + il, j0 = blockIdx.y * CT;
    const bool rok = row < nx;
    const float fD = (float)D;
    float r[M][4];
    load_row<M>(X + (size_t)(rok ? row : nx - 1) * D, D, q, r);
    stage_tile<M>(Y, ny, D, j0, lds);
    __syncthreads();
    const int jn = min(CT, ny - j0);
    for (int j = 0; j < jn; ++j) {
        float d[M][4];
        const float k = pair_kernel(pair_sqdist<M>(r, lds + j * LD, q, d), fD);
        if (rok && q == 0) K[(size_t)row * ny + j0 + j] = k;
    }
}

inline int steps_of(int dim) { return (ceil_div(dim, 4) + 3) / 4; }          // M: 1..16 for dim 1..256

template <int M, int GRAD>
void launch_pairs(const MmdShape& g, const float* x, int nx, const float* y, int ny, int D, double* Sp, double* Gp, hipStream_t s) {
    constexpr int LDS_BYTES = 2 * CT * 16 * M * (int)sizeof(float);            // at most 64 KB (M = 16)
    MMVAE_LAUNCH((mmd_pairs_kernel<M, GRAD>), dim3(g.rtx + g.rty, g.sx + g.sy), dim3(NTHR), LDS_BYTES, s, x, nx, y, ny, D, g.rtx, g.tx,
                 g.ty, g.sx, g.rpad, Sp, Gp);
}
template <int M>
void launch_matrix(const float* x, int nx, const float* y, int ny, int D, float* k, hipStream_t s) {
    constexpr int LDS_BYTES = CT * 16 * M * (int)sizeof(float);
    MMVAE_LAUNCH((mmd_kernel_matrix_kernel<M>), dim3(ceil_div(nx, RT), ceil_div(ny, CT)), dim3(NTHR), LDS_BYTES, s, x, nx, y, ny, D, k);
}

#define MMD_FOR_M(F) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11) F(12) F(13) F(14) F(15) F(16)

}  // namespace

MmdShape mmd_shape(int n_x, int n_y) {
    MmdShape g;
    g.rtx = ceil_div(n_x, RT); g.rty = ceil_div(n_y, RT);
    g.tx = ceil_div(n_x, CT); g.ty = ceil_div(n_y, CT);
    const int cap = MMD_GRID_TARGET / (g.rtx + g.rty);
    auto splits = [&](int tiles) { const int s = std::min(std::min(tiles, (int)MMD_MAX_SPLITS), cap); return s < 1 ? 1 : s; };
    g.sx = splits(g.tx); g.sy = splits(g.ty);
    g.rpad = (long long)(g.rtx + g.rty) * RT;
    return g;
}

size_t mmd_workspace_bytes(int n_x, int n_y, int dim) {
    const MmdShape g = mmd_shape(n_x, n_y);
    return (size_t)(g.sx + g.sy) * (size_t)g.rpad * (size_t)(1 + dim) * sizeof(double);
}

int launch_mmd(const float* x, int n_x, const float* y, int n_y, int dim, void* ws, float* out4, float* dx, float* dy, hipStream_t s) {
    MMVAE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "mmd: the workspace must be 8-byte aligned");
    const MmdShape g = mmd_shape(n_x, n_y);
    const int S = g.sx + g.sy;
    double* Sp = reinterpret_cast<double*>(ws);
    double* Gp = Sp + (size_t)S * (size_t)g.rpad;
    const bool grad = dx || dy;
    switch (steps_of(dim)) {
#define MMD_CASE(m)                                                                              \
    case m:                                                                                      \
        if (grad) launch_pairs<m, MMD_GRAD_XY>(g, x, n_x, y, n_y, dim, Sp, Gp, s);               \
        else launch_pairs<m, MMD_VALUE>(g, x, n_x, y, n_y, dim, Sp, Gp, s);                      \
        break;
        MMD_FOR_M(MMD_CASE)
#undef MMD_CASE
        default: MMVAE_REQUIRE(false, "mmd: dim = %d", dim);
    }
    MMVAE_TRY(mmvae_check_launch("mmd_pairs"));
    const long long elems = grad ? (long long)(n_x + n_y) * dim : 0;
    MMVAE_LAUNCH(mmd_fold_kernel, dim3((unsigned)(1 + (elems + NTHR - 1) / NTHR)), dim3(NTHR), 0, s, Sp, Gp, n_x, n_y, dim, g.rtx, g.sx, S,
                 g.rpad, grad, out4, dx, dy);
    return mmvae_check_launch("mmd_fold");
}

size_t mmd_dy_workspace_bytes(int n_x, int n_y, int dim) {
    const MmdShape g = mmd_shape(n_x, n_y);
    return (size_t)(g.sx + g.sy) * ((size_t)g.rpad + (size_t)g.rty * RT * (size_t)dim) * sizeof(double);
}

int launch_mmd_dy(const float* x, int n_x, const float* y, int n_y, int dim, void* ws, float scale, float* out4, float* dy, hipStream_t s) {
    MMVAE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "mmd_dy: the workspace must be 8-byte aligned");
    const MmdShape g = mmd_shape(n_x, n_y);
    const int S = g.sx + g.sy;
    double* Sp = reinterpret_cast<double*>(ws);
    double* Gy = Sp + (size_t)S * (size_t)g.rpad;
    switch (steps_of(dim)) {
#define MMD_CASE(m)                                                                              \
    case m:                                                                                      \
        if (dy) launch_pairs<m, MMD_GRAD_Y>(g, x, n_x, y, n_y, dim, Sp, Gy, s);                  \
        else launch_pairs<m, MMD_VALUE>(g, x, n_x, y, n_y, dim, Sp, Gy, s);                      \
        break;
        MMD_FOR_M(MMD_CASE)
#undef MMD_CASE
        default: MMVAE_REQUIRE(false, "mmd_dy: dim = %d", dim);
    }
    MMVAE_TRY(mmvae_check_launch("mmd_pairs_y"));
    const long long elems = dy ? (long long)n_y * dim : 0;
    MMVAE_LAUNCH(mmd_fold_y_kernel, dim3((unsigned)(1 + (elems + NTHR - 1) / NTHR)), dim3(NTHR), 0, s, Sp, Gy, n_x, n_y, dim, g.rtx, g.sx, S,
                 g.rpad, scale, out4, dy);
    return mmvae_check_launch("mmd_fold_y");
}

int launch_mmd_kernel_matrix(const float* x, int n_x, const float* y, int n_y, int dim, float* k, hipStream_t s) {
    switch (steps_of(dim)) {
#define MMD_CASE(m) case m: launch_matrix<m>(x, n_x, y, n_y, dim, k, s); break;
        MMD_FOR_M(MMD_CASE)
#undef MMD_CASE
        default: MMVAE_REQUIRE(false, "mmd_kernel_matrix: dim = %d", dim);
    }
    return mmvae_check_launch("mmd_kernel_matrix");
}
