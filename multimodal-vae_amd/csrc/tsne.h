// Exact t-SNE with a 2-component embedding (mnist/manifold.py: PCA + TSNE(2, perplexity 40, 300 iterations)) in fp32:
//   affinities: d_ij = sum_k (x_ik - x_jk)^2 (16 fmaf chains, coordinate k in chain k % 16, folded by a fixed tree),
//               p_{j|i} = exp(-beta_i (d_ij - min_j d_ij)) / sum,
//               beta_i searched as sklearn does (start 1, double / halve until bracketed, halve the bracket, |H - log perplexity| <=
//               1e-5, 100 steps), P_ij = (p_{j|i} + p_{i|j}) / 2n floored at 1e-12 off the diagonal, 0 on it
//   gradient:   w_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} w_ij,
//               grad_i = 4 (exaggeration sum_j P_ij w_ij (y_i - y_j) - sum_j w_ij^2 (y_i - y_j) / Z)
//               KL(P || Q) = sum P log P - sum P log w + log Z                       (P not exaggerated)
//   run:        sklearn's _gradient_descent (gains, momentum 0.5 then 0.8), every iteration enqueued on the stream
// Every pair is visited ONCE per gradient: the repulsive sum is divided by Z after the sweep, so no pass over the pairs needs Z.
//
// Affinities: one workgroup per row writes the distances into the row of P itself (it stays in L2), finds beta with up to 100 sweeps
// over that row (fp32 exp, float64 sums in a fixed order) and overwrites the row with p_{j|i}.  A second launch symmetrises in
// place: workgroup (a, b), a <= b, owns the TSNE_ST x TSNE_ST tiles (a, b) and (b, a), transposes one through LDS and writes
// both; P_ij and P_ji come from the two orders of one commutative add, so P is symmetric bit for bit.  A third, one workgroup,
// folds the float64 partial sums of P log P and P.
//
// Gradient sweep: grid = (row tiles of TSNE_RT rows) x (column splits); split c of S covers the column tiles
// [T c / S, T (c + 1) / S) of TSNE_CT columns.  Lane l of each of the 4 waves owns row l of the tile; wave w takes the columns
// [w, w + 1) TSNE_CT / 4 of every column tile.  P is read through its transpose (P_ji for P_ij: P must be symmetric, as
// affinities writes it), so a wave's load is 64 consecutive floats; y_j comes from double-buffered LDS as a broadcast.  Per
// thread: the force terms in fp32, summed over 8 columns in fp32 and in float64 above that; the three terms of the KL (w, P log w,
// P log P) in float64 per pair, from the exact 1 + |dy|^2 and a table-driven logarithm (the error of logf is biased and does not
// average out over the pairs).  The 4 waves are combined in ascending order; one float64 partial of the four force sums per
// (split, row) and one of (sum w, sum P log w, sum P log P) per workgroup go to the workspace.  The fold
// kernel (one thread per row) adds the workgroup partials in a fixed order (every workgroup the same: Z has the same bits
// everywhere), the row's splits in ascending order, and applies the update.  No atomics: two calls give identical bits.
#pragma once
#include "common.h"

enum {
    TSNE_RT = 64,             // rows per workgroup of the sweep: 4 waves, lane = row
    TSNE_CT = 128,            // columns per column tile of the sweep (32 per wave)
    TSNE_ST = 32,             // side of a symmetrisation tile
    TSNE_AT = 256,            // threads of an affinity workgroup: thread t takes the columns t, t + 256, ...
    TSNE_MAX_DIM = 256,
    TSNE_MIN_N = 3,
    TSNE_MAX_N = 32768,       // P is n * n * 4 bytes: 4 GiB
    TSNE_MAX_SPLITS = 64,
    TSNE_GRID_TARGET = 2048,  // splits = max(1, min(column tiles, TSNE_MAX_SPLITS, TSNE_GRID_TARGET / row tiles))
    TSNE_SEARCH_STEPS = 100,
};

struct TsneShape {
    int rt;                   // row tiles of the sweep
    int ct;                   // column tiles
    int s;                    // column splits
    int st;                   // symmetrisation tiles per side
    long long rpad;           // rt * TSNE_RT
};
TsneShape tsne_shape(int n);
// the larger of: the sweep's [s][rpad][4] + [s][rt][3] + [4] float64; the symmetrisation's [st][st][2] float64
size_t tsne_workspace_bytes(int n);

// P [n][n] (written), beta [n], out2 = {sum P log P, sum P}
int launch_tsne_affinities(const float* x, int n, int dim, float perplexity, float* P, float* beta, float* out2, void* ws, hipStream_t s);
// grad [n][2], out3 = {KL, Z, sum P log P}
int launch_tsne_grad(const float* P, float exaggeration, const float* y, int n, void* ws, float* grad, float* out3, hipStream_t s);
// y, update, gains [n][2] in and out; kl_trace [n_iter]; iteration k of the call is iteration first_iter + k of the schedule
int launch_tsne_run(const float* P, int n, float* y, float* update, float* gains, int first_iter, int n_iter, float learning_rate,
                    float early_exaggeration, int exaggeration_iters, float* kl_trace, void* ws, hipStream_t s);
