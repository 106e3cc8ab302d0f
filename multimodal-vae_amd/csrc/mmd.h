// Gaussian-kernel maximum mean discrepancy (coco/model.py:385-402, the InfoVAE loss term) in fp32, value and both gradients
// from one sweep over the pairs:
//   k(a, b)   = exp(-(sum_k (a_k - b_k)^2 / D) / D)
//   MMD(x, y) = mean_ij k(x_i, x_j) + mean_ij k(y_i, y_j) - 2 mean_ij k(x_i, y_j)          (diagonals included)
//   dMMD/dx_i = -(4 / (n_x^2 D^2)) sum_j k(x_i, x_j) (x_i - x_j) + (4 / (n_x n_y D^2)) sum_j k(x_i, y_j) (x_i - y_j)   (dy alike)
// Per pair: d_k = a_k - b_k, four interleaved fmaf(d, d, acc) chains (coordinate chunk c of 4 floats goes to chain c % 4, ascending)
// folded by a fixed butterfly, then expf: integer-valued inputs give exact distances, and the result of a pair does not depend on
// the tile, the split or the call it lands in.  The (n, n, D) tensors of the reference formulation never exist.
//
// Decomposition: the rows are the row tiles of x followed by those of y, the columns likewise; grid = (row tiles) x (column
// splits), the first mmd_splits(...).sx splits over x's column tiles, the rest over y's, so a workgroup sees one (row class,
// column class).  A workgroup keeps its MMD_RT rows in registers (4 lanes per row), streams column tiles of MMD_CT rows through
// double-buffered LDS, sums k and k * d over 8 columns in fp32, carries the running sums in float64 and writes one partial per
// (split, row) into the workspace.  A second kernel folds the partials in float64 in a fixed order: block 0 the three means and
// MMD (rounded to fp32 once), the others the gradient rows.  No atomics: two calls give identical bits.
#pragma once
#include "common.h"

enum {
    MMD_RT = 64,             // rows per workgroup: 256 threads, 4 lanes per row
    MMD_CT = 32,             // rows of x or y per column tile
    MMD_MAX_DIM = 256,       // D: 16 coordinates per lane and step, at most 16 steps
    MMD_MAX_N = 65536,       // n_x, n_y
    MMD_MAX_SPLITS = 64,     // column splits per class
    MMD_GRID_TARGET = 1024,  // splits per class = max(1, min(column tiles of the class, MMD_MAX_SPLITS, MMD_GRID_TARGET / row tiles))
};

struct MmdShape {
    int rtx, rty;            // row tiles of x, of y
    int tx, ty;              // column tiles of x, of y
    int sx, sy;              // column splits over x, over y: a function of (n_x, n_y) alone
    long long rpad;          // (rtx + rty) * MMD_RT: rows of one split's slab in the workspace
};
MmdShape mmd_shape(int n_x, int n_y);
// [sx + sy][rpad] float64 kernel sums, then [sx + sy][rpad][dim] float64 gradient sums
size_t mmd_workspace_bytes(int n_x, int n_y, int dim);

// out4 = {mean Kxx, mean Kyy, mean Kxy, MMD}; dx [n_x][dim], dy [n_y][dim], each may be null (both null: the value alone, and
// the y-rows-by-x-columns quarter of the pairs is skipped).  x == y is allowed.
int launch_mmd(const float* x, int n_x, const float* y, int n_y, int dim, void* ws, float* out4, float* dx, float* dy, hipStream_t s);
// The form a training step takes, where x are prior samples and only y = z has a gradient (coco/train_infovae.py:44-55): the same
// grid, but the row tiles of x run the value form of the sweep -- their kernel sums feed Kxx and Kxy, no k * d products, no gradient
// partials -- so about half of the gradient arithmetic and of the gradient workspace goes.  Per pair, per 8 columns, per split and
// in the fold the arithmetic and its order are launch_mmd's: out4 and (scale = 1) dy carry the bits launch_mmd writes.
// dy [n_y][dim] = scale * dMMD/dy (the product in float64, rounded once), or null: the value alone.  out4 may point anywhere 4 floats
// fit (a step's loss slots).  Workspace: [sx + sy][rpad] float64 kernel sums, then [sx + sy][rty * MMD_RT][dim] gradient sums.
size_t mmd_dy_workspace_bytes(int n_x, int n_y, int dim);
int launch_mmd_dy(const float* x, int n_x, const float* y, int n_y, int dim, void* ws, float scale, float* out4, float* dy, hipStream_t s);
// k [n_x][n_y] = k(x_i, y_j), the arithmetic of launch_mmd per pair
int launch_mmd_kernel_matrix(const float* x, int n_x, const float* y, int n_y, int dim, float* k, hipStream_t s);
