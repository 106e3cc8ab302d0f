// Causal tap-list convolution for PixelCNN / GatedPixelCNN training: forward, data gradient and weight gradient on
// v_mfma_f32_16x16x32_bf16 (bf16 operands rounded to nearest even, fp32 accumulation), activations fp32 channels-last
// ([position][channel], position = (b * H + i) * W + j).  A tap (r, c, dy, dx) applies kernel cell (r, c) at offset (dy, dx):
//   y[p][co]          = bias[co] + sum_t sum_ci bf16(x[p + (dy_t, dx_t)][ci]) * bf16(w[co][ci][r_t][c_t])
//   dx[p][ci]         =            sum_t sum_co bf16(g[p - (dy_t, dx_t)][co]) * bf16(w[co][ci][r_t][c_t])
//   dw[co][ci][r_t][c_t] = sum_p bf16(g[p][co]) * bf16(x[p + (dy_t, dx_t)][ci]);   a cell in no tap: 0
//   db[co]            = sum_p g[p][co]                                              (g unrounded)
// a shifted position outside its own image contributes nothing.  Only the taps that exist are computed.
//
// Forward and data gradient are ONE implicit-GEMM kernel (M = positions, N = output channels, K = taps x input channels): the
// data gradient runs it with negated offsets on a weight image packed with Cin and Cout exchanged.  A workgroup owns
// CC_TM positions x CC_TN channels; per tap it stages the shifted activation rows (rows whose shifted position leaves the image as
// zeros: decided per row and tap) and reads the packed bf16 weights [tap][channel padded to CC_TN][K padded to 32] straight from
// global memory as MFMA B fragments, inside the k-loop.  The LDS tile layouts, the fp32 -> bf16 staging and the MFMA tile are described
// in conv_tile.h, which holds the pieces shared with conv4s2.
// The weight gradient splits the positions into chunks of CC_CHUNK; workgroup (chunk, tap, 64 x 64 channel tile) writes its
// fp32 partial g^T x_shifted to the workspace, and a second launch folds the partials in ascending chunk order and scatters them
// into the (Cout, Cin, kh, kw) layout (db likewise, from a per-chunk column sum of g).  No atomics: two calls give identical bits.
// The weights are packed by a small kernel on the same stream on every call (an optimizer step changes them in place).
#pragma once
#include "common.h"

enum {
    CC_TM = 64,              // positions per workgroup (forward / data gradient)
    CC_TN = 64,              // output channels per workgroup; 64 x 64 is also the weight gradient's channel tile
    CC_KC = 128,             // input channels staged per barrier pair
    CC_CHUNK = 1024,         // positions per weight-gradient partial
    CC_KP = 64,              // positions staged per barrier pair in the weight gradient
    CC_MAX_TAPS = 64,
    CC_MAX_CELLS = 64,       // kh * kw
    CC_MAX_OFF = 7,          // |dy|, |dx|
    CC_MAX_CH = 1024,        // Cin, Cout (conv4 has out_dims * data_channels = 768 outputs)
    CC_MAX_POS = 1 << 22,    // B * H * W: positions are split into (b, i, j) with a float reciprocal, exact below 2^22
};

struct CcTaps {
    int n, cells;                                    // taps, kh * kw
    signed char dy[CC_MAX_TAPS], dx[CC_MAX_TAPS];    // offset of tap t
    signed char cell[CC_MAX_TAPS];                   // r * kw + c of tap t
    signed char tap_of_cell[CC_MAX_CELLS];           // -1: the cell is in no tap
};

struct CcShape { int B, H, W, Cin, Cout, kh, kw; };

// validates shape and taps (host array of n_taps x {r, c, dy, dx}) and fills `out`; MMVAE_EINVAL + message otherwise
int cc_make_taps(const char* what, const CcShape& s, const int* taps, int n_taps, CcTaps* out);
size_t cc_workspace_bytes(const CcShape& s, int n_taps);

int launch_cc_forward(const CcShape& s, const CcTaps& t, const float* x, const float* w, const float* bias, float* y, void* ws, hipStream_t st);
int launch_cc_backward_data(const CcShape& s, const CcTaps& t, const float* g, const float* w, float* dx, void* ws, hipStream_t st);
// dw (Cout, Cin, kh, kw) and db (Cout), each may be null
int launch_cc_backward_weight(const CcShape& s, const CcTaps& t, const float* g, const float* x, float* dw, float* db, void* ws, hipStream_t st);
