// PixelCNN output head fused with its cross entropy: the 1 x 1 convolution conv4 (hid -> V * C channels, output channel v * C + c =
// level v of data channel c) and the per-element negative log-likelihood, forward and backward, without the logits ever existing in
// global memory.  h fp32 channels-last ([position][hid], position p = (b * H + i) * W + j), target / nll / lse / g in (B, C, H, W).
//   l[p,v,c]   = bias[vC+c] + sum_k bf16(h[p,k]) bf16(w[vC+c,k])            (bf16 round to nearest even, fp32 accumulation)
//   lse[p,c]   = log sum_v exp(l[p,v,c])                                     (online over level tiles, running maximum subtracted)
//   nll[p,c]   = lse[p,c] - l[p,target[p,c],c]                               (target outside 0..V-1: NaN)
//   d[p,v,c]   = g[p,c] (exp(l[p,v,c] - lse[p,c]) - [v == target[p,c]])
//   dh[p,k]    = sum_{v,c} bf16(d) bf16(w[vC+c,k]);   dw[vC+c,k] = sum_p bf16(d) bf16(h[p,k]);   db[vC+c] = sum_p d  (unrounded)
//
// The weights are packed per call (an optimizer step changes them in place) to bf16, channel-major: row n' = c * Vp + v with
// Vp = V padded to HN_TN, so that a level tile belongs to one data channel; once as [n'][K padded to 32] (the logits' B operand)
// and once transposed as [c][hid padded][Vp] (the B operand of dh).  Padded level columns are excluded by the predicate v < V.
// A wave owns 16 positions: it keeps their h rows as bf16 MFMA A fragments in registers, loops over c and the level tiles, and
// keeps the running (max, sum) and the target logit per row (selected by comparison, never by address).  The dh kernel runs the
// same loop with the saved lse, sends each d tile through LDS as bf16 into a second MFMA against the transposed weight tile and
// accumulates 16 x hid in registers.  The dw / db kernel has the grid (chunk of HN_CHUNK positions, level tile): it recomputes l
// and d per 64 positions, accumulates d^T h (both through LDS transposed, [channel][position]) and the column sums of the
// unrounded d, and writes fp32 partials to the workspace; a fold kernel adds them in ascending chunk order and un-permutes them
// into (V * C, hid, 1, 1).  No atomics: two calls give identical bits.
#pragma once
#include "common.h"

enum {
    HN_TM = 64,              // positions per workgroup (4 waves x 16)
    HN_TN = 64,              // levels per tile
    HN_CHUNK = 1024,         // positions per dw / db partial
    HN_MAX_HID = 256,        // hid: a multiple of 8
    HN_MAX_V = 256,          // levels: 2..256
    HN_MAX_POS = 1 << 22,    // B * H * W, as the causal convolution
};

struct HnShape { int B, C, H, W, hid, V; };

bool hn_shape_ok(const HnShape& s);
size_t hn_workspace_bytes(const HnShape& s);
// lse may be null
int launch_hn_forward(const HnShape& s, const float* h, const float* w, const float* bias, const long long* target, float* nll, float* lse,
                      void* ws, hipStream_t st);
// each of dh, dw, db may be null
int launch_hn_backward(const HnShape& s, const float* h, const float* w, const float* bias, const long long* target, const float* lse,
                       const float* g, float* dh, float* dw, float* db, void* ws, hipStream_t st);
