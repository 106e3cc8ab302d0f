// 4 x 4, stride 2, pad 1 convolution and its transpose, bias-free, with a fused activation: the down- and up-sampling block of a
// small convolutional autoencoder (the MNIST InfoVAE).  bf16 operands rounded to nearest even, fp32 accumulation on
// v_mfma_f32_16x16x32_bf16, activations fp32 channels-last.  Cs = channels on the high-resolution side S (Hs x Ws), Cl = channels on
// the low-resolution side L (H x W = Hs/2 x Ws/2).  A Conv2d weight (Cout, Cin, 4, 4) and a ConvTranspose2d weight (Cin, Cout, 4, 4)
// are both (Cl, Cs, 4, 4), so three kernels serve both modules in both directions:
//   down:  pre[b,oy,ox,l] = sum_{s,ky,kx} bf16(S[b,2oy-1+ky,2ox-1+kx,s]) bf16(w[l,s,ky,kx])         conv forward, transposed-conv dgrad
//   up:    pre[b,iy,ix,s] = sum_{l,ky,kx : iy+1-ky, ix+1-kx even} bf16(L[b,(iy+1-ky)/2,(ix+1-kx)/2,l]) bf16(w[l,s,ky,kx])
//                                                                                                  transposed-conv forward, conv dgrad
//   wgrad: dw[l,s,ky,kx]  = sum_{b,oy,ox} bf16(L[b,oy,ox,l]) bf16(S[b,2oy-1+ky,2ox-1+kx,s])         both modules
// a position outside the image contributes nothing.  dst = act(pre) (none / relu / leaky / sigmoid).  Where an operand is a gradient,
// the activation's backward is applied while it is loaded, from the upstream gradient g and the SAVED OUTPUT y of the forward (the
// pre-activation is never stored), in fp32, then rounded to bf16:
//   none: g;  relu: y > 0 ? g : 0;  leaky: y > 0 ? g : slope g;  sigmoid: (g y) (1 - y)
//
// down and up are ONE implicit-GEMM kernel.  Its rows are L-side positions (b, qy, qx) in both directions.  down: 16 taps, the source
// row of tap (ky, kx) is S position (2qy-1+ky, 2qx-1+kx), K = Cs per tap, the output row is the L position itself.  up: an output
// pixel's row and column parity (py, px) selects 2 x 2 of the 16 cells, so the S side splits into four dense sub-problems
// (blockIdx.z) of 4 taps, K = Cl per tap: tap (a, c) of class (py, px) is cell (1-py+2a, 1-px+2c) read at L position (qy+py-a, qx+px-c),
// the output row is S position (2qy+py, 2qx+px).  A workgroup owns C4_TM rows x C4_TN output channels; per tap it stages the source
// rows and reads the packed bf16 weights [cell][N padded to C4_TN][K padded to 32] from global memory as MFMA B fragments (all
// k-steps of a tap, issued in front of the barrier); the source rows are fetched two taps ahead.  One fp32 chain per tap, the taps
// summed in a second chain.  The LDS tile layouts, the fp32 -> bf16 staging and the MFMA tile are described in conv_tile.h, which holds
// the pieces shared with causal_conv.
// Cs == 1 (the model's outer pair) has a GEMM dimension of 1, so it runs on the vector unit instead: down as 16 multiply-adds per
// output from the fp32 weights themselves, up as four dot products over Cl per S pixel with the weights in LDS, the weight gradient
// as per-thread sums over position slices folded in ascending order.  Same rounding, same contract, nothing to pack.
// wgrad splits the L positions into chunks; workgroup (chunk, cell, 64 x 64 channel tile) writes its fp32 partial to the workspace
// and a second launch folds the partials in ascending chunk order into (Cl, Cs, 4, 4).  No atomics: two calls give identical bits.
// The weights are packed by a small kernel on the same stream on every call (an optimizer step changes them in place).
#pragma once
#include "common.h"

enum {
    C4_TM = 64,              // L positions per workgroup (down / up)
    C4_TN = 64,              // output channels per workgroup; 64 x 64 is also the weight gradient's channel tile
    C4_CHUNK = 512,          // L positions per weight-gradient partial, at least (see c4_chunk)
    C4_MAX_CHUNKS = 64,      // partials per cell at most: the chunk grows beyond it
    C4_KP = 64,              // positions staged per barrier pair in the weight gradient
    C4_MAX_CH = 128,         // Cs, Cl (one LDS stage holds a tap's whole K)
    C4_MAX_SIDE = 64,        // Hs, Ws
    C4_MAX_POS = 1 << 24,    // B * Hs * Ws
};
enum { C4_ACT_NONE = 0, C4_ACT_RELU = 1, C4_ACT_LEAKY = 2, C4_ACT_SIGMOID = 3 };

struct C4Shape { int B, Cs, Cl, Hs, Ws; };

bool c4_shape_ok(const C4Shape& s);
int c4_chunk(const C4Shape& s);                     // L positions per weight-gradient partial for this shape, a multiple of C4_KP
size_t c4_workspace_bytes(const C4Shape& s);

// src_y: the saved output at src's positions when src is an upstream gradient (act_in says of which activation), else null
int launch_c4_down(const C4Shape& s, const float* src, const float* src_y, const float* w, float* dst, int act_in, int act_out, float slope,
                   void* ws, hipStream_t st);
int launch_c4_up(const C4Shape& s, const float* src, const float* src_y, const float* w, float* dst, int act_in, int act_out, float slope,
                 void* ws, hipStream_t st);
// y_s / y_l: the saved output on the side that carries the gradient (one of them at most), else null
int launch_c4_wgrad(const C4Shape& s, const float* s_side, const float* l_side, const float* y_s, const float* y_l, int act, float slope,
                    float* dw, void* ws, hipStream_t st);
