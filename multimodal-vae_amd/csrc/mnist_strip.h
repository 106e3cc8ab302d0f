// Column-strip fused layers of the MNIST MLPs (mnist/model.py:188-232: Linear -> BatchNorm1d -> ReLU), fp32 on
// v_mfma_f32_16x16x4_f32.  BatchNorm1d needs statistics over the whole batch but only per feature, so a workgroup that owns a strip
// of 16 output features for ALL rows of the batch finishes the layer alone: no atomics, no second launch, no grid-wide
// synchronisation, and equal inputs give equal bits.  mnist_strip.hip has the kernels; mnist_f32.hip runs them in
// mnist_f32_image_step behind the switch "mnist_strip" (mmvae_debug_set).
#pragma once
#include "common.h"

// rows one workgroup carries: 8 waves x 4 row tiles of 16 (the accumulators of a wave's tiles stay in registers through the K loop)
constexpr int MNIST_STRIP_WAVES = 8;
constexpr int MNIST_STRIP_MAX_TILES = 4;
constexpr int MNIST_STRIP_MAX_ROWS = MNIST_STRIP_WAVES * MNIST_STRIP_MAX_TILES * 16;      // 512

// r = x W^T + b; (mean, biased var) of r over the rows, two-pass, folded in a fixed order; a = relu((r - mean) rstd gamma + beta).
// training: running_mean / running_var move `updates` times by momentum 0.1 towards mean / the unbiased variance, *nbt += updates;
// eval: mean / var are the running statistics, no buffer is written.  mr = (mean, rstd) either way (the backward reads it).
struct StripFwdArgs {
    const float* x; int ldx;                 // [rows][ldx]: 16-byte aligned, ldx % 4 == 0, ldx >= K
    const float* w; const float* bias;       // [N][K] (16-byte aligned, K % 4 == 0), [N]
    const float* gamma; const float* beta;   // [N]
    float* running_mean; float* running_var; long long* nbt;
    int rows, N, K, training, updates;
    float* r; float* a;                      // out [rows][N]
    float2* mr;                              // out [N]
};
int launch_lin_bn_act_fwd32(const StripFwdArgs& a, hipStream_t s);

// d = (dy W_next) relu'(x^ gamma + beta) with x^ = (r - mean) rstd; s1 = sum_rows d, s2 = sum_rows d x^ in a fixed order;
// dgamma += s2, dbeta += s1, d_r = gamma rstd (d - s1 / rows - x^ s2 / rows): lin_dgrad32 + bn1d_bwd32_kernel of the layer below.
struct StripBwdArgs {
    const float* dy; int Nn;                 // [rows][Nn] gradient wrt the next Linear's output: 16-byte aligned, Nn % 4 == 0
    const float* w_next;                     // [Nn][N]
    const float* r; const float2* mr;        // this layer: raw output [rows][N], (mean, rstd) [N]
    const float* gamma; const float* beta;   // [N]
    int rows, N;
    float* d_r;                              // out [rows][N]
    float* dgamma; float* dbeta;             // [N] +=
};
int launch_lin_dgrad_bn_bwd32(const StripBwdArgs& a, hipStream_t s);
