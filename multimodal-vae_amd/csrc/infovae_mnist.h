// MNIST InfoVAE (mnist/model.py:238-279, mnist/train_infovae.py:45-76): the model's four fp32 Linear layers, its loss tail and its
// one-enqueue training step.  The four bias-free 4 x 4 stride-2 convolutions are conv4s2.h's, the MMD term is mmd.h's.
//
// A layer is y = act(x W^T + b), x [rows][K], W [N][K] (nn.Linear's own layout, never copied), y [rows][N], act none / relu / leaky.
// Everything runs on v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation, the reference's own arithmetic.
//   forward          y = act(x W^T + b)
//   data gradient    dx = gp W,      gp = g (.) act'(y) formed from the upstream gradient g and the SAVED OUTPUT y while the operand is
//                                    loaded (conv4s2.h's contract: relu y > 0 ? g : 0, leaky y > 0 ? g : slope g); gp is never stored
//   weight gradient  dW = gp^T x,    db = column sums of gp from the same launch (a ones column on the MFMA).  The reduction is the batch:
//                                    every dW element has exactly one writer
// perm: conv4s2 keeps activations channels-last, [rows][7][7][128], while encoder_fc.0 and decoder_fc.2 are defined on the (c, h, w)
// flattening.  With perm set, the layer's 6272-wide side (K of encoder_fc.0, N of decoder_fc.2) lives in memory at p * 128 + c for the
// weight's feature c * 49 + p: the permutation is applied where the ACTIVATION (or its gradient) is loaded or stored, the weight is read
// and its gradient written in its own order, in full lines.
// Forward and data gradient cut a long reduction into LIN_MAX_SPLIT chunks at most (lin_ksplit: a function of the layer's N and K alone,
// never of the batch); the chunks go to the workspace and a second launch folds them in ascending order and applies bias, activation
// and the store.  No atomics: two calls give identical bits, and a row's forward bits do not depend on the other rows.
#pragma once
#include "common.h"
#include "../../include/mmvae_hip.h"

enum { LIN_ACT_NONE = 0, LIN_ACT_RELU = 1, LIN_ACT_LEAKY = 2 };
enum {
    LIN_PERM_P = 49, LIN_PERM_C = 128,      // the permuted side is LIN_PERM_P * LIN_PERM_C = 6272 wide
    LIN_MAX_SPLIT = 8,
    LIN_MAX_ROWS = 65536,
    LIN_MAX_DIM = 1 << 16,                  // N, K
};

struct LinShape { int rows, N, K, act, perm; float slope; };

// null when the shape is fine, else what is wrong with it
const char* lin_shape_error(const LinShape& s);
int lin_ksplit(int blocks, int red);                    // chunks of a reduction of `red` terms, `blocks` workgroups per chunk and row block
size_t lin_fwd_workspace_bytes(const LinShape& s);      // 0: the layer needs none
size_t lin_dgrad_workspace_bytes(const LinShape& s);
int launch_lin_fwd(const LinShape& s, const float* x, const float* w, const float* b, float* y, void* ws, hipStream_t st);
int launch_lin_dgrad(const LinShape& s, const float* g, const float* y, const float* w, float* dx, void* ws, hipStream_t st);
int launch_lin_wgrad(const LinShape& s, const float* g, const float* y, const float* x, float* dw, float* db, hipStream_t st);

// The loss tail in one launch: slots[q * 16] = the q-th of MMVAE_LOSS_SLOTS partial sums of (recon - x)^2, each over a fixed range
// in a fixed order (the step's sum_slots fold adds them in ascending q), and g = coef * 2 (recon - x) (null: not wanted).
int launch_mse_tail(const float* recon, const float* x, long long n, float coef, float* g, float* slots, hipStream_t st);

struct MnistInfoVaePlan;
struct PlanBase;
MnistInfoVaePlan* mnist_infovae_create(int n_latents, int batch);
void mnist_infovae_destroy(MnistInfoVaePlan*);
PlanBase* mnist_infovae_base(MnistInfoVaePlan*);
int mnist_infovae_bind(MnistInfoVaePlan*, float* params, float* grads);
size_t mnist_infovae_step_workspace_bytes(const MnistInfoVaePlan*);
int mnist_infovae_step(MnistInfoVaePlan*, const mmvae_mnist_infovae_step_io&, int training, int do_backward, hipStream_t);
