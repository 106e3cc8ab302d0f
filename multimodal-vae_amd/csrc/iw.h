// Importance-sampled marginal log-likelihood, the model-family independent part (iw.hip): particles from the proposal,
// the online log-sum-exp accumulator over particle chunks and its finalize.  The family's scoring call (multimnist.hip:
// mm_iw_score) sits between particles and accumulate.
//
// Particle rows are example-major: row = b*K + k for example b and the call's particle k.
#pragma once
#include "common.h"

// accumulator state per (example, target): target 0 = x, 1 = y, 2 = xy;
// {running max m of log w, sum exp(log w - m), sum exp(2 (log w - m)), sum of the target's log-likelihood}
constexpr int IW_TARGETS = 3, IW_STATE = 4;
// finalize output per example: log p^(x), log p^(y), log p^(x,y), ESS x / y / xy, mean -log p(x|z), mean -log p(y|z)
constexpr int IW_OUT = 8;

// z [B][K][D] = mu + exp(logvar/2) * eps, log_ratio [B][K] = log p(z) - log q(z).  eps is Philox keyed by
// (seed, first_row + b, first_particle + k, dimension) unless `eps` ([B][K][D]) is given.
int launch_iw_particles(const float* mu, const float* logvar, int B, int D, int K, long long first_row, long long first_particle,
                        unsigned long long seed, const float* eps, float* z, float* log_ratio, hipStream_t s);
int launch_iw_init(float* state, int B, hipStream_t s);
// log p(y|z) of row r = sum over the T steps of words[r][t][targets[b][t]]; log w = log-likelihood + log_ratio.
// log_w (nullable): [B][K][3] the log weights of the call.
int launch_iw_accumulate(const float* loglik_x, const float* words, const long long* targets, int T, int V, const float* log_ratio,
                         int B, int K, float* state, float* log_w, hipStream_t s);

// Forward-only image scoring tail of the conv families (celeba_iw.hip, coco_iw.hip; each has a kernel of its own): raw bf16 NHWC
// [rows][S][S][C] output of hallucinate.6 -> BatchNorm affine + act -> ConvTranspose2d(C, 3, 4, 2, 1) -> one log p(x|z) per row
// against image [rows / K].  CelebA: S = C = 32, COCO: S = 16, C = 64.  The affine is either the table `affine` [C] (scale,
// shift) or, when that is null, made from gamma / beta / running mean / running variance [C] each.
struct IwTailArgs {
    const bf16* q3; const float2* affine;
    const float *gamma, *beta, *rmean, *rvar; float eps;
    int act;
    const float* w;                  // (C, 3, 4, 4) fp32
    const float* image;              // [rows / K][3][2S][2S]
    int rows, K;
    float* loglik;                   // [rows]
    float* logits;                   // [rows][3][2S][2S] or null
};
int launch_iw_finalize(const float* state, int B, long long K_total, float* out, hipStream_t s);
