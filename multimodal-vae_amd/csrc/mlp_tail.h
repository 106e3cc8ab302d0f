// Fused row-block launches for the last two Linears of the image encoder's classifier (n_latents = 100), and the one-expert waist of
// the image-only step that carries them on to z and back from dz (n_latents = 20, 100). See mlp_tail.hip.
#pragma once
#include "common.h"

struct Mlp2FwdArgs {
    int rows;
    const bf16* x;           // [rows][400] activated (+ dropout) output of classifier.0
    const bf16* w2;          // classifier.3 weight, fragment-major [208][416]
    const float* b2;
    const bf16* w3;          // classifier.6 weight, fragment-major [208][224]
    const float* b3;
    const uint8_t* mask; float mask_scale;      // [rows][200] keep flags of the second Dropout, or null
    bf16 *y2, *ay2;          // out [rows][200]: raw and activated (+ dropout) classifier.3 output (saved for the backward pass)
    float* out;              // out [rows][200] = (mu | logvar)
};
int launch_mlp2_fwd(const Mlp2FwdArgs& a, hipStream_t s);

struct Mlp2BwdArgs {
    int rows;
    const bf16* d_out;       // [rows][200] gradient wrt (mu | logvar)
    const bf16* w3t;         // classifier.6 weight transposed, fragment-major [208][224]  (row = classifier.3 unit)
    const bf16* w2t;         // classifier.3 weight transposed, fragment-major [400][224]  (row = classifier.0 unit)
    const bf16 *y2, *y1;     // raw pre-activations [rows][200], [rows][400]
    const uint8_t *mask2, *mask1; float mask_scale;
    bf16 *dy2, *dy1;         // out: gradients wrt the raw outputs of classifier.3 / classifier.0
    float *db2, *db1;        // += column sums of dy2 / dy1 (bias gradients of classifier.3 / classifier.0)
};
int launch_mlp2_bwd(const Mlp2BwdArgs& a, hipStream_t s);

// ---- the one-expert "waist" of the image-only VAE step (multimnist/model.py ImageVAE): no product of experts, so every row is
// independent from classifier.0's output to z, and the 16-row workgroup of mlp2_fwd / mlp2_bwd carries the latent block too.
// Compiled for n_latents = 20 and 100 (mlp2_latent1_compiled); w3 / w3t are the fragment-major packs [round_up(2D,16)][224] and
// [208][round_up(2D,32)].  Every sum is folded in a fixed order (thread, wave, workgroup; the workgroups by launch_mlp2_latent1_finish)
// without float atomics: equal inputs give equal bits.
bool mlp2_latent1_compiled(int D);
// doubles of scratch both directions share: [nblk] KL partials, then [nblk][2D] column sums of d_enc_out (nblk = ceil(rows / 16))
size_t mlp2_latent1_scratch_doubles(int rows, int D);
struct Mlp2Latent1FwdArgs : Mlp2FwdArgs {      // `out` = enc_out [rows][2D] fp32 (mu | logvar)
    int D, ldz, training;
    const float* eps;        // [rows][D], read when training
    float *mu, *logvar;      // [rows][D] or null
    float* z_f32;            // [rows][D]: eps * expf(0.5 * logvar) + mu (training) or mu
    bf16* z_bf;              // [rows][ldz]: bf16(z), column D = 1.0 (the folded bias of upsample.0), the other pad columns 0
    double* scratch;         // [blockIdx.x] = the workgroup's KL partial (kl_fwd's fp32 terms added in double)
};
int launch_mlp2_latent1_fwd(const Mlp2Latent1FwdArgs& a, hipStream_t s);
struct Mlp2Latent1BwdArgs : Mlp2BwdArgs {      // `d_out` is not read: the gradient wrt (mu | logvar) is formed here
    int D, lde, training;
    const float *mu, *logvar, *eps;     // [rows][D] (eps read when training)
    const float* dz;         // [rows][D] or null (no reconstruction term)
    float kl_coef;           // kl_lambda / B
    bf16* d_enc_out;         // out [rows][lde]: bf16 of latent1_bwd's double expression, pad columns [2D, lde) 0 (classifier.6's weight gradient reads it)
    double* scratch;         // [nblk + blockIdx.x * 2D + c] = the workgroup's column sums of the exact terms
};
int launch_mlp2_latent1_bwd(const Mlp2Latent1BwdArgs& a, hipStream_t s);
// One workgroup folds the partials in block order: loss_out[16] = column sums of loss_slots [MMVAE_LOSS_SLOTS][16], with the KL
// (column 8) + the fp32 rounding of the folded KL partials; d_bias [2D] += the folded column sums when given (the backward's finish).
int launch_mlp2_latent1_finish(const double* scratch, int rows, int D, float* d_bias_or_null, const float* loss_slots, float* loss_out, hipStream_t s);
