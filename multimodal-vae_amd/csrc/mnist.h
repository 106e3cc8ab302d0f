// MNIST MMVAE plan (mnist/model.py:14-185 ; mnist/train.py:64-81,131-147).
#pragma once
#include "layers.h"
#include "../../include/mmvae_hip.h"

struct PlanBase;

struct MnistPlan;
MnistPlan* mnist_create(int D, int B, int precision = -1);   // 0 fp32 (default), 1 bf16 operands, -1: env MMVAE_MNIST_PRECISION
int mnist_is_f32(const MnistPlan*);
void mnist_destroy(MnistPlan*);
PlanBase* mnist_base(MnistPlan*);
int mnist_step(MnistPlan*, const mmvae_mnist_step_io&, int training, int do_backward, hipStream_t);
// granular module entry points (drop-in nn.Module forwards); B rows, every call brings its workspace
int mnist_image_encoder_fwd(MnistPlan*, void* ws, size_t wsb, const float* image, int training, float* out, hipStream_t);
int mnist_image_encoder_bwd(MnistPlan*, void* ws, size_t wsb, const float* d_out, hipStream_t);
int mnist_image_decoder_fwd(MnistPlan*, void* ws, size_t wsb, const float* z, int training, float* recon, hipStream_t);
int mnist_image_decoder_bwd(MnistPlan*, void* ws, size_t wsb, const float* d_recon, const float* recon, float* dz, hipStream_t);
int mnist_text_encoder_fwd(MnistPlan*, void* ws, size_t wsb, const long long* label, int training, float* out, hipStream_t);
int mnist_text_encoder_bwd(MnistPlan*, void* ws, size_t wsb, const long long* label, const float* d_out, hipStream_t);
int mnist_text_decoder_fwd(MnistPlan*, void* ws, size_t wsb, const float* z, int training, float* logp, hipStream_t);
int mnist_text_decoder_bwd(MnistPlan*, void* ws, size_t wsb, const float* d_logp, const float* logp, float* dz, hipStream_t);
// Importance-weighted evaluation (mnist_iw.hip): eval-mode decoders on B*K particle rows z [B][K][D] (example-major, iw.h) in ONE
// kernel -> loglik_x [B*K] = sum over pixels of x*l - softplus(l) against image [B][784], words [B*K][10] = the text decoder's
// log-softmax.  Reads the bound fp32 parameters and running statistics (either precision; no pack_weights, no workspace, no row
// limit from the plan's batch); touches no plan state.
int mnist_iw_score(MnistPlan*, const float* z, const float* image, int B, int K, float* loglik_x, float* words, hipStream_t);
// image-only VAE (mnist/model.py:188-232, mnist/imageonly/train_imageonly.py:60-71,114-127): one pass over B rows on the fp32 plan
// (a bf16 plan is refused), workspace mnist_image_step_workspace_bytes; and mnist_iw_score with the image decoder alone (no label
// decoder, no words): loglik_x is bit for bit what mnist_iw_score writes there.
int mnist_image_step(MnistPlan*, const mmvae_image_step_io&, int training, int do_backward, hipStream_t);
size_t mnist_image_step_workspace_bytes(const MnistPlan*);
int mnist_iw_score_image(MnistPlan*, const float* z, const float* image, int B, int K, float* loglik_x, hipStream_t);
