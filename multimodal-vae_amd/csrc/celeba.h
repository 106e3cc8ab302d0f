// CelebA MMVAE plan (celeba/model.py:14-57,91-196 ; celeba/train.py:60-81,131-147).
#pragma once
#include "layers.h"
#include "iw.h"
#include "../../include/mmvae_hip.h"

struct PlanBase;

struct CelebaPlan;
CelebaPlan* celeba_create(int D, int B);
void celeba_destroy(CelebaPlan*);
PlanBase* celeba_base(CelebaPlan*);
int celeba_step(CelebaPlan*, const mmvae_celeba_step_io&, int training, int do_backward, hipStream_t);
// image-only VAE (celeba/model.py:60-88): one pass over B rows in the one-pass carve (img_tower.h tower_image_step), and log p(x|z) alone
int celeba_image_step(CelebaPlan*, const mmvae_image_step_io&, int training, int do_backward, hipStream_t);
size_t celeba_image_step_workspace_bytes(const CelebaPlan*);
int celeba_iw_score_image(CelebaPlan*, void* ws, size_t wsb, const float* z, const float* image, int B, int K, float* loglik_x, hipStream_t);
// granular module entry points (drop-in nn.Module forwards); B rows, every call brings its workspace
int celeba_image_encoder_fwd(CelebaPlan*, void* ws, size_t wsb, const float* image, const uint8_t* mask, int training, float* out, hipStream_t);
int celeba_image_encoder_bwd(CelebaPlan*, void* ws, size_t wsb, const float* d_out, const uint8_t* mask, hipStream_t);
int celeba_image_decoder_fwd(CelebaPlan*, void* ws, size_t wsb, const float* z, int training, float* recon, hipStream_t);
int celeba_image_decoder_bwd(CelebaPlan*, void* ws, size_t wsb, const float* d_recon, const float* recon, float* dz, hipStream_t);
int celeba_attrs_encoder_fwd(CelebaPlan*, void* ws, size_t wsb, const float* attrs, int training, float* out, hipStream_t);
int celeba_attrs_encoder_bwd(CelebaPlan*, void* ws, size_t wsb, const float* d_out, hipStream_t);
int celeba_attrs_decoder_fwd(CelebaPlan*, void* ws, size_t wsb, const float* z, int training, float* recon, hipStream_t);
int celeba_attrs_decoder_bwd(CelebaPlan*, void* ws, size_t wsb, const float* d_recon, const float* recon, float* dz, hipStream_t);
// importance-weighted evaluation (include/mmvae_hip.h: mmvae_celeba_iw_*): celeba_iw_score (celeba.hip) runs the eval-mode
// decoder body and the two scoring kernels of celeba_iw.hip
int celeba_iw_score(CelebaPlan*, void* ws, size_t wsb, const float* z, const float* image, int B, int K, float* loglik_x, float* words,
                    hipStream_t);
size_t celeba_iw_workspace_bytes(const CelebaPlan*);
// forward-only scoring tail (iw.h IwTailArgs): raw bf16 NHWC [rows][32][32][32], image [rows / K][3][64][64]
int launch_celeba_iw_tail(const IwTailArgs&, hipStream_t);
// attribute scorer on fp32 parameters: Linear(D, 64) -> BatchNorm1d (running statistics) -> Swish -> Linear(64, 18) -> words
struct CelebaIwAttrsArgs {
    const float *w0, *b0, *gamma, *beta, *rmean, *rvar, *w1, *b1; float eps;
    const float* z; long long rows; int D;
    float* words;                    // [rows][18][2] = (log(1 - p), log p)
};
int launch_celeba_iw_attrs(const CelebaIwAttrsArgs&, hipStream_t);
int celeba_iw_attrs(CelebaPlan*, const float* z, long long rows, float* words, hipStream_t);
// test / profiling aids: replay of one named layer launch of the step (img_tower.h tower_named_gemm / tower_named_wgrad) on the workspace's
// contents, and the byte offset of a named workspace buffer (-1 if unknown)
int celeba_bench_layer(CelebaPlan*, void* ws, size_t wsb, const char* layer, int iters, hipStream_t);
long long celeba_debug_offset(CelebaPlan*, const char* name);
