// MultiMNIST MMVAE plan (multimnist/model.py:21-93,150-307 ; multimnist/train.py:69-87,146-173).
#pragma once
#include "layers.h"
#include "text.h"
#include "../../include/mmvae_hip.h"

struct PlanBase;

struct MMPlan;
// (offset, length) runs of image_decoder.* / text_decoder.* in the flat buffers; returns their number (<= cap)
int mm_early_ranges(const MMPlan* P, long long* ranges, int cap);
MMPlan* mm_create(int D, int B);
void mm_destroy(MMPlan*);
PlanBase* mm_base(MMPlan*);
// forward (3 passes) + losses; training!=0 also runs backward into `grads` (which the caller zeroed)
int mm_step_fwd_bwd(MMPlan*, const mmvae_mm_step_io&, int training, int do_backward, hipStream_t);
// granular module entry points (drop-in modules); every call brings its own workspace
int mm_image_encoder_fwd(MMPlan*, void* ws, size_t wsb, const float* image, const uint8_t* m1, const uint8_t* m2,
                         int training, float* out, hipStream_t);
int mm_image_encoder_bwd(MMPlan*, void* ws, size_t wsb, const float* d_out, const uint8_t* m1, const uint8_t* m2, hipStream_t);
int mm_image_decoder_fwd(MMPlan*, void* ws, size_t wsb, const float* z, int training, float* recon, hipStream_t);
int mm_image_decoder_bwd(MMPlan*, void* ws, size_t wsb, const float* d_recon, const float* recon, float* dz, hipStream_t);
int mm_text_encoder_fwd(MMPlan*, void* ws, size_t wsb, const long long* text, float* out, hipStream_t);
int mm_text_encoder_bwd(MMPlan*, void* ws, size_t wsb, const long long* text, const float* d_out, hipStream_t);
int mm_text_decoder_fwd(MMPlan*, void* ws, size_t wsb, const float* z, int training, const uint8_t* keep,
                        const long long* force_tokens, float* words, long long* tokens, hipStream_t);
int mm_text_decoder_bwd(MMPlan*, void* ws, size_t wsb, const float* z, const uint8_t* keep, const long long* force_tokens,
                        const float* words, const long long* tokens, const float* d_words, float* dz, hipStream_t);
// importance-weighted evaluation: z [B][K][D] (B*K <= plan rows), image [B][1][50][50] -> loglik_x [B*K], words [B*K][4][12]
int mm_iw_score(MMPlan*, void* ws, size_t wsb, const float* z, const float* image, int B, int K, float* loglik_x, float* words,
                hipStream_t);
// image-only VAE (multimnist/model.py ImageVAE): one pass over B rows in the one-pass carve, and log p(x|z) alone
int mm_image_step(MMPlan*, const mmvae_image_step_io&, int training, int do_backward, hipStream_t);
size_t mm_image_step_workspace_bytes(const MMPlan*);
int mm_iw_score_image(MMPlan*, void* ws, size_t wsb, const float* z, const float* image, int B, int K, float* loglik_x, hipStream_t);
// makes `s` wait until the early gradient part of the last dp_split step is complete in the flat gradient buffer
int mm_wait_early_grads(MMPlan*, hipStream_t s);
int mm_bench_layer(MMPlan*, void* ws, size_t wsb, const char* layer, int iters, hipStream_t);
double mm_layer_flops(const MMPlan*, const char* layer);
double mm_layer_algo_flops(const MMPlan*, const char* layer);
double mm_layer_algo_bytes(const MMPlan*, const char* layer);
long long mm_debug_offset(MMPlan*, const char* name);
// the weight-refresh part of one prologue launch of mm_step alone (stage 0..2; -1: the unstaged launch)
int mm_debug_pack_stage(MMPlan*, int stage, int* blocks, hipStream_t);
