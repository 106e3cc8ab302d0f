// CelebA MMVAE plan (celeba/model.py:14-57,91-196 ; celeba/train.py:60-81,131-147).
#pragma once
#include "layers.h"
#include "../../include/mmvae_hip.h"

struct PlanBase;

struct CelebaPlan;
CelebaPlan* celeba_create(int D, int B);
void celeba_destroy(CelebaPlan*);
PlanBase* celeba_base(CelebaPlan*);
int celeba_step(CelebaPlan*, const mmvae_celeba_step_io&, int training, int do_backward, hipStream_t);
// granular module entry points (drop-in nn.Module forwards); B rows, every call brings its workspace
int celeba_image_encoder_fwd(CelebaPlan*, void* ws, size_t wsb, const float* image, const uint8_t* mask, int training, float* out, hipStream_t);
int celeba_image_encoder_bwd(CelebaPlan*, void* ws, size_t wsb, const float* d_out, const uint8_t* mask, hipStream_t);
int celeba_image_decoder_fwd(CelebaPlan*, void* ws, size_t wsb, const float* z, int training, float* recon, hipStream_t);
int celeba_image_decoder_bwd(CelebaPlan*, void* ws, size_t wsb, const float* d_recon, const float* recon, float* dz, hipStream_t);
int celeba_attrs_encoder_fwd(CelebaPlan*, void* ws, size_t wsb, const float* attrs, int training, float* out, hipStream_t);
int celeba_attrs_encoder_bwd(CelebaPlan*, void* ws, size_t wsb, const float* d_out, hipStream_t);
int celeba_attrs_decoder_fwd(CelebaPlan*, void* ws, size_t wsb, const float* z, int training, float* recon, hipStream_t);
int celeba_attrs_decoder_bwd(CelebaPlan*, void* ws, size_t wsb, const float* d_recon, const float* recon, float* dz, hipStream_t);
// test / profiling aids: replay of one named layer launch of the step (celeba.hip named_gemm / named_wgrad) on the workspace's
// contents, and the byte offset of a named workspace buffer (-1 if unknown)
int celeba_bench_layer(CelebaPlan*, void* ws, size_t wsb, const char* layer, int iters, hipStream_t);
long long celeba_debug_offset(CelebaPlan*, const char* name);
