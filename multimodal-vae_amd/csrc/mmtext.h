// Text-only VAE baseline of MultiMNIST (multimnist/model.py:123-147 TextVAE, multimnist/train_textonly.py): internal C++ API.
#pragma once
#include "../../include/mmvae_hip.h"
#include "layers.h"

struct MMTextPlan;
struct PlanBase;
MMTextPlan* mmtext_create(int n_latents, int n_hiddens, int batch);
void mmtext_destroy(MMTextPlan*);
PlanBase* mmtext_base(MMTextPlan*);
int mmtext_hidden(const MMTextPlan*);
int mmtext_step(MMTextPlan*, const mmvae_mm_text_step_io&, int training, int do_backward, hipStream_t);
int mmtext_encoder_fwd(MMTextPlan*, void* ws, size_t wsb, const long long* text, float* out, hipStream_t);
int mmtext_encoder_bwd(MMTextPlan*, void* ws, size_t wsb, const long long* text, const float* d_out, hipStream_t);
int mmtext_decoder_fwd(MMTextPlan*, void* ws, size_t wsb, const float* z, int training, const uint8_t* keep, const long long* force_tokens,
                       float* words, long long* tokens, hipStream_t);
int mmtext_decoder_bwd(MMTextPlan*, void* ws, size_t wsb, const float* z, const uint8_t* keep, const long long* force_tokens,
                       const float* words, const long long* tokens, const float* d_words, float* dz, hipStream_t);
int mmtext_iw_score(MMTextPlan*, void* ws, size_t wsb, const float* z, int B, int K, float* words, hipStream_t);
