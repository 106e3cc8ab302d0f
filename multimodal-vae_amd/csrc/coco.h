// COCO MMVAE plan (coco/model.py:22-90,147-312 ; coco/train.py:66-84,146-165).
#pragma once
#include "layers.h"
#include "iw.h"
#include "../../include/mmvae_hip.h"

struct PlanBase;

struct CocoPlan;
CocoPlan* coco_create(int D, int B, int T);      // T: caption length (coco/utils.py:12-15: 102)
void coco_destroy(CocoPlan*);
PlanBase* coco_base(CocoPlan*);
int coco_steps(const CocoPlan*);
int coco_step(CocoPlan*, const mmvae_coco_step_io&, int training, int do_backward, hipStream_t);
// image-only VAE (coco/model.py:93-117): one pass over B rows in the one-pass carve (img_tower.h tower_image_step), and log p(x|z) alone
int coco_image_step(CocoPlan*, const mmvae_image_step_io&, int training, int do_backward, hipStream_t);
size_t coco_image_step_workspace_bytes(const CocoPlan*);
int coco_iw_score_image(CocoPlan*, void* ws, size_t wsb, const float* z, const float* image, int B, int K, float* loglik_x, hipStream_t);
// InfoVAE (coco/model.py:358-402): the image-only step + lambda_mmd * MMD(prior samples, z) beside the decoder (img_tower.h TowerLatentTerm)
int coco_infovae_step(CocoPlan*, const mmvae_infovae_step_io&, int training, int do_backward, hipStream_t);
size_t coco_infovae_step_workspace_bytes(const CocoPlan*);
// text-only VAE (coco/model.py:120-144): one pass over B rows in the one-pass carve, caption half only, and the squared error of the
// particle rows' sentences alone
int coco_text_step(CocoPlan*, const mmvae_text_step_io&, int training, int do_backward, hipStream_t);
size_t coco_text_step_workspace_bytes(const CocoPlan*);
int coco_iw_score_text(CocoPlan*, void* ws, size_t wsb, const float* z, const float* text, const float* sos, int B, int K, float* sse_y, hipStream_t);
// granular module entry points (drop-in nn.Module forwards); B rows, every call brings its workspace
int coco_image_encoder_fwd(CocoPlan*, void* ws, size_t wsb, const float* image, const uint8_t* m1, const uint8_t* m2, int training, float* out, hipStream_t);
int coco_image_encoder_bwd(CocoPlan*, void* ws, size_t wsb, const float* d_out, const uint8_t* m1, const uint8_t* m2, hipStream_t);
int coco_image_decoder_fwd(CocoPlan*, void* ws, size_t wsb, const float* z, int training, float* recon, hipStream_t);
int coco_image_decoder_bwd(CocoPlan*, void* ws, size_t wsb, const float* d_recon, const float* recon, float* dz, hipStream_t);
int coco_text_encoder_fwd(CocoPlan*, void* ws, size_t wsb, const float* text, float* out, hipStream_t);
int coco_text_encoder_bwd(CocoPlan*, void* ws, size_t wsb, const float* text, const float* d_out, hipStream_t);
int coco_text_decoder_fwd(CocoPlan*, void* ws, size_t wsb, const float* z, const float* sos, const uint8_t* keep, int training, float* sentence, hipStream_t);
int coco_text_decoder_bwd(CocoPlan*, void* ws, size_t wsb, const float* z, const float* sos, const uint8_t* keep, const float* sentence, const float* d_sentence, float* dz, hipStream_t);
// test / profiling aids (include/mmvae_hip.h: mmvae_coco_bench_layer / mmvae_coco_debug_offset)
int coco_bench_layer(CocoPlan*, void* ws, size_t wsb, const char* layer, int iters, hipStream_t);
long long coco_debug_offset(CocoPlan*, const char* name);
// importance-weighted evaluation (include/mmvae_hip.h: mmvae_coco_iw_*): coco_iw_score (coco.hip) runs the eval-mode image
// decoder body, the eval-mode caption decoder and the two scoring kernels of coco_iw.hip
int coco_iw_score(CocoPlan*, void* ws, size_t wsb, const float* z, const float* image, const float* text, const float* sos, int B, int K,
                  float* loglik_x, float* sse_y, hipStream_t);
size_t coco_iw_workspace_bytes(const CocoPlan*);
// forward-only scoring tail (iw.h IwTailArgs): raw bf16 NHWC [rows][16][16][64], image [rows / K][3][32][32]
int launch_coco_iw_tail(const IwTailArgs&, hipStream_t);
// sse[row] = sum over (t, e) of (sentence[row][t][e] - text[row / K][t][e])^2 for the B*K rows; both 16-byte aligned
int launch_coco_iw_text_sse(const float* sentence, const float* text, int B, int K, int steps, float* sse, hipStream_t);
