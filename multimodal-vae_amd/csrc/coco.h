// COCO MMVAE plan (coco/model.py:22-90,147-312 ; coco/train.py:66-84,146-165).
#pragma once
#include "layers.h"
#include "../../include/mmvae_hip.h"

struct PlanBase;

struct CocoPlan;
CocoPlan* coco_create(int D, int B, int T);      // T: caption length (coco/utils.py:12-15: 102)
void coco_destroy(CocoPlan*);
PlanBase* coco_base(CocoPlan*);
int coco_steps(const CocoPlan*);
int coco_step(CocoPlan*, const mmvae_coco_step_io&, int training, int do_backward, hipStream_t);
// granular module entry points (drop-in nn.Module forwards); B rows, every call brings its workspace
int coco_image_encoder_fwd(CocoPlan*, void* ws, size_t wsb, const float* image, const uint8_t* m1, const uint8_t* m2, int training, float* out, hipStream_t);
int coco_image_encoder_bwd(CocoPlan*, void* ws, size_t wsb, const float* d_out, const uint8_t* m1, const uint8_t* m2, hipStream_t);
int coco_image_decoder_fwd(CocoPlan*, void* ws, size_t wsb, const float* z, int training, float* recon, hipStream_t);
int coco_image_decoder_bwd(CocoPlan*, void* ws, size_t wsb, const float* d_recon, const float* recon, float* dz, hipStream_t);
int coco_text_encoder_fwd(CocoPlan*, void* ws, size_t wsb, const float* text, float* out, hipStream_t);
int coco_text_encoder_bwd(CocoPlan*, void* ws, size_t wsb, const float* text, const float* d_out, hipStream_t);
int coco_text_decoder_fwd(CocoPlan*, void* ws, size_t wsb, const float* z, const float* sos, const uint8_t* keep, int training, float* sentence, hipStream_t);
int coco_text_decoder_bwd(CocoPlan*, void* ws, size_t wsb, const float* z, const float* sos, const uint8_t* keep, const float* sentence, const float* d_sentence, float* dz, hipStream_t);
