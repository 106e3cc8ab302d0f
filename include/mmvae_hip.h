/* libmmvae_hip.so -- C-ABI of the MI355X (gfx950) MMVAE ELBO engine.
 *
 * The reference (wenxuanliu/multimodal-vae) has no FFI: its hot path is reached through the Python module surface
 * of <ds>/model.py and loss_function in <ds>/train.py.  Each entry point below names the reference code it
 * replaces (paths under the reference repo).  Conventions:
 *   - plain C types only; every device buffer is owned by the caller (e.g. tensor.data_ptr()); the library never
 *     allocates or frees device memory; scratch comes from a caller-provided workspace whose size is queried;
 *   - all work is enqueued on the caller's hipStream_t (passed as void*), no hidden synchronisation;
 *   - returns 0 on success or a negative MMVAE_E* code; mmvae_last_error() gives a thread-local message;
 *   - plans (mmvae_mm_t) are host-side descriptors: one host thread per plan, one process per GPU.
 */
#ifndef MMVAE_HIP_H
#define MMVAE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMVAE_OK 0
#define MMVAE_EINVAL (-1)
#define MMVAE_EHIP (-2)
#define MMVAE_ENOSPC (-3)
#define MMVAE_ESTATE (-4)
#define MMVAE_ETIMEOUT (-5)               /* a device-side exchange of the step gave up: the step is void (mmvae_step_status) */

int mmvae_init(int device);                 /* checks the device is gfx950, makes it current */
const char* mmvae_last_error(void);
const char* mmvae_version(void);
/* Priority policy of the engine's three side streams (second-modality path, weight gradients); call before the first
 * step of the process.  1 (the default): default priority.  0: lowest priority, the side streams only fill CUs the main
 * chain leaves idle -- up to 0.8 % faster (CelebA), but ONLY while no other stream of the process carries GPU work: with
 * an H2D copy stream or a collective library's stream (RCCL under torch.distributed) active, mixed priorities slow every
 * kernel down 2-3x.  MMVAE_ESTATE if the side streams already exist with the other policy. */
int mmvae_set_stream_policy(int flat);

/* ---- collective face: the path's ONE exchange step, for hosts without a communicator of their own ----------
 * In-place SUM all-reduce of the flat fp32 gradient buffer over RCCL / xGMI, enqueued on the caller's stream; fold the
 * 1/world averaging into mmvae_adam_step's grad_scale.  librccl is bound with dlopen on first use (a copy already loaded
 * in the process -- PyTorch's -- is reused); nothing else in the library depends on it.  Rank 0 creates the 128-byte id
 * (ncclUniqueId) and hands it to the other ranks out of band (file, socket, MPI); every rank then calls mmvae_comm_init
 * with its HIP device already selected.  A PyTorch host keeps torch.distributed. */
typedef struct mmvae_comm mmvae_comm_t;
int mmvae_comm_unique_id(void* out128);
int mmvae_comm_init(mmvae_comm_t** out, int rank, int world, const void* unique_id128);
int mmvae_allreduce_grads(mmvae_comm_t*, float* flat, size_t n, void* stream);
int mmvae_comm_world(const mmvae_comm_t*);
int mmvae_comm_destroy(mmvae_comm_t*);

/* ---------------------------------------------------------------- MultiMNIST plan (multimnist/model.py:21-93) */
typedef struct MMPlan mmvae_mm_t;
mmvae_mm_t* mmvae_mm_create(int n_latents, int batch);      /* MultimodalVAE(n_latents) at a fixed batch size */
void mmvae_mm_destroy(mmvae_mm_t*);
long long mmvae_mm_param_count(const mmvae_mm_t*);          /* scalars in the flat fp32 parameter buffer */
int mmvae_mm_num_params(const mmvae_mm_t*);                 /* tensors, state_dict order (52) */
/* name (<=127 chars), ndim, shape[4], element offset of parameter i */
int mmvae_mm_param_info(const mmvae_mm_t*, int i, char* name, int* ndim, int* shape, long long* offset);
long long mmvae_mm_bn_floats(const mmvae_mm_t*);            /* running_mean|running_var of every BatchNorm */
int mmvae_mm_num_bn(const mmvae_mm_t*);
int mmvae_mm_bn_info(const mmvae_mm_t*, int i, char* prefix, int* channels, long long* offset);
long long mmvae_mm_packed_elems(const mmvae_mm_t*);         /* bf16 elements of the packed weights */
long long mmvae_mm_packed_vec_elems(const mmvae_mm_t*);     /* fp32 */
long long mmvae_mm_gpk_elems(const mmvae_mm_t*);            /* fp32 elements of the packed weight gradients */
long long mmvae_mm_gpk_vec_elems(const mmvae_mm_t*);
size_t mmvae_mm_desc_bytes(const mmvae_mm_t*, int which);   /* which: 0 = weight table, 1 = gradient table */
int mmvae_mm_desc_copy(const mmvae_mm_t*, int which, void* host_out);   /* caller uploads it to the device */
size_t mmvae_mm_workspace_bytes(const mmvae_mm_t*);
/* workspace of ONE granular module call (the *_encoder_* / *_decoder_* entry points below run a single pass over B rows;
   the fused step batches 3 passes and needs mmvae_mm_workspace_bytes) */
size_t mmvae_mm_module_workspace_bytes(const mmvae_mm_t*);
int mmvae_mm_bind(mmvae_mm_t*, float* params, float* grads, float* bn_stats, long long* bn_num_batches_tracked,
                  void* packed_bf16, float* packed_vec, float* gpk, float* gpk_vec, void* desc_dev, void* gdesc_dev);
int mmvae_mm_pack_weights(mmvae_mm_t*, void* stream);    /* refresh bf16 GEMM-layout copies after params change */
/* map[i] (int32, param_count entries) = where flat parameter i's packed gradient lives: >= 0 index into gpk, <= -2:
 * -(index + 2) into gpk_vec, -1 none.  Built once per parameter layout; input of mmvae_adam_step_packed. */
int mmvae_mm_grad_map(mmvae_mm_t*, int* map, void* stream);
/* Test aid: the weight pack run over the gradient descriptor table.  src (flat, parameter layout) -> out_bf16 [gpk_elems] bf16 and
 * out_vec [gpk_vec_elems] fp32: element i of src lands at the place mmvae_mm_grad_map names for i (the inverse, by other code). */
int mmvae_mm_debug_pack_as_grads(mmvae_mm_t*, const float* src, void* out_bf16, float* out_vec, void* stream);

/* Optimizer arguments of mmvae_mm_step_io.early_adam (torch.optim.Adam semantics, as mmvae_adam_step_packed). */
struct mmvae_early_adam {
    float* m; float* v;                     /* Adam moments, flat like the parameters */
    long long* state;                       /* the 16-byte optimizer state block (mmvae_adam_step) */
    float lr, beta1, beta2, eps, grad_scale;
    const int* gmap;                        /* mmvae_mm_grad_map */
    int* ran;                               /* host int: set to 1 when the step issued the early part, 0 when it did not (serial mode, a step
                                             * without an image-decoder backward, ...): the caller then updates every range itself */
};
/* One 3-pass ELBO step (multimnist/train.py:150-168): forward of (image,text), (image), (text), the three
 * loss_function sums and -- if do_backward -- the gradient of loss_1+loss_2+loss_3 written to `grads`
 * (the step zeroes `grads` first, i.e. it includes optimizer.zero_grad()). */
typedef struct {
    void* ws; size_t ws_bytes;
    const long long* step_counter;          /* device int64 keying the RNG streams, may be NULL */
    const float* image;                     /* [B][1][50][50] */
    const long long* text;                  /* [B][4] */
    const float* eps;                       /* [3][B][D] or NULL (Philox) */
    const uint8_t* enc_mask1;               /* [2][B][400] keep flags or NULL */
    const uint8_t* enc_mask2;               /* [2][B][200] keep flags or NULL */
    const uint8_t* gru_keep;                /* [4][3B][100] keep flags or NULL */
    int enc_dropout, gru_dropout;           /* 0 turns the respective dropout off (p = 0 fixtures) */
    const long long* force_tokens;          /* [3B][4] or NULL: overrides the greedy feedback (test hook) */
    float kl_lambda;
    float lambda_xy[3], lambda_yx[3];
    unsigned long long seed;
    float* sums;                            /* out [16]: [0..2] BCE sums, [4..6] NLL sums, [8..10] KL sums */
    float* recon_image;                     /* out [3][B][2500] or NULL */
    float* recon_text;                      /* out [3][B][4][12] or NULL */
    float* mu; float* logvar;               /* out [3][B][D] or NULL */
    long long* tokens;                      /* out [3][B][4] or NULL */
    int pass_skip[3];                       /* 1: pass k absent from this step (multimnist/paired_weak.py:84-117,
                                             * modal_weak.py:87-117): no loss, no gradient, no BatchNorm running update */
    int defer_unpack;                       /* 1: GEMM-weight gradients stay in the packed buffers for mmvae_adam_step_packed
                                             * (loss.backward() + optimizer.step() of multimnist/train.py:168,173 in one pass) */
    int pack_first;                         /* 1: the step's prologue launch also refreshes the packed bf16 weights from the
                                             * parameters (what mmvae_mm_pack_weights does): set it after an optimizer step
                                             * instead of calling mmvae_mm_pack_weights -- one launch less on the step's chain */
    int dp_split;                           /* 1 (data-parallel replica): the gradients of image_decoder.* and text_decoder.* are
                                             * complete in `grads` before the encoders' backward has run -- order a communication
                                             * stream behind them with mmvae_mm_wait_early_grads and all-reduce those two parameter
                                             * ranges while the rest of the step runs; the other ranges are complete when the step is */
    const struct mmvae_early_adam* early_adam;  /* NULL, or (with defer_unpack = 1, no data parallelism): the optimizer update of image_decoder.* and
                                             * text_decoder.* is issued INSIDE the step, on the weight-gradient stream, as soon as their gradients are
                                             * complete -- it runs beside the encoders' backward instead of behind the whole step.  The caller finishes
                                             * the optimizer step with mmvae_adam_step_packed_ranges over the remaining ranges when *ran was set. */
} mmvae_mm_step_io;
int mmvae_mm_step(mmvae_mm_t*, const mmvae_mm_step_io*, int training, int do_backward, void* stream);
/* `stream` waits (hipStreamWaitEvent) for the early gradient part of the most recent dp_split step of this plan.
 * The collective itself stays with the host framework (torch.distributed over RCCL): INTEGRATION.md, Data parallelism. */
int mmvae_mm_wait_early_grads(mmvae_mm_t*, void* stream);

/* Granular modules (drop-in for ImageEncoder/ImageDecoder/TextEncoder/TextDecoder.forward + autograd backward).
 * Every forward keeps its saved activations in the workspace passed to it; pass the same one to the backward. */
int mmvae_mm_image_encoder_fwd(mmvae_mm_t*, void* ws, size_t ws_bytes, const float* image, const uint8_t* mask1,
                               const uint8_t* mask2, int training, float* out_mu_logvar, void* stream);   /* model.py:183-188 */
int mmvae_mm_image_encoder_bwd(mmvae_mm_t*, void* ws, size_t ws_bytes, const float* d_out, const uint8_t* mask1,
                               const uint8_t* mask2, void* stream);
int mmvae_mm_image_decoder_fwd(mmvae_mm_t*, void* ws, size_t ws_bytes, const float* z, int training, float* recon,
                               void* stream);                                                           /* model.py:211-216 */
int mmvae_mm_image_decoder_bwd(mmvae_mm_t*, void* ws, size_t ws_bytes, const float* d_recon, const float* recon,
                               float* dz, void* stream);
int mmvae_mm_text_encoder_fwd(mmvae_mm_t*, void* ws, size_t ws_bytes, const long long* text, float* out_mu_logvar,
                              void* stream);                                                            /* model.py:237-247 */
int mmvae_mm_text_encoder_bwd(mmvae_mm_t*, void* ws, size_t ws_bytes, const long long* text, const float* d_out,
                              void* stream);
int mmvae_mm_text_decoder_fwd(mmvae_mm_t*, void* ws, size_t ws_bytes, const float* z, int training, const uint8_t* keep,
                              const long long* force_tokens, float* words, long long* tokens, void* stream); /* model.py:268-288 */
int mmvae_mm_text_decoder_bwd(mmvae_mm_t*, void* ws, size_t ws_bytes, const float* z, const uint8_t* keep,
                              const long long* force_tokens, const float* words, const long long* tokens,
                              const float* d_words, float* dz, void* stream);
/* Importance-weighted evaluation (the scoring step between mmvae_iw_particles and mmvae_iw_accumulate): eval-mode decoders on the
 * B*K particle rows z [B][K][n_latents] of a plan created with at least B*K rows; writes log p(x|z) [B*K] (sum over the 2500
 * pixels of x*l - softplus(l), l the pre-sigmoid logit: not clamped like the training BCE) and the text decoder's greedy
 * log-softmax outputs words [B*K][4][12].  image [B][1][50][50] are the examples the rows belong to (row b*K + k: example b).
 * No backward activations are kept; the BatchNorm running statistics are not touched.  Workspace: mmvae_mm_iw_workspace_bytes. */
size_t mmvae_mm_iw_workspace_bytes(const mmvae_mm_t*);
int mmvae_mm_iw_score(mmvae_mm_t*, void* ws, size_t ws_bytes, const float* z, const float* image, int B, int K, float* loglik_x,
                      float* words, void* stream);
/* Runs one named GEMM of the step `iters` times on the workspace contents of the last step (profiling aid).
 * "image_step:waist_fwd" | "image_step:chain_fwd" | "image_step:waist_bwd" | "image_step:chain_bwd" (test aid): the middle of
 * mmvae_mm_image_step again -- classifier.3 to z, or dz back to classifier.0's output gradient -- fused or unfused, in training mode
 * with dropout at kl_lambda = 1e-3, on the one-pass workspace of a step that drew its own eps and masks.
 * "enc_conv1_mfma" | "enc_conv1_wgrad_mfma": the first conv and its weight gradient as the fused step launches them (two workgroups
 * per image on the fp32 image batch, read from the first B * 2500 floats of tmp_f32; the gradient goes into the packed gradient
 * with float atomics) -- "enc_conv1" / "enc_conv1_wgrad" are the generic GEMMs over patches1 of the unfused step.
 * "dec_last_fused": the fused decoder tail of the step (3 BatchNorm groups, 2 with a last layer and a gradient; raw input q3, statistics
 * st_d2, target in tmp_f32, loss weights 1 / (B * 2500), BCE sums into sums); "dec_last_fused_reduce": the same followed by the sum of
 * its weight-gradient partials into the packed gradient, with logits / recon / dlogit written to the buffers of those names.
 * "enc_fc1_dgrad": classifier.0's data gradient as the encoder backward launches it -- four pixel classes, dy1 -> db4 for both dropout
 * variants against the saved r4 the B images share, conv4's BatchNorm tables aff_e2 / mr_e2 and its backward sums into red_e2. */
int mmvae_mm_bench_layer(mmvae_mm_t*, void* ws, size_t ws_bytes, const char* layer, int iters, void* stream);
double mmvae_mm_layer_flops(const mmvae_mm_t*, const char* layer);        /* executed: 2*rows*N*K, zero-padded taps included */
double mmvae_mm_layer_algo_flops(const mmvae_mm_t*, const char* layer);   /* algorithmic: the FlopCounterMode count of the reference layer */
double mmvae_mm_layer_algo_bytes(const mmvae_mm_t*, const char* layer);   /* algorithmic: each operand read once, the result written once (0: not a conv layer) */
/* measurement aid: GEMM FLOPs enqueued by this process since the last reset (counted on the host by the launchers) */
double mmvae_debug_flops(int reset);
/* test / A-B aid: named integer switches read by the launchers ("convres" = 0 turns the image-resident conv kernels off;
 * "coco_module_bf16" = 1 makes mmvae_coco_text_{encoder,decoder}_{fwd,bwd} run the training step's bf16 persistent caption
 * kernels on the module's B rows instead of the fp32 ones, 2 the forward ones without saving anything for a backward pass --
 * the backward entries then return MMVAE_EINVAL; a cluster launch that gave up waiting puts a NaN into element 0 of
 * sentence / dz.  csrc/knobs.h is the table of all of them, with their defaults).  A key the table lacks is MMVAE_EINVAL and
 * mmvae_last_error names it.  mmvae_debug_get: the current value and the default (either pointer may be NULL).
 * mmvae_debug_reset: one knob back to its default, NULL: all of them.  mmvae_debug_knob_name: the table's i-th name, NULL past
 * its end. */
int mmvae_debug_set(const char* key, int value);
int mmvae_debug_get(const char* key, int* value, int* dflt);
int mmvae_debug_reset(const char* key);
const char* mmvae_debug_knob_name(int i);
/* test aid: byte offset of a named intermediate inside the workspace (-1 if unknown); "image_step:<name>": inside the one-pass
 * workspace of mmvae_mm_image_step and of the module entry points */
long long mmvae_mm_debug_offset(mmvae_mm_t*, const char* name);
/* test aid: the weight-refresh part of ONE prologue launch of the fused step on `stream`, nothing zeroed or drawn: stage 0 the
 * main stream's, 1 and 2 the second-modality stream's, -1 the unstaged launch that refreshes every copy.
 * blocks (may be NULL): the number of pack workgroups of that launch. */
int mmvae_mm_debug_pack_stage(mmvae_mm_t*, int stage, int* blocks, void* stream);

/* ---------------------------------------------------------------- MNIST (mnist/model.py, mnist/train.py)
 * MultimodalVAE of mnist/model.py:14-50: Linear -> BatchNorm1d -> ReLU stacks (ImageEncoder :99-118, ImageDecoder
 * :121-133, TextEncoder :136-153, TextDecoder :156-170), ProductOfExperts :173-185, loss_function mnist/train.py:64-81.
 * The plan/query/bind/pack functions have the same meaning as their mmvae_mm_* counterparts above. */
typedef struct MnistPlan mmvae_mnist_t;
mmvae_mnist_t* mmvae_mnist_create(int n_latents, int batch);      /* MultimodalVAE(n_latents) mnist/model.py:14-20 */
/* precision 0 (default of mmvae_mnist_create): fp32 operands on fp32 MFMA, fp32 activations -- the reference's own
 * arithmetic (this model is Linear->BatchNorm1d->ReLU: bf16 operand rounding flips ReLU decisions and moves gradients by
 * 10-30 %); precision 1: bf16 MFMA operands like the conv models.  -1: environment MMVAE_MNIST_PRECISION=fp32|bf16 */
mmvae_mnist_t* mmvae_mnist_create_p(int n_latents, int batch, int precision);
int mmvae_mnist_precision(const mmvae_mnist_t*);
void mmvae_mnist_destroy(mmvae_mnist_t*);
long long mmvae_mnist_param_count(const mmvae_mnist_t*);
int mmvae_mnist_num_params(const mmvae_mnist_t*);
int mmvae_mnist_param_info(const mmvae_mnist_t*, int i, char* name128, int* ndim, int* shape4, long long* offset);
long long mmvae_mnist_bn_floats(const mmvae_mnist_t*);
int mmvae_mnist_num_bn(const mmvae_mnist_t*);
int mmvae_mnist_bn_info(const mmvae_mnist_t*, int i, char* prefix128, int* channels, long long* offset);
long long mmvae_mnist_packed_elems(const mmvae_mnist_t*);
long long mmvae_mnist_packed_vec_elems(const mmvae_mnist_t*);
long long mmvae_mnist_gpk_elems(const mmvae_mnist_t*);
long long mmvae_mnist_gpk_vec_elems(const mmvae_mnist_t*);
size_t mmvae_mnist_desc_bytes(const mmvae_mnist_t*, int which);
int mmvae_mnist_desc_copy(const mmvae_mnist_t*, int which, void* host_out);
size_t mmvae_mnist_workspace_bytes(const mmvae_mnist_t*);
/* workspace of ONE granular module call (the *_encoder_* / *_decoder_* entry points below run a single pass over B rows;
   the fused step batches 3 passes and needs mmvae_mnist_workspace_bytes) */
size_t mmvae_mnist_module_workspace_bytes(const mmvae_mnist_t*);
int mmvae_mnist_bind(mmvae_mnist_t*, float* params, float* grads, float* bn_stats, long long* num_batches_tracked,
                     void* packed_bf16, float* packed_vec, float* gpk, float* gpk_vec, void* desc_dev, void* gdesc_dev);
int mmvae_mnist_pack_weights(mmvae_mnist_t*, void* stream);
int mmvae_mnist_grad_map(mmvae_mnist_t*, int* map, void* stream);                /* as mmvae_mm_grad_map */
int mmvae_mnist_debug_pack_as_grads(mmvae_mnist_t*, const float* src, void* out_bf16, float* out_vec, void* stream);
/* The train() closure body of mnist/train.py:131-147 (3 passes, 3 losses, backward): same contract as mmvae_mm_step */
typedef struct {
    void* ws; size_t ws_bytes;
    const long long* step_counter;          /* device int64 keying the Philox eps stream, or NULL */
    const float* image;                     /* [B][1][28][28] fp32 */
    const long long* label;                 /* [B] int64 */
    const float* eps;                       /* [3][B][D] or NULL (drawn on device) */
    float lambda_xy[3]; float lambda_yx[3]; /* mnist/train.py:137-146: all 1 */
    float kl_coef;                          /* 1 / (B * 784/3)  (mnist/train.py:78-79) */
    unsigned long long seed;
    float* sums;                            /* out [16]: bce_sum[0..2], nll_sum[4..6], kl_sum[8..10] */
    float* recon_image;                     /* out [3][B][784] or NULL */
    float* recon_text;                      /* out [3][B][10] log-probs or NULL */
    float* mu; float* logvar;               /* out [3][B][D] or NULL */
    int pass_skip[3];                       /* 1: pass k absent from this step (mnist/paired_weak.py, mnist/modal_weak.py) */
} mmvae_mnist_step_io;
int mmvae_mnist_step(mmvae_mnist_t*, const mmvae_mnist_step_io*, int training, int do_backward, void* stream);
/* Granular modules of mnist/model.py (forward + autograd backward); workspace rules as for mmvae_mm_*_fwd/bwd.
 * Parameter gradients accumulate into the bound `grads`. */
int mmvae_mnist_image_encoder_fwd(mmvae_mnist_t*, void* ws, size_t ws_bytes, const float* image, int training,
                                  float* out_mu_logvar, void* stream);                          /* mnist/model.py:114-118 */
int mmvae_mnist_image_encoder_bwd(mmvae_mnist_t*, void* ws, size_t ws_bytes, const float* d_out, void* stream);
int mmvae_mnist_image_decoder_fwd(mmvae_mnist_t*, void* ws, size_t ws_bytes, const float* z, int training, float* recon,
                                  void* stream);                                                /* mnist/model.py:131-133 */
int mmvae_mnist_image_decoder_bwd(mmvae_mnist_t*, void* ws, size_t ws_bytes, const float* d_recon, const float* recon,
                                  float* dz, void* stream);
int mmvae_mnist_text_encoder_fwd(mmvae_mnist_t*, void* ws, size_t ws_bytes, const long long* label, int training,
                                 float* out_mu_logvar, void* stream);                           /* mnist/model.py:149-153 */
int mmvae_mnist_text_encoder_bwd(mmvae_mnist_t*, void* ws, size_t ws_bytes, const long long* label, const float* d_out,
                                 void* stream);
int mmvae_mnist_text_decoder_fwd(mmvae_mnist_t*, void* ws, size_t ws_bytes, const float* z, int training, float* log_probs,
                                 void* stream);                                                 /* mnist/model.py:168-170 */
int mmvae_mnist_text_decoder_bwd(mmvae_mnist_t*, void* ws, size_t ws_bytes, const float* d_log_probs, const float* log_probs,
                                 float* dz, void* stream);
/* Importance-weighted evaluation, the MNIST scoring step between mmvae_iw_particles and mmvae_iw_accumulate(T = 1, V = 10): ONE
 * kernel runs both eval-mode decoders (BatchNorm = the affine map of the running statistics) on the B*K particle rows
 * z [B][K][n_latents] (row b*K + k: example b) and writes loglik_x [B*K] = sum over the 784 pixels of x*l - softplus(l) (l the
 * pre-sigmoid logit, not clamped like the training BCE) against image [B][784], and words [B*K][10] = the text decoder's
 * log-softmax.  fp32 MFMA on the bound fp32 parameters whatever the plan's precision: no pack_weights, no workspace, any B*K
 * below 2^31 (independent of the plan's batch).  Nothing of the plan or the model is modified. */
int mmvae_mnist_iw_score(mmvae_mnist_t*, const float* z, const float* image, int B, int K, float* loglik_x, float* words,
                         void* stream);

/* ---------------------------------------------------------------- CelebA (celeba/model.py, celeba/train.py)
 * MultimodalVAE of celeba/model.py:14-57: conv ImageEncoder :91-128 / ImageDecoder :131-161 on 3x64x64 images,
 * AttributeEncoder :164-178 / AttributeDecoder :181-196 on 18 binary attributes (celeba/datasets.py:26-28),
 * loss_function celeba/train.py:60-81.  Plan/query/bind/pack functions as for mmvae_mm_*. */
typedef struct CelebaPlan mmvae_celeba_t;
mmvae_celeba_t* mmvae_celeba_create(int n_latents, int batch);    /* MultimodalVAE(n_latents) celeba/model.py:15-22 */
void mmvae_celeba_destroy(mmvae_celeba_t*);
long long mmvae_celeba_param_count(const mmvae_celeba_t*);
int mmvae_celeba_num_params(const mmvae_celeba_t*);
int mmvae_celeba_param_info(const mmvae_celeba_t*, int i, char* name128, int* ndim, int* shape4, long long* offset);
long long mmvae_celeba_bn_floats(const mmvae_celeba_t*);
int mmvae_celeba_num_bn(const mmvae_celeba_t*);
int mmvae_celeba_bn_info(const mmvae_celeba_t*, int i, char* prefix128, int* channels, long long* offset);
long long mmvae_celeba_packed_elems(const mmvae_celeba_t*);
long long mmvae_celeba_packed_vec_elems(const mmvae_celeba_t*);
long long mmvae_celeba_gpk_elems(const mmvae_celeba_t*);
long long mmvae_celeba_gpk_vec_elems(const mmvae_celeba_t*);
size_t mmvae_celeba_desc_bytes(const mmvae_celeba_t*, int which);
int mmvae_celeba_desc_copy(const mmvae_celeba_t*, int which, void* host_out);
size_t mmvae_celeba_workspace_bytes(const mmvae_celeba_t*);
/* workspace of ONE granular module call (the *_encoder_* / *_decoder_* entry points below run a single pass over B rows;
   the fused step batches 3 passes and needs mmvae_celeba_workspace_bytes) */
size_t mmvae_celeba_module_workspace_bytes(const mmvae_celeba_t*);
int mmvae_celeba_bind(mmvae_celeba_t*, float* params, float* grads, float* bn_stats, long long* num_batches_tracked,
                      void* packed_bf16, float* packed_vec, float* gpk, float* gpk_vec, void* desc_dev, void* gdesc_dev);
int mmvae_celeba_pack_weights(mmvae_celeba_t*, void* stream);
int mmvae_celeba_grad_map(mmvae_celeba_t*, int* map, void* stream);                /* as mmvae_mm_grad_map */
int mmvae_celeba_debug_pack_as_grads(mmvae_celeba_t*, const float* src, void* out_bf16, float* out_vec, void* stream);
/* The train() closure body of celeba/train.py:131-147 (3 passes, 3 losses, backward) */
typedef struct {
    void* ws; size_t ws_bytes;
    const long long* step_counter;          /* device int64 keying the Philox streams, or NULL */
    const float* image;                     /* [B][3][64][64] fp32 */
    const float* attrs;                     /* [B][18] fp32 */
    const float* eps;                       /* [3][B][D] or NULL (drawn on device) */
    const uint8_t* enc_mask;                /* [2][B][1024] keep flags of classifier Dropout(0.1) or NULL (drawn) */
    int enc_dropout;                        /* 0: no dropout */
    float kl_lambda;                        /* celeba/train.py:61 (1e-3) */
    float lambda_x[3]; float lambda_y[3];   /* celeba/train.py:138-147: all 1 */
    unsigned long long seed;
    float* sums;                            /* out [16]: image bce_sum[0..2], attrs bce_sum[4..6], kl_sum[8..10] */
    float* recon_image;                     /* out [3][B][3][64][64] or NULL */
    float* recon_attrs;                     /* out [3][B][18] or NULL */
    float* mu; float* logvar;               /* out [3][B][D] or NULL */
    int pass_skip[3];                       /* 1: pass k absent from this step */
    int defer_unpack;                       /* 1: the optimizer consumes the packed gradients itself (see the MultiMNIST step) */
} mmvae_celeba_step_io;
int mmvae_celeba_step(mmvae_celeba_t*, const mmvae_celeba_step_io*, int training, int do_backward, void* stream);
/* Test / profiling aids, as mmvae_mm_bench_layer / mmvae_mm_debug_offset: one named layer launch of the step `iters` times on the
 * workspace contents (enc_conv1..4, fc1, up, dec_convT1..3 and their _dgrad / _wgrad forms, fc2_dgrad, dec_last_dgrad_gemm,
 * dec_last_wgrad; the staged forms of the fused step: enc_conv3_staged, dec_convT2_staged, dec_convT3_staged,
 * enc_conv2/3_dgrad_staged, dec_convT2/3_dgrad_staged), and the byte
 * offset of a named intermediate inside the step's workspace (-1 if unknown). */
int mmvae_celeba_bench_layer(mmvae_celeba_t*, void* ws, size_t ws_bytes, const char* layer, int iters, void* stream);
long long mmvae_celeba_debug_offset(mmvae_celeba_t*, const char* name);
/* Granular modules (forward + autograd backward), workspace rules as for mmvae_mm_*_fwd/bwd */
int mmvae_celeba_image_encoder_fwd(mmvae_celeba_t*, void* ws, size_t ws_bytes, const float* image, const uint8_t* mask,
                                   int training, float* out_mu_logvar, void* stream);            /* celeba/model.py:124-128 */
int mmvae_celeba_image_encoder_bwd(mmvae_celeba_t*, void* ws, size_t ws_bytes, const float* d_out, const uint8_t* mask,
                                   void* stream);
int mmvae_celeba_image_decoder_fwd(mmvae_celeba_t*, void* ws, size_t ws_bytes, const float* z, int training, float* recon,
                                   void* stream);                                                /* celeba/model.py:157-161 */
int mmvae_celeba_image_decoder_bwd(mmvae_celeba_t*, void* ws, size_t ws_bytes, const float* d_recon, const float* recon,
                                   float* dz, void* stream);
int mmvae_celeba_attrs_encoder_fwd(mmvae_celeba_t*, void* ws, size_t ws_bytes, const float* attrs, int training,
                                   float* out_mu_logvar, void* stream);                          /* celeba/model.py:175-178 */
int mmvae_celeba_attrs_encoder_bwd(mmvae_celeba_t*, void* ws, size_t ws_bytes, const float* d_out, void* stream);
int mmvae_celeba_attrs_decoder_fwd(mmvae_celeba_t*, void* ws, size_t ws_bytes, const float* z, int training, float* recon,
                                   void* stream);                                                /* celeba/model.py:191-196 */
int mmvae_celeba_attrs_decoder_bwd(mmvae_celeba_t*, void* ws, size_t ws_bytes, const float* d_recon, const float* recon,
                                   float* dz, void* stream);
/* Importance-weighted evaluation, the CelebA scoring step between mmvae_iw_particles and mmvae_iw_accumulate(T = 18, V = 2) on the
 * B*K particle rows z [B][K][n_latents] (row b*K + k: example b; B*K at most the plan's batch):
 *   * the eval-mode image decoder body (the bf16 launches of mmvae_celeba_image_decoder_fwd up to the raw output of
 *     hallucinate.6), then ONE forward-only kernel per row: BatchNorm (running statistics) + Swish while staging, the last
 *     ConvTranspose2d(32, 3, 4, 2, 1) on the matrix cores, loglik_x [B*K] = sum over the 3x64x64 logits l of x*l - softplus(l)
 *     (not clamped like the training BCE) against image [B][3][64][64], summed in a fixed order (equal inputs: bit-equal sums);
 *   * the attribute decoder in fp32 on the bound fp32 parameters: words [B*K][18][2] = (log(1 - p_t), log p_t) of attribute t,
 *     so that targets = the attributes as int64 0 / 1 select log p(y_t | z) in mmvae_iw_accumulate.
 * Nothing of the plan's parameters, BatchNorm buffers or gradients is modified.  Workspace: mmvae_celeba_iw_workspace_bytes. */
size_t mmvae_celeba_iw_workspace_bytes(const mmvae_celeba_t*);
int mmvae_celeba_iw_score(mmvae_celeba_t*, void* ws, size_t ws_bytes, const float* z, const float* image, int B, int K,
                          float* loglik_x, float* words, void* stream);
/* Test hooks of the two scoring kernels.
 * mmvae_celeba_iw_tail needs no plan: q3_bf16 [B*K][32][32][32] (NHWC bf16, the raw output of hallucinate.6), affine [32][2]
 * (scale, shift) per channel, act one of 0 none / 1 Swish / 2 ReLU (the scoring call passes Swish), w (32,3,4,4) fp32 (rounded to
 * bf16 by the kernel), image [B][3][64][64]; loglik [B*K]; logits_or_null [B*K][3][64][64] fp32 receives the pre-sigmoid logits.
 * mmvae_celeba_iw_attrs is the attribute scorer the scoring call runs: z [rows][n_latents] fp32 -> words [rows][18][2], any
 * rows below 2^31 (independent of the plan's batch), no packed weights, no workspace. */
int mmvae_celeba_iw_tail(const void* q3_bf16, const float* affine, int act, const float* w, const float* image, int B, int K,
                         float* loglik, float* logits_or_null, void* stream);
int mmvae_celeba_iw_attrs(mmvae_celeba_t*, const float* z, long long rows, float* words, void* stream);

/* ---------------------------------------------------------------- COCO (coco/model.py, coco/train.py)
 * MultimodalVAE of coco/model.py:22-90: conv ImageEncoder :147-187 / ImageDecoder :190-216 on 3x32x32 images (the code's
 * size: Scale(32), coco/train.py:107-112), TextEncoder :219-245 (biGRU over `steps` 300-d GloVe vectors) / TextDecoder
 * :248-312 (2-layer GRU regressing one 300-d vector per step, fed back as the next input), loss_function
 * coco/train.py:66-84 (BCE + MSE + KL).  Plan/query/bind/pack functions as for mmvae_mm_*. */
typedef struct CocoPlan mmvae_coco_t;
mmvae_coco_t* mmvae_coco_create(int n_latents, int batch);        /* MultimodalVAE(n_latents), steps = 102 (coco/utils.py:12-15) */
mmvae_coco_t* mmvae_coco_create_t(int n_latents, int batch, int steps);   /* other caption lengths (tests) */
void mmvae_coco_destroy(mmvae_coco_t*);
int mmvae_coco_steps(const mmvae_coco_t*);
long long mmvae_coco_param_count(const mmvae_coco_t*);
int mmvae_coco_num_params(const mmvae_coco_t*);
int mmvae_coco_param_info(const mmvae_coco_t*, int i, char* name128, int* ndim, int* shape4, long long* offset);
long long mmvae_coco_bn_floats(const mmvae_coco_t*);
int mmvae_coco_num_bn(const mmvae_coco_t*);
int mmvae_coco_bn_info(const mmvae_coco_t*, int i, char* prefix128, int* channels, long long* offset);
long long mmvae_coco_packed_elems(const mmvae_coco_t*);
long long mmvae_coco_packed_vec_elems(const mmvae_coco_t*);
long long mmvae_coco_gpk_elems(const mmvae_coco_t*);
long long mmvae_coco_gpk_vec_elems(const mmvae_coco_t*);
size_t mmvae_coco_desc_bytes(const mmvae_coco_t*, int which);
int mmvae_coco_desc_copy(const mmvae_coco_t*, int which, void* host_out);
size_t mmvae_coco_workspace_bytes(const mmvae_coco_t*);
/* workspace of ONE granular module call (the *_encoder_* / *_decoder_* entry points below run a single pass over B rows;
   the fused step batches 3 passes and needs mmvae_coco_workspace_bytes) */
size_t mmvae_coco_module_workspace_bytes(const mmvae_coco_t*);
int mmvae_coco_bind(mmvae_coco_t*, float* params, float* grads, float* bn_stats, long long* num_batches_tracked,
                    void* packed, float* packed_vec, float* gpk, float* gpk_vec, void* desc_dev, void* gdesc_dev);
int mmvae_coco_pack_weights(mmvae_coco_t*, void* stream);
int mmvae_coco_grad_map(mmvae_coco_t*, int* map, void* stream);                /* as mmvae_mm_grad_map */
int mmvae_coco_debug_pack_as_grads(mmvae_coco_t*, const float* src, void* out_bf16, float* out_vec, void* stream);
/* The train() closure body of coco/train.py:138-173 (3 passes, 3 losses, backward) */
typedef struct {
    void* ws; size_t ws_bytes;
    const long long* step_counter;          /* device int64 keying the Philox streams, or NULL */
    const float* image;                     /* [B][3][32][32] fp32 */
    const float* text;                      /* [B][steps][300] fp32 GloVe vectors (coco/utils.py:36-47) */
    const float* sos;                       /* [300] GloVe('<s>') (coco/model.py:271-272) */
    const float* eps;                       /* [3][B][D] or NULL (drawn on device) */
    const uint8_t* enc_mask1;               /* [2][B][1024] keep flags of classifier Dropout 1 or NULL (drawn) */
    const uint8_t* enc_mask2;               /* [2][B][256] */
    const uint8_t* gru_keep;                /* [steps][3B][200] keep flags of the decoder GRU's inter-layer dropout or NULL */
    int enc_dropout; int gru_dropout;       /* 0: no dropout */
    float kl_lambda;                        /* coco/train.py:67 (1e-3) */
    float lambda_xy[3]; float lambda_yx[3]; /* coco/train.py:152-164: (1,1,0) and (1,1,1) */
    unsigned long long seed;
    float* sums;                            /* out [16]: image bce_sum[0..2], text squared-error sum[4..6], kl_sum[8..10] */
    float* recon_image;                     /* out [3][B][3][32][32] or NULL */
    float* recon_text;                      /* out [3][B][steps][300] or NULL */
    float* mu; float* logvar;               /* out [3][B][D] or NULL */
    int pass_skip[3];                       /* 1: pass k absent from this step */
    int defer_unpack;                       /* 1: the optimizer consumes the packed gradients itself (see the MultiMNIST step) */
    int pack_first;                         /* 1: the step refreshes the packed bf16 weights itself (the caller skipped mmvae_coco_pack_weights
                                               after the optimizer step): caption half on the text stream, image half on the main one */
    long long* optimizer_state;             /* the 16-byte state block this step's mmvae_adam_step* call will get, or NULL.  The caption
                                               decoder's workgroups exchange hidden-state slices through memory and give up after a
                                               bounded spin (a device that cannot keep them co-resident); such a step is void: its `sums`
                                               are NaN, its gradient is marked (element 0 = the NaN 0x7fc0dead, whose payload survives a SUM all-reduce) and
                                               the skip word of this block is set -- mmvae_adam_step* then leaves parameters, moments
                                               and step count untouched.  mmvae_step_status reports it to the host */
} mmvae_coco_step_io;
int mmvae_coco_step(mmvae_coco_t*, const mmvae_coco_step_io*, int training, int do_backward, void* stream);
/* Granular modules (forward + autograd backward), workspace rules as for mmvae_mm_*_fwd/bwd */
int mmvae_coco_image_encoder_fwd(mmvae_coco_t*, void* ws, size_t ws_bytes, const float* image, const uint8_t* mask1,
                                 const uint8_t* mask2, int training, float* out_mu_logvar, void* stream);  /* coco/model.py:182-187 */
int mmvae_coco_image_encoder_bwd(mmvae_coco_t*, void* ws, size_t ws_bytes, const float* d_out, const uint8_t* mask1,
                                 const uint8_t* mask2, void* stream);
int mmvae_coco_image_decoder_fwd(mmvae_coco_t*, void* ws, size_t ws_bytes, const float* z, int training, float* recon,
                                 void* stream);                                                  /* coco/model.py:211-216 */
int mmvae_coco_image_decoder_bwd(mmvae_coco_t*, void* ws, size_t ws_bytes, const float* d_recon, const float* recon,
                                 float* dz, void* stream);
int mmvae_coco_text_encoder_fwd(mmvae_coco_t*, void* ws, size_t ws_bytes, const float* text, float* out_mu_logvar,
                                void* stream);                                                   /* coco/model.py:236-245 */
int mmvae_coco_text_encoder_bwd(mmvae_coco_t*, void* ws, size_t ws_bytes, const float* text, const float* d_out, void* stream);
int mmvae_coco_text_decoder_fwd(mmvae_coco_t*, void* ws, size_t ws_bytes, const float* z, const float* sos,
                                const uint8_t* keep, int training, float* sentence, void* stream);  /* coco/model.py:266-288 */
int mmvae_coco_text_decoder_bwd(mmvae_coco_t*, void* ws, size_t ws_bytes, const float* z, const float* sos,
                                const uint8_t* keep, const float* sentence, const float* d_sentence, float* dz, void* stream);
/* Test / profiling aids, as mmvae_celeba_bench_layer / mmvae_celeba_debug_offset: one named launch of the step's image half
 * `iters` times on the workspace contents, built by the same definitions the step calls (csrc/coco.hip layer_gemm / layer_wgrad and
 * the builders of the stand-alone passes), and the byte offset of a named intermediate inside the step's workspace (-1 if
 * unknown).  The classifier runs its 2 dropout variants, the decoder 3 passes.  Layer names:
 *   enc_conv1, enc_conv1_wgrad; enc_conv2..4 and dec_convT1..3, each with _dgrad and _wgrad;
 *   fc1, fc2, fc3, up, each with _wgrad and _dgrad (knob "coco_layer_mask" 1: the keep flags in m1 / m2 take part);
 *   dec_last_dgrad_gemm, dec_last_wgrad;
 *   the stand-alone passes enc_bn2..4, dec_bn1..3 (BatchNorm + Swish, training mode, encoder 2 / decoder 1 running-statistics
 *   updates per group) and their _bwd forms (enc_bn4_bwd sums the two variants' gradients), im2col_dlogit (dlogit -> patches4),
 *   dec_last_fwd (target in tmp_f32, loss weights (1, 1/2, 0) / (B * 3072), logits [3B][3][32][32] at the start of slab, recon
 *   behind them, dlogit and the BCE sums where the step writes them). */
int mmvae_coco_bench_layer(mmvae_coco_t*, void* ws, size_t ws_bytes, const char* layer, int iters, void* stream);
long long mmvae_coco_debug_offset(mmvae_coco_t*, const char* name);
/* Importance-weighted evaluation, the COCO scoring step between mmvae_iw_particles and mmvae_iw_accumulate(T = 1, V = 1) on the
 * B*K particle rows z [B][K][n_latents] (row b*K + k: example b; B*K at most the plan's batch):
 *   * the eval-mode image decoder body (the bf16 launches of mmvae_coco_image_decoder_fwd up to the raw output of
 *     hallucinate.6), then ONE forward-only kernel per row: BatchNorm (running statistics) + Swish in registers, the last
 *     ConvTranspose2d(64, 3, 4, 2, 1) on the matrix cores, loglik_x [B*K] = sum over the 3x32x32 logits l of x*l - softplus(l)
 *     (not clamped like the training BCE) against image [B][3][32][32], summed in a fixed order (equal inputs: bit-equal sums);
 *   * the eval-mode caption decoder (the launches of mmvae_coco_text_decoder_fwd: own-output feedback, no dropout) into a sentence
 *     buffer [B*K][steps][300] of the workspace, then sse_y [B*K] = sum over (t, e) of (sentence - text[b])^2 against text
 *     [B][steps][300] (16-byte aligned), fp32 differences folded in a fixed order.  The caller turns it into a log-likelihood:
 *     log p(y|z) = -sse_y / (2 sigma^2) - (steps * 300 / 2) log(2 pi sigma^2), the model under which the training MSE is the NLL.
 * Nothing of the plan's parameters, BatchNorm buffers or gradients is modified.  Workspace: mmvae_coco_iw_workspace_bytes. */
size_t mmvae_coco_iw_workspace_bytes(const mmvae_coco_t*);
int mmvae_coco_iw_score(mmvae_coco_t*, void* ws, size_t ws_bytes, const float* z, const float* image, const float* text,
                        const float* sos, int B, int K, float* loglik_x, float* sse_y, void* stream);
/* Test hooks of the two scoring kernels; neither needs a plan.
 * mmvae_coco_iw_tail: q3_bf16 [B*K][16][16][64] (NHWC bf16, the raw output of hallucinate.6), affine [64][2] (scale, shift) per
 * channel, act one of 0 none / 1 Swish / 2 ReLU (the scoring call passes Swish), w (64,3,4,4) fp32 (rounded to bf16 by the
 * kernel), image [B][3][32][32]; loglik [B*K]; logits_or_null [B*K][3][32][32] fp32 receives the pre-sigmoid logits.
 * mmvae_coco_iw_text_sse: sentence [B*K][steps][300], text [B][steps][300] (both 16-byte aligned) -> sse [B*K]. */
int mmvae_coco_iw_tail(const void* q3_bf16, const float* affine, int act, const float* w, const float* image, int B, int K,
                       float* loglik, float* logits_or_null, void* stream);
int mmvae_coco_iw_text_sse(const float* sentence, const float* text, int B, int K, int steps, float* sse, void* stream);

/* ---------------------------------------------------------------- image-only VAE baselines (CelebA, COCO)
 * ImageVAE of celeba/model.py:60-88 and coco/model.py:93-117 -- the family's ImageEncoder and ImageDecoder with reparametrize between
 * them and NO product of experts -- trained by celeba/train_imageonly.py:95-113 / coco/train_imageonly.py on
 * loss = lambda_x * BCE(recon, image) / (B * pixels) + kl_lambda * KL / B.  The step runs on the family's existing plan and buffers under the
 * image_encoder.* / image_decoder.* names of its parameter table; the second modality's parameters are never read, and their
 * gradients are exactly 0 after a step with do_backward (which includes optimizer.zero_grad(), as the 3-pass steps do).
 * ONE pass over B rows: encoder with one Dropout variant and one BatchNorm running-statistics update, the one-expert latent block
 * (mmvae_latent1_*), decoder with one BatchNorm group, sigmoid + BCE, backward.  Workspace: the one-pass carve,
 * mmvae_<family>_image_step_workspace_bytes (== mmvae_<family>_module_workspace_bytes). */
typedef struct {
    void* ws; size_t ws_bytes;
    const long long* step_counter;          /* device int64 keying the Philox streams, or NULL */
    const float* image;                     /* [B][3][64][64] (CelebA) / [B][3][32][32] (COCO) fp32 */
    const float* eps;                       /* [B][D] or NULL (drawn on device) */
    const uint8_t* enc_mask1;               /* [B][1024] keep flags of the classifier's first Dropout(0.1) or NULL (drawn) */
    const uint8_t* enc_mask2;               /* COCO only: [B][256] keep flags of its second Dropout, given or NULL together with enc_mask1 */
    int enc_dropout;                        /* 0: no dropout */
    float kl_lambda;
    float lambda_x;
    unsigned long long seed;
    float* sums;                            /* out [16]: [0] BCE sum, [8] KL sum, the rest 0 */
    float* recon_image;                     /* out [B][3][side][side] or NULL */
    float* mu; float* logvar;               /* out [B][D] or NULL */
    int defer_unpack;                       /* 1: the optimizer consumes the packed gradients itself (see the MultiMNIST step) */
} mmvae_image_step_io;
int mmvae_celeba_image_step(mmvae_celeba_t*, const mmvae_image_step_io*, int training, int do_backward, void* stream);
size_t mmvae_celeba_image_step_workspace_bytes(const mmvae_celeba_t*);
int mmvae_coco_image_step(mmvae_coco_t*, const mmvae_image_step_io*, int training, int do_backward, void* stream);
size_t mmvae_coco_image_step_workspace_bytes(const mmvae_coco_t*);
/* COCO InfoVAE (coco/model.py:358-402, coco/train_infovae.py:44-55) as one enqueue: mmvae_coco_image_step with one more term,
 *   loss = lambda_x * BCE / (B * 3072) + lambda_mmd * MMD(true_samples, z) + kl_lambda * KL / B
 * (the reference's loss: lambda_x = lambda_mmd = 1, kl_lambda = 0), MMD as mmvae_mmd computes it with x = the prior samples and y = z.
 * Everything said of mmvae_coco_image_step holds: zero_grad included, one Dropout variant, one BatchNorm update per layer, nothing of
 * the caption half launched (its gradients exactly 0, its parameters and buffers not written), defer_unpack honoured, no host
 * synchronisation.  The MMD term runs as the y-only form of the pair sweep (mmvae_mmd_dy) and its fold on a side stream of the plan,
 * next to the decoder's forward and backward; the main stream waits for it once, in front of the latent block's backward, which adds
 * lambda_mmd * dMMD/dz to the decoder's dz.  With lambda_x = 0 the decoder's backward is skipped and the MMD gradient is the only dz;
 * with lambda_mmd = 0 the value is still reported and no gradient is formed.  true_samples NULL: drawn by the step's prologue on
 * Philox stream MMVAE_TRUE_SAMPLES_STREAM, keyed by seed and step_counter as eps (the values of mmvae_normal for that stream).
 * training = 0: z = mu, nothing drawn but the prior samples.  do_backward = 0: stops behind the losses, the sweep takes its
 * value-only form.  sums [16]: [0] BCE sum, [8] KL sum, [MMVAE_SUM_MMD_KXX .. MMVAE_SUM_MMD] = {mean Kxx, mean Kyy, mean Kxy, MMD},
 * every other slot 0.  Workspace: mmvae_coco_infovae_step_workspace_bytes = the one-pass carve + the sweep's partial sums, the MMD
 * gradient and the drawn samples, 16-byte aligned; nothing is allocated inside the step.
 * mmvae_coco_debug_offset "infovae_step:true_samples" | "infovae_step:dz_mmd" | "infovae_step:mmd_ws": those buffers' offsets. */
#define MMVAE_SUM_MMD_KXX 12
#define MMVAE_SUM_MMD_KYY 13
#define MMVAE_SUM_MMD_KXY 14
#define MMVAE_SUM_MMD 15
#define MMVAE_TRUE_SAMPLES_STREAM 5
typedef struct {
    void* ws; size_t ws_bytes;
    const long long* step_counter;          /* device int64 keying the Philox streams, or NULL */
    const float* image;                     /* [B][3][32][32] fp32 */
    const float* eps;                       /* [B][D] or NULL (drawn on device) */
    const uint8_t* enc_mask1;               /* [B][1024] keep flags of the classifier's first Dropout(0.1) or NULL (drawn) */
    const uint8_t* enc_mask2;               /* [B][256] keep flags of its second Dropout, given or NULL together with enc_mask1 */
    int enc_dropout;                        /* 0: no dropout */
    float kl_lambda;
    float lambda_x;
    unsigned long long seed;
    float* sums;                            /* out [16], see above */
    float* recon_image;                     /* out [B][3][32][32] or NULL */
    float* mu; float* logvar;               /* out [B][D] or NULL */
    int defer_unpack;                       /* 1: the optimizer consumes the packed gradients itself */
    const float* true_samples;              /* [B][D] prior samples or NULL (drawn on the device) */
    float lambda_mmd;                       /* weight of the MMD term; the reference's loss is lambda_x = lambda_mmd = 1, kl_lambda = 0 */
    float* z;                               /* out [B][D] or NULL */
} mmvae_infovae_step_io;
int mmvae_coco_infovae_step(mmvae_coco_t*, const mmvae_infovae_step_io*, int training, int do_backward, void* stream);
size_t mmvae_coco_infovae_step_workspace_bytes(const mmvae_coco_t*);
/* log p(x|z) of the baseline: mmvae_<family>_iw_score with the image half alone -- the eval-mode decoder body and the scoring tail
 * kernel write loglik_x [B*K]; the second modality's decoder does not run.  Workspace: mmvae_<family>_iw_workspace_bytes. */
int mmvae_celeba_iw_score_image(mmvae_celeba_t*, void* ws, size_t ws_bytes, const float* z, const float* image, int B, int K,
                                float* loglik_x, void* stream);
int mmvae_coco_iw_score_image(mmvae_coco_t*, void* ws, size_t ws_bytes, const float* z, const float* image, int B, int K,
                              float* loglik_x, void* stream);
/* MultiMNIST's ImageVAE (multimnist/model.py, trained by multimnist/train_imageonly.py) on the same struct: image [B][1][50][50],
 * enc_mask1 [B][400] and enc_mask2 [B][200] keep flags (each given or drawn on its own), coef = lambda_x / (B * 2500).  The plan is an
 * mmvae_mm_t at any n_latents 1..127; nothing of text_encoder.* / text_decoder.* is launched.  Workspace: the one-pass carve,
 * mmvae_mm_image_step_workspace_bytes (== mmvae_mm_module_workspace_bytes).  This family has a tower of its own, so the step runs
 * the launch forms of the mmvae_mm_image_* module entry points.  At n_latents = 20 and 100, with the switch "mm_image_waist" (mmvae_debug_set)
 * on, classifier.3 + classifier.6 + the latent block are ONE row-block launch per direction (csrc/mlp_tail.hip: 16 rows per workgroup from
 * classifier.0's output to z, and from dz back to classifier.0's output gradient) and one single-workgroup fold of their partial sums
 * beside the main chain; every other n_latents, or the switch at 0, runs classifier.3 / classifier.6, mmvae_latent1_fwd / _bwd and the
 * two data gradients as separate launches.  Both ways fold every sum of the latent block in a fixed order without float atomics.
 * mmvae_mm_iw_score_image: the image half of mmvae_mm_iw_score alone, loglik_x [B*K]; workspace mmvae_mm_iw_workspace_bytes. */
int mmvae_mm_image_step(mmvae_mm_t*, const mmvae_image_step_io*, int training, int do_backward, void* stream);
size_t mmvae_mm_image_step_workspace_bytes(const mmvae_mm_t*);
int mmvae_mm_iw_score_image(mmvae_mm_t*, void* ws, size_t ws_bytes, const float* z, const float* image, int B, int K, float* loglik_x,
                            void* stream);
/* MNIST's VAE (mnist/model.py:188-232, trained by mnist/imageonly/train_imageonly.py:60-71,114-127) on the same struct and an
 * mmvae_mnist_t of fp32 precision (a bf16 plan is refused; n_latents 4..124 in multiples of 4 as the plan takes them): image [B][784],
 * ONE pass over B rows -- image_encoder.net.0 .. 6, the one-expert latent block, image_decoder.net.0 .. 6, sigmoid + BCE, backward --
 * on the fp32 MFMA launches of the mmvae_mnist_image_* module entry points.  The model has no Dropout: enc_mask1 / enc_mask2 must be
 * NULL (refused otherwise) and enc_dropout is ignored; B = 1 in training is refused with BatchNorm's own message.  The reference's
 * loss (mean BCE + KLD / 784) / B is lambda_x = 1/B, kl_lambda = 1/784: sums[0] * lambda_x / (B * 784) + sums[8] * kl_lambda / B.
 * Nothing of text_encoder.* / text_decoder.* is launched: parameters, BatchNorm buffers and num_batches_tracked of that half keep
 * their bits, its gradient is exactly 0; the four image BatchNorms update their running statistics once.  The fp32 plan writes
 * every gradient straight into `grads` (defer_unpack is ignored): mmvae_adam_step over the leading image parameters is the optimizer.
 * Workspace: mmvae_mnist_image_step_workspace_bytes (a one-pass carve of its own; 0 for a bf16 plan).
 * mmvae_mnist_iw_score_image: mmvae_mnist_iw_score compiled without the label decoder and without the words output; loglik_x [B*K]
 * is bit for bit what mmvae_mnist_iw_score writes.  ws / ws_bytes are ignored (the scorer needs no workspace; the parameters keep the
 * shape of the other families' calls). */
int mmvae_mnist_image_step(mmvae_mnist_t*, const mmvae_image_step_io*, int training, int do_backward, void* stream);
size_t mmvae_mnist_image_step_workspace_bytes(const mmvae_mnist_t*);
int mmvae_mnist_iw_score_image(mmvae_mnist_t*, void* ws, size_t ws_bytes, const float* z, const float* image, int B, int K,
                               float* loglik_x, void* stream);
/* Column-strip fused layers (csrc/mnist_strip.hip): with the switch "mnist_strip" (mmvae_debug_set; 1 / 0, -1 or unset: the default, 1) on and a batch of at most
 * mmvae_mnist_strip_max_rows() rows, mmvae_mnist_image_step runs each Linear -> BatchNorm1d -> ReLU of the four BatchNorm layers as ONE
 * launch forward (a workgroup owns 16 output features and ALL rows: GEMM strip on the fp32 MFMA, two-pass batch statistics folded in a
 * fixed order through LDS, running-statistics update, affine + ReLU) and ONE launch backward (data gradient of the next Linear, ReLU',
 * the two BatchNorm sums, dgamma / dbeta and the raw-input gradient) -- no atomics, no grid-wide synchronisation, equal inputs give equal
 * bits.  Above the cap, or with the switch at 0, the step runs gemm_f32 + the BatchNorm kernels.  mmvae_mnist_step is not switched.
 * mmvae_mnist_strip_route(rows): 1 when the step takes the strip kernels at that batch, else 0.
 * mmvae_mnist_lin_bn_act_fwd / mmvae_mnist_lin_dgrad_bn_bwd (test and measurement aid): ONE such layer on plain device pointers.
 *   route 1: the strip kernel (more rows than the cap are refused); 0: the launches it replaces; -1: mmvae_mnist_strip_route(rows).
 *   fwd: x [rows][ldx], w [N][K], bias / gamma / beta / running_mean / running_var [N], nbt [1] -> r, a [rows][N], mean_rstd [N][2];
 *        training 1: batch statistics, the running statistics move once, *nbt += 1; 0: running statistics, no buffer written.
 *        The strip kernel needs K % 4 == 0, ldx % 4 == 0 and 16-byte aligned x, w.
 *   bwd: dy [rows][Nn] (gradient wrt the NEXT Linear's output), w_next [Nn][N], r [rows][N] and mean_rstd [N][2] of this layer ->
 *        d_r [rows][N]; dgamma, dbeta [N] +=.  The strip kernel needs Nn % 4 == 0 and a 16-byte aligned dy. */
int mmvae_mnist_strip_max_rows(void);
int mmvae_mnist_strip_route(int rows);
int mmvae_mnist_lin_bn_act_fwd(int route, const float* x, int ldx, const float* w, const float* bias, const float* gamma, const float* beta,
                               float* running_mean, float* running_var, long long* nbt, int rows, int N, int K, int training, float* r, float* a,
                               float* mean_rstd, void* stream);
int mmvae_mnist_lin_dgrad_bn_bwd(int route, const float* dy, int Nn, const float* w_next, const float* r, const float* mean_rstd,
                                 const float* gamma, const float* beta, int rows, int N, float* d_r, float* dgamma, float* dbeta, void* stream);
/* The one-expert latent block of that step, alone (D <= 128).  scratch: mmvae_latent1_scratch_floats(B, D) floats, 8-byte aligned, contents
 * undefined on entry and exit.  Every sum is folded in a fixed order without float atomics: equal inputs give equal bits.
 * fwd: enc_out [B][2D] -> mu, logvar [B][D] = its two halves bit for bit; z [B][D] = mu + eps * exp(logvar / 2) (training, the
 *   expression of mmvae_reparam_fwd) or mu; z_bf16 [B][ldz] = bf16(z), column D = 1.0 (the folded bias of upsample.0), the other pad
 *   columns 0; kl_sum[0] += -0.5 * sum(1 + logvar - mu^2 - exp(logvar)).
 * bwd: d_enc_out_bf16 [B][ld] = bf16 of (dz + kl_coef * mu | dz * eps * exp(logvar / 2) / 2 - kl_coef * (1 - exp(logvar)) / 2), pad
 *   columns [2D, ld) 0 (dz NULL: 0; training 0: no eps term); d_bias [2D] += column sums of the fp32 values (or NULL);
 *   loss_slots / loss_out (both or neither): loss_out[16] = sum of the [32][16] slot rows. */
size_t mmvae_latent1_scratch_floats(int B, int D);
int mmvae_latent1_fwd(const float* enc_out, const float* eps_or_null, int B, int D, int training, float* mu, float* logvar, float* z,
                      void* z_bf16, int ldz, float* kl_sum, float* scratch, void* stream);
int mmvae_latent1_bwd(const float* mu, const float* logvar, const float* eps_or_null, const float* dz_or_null, int B, int D, int training,
                      float kl_coef, void* d_enc_out_bf16, int ld, float* d_bias_or_null, const float* loss_slots_or_null,
                      float* loss_out_or_null, float* scratch, void* stream);
/* The same gradient in fp32 [B][ld] (ld >= 2D, pad columns exact zeros), for an encoder whose backward takes fp32: every element is the
 * fp32 rounding of the value mmvae_latent1_bwd rounds to bf16, so bf16(d_enc_out) equals its output bit for bit.  No bias sum, no
 * scratch, nothing is added up across threads. */
int mmvae_latent1_bwd_f32(const float* mu, const float* logvar, const float* eps_or_null, const float* dz_or_null, int B, int D,
                          int training, float kl_coef, float* d_enc_out, int ld, void* stream);

/* The streaming kernels every step runs (latent block of the three-pass models, losses, BatchNorm, embedding, column sums) on plain
 * device pointers (test and measurement aid).  Each call is exactly the launch the steps make; a shape the kernel would index out of
 * range is refused with a message.  bf16 tensors are passed as void*.  "slots" = the [32][16] loss accumulators of a step: a sum is
 * the fold of a column over the 32 rows.  "stat slots" = 16 replicas: stats / red are [G][16][C][2] and are folded over the 16.
 * latent3_fwd: img_out [2][B][2D] (mu | logvar of the image encoder, pass 0 and pass 1; img_out_b non-NULL: pass 1 is read there,
 *   [B][2D]), txt_out [B][2D] -> mu, logvar, z [3][B][D]: pass 0 = PoE{image 0, text}, pass 1 = PoE{image 1}, pass 2 = PoE{text} with
 *   PoE mu = sum(mu_i var_i) / sum(var_i), logvar = log(1 / sum(1 / var_i)), var_i = exp(logvar_i) + 1e-8 (so a one-expert pass is NOT
 *   a copy of its input); z = mu + eps * exp(logvar / 2) (eps [3][B][D]; training 0: eps may be NULL, z = mu bit for bit);
 *   z_bf16 [3B][ldz] (ldz % 8 == 0, >= D) = bf16(z), column D = 1.0, the other pad columns 0;
 *   kl_slots [32][16]: column k (k = 0..2) of row (workgroup % 32) += that workgroup's part of -0.5 sum(1 + logvar - mu^2 - exp(logvar)).
 * latent3_bwd: the gradient of  sum_k (<dz_a + dz_b, z_k> + kl_coef_k * KL_k)  wrt img_out / txt_out, from the mu / logvar the forward
 *   wrote.  dz_a, dz_b [3][B][D], each may be NULL.  The image gradient takes ONE of four forms: d_img_out_f32 [B][2D] = pass 0 + pass 1
 *   (then d_img_out_bf16 is not touched); else sum_img_variants 1: d_img_out_bf16 [B][ld] = bf16(pass 0 + pass 1); else
 *   d_img_out_bf16 [2][B][ld] = bf16 of each; ld = ld_img_out_bf (a multiple of 8 >= 2D, pad columns zeroed) or 2D when that is 0.
 *   d_txt_out [B][2D] fp32 and d_txt_out_bf16 [B][2D]: each optional.  d_img_bias, d_txt_bias [2D] += column sums (float atomics), each
 *   optional.  loss_slots / loss_out (both or neither): loss_out[16] = sum of the [32][16] slot rows.
 * sigmoid_bce: logits NHWC [G*B][H][W][ldl] (channel c at +c), target NCHW [B][C][H][W] shared by the G <= 4 groups, coef_host[G] (HOST
 *   floats) -> recon = sigmoid NCHW [G*B][C][H][W] (or NULL), dlogit = coef[g] * (p - t) / max(p (1 - p), 1e-12) * p (1 - p) (or NULL),
 *   loss_sum[g] += sum of -(t max(log p, -100) + (1 - t) max(log(1 - p), -100)): F.binary_cross_entropy of F.sigmoid in fp32.
 * logsoftmax_nll: logits [rows][classes] -> words = log_softmax; target (or NULL) int64 [target_rows], row r reads target[r %
 *   target_rows]; group g = r / rows_per_group (at most 4 groups); nll_slots [32][16] column g += sum of -words[r][target] (or NULL);
 *   dlogits_bf16 [rows][ld_d] (pads zero) and dlogits_f32 [rows][classes], each optional = coef_host[g] * (softmax - onehot);
 *   coef_host: one HOST float per group, ceil(rows / rows_per_group) of them are read.
 * bn_finalize: stats [G][16][C][2] (sum, sum of squares over `count` values) -> affine [G][C][2] = (gamma rstd, beta - mean gamma rstd),
 *   meanrstd [G][C][2]; biased variance E[x^2] - mean^2 clamped at 0; the running buffers move by torch's momentum update (unbiased
 *   variance) updates_per_group times per group in group order, except groups whose bit is set in skip_update_mask, and *nbt grows by
 *   updates_per_group * (groups not skipped).  running buffers / nbt may be NULL.  training 0: tables from the running buffers, nothing
 *   else written.
 * bn_act: the same tables (affine / meanrstd may both be NULL) and running update + a = act(r * scale + shift) on bf16 rows
 *   [rows][ld] (ld % 8 == 0, >= C rounded up to 8; columns [C, 8 ceil(C/8)) of a are written as 0), act 0 none / 1 swish / 2 relu;
 *   G * C <= 4096; rows <= G * rows_per_group.
 * bn_bwd_apply: dr = gamma rstd (db [+ db2] - sum_db / n - xhat sum_db_xhat / n), n = rows_per_group, from red [G][16][C][2] = (sum db,
 *   sum db xhat) and meanrstd; dr may alias db; dgamma[c] += sum over groups of sum_db_xhat, dbeta[c] += sum_db (each may be NULL).
 * embed_gather_stats: x_bf16 [rows][ld] = bf16(table[idx[r % idx_rows]][:C]), pads 0; colstats [G][16][C][2] += (sum, sum of squares)
 *   of the bf16 values per group of rows_per_group rows (or NULL).  embed_scatter_add: g_table[idx[r]][c] += d[r][c] (float atomics).
 * colsum_f32 / colsum_bf16: out[c] += sum_r x[r][c] for c < cols; bf16 rows have stride ld >= cols. */
int mmvae_latent3_fwd(const float* img_out, const float* img_out_b_or_null, const float* txt_out, const float* eps_or_null, int B, int D,
                      int training, float* mu, float* logvar, float* z, void* z_bf16, int ldz, float* kl_slots, void* stream);
int mmvae_latent3_bwd(const float* img_out, const float* img_out_b_or_null, const float* txt_out, const float* mu, const float* logvar,
                      const float* eps_or_null, const float* dz_a_or_null, const float* dz_b_or_null, int B, int D, int training,
                      float kl_coef0, float kl_coef1, float kl_coef2, void* d_img_out_bf16_or_null, int ld_img_out_bf, int sum_img_variants,
                      float* d_img_out_f32_or_null, float* d_img_bias_or_null, float* d_txt_out_or_null, void* d_txt_out_bf16_or_null,
                      float* d_txt_bias_or_null, const float* loss_slots_or_null, float* loss_out_or_null, void* stream);
int mmvae_sigmoid_bce(const float* logits, int ldl, const float* target, int G, int B, int C, int H, int W, const float* coef_host,
                      float* recon_or_null, float* dlogit_or_null, float* loss_sum, void* stream);
int mmvae_logsoftmax_nll(const float* logits, int rows, int classes, float* words, const long long* target_or_null, int target_rows,
                         int rows_per_group, float* nll_slots_or_null, void* dlogits_bf16_or_null, int ld_d, float* dlogits_f32_or_null,
                         const float* coef_host, void* stream);
int mmvae_bn_finalize(const float* stats, int G, int C, float count, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, long long* num_batches_tracked, int updates_per_group, unsigned skip_update_mask, float* affine,
                      float* meanrstd, float eps, float momentum, int training, void* stream);
int mmvae_bn_act(const void* r_bf16, void* a_bf16, int rows, int C, int ld, int rows_per_group, int G, int act, const float* stats,
                 float count, const float* gamma, const float* beta, float* running_mean, float* running_var, long long* num_batches_tracked,
                 int updates_per_group, unsigned skip_update_mask, float* affine_or_null, float* meanrstd_or_null, float eps, float momentum,
                 int training, void* stream);
int mmvae_bn_bwd_apply(const void* db_bf16, const void* db2_bf16_or_null, const void* r_bf16, void* dr_bf16, int rows, int C, int ld,
                       int rows_per_group, int G, const float* red, const float* meanrstd, const float* gamma, float* dgamma_or_null,
                       float* dbeta_or_null, void* stream);
int mmvae_embed_gather_stats(const float* table, int C, const long long* idx, int rows, int idx_rows, int rows_per_group, void* x_bf16,
                             int ld, float* colstats_or_null, void* stream);
int mmvae_embed_scatter_add(const void* d_bf16, int ld, int C, const long long* idx, int rows, float* g_table, void* stream);
int mmvae_colsum_f32(const float* x, int rows, int cols, float* out, void* stream);
int mmvae_colsum_bf16(const void* x_bf16, int ld, int rows, int cols, float* out, void* stream);

/* ---------------------------------------------------------------- text-only VAE baseline (COCO)
 * TextVAE of coco/model.py:120-144 -- TextEncoder and TextDecoder with reparametrize between them and NO product of experts -- trained
 * by coco/train_textonly.py:106-120 on loss = lambda_y * sum((recon - text)^2) / (B * steps * 300) + kl_lambda * KL / B.  The step runs
 * on the COCO plan and buffers under the text_encoder.* / text_decoder.* names of its parameter table (n_latents 4..124, a multiple of
 * 4: the operand padding of the caption kernels); the image half is never launched: its gradients are exactly 0 after a step with
 * do_backward (which includes optimizer.zero_grad()), its parameters, BatchNorm buffers and num_batches_tracked are not written.
 * ONE pass over B rows: the bf16 persistent caption encoder, the one-expert latent block (mmvae_latent1_fwd / mmvae_latent1_bwd_f32;
 * mu and logvar are the encoder's halves bit for bit), the caption decoder on one row group with the squared error, backward.
 * Workspace: the one-pass carve, mmvae_coco_text_step_workspace_bytes (== mmvae_coco_module_workspace_bytes). */
typedef struct {
    void* ws; size_t ws_bytes;
    const long long* step_counter;          /* device int64 keying the Philox streams, or NULL */
    const float* text;                      /* [B][steps][300] */
    const float* sos;                       /* [300] */
    const float* eps;                       /* [B][D] or NULL (drawn on device) */
    const uint8_t* gru_keep;                /* [steps][B][200] keep flags of the decoder's inter-layer Dropout or NULL (drawn) */
    int gru_dropout;                        /* 0: no dropout */
    float kl_lambda; float lambda_y;
    unsigned long long seed;
    float* sums;                            /* out [16]: [4] squared-error sum, [8] KL sum, the rest 0 */
    float* recon_text;                      /* out [B][steps][300] or NULL */
    float* mu; float* logvar;               /* out [B][D] or NULL */
    int defer_unpack; int pack_first;       /* as in mmvae_coco_step_io; pack_first refreshes the caption half's packed weights only */
    long long* optimizer_state;             /* as in mmvae_coco_step_io: a void step marks itself */
} mmvae_text_step_io;
int mmvae_coco_text_step(mmvae_coco_t*, const mmvae_text_step_io*, int training, int do_backward, void* stream);
size_t mmvae_coco_text_step_workspace_bytes(const mmvae_coco_t*);
/* sse_y of mmvae_coco_iw_score alone: the eval-mode caption decoder on the B*K particle rows and the squared-error kernel; the image
 * decoder does not run.  Workspace: mmvae_coco_iw_workspace_bytes. */
int mmvae_coco_iw_score_text(mmvae_coco_t*, void* ws, size_t ws_bytes, const float* z, const float* text, const float* sos,
                             int B, int K, float* sse_y, void* stream);

/* ---------------------------------------------------------------- text-only VAE baseline (MultiMNIST)
 * TextVAE of multimnist/model.py:123-147 -- TextEncoder and TextDecoder at n_hiddens = 50 with reparametrize between them and NO product
 * of experts -- trained by multimnist/train_textonly.py:95-113 on loss = lambda_y * NLL(recon, text) / (B * 4) + kl_lambda * KL / B.
 * A plan of its own: the parameter table is TextVAE's state_dict (encoder.embed.weight (12,H), encoder.gru.*_l0 / *_l0_reverse,
 * encoder.h2p.*, decoder.embed.weight, decoder.z2h.*, decoder.gru.*_l0 / *_l1, decoder.h2o.*), there is no BatchNorm (num_bn == 0,
 * bn_floats == 0: bind still wants non-null bn_stats / nbt pointers).  n_latents 1..127; n_hiddens 50 (the reference's) or 100 (the
 * MMVAE's width: the same kernels as mmvae_mm_text_*, bit for bit); anything else returns NULL and mmvae_last_error names 50 and 100.
 * The kernels are the MMVAE's persistent text kernels instantiated for the hidden size; at 50 the decoder's forward is the streamed
 * form at every latent size.  The plan/query/bind/pack functions have the same meaning as their mmvae_mm_* counterparts.
 * ONE workspace size: mmvae_mmtext_module_workspace_bytes (== mmvae_mmtext_workspace_bytes), one pass over B rows. */
typedef struct MMTextPlan mmvae_mmtext_t;
mmvae_mmtext_t* mmvae_mmtext_create(int n_latents, int n_hiddens, int batch);
void mmvae_mmtext_destroy(mmvae_mmtext_t*);
int mmvae_mmtext_hidden(const mmvae_mmtext_t*);
long long mmvae_mmtext_param_count(const mmvae_mmtext_t*);
int mmvae_mmtext_num_params(const mmvae_mmtext_t*);               /* 24 */
int mmvae_mmtext_param_info(const mmvae_mmtext_t*, int i, char* name, int* ndim, int* shape, long long* offset);
long long mmvae_mmtext_bn_floats(const mmvae_mmtext_t*);          /* 0 */
int mmvae_mmtext_num_bn(const mmvae_mmtext_t*);                   /* 0 */
int mmvae_mmtext_bn_info(const mmvae_mmtext_t*, int i, char* prefix, int* channels, long long* offset);
long long mmvae_mmtext_packed_elems(const mmvae_mmtext_t*);
long long mmvae_mmtext_packed_vec_elems(const mmvae_mmtext_t*);
long long mmvae_mmtext_gpk_elems(const mmvae_mmtext_t*);
long long mmvae_mmtext_gpk_vec_elems(const mmvae_mmtext_t*);
size_t mmvae_mmtext_desc_bytes(const mmvae_mmtext_t*, int which);
int mmvae_mmtext_desc_copy(const mmvae_mmtext_t*, int which, void* host_out);
size_t mmvae_mmtext_workspace_bytes(const mmvae_mmtext_t*);
size_t mmvae_mmtext_module_workspace_bytes(const mmvae_mmtext_t*);
int mmvae_mmtext_bind(mmvae_mmtext_t*, float* params, float* grads, float* bn_stats, long long* bn_num_batches_tracked,
                      void* packed_bf16, float* packed_vec, float* gpk, float* gpk_vec, void* desc_dev, void* gdesc_dev);
int mmvae_mmtext_pack_weights(mmvae_mmtext_t*, void* stream);
int mmvae_mmtext_grad_map(mmvae_mmtext_t*, int* map, void* stream);
int mmvae_mmtext_debug_pack_as_grads(mmvae_mmtext_t*, const float* src, void* out_bf16, float* out_vec, void* stream);
/* Granular modules, with the signatures and the meaning of mmvae_mm_text_* (keep: [4][B][H] flags). */
int mmvae_mmtext_encoder_fwd(mmvae_mmtext_t*, void* ws, size_t ws_bytes, const long long* text, float* out_mu_logvar, void* stream);
int mmvae_mmtext_encoder_bwd(mmvae_mmtext_t*, void* ws, size_t ws_bytes, const long long* text, const float* d_out, void* stream);
int mmvae_mmtext_decoder_fwd(mmvae_mmtext_t*, void* ws, size_t ws_bytes, const float* z, int training, const uint8_t* keep,
                             const long long* force_tokens, float* words, long long* tokens, void* stream);
int mmvae_mmtext_decoder_bwd(mmvae_mmtext_t*, void* ws, size_t ws_bytes, const float* z, const uint8_t* keep,
                             const long long* force_tokens, const float* words, const long long* tokens,
                             const float* d_words, float* dz, void* stream);
/* One step, one enqueue, everything on the caller's stream (no side stream is used): prologue (zeroing, Philox eps / keep flags,
 * optional pack_first), encoder forward, mmvae_latent1_fwd (mu | logvar are the encoder's halves bit for bit), decoder forward on one
 * row group with the fused NLL (coefficient lambda_y / (B * 4)), and -- if do_backward -- the decoder's backward with its grouped weight
 * gradients, mmvae_latent1_bwd_f32 (kl_coef = kl_lambda / B, ld = 2D), the encoder's backward, reduce and unpack (or defer_unpack).
 * The step includes optimizer.zero_grad().  training = 0: z = mu, no dropout. */
typedef struct {
    void* ws; size_t ws_bytes;
    const long long* step_counter;          /* device int64 keying the Philox streams, or NULL */
    const long long* text;                  /* [B][4] */
    const float* eps;                       /* [B][D] or NULL (drawn on device) */
    const uint8_t* gru_keep;                /* [4][B][H] keep flags of the decoder's inter-layer Dropout or NULL (drawn) */
    int gru_dropout;                        /* 0: no dropout */
    const long long* force_tokens;          /* [B][4] or NULL: overrides the greedy feedback (test hook) */
    float kl_lambda; float lambda_y;
    unsigned long long seed;
    float* sums;                            /* out [16]: [4] NLL sum, [8] KL sum, the rest 0 */
    float* recon_text;                      /* out [B][4][12] log-probabilities or NULL */
    float* mu; float* logvar;               /* out [B][D] or NULL */
    long long* tokens;                      /* out [B][4] greedy tokens or NULL */
    int defer_unpack; int pack_first;       /* as in mmvae_mm_step_io */
} mmvae_mm_text_step_io;
int mmvae_mmtext_step(mmvae_mmtext_t*, const mmvae_mm_text_step_io*, int training, int do_backward, void* stream);
/* The text half of mmvae_mm_iw_score alone: the eval-mode decoder on the B*K particle rows z [B][K][n_latents] of a plan created with
 * at least B*K rows; writes words [B*K][4][12], which feed mmvae_iw_accumulate as T = 4, V = 12. */
int mmvae_mmtext_iw_score(mmvae_mmtext_t*, void* ws, size_t ws_bytes, const float* z, int B, int K, float* words, void* stream);

/* ---------------------------------------------------------------- dataset-independent ops */
/* ProductOfExperts.forward (multimnist/model.py:355-360) over M stacked experts of n scalars each */
int mmvae_poe_fwd(const float* mu, const float* logvar, int M, int n, float* out_mu, float* out_logvar, void* stream);
int mmvae_poe_bwd(const float* mu, const float* logvar, int M, int n, const float* g_mu, const float* g_logvar,
                  float* d_mu, float* d_logvar, void* stream);
/* MultimodalVAE.reparametrize (multimnist/model.py:33-39), train mode */
int mmvae_reparam_fwd(const float* mu, const float* logvar, const float* eps, int n, float* z, void* stream);
int mmvae_reparam_bwd(const float* logvar, const float* eps, const float* dz, int n, float* d_mu, float* d_logvar, void* stream);
/* KL term of loss_function (multimnist/train.py:85): out[0] += -0.5*sum(1+lv-mu^2-exp(lv)) */
int mmvae_kl_fwd(const float* mu, const float* logvar, int n, float* out_sum, void* stream);
/* every *_bwd below: the gradient is coef * (*gscale) * d(sum)/d(input); gscale (nullable) is a DEVICE scalar -- the upstream
   gradient of the 0-d loss tensor, read by the kernel so that the host never synchronises on it */
int mmvae_kl_bwd(const float* mu, const float* logvar, int n, float coef, const float* gscale, float* d_mu, float* d_logvar, void* stream);
/* F.binary_cross_entropy on probabilities (multimnist/train.py:75): out[0] += sum of terms; bwd = coef * d/dp */
int mmvae_bce_fwd(const float* p, const float* target, long long n, float* out_sum, void* stream);
int mmvae_bce_bwd(const float* p, const float* target, long long n, float coef, const float* gscale, float* d_p, void* stream);
/* F.nll_loss on log-probs [rows][classes] (multimnist/train.py:79) */
int mmvae_nll_fwd(const float* logp, const long long* target, int rows, int classes, float* out_sum, void* stream);
int mmvae_nll_bwd(const long long* target, int rows, int classes, float coef, const float* gscale, float* d_logp, void* stream);
/* Importance-sampled marginal log-likelihood, model-family independent part.  Particle rows are example-major (row b*K + k).
 * particles: z [B][K][D] = mu + exp(logvar/2) * eps and log_ratio [B][K] = log p(z) - log q(z) (standard normal prior,
 *   q = N(mu, exp(logvar)), D <= 128); eps is Philox keyed by (seed, first_row + b, first_particle + k, dimension) only -- a particle
 *   does not depend on the batch or the chunk it is drawn in -- unless eps_or_null ([B][K][D], test hook) is given.
 * state: [B][3][4] floats per (example, target x / y / xy): running max of log w, sum exp(log w - max), sum exp(2 (log w - max)),
 *   sum of the target's log-likelihood; iw_init empties it, every iw_accumulate merges one chunk of K particles into it.
 * accumulate: log p(x|z) = loglik_x [B*K]; log p(y|z) = sum over t < T of words[row][t][targets[b][t]] (words [B*K][T][V],
 *   targets [B][T] int64, clamped to [0, V)); log w = log-likelihood + log_ratio.  log_w_out_or_null: [B][K][3] log w of the call.
 * finalize: out [B][8] = log p^(x), log p^(y), log p^(x,y) (logsumexp - log K_total), ESS x / y / xy ((sum w)^2 / sum w^2),
 *   mean -log p(x|z), mean -log p(y|z) over the K_total particles. */
int mmvae_iw_particles(const float* mu, const float* logvar, int B, int D, int K, long long first_row, long long first_particle,
                       unsigned long long seed, const float* eps_or_null, float* z_out, float* log_ratio_out, void* stream);
int mmvae_iw_init(float* state, int B, void* stream);
int mmvae_iw_accumulate(const float* loglik_x, const float* words, const long long* targets, int T, int V, const float* log_ratio,
                        int B, int K, float* state, float* log_w_out_or_null, void* stream);
int mmvae_iw_finalize(const float* state, int B, long long K_total, float* out, void* stream);
/* counter-based RNG (Philox4x32-10) */
int mmvae_normal(float* out, long long n, unsigned long long seed, const long long* step_counter, unsigned stream_id, void* stream);
int mmvae_keep_mask(uint8_t* out, long long n, float p, unsigned long long seed, const long long* step_counter,
                    unsigned stream_id, void* stream);
/* F.mse_loss of the COCO loss variant (coco/train.py:75): out[0] += sum (a-b)^2 ; bwd: d_a = coef * 2 (a-b) */
int mmvae_mse_fwd(const float* a, const float* b, long long n, float* out_sum, void* stream);
int mmvae_mse_bwd(const float* a, const float* b, long long n, float coef, const float* gscale, float* d_a, void* stream);
/* Input pipeline: the ToTensor() transform of the reference's loaders (multimnist/train.py:113-121; dataset tensors are
 * uint8 (N,50,50), multimnist/datasets.py:180-181) done on the device: dst[i] = src[i] / denom (denom = 255, IEEE division: bit-equal to ToTensor) */
int mmvae_u8_to_f32(const uint8_t* src, long long n, float denom, float* dst, void* stream);
/* ... behind `wait_event` (a hipEvent_t, or NULL): `stream` waits for the event, then converts -- one call of the enqueue thread per batch */
/* Batch gather + ToTensor in one kernel: dst[r][i] = src[idx[r]][i] / denom for `rows` rows of `row_elems` uint8 elements (a multiple of 4).
 * `src` and `idx` may be PINNED HOST memory: the device reads the rows over the host link itself -- no runtime copy call, no
 * staging buffer, no conversion kernel on the compute stream (the loader's device-gather path for small batches). */
int mmvae_gather_rows_u8_f32(const uint8_t* src, const long long* idx, long long rows, long long row_elems, float denom, float* dst, void* stream);
int mmvae_u8_to_f32_after(const uint8_t* src, long long n, float denom, float* dst, void* wait_event, void* stream);
/* One staged batch to the device: up to two asynchronous host-to-device copies (pinned sources; bytes_b may be 0) on `stream`, then
 * `event` (a hipEvent_t) recorded behind them.  One call of the loader's worker thread per batch (coco/train.py:117-128,144-147: the
 * reference's DataLoader + .cuda() per batch): a foreign-function call holds no interpreter lock while the runtime takes its own. */
int mmvae_h2d_stage(void* dst_a, const void* src_a, size_t bytes_a, void* dst_b, const void* src_b, size_t bytes_b, void* event, void* stream);
/* Events for a host-side pipeline next to the step (the loader's "copy done" / "buffers consumed" edges): created WITHOUT the
 * system-scope fence a default event performs when it completes (a write-back of the device caches for the host's benefit: one per
 * step on the compute stream slowed the kernels behind it by tens of microseconds) and without timing.  They order streams of one
 * device and tell the host THAT work finished, not what it wrote -- read results after a stream synchronisation. */
int mmvae_stream_wait_event(void* stream, void* event);   /* device-side: `stream` waits for `event` */
int mmvae_event_create(void** out);
int mmvae_event_destroy(void* event);
int mmvae_event_record(void* event, void* stream);
int mmvae_event_synchronize(void* event);            /* blocks the calling host thread */
/* torch.optim.Adam defaults (multimnist/train.py:129,173) on flat buffers; state = device int64[2] {step, ticket},
 * zero-initialised by the caller; grad_scale multiplies g first (1/world_size after a sum all-reduce). */
/* The three losses of train()'s closure from a step's `sums` block (multimnist/train.py:33-62: the weighted sum each
 * loss_function call ends with): losses[k] = w_bce[k]*sums[k] + w_nll[k]*sums[4+k] + w_kl[k]*sums[8+k].  The weights are HOST
 * arrays of 3 floats (lambda / divisor per pass, 0 for an absent pass); `sums` and `losses` are device pointers. */
int mmvae_step_losses(const float* sums, const float* w_bce, const float* w_nll, const float* w_kl, float* losses, void* stream);
/* Measurement aids (not part of the reference's interface).  mmvae_debug_set: named integer A/B switches of the library
 * (csrc/knobs.h lists them).  mmvae_debug_probe(1): every kernel the library launches through its tagged launcher carries a start
 * and a stop event of its own until mmvae_debug_probe(0); mmvae_debug_probe_read waits for them and writes one line per launch
 * "tag\tkernel\tmicroseconds\talgorithmic FLOPs\n" into buf (returns the number of lines) -- bench.py's in-step roofline. */
/* ONE more HIP stream (non-blocking, default priority) for host code that needs a copy / communication stream next to the
 * step's: a PyTorch host must not take it from torch's pool -- the first torch.cuda.Stream() creates the pool's 32 streams, past
 * the hardware queues the runtime maps streams to (GPU_MAX_HW_QUEUES) every stream of the process is then time-sliced and each
 * step runs ~2x slower (measured 0.67 -> 1.26 ms, tools/loader_probe.py).  Wrap it with torch.cuda.ExternalStream. */
int mmvae_stream_create(void** out);
int mmvae_stream_destroy(void* stream);
/* Batch assembly for the input pipeline (coco/train.py:117-128's DataLoader role): dst[i] = src[idx[i]], rows of row_bytes (a
 * multiple of 16).  `idx` and `dst` are device memory; `src` may be PINNED HOST memory -- the kernel then pulls the rows over the
 * host link itself, and the host never copies a sample (data.DeviceBatcher). */
int mmvae_gather_rows(const void* src, const long long* idx, long long rows, long long row_bytes, void* dst, void* stream);
/* Waits for `stream`, then MMVAE_OK, or MMVAE_ETIMEOUT when the step that wrote `sums` (device, [16]) declared itself void. */
int mmvae_step_status(const float* sums, void* stream);
int mmvae_debug_probe(int on);
int mmvae_debug_probe_read(char* buf, long long cap);
/* torch.optim.Adam (multimnist/train.py:129,173) on flat fp32 buffers.  `state`: 16 zero-initialised device bytes the caller keeps
 * next to the moments -- int64 step count, then two words of the kernel's own (block ticket, skip flag).  The update is dropped
 * (and the step count kept) when the skip flag is set or g[0] carries the void mark (the NaN bit pattern 0x7fc0dead, sign ignored):
 * see mmvae_coco_step_io.optimizer_state.  Any other NaN in the gradient is a value: it goes through the update and shows in the
 * parameters, as with torch.optim.Adam. */
int mmvae_adam_step(float* p, const float* g, float* m, float* v, long long n, long long* state, float lr, float beta1,
                    float beta2, float eps, float grad_scale, void* stream);
/* The same update with the unpack of the packed weight gradients fused in (mmvae_mm_step_io.defer_unpack = 1):
 * g[i] += packed gradient of i (through gmap), the completed g is written back, then Adam.  One pass instead of two. */
int mmvae_adam_step_packed(float* p, float* g, float* m, float* v, long long n, long long* state, float lr, float beta1,
                           float beta2, float eps, float grad_scale, const int* gmap, const float* gpk, const float* gpk_vec,
                           void* stream);
/* ... over `nr` (<= 4) element ranges (offset, length: multiples of 4 elements) of the flat buffers of n elements.  advance = 1: this call
 * completes the optimizer step (the step count advances); 0: an earlier part of it. */
int mmvae_adam_step_packed_ranges(float* p, float* g, float* m, float* v, long long n, const long long* ranges, int nr, int advance,
                                  long long* state, float lr, float beta1, float beta2, float eps, float grad_scale, const int* gmap,
                                  const float* gpk, const float* gpk_vec, void* stream);
/* The (offset, length) runs of the flat buffers that mmvae_mm_step_io.early_adam updates inside the step (image_decoder.*, text_decoder.*):
 * writes up to `cap` pairs to `ranges`, returns their number. */
int mmvae_mm_early_ranges(const mmvae_mm_t*, long long* ranges, int cap);

/* Nearest-word search over an embedding table (coco/glove.py: closest, closest_batch), fp32 throughout, dim = 300 only.
 * table [n_words][300], queries [n_queries][300], both 16-byte aligned device memory.
 * norms: sqnorm[v] = sum_k table[v][k]^2 (run once per table).
 * nearest: index[q] (int64) = the word that minimises sqnorm[v] - 2 q.w_v -- the dot product one fixed fmaf chain per (query, word)
 *   pair on the f32-input MFMA, equal scores resolved to the LOWEST index -- and dist[q] = sqrt(sum_k (q_k - w_k)^2) recomputed
 *   directly for that word.  Bitwise independent of how the queries are batched.  ws: device scratch of
 *   mmvae_nn_words_workspace_bytes(n_queries, n_words) bytes (MMVAE_ENOSPC when ws_bytes is less).
 * dists: dist[q][v] = sqrt(sum_k (q_k - w_k)^2) for every word, n_queries <= 8 (closest(vec, n): the caller takes the n smallest).
 * geometry: query rows per workgroup, words per vocabulary tile, the largest number of vocabulary splits.  The sweep runs on a
 *   grid of (query blocks) x (splits); a call uses S = max(1, min(max_splits, T, 1024 / ceil(n_queries / query_tile))) splits of
 *   the T = ceil(n_words / word_tile) tiles, split s covering the tiles [T s / S, T (s + 1) / S) (integer division) -- a
 *   function of the shape alone.  Tests place their winners against these edges; no result depends on them. */
long long mmvae_nn_words_workspace_bytes(int n_queries, long long n_words);
int mmvae_nn_words_geometry(int* query_tile, int* word_tile, int* max_splits);
int mmvae_nn_words_norms(const float* table, long long n_words, int dim, float* sqnorm, void* stream);
int mmvae_nn_words_nearest(const float* queries, int n_queries, const float* table, const float* sqnorm, long long n_words, int dim,
                           void* ws, long long ws_bytes, long long* index, float* dist, void* stream);
int mmvae_nn_words_dists(const float* queries, int n_queries, const float* table, long long n_words, int dim, float* dist, void* stream);

/* Gaussian-kernel maximum mean discrepancy (coco/model.py:385-402: compute_kernel, compute_mmd), fp32 in and out.
 * x [n_x][dim], y [n_y][dim] row-major device memory, 1 <= dim <= max_dim (256), 1 <= n_x, n_y <= 65536; x == y is allowed.
 *   k(a, b) = exp(-(sum_k (a_k - b_k)^2 / dim) / dim), the squared distance from coordinate differences in a fixed order
 *   MMD     = mean_ij k(x_i, x_j) + mean_ij k(y_i, y_j) - 2 mean_ij k(x_i, y_j), diagonals included
 * mmd: ONE call gives out4 = {mean Kxx, mean Kyy, mean Kxy, MMD} and, where the pointer is not null, dx = dMMD/dx [n_x][dim] and
 *   dy = dMMD/dy [n_y][dim] (with both null the value alone, at three quarters of the pairs).  Two launches: a sweep over the
 *   pairs that writes per-(split, row) float64 partial sums into ws, and a fold in float64 in a fixed order, rounded to fp32
 *   once.  No atomics: the result depends on the shape alone and two calls give identical bits.  ws: device scratch of
 *   mmvae_mmd_workspace_bytes(n_x, n_y, dim) bytes, 8-byte aligned, every byte the fold reads is rewritten by each call
 *   (MMVAE_ENOSPC when ws_bytes is less; workspace_bytes is 0 for sizes out of range).
 * kernel_matrix: k [n_x][n_y] = k(x_i, y_j) with the per-pair arithmetic of mmd.
 * geometry: rows per workgroup, rows of x or y per column tile, max_dim.  The sweep's grid is (row tiles) x (column splits):
 *   the row tiles are the ceil(n_x / row_tile) tiles of x followed by the ceil(n_y / row_tile) tiles of y (R in all); the columns
 *   of class c in {x, y} are its T_c = ceil(n_c / col_tile) tiles, cut into S_c = max(1, min(T_c, 64, 1024 / R)) splits (integer
 *   division), split s covering the tiles [T_c s / S_c, T_c (s + 1) / S_c) -- a function of (n_x, n_y) alone.  Inside a tile the
 *   columns are summed 8 at a time in fp32, everything above that in float64.  Tests place their edges against these numbers;
 *   no result depends on them beyond the last bits of a real-valued sum. */
int mmvae_mmd_geometry(int* row_tile, int* col_tile, int* max_dim);
long long mmvae_mmd_workspace_bytes(int n_x, int n_y, int dim);
int mmvae_mmd(const float* x, int n_x, const float* y, int n_y, int dim, void* ws, long long ws_bytes,
              float* out4, float* dx_or_null, float* dy_or_null, void* stream);
int mmvae_mmd_kernel_matrix(const float* x, int n_x, const float* y, int n_y, int dim, float* k, void* stream);
/* The form a training step takes (x: prior samples, no gradient wanted): out4 as mmvae_mmd, dy = scale * dMMD/dy (NULL: the value
 * alone), dx never formed.  The same grid; the row tiles of x run the value form of the sweep (kernel sums only), so about half of
 * the gradient arithmetic and of the gradient workspace goes.  Per pair, per 8 columns, per split and in the fold the arithmetic and
 * its order are mmvae_mmd's: out4, and dy at scale = 1, are bit for bit what mmvae_mmd writes.  grad_y_only must be 1 (the one form
 * this entry has; anything else is refused).  ws: mmvae_mmd_dy_workspace_bytes(n_x, n_y, dim) bytes, 8-byte aligned. */
long long mmvae_mmd_dy_workspace_bytes(int n_x, int n_y, int dim);
int mmvae_mmd_dy(const float* x, int n_x, const float* y, int n_y, int dim, void* ws, long long ws_bytes, float scale,
                 float* out4, float* dy_or_null, int grad_y_only, void* stream);

/* Incremental sampler for PixelCNN / GatedPixelCNN (coco/model.py:405-585), fp32 storage and accumulation, ONE launch per call.
 * A model is (gated, n_blocks 0..15, data_channels 1 or 3, hid_dims a multiple of 16 up to 128, out_dims 2..256); sides 1..64, any
 * batch >= 1.  Everything else is refused (MMVAE_EINVAL) before anything is launched.
 * params: the model's weights and biases as ONE flat fp32 device vector of param_elems floats, per layer weight (cout, cin, kh, kw)
 *   then bias, in the order
 *     PixelCNN:      conv1, blocks[0], blocks[2], ..., conv2, conv4
 *     GatedPixelCNN: for conv1 and every blocks.blocks[k]: vertical_conv, x_to_h_conv, vertical_gate_conv, horizontal_conv,
 *                    horizontal_gate_conv, horizontal_output; then conv2, conv4
 * pack_weights: params -> packed (packed_elems floats, 16-byte aligned), each layer tap-major [tap][cin / 4][cout][4] with cin and
 *   cout zero-padded to 16, ONLY the taps its mask keeps -- the masks apply whether or not a forward ever zeroed the weights.
 * sample: uniforms (B, C, H, W) fp32; given (B, C, H, W) int32 levels (clamped to 0..out_dims - 1) or null; the first n_given pixels
 *   in raster order take `given`, the others are drawn: the smallest v with u < CDF_v of the softmax over the pixel's out_dims
 *   logits of that channel (logit channel v * C + c), clamped to out_dims - 1.  Writes out_levels (B, C, H, W) int32, out_image =
 *   level / (out_dims - 1) fp32 and, where not null, out_logits (B, out_dims, C, H, W): the logits every pixel was drawn from.
 *   n_given = H * W is a teacher-forced evaluation of `given`.  A sample's results depend on (weights, its uniforms, its given,
 *   n_given) alone -- not on B, not on the tile it lands in; two calls give identical bits.
 *   ws: device scratch of workspace_bytes, 16-byte aligned, needs no initialisation (MMVAE_ENOSPC when ws_bytes is less;
 *   workspace_bytes and the elems queries are 0 for arguments out of range).
 * geometry: samples per workgroup, the largest hid_dims, the largest side. */
int mmvae_pixelcnn_geometry(int* sample_tile, int* max_hid, int* max_side);
long long mmvae_pixelcnn_param_elems(int gated, int n_blocks, int data_channels, int hid_dims, int out_dims);
long long mmvae_pixelcnn_packed_elems(int gated, int n_blocks, int data_channels, int hid_dims, int out_dims);
int mmvae_pixelcnn_pack_weights(int gated, int n_blocks, int data_channels, int hid_dims, int out_dims, const float* params,
                                long long n_params, float* packed, void* stream);
long long mmvae_pixelcnn_workspace_bytes(int gated, int n_blocks, int data_channels, int hid_dims, int out_dims, int batch, int height,
                                         int width);
int mmvae_pixelcnn_sample(int gated, int n_blocks, int data_channels, int hid_dims, int out_dims, const float* packed, void* ws,
                          long long ws_bytes, int batch, int height, int width, const float* uniforms, const int* given_or_null,
                          int n_given, int* out_levels, float* out_image, float* out_logits_or_null, void* stream);

/* Causal tap-list convolution for PixelCNN / GatedPixelCNN training (csrc/causal_conv.h): bf16 operands (round to nearest even),
 * fp32 accumulation, fp32 channels-last activations [batch * height * width][channels].
 * taps: HOST array of n_taps x {r, c, dy, dx}: kernel cell (r, c) of the (cout, cin, kh, kw) fp32 weight is applied at offset
 *   (dy, dx); a shifted position outside its own image contributes nothing.  A cell may appear in one tap at most.
 *   forward:          y[p][co] = bias[co] + sum_t sum_ci x[p + (dy_t, dx_t)][ci] w[co][ci][r_t][c_t]          (bias may be null)
 *   backward_data:    dx[p][ci] = sum_t sum_co g[p - (dy_t, dx_t)][co] w[co][ci][r_t][c_t]
 *   backward_weight:  dw[co][ci][r_t][c_t] = sum_p g[p][co] x[p + (dy_t, dx_t)][ci], cells in no tap exactly 0; db[co] = sum_p
 *                     g[p][co] from the unrounded g; each of dw, db may be null.  Partials per chunk of positions, folded in
 *                     ascending chunk order: no atomics, two calls give identical bits.
 *   ws: device scratch of workspace_bytes (0 for arguments out of range), 16-byte aligned, needs no initialisation; the packed
 *   weights live there for the duration of one call only (MMVAE_ENOSPC when ws_bytes is less).
 * geometry: positions and channels per workgroup tile, positions per weight-gradient chunk, the largest number of taps, the
 *   largest |dy|, |dx| and the largest channel count. */
int mmvae_causal_conv_geometry(int* pos_tile, int* channel_tile, int* wgrad_chunk, int* max_taps, int* max_offset, int* max_channels);
long long mmvae_causal_conv_workspace_bytes(int batch, int height, int width, int cin, int cout, int kh, int kw, int n_taps);
int mmvae_causal_conv_forward(const float* x, const float* weight, const float* bias_or_null, float* y, const int* taps, int n_taps,
                              int batch, int height, int width, int cin, int cout, int kh, int kw, void* ws, long long ws_bytes,
                              void* stream);
int mmvae_causal_conv_backward_data(const float* g, const float* weight, float* dx, const int* taps, int n_taps, int batch, int height,
                                    int width, int cin, int cout, int kh, int kw, void* ws, long long ws_bytes, void* stream);
int mmvae_causal_conv_backward_weight(const float* g, const float* x, float* dw_or_null, float* db_or_null, const int* taps, int n_taps,
                                      int batch, int height, int width, int cin, int cout, int kh, int kw, void* ws, long long ws_bytes,
                                      void* stream);

/* PixelCNN output head fused with its cross entropy (csrc/head_nll.h): the 1 x 1 convolution conv4 (weight (levels * channels, hid),
 * output channel v * channels + c = level v of data channel c) and the per-element negative log-likelihood, without the logits ever
 * existing in global memory.  h fp32 channels-last [batch * height * width][hid]; target (int64 levels), nll, lse and g are
 * (batch, channels, height, width).  bf16 operands (round to nearest even), fp32 accumulation:
 *   l[p,v,c] = bias[vC+c] + sum_k h[p,k] w[vC+c,k];  lse[p,c] = log sum_v exp l[p,v,c];  nll[p,c] = lse[p,c] - l[p,target[p,c],c]
 *   (a target outside 0..levels-1 reads nothing and gives NaN for that element)
 *   d[p,v,c] = g[p,c] (exp(l[p,v,c] - lse[p,c]) - [v == target[p,c]]);  dh[p,k] = sum_{v,c} d w;  dw[vC+c,k] = sum_p d h;
 *   db[vC+c] = sum_p d from the unrounded d.  The backward recomputes the logits from h, the weights and the saved lse.
 *   forward: lse may be null (evaluation).  backward: each of dh, dw, db may be null and is then not computed.
 *   Partial dw / db per chunk of positions, folded in ascending chunk order: no atomics, two calls give identical bits.
 *   ws: device scratch of workspace_bytes (0 for arguments out of range), 16-byte aligned, needs no initialisation.
 * Limits: channels 1 or 3, hid a multiple of 8 up to max_hid, levels 2..max_levels, batch * height * width <= max_positions.
 * geometry: positions per workgroup, levels per tile, positions per dw / db chunk and the three limits. */
int mmvae_head_nll_geometry(int* pos_tile, int* level_tile, int* chunk, int* max_hid, int* max_levels, int* max_positions);
long long mmvae_head_nll_workspace_bytes(int batch, int channels, int height, int width, int hid, int levels);
int mmvae_head_nll_forward(const float* h, const float* weight, const float* bias, const long long* target, float* nll, float* lse_or_null,
                           int batch, int channels, int height, int width, int hid, int levels, void* ws, long long ws_bytes, void* stream);
int mmvae_head_nll_backward(const float* h, const float* weight, const float* bias, const long long* target, const float* lse,
                            const float* g, float* dh_or_null, float* dw_or_null, float* db_or_null, int batch, int channels, int height,
                            int width, int hid, int levels, void* ws, long long ws_bytes, void* stream);

/* 4 x 4, stride 2, pad 1 convolution and its transpose, bias-free, with a fused activation (csrc/conv4s2.h): bf16 operands (round to
 * nearest even), fp32 accumulation, fp32 channels-last activations.  S is the high-resolution side [batch * hs * ws][cs], L the
 * low-resolution side [batch * hs/2 * ws/2][cl]; weight is the module's own fp32 parameter (cl, cs, 4, 4): nn.Conv2d(cs, cl, 4, 2, 1)
 * and nn.ConvTranspose2d(cl, cs, 4, 2, 1) both have it.  A position outside the image contributes nothing.
 *   down:  dst[b,oy,ox,l] = act_out(sum_{s,ky,kx} src[b,2oy-1+ky,2ox-1+kx,s] w[l,s,ky,kx])              src on S, dst on L
 *   up:    dst[b,iy,ix,s] = act_out(sum_{l,ky,kx: iy+1-ky, ix+1-kx even} src[b,(iy+1-ky)/2,(ix+1-kx)/2,l] w[l,s,ky,kx])   src on L, dst on S
 *   wgrad: dw[l,s,ky,kx]  = sum_{b,oy,ox} l_side[b,oy,ox,l] s_side[b,2oy-1+ky,2ox-1+kx,s]
 *   act: 0 none, 1 relu, 2 leaky (pre > 0 ? pre : slope pre), 3 sigmoid (1 / (1 + expf(-pre))).
 *   A gradient operand: with src_y (y_s, y_l) non-null the operand is an upstream gradient g and the pointer the forward's saved
 *   output y at the same positions; the operand used is none: g, relu: y > 0 ? g : 0, leaky: y > 0 ? g : slope g, sigmoid:
 *   (g y) (1 - y), formed in fp32 while loading (act_in / act names the activation).  So the data gradient of down is up on (g, y)
 *   and that of up is down on (g, y), both with act_out = 0.  wgrad: one of y_s, y_l at most.
 *   Partial dw per chunk of L positions, folded in ascending chunk order: no atomics, two calls give identical bits.
 *   ws: device scratch of workspace_bytes (0 for arguments out of range), 16-byte aligned, needs no initialisation; the packed
 *   weights live there for the duration of one call only (MMVAE_ENOSPC when ws_bytes is less).
 * Limits: cs, cl 1..max_channels, hs, ws even in 2..max_side, batch >= 1 (batch * hs * ws <= 2^24).
 * geometry: L positions and output channels per workgroup tile, the least number of L positions per weight-gradient chunk (a
 *   shape with more than max_chunks of them uses larger chunks), max_chunks and the two limits. */
int mmvae_conv4s2_geometry(int* pos_tile, int* channel_tile, int* wgrad_chunk, int* max_chunks, int* max_channels, int* max_side);
long long mmvae_conv4s2_workspace_bytes(int batch, int cs, int cl, int hs, int ws);
int mmvae_conv4s2_down(const float* src, const float* src_y_or_null, const float* weight, float* dst, int act_in, int act_out, float slope,
                       int batch, int cs, int cl, int hs, int ws, void* workspace, long long ws_bytes, void* stream);
int mmvae_conv4s2_up(const float* src, const float* src_y_or_null, const float* weight, float* dst, int act_in, int act_out, float slope,
                     int batch, int cs, int cl, int hs, int ws, void* workspace, long long ws_bytes, void* stream);
int mmvae_conv4s2_wgrad(const float* s_side, const float* l_side, const float* y_s_or_null, const float* y_l_or_null, int act, float slope,
                        float* dw, int batch, int cs, int cl, int hs, int ws, void* workspace, long long ws_bytes, void* stream);

/* One fp32 Linear layer with a fused activation (csrc/infovae_mnist.h): y = act(x W^T + b), x [rows][K], W [N][K] (nn.Linear's
 * layout), b [N], y [rows][N]; act 0 none, 1 relu, 2 leaky(slope).  Exact fp32 products and fp32 accumulation on
 * v_mfma_f32_16x16x4_f32.  No atomics: two calls give identical bits, and a row's forward bits do not depend on the other rows.
 *   fwd:    y = act(x W^T + b)
 *   dgrad:  dx [rows][K] = gp W with gp = g (.) act'(y), formed from the upstream gradient g [rows][N] and the SAVED OUTPUT y while
 *           the operand is loaded (relu: y > 0 ? g : 0; leaky: y > 0 ? g : slope g); y may be NULL when act = 0
 *   wgrad:  dw [N][K] = gp^T x and db [N] = column sums of gp (NULL: not wanted), one launch, one writer per element
 * perm = 1: the layer's 6272-wide side -- exactly one of N, K must be 6272 -- is kept channels-last, [rows][49][128], as conv4s2
 * keeps it: feature c * 49 + p of the weight lives at p * 128 + c of x (K side) or of y, g (N side); dx of a K-side layer is
 * written in that layout too.  The weight and its gradient stay in nn.Linear's order.
 * rows 1..65536, N and K 1..65536, every pointer 16-byte aligned; anything else is refused (MMVAE_EINVAL) before a launch.  fwd and
 * dgrad take device scratch of mmvae_lin_act_workspace_bytes(rows, N, K, which) bytes (which 0: fwd, 1: dgrad; 0 bytes: none needed,
 * the pointer may be NULL); every byte a call reads of it it has written itself. */
long long mmvae_lin_act_workspace_bytes(int rows, int n, int k, int which);
int mmvae_lin_act_fwd(const float* x, const float* w, const float* b, float* y, int rows, int n, int k, int act, float slope, int perm,
                      void* workspace, long long ws_bytes, void* stream);
int mmvae_lin_act_dgrad(const float* g, const float* y_or_null, const float* w, float* dx, int rows, int n, int k, int act, float slope,
                        int perm, void* workspace, long long ws_bytes, void* stream);
int mmvae_lin_act_wgrad(const float* g, const float* y_or_null, const float* x, float* dw, float* db_or_null, int rows, int n, int k,
                        int act, float slope, int perm, void* stream);

/* MNIST InfoVAE (mnist/model.py:238-279, mnist/train_infovae.py:45-76) as one enqueue: zero_grad, forward, loss, backward.
 *   loss = lambda_x * SSE / (B * 784) + lambda_mmd * MMD(true_samples, z)          (the reference: lambda_x = lambda_mmd = 1)
 * A plan of its own, fp32, no packed weights: the 12 parameters are InfoVAE's state_dict in its order (mmvae_mnist_infovae_param_info),
 * flat in `params`; every one of the 12 gradients is written to `grads` by each step with do_backward (no accumulation).  The
 * optimizer is one mmvae_adam_step over the flat buffers, enqueued by the caller behind the step.  n_latents 1..256 (what mmvae_mmd
 * takes), batch 1..65536; anything else: NULL, and mmvae_last_error names the range.
 * The four convolutions are mmvae_conv4s2_* (bf16 operands), the four Linear layers mmvae_lin_act_* (fp32), the MMD term is the
 * y-only sweep (mmvae_mmd_dy) with its fold on a side stream of the plan beside the decoder; weight gradients run on the shared side
 * streams; MMVAE_SERIAL=1 puts everything in order on the caller's stream.  No host synchronisation, no allocation.
 * sums [16]: [0] SSE = sum (recon - x)^2, [MMVAE_SUM_MMD_KXX .. MMVAE_SUM_MMD] = {mean Kxx, mean Kyy, mean Kxy, MMD}, bit for bit what
 * mmvae_mmd returns for (true_samples, z); every other slot 0.  true_samples NULL: drawn by the step's prologue on Philox stream
 * MMVAE_TRUE_SAMPLES_STREAM (the values of mmvae_normal for that stream, seed and step_counter).  do_backward = 0: stops behind the
 * losses (the sweep in its value-only form), `grads` is not touched.  lambda_x = 0: the decoder's backward is skipped, its gradients
 * are exactly 0 and the MMD gradient is the only dz.  lambda_mmd = 0: the value is reported, no gradient is formed.  The model has no
 * BatchNorm, dropout or reparametrisation: `training` changes nothing.  An error inside the step joins the side streams and leaves
 * the parameters untouched. */
typedef struct MnistInfoVaePlan mmvae_mnist_infovae_t;
typedef struct {
    void* ws; size_t ws_bytes;              /* mmvae_mnist_infovae_step_workspace_bytes, 16-byte aligned */
    const long long* step_counter;          /* device int64 keying the Philox stream, or NULL */
    const float* image;                     /* [B][784] fp32 */
    const float* true_samples;              /* [B][D] prior samples or NULL (drawn on the device) */
    float lambda_x;
    float lambda_mmd;
    unsigned long long seed;
    float* sums;                            /* out [16], see above */
    float* recon_image;                     /* out [B][784] or NULL */
    float* z;                               /* out [B][D] or NULL */
} mmvae_mnist_infovae_step_io;
mmvae_mnist_infovae_t* mmvae_mnist_infovae_create(int n_latents, int batch);
void mmvae_mnist_infovae_destroy(mmvae_mnist_infovae_t*);
long long mmvae_mnist_infovae_param_count(const mmvae_mnist_infovae_t*);
int mmvae_mnist_infovae_num_params(const mmvae_mnist_infovae_t*);              /* 12 */
int mmvae_mnist_infovae_param_info(const mmvae_mnist_infovae_t*, int i, char* name, int* ndim, int* shape, long long* offset);
int mmvae_mnist_infovae_bind(mmvae_mnist_infovae_t*, float* params, float* grads);
size_t mmvae_mnist_infovae_step_workspace_bytes(const mmvae_mnist_infovae_t*);
int mmvae_mnist_infovae_step(mmvae_mnist_infovae_t*, const mmvae_mnist_infovae_step_io*, int training, int do_backward, void* stream);

/* Exact t-SNE with a 2-component embedding (mnist/manifold.py: TSNE(n_components=2, perplexity=40, n_iter=300) over the test set's
 * latents), fp32 in and out, float64 sums in a fixed order, no atomics: two calls give identical bits.  3 <= n <= 32768; P is a
 * dense [n][n] fp32 matrix of the caller (4 GiB at the largest n); x [n][dim], 1 <= dim <= max_dim (256); 1 <= perplexity < n - 1.
 * Everything else is refused (MMVAE_EINVAL) before anything is launched, and workspace_bytes is 0.  ws: device scratch of
 * mmvae_tsne_workspace_bytes(n) bytes, 8-byte aligned; every byte a call reads it has written itself (MMVAE_ENOSPC when ws_bytes
 * is less).  All launches go to the caller's stream; no call synchronises.
 * affinities: d_ij = sum_k (x_ik - x_jk)^2 from coordinate differences (16 fmaf chains, coordinate k in chain k % 16 in ascending
 *   order, folded by a fixed tree: the rounding of a 256-term sum stays near that of a pairwise one); beta_i by sklearn's search
 *   (start 1, double / halve until bracketed, then halve the bracket; stops at |H_i - log perplexity| <= 1e-5 or after 100 steps)
 *   on p_{j|i} = exp(-beta_i (d_ij - min_{j != i} d_ij)) / sum, j != i; then P_ij = (p_{j|i} + p_{i|j}) / 2n, floored at 1e-12 off
 *   the diagonal, exactly 0 on it, and symmetric bit for bit.  beta [n]: the beta_i the row was written with.  out2 = {sum P log P,
 *   sum P}, folded in float64.
 * grad: with w_ij = 1 / (1 + |y_i - y_j|^2) and Z = sum_{i != j} w_ij,
 *     grad_i = 4 (exaggeration sum_j P_ij w_ij (y_i - y_j) - sum_j w_ij^2 (y_i - y_j) / Z)              grad [n][2], y [n][2]
 *     KL     = sum P log P - sum P log w + log Z                                                       (P itself, never exaggerated)
 *   out3 = {KL, Z, sum P log P}.  ONE sweep over the pairs: the repulsive sums are divided by Z afterwards.  P MUST BE SYMMETRIC,
 *   as affinities writes it: the sweep reads P_ji where the formula says P_ij, so that a wave reads consecutive addresses.
 * run: n_iter iterations of sklearn's _gradient_descent, all enqueued on the stream: per iteration the sweep and one fold / update
 *   kernel.  Iteration k of the call is iteration first_iter + k of the schedule: exaggeration early_exaggeration and momentum 0.5
 *   while first_iter + k < exaggeration_iters, then 1 and 0.8.  gains + 0.2 where update * grad < 0, else * 0.8, floor 0.01;
 *   update = momentum update - learning_rate gains grad; y += update; no recentring.  y, update, gains [n][2] are in and out, so
 *   a + b iterations in two calls give the bits of a + b in one.  kl_trace [n_iter]: each iteration's KL, before its update.
 * geometry: row_tile (rows per sweep workgroup), col_tile (columns per column tile of the sweep), sym_tile (side of a
 *   symmetrisation tile; workgroup (a, b), a <= b, writes tiles (a, b) and (b, a)), row_threads (threads of an affinity workgroup,
 *   one per row i: thread t takes the columns t, t + row_threads, ...), max_dim.  The sweep's grid is R = ceil(n / row_tile) row
 *   tiles x S column splits, S = max(1, min(T, 64, 2048 / R)) with T = ceil(n / col_tile); split c covers the column tiles
 *   [T c / S, T (c + 1) / S).  Within a tile a wave sums the force terms of 8 columns at a time in fp32, everything above that
 *   and the terms of Z and of the KL in float64.  Tests place their edges against these numbers; no result depends on them
 *   beyond the last bits of a real-valued sum. */
int mmvae_tsne_geometry(int* row_tile, int* col_tile, int* sym_tile, int* row_threads, int* max_dim);
long long mmvae_tsne_workspace_bytes(int n);
int mmvae_tsne_affinities(const float* x, int n, int dim, float perplexity, float* P, float* beta, float* out2, void* workspace,
                          long long ws_bytes, void* stream);
int mmvae_tsne_grad(const float* P, float exaggeration, const float* y, int n, void* workspace, long long ws_bytes, float* grad, float* out3,
                    void* stream);
int mmvae_tsne_run(const float* P, int n, float* y, float* update, float* gains, int first_iter, int n_iter, float learning_rate,
                   float early_exaggeration, int exaggeration_iters, float* kl_trace, void* workspace, long long ws_bytes, void* stream);

/* MultiMNIST canvases made on the device (multimnist/datasets.py; csrc/multimnist_gen.h, csrc/mmgen_core.h): 0 .. 4 MNIST digits per
 * 50 x 50 canvas, each resized as Pillow's 8-bit bilinear resample does it (bit for bit) and added at its place; a canvas whose sum
 * passes 255 anywhere is drawn again.  Integer arithmetic and Philox4x32-10 draws keyed by (seed, global canvas index): canvas
 * first_canvas + i is the same whatever the call that makes it, and two calls give identical bits.  csrc/mmgen_core.h states the
 * resize, every draw and the bounds.
 * digits: device, uint8 [n_digits][28][28], 4-byte aligned; digit_labels: device, int64 [n_digits] (copied into the text as they are);
 * tables: a DEVICE copy of the mmvae_mmgen_table_bytes() bytes that the host function build_tables fills (needs no GPU): per side
 * side_min .. side_max and output index (xmin, tap count, max_taps int32 taps), then the 32-bit side thresholds.
 * geometry: side_min, side_max (the sides the tables hold), max_taps, max_attempts, max_redraws, canvas (50).
 * generate: flags = 1 fixed | 2 no_resize | 4 no_translate | 8 reverse | 16 scramble | 32 no_repeat (the last three need fixed);
 *   0 <= min_digits <= max_digits <= 4.  Outputs, device: images_u8 [n][50][50] and / or images_f32 [n][50][50] = u8 / 255 (IEEE
 *   division; 16-byte aligned), at least one of them; text int64 [n][4], FILL (11) past the digits; optional params int32 [n][4][4] =
 *   (digit index or -1, side, top, left) per slot, attempts int32 [n] (1-based count of the accepted attempt) and fail_count int32
 *   [1].  A canvas that used up max_attempts is REPORTED, not retried for ever: zeros, FILL text, params -1 / 0, attempts 0, and
 *   *fail_count incremented (fail_count is only ever added to: clear it yourself).  The kernel always terminates.
 * render: the same render path from an explicit params table [n][4][4] (device), no draws and no rejection: the sum is clamped to
 *   255 and overflow [n] (required) is 1 where that happened, else 0.  A canvas with a slot outside (index < n_digits, side_min <=
 *   side <= side_max, top, left >= 0, top + side <= 50, left + side <= 50) is not rendered: zeros and overflow = -1.
 * Pointers, flags and counts are checked before anything is launched (MMVAE_EINVAL); n = 0 launches nothing. */
int mmvae_mmgen_geometry(int* side_min, int* side_max, int* max_taps, int* max_attempts, int* max_redraws, int* canvas);
long long mmvae_mmgen_table_bytes(void);
int mmvae_mmgen_build_tables(void* host_buf);
int mmvae_mmgen_generate(const unsigned char* digits, const long long* digit_labels, int n_digits, const void* tables, int flags,
                         int min_digits, int max_digits, unsigned long long seed, unsigned long long first_canvas, int n,
                         unsigned char* images_u8_or_null, float* images_f32_or_null, long long* text, int* params_or_null,
                         int* attempts_or_null, int* fail_count_or_null, void* stream);
int mmvae_mmgen_render(const unsigned char* digits, int n_digits, const void* tables, const int* params, int n,
                       unsigned char* images_u8_or_null, float* images_f32_or_null, int* overflow, void* stream);

/* Scale(S) + CenterCrop(S) + ToTensor of a ragged batch of decoded RGB images (celeba/train.py:102-104, coco/train.py:107-112;
 * csrc/imgprep.h, csrc/imgprep_core.h): torchvision's Scale / CenterCrop of that era over Pillow's 8-bit BILINEAR resample, bit for
 * bit, in integer arithmetic.  csrc/imgprep_core.h states the scaled size, the coefficients (2^22 fixed point, float64 without fused
 * multiply-add), the crop offsets and the limits.  One workgroup per image, no atomics: two calls give identical bits and an
 * image's result does not depend on the batch it is in.
 * geometry: the input sides the kernel takes (1 .. max_side), the output sides (1 .. max_out), and 22.
 * layout (host): for one image the scaled size (ow, oh) and the crop offsets (x1, y1).
 * coeffs (host, needs no GPU): for the axis n_in -> n_out and the output indices first .. first + count - 1 the first tap, the tap
 *   count and the int32 coefficients, `stride` per index, zeros past the count; MMVAE_EINVAL when an index has more taps than stride.
 *   The SAME functions as the kernel's, compiled for the host: what a test checks here is what the device computes.
 * scale_crop: pixels: device, the images back to back or not, image i = 3 heights[i] widths[i] bytes (HWC) from byte offsets[i];
 *   pixels_bytes: the bytes of `pixels` that may be read; offsets int64 [n], heights, widths int32 [n], status int32 [n]: device.
 *   Outputs, device, planar: out_u8 [n][3][S][S] and / or out_f32 [n][3][S][S] = u8 / 255 (IEEE division), at least one of them.
 *   The kernel itself refuses an image whose descriptor is unusable -- a side outside 1 .. max_side, offsets[i] < 0, or offsets[i] +
 *   3 h w > pixels_bytes: nothing of it is read, its outputs are zeros and status[i] = -1; otherwise status[i] = 0.  Neighbours are
 *   unaffected.  No byte outside [pixels, pixels + pixels_bytes) is read.
 * Pointers, S and counts are checked before anything is launched (MMVAE_EINVAL); n = 0 launches nothing. */
int mmvae_imgprep_geometry(int* max_side, int* max_out, int* precision_bits);
int mmvae_imgprep_layout(int h, int w, int S, int* ow, int* oh, int* x1, int* y1);
int mmvae_imgprep_coeffs(int n_in, int n_out, int first, int count, int stride, int* xmin, int* taps, int* coefs);
int mmvae_imgprep_scale_crop(const unsigned char* pixels, long long pixels_bytes, const long long* offsets, const int* heights,
                             const int* widths, int n, int S, unsigned char* out_u8_or_null, float* out_f32_or_null, int* status,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif
