// extern "C" boundary of libmmvae_hip.so (see include/mmvae_hip.h).
#include "../../include/mmvae_hip.h"
#include "multimnist.h"
#include "mmtext.h"
#include "mnist.h"
#include "mnist_plan.h"
#include "mnist_strip.h"
#include "celeba.h"
#include "coco.h"
#include "plan_base.h"
#include "iw.h"
#include "nn_words.h"
#include "mmd.h"
#include "tsne.h"
#include "pixelcnn.h"
#include "causal_conv.h"
#include "head_nll.h"
#include "conv4s2.h"
#include "infovae_mnist.h"
#include "multimnist_gen.h"
#include "imgprep.h"
#include <cstring>
#include <exception>

const char* mmvae_error_string();

// Runs `f` and maps an exception that escapes it to mmvae_set_error + MMVAE_ESTATE.
template <class F>
static int guarded(F&& f) {
    try {
        return f();
    } catch (const std::exception& e) {
        mmvae_set_error("internal exception: %s", e.what());
        return MMVAE_ESTATE;
    } catch (...) {
        mmvae_set_error("internal exception");
        return MMVAE_ESTATE;
    }
}

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }


// ---- generic plan queries / bind / pack: every model family gets them from MMVAE_PLAN_API over its PlanBase
static long long pb_bn_floats(const PlanBase* b) { return b->bn_list.empty() ? 0 : b->bn_list.back().stat_off + 2 * b->bn_list.back().C; }
static int pb_param_info(const PlanBase* b, int i, char* name, int* ndim, int* shape, long long* offset) {
    const auto& v = b->params;
    MMVAE_REQUIRE(i >= 0 && i < (int)v.size(), "param index %d out of range", i);
    strncpy(name, v[i].name.c_str(), 127); name[127] = 0;
    *ndim = v[i].ndim;
    for (int k = 0; k < 4; ++k) shape[k] = k < v[i].ndim ? v[i].shape[k] : 1;
    *offset = v[i].offset;
    return MMVAE_OK;
}
static int pb_bn_info(const PlanBase* b, int i, char* prefix, int* channels, long long* offset) {
    MMVAE_REQUIRE(i >= 0 && i < (int)b->bn_list.size(), "bn index %d out of range", i);
    strncpy(prefix, b->bn_names[i].c_str(), 127); prefix[127] = 0;
    *channels = b->bn_list[i].C; *offset = b->bn_list[i].stat_off;
    return MMVAE_OK;
}
static int pb_bind(PlanBase* P, float* params, float* grads, float* bn_stats, long long* nbt, void* packed, float* packed_vec,
                   float* gpk, float* gpk_vec, void* desc_dev, void* gdesc_dev) {
    MMVAE_REQUIRE(P && params && grads && bn_stats && nbt && packed && packed_vec && gpk && gpk_vec && desc_dev && gdesc_dev,
                  "bind: null buffer");
    ModelBuffers& b = P->buf;
    b.params = params; b.grads = grads; b.bn_stats = bn_stats; b.bn_nbt = nbt; b.packed = (bf16*)packed; b.packed_vec = packed_vec;
    b.gpk = gpk; b.gpk_vec = gpk_vec; b.desc_dev = (PackDesc*)desc_dev; b.gdesc_dev = (PackDesc*)gdesc_dev;
    P->bound = true;
    return MMVAE_OK;
}
static int pb_pack(PlanBase* P, hipStream_t s) {
    MMVAE_TRY(check_bound(P));
    if (P->no_pack) return MMVAE_OK;
    return launch_pack(P->buf.desc_dev, P->pk.d.data(), (int)P->pk.d.size(), P->buf.params, P->buf.packed, P->buf.packed_vec, s);
}
static int pb_grad_map(PlanBase* P, int* map, hipStream_t s) {
    MMVAE_TRY(check_bound(P));
    MMVAE_REQUIRE(map != nullptr, "grad_map: null argument");
    return launch_unpack_map(P->buf.gdesc_dev, P->gk.d.data(), (int)P->gk.d.size(), P->nparams, P->gk.mat_elems, map, s);
}
// The weight pack (pack_block) run over the GRADIENT descriptor table: `src` (flat, parameter layout) lands where the packed gradient
// of each element lives -- bf16 [gpk_elems] for the matrices, fp32 [gpk_vec_elems] for the fp32 packs.  The inverse of grad_map,
// derived by other code: what the tests compare the map with.
static int pb_debug_pack_as_grads(PlanBase* P, const float* src, void* out_bf16, float* out_vec, hipStream_t s) {
    MMVAE_TRY(check_bound(P));
    MMVAE_REQUIRE(src && out_bf16 && out_vec, "debug_pack_as_grads: null argument");
    MMVAE_REQUIRE(!P->gk.d.empty(), "debug_pack_as_grads: the plan keeps no packed gradients");
    return launch_pack(P->buf.gdesc_dev, P->gk.d.data(), (int)P->gk.d.size(), src, (bf16*)out_bf16, out_vec, s);
}
#define MMVAE_PLAN_API(pfx, T, BASE)                                                                                      \
    long long mmvae_##pfx##_param_count(const T* p) { return BASE(p)->nparams; }                                          \
    int mmvae_##pfx##_num_params(const T* p) { return (int)BASE(p)->params.size(); }                                      \
    int mmvae_##pfx##_param_info(const T* p, int i, char* name, int* ndim, int* shape, long long* offset) {               \
        return pb_param_info(BASE(p), i, name, ndim, shape, offset);                                                      \
    }                                                                                                                     \
    long long mmvae_##pfx##_bn_floats(const T* p) { return pb_bn_floats(BASE(p)); }                                       \
    int mmvae_##pfx##_num_bn(const T* p) { return (int)BASE(p)->bn_list.size(); }                                         \
    int mmvae_##pfx##_bn_info(const T* p, int i, char* prefix, int* channels, long long* offset) {                        \
        return pb_bn_info(BASE(p), i, prefix, channels, offset);                                                          \
    }                                                                                                                     \
    long long mmvae_##pfx##_packed_elems(const T* p) { return BASE(p)->pk.mat_elems; }                                    \
    long long mmvae_##pfx##_packed_vec_elems(const T* p) { return BASE(p)->pk.vec_elems > 0 ? BASE(p)->pk.vec_elems : 64; } \
    long long mmvae_##pfx##_gpk_elems(const T* p) { return BASE(p)->gk.mat_elems; }                                       \
    long long mmvae_##pfx##_gpk_vec_elems(const T* p) { return BASE(p)->gk.vec_elems > 0 ? BASE(p)->gk.vec_elems : 64; }  \
    size_t mmvae_##pfx##_desc_bytes(const T* p, int which) {                                                              \
        return sizeof(PackDesc) * (which == 0 ? BASE(p)->pk.d.size() : BASE(p)->gk.d.size());                             \
    }                                                                                                                     \
    int mmvae_##pfx##_desc_copy(const T* p, int which, void* host_out) {                                                  \
        memcpy(host_out, which == 0 ? BASE(p)->pk.d.data() : BASE(p)->gk.d.data(), mmvae_##pfx##_desc_bytes(p, which));   \
        return MMVAE_OK;                                                                                                  \
    }                                                                                                                     \
    size_t mmvae_##pfx##_workspace_bytes(const T* p) { return BASE(p)->ws_bytes; }                                        \
    size_t mmvae_##pfx##_module_workspace_bytes(const T* p) {                                                             \
        return BASE(p)->ws_bytes_module ? BASE(p)->ws_bytes_module : BASE(p)->ws_bytes;                                   \
    }                                                                                                                     \
    int mmvae_##pfx##_bind(T* p, float* params, float* grads, float* bn_stats, long long* nbt, void* packed,              \
                           float* packed_vec, float* gpk, float* gpk_vec, void* desc_dev, void* gdesc_dev) {              \
        return guarded([&] {                                                                                              \
            return pb_bind(BASE(p), params, grads, bn_stats, nbt, packed, packed_vec, gpk, gpk_vec, desc_dev, gdesc_dev); \
        });                                                                                                               \
    }                                                                                                                     \
    int mmvae_##pfx##_pack_weights(T* p, void* stream) {                                                                  \
        return guarded([&] { return pb_pack(BASE(p), S(stream)); });                                                      \
    }                                                                                                                     \
    int mmvae_##pfx##_grad_map(T* p, int* map, void* stream) {                                                            \
        return guarded([&] { return pb_grad_map(BASE(p), map, S(stream)); });                                             \
    }                                                                                                                     \
    int mmvae_##pfx##_debug_pack_as_grads(T* p, const float* src, void* out_bf16, float* out_vec, void* stream) {         \
        return guarded([&] { return pb_debug_pack_as_grads(BASE(p), src, out_bf16, out_vec, S(stream)); });               \
    }
static inline PlanBase* mm_b(const mmvae_mm_t* p) { return mm_base(const_cast<mmvae_mm_t*>(p)); }
static inline PlanBase* mmtext_b(const mmvae_mmtext_t* p) { return mmtext_base(const_cast<mmvae_mmtext_t*>(p)); }
static inline PlanBase* mnist_b(const mmvae_mnist_t* p) { return mnist_base(const_cast<mmvae_mnist_t*>(p)); }
static inline PlanBase* celeba_b(const mmvae_celeba_t* p) { return celeba_base(const_cast<mmvae_celeba_t*>(p)); }
static inline PlanBase* coco_b(const mmvae_coco_t* p) { return coco_base(const_cast<mmvae_coco_t*>(p)); }

extern "C" {

const char* mmvae_last_error(void) { return mmvae_error_string(); }
const char* mmvae_version(void) { return "mmvae-hip 0.1 (gfx950)"; }

int mmvae_init(int device) {
    return guarded([&]() -> int {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n == 0) { mmvae_set_error("no HIP device visible"); return MMVAE_EHIP; }
        MMVAE_REQUIRE(device >= 0 && device < n, "device %d out of range (%d visible)", device, n);
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess) { mmvae_set_error("hipGetDeviceProperties failed"); return MMVAE_EHIP; }
        MMVAE_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
        if (hipSetDevice(device) != hipSuccess) { mmvae_set_error("hipSetDevice failed"); return MMVAE_EHIP; }
        return MMVAE_OK;
    });
}

mmvae_mm_t* mmvae_mm_create(int n_latents, int batch) {
    try { return mm_create(n_latents, batch); } catch (...) { mmvae_set_error("mm_create failed"); return nullptr; }
}
void mmvae_mm_destroy(mmvae_mm_t* p) { mm_destroy(p); }
MMVAE_PLAN_API(mm, mmvae_mm_t, mm_b)
int mmvae_mm_wait_early_grads(mmvae_mm_t* p, void* stream) {
    return guarded([&] { return mm_wait_early_grads(p, S(stream)); });
}
int mmvae_mm_step(mmvae_mm_t* p, const mmvae_mm_step_io* io, int training, int do_backward, void* stream) {
    return guarded([&]() -> int {
        MMVAE_REQUIRE(p && io, "mmvae_mm_step: null argument");
        return mm_step_fwd_bwd(p, *io, training, do_backward, S(stream));
    });
}
int mmvae_mm_image_encoder_fwd(mmvae_mm_t* p, void* ws, size_t wsb, const float* image, const uint8_t* m1, const uint8_t* m2,
                               int training, float* out, void* stream) {
    return guarded([&] { return mm_image_encoder_fwd(p, ws, wsb, image, m1, m2, training, out, S(stream)); });
}
int mmvae_mm_image_encoder_bwd(mmvae_mm_t* p, void* ws, size_t wsb, const float* d_out, const uint8_t* m1, const uint8_t* m2, void* stream) {
    return guarded([&] { return mm_image_encoder_bwd(p, ws, wsb, d_out, m1, m2, S(stream)); });
}
int mmvae_mm_image_decoder_fwd(mmvae_mm_t* p, void* ws, size_t wsb, const float* z, int training, float* recon, void* stream) {
    return guarded([&] { return mm_image_decoder_fwd(p, ws, wsb, z, training, recon, S(stream)); });
}
int mmvae_mm_image_decoder_bwd(mmvae_mm_t* p, void* ws, size_t wsb, const float* d_recon, const float* recon, float* dz, void* stream) {
    return guarded([&] { return mm_image_decoder_bwd(p, ws, wsb, d_recon, recon, dz, S(stream)); });
}
int mmvae_mm_text_encoder_fwd(mmvae_mm_t* p, void* ws, size_t wsb, const long long* text, float* out, void* stream) {
    return guarded([&] { return mm_text_encoder_fwd(p, ws, wsb, text, out, S(stream)); });
}
int mmvae_mm_text_encoder_bwd(mmvae_mm_t* p, void* ws, size_t wsb, const long long* text, const float* d_out, void* stream) {
    return guarded([&] { return mm_text_encoder_bwd(p, ws, wsb, text, d_out, S(stream)); });
}
int mmvae_mm_text_decoder_fwd(mmvae_mm_t* p, void* ws, size_t wsb, const float* z, int training, const uint8_t* keep,
                              const long long* force_tokens, float* words, long long* tokens, void* stream) {
    return guarded([&] { return mm_text_decoder_fwd(p, ws, wsb, z, training, keep, force_tokens, words, tokens, S(stream)); });
}
int mmvae_mm_text_decoder_bwd(mmvae_mm_t* p, void* ws, size_t wsb, const float* z, const uint8_t* keep, const long long* force_tokens,
                              const float* words, const long long* tokens, const float* d_words, float* dz, void* stream) {
    return guarded([&] { return mm_text_decoder_bwd(p, ws, wsb, z, keep, force_tokens, words, tokens, d_words, dz, S(stream)); });
}
size_t mmvae_mm_iw_workspace_bytes(const mmvae_mm_t* p) { return mm_b(p)->ws_bytes_module; }
int mmvae_mm_iw_score(mmvae_mm_t* p, void* ws, size_t wsb, const float* z, const float* image, int B, int K, float* loglik_x,
                      float* words, void* stream) {
    return guarded([&] { return mm_iw_score(p, ws, wsb, z, image, B, K, loglik_x, words, S(stream)); });
}
int mmvae_mm_image_step(mmvae_mm_t* p, const mmvae_image_step_io* io, int training, int do_backward, void* stream) {
    return guarded([&]() -> int {
        MMVAE_REQUIRE(p && io, "mmvae_mm_image_step: null argument");
        return mm_image_step(p, *io, training, do_backward, S(stream));
    });
}
size_t mmvae_mm_image_step_workspace_bytes(const mmvae_mm_t* p) { return p ? mm_image_step_workspace_bytes(p) : 0; }
int mmvae_mm_iw_score_image(mmvae_mm_t* p, void* ws, size_t wsb, const float* z, const float* image, int B, int K, float* loglik_x, void* st) {
    return guarded([&] { return mm_iw_score_image(p, ws, wsb, z, image, B, K, loglik_x, S(st)); });
}
int mmvae_mm_bench_layer(mmvae_mm_t* p, void* ws, size_t wsb, const char* layer, int iters, void* stream) {
    return guarded([&] { return mm_bench_layer(p, ws, wsb, layer, iters, S(stream)); });
}
double mmvae_mm_layer_flops(const mmvae_mm_t* p, const char* layer) { return mm_layer_flops(p, layer); }
double mmvae_mm_layer_algo_flops(const mmvae_mm_t* p, const char* layer) { return mm_layer_algo_flops(p, layer); }
double mmvae_mm_layer_algo_bytes(const mmvae_mm_t* p, const char* layer) { return mm_layer_algo_bytes(p, layer); }
long long mmvae_mm_debug_offset(mmvae_mm_t* p, const char* name) { return mm_debug_offset(p, name); }
int mmvae_mm_debug_pack_stage(mmvae_mm_t* p, int stage, int* blocks, void* stream) {
    MMVAE_REQUIRE(p && stage >= -1 && stage <= 2, "debug_pack_stage: null plan or stage %d", stage);
    return mm_debug_pack_stage(p, stage, blocks, (hipStream_t)stream);
}

// ---- MultiMNIST text-only VAE baseline (multimnist/model.py:123-147, multimnist/train_textonly.py)
mmvae_mmtext_t* mmvae_mmtext_create(int n_latents, int n_hiddens, int batch) {
    try { return mmtext_create(n_latents, n_hiddens, batch); } catch (...) { mmvae_set_error("mmtext_create failed"); return nullptr; }
}
void mmvae_mmtext_destroy(mmvae_mmtext_t* p) { mmtext_destroy(p); }
int mmvae_mmtext_hidden(const mmvae_mmtext_t* p) { return mmtext_hidden(p); }
MMVAE_PLAN_API(mmtext, mmvae_mmtext_t, mmtext_b)
int mmvae_mmtext_step(mmvae_mmtext_t* p, const mmvae_mm_text_step_io* io, int training, int do_backward, void* stream) {
    return guarded([&]() -> int {
        MMVAE_REQUIRE(p && io, "mmvae_mmtext_step: null argument");
        return mmtext_step(p, *io, training, do_backward, S(stream));
    });
}
int mmvae_mmtext_encoder_fwd(mmvae_mmtext_t* p, void* ws, size_t wsb, const long long* text, float* out, void* stream) {
    return guarded([&] { return mmtext_encoder_fwd(p, ws, wsb, text, out, S(stream)); });
}
int mmvae_mmtext_encoder_bwd(mmvae_mmtext_t* p, void* ws, size_t wsb, const long long* text, const float* d_out, void* stream) {
    return guarded([&] { return mmtext_encoder_bwd(p, ws, wsb, text, d_out, S(stream)); });
}
int mmvae_mmtext_decoder_fwd(mmvae_mmtext_t* p, void* ws, size_t wsb, const float* z, int training, const uint8_t* keep,
                             const long long* force_tokens, float* words, long long* tokens, void* stream) {
    return guarded([&] { return mmtext_decoder_fwd(p, ws, wsb, z, training, keep, force_tokens, words, tokens, S(stream)); });
}
int mmvae_mmtext_decoder_bwd(mmvae_mmtext_t* p, void* ws, size_t wsb, const float* z, const uint8_t* keep, const long long* force_tokens,
                             const float* words, const long long* tokens, const float* d_words, float* dz, void* stream) {
    return guarded([&] { return mmtext_decoder_bwd(p, ws, wsb, z, keep, force_tokens, words, tokens, d_words, dz, S(stream)); });
}
int mmvae_mmtext_iw_score(mmvae_mmtext_t* p, void* ws, size_t wsb, const float* z, int B, int K, float* words, void* stream) {
    return guarded([&] { return mmtext_iw_score(p, ws, wsb, z, B, K, words, S(stream)); });
}

// ---- MNIST (mnist/model.py, mnist/train.py)
mmvae_mnist_t* mmvae_mnist_create(int n_latents, int batch) {
    try { return mnist_create(n_latents, batch); } catch (...) { mmvae_set_error("mnist_create failed"); return nullptr; }
}
mmvae_mnist_t* mmvae_mnist_create_p(int n_latents, int batch, int precision) {
    try { return mnist_create(n_latents, batch, precision); } catch (...) { mmvae_set_error("mnist_create failed"); return nullptr; }
}
int mmvae_mnist_precision(const mmvae_mnist_t* p) { return mnist_is_f32(p) ? 0 : 1; }
void mmvae_mnist_destroy(mmvae_mnist_t* p) { mnist_destroy(p); }
MMVAE_PLAN_API(mnist, mmvae_mnist_t, mnist_b)
int mmvae_mnist_step(mmvae_mnist_t* p, const mmvae_mnist_step_io* io, int training, int do_backward, void* stream) {
    return guarded([&]() -> int {
        MMVAE_REQUIRE(p && io, "mmvae_mnist_step: null argument");
        return mnist_step(p, *io, training, do_backward, S(stream));
    });
}

int mmvae_mnist_image_encoder_fwd(mmvae_mnist_t* p, void* ws, size_t wsb, const float* in, int training, float* out, void* st) {
    return guarded([&] { return mnist_image_encoder_fwd(p, ws, wsb, in, training, out, S(st)); });
}
int mmvae_mnist_image_decoder_fwd(mmvae_mnist_t* p, void* ws, size_t wsb, const float* in, int training, float* out, void* st) {
    return guarded([&] { return mnist_image_decoder_fwd(p, ws, wsb, in, training, out, S(st)); });
}
int mmvae_mnist_text_encoder_fwd(mmvae_mnist_t* p, void* ws, size_t wsb, const long long* in, int training, float* out, void* st) {
    return guarded([&] { return mnist_text_encoder_fwd(p, ws, wsb, in, training, out, S(st)); });
}
int mmvae_mnist_text_decoder_fwd(mmvae_mnist_t* p, void* ws, size_t wsb, const float* in, int training, float* out, void* st) {
    return guarded([&] { return mnist_text_decoder_fwd(p, ws, wsb, in, training, out, S(st)); });
}
int mmvae_mnist_image_encoder_bwd(mmvae_mnist_t* p, void* ws, size_t wsb, const float* d_out, void* st) {
    return guarded([&] { return mnist_image_encoder_bwd(p, ws, wsb, d_out, S(st)); });
}
int mmvae_mnist_image_decoder_bwd(mmvae_mnist_t* p, void* ws, size_t wsb, const float* d_recon, const float* recon, float* dz, void* st) {
    return guarded([&] { return mnist_image_decoder_bwd(p, ws, wsb, d_recon, recon, dz, S(st)); });
}
int mmvae_mnist_text_encoder_bwd(mmvae_mnist_t* p, void* ws, size_t wsb, const long long* label, const float* d_out, void* st) {
    return guarded([&] { return mnist_text_encoder_bwd(p, ws, wsb, label, d_out, S(st)); });
}
int mmvae_mnist_text_decoder_bwd(mmvae_mnist_t* p, void* ws, size_t wsb, const float* d_logp, const float* logp, float* dz, void* st) {
    return guarded([&] { return mnist_text_decoder_bwd(p, ws, wsb, d_logp, logp, dz, S(st)); });
}
int mmvae_mnist_iw_score(mmvae_mnist_t* p, const float* z, const float* image, int B, int K, float* loglik_x, float* words, void* st) {
    return guarded([&] { return mnist_iw_score(p, z, image, B, K, loglik_x, words, S(st)); });
}
int mmvae_mnist_image_step(mmvae_mnist_t* p, const mmvae_image_step_io* io, int training, int do_backward, void* stream) {
    return guarded([&]() -> int {
        MMVAE_REQUIRE(p && io, "mmvae_mnist_image_step: null argument");
        return mnist_image_step(p, *io, training, do_backward, S(stream));
    });
}
int mmvae_mnist_strip_max_rows(void) { return MNIST_STRIP_MAX_ROWS; }
int mmvae_mnist_strip_route(int rows) { return mnist_strip_route(rows); }
int mmvae_mnist_lin_bn_act_fwd(int route, const float* x, int ldx, const float* w, const float* bias, const float* gamma, const float* beta,
                               float* running_mean, float* running_var, long long* nbt, int rows, int N, int K, int training, float* r, float* a,
                               float* mean_rstd, void* st) {
    return guarded([&] {
        StripFwdArgs f{};
        f.x = x; f.ldx = ldx; f.w = w; f.bias = bias; f.gamma = gamma; f.beta = beta; f.running_mean = running_mean; f.running_var = running_var;
        f.nbt = nbt; f.rows = rows; f.N = N; f.K = K; f.training = training; f.updates = 1; f.r = r; f.a = a; f.mr = reinterpret_cast<float2*>(mean_rstd);
        return mnist_lin_bn_act_fwd(route, f, S(st));
    });
}
int mmvae_mnist_lin_dgrad_bn_bwd(int route, const float* dy, int Nn, const float* w_next, const float* r, const float* mean_rstd, const float* gamma,
                                 const float* beta, int rows, int N, float* d_r, float* dgamma, float* dbeta, void* st) {
    return guarded([&] {
        StripBwdArgs b{};
        b.dy = dy; b.Nn = Nn; b.w_next = w_next; b.r = r; b.mr = reinterpret_cast<const float2*>(mean_rstd); b.gamma = gamma; b.beta = beta;
        b.rows = rows; b.N = N; b.d_r = d_r; b.dgamma = dgamma; b.dbeta = dbeta;
        return mnist_lin_dgrad_bn_bwd(route, b, S(st));
    });
}
size_t mmvae_mnist_image_step_workspace_bytes(const mmvae_mnist_t* p) { return p ? mnist_image_step_workspace_bytes(p) : 0; }
int mmvae_mnist_iw_score_image(mmvae_mnist_t* p, void*, size_t, const float* z, const float* image, int B, int K, float* loglik_x, void* st) {
    return guarded([&] { return mnist_iw_score_image(p, z, image, B, K, loglik_x, S(st)); });
}

// ---- CelebA (celeba/model.py, celeba/train.py)
mmvae_celeba_t* mmvae_celeba_create(int n_latents, int batch) {
    try { return celeba_create(n_latents, batch); } catch (...) { mmvae_set_error("celeba_create failed"); return nullptr; }
}
void mmvae_celeba_destroy(mmvae_celeba_t* p) { celeba_destroy(p); }
MMVAE_PLAN_API(celeba, mmvae_celeba_t, celeba_b)
int mmvae_celeba_step(mmvae_celeba_t* p, const mmvae_celeba_step_io* io, int training, int do_backward, void* stream) {
    return guarded([&]() -> int {
        MMVAE_REQUIRE(p && io, "mmvae_celeba_step: null argument");
        return celeba_step(p, *io, training, do_backward, S(stream));
    });
}
int mmvae_celeba_bench_layer(mmvae_celeba_t* p, void* ws, size_t wsb, const char* layer, int iters, void* stream) {
    return guarded([&] { return celeba_bench_layer(p, ws, wsb, layer, iters, S(stream)); });
}
long long mmvae_celeba_debug_offset(mmvae_celeba_t* p, const char* name) { return celeba_debug_offset(p, name); }
int mmvae_celeba_image_step(mmvae_celeba_t* p, const mmvae_image_step_io* io, int training, int do_backward, void* stream) {
    return guarded([&]() -> int {
        MMVAE_REQUIRE(p && io, "mmvae_celeba_image_step: null argument");
        return celeba_image_step(p, *io, training, do_backward, S(stream));
    });
}
size_t mmvae_celeba_image_step_workspace_bytes(const mmvae_celeba_t* p) { return p ? celeba_image_step_workspace_bytes(p) : 0; }
int mmvae_celeba_iw_score_image(mmvae_celeba_t* p, void* ws, size_t wsb, const float* z, const float* image, int B, int K, float* loglik_x, void* st) {
    return guarded([&] { return celeba_iw_score_image(p, ws, wsb, z, image, B, K, loglik_x, S(st)); });
}
int mmvae_celeba_image_encoder_fwd(mmvae_celeba_t* p, void* ws, size_t wsb, const float* image, const uint8_t* mask, int training, float* out, void* st) {
    return guarded([&] { return celeba_image_encoder_fwd(p, ws, wsb, image, mask, training, out, S(st)); });
}
int mmvae_celeba_image_encoder_bwd(mmvae_celeba_t* p, void* ws, size_t wsb, const float* d_out, const uint8_t* mask, void* st) {
    return guarded([&] { return celeba_image_encoder_bwd(p, ws, wsb, d_out, mask, S(st)); });
}
int mmvae_celeba_image_decoder_fwd(mmvae_celeba_t* p, void* ws, size_t wsb, const float* z, int training, float* recon, void* st) {
    return guarded([&] { return celeba_image_decoder_fwd(p, ws, wsb, z, training, recon, S(st)); });
}
int mmvae_celeba_image_decoder_bwd(mmvae_celeba_t* p, void* ws, size_t wsb, const float* d_recon, const float* recon, float* dz, void* st) {
    return guarded([&] { return celeba_image_decoder_bwd(p, ws, wsb, d_recon, recon, dz, S(st)); });
}
int mmvae_celeba_attrs_encoder_fwd(mmvae_celeba_t* p, void* ws, size_t wsb, const float* attrs, int training, float* out, void* st) {
    return guarded([&] { return celeba_attrs_encoder_fwd(p, ws, wsb, attrs, training, out, S(st)); });
}
int mmvae_celeba_attrs_encoder_bwd(mmvae_celeba_t* p, void* ws, size_t wsb, const float* d_out, void* st) {
    return guarded([&] { return celeba_attrs_encoder_bwd(p, ws, wsb, d_out, S(st)); });
}
int mmvae_celeba_attrs_decoder_fwd(mmvae_celeba_t* p, void* ws, size_t wsb, const float* z, int training, float* recon, void* st) {
    return guarded([&] { return celeba_attrs_decoder_fwd(p, ws, wsb, z, training, recon, S(st)); });
}
int mmvae_celeba_attrs_decoder_bwd(mmvae_celeba_t* p, void* ws, size_t wsb, const float* d_recon, const float* recon, float* dz, void* st) {
    return guarded([&] { return celeba_attrs_decoder_bwd(p, ws, wsb, d_recon, recon, dz, S(st)); });
}
size_t mmvae_celeba_iw_workspace_bytes(const mmvae_celeba_t* p) { return celeba_iw_workspace_bytes(p); }
int mmvae_celeba_iw_score(mmvae_celeba_t* p, void* ws, size_t wsb, const float* z, const float* image, int B, int K, float* loglik_x,
                          float* words, void* st) {
    return guarded([&] { return celeba_iw_score(p, ws, wsb, z, image, B, K, loglik_x, words, S(st)); });
}
int mmvae_celeba_iw_tail(const void* q3, const float* affine, int act, const float* w, const float* image, int B, int K, float* loglik,
                         float* logits, void* st) {
    return guarded([&]() -> int {
        MMVAE_REQUIRE(affine != nullptr, "mmvae_celeba_iw_tail: null affine table");
        MMVAE_REQUIRE(B >= 1 && K >= 1 && (long long)B * K <= 0x3FFFFFFF, "mmvae_celeba_iw_tail: B=%d K=%d out of range", B, K);
        IwTailArgs a{};
        a.q3 = static_cast<const bf16*>(q3); a.affine = reinterpret_cast<const float2*>(affine); a.act = act; a.w = w; a.image = image;
        a.rows = B * K; a.K = K; a.loglik = loglik; a.logits = logits;
        return launch_celeba_iw_tail(a, S(st));
    });
}
int mmvae_celeba_iw_attrs(mmvae_celeba_t* p, const float* z, long long rows, float* words, void* st) {
    return guarded([&] { return celeba_iw_attrs(p, z, rows, words, S(st)); });
}

// ---- COCO (coco/model.py, coco/train.py)
mmvae_coco_t* mmvae_coco_create_t(int n_latents, int batch, int steps) {
    try { return coco_create(n_latents, batch, steps); } catch (...) { mmvae_set_error("coco_create failed"); return nullptr; }
}
mmvae_coco_t* mmvae_coco_create(int n_latents, int batch) { return mmvae_coco_create_t(n_latents, batch, 102); }
void mmvae_coco_destroy(mmvae_coco_t* p) { coco_destroy(p); }
int mmvae_coco_steps(const mmvae_coco_t* p) { return p ? coco_steps(p) : 0; }
MMVAE_PLAN_API(coco, mmvae_coco_t, coco_b)
int mmvae_coco_step(mmvae_coco_t* p, const mmvae_coco_step_io* io, int training, int do_backward, void* stream) {
    return guarded([&]() -> int {
        MMVAE_REQUIRE(p && io, "mmvae_coco_step: null argument");
        return coco_step(p, *io, training, do_backward, S(stream));
    });
}
int mmvae_coco_image_step(mmvae_coco_t* p, const mmvae_image_step_io* io, int training, int do_backward, void* stream) {
    return guarded([&]() -> int {
        MMVAE_REQUIRE(p && io, "mmvae_coco_image_step: null argument");
        return coco_image_step(p, *io, training, do_backward, S(stream));
    });
}
size_t mmvae_coco_image_step_workspace_bytes(const mmvae_coco_t* p) { return p ? coco_image_step_workspace_bytes(p) : 0; }
int mmvae_coco_infovae_step(mmvae_coco_t* p, const mmvae_infovae_step_io* io, int training, int do_backward, void* stream) {
    return guarded([&]() -> int {
        MMVAE_REQUIRE(p && io, "mmvae_coco_infovae_step: null argument");
        return coco_infovae_step(p, *io, training, do_backward, S(stream));
    });
}
size_t mmvae_coco_infovae_step_workspace_bytes(const mmvae_coco_t* p) { return p ? coco_infovae_step_workspace_bytes(p) : 0; }
int mmvae_coco_iw_score_image(mmvae_coco_t* p, void* ws, size_t wsb, const float* z, const float* image, int B, int K, float* loglik_x, void* st) {
    return guarded([&] { return coco_iw_score_image(p, ws, wsb, z, image, B, K, loglik_x, S(st)); });
}
int mmvae_coco_text_step(mmvae_coco_t* p, const mmvae_text_step_io* io, int training, int do_backward, void* stream) {
    return guarded([&]() -> int {
        MMVAE_REQUIRE(p && io, "mmvae_coco_text_step: null argument");
        return coco_text_step(p, *io, training, do_backward, S(stream));
    });
}
size_t mmvae_coco_text_step_workspace_bytes(const mmvae_coco_t* p) { return p ? coco_text_step_workspace_bytes(p) : 0; }
int mmvae_coco_iw_score_text(mmvae_coco_t* p, void* ws, size_t wsb, const float* z, const float* text, const float* sos, int B, int K,
                             float* sse_y, void* st) {
    return guarded([&] { return coco_iw_score_text(p, ws, wsb, z, text, sos, B, K, sse_y, S(st)); });
}
int mmvae_coco_image_encoder_fwd(mmvae_coco_t* p, void* ws, size_t wsb, const float* image, const uint8_t* m1, const uint8_t* m2, int training, float* out, void* st) {
    return guarded([&] { return coco_image_encoder_fwd(p, ws, wsb, image, m1, m2, training, out, S(st)); });
}
int mmvae_coco_image_encoder_bwd(mmvae_coco_t* p, void* ws, size_t wsb, const float* d_out, const uint8_t* m1, const uint8_t* m2, void* st) {
    return guarded([&] { return coco_image_encoder_bwd(p, ws, wsb, d_out, m1, m2, S(st)); });
}
int mmvae_coco_image_decoder_fwd(mmvae_coco_t* p, void* ws, size_t wsb, const float* z, int training, float* recon, void* st) {
    return guarded([&] { return coco_image_decoder_fwd(p, ws, wsb, z, training, recon, S(st)); });
}
int mmvae_coco_image_decoder_bwd(mmvae_coco_t* p, void* ws, size_t wsb, const float* d_recon, const float* recon, float* dz, void* st) {
    return guarded([&] { return coco_image_decoder_bwd(p, ws, wsb, d_recon, recon, dz, S(st)); });
}
int mmvae_coco_text_encoder_fwd(mmvae_coco_t* p, void* ws, size_t wsb, const float* text, float* out, void* st) {
    return guarded([&] { return coco_text_encoder_fwd(p, ws, wsb, text, out, S(st)); });
}
int mmvae_coco_text_encoder_bwd(mmvae_coco_t* p, void* ws, size_t wsb, const float* text, const float* d_out, void* st) {
    return guarded([&] { return coco_text_encoder_bwd(p, ws, wsb, text, d_out, S(st)); });
}
int mmvae_coco_text_decoder_fwd(mmvae_coco_t* p, void* ws, size_t wsb, const float* z, const float* sos, const uint8_t* keep, int training, float* sentence, void* st) {
    return guarded([&] { return coco_text_decoder_fwd(p, ws, wsb, z, sos, keep, training, sentence, S(st)); });
}
int mmvae_coco_text_decoder_bwd(mmvae_coco_t* p, void* ws, size_t wsb, const float* z, const float* sos, const uint8_t* keep, const float* sentence, const float* d_sentence, float* dz, void* st) {
    return guarded([&] { return coco_text_decoder_bwd(p, ws, wsb, z, sos, keep, sentence, d_sentence, dz, S(st)); });
}
int mmvae_coco_bench_layer(mmvae_coco_t* p, void* ws, size_t wsb, const char* layer, int iters, void* stream) {
    return guarded([&] { return coco_bench_layer(p, ws, wsb, layer, iters, S(stream)); });
}
long long mmvae_coco_debug_offset(mmvae_coco_t* p, const char* name) { return coco_debug_offset(p, name); }
size_t mmvae_coco_iw_workspace_bytes(const mmvae_coco_t* p) { return p ? coco_iw_workspace_bytes(p) : 0; }
int mmvae_coco_iw_score(mmvae_coco_t* p, void* ws, size_t wsb, const float* z, const float* image, const float* text, const float* sos,
                        int B, int K, float* loglik_x, float* sse_y, void* st) {
    return guarded([&] { return coco_iw_score(p, ws, wsb, z, image, text, sos, B, K, loglik_x, sse_y, S(st)); });
}
int mmvae_coco_iw_tail(const void* q3, const float* affine, int act, const float* w, const float* image, int B, int K, float* loglik,
                       float* logits, void* st) {
    return guarded([&]() -> int {
        MMVAE_REQUIRE(affine != nullptr, "mmvae_coco_iw_tail: null affine table");
        MMVAE_REQUIRE(B >= 1 && K >= 1 && (long long)B * K <= 0x3FFFFFFF, "mmvae_coco_iw_tail: B=%d K=%d out of range", B, K);
        IwTailArgs a{};
        a.q3 = static_cast<const bf16*>(q3); a.affine = reinterpret_cast<const float2*>(affine); a.act = act; a.w = w; a.image = image;
        a.rows = B * K; a.K = K; a.loglik = loglik; a.logits = logits;
        return launch_coco_iw_tail(a, S(st));
    });
}
int mmvae_coco_iw_text_sse(const float* sentence, const float* text, int B, int K, int steps, float* sse, void* st) {
    return guarded([&] { return launch_coco_iw_text_sse(sentence, text, B, K, steps, sse, S(st)); });
}


int mmvae_poe_fwd(const float* mu, const float* lv, int M, int n, float* omu, float* olv, void* s) { return launch_poe_fwd(mu, lv, M, n, omu, olv, S(s)); }
int mmvae_poe_bwd(const float* mu, const float* lv, int M, int n, const float* gmu, const float* glv, float* dmu, float* dlv, void* s) {
    return launch_poe_bwd(mu, lv, M, n, gmu, glv, dmu, dlv, S(s));
}
int mmvae_reparam_fwd(const float* mu, const float* lv, const float* eps, int n, float* z, void* s) { return launch_reparam_fwd(mu, lv, eps, n, z, S(s)); }
int mmvae_reparam_bwd(const float* lv, const float* eps, const float* dz, int n, float* dmu, float* dlv, void* s) {
    return launch_reparam_bwd(lv, eps, dz, n, dmu, dlv, S(s));
}
size_t mmvae_latent1_scratch_floats(int B, int D) { return B >= 1 && D >= 1 ? launch_latent1_scratch_floats(B, D) : 0; }
int mmvae_latent1_fwd(const float* enc_out, const float* eps, int B, int D, int training, float* mu, float* logvar, float* z, void* z_bf16,
                      int ldz, float* kl_sum, float* scratch, void* st) {
    return guarded([&] {
        Latent1Args a{};
        a.B = B; a.D = D; a.enc_out = enc_out; a.eps = eps; a.mu = mu; a.logvar = logvar; a.z_f32 = z; a.z_bf = (bf16*)z_bf16; a.ldz = ldz;
        a.kl_sum = kl_sum; a.training = training; a.scratch = scratch;
        return launch_latent1_fwd(a, S(st));
    });
}
int mmvae_latent1_bwd(const float* mu, const float* logvar, const float* eps, const float* dz, int B, int D, int training, float kl_coef,
                      void* d_enc_out_bf16, int ld, float* d_bias, const float* loss_slots, float* loss_out, float* scratch, void* st) {
    return guarded([&] {
        Latent1BwdArgs a{};
        a.f.B = B; a.f.D = D; a.f.mu = const_cast<float*>(mu); a.f.logvar = const_cast<float*>(logvar); a.f.eps = eps; a.f.training = training;
        a.f.scratch = scratch;
        a.dz = dz; a.kl_coef = kl_coef; a.d_enc_out = (bf16*)d_enc_out_bf16; a.ld = ld; a.d_bias = d_bias; a.loss_slots = loss_slots; a.loss_out = loss_out;
        return launch_latent1_bwd(a, S(st));
    });
}
int mmvae_latent1_bwd_f32(const float* mu, const float* logvar, const float* eps, const float* dz, int B, int D, int training, float kl_coef,
                          float* d_enc_out, int ld, void* st) {
    return guarded([&] {
        Latent1BwdF32Args a{};
        a.B = B; a.D = D; a.mu = mu; a.logvar = logvar; a.eps = eps; a.dz = dz; a.training = training; a.kl_coef = kl_coef;
        a.d_enc_out = d_enc_out; a.ld = ld;
        return launch_latent1_bwd_f32(a, S(st));
    });
}
// ---- the streaming kernels of every step on plain device pointers (test and measurement aid): each fills the argument struct of the step's
// own launcher, whose checks refuse what the kernel would index out of range
int mmvae_latent3_fwd(const float* img_out, const float* img_out_b, const float* txt_out, const float* eps, int B, int D, int training,
                      float* mu, float* logvar, float* z, void* z_bf16, int ldz, float* kl_slots, void* st) {
    return guarded([&] {
        Latent3Args a{};
        a.B = B; a.D = D; a.img_out = img_out; a.img_out_b = img_out_b; a.txt_out = txt_out; a.eps = eps; a.mu = mu; a.logvar = logvar;
        a.z_f32 = z; a.z_bf = (bf16*)z_bf16; a.ldz = ldz; a.kl_sum = kl_slots; a.training = training;
        return launch_latent3_fwd(a, S(st));
    });
}
int mmvae_latent3_bwd(const float* img_out, const float* img_out_b, const float* txt_out, const float* mu, const float* logvar,
                      const float* eps, const float* dz_a, const float* dz_b, int B, int D, int training, float kl_coef0, float kl_coef1,
                      float kl_coef2, void* d_img_out_bf16, int ld_img_out_bf, int sum_img_variants, float* d_img_out_f32, float* d_img_bias,
                      float* d_txt_out, void* d_txt_out_bf16, float* d_txt_bias, const float* loss_slots, float* loss_out, void* st) {
    return guarded([&] {
        Latent3BwdArgs a{};
        a.f.B = B; a.f.D = D; a.f.img_out = img_out; a.f.img_out_b = img_out_b; a.f.txt_out = txt_out; a.f.eps = eps;
        a.f.mu = const_cast<float*>(mu); a.f.logvar = const_cast<float*>(logvar); a.f.training = training;
        a.dz_a = dz_a; a.dz_b = dz_b; a.kl_coef[0] = kl_coef0; a.kl_coef[1] = kl_coef1; a.kl_coef[2] = kl_coef2;
        a.d_img_out_bf = (bf16*)d_img_out_bf16; a.ld_img_out_bf = ld_img_out_bf; a.sum_img_variants = sum_img_variants;
        a.d_img_out_f32 = d_img_out_f32; a.d_img_bias = d_img_bias; a.d_txt_out = d_txt_out; a.d_txt_out_bf = (bf16*)d_txt_out_bf16;
        a.d_txt_bias = d_txt_bias; a.loss_slots = loss_slots; a.loss_out = loss_out;
        return launch_latent3_bwd(a, S(st));
    });
}
int mmvae_sigmoid_bce(const float* logits, int ldl, const float* target, int G, int B, int C, int H, int W, const float* coef_host,
                      float* recon, float* dlogit, float* loss_sum, void* st) {
    return guarded([&] {
        MMVAE_REQUIRE(G >= 1 && G <= 4 && coef_host, "sigmoid_bce: G=%d (1..4) or coef missing", G);
        BceArgs a{};
        a.logits = logits; a.ldl = ldl; a.target = target; a.G = G; a.B = B; a.C = C; a.H = H; a.W = W; a.recon = recon; a.dlogit = dlogit;
        for (int g = 0; g < G; ++g) a.coef[g] = coef_host[g];
        a.loss_sum = loss_sum;
        return launch_sigmoid_bce(a, S(st));
    });
}
int mmvae_logsoftmax_nll(const float* logits, int rows, int classes, float* words, const long long* target, int target_rows,
                         int rows_per_group, float* nll_slots, void* dlogits_bf16, int ld_d, float* dlogits_f32, const float* coef_host,
                         void* st) {
    return guarded([&] {
        MMVAE_REQUIRE(coef_host && rows >= 1 && rows_per_group >= 1 && (rows + rows_per_group - 1) / rows_per_group <= 4,
                      "logsoftmax_nll: coef missing, or rows=%d are not 1..4 groups of %d", rows, rows_per_group);
        LogSoftmaxNllArgs a{};
        a.logits = logits; a.rows = rows; a.classes = classes; a.words = words; a.target = target; a.target_rows = target_rows;
        a.rows_per_group = rows_per_group; a.nll_sum = nll_slots; a.dlogits = (bf16*)dlogits_bf16; a.ld_d = ld_d; a.dlogits_f32 = dlogits_f32;
        for (int g = 0; g < (rows + rows_per_group - 1) / rows_per_group; ++g) a.coef[g] = coef_host[g];
        return launch_logsoftmax_nll(a, S(st));
    });
}
static BnFinalizeArgs bn_fin_of(const float* stats, int G, int C, float count, const float* gamma, const float* beta, float* running_mean,
                                float* running_var, long long* nbt, int updates_per_group, unsigned skip_update_mask, float* affine,
                                float* meanrstd, float eps, float momentum, int training) {
    BnFinalizeArgs f{};
    f.stats = (const float2*)stats; f.G = G; f.C = C; f.count = count; f.gamma = gamma; f.beta = beta; f.running_mean = running_mean;
    f.running_var = running_var; f.num_batches_tracked = nbt; f.updates_per_group = updates_per_group; f.skip_update_mask = skip_update_mask;
    f.affine = (float2*)affine; f.meanrstd = (float2*)meanrstd; f.eps = eps; f.momentum = momentum; f.training = training;
    return f;
}
int mmvae_bn_finalize(const float* stats, int G, int C, float count, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, long long* nbt, int updates_per_group, unsigned skip_update_mask, float* affine, float* meanrstd,
                      float eps, float momentum, int training, void* st) {
    return guarded([&] {
        return launch_bn_finalize(bn_fin_of(stats, G, C, count, gamma, beta, running_mean, running_var, nbt, updates_per_group,
                                            skip_update_mask, affine, meanrstd, eps, momentum, training), S(st));
    });
}
int mmvae_bn_act(const void* r_bf16, void* a_bf16, int rows, int C, int ld, int rows_per_group, int G, int act, const float* stats,
                 float count, const float* gamma, const float* beta, float* running_mean, float* running_var, long long* nbt,
                 int updates_per_group, unsigned skip_update_mask, float* affine, float* meanrstd, float eps, float momentum, int training,
                 void* st) {
    return guarded([&] {
        MMVAE_REQUIRE(act == ACT_NONE || act == ACT_SWISH || act == ACT_RELU, "bn_act: activation code %d", act);
        BnActArgs a{};
        a.r = (const bf16*)r_bf16; a.a = (bf16*)a_bf16; a.rows = rows; a.C = C; a.ld = ld; a.rows_per_group = rows_per_group; a.G = G; a.act = act;
        a.fin = bn_fin_of(stats, G, C, count, gamma, beta, running_mean, running_var, nbt, updates_per_group, skip_update_mask, affine,
                          meanrstd, eps, momentum, training);
        return launch_bn_act(a, S(st));
    });
}
int mmvae_bn_bwd_apply(const void* db_bf16, const void* db2_bf16, const void* r_bf16, void* dr_bf16, int rows, int C, int ld,
                       int rows_per_group, int G, const float* red, const float* meanrstd, const float* gamma, float* dgamma, float* dbeta,
                       void* st) {
    return guarded([&] {
        BnBwdApplyArgs a{};
        a.db = (const bf16*)db_bf16; a.db2 = (const bf16*)db2_bf16; a.r = (const bf16*)r_bf16; a.dr = (bf16*)dr_bf16; a.rows = rows; a.C = C;
        a.ld = ld; a.rows_per_group = rows_per_group; a.G = G; a.red = (const float2*)red; a.meanrstd = (const float2*)meanrstd;
        a.gamma = gamma; a.dgamma = dgamma; a.dbeta = dbeta;
        return launch_bn_bwd_apply(a, S(st));
    });
}
int mmvae_embed_gather_stats(const float* table, int C, const long long* idx, int rows, int idx_rows, int rows_per_group, void* x_bf16,
                             int ld, float* colstats, void* st) {
    return guarded([&] { return launch_embed_gather_stats(table, C, idx, rows, idx_rows, rows_per_group, (bf16*)x_bf16, ld, (float2*)colstats, S(st)); });
}
int mmvae_embed_scatter_add(const void* d_bf16, int ld, int C, const long long* idx, int rows, float* g_table, void* st) {
    return guarded([&] { return launch_embed_scatter_add((const bf16*)d_bf16, ld, C, idx, rows, g_table, S(st)); });
}
int mmvae_colsum_f32(const float* x, int rows, int cols, float* out, void* st) {
    return guarded([&] { return launch_colsum_f32(x, rows, cols, out, S(st)); });
}
int mmvae_colsum_bf16(const void* x_bf16, int ld, int rows, int cols, float* out, void* st) {
    return guarded([&] { return launch_colsum_bf16((const bf16*)x_bf16, ld, rows, cols, out, S(st)); });
}
int mmvae_kl_fwd(const float* mu, const float* lv, int n, float* out, void* s) { return launch_kl_fwd(mu, lv, n, out, S(s)); }
int mmvae_kl_bwd(const float* mu, const float* lv, int n, float coef, const float* gs, float* dmu, float* dlv, void* s) { return launch_kl_bwd(mu, lv, n, coef, gs, dmu, dlv, S(s)); }
int mmvae_bce_fwd(const float* p, const float* t, long long n, float* out, void* s) { return launch_bce_fwd(p, t, n, out, S(s)); }
int mmvae_bce_bwd(const float* p, const float* t, long long n, float coef, const float* gs, float* dp, void* s) { return launch_bce_bwd(p, t, n, coef, gs, dp, S(s)); }
int mmvae_nll_fwd(const float* lp, const long long* tg, int rows, int classes, float* out, void* s) { return launch_nll_fwd(lp, tg, rows, classes, out, S(s)); }
int mmvae_nll_bwd(const long long* tg, int rows, int classes, float coef, const float* gs, float* dlp, void* s) { return launch_nll_bwd(tg, rows, classes, coef, gs, dlp, S(s)); }
int mmvae_iw_particles(const float* mu, const float* lv, int B, int D, int K, long long first_row, long long first_particle,
                       unsigned long long seed, const float* eps, float* z, float* log_ratio, void* s) {
    return launch_iw_particles(mu, lv, B, D, K, first_row, first_particle, seed, eps, z, log_ratio, S(s));
}
int mmvae_iw_init(float* state, int B, void* s) { return launch_iw_init(state, B, S(s)); }
int mmvae_iw_accumulate(const float* lx, const float* words, const long long* targets, int T, int V, const float* log_ratio, int B, int K,
                        float* state, float* log_w, void* s) {
    return launch_iw_accumulate(lx, words, targets, T, V, log_ratio, B, K, state, log_w, S(s));
}
int mmvae_iw_finalize(const float* state, int B, long long K_total, float* out, void* s) { return launch_iw_finalize(state, B, K_total, out, S(s)); }
int mmvae_normal(float* out, long long n, unsigned long long seed, const long long* ctr, unsigned sid, void* s) { return launch_normal(out, n, seed, ctr, sid, S(s)); }
int mmvae_keep_mask(uint8_t* out, long long n, float p, unsigned long long seed, const long long* ctr, unsigned sid, void* s) {
    return launch_keep_mask(out, n, p, seed, ctr, sid, S(s));
}
int mmvae_mse_fwd(const float* a, const float* b, long long n, float* out, void* s) { return launch_mse_fwd(a, b, n, out, S(s)); }
int mmvae_mse_bwd(const float* a, const float* b, long long n, float coef, const float* gs, float* da, void* s) { return launch_mse_bwd(a, b, n, coef, gs, da, S(s)); }
int mmvae_u8_to_f32(const uint8_t* src, long long n, float denom, float* dst, void* s) { return launch_u8_to_f32(src, n, denom, dst, S(s)); }
int mmvae_u8_to_f32_after(const uint8_t* src, long long n, float denom, float* dst, void* wait_event, void* s) {
    if (wait_event && hipStreamWaitEvent(S(s), reinterpret_cast<hipEvent_t>(wait_event), 0) != hipSuccess) {
        mmvae_set_error("u8_to_f32_after: hipStreamWaitEvent: %s", hipGetErrorString(hipGetLastError()));
        return MMVAE_EHIP;
    }
    return launch_u8_to_f32(src, n, denom, dst, S(s));
}
int mmvae_gather_rows_u8_f32(const uint8_t* src, const long long* idx, long long rows, long long row_elems, float denom, float* dst, void* s) {
    return launch_gather_rows_u8_f32(src, idx, rows, row_elems, denom, dst, S(s));
}
int mmvae_stream_wait_event(void* s, void* e) {
    MMVAE_REQUIRE(e, "stream_wait_event: null event");
    if (hipStreamWaitEvent(S(s), reinterpret_cast<hipEvent_t>(e), 0) != hipSuccess) { mmvae_set_error("hipStreamWaitEvent: %s", hipGetErrorString(hipGetLastError())); return MMVAE_EHIP; }
    return MMVAE_OK;
}
int mmvae_event_create(void** out) {
    MMVAE_REQUIRE(out, "event_create: null argument");
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess) {
        mmvae_set_error("hipEventCreate failed: %s", hipGetErrorString(hipGetLastError()));
        return MMVAE_EHIP;
    }
    *out = e;
    return MMVAE_OK;
}
int mmvae_event_destroy(void* e) { return e && hipEventDestroy(reinterpret_cast<hipEvent_t>(e)) != hipSuccess ? MMVAE_EHIP : MMVAE_OK; }
int mmvae_event_record(void* e, void* s) {
    MMVAE_REQUIRE(e, "event_record: null event");
    if (hipEventRecord(reinterpret_cast<hipEvent_t>(e), S(s)) != hipSuccess) { mmvae_set_error("hipEventRecord: %s", hipGetErrorString(hipGetLastError())); return MMVAE_EHIP; }
    return MMVAE_OK;
}
int mmvae_event_synchronize(void* e) {
    MMVAE_REQUIRE(e, "event_synchronize: null event");
    if (hipEventSynchronize(reinterpret_cast<hipEvent_t>(e)) != hipSuccess) { mmvae_set_error("hipEventSynchronize: %s", hipGetErrorString(hipGetLastError())); return MMVAE_EHIP; }
    return MMVAE_OK;
}
int mmvae_h2d_stage(void* dst_a, const void* src_a, size_t bytes_a, void* dst_b, const void* src_b, size_t bytes_b, void* event, void* s) {
    MMVAE_REQUIRE(dst_a && src_a && bytes_a > 0 && event && (bytes_b == 0 || (dst_b && src_b)), "h2d_stage: null argument");
    hipError_t e = hipMemcpyAsync(dst_a, src_a, bytes_a, hipMemcpyHostToDevice, S(s));
    if (e == hipSuccess && bytes_b > 0) e = hipMemcpyAsync(dst_b, src_b, bytes_b, hipMemcpyHostToDevice, S(s));
    if (e == hipSuccess) e = hipEventRecord(reinterpret_cast<hipEvent_t>(event), S(s));
    if (e != hipSuccess) { mmvae_set_error("h2d_stage: %s", hipGetErrorString(e)); (void)hipGetLastError(); return MMVAE_EHIP; }
    return MMVAE_OK;
}
int mmvae_adam_step(float* p, const float* g, float* m, float* v, long long n, long long* state, float lr, float b1, float b2,
                    float eps, float grad_scale, void* s) {
    AdamArgs a{};
    a.p = p; a.g = g; a.m = m; a.v = v; a.n = n; a.step = state; a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = eps; a.grad_scale = grad_scale;
    return launch_adam(a, S(s));
}
int mmvae_stream_create(void** out) {
    MMVAE_REQUIRE(out, "stream_create: null argument");
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
        mmvae_set_error("hipStreamCreate failed: %s", hipGetErrorString(hipGetLastError()));
        return MMVAE_EHIP;
    }
    *out = s;
    return MMVAE_OK;
}
int mmvae_stream_destroy(void* s) {
    if (s && hipStreamDestroy(S(s)) != hipSuccess) { mmvae_set_error("hipStreamDestroy failed"); return MMVAE_EHIP; }
    return MMVAE_OK;
}
int mmvae_gather_rows(const void* src, const long long* idx, long long rows, long long row_bytes, void* dst, void* s) {
    return launch_gather_rows(src, idx, rows, row_bytes, dst, S(s));
}
int mmvae_step_status(const float* sums, void* s) {
    MMVAE_REQUIRE(sums, "step_status: null sums");
    float h[16];
    if (hipMemcpyAsync(h, sums, sizeof(h), hipMemcpyDeviceToHost, S(s)) != hipSuccess || hipStreamSynchronize(S(s)) != hipSuccess) {
        mmvae_set_error("step_status: %s", hipGetErrorString(hipGetLastError()));
        return MMVAE_EHIP;
    }
    if (h[15] != h[15]) {        // only a void step writes NaN there (no loss term accumulates into word 15)
        mmvae_set_error("the step gave up on a device-side exchange (caption decoder cluster): losses are NaN, the optimizer update was skipped");
        return MMVAE_ETIMEOUT;
    }
    return MMVAE_OK;
}
int mmvae_step_losses(const float* sums, const float* w_bce, const float* w_nll, const float* w_kl, float* losses, void* s) {
    MMVAE_REQUIRE(w_bce && w_nll && w_kl, "step_losses: null weights");
    StepLossArgs a{};
    a.sums = sums; a.out = losses;
    for (int k = 0; k < 3; ++k) { a.w_bce[k] = w_bce[k]; a.w_nll[k] = w_nll[k]; a.w_kl[k] = w_kl[k]; }
    return launch_step_losses(a, S(s));
}
int mmvae_adam_step_packed_ranges(float* p, float* g, float* m, float* v, long long n, const long long* ranges, int nr, int advance,
                                  long long* state, float lr, float b1, float b2, float eps, float grad_scale, const int* gmap,
                                  const float* gpk, const float* gpk_vec, void* s) {
    MMVAE_REQUIRE(gmap && gpk && gpk_vec && ranges && nr >= 1 && nr <= 4, "adam_step_packed_ranges: null argument or more than 4 ranges");
    AdamArgs a{};
    a.p = p; a.g = g; a.m = m; a.v = v; a.n = n; a.step = state; a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = eps; a.grad_scale = grad_scale;
    a.gmap = gmap; a.gpk = gpk; a.gpk_vec = gpk_vec; a.g_out = g;
    a.nr = nr; a.no_advance = advance ? 0 : 1;
    for (int r = 0; r < nr; ++r) { a.roff[r] = ranges[2 * r]; a.rlen[r] = ranges[2 * r + 1]; }
    return launch_adam(a, S(s));
}
int mmvae_mm_early_ranges(const mmvae_mm_t* p, long long* ranges, int cap) {
    if (!p || !ranges) return 0;
    return mm_early_ranges(p, ranges, cap);
}
int mmvae_adam_step_packed(float* p, float* g, float* m, float* v, long long n, long long* state, float lr, float b1, float b2,
                           float eps, float grad_scale, const int* gmap, const float* gpk, const float* gpk_vec, void* s) {
    MMVAE_REQUIRE(gmap && gpk && gpk_vec, "adam_step_packed: null gradient map / packed buffers");
    AdamArgs a{};
    a.p = p; a.g = g; a.m = m; a.v = v; a.n = n; a.step = state; a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = eps; a.grad_scale = grad_scale;
    a.gmap = gmap; a.gpk = gpk; a.gpk_vec = gpk_vec; a.g_out = g;
    return launch_adam(a, S(s));
}

}  // extern "C"

// ---- the workspace check of every stand-alone op: a null (align16: or misaligned) buffer is MMVAE_EINVAL, one below `need` MMVAE_ENOSPC
static int ws_fits(const char* what, const void* ws, long long ws_bytes, long long need, bool align16) {
    if (align16) MMVAE_REQUIRE(ws && aligned16(ws), "%s: the workspace must be a 16-byte aligned device buffer", what);
    else MMVAE_REQUIRE(ws, "%s: null workspace", what);
    if (ws_bytes < need) { mmvae_set_error("%s: workspace too small (%lld < %lld)", what, ws_bytes, need); return MMVAE_ENOSPC; }
    return MMVAE_OK;
}

// ---- nearest-word search over an embedding table (nn_words.h)
long long mmvae_nn_words_workspace_bytes(int n_queries, long long n_words) {
    if (n_queries <= 0 || n_words <= 0) return 0;
    return (long long)nn_words_workspace_bytes(n_queries, n_words);
}
int mmvae_nn_words_geometry(int* query_tile, int* word_tile, int* max_splits) {
    MMVAE_REQUIRE(query_tile && word_tile && max_splits, "nn_words_geometry: null argument");
    *query_tile = NNW_TQ; *word_tile = NNW_TV; *max_splits = NNW_MAX_SPLITS;
    return MMVAE_OK;
}
int mmvae_nn_words_norms(const float* table, long long n_words, int dim, float* sqnorm, void* s) {
    MMVAE_REQUIRE(table && sqnorm, "nn_words_norms: null argument");
    MMVAE_REQUIRE(n_words > 0, "nn_words_norms: n_words = %lld", n_words);
    MMVAE_REQUIRE(dim == NNW_DIM, "nn_words_norms: dim = %d, the kernels are built for %d", dim, NNW_DIM);
    return launch_nn_words_norms(table, n_words, sqnorm, S(s));
}
int mmvae_nn_words_nearest(const float* queries, int n_queries, const float* table, const float* sqnorm, long long n_words, int dim,
                           void* ws, long long ws_bytes, long long* index, float* dist, void* s) {
    MMVAE_REQUIRE(queries && table && sqnorm && ws && index && dist, "nn_words_nearest: null argument");
    MMVAE_REQUIRE(n_queries > 0 && n_words > 0, "nn_words_nearest: n_queries = %d, n_words = %lld", n_queries, n_words);
    MMVAE_REQUIRE(dim == NNW_DIM, "nn_words_nearest: dim = %d, the kernels are built for %d", dim, NNW_DIM);
    MMVAE_TRY(ws_fits("nn_words_nearest", ws, ws_bytes, (long long)nn_words_workspace_bytes(n_queries, n_words), false));
    return launch_nn_words_nearest(queries, n_queries, table, sqnorm, n_words, ws, index, dist, S(s));
}
int mmvae_nn_words_dists(const float* queries, int n_queries, const float* table, long long n_words, int dim, float* dist, void* s) {
    MMVAE_REQUIRE(queries && table && dist, "nn_words_dists: null argument");
    MMVAE_REQUIRE(n_queries > 0 && n_queries <= NNW_MAX_DISTS, "nn_words_dists: n_queries = %d, need 1..%d", n_queries, NNW_MAX_DISTS);
    MMVAE_REQUIRE(n_words > 0, "nn_words_dists: n_words = %lld", n_words);
    MMVAE_REQUIRE(dim == NNW_DIM, "nn_words_dists: dim = %d, the kernels are built for %d", dim, NNW_DIM);
    return launch_nn_words_dists(queries, n_queries, table, n_words, dist, S(s));
}

// ---- Gaussian-kernel MMD, value + both gradients (mmd.h)
static bool mmd_sizes_ok(const char* what, int n_x, int n_y, int dim) {
    if (n_x < 1 || n_x > MMD_MAX_N || n_y < 1 || n_y > MMD_MAX_N) {
        mmvae_set_error("%s: n_x = %d, n_y = %d, need 1..%d", what, n_x, n_y, (int)MMD_MAX_N);
        return false;
    }
    if (dim < 1 || dim > MMD_MAX_DIM) {
        mmvae_set_error("%s: dim = %d, need 1..%d", what, dim, (int)MMD_MAX_DIM);
        return false;
    }
    return true;
}
int mmvae_mmd_geometry(int* row_tile, int* col_tile, int* max_dim) {
    MMVAE_REQUIRE(row_tile && col_tile && max_dim, "mmd_geometry: null argument");
    *row_tile = MMD_RT; *col_tile = MMD_CT; *max_dim = MMD_MAX_DIM;
    return MMVAE_OK;
}
long long mmvae_mmd_workspace_bytes(int n_x, int n_y, int dim) {
    if (n_x < 1 || n_x > MMD_MAX_N || n_y < 1 || n_y > MMD_MAX_N || dim < 1 || dim > MMD_MAX_DIM) return 0;
    return (long long)mmd_workspace_bytes(n_x, n_y, dim);
}
int mmvae_mmd(const float* x, int n_x, const float* y, int n_y, int dim, void* ws, long long ws_bytes, float* out4, float* dx, float* dy,
              void* s) {
    MMVAE_REQUIRE(x && y && ws && out4, "mmd: null argument");
    if (!mmd_sizes_ok("mmd", n_x, n_y, dim)) return MMVAE_EINVAL;
    MMVAE_TRY(ws_fits("mmd", ws, ws_bytes, (long long)mmd_workspace_bytes(n_x, n_y, dim), false));
    return launch_mmd(x, n_x, y, n_y, dim, ws, out4, dx, dy, S(s));
}
long long mmvae_mmd_dy_workspace_bytes(int n_x, int n_y, int dim) {
    if (n_x < 1 || n_x > MMD_MAX_N || n_y < 1 || n_y > MMD_MAX_N || dim < 1 || dim > MMD_MAX_DIM) return 0;
    return (long long)mmd_dy_workspace_bytes(n_x, n_y, dim);
}
int mmvae_mmd_dy(const float* x, int n_x, const float* y, int n_y, int dim, void* ws, long long ws_bytes, float scale, float* out4, float* dy,
                 int grad_y_only, void* s) {
    MMVAE_REQUIRE(x && y && ws && out4, "mmd_dy: null argument");
    MMVAE_REQUIRE(grad_y_only == 1, "mmd_dy: grad_y_only = %d, this entry computes the gradient for y alone (mmvae_mmd has both)", grad_y_only);
    if (!mmd_sizes_ok("mmd_dy", n_x, n_y, dim)) return MMVAE_EINVAL;
    MMVAE_TRY(ws_fits("mmd_dy", ws, ws_bytes, (long long)mmd_dy_workspace_bytes(n_x, n_y, dim), false));
    return launch_mmd_dy(x, n_x, y, n_y, dim, ws, scale, out4, dy, S(s));
}
int mmvae_mmd_kernel_matrix(const float* x, int n_x, const float* y, int n_y, int dim, float* k, void* s) {
    MMVAE_REQUIRE(x && y && k, "mmd_kernel_matrix: null argument");
    if (!mmd_sizes_ok("mmd_kernel_matrix", n_x, n_y, dim)) return MMVAE_EINVAL;
    return launch_mmd_kernel_matrix(x, n_x, y, n_y, dim, k, S(s));
}

// ---- PixelCNN / GatedPixelCNN incremental sampler (pixelcnn.h)
static bool pcnn_model_ok(const char* what, const PcnnCfg& c) {
    if (pcnn_cfg_ok(c)) return true;
    mmvae_set_error("%s: gated = %d, n_blocks = %d, data_channels = %d, hid_dims = %d, out_dims = %d: need n_blocks 0..%d, data_channels 1 or 3, "
                    "hid_dims a multiple of 16 in 16..%d, out_dims 2..%d", what, c.gated, c.n_blocks, c.channels, c.hid, c.levels,
                    (int)PCNN_MAX_BLOCKS, (int)PCNN_MAX_HID, (int)PCNN_MAX_LEVELS);
    return false;
}
static bool pcnn_shape_ok(const char* what, int batch, int height, int width) {
    if (batch >= 1 && height >= 1 && height <= PCNN_MAX_SIDE && width >= 1 && width <= PCNN_MAX_SIDE) return true;
    mmvae_set_error("%s: batch = %d, height = %d, width = %d: need batch >= 1 and sides 1..%d", what, batch, height, width, (int)PCNN_MAX_SIDE);
    return false;
}
int mmvae_pixelcnn_geometry(int* sample_tile, int* max_hid, int* max_side) {
    MMVAE_REQUIRE(sample_tile && max_hid && max_side, "pixelcnn_geometry: null argument");
    *sample_tile = PCNN_TILE; *max_hid = PCNN_MAX_HID; *max_side = PCNN_MAX_SIDE;
    return MMVAE_OK;
}
long long mmvae_pixelcnn_param_elems(int gated, int n_blocks, int channels, int hid, int levels) {
    const PcnnCfg c{gated, n_blocks, channels, hid, levels};
    return pcnn_cfg_ok(c) ? pcnn_plan(c, 1)->param_floats : 0;
}
long long mmvae_pixelcnn_packed_elems(int gated, int n_blocks, int channels, int hid, int levels) {
    const PcnnCfg c{gated, n_blocks, channels, hid, levels};
    return pcnn_cfg_ok(c) ? pcnn_plan(c, 1)->packed_floats : 0;
}
int mmvae_pixelcnn_pack_weights(int gated, int n_blocks, int channels, int hid, int levels, const float* params, long long n_params,
                                float* packed, void* s) {
    const PcnnCfg c{gated, n_blocks, channels, hid, levels};
    if (!pcnn_model_ok("pixelcnn_pack_weights", c)) return MMVAE_EINVAL;
    MMVAE_REQUIRE(params && packed, "pixelcnn_pack_weights: null argument");
    const long long want = pcnn_plan(c, 1)->param_floats;
    MMVAE_REQUIRE(n_params == want, "pixelcnn_pack_weights: %lld parameters given, the model has %lld", n_params, want);
    return guarded([&] { return launch_pcnn_pack(c, params, packed, S(s)); });
}
long long mmvae_pixelcnn_workspace_bytes(int gated, int n_blocks, int channels, int hid, int levels, int batch, int height, int width) {
    const PcnnCfg c{gated, n_blocks, channels, hid, levels};
    if (!pcnn_cfg_ok(c) || batch < 1 || height < 1 || height > PCNN_MAX_SIDE || width < 1 || width > PCNN_MAX_SIDE) return 0;
    const long long tiles = (batch + PCNN_TILE - 1) / PCNN_TILE;
    return (long long)pcnn_header_bytes() + tiles * pcnn_plan(c, width)->slab_floats * (long long)sizeof(float);
}
int mmvae_pixelcnn_sample(int gated, int n_blocks, int channels, int hid, int levels, const float* packed, void* ws, long long ws_bytes,
                          int batch, int height, int width, const float* uniforms, const int* given, int n_given, int* out_levels,
                          float* out_image, float* out_logits, void* s) {
    const PcnnCfg c{gated, n_blocks, channels, hid, levels};
    if (!pcnn_model_ok("pixelcnn_sample", c) || !pcnn_shape_ok("pixelcnn_sample", batch, height, width)) return MMVAE_EINVAL;
    MMVAE_REQUIRE(packed && ws && uniforms && out_levels && out_image, "pixelcnn_sample: null argument");
    MMVAE_REQUIRE(n_given >= 0 && n_given <= height * width, "pixelcnn_sample: n_given = %d, need 0..%d", n_given, height * width);
    MMVAE_REQUIRE(n_given == 0 || given, "pixelcnn_sample: n_given = %d without given", n_given);
    MMVAE_TRY(ws_fits("pixelcnn_sample", ws, ws_bytes, mmvae_pixelcnn_workspace_bytes(gated, n_blocks, channels, hid, levels, batch, height, width), false));
    return guarded([&] { return launch_pcnn_sample(c, packed, ws, batch, height, width, uniforms, given, n_given, out_levels, out_image, out_logits, S(s)); });
}

// ---- causal tap-list convolution for PixelCNN training (causal_conv.h)
int mmvae_causal_conv_geometry(int* pos_tile, int* channel_tile, int* wgrad_chunk, int* max_taps, int* max_offset, int* max_channels) {
    MMVAE_REQUIRE(pos_tile && channel_tile && wgrad_chunk && max_taps && max_offset && max_channels, "causal_conv_geometry: null argument");
    *pos_tile = CC_TM; *channel_tile = CC_TN; *wgrad_chunk = CC_CHUNK; *max_taps = CC_MAX_TAPS; *max_offset = CC_MAX_OFF; *max_channels = CC_MAX_CH;
    return MMVAE_OK;
}
static bool cc_sizes_ok(const CcShape& s, int n_taps) {
    return s.B >= 1 && s.H >= 1 && s.W >= 1 && (long long)s.B * s.H * s.W <= CC_MAX_POS && s.Cin >= 1 && s.Cin <= CC_MAX_CH && s.Cout >= 1 &&
           s.Cout <= CC_MAX_CH && s.kh >= 1 && s.kw >= 1 && s.kh * s.kw <= CC_MAX_CELLS && n_taps >= 1 && n_taps <= CC_MAX_TAPS;
}
long long mmvae_causal_conv_workspace_bytes(int batch, int height, int width, int cin, int cout, int kh, int kw, int n_taps) {
    const CcShape s{batch, height, width, cin, cout, kh, kw};
    return cc_sizes_ok(s, n_taps) ? (long long)cc_workspace_bytes(s, n_taps) : 0;
}
static int cc_prepare(const char* what, const CcShape& s, const int* taps, int n_taps, const void* ws, long long ws_bytes, CcTaps* t) {
    MMVAE_TRY(cc_make_taps(what, s, taps, n_taps, t));
    return ws_fits(what, ws, ws_bytes, (long long)cc_workspace_bytes(s, n_taps), false);
}
int mmvae_causal_conv_forward(const float* x, const float* weight, const float* bias, float* y, const int* taps, int n_taps, int batch,
                              int height, int width, int cin, int cout, int kh, int kw, void* ws, long long ws_bytes, void* st) {
    const CcShape s{batch, height, width, cin, cout, kh, kw};
    CcTaps t;
    MMVAE_TRY(cc_prepare("causal_conv_forward", s, taps, n_taps, ws, ws_bytes, &t));
    MMVAE_REQUIRE(x && weight && y, "causal_conv_forward: null argument");
    return guarded([&] { return launch_cc_forward(s, t, x, weight, bias, y, ws, S(st)); });
}
int mmvae_causal_conv_backward_data(const float* g, const float* weight, float* dx, const int* taps, int n_taps, int batch, int height,
                                    int width, int cin, int cout, int kh, int kw, void* ws, long long ws_bytes, void* st) {
    const CcShape s{batch, height, width, cin, cout, kh, kw};
    CcTaps t;
    MMVAE_TRY(cc_prepare("causal_conv_backward_data", s, taps, n_taps, ws, ws_bytes, &t));
    MMVAE_REQUIRE(g && weight && dx, "causal_conv_backward_data: null argument");
    return guarded([&] { return launch_cc_backward_data(s, t, g, weight, dx, ws, S(st)); });
}
int mmvae_causal_conv_backward_weight(const float* g, const float* x, float* dw, float* db, const int* taps, int n_taps, int batch, int height,
                                      int width, int cin, int cout, int kh, int kw, void* ws, long long ws_bytes, void* st) {
    const CcShape s{batch, height, width, cin, cout, kh, kw};
    CcTaps t;
    MMVAE_TRY(cc_prepare("causal_conv_backward_weight", s, taps, n_taps, ws, ws_bytes, &t));
    MMVAE_REQUIRE(g && (x || !dw), "causal_conv_backward_weight: null argument");
    return guarded([&] { return launch_cc_backward_weight(s, t, g, x, dw, db, ws, S(st)); });
}

// ---- PixelCNN output head fused with its cross entropy (head_nll.h)
int mmvae_head_nll_geometry(int* pos_tile, int* level_tile, int* chunk, int* max_hid, int* max_levels, int* max_positions) {
    MMVAE_REQUIRE(pos_tile && level_tile && chunk && max_hid && max_levels && max_positions, "head_nll_geometry: null argument");
    *pos_tile = HN_TM; *level_tile = HN_TN; *chunk = HN_CHUNK; *max_hid = HN_MAX_HID; *max_levels = HN_MAX_V; *max_positions = HN_MAX_POS;
    return MMVAE_OK;
}
long long mmvae_head_nll_workspace_bytes(int batch, int channels, int height, int width, int hid, int levels) {
    const HnShape s{batch, channels, height, width, hid, levels};
    return hn_shape_ok(s) ? (long long)hn_workspace_bytes(s) : 0;
}
static int hn_prepare(const char* what, const HnShape& s, const float* h, const void* ws, long long ws_bytes) {
    MMVAE_REQUIRE(hn_shape_ok(s), "%s: batch = %d, channels = %d, height = %d, width = %d, hid = %d, levels = %d: need batch * height * width "
                  "in 1..%d, channels 1 or 3, hid a multiple of 8 in 8..%d, levels 2..%d", what, s.B, s.C, s.H, s.W, s.hid, s.V,
                  (int)HN_MAX_POS, (int)HN_MAX_HID, (int)HN_MAX_V);
    // (h is checked between the workspace's alignment and its size, so the alignment line stays here)
    MMVAE_REQUIRE(ws && aligned16(ws), "%s: the workspace must be a 16-byte aligned device buffer", what);
    MMVAE_REQUIRE(h && aligned16(h), "%s: h must be a 16-byte aligned device buffer", what);
    return ws_fits(what, ws, ws_bytes, (long long)hn_workspace_bytes(s), false);
}
int mmvae_head_nll_forward(const float* h, const float* weight, const float* bias, const long long* target, float* nll, float* lse, int batch,
                           int channels, int height, int width, int hid, int levels, void* ws, long long ws_bytes, void* st) {
    const HnShape s{batch, channels, height, width, hid, levels};
    MMVAE_TRY(hn_prepare("head_nll_forward", s, h, ws, ws_bytes));
    MMVAE_REQUIRE(weight && bias && target && nll, "head_nll_forward: null argument");
    return guarded([&] { return launch_hn_forward(s, h, weight, bias, target, nll, lse, ws, S(st)); });
}
int mmvae_head_nll_backward(const float* h, const float* weight, const float* bias, const long long* target, const float* lse, const float* g,
                            float* dh, float* dw, float* db, int batch, int channels, int height, int width, int hid, int levels, void* ws,
                            long long ws_bytes, void* st) {
    const HnShape s{batch, channels, height, width, hid, levels};
    MMVAE_TRY(hn_prepare("head_nll_backward", s, h, ws, ws_bytes));
    MMVAE_REQUIRE(weight && bias && target && lse && g, "head_nll_backward: null argument");
    return guarded([&] { return launch_hn_backward(s, h, weight, bias, target, lse, g, dh, dw, db, ws, S(st)); });
}

// ---- 4 x 4 stride-2 convolution / transposed convolution with a fused activation (conv4s2.h)
int mmvae_conv4s2_geometry(int* pos_tile, int* channel_tile, int* wgrad_chunk, int* max_chunks, int* max_channels, int* max_side) {
    MMVAE_REQUIRE(pos_tile && channel_tile && wgrad_chunk && max_chunks && max_channels && max_side, "conv4s2_geometry: null argument");
    *pos_tile = C4_TM; *channel_tile = C4_TN; *wgrad_chunk = C4_CHUNK; *max_chunks = C4_MAX_CHUNKS; *max_channels = C4_MAX_CH; *max_side = C4_MAX_SIDE;
    return MMVAE_OK;
}
long long mmvae_conv4s2_workspace_bytes(int batch, int cs, int cl, int hs, int ws) {
    const C4Shape s{batch, cs, cl, hs, ws};
    return c4_shape_ok(s) ? (long long)c4_workspace_bytes(s) : 0;
}
static bool c4_act_ok(int act) { return act >= C4_ACT_NONE && act <= C4_ACT_SIGMOID; }
static int c4_prepare(const char* what, const C4Shape& s, const void* ws, long long ws_bytes) {
    MMVAE_REQUIRE(c4_shape_ok(s), "%s: batch = %d, Cs = %d, Cl = %d, Hs = %d, Ws = %d: need batch >= 1, channels 1..%d, even sides 2..%d and "
                  "batch * Hs * Ws <= %d", what, s.B, s.Cs, s.Cl, s.Hs, s.Ws, (int)C4_MAX_CH, (int)C4_MAX_SIDE, (int)C4_MAX_POS);
    return ws_fits(what, ws, ws_bytes, (long long)c4_workspace_bytes(s), true);
}
int mmvae_conv4s2_down(const float* src, const float* src_y, const float* weight, float* dst, int act_in, int act_out, float slope, int batch,
                       int cs, int cl, int hs, int ws_, void* ws, long long ws_bytes, void* st) {
    const C4Shape s{batch, cs, cl, hs, ws_};
    MMVAE_TRY(c4_prepare("conv4s2_down", s, ws, ws_bytes));
    MMVAE_REQUIRE(src && weight && dst, "conv4s2_down: null argument");
    MMVAE_REQUIRE(c4_act_ok(act_in) && c4_act_ok(act_out), "conv4s2_down: act_in = %d, act_out = %d, need 0..3", act_in, act_out);
    return guarded([&] { return launch_c4_down(s, src, src_y, weight, dst, act_in, act_out, slope, ws, S(st)); });
}
int mmvae_conv4s2_up(const float* src, const float* src_y, const float* weight, float* dst, int act_in, int act_out, float slope, int batch,
                     int cs, int cl, int hs, int ws_, void* ws, long long ws_bytes, void* st) {
    const C4Shape s{batch, cs, cl, hs, ws_};
    MMVAE_TRY(c4_prepare("conv4s2_up", s, ws, ws_bytes));
    MMVAE_REQUIRE(src && weight && dst, "conv4s2_up: null argument");
    MMVAE_REQUIRE(c4_act_ok(act_in) && c4_act_ok(act_out), "conv4s2_up: act_in = %d, act_out = %d, need 0..3", act_in, act_out);
    return guarded([&] { return launch_c4_up(s, src, src_y, weight, dst, act_in, act_out, slope, ws, S(st)); });
}
int mmvae_conv4s2_wgrad(const float* s_side, const float* l_side, const float* y_s, const float* y_l, int act, float slope, float* dw, int batch,
                        int cs, int cl, int hs, int ws_, void* ws, long long ws_bytes, void* st) {
    const C4Shape s{batch, cs, cl, hs, ws_};
    MMVAE_TRY(c4_prepare("conv4s2_wgrad", s, ws, ws_bytes));
    MMVAE_REQUIRE(s_side && l_side && dw, "conv4s2_wgrad: null argument");
    MMVAE_REQUIRE(c4_act_ok(act) && !(y_s && y_l), "conv4s2_wgrad: act = %d (need 0..3), and one side at most carries a gradient", act);
    return guarded([&] { return launch_c4_wgrad(s, s_side, l_side, y_s, y_l, act, slope, dw, ws, S(st)); });
}

// ---- fp32 Linear + activation layers and the MNIST InfoVAE step (infovae_mnist.h)
static int lin_prepare(const char* what, const LinShape& s, int which, const void* ws, long long ws_bytes) {
    const char* e = lin_shape_error(s);
    MMVAE_REQUIRE(e == nullptr, "%s: rows = %d, N = %d, K = %d, act = %d, perm = %d: %s", what, s.rows, s.N, s.K, s.act, s.perm, e);
    const long long need = (long long)(which == 0 ? lin_fwd_workspace_bytes(s) : lin_dgrad_workspace_bytes(s));
    return need > 0 ? ws_fits(what, ws, ws_bytes, need, true) : MMVAE_OK;
}
long long mmvae_lin_act_workspace_bytes(int rows, int n, int k, int which) {
    const LinShape s{rows, n, k, LIN_ACT_NONE, 0, 0.f};
    if (lin_shape_error(s) || which < 0 || which > 1) return 0;
    return (long long)(which == 0 ? lin_fwd_workspace_bytes(s) : lin_dgrad_workspace_bytes(s));
}
int mmvae_lin_act_fwd(const float* x, const float* w, const float* b, float* y, int rows, int n, int k, int act, float slope, int perm,
                      void* ws, long long ws_bytes, void* st) {
    const LinShape s{rows, n, k, act, perm, slope};
    MMVAE_TRY(lin_prepare("lin_act_fwd", s, 0, ws, ws_bytes));
    return guarded([&] { return launch_lin_fwd(s, x, w, b, y, ws, S(st)); });
}
int mmvae_lin_act_dgrad(const float* g, const float* y, const float* w, float* dx, int rows, int n, int k, int act, float slope, int perm,
                        void* ws, long long ws_bytes, void* st) {
    const LinShape s{rows, n, k, act, perm, slope};
    MMVAE_TRY(lin_prepare("lin_act_dgrad", s, 1, ws, ws_bytes));
    return guarded([&] { return launch_lin_dgrad(s, g, y, w, dx, ws, S(st)); });
}
int mmvae_lin_act_wgrad(const float* g, const float* y, const float* x, float* dw, float* db, int rows, int n, int k, int act, float slope,
                        int perm, void* st) {
    const LinShape s{rows, n, k, act, perm, slope};
    return guarded([&] { return launch_lin_wgrad(s, g, y, x, dw, db, S(st)); });
}
mmvae_mnist_infovae_t* mmvae_mnist_infovae_create(int n_latents, int batch) {
    try { return mnist_infovae_create(n_latents, batch); } catch (...) { mmvae_set_error("mnist_infovae_create failed"); return nullptr; }
}
void mmvae_mnist_infovae_destroy(mmvae_mnist_infovae_t* p) { mnist_infovae_destroy(p); }
long long mmvae_mnist_infovae_param_count(const mmvae_mnist_infovae_t* p) { return mnist_infovae_base(const_cast<mmvae_mnist_infovae_t*>(p))->nparams; }
int mmvae_mnist_infovae_num_params(const mmvae_mnist_infovae_t* p) { return (int)mnist_infovae_base(const_cast<mmvae_mnist_infovae_t*>(p))->params.size(); }
int mmvae_mnist_infovae_param_info(const mmvae_mnist_infovae_t* p, int i, char* name, int* ndim, int* shape, long long* offset) {
    return pb_param_info(mnist_infovae_base(const_cast<mmvae_mnist_infovae_t*>(p)), i, name, ndim, shape, offset);
}
int mmvae_mnist_infovae_bind(mmvae_mnist_infovae_t* p, float* params, float* grads) {
    return guarded([&] { return mnist_infovae_bind(p, params, grads); });
}
size_t mmvae_mnist_infovae_step_workspace_bytes(const mmvae_mnist_infovae_t* p) { return mnist_infovae_step_workspace_bytes(p); }
int mmvae_mnist_infovae_step(mmvae_mnist_infovae_t* p, const mmvae_mnist_infovae_step_io* io, int training, int do_backward, void* stream) {
    return guarded([&]() -> int {
        MMVAE_REQUIRE(p && io, "mmvae_mnist_infovae_step: null argument");
        return mnist_infovae_step(p, *io, training, do_backward, S(stream));
    });
}

// ---- MultiMNIST canvases made on the device (multimnist_gen.h, mmgen_core.h)
int mmvae_mmgen_geometry(int* side_min, int* side_max, int* max_taps, int* max_attempts, int* max_redraws, int* canvas) {
    MMVAE_REQUIRE(side_min && side_max && max_taps && max_attempts && max_redraws && canvas, "mmgen_geometry: null argument");
    *side_min = mmgen::SIDE_MIN; *side_max = mmgen::SIDE_MAX; *max_taps = mmgen::MAX_TAPS; *max_attempts = mmgen::MAX_ATTEMPTS;
    *max_redraws = mmgen::MAX_REDRAWS; *canvas = mmgen::CANVAS;
    return MMVAE_OK;
}
long long mmvae_mmgen_table_bytes() { return (long long)mmgen::TABLE_WORDS * 4; }
int mmvae_mmgen_build_tables(void* host_buf) {
    MMVAE_REQUIRE(host_buf && (reinterpret_cast<uintptr_t>(host_buf) & 3) == 0, "mmgen_build_tables: null or unaligned buffer");
    const int taps = mmgen::build_tables(static_cast<int32_t*>(host_buf));
    MMVAE_REQUIRE(taps >= 1 && taps <= mmgen::MAX_TAPS, "mmgen_build_tables: a side in %d..%d needs more than %d taps", (int)mmgen::SIDE_MIN,
                  (int)mmgen::SIDE_MAX, (int)mmgen::MAX_TAPS);
    return MMVAE_OK;
}
static int mmgen_images_ok(const char* what, const void* digits, int n_digits, const void* tables, int n, const void* u8, const void* f32) {
    MMVAE_REQUIRE(digits && tables, "%s: null argument", what);
    MMVAE_REQUIRE(u8 || f32, "%s: neither a uint8 nor a float32 image output", what);
    MMVAE_REQUIRE(n_digits >= 1, "%s: %d digits, need at least 1", what, n_digits);
    MMVAE_REQUIRE(n >= 0, "%s: n = %d", what, n);
    MMVAE_REQUIRE((reinterpret_cast<uintptr_t>(digits) & 3) == 0 && (reinterpret_cast<uintptr_t>(tables) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(u8) & 3) == 0 && aligned16(f32),
                  "%s: digits, tables and the uint8 images must be 4-byte aligned, the float32 images 16-byte aligned", what);
    return MMVAE_OK;
}
int mmvae_mmgen_generate(const unsigned char* digits, const long long* digit_labels, int n_digits, const void* tables, int flags, int min_digits,
                         int max_digits, unsigned long long seed, unsigned long long first_canvas, int n, unsigned char* images_u8,
                         float* images_f32, long long* text, int* params, int* attempts, int* fail_count, void* st) {
    MMVAE_TRY(mmgen_images_ok("mmgen_generate", digits, n_digits, tables, n, images_u8, images_f32));
    MMVAE_REQUIRE(digit_labels && text, "mmgen_generate: null argument");
    MMVAE_REQUIRE(mmgen::flags_ok(flags, min_digits, max_digits),
                  "mmgen_generate: flags = %d, min_digits = %d, max_digits = %d: need 0 <= min <= max <= %d, known flags, and "
                  "reverse / scramble / no_repeat only with fixed", flags, min_digits, max_digits, (int)mmgen::MAX_DIGITS);
    return guarded([&] {
        return launch_mmgen_generate(digits, digit_labels, n_digits, static_cast<const int32_t*>(tables), flags, min_digits, max_digits, seed,
                                     first_canvas, n, images_u8, images_f32, text, params, attempts, fail_count, S(st));
    });
}
int mmvae_mmgen_render(const unsigned char* digits, int n_digits, const void* tables, const int* params, int n, unsigned char* images_u8,
                       float* images_f32, int* overflow, void* st) {
    MMVAE_TRY(mmgen_images_ok("mmgen_render", digits, n_digits, tables, n, images_u8, images_f32));
    MMVAE_REQUIRE(params && overflow, "mmgen_render: null argument");
    return guarded([&] {
        return launch_mmgen_render(digits, n_digits, static_cast<const int32_t*>(tables), params, n, images_u8, images_f32, overflow, S(st));
    });
}

// ---- Scale + CenterCrop + ToTensor of a ragged image batch (imgprep.h, imgprep_core.h)
int mmvae_imgprep_geometry(int* max_side, int* max_out, int* precision_bits) {
    MMVAE_REQUIRE(max_side && max_out && precision_bits, "imgprep_geometry: null argument");
    *max_side = imgprep::MAX_SIDE; *max_out = imgprep::MAX_OUT; *precision_bits = imgprep::PRECISION_BITS;
    return MMVAE_OK;
}
int mmvae_imgprep_layout(int h, int w, int S, int* ow, int* oh, int* x1, int* y1) {
    MMVAE_REQUIRE(ow && oh && x1 && y1, "imgprep_layout: null argument");
    MMVAE_REQUIRE(imgprep::sides_ok(h, w) && S >= 1 && S <= imgprep::MAX_OUT, "imgprep_layout: h = %d, w = %d (need 1..%d), S = %d (need 1..%d)", h, w,
                  (int)imgprep::MAX_SIDE, S, (int)imgprep::MAX_OUT);
    imgprep::scaled_size(w, h, S, ow, oh);
    *x1 = imgprep::crop_offset(*ow - S); *y1 = imgprep::crop_offset(*oh - S);
    return MMVAE_OK;
}
int mmvae_imgprep_coeffs(int n_in, int n_out, int first, int count, int stride, int* xmin, int* taps, int* coefs) {
    MMVAE_REQUIRE(xmin && taps && coefs, "imgprep_coeffs: null argument");
    MMVAE_REQUIRE(n_in >= 1 && n_in <= imgprep::MAX_SIDE && n_out >= 1 && first >= 0 && count >= 0 && first <= n_out - count && stride >= 1,
                  "imgprep_coeffs: n_in = %d (need 1..%d), n_out = %d, indices %d .. %d + %d, stride %d", n_in, (int)imgprep::MAX_SIDE, n_out, first,
                  first, count, stride);
    for (int j = 0; j < count; ++j) {
        const imgprep::Span sp = imgprep::span_of(n_in, n_out, first + j);
        MMVAE_REQUIRE(sp.n <= stride, "imgprep_coeffs: index %d has %d taps, the rows hold %d", first + j, sp.n, stride);
        xmin[j] = sp.xmin; taps[j] = sp.n;
        for (int t = 0; t < stride; ++t)
            coefs[(long long)j * stride + t] = t < sp.n ? imgprep::coef_at(n_in, n_out, first + j, sp.xmin, sp.ww, t) : 0;
    }
    return MMVAE_OK;
}
int mmvae_imgprep_scale_crop(const unsigned char* pixels, long long pixels_bytes, const long long* offsets, const int* heights, const int* widths,
                             int n, int side, unsigned char* out_u8, float* out_f32, int* status, void* st) {
    MMVAE_REQUIRE(pixels && offsets && heights && widths && status, "imgprep_scale_crop: null argument");
    MMVAE_REQUIRE(out_u8 || out_f32, "imgprep_scale_crop: neither a uint8 nor a float32 image output");
    MMVAE_REQUIRE(n >= 0 && pixels_bytes >= 0, "imgprep_scale_crop: n = %d, pixels_bytes = %lld", n, pixels_bytes);
    MMVAE_REQUIRE(side >= 1 && side <= imgprep::MAX_OUT, "imgprep_scale_crop: S = %d, need 1..%d", side, (int)imgprep::MAX_OUT);
    MMVAE_REQUIRE((reinterpret_cast<uintptr_t>(offsets) & 7) == 0 && (reinterpret_cast<uintptr_t>(heights) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(widths) & 3) == 0 && (reinterpret_cast<uintptr_t>(status) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(out_f32) & 3) == 0,
                  "imgprep_scale_crop: offsets must be 8-byte aligned, heights, widths, status and the float32 images 4-byte aligned");
    return guarded([&] { return launch_imgprep_scale_crop(pixels, pixels_bytes, offsets, heights, widths, n, side, out_u8, out_f32, status, S(st)); });
}

// ---- exact t-SNE with a 2-component embedding (tsne.h)
static bool tsne_n_ok(const char* what, int n) {
    if (n < TSNE_MIN_N || n > TSNE_MAX_N) {
        mmvae_set_error("%s: n = %d, need %d..%d", what, n, (int)TSNE_MIN_N, (int)TSNE_MAX_N);
        return false;
    }
    return true;
}
static int tsne_ws_ok(const char* what, int n, const void* ws, long long ws_bytes) {
    MMVAE_REQUIRE(ws, "%s: null argument", what);      // (this op's wording for a null workspace)
    return ws_fits(what, ws, ws_bytes, (long long)tsne_workspace_bytes(n), false);
}
int mmvae_tsne_geometry(int* row_tile, int* col_tile, int* sym_tile, int* row_threads, int* max_dim) {
    MMVAE_REQUIRE(row_tile && col_tile && sym_tile && row_threads && max_dim, "tsne_geometry: null argument");
    *row_tile = TSNE_RT; *col_tile = TSNE_CT; *sym_tile = TSNE_ST; *row_threads = TSNE_AT; *max_dim = TSNE_MAX_DIM;
    return MMVAE_OK;
}
long long mmvae_tsne_workspace_bytes(int n) {
    if (n < TSNE_MIN_N || n > TSNE_MAX_N) return 0;
    return (long long)tsne_workspace_bytes(n);
}
int mmvae_tsne_affinities(const float* x, int n, int dim, float perplexity, float* P, float* beta, float* out2, void* ws, long long ws_bytes,
                          void* s) {
    MMVAE_REQUIRE(x && P && beta && out2, "tsne_affinities: null argument");
    if (!tsne_n_ok("tsne_affinities", n)) return MMVAE_EINVAL;
    MMVAE_REQUIRE(dim >= 1 && dim <= TSNE_MAX_DIM, "tsne_affinities: dim = %d, need 1..%d", dim, (int)TSNE_MAX_DIM);
    MMVAE_REQUIRE(perplexity >= 1.f && perplexity < (float)(n - 1), "tsne_affinities: perplexity = %g, need 1 <= perplexity < n - 1 = %d",
                  (double)perplexity, n - 1);
    MMVAE_TRY(tsne_ws_ok("tsne_affinities", n, ws, ws_bytes));
    return guarded([&] { return launch_tsne_affinities(x, n, dim, perplexity, P, beta, out2, ws, S(s)); });
}
int mmvae_tsne_grad(const float* P, float exaggeration, const float* y, int n, void* ws, long long ws_bytes, float* grad, float* out3, void* s) {
    MMVAE_REQUIRE(P && y && grad && out3, "tsne_grad: null argument");
    if (!tsne_n_ok("tsne_grad", n)) return MMVAE_EINVAL;
    MMVAE_REQUIRE(exaggeration > 0.f && exaggeration <= 3.0e38f, "tsne_grad: exaggeration = %g, need a positive finite number", (double)exaggeration);
    MMVAE_TRY(tsne_ws_ok("tsne_grad", n, ws, ws_bytes));
    return guarded([&] { return launch_tsne_grad(P, exaggeration, y, n, ws, grad, out3, S(s)); });
}
int mmvae_tsne_run(const float* P, int n, float* y, float* update, float* gains, int first_iter, int n_iter, float learning_rate,
                   float early_exaggeration, int exaggeration_iters, float* kl_trace, void* ws, long long ws_bytes, void* s) {
    MMVAE_REQUIRE(P && y && update && gains && kl_trace, "tsne_run: null argument");
    if (!tsne_n_ok("tsne_run", n)) return MMVAE_EINVAL;
    MMVAE_REQUIRE(first_iter >= 0 && n_iter >= 1 && n_iter <= 1000000, "tsne_run: first_iter = %d, n_iter = %d, need first_iter >= 0, n_iter 1..1000000",
                  first_iter, n_iter);
    MMVAE_REQUIRE(learning_rate > 0.f && learning_rate <= 3.0e38f && early_exaggeration > 0.f && early_exaggeration <= 3.0e38f,
                  "tsne_run: learning_rate = %g, early_exaggeration = %g, need positive finite numbers", (double)learning_rate,
                  (double)early_exaggeration);
    MMVAE_TRY(tsne_ws_ok("tsne_run", n, ws, ws_bytes));
    return guarded([&] {
        return launch_tsne_run(P, n, y, update, gains, first_iter, n_iter, learning_rate, early_exaggeration, exaggeration_iters, kl_trace, ws, S(s));
    });
}
