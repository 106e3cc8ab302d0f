// CelebA MMVAE (celeba/model.py:14-57,91-196 ; celeba/train.py:60-81,131-147) on the shared gather-GEMM / BatchNorm /
// thin-layer kernels.  3x64x64 images, 5x5x256 bottleneck, fc 6400 <-> 1024, 18 binary attributes through
// Linear -> BatchNorm1d -> Swish MLPs, sigmoid + BCE on both modalities.
//
// Passes (celeba/train.py:138-147): (image,attrs), (image), (attrs), every lambda 1, kl_lambda 1e-3.  Image-encoder
// convolutions run once for passes 1 and 2 (classifier twice: independent Dropout masks), the attribute encoder once
// for passes 1 and 3 (no dropout: identical), decoders on 3B rows with BatchNorm statistics per pass.
#include "celeba.h"
#include "img_tower.h"
#include <cstring>

namespace {
constexpr int IMG = 64, NPIX = 3 * IMG * IMG, NA = 18, NA_LD = 24, FEAT = 6400, HID = 1024;
}

struct CelebaPlan : TowerPlan {      // image half: img_tower.h
    MlpLin fc2, ae[2], ad[2];
    BnL abn[2];                      // attrs_encoder.net.1, attrs_decoder.net.1
    struct W : TowerW {
        char* zero_begin; size_t zero_bytes;
        float2 *st_a[2], *red_a[2];
        float* sums; float* dz_img; float* dz_att;
        float2 *aff_a[2], *mr_a[2];
        float* encout; uint8_t* m1;
        bf16 *att_bf, *r_ae, *a_ae; float* attout;
        float *eps, *mu, *logvar, *z_f32;
        bf16 *r_ad, *a_ad; float *alogits, *arecon, *dalogit; bf16* dalogit_bf;
        bf16 *d_ad;
        bf16 *d_encout, *d_attout_bf, *d_ae;
        float* tmp_f32;
    } w;
    CelebaPlan() { tw = &w; }
};

namespace {

BnTabs atabs(CelebaPlan& P, int i) { CelebaPlan::W& w = P.w; return BnTabs{w.st_a[i], w.red_a[i], w.aff_a[i], w.mr_a[i]}; }

void build(CelebaPlan& P) {
    const int D = P.D;
    auto lin = [&](const std::string& n, int o, int i) { add_param(P, n + ".weight", {o, i}); add_param(P, n + ".bias", {o}); };
    auto bnp = [&](const std::string& n, int c) { add_param(P, n + ".weight", {c}); add_param(P, n + ".bias", {c}); };
    add_param(P, "image_encoder.features.0.weight", {32, 3, 4, 4});
    add_param(P, "image_encoder.features.2.weight", {64, 32, 4, 4}); bnp("image_encoder.features.3", 64);
    add_param(P, "image_encoder.features.5.weight", {128, 64, 4, 4}); bnp("image_encoder.features.6", 128);
    add_param(P, "image_encoder.features.8.weight", {256, 128, 4, 4}); bnp("image_encoder.features.9", 256);
    lin("image_encoder.classifier.0", HID, FEAT);
    lin("image_encoder.classifier.3", 2 * D, HID);
    lin("image_decoder.upsample.0", FEAT, D);
    add_param(P, "image_decoder.hallucinate.0.weight", {256, 128, 4, 4}); bnp("image_decoder.hallucinate.1", 128);
    add_param(P, "image_decoder.hallucinate.3.weight", {128, 64, 4, 4}); bnp("image_decoder.hallucinate.4", 64);
    add_param(P, "image_decoder.hallucinate.6.weight", {64, 32, 4, 4}); bnp("image_decoder.hallucinate.7", 32);
    add_param(P, "image_decoder.hallucinate.9.weight", {32, 3, 4, 4});
    lin("attrs_encoder.net.0", 64, NA); bnp("attrs_encoder.net.1", 64); lin("attrs_encoder.net.3", 2 * D, 64);
    lin("attrs_decoder.net.0", 64, D); bnp("attrs_decoder.net.1", 64); lin("attrs_decoder.net.3", NA, 64);

    // image encoder (celeba/model.py:100-112), image decoder (celeba/model.py:140-151)
    const ConvGeom enc[4] = {ConvGeom{3, 32, 4, 4, 2, 1, 64, 64, 32, 32, false}, ConvGeom{32, 64, 4, 4, 2, 1, 32, 32, 16, 16, false},
                             ConvGeom{64, 128, 4, 4, 2, 1, 16, 16, 8, 8, false}, ConvGeom{128, 256, 4, 4, 1, 0, 8, 8, 5, 5, false}};
    const ConvGeom dec[4] = {ConvGeom{256, 128, 4, 4, 1, 0, 5, 5, 8, 8, true}, ConvGeom{128, 64, 4, 4, 2, 1, 8, 8, 16, 16, true},
                             ConvGeom{64, 32, 4, 4, 2, 1, 16, 16, 32, 32, true}, ConvGeom{32, 3, 4, 4, 2, 1, 32, 32, 64, 64, true}};
    P.geo = TowerGeom{IMG, 32, 32, 5, 256, FEAT, HID};
    long long so = tower_build_convs(P, enc, dec);
    const char* abnn[2] = {"attrs_encoder.net.1", "attrs_decoder.net.1"};
    for (int i = 0; i < 2; ++i) {
        P.abn[i] = BnL{off(P, std::string(abnn[i]) + ".weight"), off(P, std::string(abnn[i]) + ".bias"), 64, so, 6 + i};
        P.bn_names.push_back(abnn[i]); P.bn_list.push_back(P.abn[i]);
        so += 2 * 64;
    }
    add_frag_packs(P, P.conv[2]);      // 8x8 / 16x16 layers: direct-B image-resident kernels (convres.hip)
    add_frag_packs(P, P.convT[1]);
    tower_build_fc1(P);
    mlp_lin_init(P, P.fc2, "image_encoder.classifier.3", 2 * D, HID, -1, true);
    tower_build_up(P);
    mlp_lin_init(P, P.ae[0], "attrs_encoder.net.0", 64, NA, 6, false);
    mlp_lin_init(P, P.ae[1], "attrs_encoder.net.3", 2 * D, 64, -1, true);
    mlp_lin_init(P, P.ad[0], "attrs_decoder.net.0", 64, D, 7, true, P.ldz);     // operand is z_bf
    mlp_lin_init(P, P.ad[1], "attrs_decoder.net.3", NA, 64, -1, true);
}

void carve(CelebaPlan& P, Workspace& ws) {
    CelebaPlan::W& w = P.w;
    const size_t B = P.B, D = P.D, B3 = (size_t)P.carve_passes * B, B2 = (size_t)(P.carve_passes < 2 ? P.carve_passes : 2) * B;
    const int SS = MMVAE_STAT_SLOTS;
    const int ec[3] = {64, 128, 256}, dc[3] = {128, 64, 32};
    char* z0 = ws.take<char>(0);
    for (int i = 0; i < 3; ++i) { w.st_e[i] = ws.take<float2>(SS * ec[i]); w.red_e[i] = ws.take<float2>(SS * ec[i]); }
    for (int i = 0; i < 3; ++i) { w.st_d[i] = ws.take<float2>(3 * SS * dc[i]); w.red_d[i] = ws.take<float2>(3 * SS * dc[i]); }
    for (int i = 0; i < 2; ++i) { w.st_a[i] = ws.take<float2>(3 * SS * 64); w.red_a[i] = ws.take<float2>(3 * SS * 64); }
    w.sums = ws.take<float>(16 * MMVAE_LOSS_SLOTS);
    P.sk_cnt = ws.take<unsigned>(1024);
    w.dz_img = ws.take<float>(B3 * D); w.dz_att = ws.take<float>(B3 * D);
    char* z1 = ws.take<char>(0);
    w.zero_begin = z0; w.zero_bytes = (size_t)(z1 - z0);
    for (int i = 0; i < 3; ++i) { w.aff_e[i] = ws.take<float2>(ec[i]); w.mr_e[i] = ws.take<float2>(ec[i]); }
    for (int i = 0; i < 3; ++i) { w.aff_d[i] = ws.take<float2>(3 * dc[i]); w.mr_d[i] = ws.take<float2>(3 * dc[i]); }
    for (int i = 0; i < 2; ++i) { w.aff_a[i] = ws.take<float2>(3 * 64); w.mr_a[i] = ws.take<float2>(3 * 64); }
    w.patches1 = ws.take<bf16>(B * 1024 * 48);
    w.r1 = ws.take<bf16>(B * 1024 * 32); w.r2 = ws.take<bf16>(B * 256 * 64); w.r3 = ws.take<bf16>(B * 64 * 128); w.r4 = ws.take<bf16>(B * FEAT);
    w.a1 = ws.take<bf16>(B * 1024 * 32); w.a2 = ws.take<bf16>(B * 256 * 64); w.a3 = ws.take<bf16>(B * 64 * 128); w.a4 = ws.take<bf16>(B * FEAT);
    w.y1 = ws.take<bf16>(B2 * HID); w.ay1 = ws.take<bf16>(B2 * HID);
    w.encout = ws.take<float>(B2 * 2 * D); w.m1 = ws.take<uint8_t>(B2 * HID);
    w.att_bf = ws.take<bf16>(B * NA_LD); w.r_ae = ws.take<bf16>(B * 64); w.a_ae = ws.take<bf16>(B * 64); w.attout = ws.take<float>(B * 2 * D);
    w.eps = ws.take<float>(B3 * D); w.mu = ws.take<float>(B3 * D); w.logvar = ws.take<float>(B3 * D);
    w.z_f32 = ws.take<float>(B3 * D); w.z_bf = ws.take<bf16>(B3 * P.ldz);
    w.u = ws.take<bf16>(B3 * FEAT); w.au = ws.take<bf16>(B3 * FEAT);
    w.q1 = ws.take<bf16>(B3 * 64 * 128); w.q2 = ws.take<bf16>(B3 * 256 * 64); w.q3 = ws.take<bf16>(B3 * 1024 * 32);
    w.aq1 = ws.take<bf16>(B3 * 64 * 128); w.aq2 = ws.take<bf16>(B3 * 256 * 64); w.aq3 = ws.take<bf16>(B3 * 1024 * 32);
    w.dlogit = ws.take<float>(B3 * NPIX);
    w.r_ad = ws.take<bf16>(B3 * 64); w.a_ad = ws.take<bf16>(B3 * 64);
    w.alogits = ws.take<float>(B3 * NA); w.arecon = ws.take<float>(B3 * NA); w.dalogit = ws.take<float>(B3 * NA);
    w.dalogit_bf = ws.take<bf16>(B3 * NA_LD);
    w.patches4 = ws.take<bf16>(B3 * 1024 * 48);
    w.d3 = ws.take<bf16>(B3 * 1024 * 32); w.d2 = ws.take<bf16>(B3 * 256 * 64); w.d1 = ws.take<bf16>(B3 * 64 * 128);
    w.du = ws.take<bf16>(B3 * FEAT); w.d_ad = ws.take<bf16>(B3 * 64);
    w.d_encout = ws.take<bf16>(B2 * 2 * D); w.d_attout_bf = ws.take<bf16>(B * 2 * D); w.d_ae = ws.take<bf16>(B * 64);
    w.dy1 = ws.take<bf16>(B2 * HID); w.db4 = ws.take<bf16>(B2 * FEAT); w.dr4 = ws.take<bf16>(B * FEAT);
    w.d3e = ws.take<bf16>(B * 64 * 128); w.d2e = ws.take<bf16>(B * 256 * 64); w.d1e = ws.take<bf16>(B * 1024 * 32);
    w.tmp_f32 = ws.take<float>(B3 * NPIX);
    P.sk_floats = (size_t)256 * 128 * 128;
    P.sk_buf = ws.take<float>(P.sk_floats);
    // weight-gradient partial-tile slabs (written and read once per step, never zeroed): gemm.h WgradSlabCtx
    w.slab_floats = (size_t)(P.carve_passes >= 3 ? 48 : 16) << 20;
    w.slab = ws.take<float>(w.slab_floats);
}

// zero-padded bf16 copy of fp32 rows: out[r][0..ld) = (x[r][0..cols), 0...)
__global__ void cast_pad_kernel(const float* x, int rows, int cols, bf16* out, int ld) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * ld) return;
    const int r = i / ld, c = i - r * ld;
    out[i] = (bf16)(c < cols ? x[(size_t)r * cols + c] : 0.f);
}
int cast_pad(const float* x, int rows, int cols, bf16* out, int ld, hipStream_t s) {
    hipLaunchKernelGGL(cast_pad_kernel, dim3(ceil_div(rows * ld, 256)), dim3(256), 0, s, x, rows, cols, out, ld);
    return mmvae_check_launch("cast_pad");
}

// ================================================================== image encoder (celeba/model.py:124-128)
// The launches of the conv chain, classifier.0 and the decoder body are the tower's (img_tower.h: tower_gemm / tower_wgrad and
// the passes around them); `fuse` is the tower's: the fused step at B % 4 == 0.
// classifier.3, input gradient: d_out [n*B][2D]; mask: keep flags of the classifier Dropout or null
GemmParams fc2_dgrad_gemm(CelebaPlan& P, int n, const uint8_t* mask, const bf16* d_out) {
    CelebaPlan::W& w = P.w;
    const int rows = n * P.B;
    GatherPlan pd = dense_plan(rows, P.fc2.ldo, P.fc2.ldo, HID);
    GemmParams d = gemm_of(P, pd, &P.fc2.pk_dgrad, 1, rows);
    d.c.A = d_out; d.out_bf = w.dy1; d.ldo = HID;
    d.d_r = w.y1; d.d_ld = HID; d.d_act = ACT_SWISH; if (mask) { d.d_mask = mask; d.d_mask_scale = 1.f / (1.f - DROP_P); }
    d.d_colsum = P.buf.grads + P.fc1.b_off;
    return d;
}

int enc_fwd(CelebaPlan& P, const float* image, int variants, const uint8_t* m1, int dropout, int training, int bn_updates,
            float* out, hipStream_t s, bool fuse = false) {
    MMVAE_TRY(tower_enc_fwd(P, image, training, bn_updates, s, fuse));
    const bool drop = training && dropout;
    MMVAE_TRY(launch_gemm_gather(tower_gemm(P, TW_FC1, 0, variants, training, drop ? m1 : nullptr), s));
    return mlp_fwd(P, P.fc2, P.w.ay1, variants * P.B, 1, nullptr, out, nullptr, s);
}

// d_out: bf16 [variants*B][2D]; the bias gradient of classifier.3 must already be accumulated by the caller
int enc_bwd(CelebaPlan& P, const bf16* d_out, int variants, const uint8_t* m1, int dropout, hipStream_t s, bool fuse = false) {
    // classifier.3
    MMVAE_TRY(mlp_wgrad(P, P.fc2, d_out, P.w.ay1, variants * P.B, s));
    MMVAE_TRY(launch_gemm_gather(fc2_dgrad_gemm(P, variants, dropout ? m1 : nullptr, d_out), s));
    // classifier.0: wgrad gathers the shared 5x5x256 map; the input gradient is one dense GEMM over NHWC columns
    MMVAE_TRY(wgrad_async(P, tower_wgrad(P, TW_W_FC1, 0, variants), s));
    MMVAE_TRY(launch_gemm_gather(tower_gemm(P, TW_FC1_DGRAD, 0, variants), s));
    return tower_enc_bwd(P, variants, s, fuse);
}

// ================================================================== image decoder (celeba/model.py:157-161)
// fused_bwd_groups >= 0 (the fused step): BatchNorm + Swish of hallucinate.7, the last ConvTranspose2d, sigmoid + BCE and -- for
// the first fused_bwd_groups passes -- its input / weight gradients in ONE kernel per image (dec_last.hip dec_last_ca_kernel);
// last_groups: passes whose last layer is computed at all
// last == nullptr (celeba_iw_score): the body only -- it ends with the raw output of hallucinate.6 in q3, whose BatchNorm + Swish
// belong to the caller's own tail
int dec_fwd(CelebaPlan& P, int groups, int training, ConvTLastFwdArgs* last, hipStream_t s, int last_groups = -1, int fused_bwd_groups = -1,
            bool fuse = false) {
    CelebaPlan::W& w = P.w;
    const int B = P.B;
    MMVAE_TRY(tower_dec_fwd(P, groups, training, last && fused_bwd_groups < 0, s, fuse));
    if (!last) return MMVAE_OK;
    if (fused_bwd_groups < 0) return launch_convt_last_fwd(dec_last_args(P, *last, groups), s);
    const ConvL& L = P.convT[2];
    const BnL& b = P.bn[L.bn];
    DecLastFusedArgs x{};
    x.r = w.q3; x.act = ACT_SWISH; x.w = P.buf.params + P.convT[3].w_off;
    x.G = last_groups > 0 ? last_groups : groups; x.B = B; x.IH = 32; x.IW = 32; x.Cin = 32; x.Cout = 3;
    x.bwd_groups = std::min(fused_bwd_groups, x.G);
    x.fin = bn_fin_args(P, b, B * L.g.OH * L.g.OW, groups, w.st_d[2], 1, w.aff_d[2], w.mr_d[2], training);
    x.target = last->target; x.logits = last->logits; x.recon = last->recon; x.dlogit = nullptr;
    for (int k = 0; k < 4; ++k) x.coef[k] = last->coef[k];
    x.loss_sum = last->loss_sum;
    if (x.bwd_groups > 0) {
        const int chunks = x.bwd_groups * B;
        x.wslab = P.slab.take((size_t)chunks * 32 * 48);
        MMVAE_REQUIRE(x.wslab != nullptr, "fused decoder tail: the weight-gradient slab pool is exhausted");
        x.db = w.d3; x.red = w.red_d[2];
        WgradSlabJob j{};
        const PackDesc& gd = P.gk.d[P.convT[3].gk[0]];
        j.dst = P.buf.gpk + gd.dst_off; j.slab = x.wslab; j.N = 32; j.K = 48; j.Kpad = gd.Kpad; j.chunks = chunks;
        j.chunk_stride = 32 * 48; j.src_ld = 48;
        j.stream = s;            // (dec_bwd moves the sum behind its first weight gradient, off the main chain)
        P.slab.jobs.push_back(j);
    }
    return launch_dec_last_ca(x, s);
}

// dlogit: fp32 NCHW [groups*B][3][64][64] (grad wrt the pre-sigmoid logits). Writes dz (fp32 [groups*B][D]).
int dec_bwd(CelebaPlan& P, const float* dlogit, int groups, float* dz, hipStream_t s, bool last_fused = false, bool fuse = false) {
    if (last_fused && P.wgrad_forked && !mmvae_serial()) {
        // d3, the BatchNorm-backward sums and the per-image weight-gradient partials of the last layer came out of the fused tail
        // (dec_fwd); the sum of the partials goes behind the first weight gradient below, on its side stream (wgrad_async)
        hipStream_t wst = (P.wgrad_rr & 1) ? P.st_wgrad2 : P.st_wgrad;
        for (WgradSlabJob& j : P.slab.jobs) if (j.stream == s && j.src_ld == 48) j.stream = wst;
    }
    return tower_dec_bwd(P, dlogit, groups, dz, s, last_fused, fuse);
}


// ================================================================== attribute MLPs (celeba/model.py:164-196)
int att_enc_fwd(CelebaPlan& P, const float* attrs, int training, int updates, float* out, hipStream_t s) {
    CelebaPlan::W& w = P.w;
    const int B = P.B;
    MMVAE_TRY(cast_pad(attrs, B, NA, w.att_bf, NA_LD, s));
    MMVAE_TRY(mlp_fwd(P, P.ae[0], w.att_bf, B, 1, w.r_ae, nullptr, training ? w.st_a[0] : nullptr, s));
    MMVAE_TRY(bn1d_act(P, P.abn[0], atabs(P, 0), w.r_ae, w.a_ae, B, 1, 64, updates, training, ACT_SWISH, s));
    return mlp_fwd(P, P.ae[1], w.a_ae, B, 1, nullptr, out, nullptr, s);
}
// d_out_bf: bf16 [B][2D]; the bias gradient of net.3 must already be accumulated by the caller
int att_enc_bwd(CelebaPlan& P, const bf16* d_out_bf, hipStream_t s) {
    CelebaPlan::W& w = P.w;
    const int B = P.B;
    BnTabs t = atabs(P, 0);
    MMVAE_TRY(mlp_wgrad(P, P.ae[1], d_out_bf, w.a_ae, B, s));
    MMVAE_TRY(mlp_dgrad(P, P.ae[1], d_out_bf, B, 1, w.d_ae, nullptr, 64, w.r_ae, &t, ACT_SWISH, s));
    MMVAE_TRY(bn1d_bwd(P, P.abn[0], t, w.d_ae, w.r_ae, B, 1, 64, s));
    return mlp_wgrad(P, P.ae[0], w.d_ae, w.att_bf, B, s);
}
int att_dec_fwd(CelebaPlan& P, int groups, int training, float* logits, hipStream_t s) {
    CelebaPlan::W& w = P.w;
    const int rows = groups * P.B;
    MMVAE_TRY(mlp_fwd(P, P.ad[0], w.z_bf, rows, groups, w.r_ad, nullptr, training ? w.st_a[1] : nullptr, s));
    MMVAE_TRY(bn1d_act(P, P.abn[1], atabs(P, 1), w.r_ad, w.a_ad, rows, groups, 64, 1, training, ACT_SWISH, s));
    return mlp_fwd(P, P.ad[1], w.a_ad, rows, 1, nullptr, logits, nullptr, s);
}
// dalogit: fp32 [groups*B][18]
int att_dec_bwd(CelebaPlan& P, const float* dalogit, int groups, float* dz, hipStream_t s) {
    CelebaPlan::W& w = P.w;
    const int rows = groups * P.B;
    BnTabs t = atabs(P, 1);
    MMVAE_TRY(cast_pad(dalogit, rows, NA, w.dalogit_bf, NA_LD, s));
    MMVAE_TRY(launch_colsum_f32(dalogit, rows, NA, P.buf.grads + P.ad[1].b_off, s));
    MMVAE_TRY(mlp_wgrad(P, P.ad[1], w.dalogit_bf, w.a_ad, rows, s));
    MMVAE_TRY(mlp_dgrad(P, P.ad[1], w.dalogit_bf, rows, groups, w.d_ad, nullptr, 64, w.r_ad, &t, ACT_SWISH, s));
    MMVAE_TRY(bn1d_bwd(P, P.abn[1], t, w.d_ad, w.r_ad, rows, groups, 64, s));
    MMVAE_TRY(mlp_wgrad(P, P.ad[0], w.d_ad, w.z_bf, rows, s));
    return mlp_dgrad(P, P.ad[0], w.d_ad, rows, 1, nullptr, dz, P.D, nullptr, nullptr, 0, s);
}

int use_ws(CelebaPlan* P, void* ws, size_t bytes, bool module = true) {
    MMVAE_TRY(plan_use_ws(P, ws, bytes, module, carve));
    P->wgrad_forked = false;
    return MMVAE_OK;
}

}  // namespace

CelebaPlan* celeba_create(int D, int B) {
    if (D < 4 || D > 124 || D % 4 != 0 || B < 1) { mmvae_set_error("celeba_create: need n_latents in 4..124, a multiple of 4, and batch >= 1"); return nullptr; }
    CelebaPlan* P = new CelebaPlan();
    P->D = D; P->B = B;
    build(*P);
    plan_size_workspaces(*P, carve);
    return P;
}
void celeba_destroy(CelebaPlan* P) { delete P; }
PlanBase* celeba_base(CelebaPlan* P) { return P; }

static int celeba_step_body(CelebaPlan* Pp, const mmvae_celeba_step_io& io, int training, int do_backward, hipStream_t s);
int celeba_step(CelebaPlan* Pp, const mmvae_celeba_step_io& io, int training, int do_backward, hipStream_t s) {
    return plan_step(Pp, io, training, do_backward, s, celeba_step_body);
}
static int celeba_step_body(CelebaPlan* Pp, const mmvae_celeba_step_io& io, int training, int do_backward, hipStream_t s) {
    MMVAE_TRY(use_ws(Pp, io.ws, io.ws_bytes, false));
    CelebaPlan& P = *Pp;
    CelebaPlan::W& w = P.w;
    const int B = P.B, D = P.D, B3 = 3 * B;
    MMVAE_REQUIRE(io.image && io.attrs && io.sums, "celeba step: image/attrs/sums must be given");
    const float* eps = io.eps;
    const uint8_t* m1 = io.enc_mask;
    StepBeginArgs sb{};
    sb.zero_ptr[0] = w.zero_begin; sb.zero_bytes[0] = w.zero_bytes;
    if (do_backward) {
        sb.zero_ptr[1] = P.buf.gpk; sb.zero_bytes[1] = (size_t)P.gk.mat_elems * sizeof(float);
        sb.zero_ptr[2] = P.buf.grads; sb.zero_bytes[2] = (size_t)(P.nparams / 4) * 16;
    }
    sb.p = DROP_P; sb.seed = io.seed; sb.step = io.step_counter;
    if (training && !eps) { sb.eps = w.eps; sb.n_eps = (long long)B3 * D; eps = w.eps; }
    if (training && io.enc_dropout && !m1) { sb.mask[0] = w.m1; sb.n_mask[0] = (long long)2 * B * HID; m1 = w.m1; }
    MMVAE_TRY(launch_step_begin(sb, s));
    if (do_backward && P.nparams % 4 != 0)
        MMVAE_TRY(launch_fill_zero(P.buf.grads + (P.nparams / 4) * 4, (size_t)(P.nparams % 4) * sizeof(float), s));
    const int enc_drop = training && io.enc_dropout;
    const int sk[3] = {io.pass_skip[0] != 0, io.pass_skip[1] != 0, io.pass_skip[2] != 0};
    P.dec_skip_mask = (unsigned)(sk[0] | (sk[1] << 1) | (sk[2] << 2));
    MMVAE_TRY(ensure_streams(P));
    const bool serial = mmvae_serial();
    hipStream_t T = serial ? s : P.st_text;
    // ---- encoders: attribute MLP on the side stream, image encoder on main
    MMVAE_TRY(edge(P, s, T));
    P.no_splitk = !serial;
    MMVAE_TRY(att_enc_fwd(P, io.attrs, training, 2 - sk[0] - sk[2], w.attout, T));
    P.no_splitk = false;
    // BatchNorm passes folded into the staging of the image-resident conv kernels (convres.hip; their tiles hold 4 / 2 images)
    const bool fuse = mmvae_knob(K_ca_fuse_bn) && mmvae_knob(K_convres) && mmvae_knob(K_convres_celeba) && B % 4 == 0;
    MMVAE_TRY(enc_fwd(P, io.image, 2, m1, enc_drop, training, 2 - sk[0] - sk[1], w.encout, s, fuse));
    MMVAE_TRY(edge(P, T, s));
    Latent3Args la{};
    la.B = B; la.D = D; la.img_out = w.encout; la.txt_out = w.attout; la.eps = eps;
    la.mu = io.mu ? io.mu : w.mu; la.logvar = io.logvar ? io.logvar : w.logvar;
    la.z_f32 = w.z_f32; la.z_bf = w.z_bf; la.ldz = P.ldz; la.kl_sum = w.sums + 8; la.training = training;
    MMVAE_TRY(launch_latent3_fwd(la, s));
    // ---- attribute decoder (+ BCE, + its backward) on the side stream, image decoder on main
    MMVAE_TRY(edge(P, s, T));
    P.no_splitk = !serial;
    MMVAE_TRY(att_dec_fwd(P, 3, training, w.alogits, T));
    {
        BceArgs bc{};
        bc.logits = w.alogits; bc.ldl = NA; bc.target = io.attrs; bc.G = 3; bc.B = B; bc.C = NA; bc.H = 1; bc.W = 1;
        bc.recon = io.recon_attrs ? io.recon_attrs : w.arecon; bc.dlogit = do_backward ? w.dalogit : nullptr; bc.loss_sum = w.sums + 4;
        // celeba/train.py:69-73: mean over the batch per attribute, averaged over the 18 attributes
        for (int k = 0; k < 3; ++k) bc.coef[k] = sk[k] ? 0.f : io.lambda_y[k] / (float)(B * NA);
        MMVAE_TRY(launch_sigmoid_bce(bc, T));
    }
    if (do_backward) {
        P.wgrad_forked = false;      // the side stream runs its own weight gradients in order
        MMVAE_TRY(att_dec_bwd(P, w.dalogit, 3, w.dz_att, T));
    }
    P.no_splitk = false;
    ConvTLastFwdArgs last{};
    last.target = io.image; last.recon = io.recon_image; last.dlogit = do_backward ? w.dlogit : nullptr; last.loss_sum = w.sums;
    for (int k = 0; k < 3; ++k) last.coef[k] = sk[k] ? 0.f : io.lambda_x[k] / (float)(B * NPIX);
    int img_groups = 3;         // passes whose image term has a gradient (a pass with lambda_x = 0 has exactly none)
    while (img_groups > 0 && (io.lambda_x[img_groups - 1] == 0.f || sk[img_groups - 1])) --img_groups;
    int last_groups = 3;        // passes whose reconstruction is looked at by anyone
    if (!io.recon_image)
        while (last_groups > 1 && last.coef[last_groups - 1] == 0.f) --last_groups;
    const bool fuse_tail = P.slab.pool != nullptr && mmvae_knob(K_dec_last_ca) != 0;
    MMVAE_TRY(dec_fwd(P, 3, training, &last, s, last_groups, fuse_tail ? (do_backward ? std::min(img_groups, last_groups) : 0) : -1, fuse));
    if (!do_backward) {
        MMVAE_TRY(edge(P, T, s));
        hipLaunchKernelGGL(sum_slots_kernel, dim3(1), dim3(64), 0, s, w.sums, io.sums);
        return mmvae_check_launch("sum_slots");
    }
    // =============================== backward ===============================
    P.wgrad_forked = true;
    int rc = MMVAE_OK;
    if (img_groups > 0) rc = dec_bwd(P, w.dlogit, img_groups, w.dz_img, s, fuse_tail, fuse);
    if (rc == MMVAE_OK) rc = edge(P, T, s);          // dz of the attribute decoder
    Latent3BwdArgs lb{};
    lb.f = la; lb.dz_a = w.dz_img; lb.dz_b = w.dz_att;
    for (int k = 0; k < 3; ++k) lb.kl_coef[k] = sk[k] ? 0.f : io.kl_lambda / (float)B;
    lb.d_img_out_bf = w.d_encout; lb.d_img_bias = P.buf.grads + P.fc2.b_off;
    lb.d_txt_out = nullptr; lb.d_txt_out_bf = w.d_attout_bf; lb.d_txt_bias = P.buf.grads + P.ae[1].b_off;
    if (rc == MMVAE_OK) rc = launch_latent3_bwd(lb, s);
    if (rc == MMVAE_OK) rc = edge(P, s, T);
    P.wgrad_forked = false; P.no_splitk = !serial;
    if (rc == MMVAE_OK) rc = att_enc_bwd(P, w.d_attout_bf, T);
    P.wgrad_forked = true; P.no_splitk = false;
    if (rc == MMVAE_OK) rc = enc_bwd(P, w.d_encout, 2, m1, enc_drop, s, fuse);
    P.wgrad_forked = false;
    MMVAE_TRY(rc);
    MMVAE_TRY(join_sides(P, T, s));
    hipLaunchKernelGGL(sum_slots_kernel, dim3(1), dim3(64), 0, s, w.sums, io.sums);
    MMVAE_TRY(mmvae_check_launch("sum_slots"));
    return io.defer_unpack ? MMVAE_OK : plan_unpack(P, s, true);
}

// ---------------------------------------------------------------- image-only VAE (celeba/model.py:60-88, celeba/train_imageonly.py)
// One pass on B rows in the one-pass carve (img_tower.h tower_image_step); the attribute half of the plan is not touched: its
// gradients stay at the zero the step's prologue wrote.
namespace {
struct CelebaImageTail {
    int mask_width[2] = {HID, 0};
    uint8_t* m2(CelebaPlan&) const { return nullptr; }
    long long last_bias(const CelebaPlan& P) const { return P.fc2.b_off; }
    int enc_fwd(CelebaPlan& P, const float* image, const uint8_t* m1, const uint8_t*, int drop, int training, float* out, hipStream_t s) const {
        return ::enc_fwd(P, image, 1, m1, drop, training, 1, out, s);
    }
    int enc_bwd(CelebaPlan& P, const bf16* d_out, const uint8_t* m1, const uint8_t*, int drop, hipStream_t s) const {
        return ::enc_bwd(P, d_out, 1, m1, drop, s);
    }
};
int celeba_image_step_body(CelebaPlan* P, const mmvae_image_step_io& io, int training, int do_backward, hipStream_t s) {
    MMVAE_REQUIRE(io.enc_mask2 == nullptr, "mmvae_celeba_image_step: the CelebA classifier has one Dropout (enc_mask2 must be NULL)");
    MMVAE_TRY(use_ws(P, io.ws, io.ws_bytes));
    return tower_image_step(*P, io, training, do_backward, s, CelebaImageTail{});
}
}  // namespace
size_t celeba_image_step_workspace_bytes(const CelebaPlan* P) { return P->ws_bytes_module; }
int celeba_image_step(CelebaPlan* P, const mmvae_image_step_io& io, int training, int do_backward, hipStream_t s) {
    return plan_step(P, io, training, do_backward, s, celeba_image_step_body);
}
// log p(x | z) of the particle rows alone: celeba_iw_score without the attribute scorer
int celeba_iw_score_image(CelebaPlan* P, void* ws, size_t wsb, const float* z, const float* image, int B, int K, float* loglik_x, hipStream_t s) {
    MMVAE_REQUIRE(P && z && image && loglik_x, "mmvae_celeba_iw_score_image: null argument");
    MMVAE_REQUIRE(B >= 1 && K >= 1 && (long long)B * K <= P->B,
                  "mmvae_celeba_iw_score_image: %d examples x %d particles exceed the plan's %d rows", B, K, P->B);
    MMVAE_TRY(use_ws(P, ws, wsb));
    const int rows = B * K;
    MMVAE_TRY(launch_fill_zero(P->w.zero_begin, P->w.zero_bytes, s));
    MMVAE_TRY(tower_iw_particles(*P, z, rows, s));
    MMVAE_TRY(dec_fwd(*P, 1, 0, nullptr, s));
    return launch_celeba_iw_tail(tower_iw_tail_args(*P, image, rows, K, loglik_x), s);
}

// ---------------------------------------------------------------- granular module entry points (drop-in modules)
int celeba_image_encoder_fwd(CelebaPlan* P, void* ws, size_t wsb, const float* image, const uint8_t* mask, int training, float* out, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    MMVAE_TRY(launch_fill_zero(P->w.zero_begin, P->w.zero_bytes, s));
    return enc_fwd(*P, image, 1, mask, training && mask != nullptr, training, 1, out, s);
}
int celeba_image_encoder_bwd(CelebaPlan* P, void* ws, size_t wsb, const float* d_out, const uint8_t* mask, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    CelebaPlan::W& w = P->w;
    const int rows = P->B, D2 = 2 * P->D;
    MMVAE_TRY(plan_zero_gpk(*P, s));
    MMVAE_TRY(launch_cast_bf16(d_out, (long long)rows * D2, w.d_encout, s));
    MMVAE_TRY(launch_colsum_f32(d_out, rows, D2, P->buf.grads + P->fc2.b_off, s));
    MMVAE_TRY(enc_bwd(*P, w.d_encout, 1, mask, mask != nullptr, s));
    return plan_unpack(*P, s, true);
}
int celeba_image_decoder_fwd(CelebaPlan* P, void* ws, size_t wsb, const float* z, int training, float* recon, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    CelebaPlan::W& w = P->w;
    const int rows = P->B;
    MMVAE_TRY(launch_fill_zero(w.zero_begin, w.zero_bytes, s));
    hipLaunchKernelGGL(cast_z_kernel, dim3(ceil_div(rows * P->ldz, 256)), dim3(256), 0, s, z, rows, P->D, w.z_bf, P->ldz);
    MMVAE_TRY(mmvae_check_launch("cast_z"));
    ConvTLastFwdArgs last{};
    last.recon = recon;
    return dec_fwd(*P, 1, training, &last, s);
}
int celeba_image_decoder_bwd(CelebaPlan* P, void* ws, size_t wsb, const float* d_recon, const float* recon, float* dz, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    CelebaPlan::W& w = P->w;
    const long long n = (long long)P->B * NPIX;
    MMVAE_TRY(plan_zero_gpk(*P, s));
    hipLaunchKernelGGL(sigmoid_bwd_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, d_recon, recon, n, w.tmp_f32);
    MMVAE_TRY(mmvae_check_launch("sigmoid_bwd"));
    MMVAE_TRY(dec_bwd(*P, w.tmp_f32, 1, dz, s));
    return plan_unpack(*P, s, true);
}
int celeba_attrs_encoder_fwd(CelebaPlan* P, void* ws, size_t wsb, const float* attrs, int training, float* out, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    MMVAE_TRY(launch_fill_zero(P->w.zero_begin, P->w.zero_bytes, s));
    return att_enc_fwd(*P, attrs, training, 1, out, s);
}
int celeba_attrs_encoder_bwd(CelebaPlan* P, void* ws, size_t wsb, const float* d_out, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    CelebaPlan::W& w = P->w;
    const int rows = P->B, D2 = 2 * P->D;
    MMVAE_TRY(plan_zero_gpk(*P, s));
    MMVAE_TRY(launch_cast_bf16(d_out, (long long)rows * D2, w.d_attout_bf, s));
    MMVAE_TRY(launch_colsum_f32(d_out, rows, D2, P->buf.grads + P->ae[1].b_off, s));
    MMVAE_TRY(att_enc_bwd(*P, w.d_attout_bf, s));
    return plan_unpack(*P, s, true);
}
int celeba_attrs_decoder_fwd(CelebaPlan* P, void* ws, size_t wsb, const float* z, int training, float* recon, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    CelebaPlan::W& w = P->w;
    const int rows = P->B;
    MMVAE_TRY(launch_fill_zero(w.zero_begin, w.zero_bytes, s));
    hipLaunchKernelGGL(cast_z_kernel, dim3(ceil_div(rows * P->ldz, 256)), dim3(256), 0, s, z, rows, P->D, w.z_bf, P->ldz);
    MMVAE_TRY(mmvae_check_launch("cast_z"));
    MMVAE_TRY(att_dec_fwd(*P, 1, training, w.alogits, s));
    const long long n = (long long)rows * NA;
    hipLaunchKernelGGL(sigmoid_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, w.alogits, n, recon);
    return mmvae_check_launch("sigmoid");
}
int celeba_attrs_decoder_bwd(CelebaPlan* P, void* ws, size_t wsb, const float* d_recon, const float* recon, float* dz, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    CelebaPlan::W& w = P->w;
    const long long n = (long long)P->B * NA;
    MMVAE_TRY(plan_zero_gpk(*P, s));
    hipLaunchKernelGGL(sigmoid_bwd_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, d_recon, recon, n, w.dalogit);
    MMVAE_TRY(mmvae_check_launch("sigmoid_bwd"));
    MMVAE_TRY(att_dec_bwd(*P, w.dalogit, 1, dz, s));
    return plan_unpack(*P, s, true);
}

// ---------------------------------------------------------------- importance-weighted evaluation (iw.h, celeba_iw.hip)
// Eval-mode decoders on the B*K particle rows z [B][K][D].  Image: the bf16 decoder body of celeba_image_decoder_fwd up to the
// raw output of hallucinate.6 (no stand-alone BatchNorm + Swish pass over it), then the forward-only scoring tail -- one
// log p(x|z) per row against the row's own example.  Attributes: the fp32 scorer on the bound parameters.  No backward
// activation is kept; parameters, BatchNorm buffers and gradients are only read.
size_t celeba_iw_workspace_bytes(const CelebaPlan* P) { return P->ws_bytes_module; }
int celeba_iw_attrs(CelebaPlan* P, const float* z, long long rows, float* words, hipStream_t s) {
    MMVAE_TRY(check_bound(P));
    const BnL& b = P->abn[1];
    const float* p = P->buf.params;
    CelebaIwAttrsArgs a{};
    a.w0 = p + P->ad[0].w_off; a.b0 = p + P->ad[0].b_off; a.w1 = p + P->ad[1].w_off; a.b1 = p + P->ad[1].b_off;
    a.gamma = p + b.w_off; a.beta = p + b.b_off; a.rmean = P->buf.bn_stats + b.stat_off; a.rvar = a.rmean + b.C; a.eps = BN_EPS;
    a.z = z; a.rows = rows; a.D = P->D; a.words = words;
    return launch_celeba_iw_attrs(a, s);
}
int celeba_iw_score(CelebaPlan* P, void* ws, size_t wsb, const float* z, const float* image, int B, int K, float* loglik_x, float* words,
                    hipStream_t s) {
    MMVAE_REQUIRE(P && z && image && loglik_x && words, "mmvae_celeba_iw_score: null argument");
    MMVAE_REQUIRE(B >= 1 && K >= 1 && (long long)B * K <= P->B,
                  "mmvae_celeba_iw_score: %d examples x %d particles exceed the plan's %d rows", B, K, P->B);
    MMVAE_TRY(use_ws(P, ws, wsb));
    const int rows = B * K;
    MMVAE_TRY(launch_fill_zero(P->w.zero_begin, P->w.zero_bytes, s));
    MMVAE_TRY(tower_iw_particles(*P, z, rows, s));
    MMVAE_TRY(dec_fwd(*P, 1, 0, nullptr, s));
    MMVAE_TRY(launch_celeba_iw_tail(tower_iw_tail_args(*P, image, rows, K, loglik_x), s));
    return celeba_iw_attrs(P, z, rows, words, s);
}

// ---------------------------------------------------------------- test / profiling aid: replay one layer of the step
// The tower's names (img_tower.h tower_named_gemm / tower_named_wgrad, with the _staged forms) and fc2_dgrad.  Knob
// "celeba_layer_mask" (0): the keep flags in W::m1 take part in fc1 / fc2_dgrad as in a step with classifier dropout.  fc2_dgrad
// reads d_encout and, as in the step, adds its column sums to the bias gradient of classifier.0 in the flat gradients; up_dgrad
// writes dz into dz_img.
int celeba_bench_layer(CelebaPlan* P, void* ws, size_t wsb, const char* layer, int iters, hipStream_t s) {
    MMVAE_REQUIRE(P && layer, "mmvae_celeba_bench_layer: null argument");
    MMVAE_TRY(use_ws(P, ws, wsb, false));
    CelebaPlan::W& w = P->w;
    const std::string name = layer;
    const uint8_t* mask = mmvae_knob(K_celeba_layer_mask) ? w.m1 : nullptr;
    WgradParams wg{};
    if (tower_named_wgrad(*P, name, wg)) return tower_replay_wgrad(*P, wg, iters, s);
    GemmParams g{};
    GatherTransform tr{};
    if (name == "fc2_dgrad") g = fc2_dgrad_gemm(*P, 2, mask, w.d_encout);
    else { MMVAE_REQUIRE(tower_named_gemm(*P, name, mask, w.dz_img, true, g, tr), "mmvae_celeba_bench_layer: unknown layer '%s'", layer); }
    for (int i = 0; i < iters; ++i) MMVAE_TRY(launch_gemm_gather(g, s));
    return MMVAE_OK;
}
// byte offset of a named workspace buffer of the fused step's carving (3 passes), -1 if unknown
long long celeba_debug_offset(CelebaPlan* P, const char* name) {
    if (!P || !name) return -1;
    Workspace ws((void*)0x1000, (size_t)1 << 40);      // (every call that works in a workspace carves its own again: plan_use_ws)
    P->carve_passes = 3;
    carve(*P, ws);
    CelebaPlan::W& w = P->w;
    std::map<std::string, const void*> m = tower_debug_names(w);
    m.insert({{"encout", w.encout}, {"m1", w.m1}, {"z_f32", w.z_f32}, {"dz_img", w.dz_img}, {"dz_att", w.dz_att},
              {"d_encout", w.d_encout}, {"tmp_f32", w.tmp_f32}});
    return tower_offset_of(m, name, (const void*)0x1000);
}
