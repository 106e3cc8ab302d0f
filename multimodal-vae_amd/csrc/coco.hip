// COCO MMVAE (coco/model.py:22-90,147-312 ; coco/train.py:66-84,146-165).
//
// Image half on the shared bf16 gather-GEMM / BatchNorm / thin-layer kernels: 3x32x32 images, four k4 s2 p1 convolutions
// (64/128/256/512 channels), classifier 2048-1024-256-2D with two Dropouts, decoder Linear(D,2048) + four transposed
// convolutions, sigmoid + BCE.  Caption half (coco_text.hip) in fp32: biGRU encoder over 102 GloVe vectors, 2-layer GRU
// decoder with vector feedback, MSE loss.
//
// Passes (coco/train.py:146-165): (image,text), (image), (text) with lambda_xy = (1,1,0), lambda_yx = (1,1,1).  Image
// features run once for passes 1 and 2 (classifier twice: independent Dropout masks), the caption encoder once for
// passes 1 and 3 (no dropout: identical), decoders on 3B rows with BatchNorm statistics per pass.  The caption half runs
// on the side stream next to the image half.
#include "coco_plan.h"
#include <cstring>

namespace {
constexpr int IMG = 32, NPIX = 3 * IMG * IMG, FEAT = 2048, HID1 = 1024, HID2 = 256;

void build(CocoPlan& P) {
    const int D = P.D;
    auto lin = [&](const std::string& n, int o, int i) { add_param(P, n + ".weight", {o, i}); add_param(P, n + ".bias", {o}); };
    auto bnp = [&](const std::string& n, int c) { add_param(P, n + ".weight", {c}); add_param(P, n + ".bias", {c}); };
    auto gru = [&](const std::string& n, const char* sfx, int in) {
        add_param(P, n + ".weight_ih_" + sfx, {COCO_G, in}); add_param(P, n + ".weight_hh_" + sfx, {COCO_G, COCO_H});
        add_param(P, n + ".bias_ih_" + sfx, {COCO_G}); add_param(P, n + ".bias_hh_" + sfx, {COCO_G});
    };
    add_param(P, "image_encoder.features.0.weight", {64, 3, 4, 4});
    add_param(P, "image_encoder.features.2.weight", {128, 64, 4, 4}); bnp("image_encoder.features.3", 128);
    add_param(P, "image_encoder.features.5.weight", {256, 128, 4, 4}); bnp("image_encoder.features.6", 256);
    add_param(P, "image_encoder.features.8.weight", {512, 256, 4, 4}); bnp("image_encoder.features.9", 512);
    lin("image_encoder.classifier.0", HID1, FEAT);
    lin("image_encoder.classifier.3", HID2, HID1);
    lin("image_encoder.classifier.6", 2 * D, HID2);
    lin("image_decoder.upsample.0", FEAT, D);
    add_param(P, "image_decoder.hallucinate.0.weight", {512, 256, 4, 4}); bnp("image_decoder.hallucinate.1", 256);
    add_param(P, "image_decoder.hallucinate.3.weight", {256, 128, 4, 4}); bnp("image_decoder.hallucinate.4", 128);
    add_param(P, "image_decoder.hallucinate.6.weight", {128, 64, 4, 4}); bnp("image_decoder.hallucinate.7", 64);
    add_param(P, "image_decoder.hallucinate.9.weight", {64, 3, 4, 4});
    gru("text_encoder.gru", "l0", COCO_E); gru("text_encoder.gru", "l0_reverse", COCO_E);
    lin("text_encoder.h2p", 2 * D, COCO_H);
    lin("text_decoder.z2h", COCO_H, D);
    gru("text_decoder.gru", "l0", COCO_E + D); gru("text_decoder.gru", "l1", COCO_H);
    lin("text_decoder.h2o", COCO_E, COCO_H + D);

    // image encoder (coco/model.py:157-169), image decoder (coco/model.py:197-208)
    const ConvGeom enc[4] = {ConvGeom{3, 64, 4, 4, 2, 1, 32, 32, 16, 16, false}, ConvGeom{64, 128, 4, 4, 2, 1, 16, 16, 8, 8, false},
                             ConvGeom{128, 256, 4, 4, 2, 1, 8, 8, 4, 4, false}, ConvGeom{256, 512, 4, 4, 2, 1, 4, 4, 2, 2, false}};
    const ConvGeom dec[4] = {ConvGeom{512, 256, 4, 4, 2, 1, 2, 2, 4, 4, true}, ConvGeom{256, 128, 4, 4, 2, 1, 4, 4, 8, 8, true},
                             ConvGeom{128, 64, 4, 4, 2, 1, 8, 8, 16, 16, true}, ConvGeom{64, 3, 4, 4, 2, 1, 16, 16, 32, 32, true}};
    P.geo = TowerGeom{IMG, 16, 64, 2, 512, FEAT, HID1};
    tower_build_convs(P, enc, dec);
    add_frag_packs(P, P.conv[1]);      // 8x8 / 16x16 layers: direct-B image-resident kernels (convres.hip)
    add_frag_packs(P, P.convT[2]);
    tower_build_fc1(P);
    auto dense = [&](LinL& f, const std::string& n, int N, int K) {
        f.w_off = off(P, n + ".weight"); f.b_off = off(P, n + ".bias"); f.N = N; f.K = K;
        f.pk_fwd = P.pk.add(pack_dense(f.w_off, N, K, npad_for(N), round_up(round_up(K, 8), 64), K, 1));
        f.gk = P.gk.add(pack_dense(f.w_off, N, K, round_up(N, 64), round_up(round_up(K, 8), 64), K, 1));
        f.pk_dgrad = P.pk.add(pack_dense(f.w_off, K, N, npad_for(K), round_up(round_up(N, 8), 64), 1, K));
    };
    dense(P.fc2, "image_encoder.classifier.3", HID2, HID1);
    dense(P.fc3, "image_encoder.classifier.6", 2 * D, HID2);
    tower_build_up(P);
    P.pk_text_begin = (int)P.pk.d.size();
    coco_text_build(P);
}

void carve(CocoPlan& P, Workspace& ws) {
    CocoPlan::W& w = P.w;
    const size_t B = P.B, D = P.D, B3 = (size_t)P.carve_passes * B, B2 = (size_t)(P.carve_passes < 2 ? P.carve_passes : 2) * B, T = P.T;
    const int SS = MMVAE_STAT_SLOTS;
    const int ec[3] = {128, 256, 512}, dc[3] = {256, 128, 64};
    // carve_iw (coco_iw_score): only what the eval-mode forward of the two decoders touches gets room; everything wrapped in
    // bk() -- the encoders' buffers, what a backward pass reads or writes, the bf16 caption kernels' operands -- is empty
    const bool iw = P.carve_iw;
    auto bk = [iw](size_t n) { return iw ? (size_t)0 : n; };
    char* z0 = ws.take<char>(0);
    for (int i = 0; i < 3; ++i) { w.st_e[i] = ws.take<float2>(SS * ec[i]); w.red_e[i] = ws.take<float2>(SS * ec[i]); }
    for (int i = 0; i < 3; ++i) { w.st_d[i] = ws.take<float2>(3 * SS * dc[i]); w.red_d[i] = ws.take<float2>(3 * SS * dc[i]); }
    w.sums = ws.take<float>(16 * MMVAE_LOSS_SLOTS);
    P.sk_cnt = ws.take<unsigned>(1024);
    w.dz_img = ws.take<float>(B3 * D);
    w.td_dh0 = ws.take<float>(B3 * COCO_H); w.td_dh1 = ws.take<float>(B3 * COCO_H); w.zeros_h = ws.take<float>(B3 * COCO_H);
    char* z1 = ws.take<char>(0);
    w.zero_begin = z0; w.zero_bytes = (size_t)(z1 - z0);
    w.dz_txt = ws.take<float>(B3 * D);
    for (int i = 0; i < 3; ++i) { w.aff_e[i] = ws.take<float2>(ec[i]); w.mr_e[i] = ws.take<float2>(ec[i]); }
    for (int i = 0; i < 3; ++i) { w.aff_d[i] = ws.take<float2>(3 * dc[i]); w.mr_d[i] = ws.take<float2>(3 * dc[i]); }
    w.patches1 = ws.take<bf16>(bk(B * 256 * 48));
    w.r1 = ws.take<bf16>(bk(B * 256 * 64)); w.r2 = ws.take<bf16>(bk(B * 64 * 128)); w.r3 = ws.take<bf16>(bk(B * 16 * 256)); w.r4 = ws.take<bf16>(bk(B * FEAT));
    w.a1 = ws.take<bf16>(bk(B * 256 * 64)); w.a2 = ws.take<bf16>(bk(B * 64 * 128)); w.a3 = ws.take<bf16>(bk(B * 16 * 256)); w.a4 = ws.take<bf16>(bk(B * FEAT));
    w.y1 = ws.take<bf16>(bk(B2 * HID1)); w.ay1 = ws.take<bf16>(bk(B2 * HID1)); w.y2 = ws.take<bf16>(bk(B2 * HID2)); w.ay2 = ws.take<bf16>(bk(B2 * HID2));
    w.encout = ws.take<float>(bk(B2 * 2 * D)); w.m1 = ws.take<uint8_t>(bk(B2 * HID1)); w.m2 = ws.take<uint8_t>(bk(B2 * HID2));
    w.gkeep = ws.take<uint8_t>(bk(T * B3 * COCO_H));
    w.eps = ws.take<float>(B3 * D); w.mu = ws.take<float>(B3 * D); w.logvar = ws.take<float>(B3 * D);
    w.z_f32 = ws.take<float>(B3 * D); w.z_bf = ws.take<bf16>(B3 * P.ldz);
    w.u = ws.take<bf16>(B3 * FEAT); w.au = ws.take<bf16>(B3 * FEAT);
    w.q1 = ws.take<bf16>(B3 * 16 * 256); w.q2 = ws.take<bf16>(B3 * 64 * 128); w.q3 = ws.take<bf16>(B3 * 256 * 64);
    w.aq1 = ws.take<bf16>(B3 * 16 * 256); w.aq2 = ws.take<bf16>(B3 * 64 * 128); w.aq3 = ws.take<bf16>(bk(B3 * 256 * 64));   // (the scoring tail activates q3 itself)
    w.dlogit = ws.take<float>(bk(B3 * NPIX));
    w.patches4 = ws.take<bf16>(bk(B3 * 256 * 48));
    w.d3 = ws.take<bf16>(bk(B3 * 256 * 64)); w.d2 = ws.take<bf16>(bk(B3 * 64 * 128)); w.d1 = ws.take<bf16>(bk(B3 * 16 * 256));
    w.du = ws.take<bf16>(bk(B3 * FEAT));
    w.d_encout = ws.take<bf16>(bk(B2 * 2 * D)); w.dy2 = ws.take<bf16>(bk(B2 * HID2)); w.dy1 = ws.take<bf16>(bk(B2 * HID1));
    w.db4 = ws.take<bf16>(bk(B2 * FEAT)); w.dr4 = ws.take<bf16>(bk(B * FEAT));
    w.d3e = ws.take<bf16>(bk(B * 16 * 256)); w.d2e = ws.take<bf16>(bk(B * 64 * 128)); w.d1e = ws.take<bf16>(bk(B * 256 * 64));
    w.tmp_f32 = ws.take<float>(bk(B3 * NPIX));
    P.sk_floats = (size_t)256 * 128 * 128;
    P.sk_buf = ws.take<float>(P.sk_floats);
    // weight-gradient partial-tile slabs (written and read once per step, never zeroed): gemm.h WgradSlabCtx
    w.slab_floats = bk((size_t)(P.carve_passes >= 3 ? 48 : 16) << 20);
    w.slab = ws.take<float>(w.slab_floats);
    coco_text_carve(P, ws);
}

// ================================================================== the classifier behind classifier.0
// The launches of the conv chain, classifier.0 and the decoder are the tower's (img_tower.h: tower_gemm / tower_wgrad and the
// passes around them); classifier.3 / classifier.6 are built here, for the step and for coco_bench_layer alike.  n: dropout variants.
enum CoGemm { CO_FC2, CO_FC3, CO_FC3_DGRAD, CO_FC2_DGRAD };
enum CoWgrad { CO_W_FC2, CO_W_FC3 };

// mask: keep flags of the classifier Dropout the layer applies (CO_FC2_DGRAD: m1, CO_FC2 / CO_FC3_DGRAD: m2) or null;
// aux: CO_FC3 the fp32 result [n*B][2D], CO_FC3_DGRAD the operand d_out [n*B][2D]
GemmParams layer_gemm(CocoPlan& P, CoGemm kind, int n, const uint8_t* mask = nullptr, const void* aux = nullptr) {
    CocoPlan::W& w = P.w;
    const int rows = n * P.B, D2 = 2 * P.D;
    const float ms = 1.f / (1.f - DROP_P);
    switch (kind) {
    case CO_FC2: {   // classifier.3 + Swish + Dropout
        GatherPlan pl = dense_plan(rows, HID1, HID1, HID2);
        GemmParams g = gemm_of(P, pl, &P.fc2.pk_fwd, 1, rows);
        g.c.A = w.ay1;
        g.bias = P.buf.params + P.fc2.b_off; g.out_bf = w.y2; g.ldo = HID2;
        g.out_act_bf = w.ay2; g.e_act = ACT_SWISH; if (mask) { g.e_mask = mask; g.e_mask_scale = ms; }
        return g;
    }
    case CO_FC3: {   // classifier.6
        GatherPlan pl = dense_plan(rows, HID2, HID2, D2);
        GemmParams g = gemm_of(P, pl, &P.fc3.pk_fwd, 1, rows);
        g.c.A = w.ay2;
        g.bias = P.buf.params + P.fc3.b_off; g.out_f = (float*)aux; g.ldo = D2;
        return g;
    }
    case CO_FC3_DGRAD: {   // classifier.6: its column sums are the bias gradient of classifier.3
        GatherPlan pd = dense_plan(rows, D2, D2, HID2);
        GemmParams d = gemm_of(P, pd, &P.fc3.pk_dgrad, 1, rows);
        d.c.A = (const bf16*)aux; d.out_bf = w.dy2; d.ldo = HID2;
        d.d_r = w.y2; d.d_ld = HID2; d.d_act = ACT_SWISH; if (mask) { d.d_mask = mask; d.d_mask_scale = ms; }
        d.d_colsum = P.buf.grads + P.fc2.b_off;
        return d;
    }
    case CO_FC2_DGRAD: {   // classifier.3: its column sums are the bias gradient of classifier.0
        GatherPlan pd = dense_plan(rows, HID2, HID2, HID1);
        GemmParams d = gemm_of(P, pd, &P.fc2.pk_dgrad, 1, rows);
        d.c.A = w.dy2; d.out_bf = w.dy1; d.ldo = HID1;
        d.d_r = w.y1; d.d_ld = HID1; d.d_act = ACT_SWISH; if (mask) { d.d_mask = mask; d.d_mask_scale = ms; }
        d.d_colsum = P.buf.grads + P.fc1.b_off;
        return d;
    }
    }
    return GemmParams{};
}

// aux: CO_W_FC3 the operand d_out [n*B][2D]
WgradParams layer_wgrad(CocoPlan& P, CoWgrad kind, int n, const bf16* aux = nullptr) {
    CocoPlan::W& w = P.w;
    const int rows = n * P.B;
    if (kind == CO_W_FC2) {   // classifier.3
        GatherPlan pl = dense_plan(rows, HID1, HID1, HID2);
        WgradParams g = wgrad_of(P, pl, &P.fc2.gk, 1, rows);
        g.c.A = w.ay1; g.P = w.dy2; g.ldp = HID2;
        return g;
    }
    GatherPlan pl = dense_plan(rows, HID2, HID2, 2 * P.D);   // classifier.6
    WgradParams g = wgrad_of(P, pl, &P.fc3.gk, 1, rows);
    g.c.A = w.ay2; g.P = aux; g.ldp = 2 * P.D;
    return g;
}

// ================================================================== image encoder (coco/model.py:182-187)
int enc_fwd(CocoPlan& P, const float* image, int variants, const uint8_t* m1, const uint8_t* m2, int dropout, int training,
            int bn_updates, float* out, hipStream_t s) {
    MMVAE_TRY(tower_enc_fwd(P, image, training, bn_updates, s));
    const bool drop = training && dropout;
    MMVAE_TRY(launch_gemm_gather(tower_gemm(P, TW_FC1, 0, variants, training, drop ? m1 : nullptr), s));
    MMVAE_TRY(launch_gemm_gather(layer_gemm(P, CO_FC2, variants, drop ? m2 : nullptr), s));
    return launch_gemm_gather(layer_gemm(P, CO_FC3, variants, nullptr, out), s);
}

// d_out: bf16 [variants*B][2D]; the bias gradient of classifier.6 must already be accumulated by the caller
int enc_bwd(CocoPlan& P, const bf16* d_out, int variants, const uint8_t* m1, const uint8_t* m2, int dropout, hipStream_t s) {
    // classifier.6
    MMVAE_TRY(wgrad_async(P, layer_wgrad(P, CO_W_FC3, variants, d_out), s));
    MMVAE_TRY(launch_gemm_gather(layer_gemm(P, CO_FC3_DGRAD, variants, dropout ? m2 : nullptr, d_out), s));
    // classifier.3
    MMVAE_TRY(wgrad_async(P, layer_wgrad(P, CO_W_FC2, variants), s));
    MMVAE_TRY(launch_gemm_gather(layer_gemm(P, CO_FC2_DGRAD, variants, dropout ? m1 : nullptr), s));
    // classifier.0: wgrad gathers the shared 2x2x512 map; the input gradient is one dense GEMM over NHWC columns
    MMVAE_TRY(wgrad_async(P, tower_wgrad(P, TW_W_FC1, 0, variants), s));
    MMVAE_TRY(launch_gemm_gather(tower_gemm(P, TW_FC1_DGRAD, 0, variants), s));
    return tower_enc_bwd(P, variants, s);
}

// ================================================================== image decoder (coco/model.py:211-216)
// last == nullptr (coco_iw_score): the body only -- it ends with the raw output of hallucinate.6 in q3, whose BatchNorm + Swish
// belong to the caller's own tail
int dec_fwd(CocoPlan& P, int groups, int training, ConvTLastFwdArgs* last, hipStream_t s) {
    MMVAE_TRY(tower_dec_fwd(P, groups, training, last != nullptr, s));
    if (!last) return MMVAE_OK;
    return launch_convt_last_fwd(dec_last_args(P, *last, groups), s);
}

int use_ws(CocoPlan* P, void* ws, size_t bytes, bool module = true) {
    MMVAE_TRY(plan_use_ws(P, ws, bytes, module, carve));
    P->wgrad_forked = false;
    P->dec_wg_pending = false;
    P->comb_fresh = false; P->dw16_fresh = false; P->dec_wg_composed = false;
    P->cl_alarm_f = P->cl_alarm_b = nullptr;
    return MMVAE_OK;
}
// coco_iw_score: its own (smaller) carve, with every check and reset of use_ws against ws_bytes_iw
int use_ws_iw(CocoPlan* P, void* ws, size_t bytes) {
    const size_t module_bytes = P->ws_bytes_module;
    P->ws_bytes_module = P->ws_bytes_iw; P->carve_iw = true;
    const int rc = use_ws(P, ws, bytes);
    P->ws_bytes_module = module_bytes; P->carve_iw = false;
    return rc;
}
int zero_ws(CocoPlan& P, hipStream_t s) { return launch_fill_zero(P.w.zero_begin, P.w.zero_bytes, s); }

}  // namespace

CocoPlan* coco_create(int D, int B, int T) {
    if (D < 4 || D > 124 || D % 4 != 0 || B < 1 || T < 1 || T > 1024) {
        mmvae_set_error("coco_create: need n_latents in 4..124, a multiple of 4, batch >= 1 and 1 <= steps <= 1024");
        return nullptr;
    }
    CocoPlan* P = new CocoPlan();
    P->D = D; P->B = B; P->T = T;
    build(*P);
    plan_size_workspaces(*P, carve);
    {   // the scoring call's workspace: one pass, forward buffers of the two decoders only
        P->carve_iw = true; P->carve_passes = 1;
        Workspace wi(nullptr, 0);
        carve(*P, wi);
        P->ws_bytes_iw = wi.used();
        P->carve_iw = false; P->carve_passes = 3;
    }
    return P;
}
void coco_destroy(CocoPlan* P) { delete P; }
PlanBase* coco_base(CocoPlan* P) { return P; }
int coco_steps(const CocoPlan* P) { return P->T; }

static int coco_step_body(CocoPlan* Pp, const mmvae_coco_step_io& io, int training, int do_backward, hipStream_t s);
int coco_step(CocoPlan* Pp, const mmvae_coco_step_io& io, int training, int do_backward, hipStream_t s) {
    return plan_step(Pp, io, training, do_backward, s, coco_step_body);
}
static int coco_step_body(CocoPlan* Pp, const mmvae_coco_step_io& io, int training, int do_backward, hipStream_t s) {
    MMVAE_TRY(use_ws(Pp, io.ws, io.ws_bytes, false));
    CocoPlan& P = *Pp;
    CocoPlan::W& w = P.w;
    const int B = P.B, D = P.D, B3 = 3 * B, T = P.T;
    MMVAE_REQUIRE(io.image && io.text && io.sos && io.sums, "coco step: image/text/sos/sums must be given");
    const float* eps = io.eps;
    const uint8_t *m1 = io.enc_mask1, *m2 = io.enc_mask2, *gk = io.gru_keep;
    StepBeginArgs sb{};
    sb.zero_ptr[0] = w.zero_begin; sb.zero_bytes[0] = w.zero_bytes;
    if (do_backward) {
        sb.zero_ptr[1] = P.buf.gpk; sb.zero_bytes[1] = (size_t)P.gk.mat_elems * sizeof(float);
        sb.zero_ptr[2] = P.buf.grads; sb.zero_bytes[2] = (size_t)(P.nparams / 4) * 16;
    }
    sb.p = DROP_P; sb.seed = io.seed; sb.step = io.step_counter;
    if (training && !eps) { sb.eps = w.eps; sb.n_eps = (long long)B3 * D; eps = w.eps; }
    if (training && io.enc_dropout && !m1) { sb.mask[0] = w.m1; sb.n_mask[0] = (long long)2 * B * HID1; m1 = w.m1; }
    if (training && io.enc_dropout && !m2) { sb.mask[1] = w.m2; sb.n_mask[1] = (long long)2 * B * HID2; m2 = w.m2; }
    if (training && io.gru_dropout && !gk) { sb.mask[2] = w.gkeep; sb.n_mask[2] = (long long)T * B3 * COCO_H; gk = w.gkeep; }
    if (!(training && io.gru_dropout)) gk = nullptr;
    MMVAE_TRY(launch_step_begin(sb, s));
    if (do_backward && P.nparams % 4 != 0)
        MMVAE_TRY(launch_fill_zero(P.buf.grads + (P.nparams / 4) * 4, (size_t)(P.nparams % 4) * sizeof(float), s));
    const int enc_drop = training && io.enc_dropout;
    const int sk[3] = {io.pass_skip[0] != 0, io.pass_skip[1] != 0, io.pass_skip[2] != 0};
    P.dec_skip_mask = (unsigned)(sk[0] | (sk[1] << 1) | (sk[2] << 2));
    MMVAE_TRY(ensure_streams(P));
    const bool serial = mmvae_serial();
    hipStream_t Tx = serial ? s : P.st_text;
    // ---- encoders: caption GRU on the side stream, image encoder on main
    MMVAE_TRY(edge(P, s, Tx));
    hipStream_t Sd = serial ? s : P.st_wgrad;       // idle until the backward pass: the caption decoder's packs
    const bool packing = io.pack_first && !P.no_pack;
    if (packing) {      // the caption encoder's recurrence opens the critical chain: its (few) packs first, everything else beside them
        const int nd = (int)P.pk.d.size();
        auto range = [&](int d0, int d1, hipStream_t st) {
            return launch_pack_range(P.buf.desc_dev, P.pk.d.data(), nd, d0, d1, P.buf.params, P.buf.packed, P.buf.packed_vec, st);
        };
        MMVAE_TRY(range(P.pk_text_begin, P.pk_textdec_begin, Tx));
        if (Sd != s) MMVAE_TRY(edge(P, s, Sd));
        MMVAE_TRY(range(P.pk_textdec_begin, nd, Sd));
        MMVAE_TRY(range(0, P.pk_text_begin, s));
    }
    MMVAE_TRY(coco_text_enc_fwd(P, io.text, do_backward, w.txtout, Tx, true, serial ? nullptr : &s));
    MMVAE_TRY(enc_fwd(P, io.image, 2, m1, m2, enc_drop, training, 2 - sk[0] - sk[1], w.encout, s));
    if (coco_text_dec_composed(P, B3)) MMVAE_TRY(coco_text_dec_prepare(P, io.sos, s));     // (main stream: idle here until the caption encoder is through)
    MMVAE_TRY(edge(P, Tx, s));
    Latent3Args la{};
    la.B = B; la.D = D; la.img_out = w.encout; la.txt_out = w.txtout; la.eps = eps;
    la.mu = io.mu ? io.mu : w.mu; la.logvar = io.logvar ? io.logvar : w.logvar;
    la.z_f32 = w.z_f32; la.z_bf = w.z_bf; la.ldz = P.ldz; la.kl_sum = w.sums + 8; la.training = training;
    MMVAE_TRY(launch_latent3_fwd(la, s));
    // ---- caption decoder (+ MSE, + its backward) on the side stream, image decoder on main
    MMVAE_TRY(edge(P, s, Tx));
    if (packing && Sd != Tx) MMVAE_TRY(edge(P, Sd, Tx));
    float* sentence = io.recon_text ? io.recon_text : w.td_recon;
    {
        CocoMseFuse mf{};
        for (int k = 0; k < 3; ++k) mf.coef[k] = sk[k] ? 0.f : io.lambda_yx[k] / ((float)B * (float)T * (float)COCO_E);
        mf.target = io.text; mf.loss_sum = w.sums; mf.dw = do_backward ? w.td_dw : nullptr; mf.dw16 = P.text_bf16 ? w.tb_dw16 : nullptr;
        MMVAE_TRY(coco_text_dec_fwd(P, w.z_f32, 3, io.sos, gk, do_backward, sentence, Tx, true, &mf));
        if (!P.mse_fused)       // (no bf16 copy of the gradient here: only the composed BPTT kernel reads one, and converts it itself then)
            MMVAE_TRY(coco_mse3(sentence, io.text, 3, (long long)B * T * COCO_E, mf.coef, w.sums, mf.dw, Tx));
        P.dw16_fresh = do_backward && P.mse_fused;
    }
    if (do_backward) MMVAE_TRY(coco_text_dec_bwd(P, w.z_f32, 3, io.sos, gk, sentence, w.td_dw, w.dz_txt, Tx, serial ? Tx : P.st_wgrad2, true));
    ConvTLastFwdArgs last{};
    last.target = io.image; last.recon = io.recon_image; last.dlogit = do_backward ? w.dlogit : nullptr; last.loss_sum = w.sums;
    for (int k = 0; k < 3; ++k) last.coef[k] = sk[k] ? 0.f : io.lambda_xy[k] / (float)(B * NPIX);
    MMVAE_TRY(dec_fwd(P, 3, training, &last, s));
    if (!do_backward) {
        MMVAE_TRY(edge(P, Tx, s));
        hipLaunchKernelGGL(sum_slots_kernel, dim3(1), dim3(64), 0, s, w.sums, io.sums, P.cl_alarm_f, (const unsigned*)nullptr);
        return mmvae_check_launch("sum_slots");
    }
    // =============================== backward ===============================
    P.wgrad_forked = true;
    int img_groups = 3;
    while (img_groups > 0 && (io.lambda_xy[img_groups - 1] == 0.f || sk[img_groups - 1])) --img_groups;
    int rc = MMVAE_OK;
    if (img_groups > 0) rc = tower_dec_bwd(P, w.dlogit, img_groups, w.dz_img, s);
    if (rc == MMVAE_OK) rc = edge(P, Tx, s);          // dz of the caption decoder
    Latent3BwdArgs lb{};
    lb.f = la; lb.dz_a = w.dz_img; lb.dz_b = w.dz_txt;
    for (int k = 0; k < 3; ++k) lb.kl_coef[k] = sk[k] ? 0.f : io.kl_lambda / (float)B;
    lb.d_img_out_bf = w.d_encout; lb.d_img_bias = P.buf.grads + P.fc3.b_off;
    lb.d_txt_out = w.d_txtout;
    if (rc == MMVAE_OK) rc = launch_latent3_bwd(lb, s);
    if (rc == MMVAE_OK) rc = edge(P, s, Tx);
    if (rc == MMVAE_OK) rc = coco_text_enc_bwd(P, io.text, w.d_txtout, Tx, serial ? Tx : P.st_wgrad2, true);
    if (rc == MMVAE_OK) rc = coco_text_dec_wgrads(P, serial ? Tx : P.st_wgrad2);   // (no-op: issued behind the encoder's BPTT launch)
    if (rc == MMVAE_OK) rc = enc_bwd(P, w.d_encout, 2, m1, m2, enc_drop, s);
    P.wgrad_forked = false;
    MMVAE_TRY(rc);
    MMVAE_TRY(edge(P, Tx, s));
    MMVAE_TRY(edge(P, P.st_wgrad, s));
    if (P.st_wgrad2 != P.st_wgrad) MMVAE_TRY(edge(P, P.st_wgrad2, s));
    if (io.defer_unpack) MMVAE_TRY(launch_wgrad_reduce(&P.slab, s));  // the packed gradients are complete; Adam gathers them
    else MMVAE_TRY(plan_unpack(P, s, true));
    // (timeout words of the decoder's cluster launches of THIS step: zeroed before each of them, set only when an exchange gave up;
    //  last kernel of the step, so that the mark in the gradient is not overwritten)
    hipLaunchKernelGGL(sum_slots_kernel, dim3(1), dim3(64), 0, s, w.sums, io.sums, P.cl_alarm_f, P.cl_alarm_b, io.optimizer_state, P.buf.grads);
    return mmvae_check_launch("sum_slots");
}

// ---------------------------------------------------------------- image-only VAE (coco/model.py:93-117, coco/train_imageonly.py)
// One pass on B rows in the one-pass carve (img_tower.h tower_image_step); the caption half of the plan is not touched: no GRU
// step runs, its gradients stay at the zero the step's prologue wrote.
namespace {
struct CocoImageTail {
    int mask_width[2] = {HID1, HID2};
    uint8_t* m2(CocoPlan& P) const { return P.w.m2; }
    long long last_bias(const CocoPlan& P) const { return P.fc3.b_off; }
    int enc_fwd(CocoPlan& P, const float* image, const uint8_t* m1, const uint8_t* m2, int drop, int training, float* out, hipStream_t s) const {
        return ::enc_fwd(P, image, 1, m1, m2, drop, training, 1, out, s);
    }
    int enc_bwd(CocoPlan& P, const bf16* d_out, const uint8_t* m1, const uint8_t* m2, int drop, hipStream_t s) const {
        return ::enc_bwd(P, d_out, 1, m1, m2, drop, s);
    }
};
int coco_image_step_body(CocoPlan* P, const mmvae_image_step_io& io, int training, int do_backward, hipStream_t s) {
    MMVAE_REQUIRE((io.enc_mask1 == nullptr) == (io.enc_mask2 == nullptr), "mmvae_coco_image_step: enc_mask1 / enc_mask2 go together");
    MMVAE_TRY(use_ws(P, io.ws, io.ws_bytes));
    return tower_image_step(*P, io, training, do_backward, s, CocoImageTail{});
}
}  // namespace
size_t coco_image_step_workspace_bytes(const CocoPlan* P) { return P->ws_bytes_module; }
int coco_image_step(CocoPlan* P, const mmvae_image_step_io& io, int training, int do_backward, hipStream_t s) {
    return plan_step(P, io, training, do_backward, s, coco_image_step_body);
}
// ---------------------------------------------------------------- InfoVAE (coco/model.py:358-402, coco/train_infovae.py:44-55)
// The image-only step with one more term in z: lambda_mmd * MMD(prior samples, z) (img_tower.h TowerLatentTerm).  Its workspace is the
// one-pass carve followed by the term's own buffers: the sweep's float64 partial sums, lambda_mmd * dMMD/dz and the drawn prior samples.
namespace {
struct InfoVaeCarve { size_t ws_off, dz_off, drawn_off, total; };
InfoVaeCarve infovae_carve(const CocoPlan* P) {
    auto up16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    InfoVaeCarve c;
    c.ws_off = up16(P->ws_bytes_module);
    c.dz_off = c.ws_off + up16(mmd_dy_workspace_bytes(P->B, P->B, P->D));
    c.drawn_off = c.dz_off + up16((size_t)P->B * P->D * sizeof(float));
    c.total = c.drawn_off + up16((size_t)P->B * P->D * sizeof(float));
    return c;
}
int coco_infovae_step_body(CocoPlan* P, const mmvae_infovae_step_io& io, int training, int do_backward, hipStream_t s) {
    MMVAE_REQUIRE((io.enc_mask1 == nullptr) == (io.enc_mask2 == nullptr), "mmvae_coco_infovae_step: enc_mask1 / enc_mask2 go together");
    MMVAE_TRY(check_bound(P));
    const InfoVaeCarve c = infovae_carve(P);
    MMVAE_REQUIRE(io.ws != nullptr && io.ws_bytes >= c.total, "mmvae_coco_infovae_step: workspace too small (%zu < %zu)", io.ws_bytes, c.total);
    MMVAE_REQUIRE((reinterpret_cast<uintptr_t>(io.ws) & 15) == 0, "mmvae_coco_infovae_step: the workspace must be 16-byte aligned");
    MMVAE_TRY(use_ws(P, io.ws, io.ws_bytes));
    mmvae_image_step_io im{};
    im.ws = io.ws; im.ws_bytes = io.ws_bytes; im.step_counter = io.step_counter; im.image = io.image; im.eps = io.eps;
    im.enc_mask1 = io.enc_mask1; im.enc_mask2 = io.enc_mask2; im.enc_dropout = io.enc_dropout; im.kl_lambda = io.kl_lambda;
    im.lambda_x = io.lambda_x; im.seed = io.seed; im.sums = io.sums; im.recon_image = io.recon_image; im.mu = io.mu; im.logvar = io.logvar;
    im.defer_unpack = io.defer_unpack;
    char* base = (char*)io.ws;
    TowerLatentTerm lt{};
    lt.samples = io.true_samples; lt.drawn = (float*)(base + c.drawn_off); lt.philox_stream = MMVAE_TRUE_SAMPLES_STREAM;
    lt.lambda = io.lambda_mmd; lt.ws = base + c.ws_off; lt.dz = (float*)(base + c.dz_off); lt.z_out = io.z; lt.slot = MMVAE_SUM_MMD_KXX;
    return tower_image_step(*P, im, training, do_backward, s, CocoImageTail{}, &lt);
}
}  // namespace
size_t coco_infovae_step_workspace_bytes(const CocoPlan* P) { return infovae_carve(P).total; }
int coco_infovae_step(CocoPlan* P, const mmvae_infovae_step_io& io, int training, int do_backward, hipStream_t s) {
    return plan_step(P, io, training, do_backward, s, coco_infovae_step_body);
}
// log p(x | z) of the particle rows alone: coco_iw_score without the caption decoder (the same, smaller, carve)
int coco_iw_score_image(CocoPlan* P, void* ws, size_t wsb, const float* z, const float* image, int B, int K, float* loglik_x, hipStream_t s) {
    MMVAE_REQUIRE(P && z && image && loglik_x, "mmvae_coco_iw_score_image: null argument");
    MMVAE_REQUIRE(B >= 1 && K >= 1 && (long long)B * K <= P->B,
                  "mmvae_coco_iw_score_image: %d examples x %d particles exceed the plan's %d rows", B, K, P->B);
    MMVAE_TRY(use_ws_iw(P, ws, wsb));
    const int rows = B * K;
    MMVAE_TRY(zero_ws(*P, s));
    MMVAE_TRY(tower_iw_particles(*P, z, rows, s));
    MMVAE_TRY(dec_fwd(*P, 1, 0, nullptr, s));
    return launch_coco_iw_tail(tower_iw_tail_args(*P, image, rows, K, loglik_x), s);
}

// ---------------------------------------------------------------- text-only VAE (coco/model.py:120-144, coco/train_textonly.py:106-120)
// One pass on B rows in the one-pass carve: caption encoder (bf16 persistent kernels), latent1 -- no product of experts --, caption
// decoder with ONE row group and the squared error on it, and the backward chain.  The image half of the plan is not touched: no
// conv, dense or BatchNorm launch runs, its gradients stay at the zero the step's prologue wrote, its parameters and BatchNorm
// buffers are not written.  Everything runs on the caller's stream except what the 3-pass step also takes off the caption chain: the
// weight gradients, which only feed the optimizer (second weight-gradient stream; MMVAE_SERIAL: in order).
static int coco_text_step_body(CocoPlan* Pp, const mmvae_text_step_io& io, int training, int do_backward, hipStream_t s) {
    MMVAE_TRY(use_ws(Pp, io.ws, io.ws_bytes));
    CocoPlan& P = *Pp;
    CocoPlan::W& w = P.w;
    const int B = P.B, D = P.D, T = P.T;
    MMVAE_REQUIRE(io.text && io.sos && io.sums, "coco text step: text/sos/sums must be given");
    MMVAE_REQUIRE(launch_latent1_scratch_floats(B, D) <= (size_t)B * NPIX, "coco text step: no room for the latent block's partial sums");
    const float* eps = io.eps;
    const uint8_t* gk = io.gru_keep;
    StepBeginArgs sb{};
    sb.zero_ptr[0] = w.zero_begin; sb.zero_bytes[0] = w.zero_bytes;
    if (do_backward) {
        sb.zero_ptr[1] = P.buf.gpk; sb.zero_bytes[1] = (size_t)P.gk.mat_elems * sizeof(float);
        sb.zero_ptr[2] = P.buf.grads; sb.zero_bytes[2] = (size_t)(P.nparams / 4) * 16;
    }
    sb.p = DROP_P; sb.seed = io.seed; sb.step = io.step_counter;
    if (training && !eps) { sb.eps = w.eps; sb.n_eps = (long long)B * D; eps = w.eps; }
    if (training && io.gru_dropout && !gk) { sb.mask[2] = w.gkeep; sb.n_mask[2] = (long long)T * B * COCO_H; gk = w.gkeep; }
    if (!(training && io.gru_dropout)) gk = nullptr;
    MMVAE_TRY(launch_step_begin(sb, s));
    if (do_backward && P.nparams % 4 != 0)
        MMVAE_TRY(launch_fill_zero(P.buf.grads + (P.nparams / 4) * 4, (size_t)(P.nparams % 4) * sizeof(float), s));
    MMVAE_TRY(ensure_streams(P));
    const bool serial = mmvae_serial();
    hipStream_t Sw = serial ? s : P.st_wgrad2;
    if (io.pack_first && !P.no_pack)      // the caption half's packs only (the table's tail): the image half's are never read here
        MMVAE_TRY(launch_pack_range(P.buf.desc_dev, P.pk.d.data(), (int)P.pk.d.size(), P.pk_text_begin, (int)P.pk.d.size(), P.buf.params,
                                    P.buf.packed, P.buf.packed_vec, s));
    MMVAE_TRY(coco_text_enc_fwd(P, io.text, do_backward, w.txtout, s, true));
    Latent1Args la{};
    la.B = B; la.D = D; la.enc_out = w.txtout; la.eps = eps;
    la.mu = io.mu ? io.mu : w.mu; la.logvar = io.logvar ? io.logvar : w.logvar;
    la.z_f32 = w.z_f32; la.z_bf = w.z_bf; la.ldz = P.ldz; la.kl_sum = w.sums + 8; la.training = training;
    la.scratch = w.tmp_f32;         // (the module image decoder's sigmoid-backward buffer: nobody else's in this step)
    MMVAE_TRY(launch_latent1_fwd(la, s));
    float* sentence = io.recon_text ? io.recon_text : w.td_recon;
    {
        CocoMseFuse mf{};
        mf.coef[0] = io.lambda_y / ((float)B * (float)T * (float)COCO_E);
        mf.target = io.text; mf.loss_sum = w.sums; mf.dw = do_backward ? w.td_dw : nullptr; mf.dw16 = P.text_bf16 ? w.tb_dw16 : nullptr;
        MMVAE_TRY(coco_text_dec_fwd(P, w.z_f32, 1, io.sos, gk, do_backward, sentence, s, true, &mf));
        if (!P.mse_fused)
            MMVAE_TRY(coco_mse3(sentence, io.text, 1, (long long)B * T * COCO_E, mf.coef, w.sums, mf.dw, s));
        P.dw16_fresh = do_backward && P.mse_fused;
    }
    if (!do_backward) {
        hipLaunchKernelGGL(sum_slots_kernel, dim3(1), dim3(64), 0, s, w.sums, io.sums, P.cl_alarm_f, (const unsigned*)nullptr);
        return mmvae_check_launch("sum_slots");
    }
    // =============================== backward ===============================
    MMVAE_TRY(coco_text_dec_bwd(P, w.z_f32, 1, io.sos, gk, sentence, w.td_dw, w.dz_txt, s, Sw, true));
    Latent1BwdF32Args lb{};
    lb.B = B; lb.D = D; lb.mu = la.mu; lb.logvar = la.logvar; lb.eps = eps; lb.dz = w.dz_txt; lb.training = training;
    lb.kl_coef = io.kl_lambda / (float)B; lb.d_enc_out = w.d_txtout; lb.ld = 2 * D;
    MMVAE_TRY(launch_latent1_bwd_f32(lb, s));
    MMVAE_TRY(coco_text_enc_bwd(P, io.text, w.d_txtout, s, Sw, true));
    MMVAE_TRY(coco_text_dec_wgrads(P, Sw));          // (no-op: issued behind the encoder's BPTT launch)
    MMVAE_TRY(join_sides(P, s, s));
    if (io.defer_unpack) MMVAE_TRY(launch_wgrad_reduce(&P.slab, s));  // the packed gradients are complete; Adam gathers them
    else MMVAE_TRY(plan_unpack(P, s, true));
    // (last kernel of the step, as in coco_step_body: the mark of a void step in the gradient is not overwritten)
    hipLaunchKernelGGL(sum_slots_kernel, dim3(1), dim3(64), 0, s, w.sums, io.sums, P.cl_alarm_f, P.cl_alarm_b, io.optimizer_state, P.buf.grads);
    return mmvae_check_launch("sum_slots");
}
size_t coco_text_step_workspace_bytes(const CocoPlan* P) { return P->ws_bytes_module; }
int coco_text_step(CocoPlan* P, const mmvae_text_step_io& io, int training, int do_backward, hipStream_t s) {
    return plan_step(P, io, training, do_backward, s, coco_text_step_body);
}
// sum of squared errors of the particle rows' sentences alone: coco_iw_score without the image decoder (the same, smaller, carve)
int coco_iw_score_text(CocoPlan* P, void* ws, size_t wsb, const float* z, const float* text, const float* sos, int B, int K, float* sse_y,
                       hipStream_t s) {
    MMVAE_REQUIRE(P && z && text && sos && sse_y, "mmvae_coco_iw_score_text: null argument");
    MMVAE_REQUIRE(B >= 1 && K >= 1 && (long long)B * K <= P->B,
                  "mmvae_coco_iw_score_text: %d examples x %d particles exceed the plan's %d rows", B, K, P->B);
    MMVAE_TRY(use_ws_iw(P, ws, wsb));
    CocoPlan::W& w = P->w;
    const int rows = B * K;
    MMVAE_TRY(zero_ws(*P, s));
    const float* zt = z;
    if (rows < P->B) {    // the caption decoder runs the plan's rows: the rows behind the particles are zeros, as in coco_iw_score
        MMVAE_TRY(launch_fill_zero(w.z_f32, (size_t)P->B * P->D * sizeof(float), s));
        MMVAE_REQUIRE(hipMemcpyAsync(w.z_f32, z, (size_t)rows * P->D * sizeof(float), hipMemcpyDeviceToDevice, s) == hipSuccess,
                      "mmvae_coco_iw_score_text: copy of the particles failed");
        zt = w.z_f32;
    }
    MMVAE_TRY(coco_text_dec_fwd(*P, zt, 1, sos, nullptr, 0, w.td_recon, s));
    return launch_coco_iw_text_sse(w.td_recon, text, B, K, P->T, sse_y, s);
}

// ---------------------------------------------------------------- granular module entry points (drop-in modules)
int coco_image_encoder_fwd(CocoPlan* P, void* ws, size_t wsb, const float* image, const uint8_t* m1, const uint8_t* m2, int training,
                           float* out, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    MMVAE_TRY(zero_ws(*P, s));
    return enc_fwd(*P, image, 1, m1, m2, training && m1 != nullptr && m2 != nullptr, training, 1, out, s);
}
int coco_image_encoder_bwd(CocoPlan* P, void* ws, size_t wsb, const float* d_out, const uint8_t* m1, const uint8_t* m2, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    CocoPlan::W& w = P->w;
    const int rows = P->B, D2 = 2 * P->D;
    MMVAE_TRY(plan_zero_gpk(*P, s));
    MMVAE_TRY(launch_cast_bf16(d_out, (long long)rows * D2, w.d_encout, s));
    MMVAE_TRY(launch_colsum_f32(d_out, rows, D2, P->buf.grads + P->fc3.b_off, s));
    MMVAE_TRY(enc_bwd(*P, w.d_encout, 1, m1, m2, m1 != nullptr && m2 != nullptr, s));
    return plan_unpack(*P, s, true);
}
int coco_image_decoder_fwd(CocoPlan* P, void* ws, size_t wsb, const float* z, int training, float* recon, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    CocoPlan::W& w = P->w;
    const int rows = P->B;
    MMVAE_TRY(zero_ws(*P, s));
    hipLaunchKernelGGL(cast_z_kernel, dim3(ceil_div(rows * P->ldz, 256)), dim3(256), 0, s, z, rows, P->D, w.z_bf, P->ldz);
    MMVAE_TRY(mmvae_check_launch("cast_z"));
    ConvTLastFwdArgs last{};
    last.recon = recon;
    return dec_fwd(*P, 1, training, &last, s);
}
int coco_image_decoder_bwd(CocoPlan* P, void* ws, size_t wsb, const float* d_recon, const float* recon, float* dz, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    CocoPlan::W& w = P->w;
    const long long n = (long long)P->B * NPIX;
    MMVAE_TRY(plan_zero_gpk(*P, s));
    hipLaunchKernelGGL(sigmoid_bwd_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, d_recon, recon, n, w.tmp_f32);
    MMVAE_TRY(mmvae_check_launch("sigmoid_bwd"));
    MMVAE_TRY(tower_dec_bwd(*P, w.tmp_f32, 1, dz, s));
    return plan_unpack(*P, s, true);
}
// Caption modules.  Knob "coco_module_bf16" (0, test aid): 1 runs the bf16 persistent kernels of the training step
// (coco_text_bf16.hip) on the module's one group of B rows -- packed weights of the current parameters, zeroed packed gradient
// and its unpack around each backward, the decoder's weight gradients inline; 2 runs the forward kernels without saving
// anything for a backward pass (the SAVE = false instantiations), and the backward entries refuse.  0: the fp32 kernels of
// coco_text.hip, as before.
static int module_bf16() { return mmvae_knob(K_coco_module_bf16); }
static int module_pack(CocoPlan& P, hipStream_t s) {
    return launch_pack(P.buf.desc_dev, P.pk.d.data(), (int)P.pk.d.size(), P.buf.params, P.buf.packed, P.buf.packed_vec, s);
}
// A cluster launch that gave up waiting for a peer set its timeout word: element 0 of the result says so (the step: sum_slots_kernel)
static __global__ void module_alarm_kernel(const unsigned* alarm, float* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && *alarm) out[0] = __builtin_nanf("");
}
static int module_alarm(const unsigned* alarm, float* out, hipStream_t s) {
    if (!alarm) return MMVAE_OK;
    hipLaunchKernelGGL(module_alarm_kernel, dim3(1), dim3(64), 0, s, alarm, out);
    return mmvae_check_launch("module_alarm");
}
int coco_text_encoder_fwd(CocoPlan* P, void* ws, size_t wsb, const float* text, float* out, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    MMVAE_TRY(zero_ws(*P, s));
    const int mb = module_bf16();
    if (mb) {
        MMVAE_REQUIRE(P->text_bf16 && (mb == 1 || mb == 2), "coco_module_bf16 = %d: needs the bf16 caption kernels and a value of 0, 1 or 2", mb);
        MMVAE_TRY(module_pack(*P, s));
        return coco_text_enc_fwd(*P, text, mb == 1, out, s, true);
    }
    return coco_text_enc_fwd(*P, text, 1, out, s, false);
}
int coco_text_encoder_bwd(CocoPlan* P, void* ws, size_t wsb, const float* text, const float* d_out, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    const int mb = module_bf16();
    if (mb) {
        MMVAE_REQUIRE(P->text_bf16 && mb == 1, "coco_module_bf16 = %d: the forward pass saved nothing for a backward pass", mb);
        MMVAE_TRY(module_pack(*P, s));
        MMVAE_TRY(plan_zero_gpk(*P, s));
        MMVAE_TRY(coco_text_enc_bwd(*P, text, d_out, s, s, true));
        return plan_unpack(*P, s, true);
    }
    return coco_text_enc_bwd(*P, text, d_out, s, s, false);
}
int coco_text_decoder_fwd(CocoPlan* P, void* ws, size_t wsb, const float* z, const float* sos, const uint8_t* keep, int training,
                          float* sentence, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    MMVAE_TRY(zero_ws(*P, s));
    const int mb = module_bf16();
    if (mb) {
        MMVAE_REQUIRE(P->text_bf16 && (mb == 1 || mb == 2), "coco_module_bf16 = %d: needs the bf16 caption kernels and a value of 0, 1 or 2", mb);
        MMVAE_TRY(module_pack(*P, s));
        // (use_ws reset comb_fresh: the composed form makes W_comb of the current parameters inside coco_text_dec_fwd)
        MMVAE_TRY(coco_text_dec_fwd(*P, z, 1, sos, training ? keep : nullptr, mb == 1, sentence, s, true));
        return module_alarm(P->cl_alarm_f, sentence, s);
    }
    return coco_text_dec_fwd(*P, z, 1, sos, training ? keep : nullptr, 1, sentence, s);
}
int coco_text_decoder_bwd(CocoPlan* P, void* ws, size_t wsb, const float* z, const float* sos, const uint8_t* keep, const float* sentence,
                          const float* d_sentence, float* dz, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    CocoPlan::W& w = P->w;
    const size_t n = (size_t)P->B * P->T * COCO_E;
    const int mb = module_bf16();
    if (mb) {
        MMVAE_REQUIRE(P->text_bf16 && mb == 1, "coco_module_bf16 = %d: the forward pass saved nothing for a backward pass", mb);
        MMVAE_TRY(module_pack(*P, s));
        MMVAE_TRY(plan_zero_gpk(*P, s));
        MMVAE_REQUIRE(hipMemcpyAsync(w.td_dw, d_sentence, n * sizeof(float), hipMemcpyDeviceToDevice, s) == hipSuccess,
                      "coco_text_decoder_bwd: copy of the loss gradient failed");
        // use_ws left dw16_fresh and comb_fresh false: the composed BPTT makes its bf16 copy of the loss gradient and W_comb^T
        // itself; sw == s: the weight gradients are issued inline, into the packed gradient
        MMVAE_TRY(coco_text_dec_bwd(*P, z, 1, sos, keep, sentence, w.td_dw, dz, s, s, true));
        MMVAE_TRY(plan_unpack(*P, s, true));
        return module_alarm(P->cl_alarm_b, dz, s);
    }
    MMVAE_TRY(launch_fill_zero(w.td_dh0, (size_t)P->B * COCO_H * sizeof(float), s));
    MMVAE_TRY(launch_fill_zero(w.td_dh1, (size_t)P->B * COCO_H * sizeof(float), s));
    hipMemcpyAsync(w.td_dw, d_sentence, n * sizeof(float), hipMemcpyDeviceToDevice, s);
    return coco_text_dec_bwd(*P, z, 1, sos, keep, sentence, w.td_dw, dz, s, s);
}

// ---------------------------------------------------------------- importance-weighted evaluation (iw.h, coco_iw.hip)
// Eval-mode decoders on the B*K particle rows z [B][K][D].  Image: the bf16 decoder body of coco_image_decoder_fwd up to the raw
// output of hallucinate.6 (no stand-alone BatchNorm + Swish pass over it), then the forward-only scoring tail -- one log p(x|z)
// per row against the row's own example.  Caption: the launches of coco_text_decoder_fwd in eval mode (own-output feedback, no
// dropout, nothing saved for a backward pass) into the workspace's sentence buffer, then one squared-error sum per row.  No
// backward activation is kept; parameters, BatchNorm buffers and gradients are only read.
size_t coco_iw_workspace_bytes(const CocoPlan* P) { return P->ws_bytes_iw; }
int coco_iw_score(CocoPlan* P, void* ws, size_t wsb, const float* z, const float* image, const float* text, const float* sos, int B, int K,
                  float* loglik_x, float* sse_y, hipStream_t s) {
    MMVAE_REQUIRE(P && z && image && text && sos && loglik_x && sse_y, "mmvae_coco_iw_score: null argument");
    MMVAE_REQUIRE(B >= 1 && K >= 1 && (long long)B * K <= P->B,
                  "mmvae_coco_iw_score: %d examples x %d particles exceed the plan's %d rows", B, K, P->B);
    MMVAE_TRY(use_ws_iw(P, ws, wsb));
    CocoPlan::W& w = P->w;
    const int rows = B * K;
    MMVAE_TRY(zero_ws(*P, s));
    MMVAE_TRY(tower_iw_particles(*P, z, rows, s));
    const float* zt = z;
    if (rows < P->B) {    // the caption decoder runs the plan's rows as well: its fp32 particles get the same zero rows
        MMVAE_TRY(launch_fill_zero(w.z_f32, (size_t)P->B * P->D * sizeof(float), s));
        MMVAE_REQUIRE(hipMemcpyAsync(w.z_f32, z, (size_t)rows * P->D * sizeof(float), hipMemcpyDeviceToDevice, s) == hipSuccess,
                      "mmvae_coco_iw_score: copy of the particles failed");
        zt = w.z_f32;
    }
    MMVAE_TRY(dec_fwd(*P, 1, 0, nullptr, s));
    MMVAE_TRY(launch_coco_iw_tail(tower_iw_tail_args(*P, image, rows, K, loglik_x), s));
    MMVAE_TRY(coco_text_dec_fwd(*P, zt, 1, sos, nullptr, 0, w.td_recon, s));
    return launch_coco_iw_text_sse(w.td_recon, text, B, K, P->T, sse_y, s);
}

// ---------------------------------------------------------------- test / profiling aid: replay one launch of the step
// The tower's names (img_tower.h tower_named_gemm / tower_named_wgrad), fc2 / fc3 (+ _dgrad, _wgrad) and the stand-alone passes: enc_bn<l> /
// dec_bn<l> (+ _bwd), im2col_dlogit, dec_last_fwd.  The classifier runs its 2 dropout variants, the decoder 3 passes forward and
// backward (the default step), BatchNorm makes the running-statistics updates of the default step (encoder 2, decoder 1 per
// group).  Knob "coco_layer_mask" (0): the keep flags in W::m1 / W::m2 take part in fc1 / fc2 / fc3_dgrad / fc2_dgrad as in a step
// with classifier dropout.  fc3 writes encout; fc3_dgrad / fc3_wgrad read d_encout; fc3_dgrad and fc2_dgrad add, as in the step,
// their column sums to the bias gradients of classifier.3 / classifier.0 in the flat gradients; up_dgrad writes dz into dz_img.
// dec_last_fwd: target [B][3][32][32] in tmp_f32, loss weights (1, 1/2, 0) / (B * 3072), dlogit into dlogit, BCE sums into sums,
// logits [3B][3][32][32] at the start of the weight-gradient slab and recon right behind them.
static bool named_gemm(CocoPlan& P, const std::string& name, GemmParams& g) {
    CocoPlan::W& w = P.w;
    const bool masked = mmvae_knob(K_coco_layer_mask) != 0;
    const uint8_t *m1 = masked ? w.m1 : nullptr, *m2 = masked ? w.m2 : nullptr;
    if (name == "fc2") { g = layer_gemm(P, CO_FC2, 2, m2); return true; }
    if (name == "fc3") { g = layer_gemm(P, CO_FC3, 2, nullptr, w.encout); return true; }
    if (name == "fc3_dgrad") { g = layer_gemm(P, CO_FC3_DGRAD, 2, m2, w.d_encout); return true; }
    if (name == "fc2_dgrad") { g = layer_gemm(P, CO_FC2_DGRAD, 2, m1); return true; }
    GatherTransform tr{};      // (no staged names here: never filled)
    return tower_named_gemm(P, name, m1, w.dz_img, false, g, tr);
}
static bool named_wgrad(CocoPlan& P, const std::string& name, WgradParams& g) {
    if (name == "fc2_wgrad") { g = layer_wgrad(P, CO_W_FC2, 2); return true; }
    if (name == "fc3_wgrad") { g = layer_wgrad(P, CO_W_FC3, 2, P.w.d_encout); return true; }
    return tower_named_wgrad(P, name, g);
}
// 1: launched, 0: not a stand-alone pass, < 0: error
static int named_pass(CocoPlan& P, const std::string& name, hipStream_t s) {
    CocoPlan::W& w = P.w;
    for (int l = 1; l < 4; ++l) {
        const std::string n = "enc_bn" + std::to_string(l + 1);
        if (name == n) { const int rc = enc_bn_act(P, l, 2, 1, s); return rc == MMVAE_OK ? 1 : rc; }
        if (name == n + "_bwd") { const int rc = launch_bn_bwd_apply(enc_bn_bwd_args(P, l, 2), s); return rc == MMVAE_OK ? 1 : rc; }
    }
    for (int l = 0; l < 3; ++l) {
        const std::string n = "dec_bn" + std::to_string(l + 1);
        if (name == n) { P.dec_skip_mask = 0; const int rc = dec_bn_act(P, l, 3, 1, s); return rc == MMVAE_OK ? 1 : rc; }
        if (name == n + "_bwd") { const int rc = launch_bn_bwd_apply(dec_bn_bwd_args(P, l, 3), s); return rc == MMVAE_OK ? 1 : rc; }
    }
    if (name == "im2col_dlogit") { const int rc = im2col_dlogit(P, w.dlogit, 3, s); return rc == MMVAE_OK ? 1 : rc; }
    if (name == "dec_last_fwd") {
        const size_t n3 = (size_t)3 * P.B * NPIX;
        if (w.slab_floats < 2 * n3) { mmvae_set_error("mmvae_coco_bench_layer: dec_last_fwd needs %zu floats of the slab", 2 * n3); return MMVAE_EINVAL; }
        ConvTLastFwdArgs last{};
        last.target = w.tmp_f32; last.logits = w.slab; last.recon = w.slab + n3; last.dlogit = w.dlogit; last.loss_sum = w.sums;
        const float lam[3] = {1.f, 0.5f, 0.f};
        for (int k = 0; k < 3; ++k) last.coef[k] = lam[k] / (float)(P.B * NPIX);
        const int rc = launch_convt_last_fwd(dec_last_args(P, last, 3), s);
        return rc == MMVAE_OK ? 1 : rc;
    }
    return 0;
}
int coco_bench_layer(CocoPlan* P, void* ws, size_t wsb, const char* layer, int iters, hipStream_t s) {
    MMVAE_REQUIRE(P && layer, "mmvae_coco_bench_layer: null argument");
    MMVAE_TRY(use_ws(P, ws, wsb, false));
    WgradParams wg{};
    if (named_wgrad(*P, layer, wg)) return tower_replay_wgrad(*P, wg, iters, s);
    GemmParams g{};
    if (named_gemm(*P, layer, g)) {
        for (int i = 0; i < iters; ++i) MMVAE_TRY(launch_gemm_gather(g, s));
        return MMVAE_OK;
    }
    for (int i = 0; i < iters; ++i) {
        const int rc = named_pass(*P, layer, s);
        MMVAE_REQUIRE(rc != 0, "mmvae_coco_bench_layer: unknown layer '%s'", layer);
        if (rc < 0) return rc;
    }
    return MMVAE_OK;
}
// byte offset of a named workspace buffer of the fused step's carving (3 passes), -1 if unknown
long long coco_debug_offset(CocoPlan* P, const char* name) {
    if (!P || !name) return -1;
    if (std::strncmp(name, "infovae_step:", 13) == 0) {      // the InfoVAE step's own buffers behind the one-pass carve
        const InfoVaeCarve c = infovae_carve(P);
        const std::string n = name + 13;
        return n == "mmd_ws" ? (long long)c.ws_off : n == "dz_mmd" ? (long long)c.dz_off : n == "true_samples" ? (long long)c.drawn_off : -1;
    }
    Workspace ws((void*)0x1000, (size_t)1 << 40);      // (every call that works in a workspace carves its own again: plan_use_ws)
    P->carve_passes = 3; P->carve_iw = false;
    carve(*P, ws);
    CocoPlan::W& w = P->w;
    std::map<std::string, const void*> m = tower_debug_names(w);
    m.insert({{"y2", w.y2}, {"ay2", w.ay2}, {"encout", w.encout}, {"m1", w.m1}, {"m2", w.m2}, {"z_f32", w.z_f32}, {"dz_img", w.dz_img},
              {"d_encout", w.d_encout}, {"dy2", w.dy2}, {"tmp_f32", w.tmp_f32}, {"sums", w.sums}});
    return tower_offset_of(m, name, (const void*)0x1000);
}
