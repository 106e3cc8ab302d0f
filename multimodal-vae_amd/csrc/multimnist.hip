// MultiMNIST MMVAE: layer plans, weight-pack tables and the kernel sequences of the ELBO step.
// Reference: multimnist/model.py:21-93 (MultimodalVAE), :150-216 (image enc/dec), :219-307 (text enc/dec),
//            multimnist/train.py:69-87 (loss_function), :146-173 (3-pass step).
#include "multimnist.h"
#include <memory>
#include "mlp_tail.h"
#include "plan_base.h"
#include "thin.h"
#include "text_plan.h"
#include <cstring>

namespace {
constexpr int IMG = 50, NPIX = 2500;
}

struct MMPlan : PlanBase {
    int ldz, kx, kz;
    int lde;        // row stride of the bf16 gradient of the image encoder's output [rows][2D]: round_up(2D, 8), pad columns zero
    ConvL conv[4], convT[4];
    LinL fc[3], up;
    BnL bn[6];
    // text packs (text_plan.h)
    int H = TXT_H;
    const char *te_name = "text_encoder", *td_name = "text_decoder";
    TextGruIdx te_f, te_r, td0, td1;
    const float* step_image = nullptr;      // the image batch of the running fused step (conv1's weight gradient rebuilds its patches)
    hipEvent_t ev_dz = nullptr;             // fused step: completion of the text decoder's backward kernel (what the main chain joins on)
    hipEvent_t ev_txtgrads = nullptr;       // fused step: every gradient of text_decoder.* is complete (recorded on the second-modality stream)
    int te_h2p, te_h2pT, g_te_h2p, td_z2h, td_z2hT, g_td_z2h, td_h2o, td_h2oT, g_td_h2o;
    // fused classifier tail (mlp_tail.hip; n_latents = 100 only): fragment-major copies of classifier.3 / classifier.6
    bool mlp_tail = false;
    int mt_w2, mt_w3, mt_w3t, mt_w2t;
    // one-expert waist of the image-only step (mlp_tail.hip; n_latents = 20 and 100): the same four copies, classifier.6's at the
    // widths of 2D (at n_latents = 100 they ARE the mt_ ones)
    bool waist = false;
    int wa_w2, wa_w3, wa_w3t, wa_w2t;
    // ---- workspace pointers
    struct W {
        char* zero_begin; size_t zero_bytes;
        float2 *st_e[3], *red_e[3], *st_d[3], *red_d[3];
        float* sums; float* dz_img; float* dz_txt;
        float2 *aff_e[3], *mr_e[3], *aff_d[3], *mr_d[3];
        bf16 *patches1, *r1, *r2, *r3, *r4, *y1, *y2;
        bf16 *a1, *a2, *a3, *a4, *ay1, *ay2, *au, *aq1, *aq2, *aq3;
        float* encout; uint8_t *m1, *m2, *gkeep;
        float *txtout, *te_gates_f, *te_gates_r; bf16 *te_x, *te_hprev, *te_hsum;
        float *eps, *mu, *logvar, *z_f32; bf16* z_bf;
        bf16 *u, *q1, *q2, *q3; float *logits, *recon, *dlogit;
        float *words, *dwords, *td_gates; long long* tokens;
        bf16 *td_x0, *td_h0p, *td_mid, *td_h1p, *td_hz, *td_zbf;
        bf16 *dgi0, *dgh0, *dgi1, *dgh1, *dlogit_bf, *dhinit;
        bf16 *patches4, *d3, *d2, *d1, *du;
        bf16 *d_encout; float* d_txtout; bf16* te_dout_bf; bf16 *te_dgi_f, *te_dgh_f, *te_dgi_r;
        bf16 *dy2, *dy1, *db4, *dr4, *d3e, *d2e, *d1e;
        bf16 *d3r, *d2r, *d1r, *d3er, *d2er;       // BatchNorm-backward outputs kept apart from db (fused staging: see dec_bwd / enc_bwd)
        float* tmp_f32;
        float* slab; size_t slab_floats;
    } w;
};

namespace {

void build_params(MMPlan& P) {
    const int D = P.D;
    auto bn = [&](const std::string& n, int c) { add_param(P, n + ".weight", {c}); add_param(P, n + ".bias", {c}); };
    add_param(P, "image_encoder.features.0.weight", {32, 1, 4, 4});
    add_param(P, "image_encoder.features.2.weight", {64, 32, 4, 4}); bn("image_encoder.features.3", 64);
    add_param(P, "image_encoder.features.5.weight", {128, 64, 4, 4}); bn("image_encoder.features.6", 128);
    add_param(P, "image_encoder.features.8.weight", {256, 128, 4, 4}); bn("image_encoder.features.9", 256);
    add_param(P, "image_encoder.classifier.0.weight", {400, 1024}); add_param(P, "image_encoder.classifier.0.bias", {400});
    add_param(P, "image_encoder.classifier.3.weight", {200, 400}); add_param(P, "image_encoder.classifier.3.bias", {200});
    add_param(P, "image_encoder.classifier.6.weight", {2 * D, 200}); add_param(P, "image_encoder.classifier.6.bias", {2 * D});
    add_param(P, "image_decoder.upsample.0.weight", {1024, D}); add_param(P, "image_decoder.upsample.0.bias", {1024});
    add_param(P, "image_decoder.hallucinate.0.weight", {256, 128, 4, 4}); bn("image_decoder.hallucinate.1", 128);
    add_param(P, "image_decoder.hallucinate.3.weight", {128, 64, 4, 4}); bn("image_decoder.hallucinate.4", 64);
    add_param(P, "image_decoder.hallucinate.6.weight", {64, 32, 5, 5}); bn("image_decoder.hallucinate.7", 32);
    add_param(P, "image_decoder.hallucinate.9.weight", {32, 1, 4, 4});
    text_add_encoder_params(P);
    text_add_decoder_params(P);
}

void build_plan(MMPlan& P) {
    const int D = P.D;
    P.ldz = round_up(D + 1, 8); P.kz = round_up(D, 32); P.kx = txt_kx(P.H, D);
    P.lde = round_up(2 * D, 8);
    build_params(P);
    // BatchNorm tables (state_dict order)
    const char* bnn[6] = {"image_encoder.features.3", "image_encoder.features.6", "image_encoder.features.9",
                          "image_decoder.hallucinate.1", "image_decoder.hallucinate.4", "image_decoder.hallucinate.7"};
    const int bnc[6] = {64, 128, 256, 128, 64, 32};
    long long so = 0;
    for (int i = 0; i < 6; ++i) {
        P.bn[i] = BnL{off(P, std::string(bnn[i]) + ".weight"), off(P, std::string(bnn[i]) + ".bias"), bnc[i], so, i};
        P.bn_names.push_back(bnn[i]); P.bn_list.push_back(P.bn[i]);
        so += 2 * bnc[i];
    }
    // encoder convs (multimnist/model.py:160-169)
    build_conv(P, P.conv[0], "image_encoder.features.0.weight", ConvGeom{1, 32, 4, 4, 2, 1, 50, 50, 25, 25, false}, -1, false, true, false);
    build_conv(P, P.conv[1], "image_encoder.features.2.weight", ConvGeom{32, 64, 4, 4, 2, 1, 25, 25, 12, 12, false}, 0, true, false, false);
    build_conv(P, P.conv[2], "image_encoder.features.5.weight", ConvGeom{64, 128, 4, 4, 2, 1, 12, 12, 6, 6, false}, 1, true, false, false);
    build_conv(P, P.conv[3], "image_encoder.features.8.weight", ConvGeom{128, 256, 4, 4, 2, 0, 6, 6, 2, 2, false}, 2, true, false, false);
    // decoder transposed convs (multimnist/model.py:199-208)
    build_conv(P, P.convT[0], "image_decoder.hallucinate.0.weight", ConvGeom{256, 128, 4, 4, 2, 0, 2, 2, 6, 6, true}, 3, true, false, false);
    build_conv(P, P.convT[1], "image_decoder.hallucinate.3.weight", ConvGeom{128, 64, 4, 4, 2, 1, 6, 6, 12, 12, true}, 4, true, false, false);
    build_conv(P, P.convT[2], "image_decoder.hallucinate.6.weight", ConvGeom{64, 32, 5, 5, 2, 1, 12, 12, 25, 25, true}, 5, true, false, false);
    build_conv(P, P.convT[3], "image_decoder.hallucinate.9.weight", ConvGeom{32, 1, 4, 4, 2, 1, 25, 25, 50, 50, true}, -1, true, false, true);
    add_frag_packs(P, P.conv[2]);      // 6x6 / 12x12 layers with 64-256 KB of weights per class: direct-B kernels (convres.hip)
    add_frag_packs(P, P.convT[1]);
    add_frag_packs(P, P.conv[3]);      // the 2x2 <-> 6x6 bottleneck layers (1 MB of weights each)
    add_frag_packs(P, P.convT[0]);

    // classifier (multimnist/model.py:173-179). fc1 consumes the NCHW flatten c*4+y*2+x of a (256,2,2) map that
    // lives here as NHWC [2][2][256]: a 2x2-tap gather with k = (y*2+x)*256 + c.
    {
        LinL& f = P.fc[0];
        f.w_off = off(P, "image_encoder.classifier.0.weight"); f.b_off = off(P, "image_encoder.classifier.0.bias");
        f.N = 400; f.K = 1024; f.pk_dgrad = -1;
        PackDesc d = pack_dense(f.w_off, 400, 1024, npad_for(400), 1024, 1024, 0);
        d.TW = 2; d.C = 256; d.s_ty = 2; d.s_tx = 1; d.s_c = 4;
        f.pk_fwd = P.pk.add(d);
        PackDesc gd = d; gd.Npad = round_up(400, 64);
        f.gk = P.gk.add(gd);
        // dgrad: one class per pixel s of the 2x2 map: da[n][s][c] = sum_j dy[n][j] * W[j][c*4+s]
        for (int sidx = 0; sidx < 4; ++sidx)
            f.pk_dgrad4[sidx] = P.pk.add(pack_dense(f.w_off + sidx, 256, 400, npad_for(256), round_up(400, 64), 4, 1024));
    }
    auto lin = [&](LinL& f, const std::string& n, int N, int K) {
        f.w_off = off(P, n + ".weight"); f.b_off = off(P, n + ".bias"); f.N = N; f.K = K;
        f.pk_fwd = P.pk.add(pack_dense(f.w_off, N, K, npad_for(N), round_up(round_up(K, 8), 64), K, 1));
        f.gk = P.gk.add(pack_dense(f.w_off, N, K, round_up(N, 64), round_up(round_up(K, 8), 64), K, 1));
        f.pk_dgrad = P.pk.add(pack_dense(f.w_off, K, N, npad_for(K), round_up(round_up(N, 8), 64), 1, K));
    };
    lin(P.fc[1], "image_encoder.classifier.3", 200, 400);
    lin(P.fc[2], "image_encoder.classifier.6", 2 * D, 200);
    if (D == 100) {      // the widths mlp_tail.hip is compiled for
        P.mlp_tail = true;
        auto fragd = [&](PackDesc d) { d.frag = 1; return P.pk.add(d); };
        P.mt_w2 = fragd(pack_dense(P.fc[1].w_off, 200, 400, 208, 416, 400, 1));
        P.mt_w3 = fragd(pack_dense(P.fc[2].w_off, 200, 200, 208, 224, 200, 1));
        P.mt_w3t = fragd(pack_dense(P.fc[2].w_off, 200, 200, 208, 224, 1, 200));    // [fc2 unit][fc3 output]
        P.mt_w2t = fragd(pack_dense(P.fc[1].w_off, 400, 200, 400, 224, 1, 400));    // [fc1 unit][fc2 unit]
        P.waist = true; P.wa_w2 = P.mt_w2; P.wa_w3 = P.mt_w3; P.wa_w3t = P.mt_w3t; P.wa_w2t = P.mt_w2t;
    } else if (mlp2_latent1_compiled(D)) {      // n_latents = 20: read by the image-only step alone (mm_image_step_body)
        P.waist = true;
        auto fragd = [&](PackDesc d) { d.frag = 1; return P.pk.add(d); };
        P.wa_w2 = fragd(pack_dense(P.fc[1].w_off, 200, 400, 208, 416, 400, 1));
        P.wa_w3 = fragd(pack_dense(P.fc[2].w_off, 2 * D, 200, round_up(2 * D, 16), 224, 200, 1));
        P.wa_w3t = fragd(pack_dense(P.fc[2].w_off, 200, 2 * D, 208, round_up(2 * D, 32), 1, 200));      // [fc2 unit][fc3 output]
        P.wa_w2t = fragd(pack_dense(P.fc[1].w_off, 400, 200, 400, 224, 1, 400));                        // [fc1 unit][fc2 unit]
    }
    {   // upsample Linear(D, 1024): output columns permuted to NHWC n' = s*256 + c  <->  row c*4 + s
        LinL& f = P.up;
        f.w_off = off(P, "image_decoder.upsample.0.weight"); f.b_off = off(P, "image_decoder.upsample.0.bias");
        f.N = 1024; f.K = D;
        // the bias rides in packed column D (the operand z carries a 1.0 there), so its permutation and its
        // gradient (column D of the packed weight gradient) come for free
        PackDesc d = pack_dense(f.w_off, 1024, D, npad_for(1024), round_up(P.ldz, 64), 0, 1);
        d.NL = 256; d.s_nhi = D; d.s_nlo = 4 * D;
        d.bias_off = f.b_off; d.b_nhi = 1; d.b_nlo = 4;
        f.pk_fwd = P.pk.add(d);
        PackDesc gd = d; f.gk = P.gk.add(gd);
        // dgrad: dz[rows][D] = du[rows][1024 NHWC] x W_D[D][1024]
        PackDesc t = pack_dense(f.w_off, D, 1024, npad_for(D), 1024, 1, 0);
        t.TW = 4; t.C = 256; t.s_ty = 0; t.s_tx = D; t.s_c = 4 * D;
        f.pk_dgrad = P.pk.add(t);
    }
    text_build_packs(P);       // the row-tile kernels' packs (text_plan.h)
    // Stage of the fused step that refreshes each bf16 copy after an optimizer step (mm_step_body; PackDesc::part of the WEIGHT table):
    //   0  the prologue on the main stream: what the image encoder's FORWARD reads (it starts right behind the prologue)
    //   1  the second-modality stream, in front of the text encoder: every text_encoder.* / text_decoder.* copy
    //   2  the second-modality stream, behind the text encoder's forward: image_decoder.* and the copies only the image encoder's
    //      BACKWARD reads (data-gradient forms) -- the main chain joins that stream before the product of experts, long before it needs them
    // The gather that makes these copies is the slowest part of the prologue (12 of 26 us on the main chain with everything in stage 0).
    for (PackDesc& d : P.pk.d) {
        d.part = 0;
        for (const ParamInfo& pi : P.params)
            if (d.src_off >= pi.offset && d.src_off < pi.offset + pi.numel)
                d.part = pi.name.rfind("text_", 0) == 0 ? 1 : pi.name.rfind("image_decoder.", 0) == 0 ? 2 : 0;
    }
    {
        auto late = [&](int idx) { if (idx >= 0) P.pk.d[idx].part = 2; };
        for (int l = 0; l < 4; ++l)
            for (int i = 0; i < 4; ++i) { late(P.conv[l].pk_dgrad[i]); late(P.conv[l].pk_dgrad_f[i]); }
        for (int i = 0; i < 4; ++i) late(P.fc[0].pk_dgrad4[i]);
        late(P.fc[1].pk_dgrad); late(P.fc[2].pk_dgrad);
        if (P.waist) { late(P.wa_w3t); late(P.wa_w2t); }
    }
    // gradient descriptors of the decoders (image_decoder.*, text_decoder.*): complete before the encoders' backward has run
    // (mmvae_mm_step_io::dp_split scatters them into the flat gradient buffer early)
    for (PackDesc& d : P.gk.d)
        for (const ParamInfo& pi : P.params)
            if (d.src_off >= pi.offset && d.src_off < pi.offset + pi.numel)
                d.part = pi.name.rfind("image_decoder.", 0) == 0 || pi.name.rfind("text_decoder.", 0) == 0;
}

// ------------------------------------------------------------------ workspace
void carve(MMPlan& P, Workspace& ws) {
    MMPlan::W& w = P.w;
    const size_t B = P.B, D = P.D, B3 = (size_t)P.carve_passes * B, B2 = (size_t)(P.carve_passes < 2 ? P.carve_passes : 2) * B;
    char* z0 = ws.take<char>(0);
    const int ec[3] = {64, 128, 256}, dc[3] = {128, 64, 32};
    const int SS = MMVAE_STAT_SLOTS;
    for (int i = 0; i < 3; ++i) { w.st_e[i] = ws.take<float2>(SS * ec[i]); w.red_e[i] = ws.take<float2>(SS * ec[i]); }
    for (int i = 0; i < 3; ++i) { w.st_d[i] = ws.take<float2>(3 * SS * dc[i]); w.red_d[i] = ws.take<float2>(3 * SS * dc[i]); }
    w.sums = ws.take<float>(16 * MMVAE_LOSS_SLOTS);
    P.sk_cnt = ws.take<unsigned>(1024);
    w.dz_img = ws.take<float>(B3 * D);
    w.dz_txt = ws.take<float>(B3 * D);
    char* z1 = ws.take<char>(0);
    w.zero_begin = z0; w.zero_bytes = (size_t)(z1 - z0);
    for (int i = 0; i < 3; ++i) { w.aff_e[i] = ws.take<float2>(ec[i]); w.mr_e[i] = ws.take<float2>(ec[i]); }
    for (int i = 0; i < 3; ++i) { w.aff_d[i] = ws.take<float2>(3 * dc[i]); w.mr_d[i] = ws.take<float2>(3 * dc[i]); }
    w.patches1 = ws.take<bf16>(B * 625 * 16);
    w.r1 = ws.take<bf16>(B * 625 * 32); w.r2 = ws.take<bf16>(B * 144 * 64); w.r3 = ws.take<bf16>(B * 36 * 128);
    w.r4 = ws.take<bf16>(B * 4 * 256);
    w.y1 = ws.take<bf16>(B2 * 400); w.y2 = ws.take<bf16>(B2 * 200);
    w.a1 = ws.take<bf16>(B * 625 * 32); w.a2 = ws.take<bf16>(B * 144 * 64); w.a3 = ws.take<bf16>(B * 36 * 128);
    w.a4 = ws.take<bf16>(B * 4 * 256); w.ay1 = ws.take<bf16>(B2 * 400); w.ay2 = ws.take<bf16>(B2 * 200);
    w.au = ws.take<bf16>(B3 * 1024); w.aq1 = ws.take<bf16>(B3 * 36 * 128); w.aq2 = ws.take<bf16>(B3 * 144 * 64);
    w.aq3 = ws.take<bf16>(B3 * 625 * 32);
    w.encout = ws.take<float>(B2 * 2 * D);
    w.m1 = ws.take<uint8_t>(B2 * 400); w.m2 = ws.take<uint8_t>(B2 * 200); w.gkeep = ws.take<uint8_t>(4 * B3 * P.H);
    carve_text_enc(w, ws, B, D, P.H);
    w.eps = ws.take<float>(B3 * D); w.mu = ws.take<float>(B3 * D); w.logvar = ws.take<float>(B3 * D);
    w.z_f32 = ws.take<float>(B3 * D); w.z_bf = ws.take<bf16>(B3 * P.ldz);
    w.u = ws.take<bf16>(B3 * 1024); w.q1 = ws.take<bf16>(B3 * 36 * 128); w.q2 = ws.take<bf16>(B3 * 144 * 64);
    w.q3 = ws.take<bf16>(B3 * 625 * 32);
    w.logits = ws.take<float>(B3 * NPIX); w.recon = ws.take<float>(B3 * NPIX); w.dlogit = ws.take<float>(B3 * NPIX);
    carve_text_dec(w, ws, B3, P.H, P.kx, P.kz);
    w.patches4 = ws.take<bf16>(B3 * 625 * 16);
    w.d3 = ws.take<bf16>(B3 * 625 * 32); w.d2 = ws.take<bf16>(B3 * 144 * 64); w.d1 = ws.take<bf16>(B3 * 36 * 128);
    w.du = ws.take<bf16>(B3 * 1024);
    w.d_encout = ws.take<bf16>(B2 * P.lde);
    carve_text_enc_bwd(w, ws, B, D, P.H);
    w.dy2 = ws.take<bf16>(B2 * 200); w.dy1 = ws.take<bf16>(B2 * 400);
    w.db4 = ws.take<bf16>(B2 * 1024); w.dr4 = ws.take<bf16>(B * 1024);
    w.d3e = ws.take<bf16>(B * 36 * 128); w.d2e = ws.take<bf16>(B * 144 * 64); w.d1e = ws.take<bf16>(B * 625 * 32);
    w.d3r = ws.take<bf16>(B3 * 625 * 32); w.d2r = ws.take<bf16>(B3 * 144 * 64); w.d1r = ws.take<bf16>(B3 * 36 * 128);
    w.d3er = ws.take<bf16>(B * 36 * 128); w.d2er = ws.take<bf16>(B * 144 * 64);
    w.tmp_f32 = ws.take<float>(B3 * NPIX);
    P.sk_floats = (size_t)256 * 128 * 128;                 // split-K partial slabs (fully overwritten, never zeroed)
    P.sk_buf = ws.take<float>(P.sk_floats);
    // weight-gradient partial-tile slabs (written and read once per step, never zeroed): gemm.h WgradSlabCtx
    w.slab_floats = (size_t)(P.carve_passes >= 3 ? 48 : 16) << 20;
    w.slab = ws.take<float>(w.slab_floats);
}

// ================================================================== launch arguments
// ONE definition per launch, as in img_tower.h: every GemmParams / WgradParams and the arguments of every stand-alone pass of
// the image half are built here, for the step (enc_fwd / enc_bwd / dec_fwd / dec_bwd / fused_tail) and for the replay of one
// launch on a test's own operands (mm_bench_layer): a test cannot pass on a copy of the parameters that drifted from the step.

// the tensors along the two conv chains, by layer: raw / activated / gradient; drr / dqr: the BatchNorm-backward outputs the fused
// step keeps apart from db (see enc_bwd / dec_bwd)
struct MMChains { bf16 *r[4], *a[4], *dr[4], *drr[4], *q[4], *aq[4], *dq[4], *dqr[4]; };
MMChains mm_chains(const MMPlan::W& w) {
    return MMChains{{w.r1, w.r2, w.r3, w.r4}, {w.a1, w.a2, w.a3, w.a4}, {w.d1e, w.d2e, w.d3e, w.dr4}, {nullptr, w.d2er, w.d3er, nullptr},
                    {w.u, w.q1, w.q2, w.q3}, {w.au, w.aq1, w.aq2, w.aq3}, {w.du, w.d1, w.d2, w.d3}, {nullptr, w.d1r, w.d2r, w.d3r}};
}

// l: layer index (conv[l] / convT[l]); n: row blocks -- dropout variants of the classifier, BatchNorm groups (passes) of the decoder.
enum MMGemm { MM_ENC_CONV1, MM_ENC_CONV, MM_ENC_CONV_DGRAD, MM_FC1, MM_FC1_DGRAD, MM_FC2, MM_FC3, MM_FC3_DGRAD, MM_FC2_DGRAD, MM_UP, MM_UP_DGRAD,
              MM_DEC_CONVT, MM_DEC_CONVT_DGRAD, MM_DEC_LAST_DGRAD };
enum MMWgrad { MM_W_ENC_CONV1, MM_W_ENC_CONV, MM_W_FC1, MM_W_FC2, MM_W_FC3, MM_W_UP, MM_W_DEC_CONVT, MM_W_DEC_LAST };

// classifier.0 over the NHWC 2x2x256 feature map the variants share: a 2x2-tap gather
GatherPlan fc1_plan(int rows) { return plan_fwdform(2, 2, 1, 1, 256, 2, 2, 1, 0, 400, 1, rows); }

// training: column statistics of the conv layers; mask: keep flags of the Dropout behind the layer (MM_FC1, MM_FC2) or behind the
// layer whose input gradient this is (MM_FC3_DGRAD: classifier.3's, MM_FC2_DGRAD: classifier.0's), or null.
// aux: MM_FC3 the fp32 result [n*B][2D]; MM_UP_DGRAD the fp32 result dz [n*B][D]; MM_FC3_DGRAD the operand d_out, bf16 [n*B][lde]
// with columns 2D.. zero (the generic kernels read their operands in 8-column vectors; 2D is a multiple of 8 only when n_latents
// is a multiple of 4).  colsum (MM_FC3_DGRAD, MM_FC2_DGRAD): where the column sums of the result go; null: the bias gradient of
// the layer below, classifier.3's / classifier.0's
GemmParams mm_gemm(MMPlan& P, MMGemm kind, int l, int n, int training = 1, const uint8_t* mask = nullptr, const void* aux = nullptr,
                   float* colsum = nullptr) {
    MMPlan::W& w = P.w;
    const MMChains t = mm_chains(w);
    const int B = P.B, rows = n * B, rows1 = B * 625;
    const float ms = 1.f / (1.f - DROP_P);
    // a dense layer: `groups` blocks of group_n rows with K operand columns, N outputs
    auto dense = [&](const int* pk, int groups, int group_n, int K, int N) { return gemm_of(P, dense_plan(group_n, K, K, N), pk, groups, group_n); };
    GemmParams g{};
    switch (kind) {
    case MM_ENC_CONV1:   // conv1 over the im2col patches + Swish (no BatchNorm): the epilogue emits raw and activated
        g = dense(P.conv[0].pk_fwd, 1, rows1, 16, 32);
        g.c.A = w.patches1; g.out_bf = w.r1; g.ldo = 32; g.out_act_bf = w.a1; g.e_act = ACT_SWISH;
        break;
    case MM_ENC_CONV: {
        const ConvL& L = P.conv[l];
        g = gemm_of(P, L.fwd, L.pk_fwd, 1, B, L.pk_fwd_f);
        g.c.A = t.a[l - 1]; g.out_bf = t.r[l]; g.ldo = L.g.Cout;
        g.colstats = training ? w.st_e[l - 1] : nullptr;
        break;
    }
    case MM_ENC_CONV_DGRAD: {   // class form, with the d-activation of the producer layer fused in the epilogue
        const ConvL& L = P.conv[l];
        g = gemm_of(P, L.dgrad, L.pk_dgrad, 1, B, L.pk_dgrad_f);
        g.c.A = t.dr[l]; g.out_bf = t.dr[l - 1]; g.ldo = L.g.Cin;
        g.d_r = t.r[l - 1]; g.d_ld = L.g.Cin; g.d_act = ACT_SWISH;
        if (l > 1) { g.d_affine = w.aff_e[l - 2]; g.d_meanrstd = w.mr_e[l - 2]; g.d_red = w.red_e[l - 2]; }
        break;
    }
    case MM_FC1:
        g = gemm_of(P, fc1_plan(rows), &P.fc[0].pk_fwd, 1, rows);
        g.c.A = w.a4; g.c.a_bcast_n = B;
        g.bias = P.buf.params + P.fc[0].b_off; g.out_bf = w.y1; g.ldo = 400;
        g.out_act_bf = w.ay1; g.e_act = ACT_SWISH; if (mask) { g.e_mask = mask; g.e_mask_scale = ms; }
        break;
    case MM_FC1_DGRAD: {
        // 4 classes = the 4 pixels of the 2x2 map, each with its own [256][400] matrix; the NHWC gradients of `rows` samples (both
        // dropout variants) against the map the B images share, with the BatchNorm-backward sums of conv4
        GatherPlan pd{};
        pd.c.AH = 1; pd.c.AW = 1; pd.c.Ald = 400; pd.c.C = 400; pd.c.sy = pd.c.sx = 1; pd.c.dy = pd.c.dx = 1;
        pd.c.OH = 2; pd.c.OW = 2; pd.c.osy = pd.c.osx = 1; pd.c.N = 256; pd.c.nclasses = 4;
        for (int sidx = 0; sidx < 4; ++sidx) {
            GatherClass& k = pd.cls[sidx];
            k.OY = 1; k.OX = 1; k.TH = 1; k.TW = 1; k.offy = 0; k.offx = 0; k.ooy = sidx / 2; k.oox = sidx % 2;
            k.K = 400; k.Kpad = round_up(400, 64);
        }
        g = gemm_of(P, pd, P.fc[0].pk_dgrad4, 1, rows);
        g.c.A = w.dy1; g.out_bf = w.db4; g.ldo = 256;
        g.d_r = w.r4; g.d_ld = 256; g.d_bcast_n = B; g.d_act = ACT_SWISH;
        g.d_affine = w.aff_e[2]; g.d_meanrstd = w.mr_e[2]; g.d_red = w.red_e[2];
        break;
    }
    case MM_FC2:
        g = dense(&P.fc[1].pk_fwd, 1, rows, 400, 200);
        g.c.A = w.ay1; g.bias = P.buf.params + P.fc[1].b_off; g.out_bf = w.y2; g.ldo = 200;
        g.out_act_bf = w.ay2; g.e_act = ACT_SWISH; if (mask) { g.e_mask = mask; g.e_mask_scale = ms; }
        break;
    case MM_FC3:
        g = dense(&P.fc[2].pk_fwd, 1, rows, 200, 2 * P.D);
        g.c.A = w.ay2; g.bias = P.buf.params + P.fc[2].b_off; g.out_f = (float*)aux; g.ldo = 2 * P.D;
        break;
    case MM_FC3_DGRAD:   // K = lde: the zero pad columns meet the zero pad of the packed weights
        g = dense(&P.fc[2].pk_dgrad, 1, rows, P.lde, 200);
        g.c.A = (const bf16*)aux; g.out_bf = w.dy2; g.ldo = 200;
        g.d_r = w.y2; g.d_ld = 200; g.d_act = ACT_SWISH; if (mask) { g.d_mask = mask; g.d_mask_scale = ms; }
        g.d_colsum = colsum ? colsum : P.buf.grads + P.fc[1].b_off;
        break;
    case MM_FC2_DGRAD:
        g = dense(&P.fc[1].pk_dgrad, 1, rows, 200, 400);
        g.c.A = w.dy2; g.out_bf = w.dy1; g.ldo = 400;
        g.d_r = w.y1; g.d_ld = 400; g.d_act = ACT_SWISH; if (mask) { g.d_mask = mask; g.d_mask_scale = ms; }
        g.d_colsum = colsum ? colsum : P.buf.grads + P.fc[0].b_off;
        break;
    case MM_UP:   // z_bf: [rows][ldz] with column D == 1.0 (folded bias)
        g = dense(&P.up.pk_fwd, 1, rows, P.ldz, 1024);
        g.c.A = w.z_bf; g.out_bf = w.u; g.ldo = 1024; g.out_act_bf = w.au; g.e_act = ACT_SWISH;
        break;
    case MM_UP_DGRAD:
        g = dense(&P.up.pk_dgrad, 1, rows, 1024, P.D);
        g.c.A = w.du; g.out_f = (float*)aux; g.ldo = P.D;
        break;
    case MM_DEC_CONVT: {
        const ConvL& L = P.convT[l];
        g = gemm_of(P, L.fwd, L.pk_fwd, n, B, L.pk_fwd_f);
        g.c.A = t.aq[l]; g.out_bf = t.q[l + 1]; g.ldo = L.g.Cout;
        g.colstats = training ? w.st_d[l] : nullptr;
        break;
    }
    case MM_DEC_CONVT_DGRAD: {
        const ConvL& L = P.convT[l];
        g = gemm_of(P, L.dgrad, L.pk_dgrad, n, B, L.pk_dgrad_f);
        g.c.A = t.dq[l + 1]; g.out_bf = t.dq[l]; g.ldo = L.g.Cin;
        g.d_r = t.q[l]; g.d_ld = L.g.Cin; g.d_act = ACT_SWISH;
        if (l > 0) { g.d_affine = w.aff_d[l - 1]; g.d_meanrstd = w.mr_d[l - 1]; g.d_red = w.red_d[l - 1]; }
        break;
    }
    case MM_DEC_LAST_DGRAD:
        // last transposed conv (32 -> 1) through the im2col patches of dlogit (K = 16 taps): input gradient = dense GEMM patches x W
        // with d-Swish + BatchNorm-backward sums in the epilogue.  (The direct dot-product kernel convt_last_dgrad is VALU-bound:
        // 52 us against 39 us for this GEMM at B=256.)
        g = dense(P.convT[3].pk_dgrad, n, rows1, 16, 32);
        g.c.A = w.patches4; g.out_bf = w.d3; g.ldo = 32;
        g.d_r = w.q3; g.d_ld = 32; g.d_act = ACT_SWISH; g.d_affine = w.aff_d[2]; g.d_meanrstd = w.mr_d[2]; g.d_red = w.red_d[2];
        break;
    }
    return g;
}

// p: MM_W_ENC_CONV / MM_W_DEC_CONVT the gradient of the layer's raw output -- dr[l] / dq[l + 1], or the buffer of its own that a fused
// layer's BatchNorm backward writes (drr[l] / dqr[l + 1]); MM_W_FC3 the gradient of the encoder's output, bf16 [n*B][lde]
WgradParams mm_wgrad(MMPlan& P, MMWgrad kind, int l, int n, const bf16* p = nullptr) {
    MMPlan::W& w = P.w;
    const MMChains t = mm_chains(w);
    const int B = P.B, rows = n * B, rows1 = B * 625;
    auto dense = [&](const int* gk, int nrows, int K, int N) { return wgrad_of(P, dense_plan(nrows, K, K, N), gk, 1, nrows); };
    WgradParams g{};
    switch (kind) {
    case MM_W_ENC_CONV1:   // conv1 over the im2col patches
        g = dense(P.conv[0].gk, rows1, 16, 32);
        g.c.A = w.patches1; g.P = w.d1e; g.ldp = 32;
        break;
    case MM_W_ENC_CONV:   // rows over the output grid, the activated input gathered in forward form
        g = wgrad_of(P, P.conv[l].fwd, P.conv[l].gk, 1, B);
        g.c.A = t.a[l - 1]; g.P = p; g.ldp = P.conv[l].g.Cout;
        break;
    case MM_W_FC1:   // classifier.0: gathers the shared 2x2x256 map
        g = wgrad_of(P, fc1_plan(rows), &P.fc[0].gk, 1, rows);
        g.c.A = w.a4; g.c.a_bcast_n = B; g.P = w.dy1; g.ldp = 400;
        break;
    case MM_W_FC2:
        g = dense(&P.fc[1].gk, rows, 400, 200);
        g.c.A = w.ay1; g.P = w.dy2; g.ldp = 200;
        break;
    case MM_W_FC3:
        g = dense(&P.fc[2].gk, rows, 200, 2 * P.D);
        g.c.A = w.ay2; g.P = p; g.ldp = P.lde;
        break;
    case MM_W_UP:   // upsample Linear: weight (+ folded bias) gradient
        g = dense(&P.up.gk, rows, P.ldz, 1024);
        g.c.A = w.z_bf; g.P = w.du; g.ldp = 1024;
        break;
    case MM_W_DEC_CONVT:
        g = convT_wgrad(P, P.convT[l], n, B, t.aq[l], p);
        break;
    case MM_W_DEC_LAST: {   // last transposed conv (32 -> 1): patches^T x activated input
        GatherPlan pl = plan_fwdform(1, 1, 25, 25, 16, 1, 1, 1, 0, 32, n, B);   // rows (n, iy, ix), dense K=16
        g = wgrad_of(P, pl, P.convT[3].gk, n, B);
        g.c.A = w.patches4; g.c.AH = 25; g.c.AW = 25; g.c.sy = g.c.sx = 1;
        g.P = w.aq3; g.ldp = 32;
        break;
    }
    }
    return g;
}

// ---- the stand-alone passes
// BatchNorm backward behind conv[l] (l = 1..3) / convT[l] (l = 0..2) into `dr`: db itself, or the fused layers' buffer apart from
// it; features.9 (l = 3) sums the gradients of the 2 classifier variants (db2)
BnBwdApplyArgs mm_enc_bn_bwd_args(MMPlan& P, int l, int variants, bf16* dr) {
    MMPlan::W& w = P.w;
    const MMChains t = mm_chains(w);
    const int B = P.B;
    const ConvL& L = P.conv[l];
    const BnL& b = P.bn[L.bn];
    const int pix = L.g.OH * L.g.OW;
    BnBwdApplyArgs x{};
    x.db = (l == 3) ? w.db4 : t.dr[l];
    x.db2 = (l == 3 && variants == 2) ? w.db4 + (size_t)B * 1024 : nullptr;
    x.r = t.r[l]; x.dr = dr; x.rows = B * pix; x.C = L.g.Cout; x.ld = L.g.Cout; x.rows_per_group = B * pix; x.G = 1;
    x.red = w.red_e[l - 1]; x.meanrstd = w.mr_e[l - 1]; x.gamma = P.buf.params + b.w_off;
    x.dgamma = P.buf.grads + b.w_off; x.dbeta = P.buf.grads + b.b_off;
    return x;
}
BnBwdApplyArgs mm_dec_bn_bwd_args(MMPlan& P, int l, int groups, bf16* dr) {
    MMPlan::W& w = P.w;
    const MMChains t = mm_chains(w);
    const int B = P.B, rows = groups * B;
    const ConvL& L = P.convT[l];
    const BnL& b = P.bn[L.bn];
    const int pix = L.g.OH * L.g.OW;
    BnBwdApplyArgs x{};
    x.db = t.dq[l + 1]; x.r = t.q[l + 1]; x.dr = dr; x.rows = rows * pix; x.C = L.g.Cout; x.ld = L.g.Cout;
    x.rows_per_group = B * pix; x.G = groups;
    x.red = w.red_d[l]; x.meanrstd = w.mr_d[l]; x.gamma = P.buf.params + b.w_off;
    x.dgamma = P.buf.grads + b.w_off; x.dbeta = P.buf.grads + b.b_off;
    return x;
}
// BatchNorm + Swish behind conv[l] (l = 1..3) / convT[l] (l = 0..2): tables, running statistics, activated tensor
int mm_enc_bn_act(MMPlan& P, int l, int bn_updates, int training, hipStream_t s) {
    MMPlan::W& w = P.w;
    const MMChains t = mm_chains(w);
    const ConvL& L = P.conv[l];
    const int rows = P.B * L.g.OH * L.g.OW;
    return bn_act(P, P.bn[L.bn], t.r[l], t.a[l], rows, rows, 1, w.st_e[l - 1], bn_updates, w.aff_e[l - 1], w.mr_e[l - 1], training, s);
}
int mm_dec_bn_act(MMPlan& P, int l, int groups, int training, hipStream_t s) {
    MMPlan::W& w = P.w;
    const MMChains t = mm_chains(w);
    const ConvL& L = P.convT[l];
    const int rpg = P.B * L.g.OH * L.g.OW;
    return bn_act(P, P.bn[L.bn], t.q[l + 1], t.aq[l + 1], groups * rpg, rpg, groups, w.st_d[l], 1, w.aff_d[l], w.mr_d[l], training, s);
}
// The same pass for the input of conv[l] (l >= 2) / convT[l] (l >= 1) where the layer staged the raw tensor itself and left
// nothing behind: a[l - 1] / aq[l], the operand of the layer's weight gradient, made in front of it off the main chain
// (plan_base.h bn_act_side); `groups` row blocks
struct MMActSide { BnL b; const bf16* r; bf16* a; int rows_per_group; const float2* st; };
MMActSide mm_enc_act_side(MMPlan& P, int l) {
    const MMChains t = mm_chains(P.w);
    const ConvL& Lp = P.conv[l - 1];
    return MMActSide{P.bn[Lp.bn], t.r[l - 1], t.a[l - 1], P.B * Lp.g.OH * Lp.g.OW, P.w.st_e[l - 2]};
}
MMActSide mm_dec_act_side(MMPlan& P, int l) {
    const MMChains t = mm_chains(P.w);
    const ConvL& Lp = P.convT[l - 1];
    return MMActSide{P.bn[Lp.bn], t.q[l], t.aq[l], P.B * Lp.g.OH * Lp.g.OW, P.w.st_d[l - 1]};
}
int mm_act_side(MMPlan& P, const MMActSide& x, int groups, int training, hipStream_t s) {
    return bn_act_side(P, x.b, x.r, x.a, groups * x.rows_per_group, x.rows_per_group, groups, x.st, training, s);
}
// last transposed conv (32 -> 1) + sigmoid (+ BCE and its gradient): `last` carries the caller's target / outputs / loss weights
ConvTLastFwdArgs mm_dec_last_args(MMPlan& P, const ConvTLastFwdArgs& last, int groups) {
    ConvTLastFwdArgs x = last;
    x.act = P.w.aq3; x.w = P.buf.params + P.convT[3].w_off; x.G = groups; x.B = P.B; x.IH = 25; x.IW = 25; x.Cin = 32; x.Cout = 1;
    return x;
}

// Staging transforms of the fused step (gemm.h GatherTransform; image-resident kernels only): `tr` is read by the launcher and
// must outlive the launch.  With knob mm_stage_out (read here, when the launch is issued) the staged tensor is also left behind
// for the weight gradient (GatherTransform::out).
// kind 1: forward layer l stages Swish(BatchNorm(raw output of the layer below)) itself, writes that layer's tables and updates
// its running statistics; out: a[l - 1] / aq[l], the operand of this layer's weight gradient
void mm_stage_fwd_enc(MMPlan& P, int l, GemmParams& g, GatherTransform& tr, int bn_updates, int training) {
    MMPlan::W& w = P.w;
    const MMChains t = mm_chains(w);
    const ConvL& Lp = P.conv[l - 1];
    tr.kind = 1;
    tr.fin = bn_fin_args(P, P.bn[Lp.bn], P.B * Lp.g.OH * Lp.g.OW, 1, w.st_e[l - 2], bn_updates, w.aff_e[l - 2], w.mr_e[l - 2], training);
    if (mmvae_knob(K_mm_stage_out)) tr.out = t.a[l - 1];
    g.c.A = t.r[l - 1]; g.tr = &tr;
}
void mm_stage_fwd_dec(MMPlan& P, int l, int groups, GemmParams& g, GatherTransform& tr, int training) {
    MMPlan::W& w = P.w;
    const MMChains t = mm_chains(w);
    const ConvL& Lp = P.convT[l - 1];
    tr.kind = 1;
    tr.fin = bn_fin_args(P, P.bn[Lp.bn], P.B * Lp.g.OH * Lp.g.OW, groups, w.st_d[l - 1], 1, w.aff_d[l - 1], w.mr_d[l - 1], training);
    if (mmvae_knob(K_mm_stage_out)) tr.out = t.aq[l];
    g.c.A = t.q[l]; g.tr = &tr;
}
// kind 2: the data gradient of layer l applies the BatchNorm backward of the layer's own BatchNorm to db while staging it.  Not
// in place: out is drr[l] / dqr[l + 1], a buffer apart from db, and with it go the BatchNorm parameter gradients -- in the
// encoder for conv3 alone (conv2's dr and parameter gradients come from the bn_bwd_apply launch in front of its weight gradient)
void mm_stage_bwd_enc(MMPlan& P, int l, GemmParams& d, GatherTransform& tr) {
    MMPlan::W& w = P.w;
    const MMChains t = mm_chains(w);
    const ConvL& L = P.conv[l];
    const BnL& b = P.bn[L.bn];
    tr.kind = 2; tr.r = t.r[l]; tr.red = w.red_e[l - 1]; tr.mr = w.mr_e[l - 1]; tr.gamma = P.buf.params + b.w_off;
    tr.inv_cnt = 1.f / (float)(P.B * L.g.OH * L.g.OW); tr.groups = 1;
    if (l == 2 && mmvae_knob(K_mm_stage_out)) { tr.out = t.drr[l]; tr.dgamma = P.buf.grads + b.w_off; tr.dbeta = P.buf.grads + b.b_off; }
    d.tr = &tr;
}
void mm_stage_bwd_dec(MMPlan& P, int l, int groups, GemmParams& d, GatherTransform& tr) {
    MMPlan::W& w = P.w;
    const MMChains t = mm_chains(w);
    const ConvL& L = P.convT[l];
    const BnL& b = P.bn[L.bn];
    tr.kind = 2; tr.r = t.q[l + 1]; tr.red = w.red_d[l]; tr.mr = w.mr_d[l]; tr.gamma = P.buf.params + b.w_off;
    tr.inv_cnt = 1.f / (float)(P.B * L.g.OH * L.g.OW); tr.groups = groups;
    if (mmvae_knob(K_mm_stage_out)) { tr.out = t.dqr[l + 1]; tr.dgamma = P.buf.grads + b.w_off; tr.dbeta = P.buf.grads + b.b_off; }
    d.tr = &tr;
}

// ---- the row-block launches of mlp_tail.hip: the block their plain and their waist (Mlp2Latent1*) forms share.  waist: the copies of
// classifier.6 at the widths of 2D (wa_*; at n_latents = 100 they are the mt_* ones)
// classifier.3 + Swish + Dropout + classifier.6 on ay1; mask: keep flags of the second Dropout or null
void mm_mlp2_fwd_args(MMPlan& P, Mlp2FwdArgs& a, bool waist, int rows, const uint8_t* mask, float* out) {
    MMPlan::W& w = P.w;
    a.rows = rows; a.x = w.ay1;
    a.w2 = P.buf.packed + P.pk.d[waist ? P.wa_w2 : P.mt_w2].dst_off; a.b2 = P.buf.params + P.fc[1].b_off;
    a.w3 = P.buf.packed + P.pk.d[waist ? P.wa_w3 : P.mt_w3].dst_off; a.b3 = P.buf.params + P.fc[2].b_off;
    if (mask) { a.mask = mask; a.mask_scale = 1.f / (1.f - DROP_P); }
    a.y2 = w.y2; a.ay2 = w.ay2; a.out = out;
}
// both data gradients and the bias gradients of classifier.3 / classifier.0; m1 / m2: keep flags of the two Dropouts, or both null
void mm_mlp2_bwd_args(MMPlan& P, Mlp2BwdArgs& a, bool waist, int rows, const uint8_t* m1, const uint8_t* m2) {
    MMPlan::W& w = P.w;
    a.rows = rows;
    a.w3t = P.buf.packed + P.pk.d[waist ? P.wa_w3t : P.mt_w3t].dst_off; a.w2t = P.buf.packed + P.pk.d[waist ? P.wa_w2t : P.mt_w2t].dst_off;
    a.y2 = w.y2; a.y1 = w.y1;
    if (m1 || m2) { a.mask2 = m2; a.mask1 = m1; a.mask_scale = 1.f / (1.f - DROP_P); }
    a.dy2 = w.dy2; a.dy1 = w.dy1;
    a.db2 = P.buf.grads + P.fc[1].b_off; a.db1 = P.buf.grads + P.fc[0].b_off;
}

// ================================================================== image encoder
// convs once on B images; classifier on variants*B rows (different dropout masks): multimnist/model.py:183-188
// Every layer output is kept twice: raw (r*, y*: backward needs the pre-activation) and activated (a*: the next
// GEMM's operand, staged by pure copies).
// `fuse`: the layers whose consumer is an image-resident kernel (convres.hip) hand it the RAW tensor and the BatchNorm
// statistics (GatherTransform kind 1); the materialised activation is made later, off the main chain, for the weight gradient
int enc_fwd(MMPlan& P, const float* image, int variants, const uint8_t* m1, const uint8_t* m2, int dropout, int training,
            int bn_updates, float* out, hipStream_t s, bool fuse = false, const Mlp2Latent1FwdArgs* waist = nullptr, bool tail_only = false) {
    MMPlan::W& w = P.w;
    const int B = P.B;
    const int rows = variants * B;
    const bool drop = training && dropout;
    const uint8_t *k1 = drop ? m1 : nullptr, *k2 = drop ? m2 : nullptr;
    if (!tail_only) {      // (tail_only: classifier.3 onwards, on the ay1 of an earlier call -- mm_bench_layer's replay of the image step's middle)
    if (fuse && mmvae_knob(K_mm_conv1_mfma)) {      // one workgroup per image on the matrix cores (conv1.hip)
        const PackDesc& d = P.pk.d[P.conv[0].pk_fwd[0]];
        MMVAE_TRY(launch_conv1_fwd_mfma(image, B, P.buf.packed + d.dst_off, d.Kpad, w.r1, w.a1, s));
    } else {
        MMVAE_TRY(launch_im2col_small(image, B, 1, IMG, IMG, 4, 4, 2, 1, 25, 25, w.patches1, 16, s));
        MMVAE_TRY(launch_gemm_gather(mm_gemm(P, MM_ENC_CONV1, 0, 1), s));
    }
    for (int l = 1; l < 4; ++l) {
        GemmParams g = mm_gemm(P, MM_ENC_CONV, l, 1, training);
        GatherTransform tr{};
        // conv3 / conv4 stage Swish(BatchNorm(raw output of the layer below)) themselves; a2 / a3, the operands of their weight
        // gradients, are a by-product of the staging
        if (fuse && l >= 2) mm_stage_fwd_enc(P, l, g, tr, bn_updates, training);
        MMVAE_TRY(launch_gemm_gather(g, s));
        if (fuse && l <= 2) continue;  // a2 / a3 are made in front of the next layer's weight gradient (enc_bwd)
        MMVAE_TRY(mm_enc_bn_act(P, l, bn_updates, training, s));
    }
    MMVAE_TRY(launch_gemm_gather(mm_gemm(P, MM_FC1, 0, variants, training, k1), s));
    }
    if (waist) {           // image-only step: the same launch goes on to (mu | logvar), z and the KL partials (the caller's fields)
        Mlp2Latent1FwdArgs a = *waist;
        mm_mlp2_fwd_args(P, a, true, rows, k2, out);
        return launch_mlp2_latent1_fwd(a, s);
    }
    if (P.mlp_tail) {      // classifier.3 + Swish + Dropout + classifier.6 in one row-block launch
        Mlp2FwdArgs a{};
        mm_mlp2_fwd_args(P, a, false, rows, k2, out);
        return launch_mlp2_fwd(a, s);
    }
    MMVAE_TRY(launch_gemm_gather(mm_gemm(P, MM_FC2, 0, variants, training, k2), s));
    return launch_gemm_gather(mm_gemm(P, MM_FC3, 0, variants, training, nullptr, out), s);
}

// d_out: bf16 [variants*B][lde], columns 2D.. zero (the generic kernels read their operands in 8-column vectors; 2D is a multiple
// of 8 only when n_latents is a multiple of 4); the bias gradient of classifier.6 must already be accumulated by the caller
// `waist` (image-only step): d_out (= w.d_encout) does not exist yet -- the waist launch forms it, and its finish launch the bias gradient
int enc_bwd(MMPlan& P, const bf16* d_out, int variants, const uint8_t* m1, const uint8_t* m2, int dropout, hipStream_t s, bool fuse = false,
            const Mlp2Latent1BwdArgs* waist = nullptr, float* loss_out = nullptr, bool tail_only = false) {
    MMPlan::W& w = P.w;
    const MMChains t = mm_chains(w);
    const int B = P.B, rows = variants * B;
    const uint8_t *k1 = dropout ? m1 : nullptr, *k2 = dropout ? m2 : nullptr;
    // fused step: the three classifier weight gradients (0.04-0.4 GFLOP each, every one a launch at the kernel-latency floor) go
    // out as ONE grouped launch behind conv4's data gradient
    const bool grouped = fuse && P.mlp_tail && !waist;
    auto cls_w = std::make_shared<std::vector<WgradParams>>();
    auto cls_wgrad = [&](const WgradParams& g) {
        if (!grouped) return wgrad_async(P, g, s);
        cls_w->push_back(g);
        return (int)MMVAE_OK;
    };
    const WgradParams g3 = mm_wgrad(P, MM_W_FC3, 0, variants, d_out), g2 = mm_wgrad(P, MM_W_FC2, 0, variants);
    if (waist) {           // latent backward + both data gradients in one row-block launch
        Mlp2Latent1BwdArgs a = *waist;
        mm_mlp2_bwd_args(P, a, true, rows, k1, k2);
        a.d_enc_out = w.d_encout; a.lde = P.lde;
        MMVAE_TRY(launch_mlp2_latent1_bwd(a, s));
        {   // the fold of the partials (KL of the forward, classifier.6's bias gradient) and the loss sums: nobody on the main chain
            // reads them, so the one-workgroup launch goes beside it
            hipStream_t fs = s;
            MMVAE_TRY(wgrad_side_stream(P, s, &fs));
            MMVAE_TRY(launch_mlp2_latent1_finish(a.scratch, rows, P.D, P.buf.grads + P.fc[2].b_off, w.sums, loss_out, fs));
        }
        MMVAE_TRY(cls_wgrad(g3));
        MMVAE_TRY(cls_wgrad(g2));
    } else if (P.mlp_tail) {      // both data gradients in one row-block launch; the weight gradients follow on the side stream
        MMVAE_TRY(cls_wgrad(g3));
        Mlp2BwdArgs a{};
        mm_mlp2_bwd_args(P, a, false, rows, k1, k2);
        a.d_out = d_out;
        MMVAE_TRY(launch_mlp2_bwd(a, s));
        MMVAE_TRY(cls_wgrad(g2));
    } else {
        MMVAE_TRY(cls_wgrad(g3));
        MMVAE_TRY(launch_gemm_gather(mm_gemm(P, MM_FC3_DGRAD, 0, variants, 1, k2, d_out), s));
        MMVAE_TRY(cls_wgrad(g2));
        MMVAE_TRY(launch_gemm_gather(mm_gemm(P, MM_FC2_DGRAD, 0, variants, 1, k1), s));
    }
    if (tail_only) return MMVAE_OK;        // (down to classifier.0's output gradient: mm_bench_layer's replay of the image step's middle)
    // classifier.0: the weight gradient gathers the shared 2x2x256 map; the data gradient emits NHWC gradients for `rows` samples
    MMVAE_TRY(cls_wgrad(mm_wgrad(P, MM_W_FC1, 0, variants)));
    if (grouped) {
        MMPlan* pp = &P;
        side_later(P, [pp, cls_w](hipStream_t ws_) {
            MMVAE_TRY(launch_wgrad_group(cls_w->data(), (int)cls_w->size(), ws_, &pp->slab));
            return pp->batch_reduce ? MMVAE_OK : launch_wgrad_reduce(&pp->slab, ws_, true);
        }, mmvae_knob(K_mm_cls_lane));
    }
    MMVAE_TRY(launch_gemm_gather(mm_gemm(P, MM_FC1_DGRAD, 0, variants), s));
    // ---- conv stack (features shared by all variants: gradients of the variants add up)
    for (int l = 3; l >= 1; --l) {
        // conv3 / conv2: the image-resident data-gradient kernel applies the BatchNorm backward to db while staging it
        // (GatherTransform kind 2); the materialised dr is only the weight gradient's operand and is made in front of it,
        // off the main chain, into a buffer of its own (db is still being read by the data gradient)
        const bool fl = fuse && l < 3;
        const BnBwdApplyArgs x = mm_enc_bn_bwd_args(P, l, variants, fl ? t.drr[l] : t.dr[l]);
        if (!fl) MMVAE_TRY(launch_bn_bwd_apply(x, s));
        // Forks are bound to a producer kernel's completion: a fused layer's operands came out of the previous data gradient (the
        // current event); the unfused conv4 issues its weight gradient behind its own data gradient, on the event conv3's needs anyway
        const WgradParams gw = mm_wgrad(P, MM_W_ENC_CONV, l, 1, x.dr);
        if (fuse) {
            // fused layers (conv3, conv2): the weight gradient runs on a side stream on operands that are by-products of the main
            // chain's staging (GatherTransform::out) or are materialised right in front of it, off the main chain.
            // With staging by-products the forward of conv3 / conv4 left a2 / a3 behind and conv3's data gradient below
            // leaves its BatchNorm-backward dr behind: nothing to materialise in front of the kernel
            MMPlan* pp = &P;
            const bool byp = mmvae_knob(K_mm_stage_out) != 0;
            const bool actp = l >= 2 && !byp;      // a[l-1] = Swish(BatchNorm(r[l-1])) was never materialised (conv3, conv4)
            const bool bnb = fl && !(byp && l == 2);
            const MMActSide as = actp ? mm_enc_act_side(P, l) : MMActSide{};
            // lane 1: the LAST weight gradients of the step (conv3's, conv2's) go to the second-modality stream -- it has run dry
            // by then, and the weight-gradient stream still holds the classifier's and conv4's
            side_later(P, [pp, x, gw, bnb, actp, as](hipStream_t ws_) {
                if (bnb) MMVAE_TRY(launch_bn_bwd_apply(x, ws_));
                if (actp) MMVAE_TRY(mm_act_side(*pp, as, 1, 1, ws_));
                return wgrad_on(*pp, gw, ws_);
            }, l == 1 ? 1 : l == 2 ? mmvae_knob(K_mm_conv3_lane) : mmvae_knob(K_mm_conv4_lane));
            if (l == 1) MMVAE_TRY(side_flush(P, s));    // conv2's: its operands came out of conv3's data gradient (current event)
        }
        {
            GemmParams d = mm_gemm(P, MM_ENC_CONV_DGRAD, l, 1);
            GatherTransform tr{};
            if (fl) mm_stage_bwd_enc(P, l, d, tr);      // conv3 also leaves dr for its weight gradient + the BatchNorm parameter gradients
            // forks: behind conv4's data gradient (classifier + conv4 + conv3 weight gradients) and behind conv3's (conv2's)
            // (knob mm_forks = 1: ONE fork for the whole encoder backward, behind conv3's data gradient -- a kernel that carries a
            //  completion event ends with a system-scope release, ~8 us on the main chain per fork: tools/step_parts.py)
            const bool flush = fuse && P.wgrad_forked && (mmvae_knob(K_mm_forks) ? l == 2 : l >= 2);
            if (flush) arm_fork(P);
            MMVAE_TRY(launch_gemm_gather(d, s));
            if (flush) { MMVAE_TRY(commit_fork(P, s)); MMVAE_TRY(side_flush(P, s)); }
        }
        if (!fuse) MMVAE_TRY(wgrad_async(P, gw, s));
    }
    if (fuse && !P.wgrad_forked) MMVAE_TRY(side_flush(P, s));     // unforked (serial) use: nothing to wait for
    if (fuse && mmvae_knob(K_mm_conv1_mfma) && P.step_image) {       // the LAST kernel of the backward chain: conv1.hip
        const PackDesc& gd = P.gk.d[P.conv[0].gk[0]];
        return launch_conv1_wgrad_mfma(P.step_image, B, w.d1e, P.buf.gpk + gd.dst_off, gd.Kpad, s);
    }
    // conv1 wgrad over the im2col patches: the LAST kernel of the backward chain -- it stays on the main stream (a hop to a side
    // stream and back would put two event latencies on the critical path).  fp32 atomics into the (zeroed) packed gradient instead
    // of slab copies + a reduce launch: this is the last kernel in front of the optimizer, a second launch here is pure tail
    // latency (the tile is 32 x 16)
    return launch_wgrad(mm_wgrad(P, MM_W_ENC_CONV1, 0, 1), s, nullptr);
}

// ================================================================== image decoder (multimnist/model.py:211-216)
// z_bf: [groups*B][ldz] with column D == 1.0 (folded bias).  The last layer is the fused direct kernel
// ConvTranspose2d(32,1) + sigmoid (+ BCE and its gradient when `bce` is given).
// BatchNorm finalize of hallucinate.7 + the thin last layer + (for the first bwd_groups groups) its gradients: thin.h
int fused_tail(MMPlan& P, int groups, int training, const ConvTLastFwdArgs* last, int last_groups, int fused_bwd_groups, hipStream_t s,
               float* dlogit_dump = nullptr) {
    MMPlan::W& w = P.w;
    const int B = P.B;
    const ConvL& L = P.convT[2];
    DecLastFusedArgs x{};
    x.r = w.q3; x.act = ACT_SWISH; x.w = P.buf.params + P.convT[3].w_off;
    x.G = last_groups > 0 ? last_groups : groups; x.B = B; x.IH = 25; x.IW = 25; x.Cin = 32;
    x.bwd_groups = std::min(fused_bwd_groups, x.G);
    x.fin = bn_fin_args(P, P.bn[L.bn], B * L.g.OH * L.g.OW, groups, w.st_d[2], 1, w.aff_d[2], w.mr_d[2], training);
    x.target = last->target; x.logits = last->logits; x.recon = last->recon; x.dlogit = dlogit_dump;      // (the step keeps dlogit in LDS)
    for (int k = 0; k < 4; ++k) x.coef[k] = last->coef[k];
    x.loss_sum = last->loss_sum;
    if (last->loglik) { x.loglik = last->loglik; x.rows_per_target = last->rows_per_target; x.B = last->rows; }
    if (x.bwd_groups > 0) {
        const int chunks = x.bwd_groups * B * dec_last_wgrad_partials(x);
        x.wslab = P.slab.take((size_t)chunks * 32 * 16);
        MMVAE_REQUIRE(x.wslab != nullptr, "fused decoder tail: the weight-gradient slab pool is exhausted");
        x.db = w.d3; x.red = w.red_d[2];
        WgradSlabJob j{};
        const PackDesc& gd = P.gk.d[P.convT[3].gk[0]];
        j.dst = P.buf.gpk + gd.dst_off; j.slab = x.wslab; j.N = 32; j.K = 16; j.Kpad = gd.Kpad; j.chunks = chunks;
        j.chunk_stride = 32 * 16; j.src_ld = 16; j.stream = s;
        P.slab.jobs.push_back(j);
    }
    return launch_dec_last_fused(x, s);
}

// `fused_bwd_groups` >= 0: the fused tail (thin.h DecLastFusedArgs) replaces bn_act of the last BatchNorm + the thin last
// layer, and for the first fused_bwd_groups groups also the last layer's data / weight gradients (step path only: the
// granular modules get their upstream gradient from autograd and keep the separate kernels).
int dec_fwd(MMPlan& P, int groups, int training, ConvTLastFwdArgs* last, hipStream_t s, int last_groups = -1, int fused_bwd_groups = -1,
            bool fuse = false) {
    MMVAE_TRY(launch_gemm_gather(mm_gemm(P, MM_UP, 0, groups), s));
    for (int l = 0; l < 3; ++l) {
        GemmParams g = mm_gemm(P, MM_DEC_CONVT, l, groups, training);
        GatherTransform tr{};
        // convT2 / convT3 stage Swish(BatchNorm(q[l])) themselves; aq[l], the operand of this layer's weight gradient, is a
        // by-product of the staging
        if (fuse && l >= 1) mm_stage_fwd_dec(P, l, groups, g, tr, training);
        MMVAE_TRY(launch_gemm_gather(g, s));
        if (l == 2 && fused_bwd_groups >= 0) continue;
        if (fuse && l <= 1) continue;  // aq[l+1] is made in front of the next layer's weight gradient (dec_bwd)
        MMVAE_TRY(mm_dec_bn_act(P, l, groups, training, s));
    }
    if (fused_bwd_groups >= 0) return fused_tail(P, groups, training, last, last_groups, fused_bwd_groups, s);
    return launch_convt_last_fwd(mm_dec_last_args(P, *last, last_groups > 0 ? last_groups : groups), s);
}

// dlogit: fp32 NCHW [groups*B][1][50][50] (grad wrt the pre-sigmoid logits). Writes dz (fp32 [groups*B][D]).
int dec_bwd(MMPlan& P, const float* dlogit, int groups, float* dz, hipStream_t s, bool last_fused = false, bool fuse = false,
            int fwd_groups = 0, int training = 1) {
    MMPlan::W& w = P.w;
    const MMChains t = mm_chains(w);
    MMPlan* pp = &P;
    if (last_fused) {
        // d3, the BatchNorm-backward sums and the weight-gradient partials of the last layer came out of the fused tail
        // (dec_fwd); only the sum of the partials is left, off the main chain
        if (P.wgrad_forked) {
            PlanBase* pb = &P;
            side_later(P, [pb, s](hipStream_t wst) {
                for (WgradSlabJob& j : pb->slab.jobs) if (j.stream == s && j.src_ld == 16) j.stream = wst;
                return launch_wgrad_reduce(&pb->slab, wst, true);
            });
        }
    } else {   // last transposed conv (32 -> 1): both gradients go through the im2col patches of dlogit (K = 16 taps)
        MMVAE_TRY(launch_im2col_small(dlogit, groups * P.B, 1, IMG, IMG, 4, 4, 2, 1, 25, 25, w.patches4, 16, s));
        arm_fork(P);
        MMVAE_TRY(launch_gemm_gather(mm_gemm(P, MM_DEC_LAST_DGRAD, 3, groups), s));
        MMVAE_TRY(commit_fork(P, s));
        MMVAE_TRY(wgrad_async(P, mm_wgrad(P, MM_W_DEC_LAST, 3, groups), s));
    }
    for (int l = 2; l >= 0; --l) {
        // convT3 / convT2: the image-resident data-gradient kernel applies the BatchNorm backward while it stages db
        // (GatherTransform kind 2); dr and the activated layer input are only the weight gradient's operands and are made in
        // front of it on the side stream (enc_bwd has the same arrangement)
        const bool fl = fuse;          // (hallucinate.0 too: its input is the upsample Linear's activation, no BatchNorm below it)
        const BnBwdApplyArgs x = mm_dec_bn_bwd_args(P, l, groups, fl ? t.dqr[l + 1] : t.dq[l + 1]);
        if (!fl) MMVAE_TRY(launch_bn_bwd_apply(x, s));
        // Forks are bound to a producer kernel's completion (arm_fork / commit_fork).  Fused layers: the operands of the
        // weight gradient came out of the previous data gradient (or the fused tail), whose event is the current one.  The
        // unfused first layer: its weight gradient is issued behind the layer's own data gradient, on the event the upsample
        // weight gradient needs anyway (one bound event less on the main chain)
        const WgradParams gw = mm_wgrad(P, MM_W_DEC_CONVT, l, groups, x.dr);
        if (fl) {
            // the streamed weight-gradient kernel on operands materialised right in front of it, on the side stream: the
            // BatchNorm backward of db (its own buffer: the data gradient on the main chain still reads db) and, above the
            // first layer, the layer input aq[l] = Swish(BatchNorm(q[l])) that the forward never wrote
            // (with staging by-products, GatherTransform::out, both come out of kernels of the main chain instead: aq[l]
            //  out of this layer's forward, dr out of this layer's data gradient below -- the side work is the GEMM alone)
            const bool byp = mmvae_knob(K_mm_stage_out) != 0;
            const bool actp = l >= 1 && !byp;
            const MMActSide as = actp ? mm_dec_act_side(P, l) : MMActSide{};
            side_later(P, [pp, x, gw, byp, actp, as, groups, training](hipStream_t ws_) {
                if (!byp) MMVAE_TRY(launch_bn_bwd_apply(x, ws_));
                if (actp) MMVAE_TRY(mm_act_side(*pp, as, groups, training, ws_));
                return wgrad_on(*pp, gw, ws_);
            });
        } else if (l == 0) {
            side_later(P, [pp, gw](hipStream_t ws_) { return wgrad_on(*pp, gw, ws_); });
        }
        {
            GemmParams d = mm_gemm(P, MM_DEC_CONVT_DGRAD, l, groups);
            GatherTransform tr{};
            if (fl) mm_stage_bwd_dec(P, l, groups, d, tr);
            // the side work collected so far forks off the completion of the first and of the last data gradient
            const bool flush = P.wgrad_forked && ((l == 2 && !mmvae_knob(K_mm_forks)) || l == 0);
            if (flush) arm_fork(P);
            MMVAE_TRY(launch_gemm_gather(d, s));
            if (flush) { MMVAE_TRY(commit_fork(P, s)); if (l == 2) MMVAE_TRY(side_flush(P, s)); }
        }
        if (!fl && l != 0) MMVAE_TRY(wgrad_async(P, gw, s));
    }
    // upsample Linear: weight (+ folded bias) gradient and dz
    const WgradParams gu = mm_wgrad(P, MM_W_UP, 0, groups);
    side_later(P, [pp, gu](hipStream_t ws_) { return wgrad_on(*pp, gu, ws_); });
    MMVAE_TRY(side_flush(P, s));                // forks off the last data gradient above (du is its output)
    return launch_gemm_gather(mm_gemm(P, MM_UP_DGRAD, 0, groups, 1, nullptr, dz), s);
}

// ================================================================== text modules (argument builders and grouped weight gradients: text_plan.h)
TextEncArgs te_args(MMPlan& P, const long long* text, float* out, bool save) { return text_enc_args(P, text, out, save); }
int txt_enc_bwd(MMPlan& P, const long long* text, const float* d_out, hipStream_t s) { return text_enc_bwd(P, text, d_out, s); }
TextDecArgs td_args(MMPlan& P, const float* z, int groups, bool save) { return text_dec_args(P, z, groups, save); }
int txt_dec_bwd(MMPlan& P, const TextDecArgs& f, const float* dwords, float* dz, hipStream_t s) {
    const int R = f.R;
    const TextDecBwdArgs a = text_dec_bwd_args(P, f, dwords, dz);
    // In the fused step the main chain needs dz (and the NLL sums) of THIS kernel, not the weight gradients enqueued behind it on the
    // same stream: the join is the kernel's own completion event (a join on "everything enqueued on T so far" made the main chain wait
    // for ~45 us of weight-gradient launches; measured on the traces of round 4: the second-modality stream was co-critical)
    P.ev_dz = nullptr;
    const bool own_ev = P.in_step && s == P.st_text && mmvae_knob(K_mm_dz_event) != 0;
    if (own_ev) {
        P.ev_dz = next_ev(P);
        if (!P.capturing && !mmvae_knob(K_no_stop_events)) mmvae_arm_stop_event(P.ev_dz);
    }
    MMVAE_TRY(launch_text_decoder_bwd(a, s));
    if (own_ev && (mmvae_take_stop_event() != nullptr || P.capturing || mmvae_knob(K_no_stop_events)) && hipEventRecord(P.ev_dz, s) != hipSuccess) {
        mmvae_set_error("text decoder event failed: %s", hipGetErrorString(hipGetLastError()));
        return MMVAE_EHIP;
    }
    MMVAE_TRY(text_dec_wgrads(P, R, s));
    // every gradient of text_decoder.* is complete on this stream here: the early optimizer part waits for this event
    P.ev_txtgrads = nullptr;
    if (own_ev) {
        P.ev_txtgrads = next_ev(P);
        if (hipEventRecord(P.ev_txtgrads, s) != hipSuccess) {
            mmvae_set_error("text decoder event failed: %s", hipGetErrorString(hipGetLastError()));
            return MMVAE_EHIP;
        }
    }
    return MMVAE_OK;
}

}  // namespace

// ================================================================== public (internal C++) API
MMPlan* mm_create(int D, int B) {
    if (D < 1 || D > 127 || B < 1) { mmvae_set_error("mm_create: need 1 <= n_latents <= 127 and batch >= 1"); return nullptr; }
    MMPlan* P = new MMPlan();
    P->D = D; P->B = B;
    // round 3: two weight-gradient streams side by side (the chain was the step's tail: 758 -> 718 us); round 4, with the ring-staged
    // kernels on half the chip each: ONE stream again (643 -> 634 us; knob one_wgrad_stream)
    P->single_wgrad_stream = true;
    build_plan(*P);
    plan_size_workspaces(*P, carve);
    return P;
}
void mm_destroy(MMPlan* P) { delete P; }
int mm_early_ranges(const MMPlan* P, long long* ranges, int cap) {
    int n = 0;
    for (const ParamInfo& pi : P->params) {
        if (pi.name.rfind("image_decoder.", 0) != 0 && pi.name.rfind("text_decoder.", 0) != 0) continue;
        if (n > 0 && ranges[2 * (n - 1)] + ranges[2 * (n - 1) + 1] == pi.offset) { ranges[2 * (n - 1) + 1] += pi.numel; continue; }
        if (n == cap) return 0;                    // (does not fit: the caller updates everything itself)
        ranges[2 * n] = pi.offset; ranges[2 * n + 1] = pi.numel; ++n;
    }
    for (int r = 0; r < n; ++r)
        if (ranges[2 * r] % 4 != 0 || ranges[2 * r + 1] % 4 != 0) return 0;
    return n;
}
PlanBase* mm_base(MMPlan* P) { return P; }

// (no reset of its own behind the shared part: wgrad_forked is cleared where the step leaves its backward pass)
static int use_ws(MMPlan* P, void* ws, size_t bytes, bool module = true) { return plan_use_ws(P, ws, bytes, module, carve); }

static int mm_step_body(MMPlan* Pp, const mmvae_mm_step_io& io, int training, int do_backward, hipStream_t s);
int mm_step_fwd_bwd(MMPlan* Pp, const mmvae_mm_step_io& io, int training, int do_backward, hipStream_t s) {
    if (const mmvae_early_adam* e = io.early_adam) {
        MMVAE_REQUIRE(e->m && e->v && e->state && e->gmap && e->ran, "mmvae_mm_step: early_adam with a null field");
        *e->ran = 0;
    }
    return plan_step(Pp, io, training, do_backward, s, mm_step_body);
}
static int mm_step_body(MMPlan* Pp, const mmvae_mm_step_io& io, int training, int do_backward, hipStream_t s) {
    MMVAE_TRY(use_ws(Pp, io.ws, io.ws_bytes, false));
    MMPlan& P = *Pp;
    MMPlan::W& w = P.w;
    const int B = P.B, D = P.D, B3 = 3 * B;
    MMVAE_REQUIRE(io.image && io.text && io.sums, "step: image/text/sums must be given");
    // ---- one prologue launch: zero every accumulation buffer, draw eps / dropout keep flags (Philox keyed by the
    //      device step counter) unless the caller injected them
    const float* eps = io.eps;
    const uint8_t *m1 = io.enc_mask1, *m2 = io.enc_mask2, *gk = io.gru_keep;
    // Staged prologue (knob mm_stage_begin, default on): the main stream's launch zeroes the workspace accumulators, draws the random
    // numbers and refreshes only the weight copies the image encoder's forward reads; the gradient buffers (first written in the
    // backward pass) and the other copies are done on the second-modality stream, which the main chain joins in front of the
    // product of experts anyway.  26 -> 9 us of prologue on the main chain.
    const bool serial0 = mmvae_serial();
    const bool staged = mmvae_knob(K_mm_stage_begin) != 0 && !serial0;
    StepBeginArgs sb{}, sb2{};
    sb.zero_ptr[0] = w.zero_begin; sb.zero_bytes[0] = w.zero_bytes;
    StepBeginArgs& sz = staged ? sb2 : sb;
    if (do_backward) {
        sz.zero_ptr[1] = P.buf.gpk; sz.zero_bytes[1] = (size_t)P.gk.mat_elems * sizeof(float);
        sz.zero_ptr[2] = P.buf.grads; sz.zero_bytes[2] = (size_t)(P.nparams / 4) * 16;     // tail (< 4 floats) below
        const int skipz = mmvae_knob(K_dbg_begin_skip_zero);      // measurement aid (results are garbage): 1 gpk, 2 grads, 3 both
        if (skipz & 1) sz.zero_ptr[1] = nullptr;
        if (skipz & 2) sz.zero_ptr[2] = nullptr;
    }
    sb.p = DROP_P; sb.seed = io.seed; sb.step = io.step_counter;
    if (training && !eps) { sb.eps = w.eps; sb.n_eps = (long long)B3 * D; eps = w.eps; }
    if (training && io.enc_dropout && !m1) { sb.mask[0] = w.m1; sb.n_mask[0] = (long long)2 * B * 400; m1 = w.m1; }
    if (training && io.enc_dropout && !m2) { sb.mask[1] = w.m2; sb.n_mask[1] = (long long)2 * B * 200; m2 = w.m2; }
    if (training && io.gru_dropout && !gk) { sb.mask[2] = w.gkeep; sb.n_mask[2] = (long long)4 * B3 * P.H; gk = w.gkeep; }
    const int skipb = mmvae_knob(K_dbg_begin_skip);              // measurement aid (results are garbage): 1 no pack, 2 no random draws, 4 no workspace zeroing
    if (skipb & 2) { sb.eps = nullptr; sb.mask[0] = sb.mask[1] = sb.mask[2] = nullptr; }
    if (skipb & 4) sb.zero_ptr[0] = nullptr;
    const bool pack_now = io.pack_first && !(skipb & 1);
    if (pack_now) {
        MMVAE_TRY(step_begin_with_pack(sb, P.buf.desc_dev, P.pk.d.data(), (int)P.pk.d.size(), P.buf.params, P.buf.packed, P.buf.packed_vec,
                                       staged ? 1u << 0 : 0u));
    }
    MMVAE_TRY(ensure_streams(P));
    P.in_step = true;
    {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        P.capturing = hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
    }
    arm_fork(P);                    // the text path forks off the prologue kernel's completion
    MMVAE_TRY(launch_step_begin(sb, s));
    MMVAE_TRY(commit_fork(P, s));
    if (do_backward && P.nparams % 4 != 0)
        MMVAE_TRY(launch_fill_zero(P.buf.grads + (P.nparams / 4) * 4, (size_t)(P.nparams % 4) * sizeof(float), s));
    const int enc_drop = training && io.enc_dropout;
    // weak-supervision variants (multimnist/paired_weak.py:84-117, modal_weak.py:87-117): an absent pass contributes no
    // loss, no gradient and no BatchNorm running-statistics update; its rows are still computed (batched with the others)
    const int sk[3] = {io.pass_skip[0] != 0, io.pass_skip[1] != 0, io.pass_skip[2] != 0};
    P.dec_skip_mask = (unsigned)(sk[0] | (sk[1] << 1) | (sk[2] << 2));
    const int enc_updates = 2 - sk[0] - sk[1];
    const bool serial = mmvae_serial();      // profiling aid: one stream, no overlap
    hipStream_t T = serial ? s : P.st_text;
    // ---- encoders: image features once for passes 1 and 2 (main), text encoder once for passes 1 and 3 (side)
    if (T != s) MMVAE_TRY(fork_to(P, T));
    if (staged && pack_now) {       // stage 1: the text copies, in front of the text encoder
        StepBeginArgs st1{};
        MMVAE_TRY(step_begin_with_pack(st1, P.buf.desc_dev, P.pk.d.data(), (int)P.pk.d.size(), P.buf.params, P.buf.packed, P.buf.packed_vec, 1u << 1));
        MMVAE_TRY(launch_step_begin(st1, T));
    }
    {
        TextEncArgs a = te_args(P, io.text, w.txtout, do_backward);
        MMVAE_TRY(launch_text_encoder_fwd(a, T));
    }
    if (staged && (pack_now || sb2.zero_ptr[1] || sb2.zero_ptr[2])) {      // stage 2: gradient buffers + the copies of the decoders / the backward pass
        if (pack_now)
            MMVAE_TRY(step_begin_with_pack(sb2, P.buf.desc_dev, P.pk.d.data(), (int)P.pk.d.size(), P.buf.params, P.buf.packed, P.buf.packed_vec, 1u << 2));
        MMVAE_TRY(launch_step_begin(sb2, T));
    }
    P.step_image = io.image;
    // B % 8: the fused layers have no fallback kernel ("forced" launches) and conv4's geometry is compiled for 8 images per
    // workgroup only; other batch sizes run the unfused bn_act + gather-GEMM chain
    const bool fuse = mmvae_knob(K_mm_fuse_bn) != 0 && mmvae_knob(K_convres) != 0 && B % 8 == 0;
    MMVAE_TRY(enc_fwd(P, io.image, 2, m1, m2, enc_drop, training, enc_updates, w.encout, s, fuse));
    MMVAE_TRY(edge(P, T, s));
    // ---- product of experts + reparametrisation + KL for the three passes
    Latent3Args la{};
    la.B = B; la.D = D; la.img_out = w.encout; la.txt_out = w.txtout; la.eps = eps;
    la.mu = io.mu ? io.mu : w.mu; la.logvar = io.logvar ? io.logvar : w.logvar;
    la.z_f32 = w.z_f32; la.z_bf = w.z_bf; la.ldz = P.ldz; la.kl_sum = w.sums + 8; la.training = training;
    arm_fork(P);
    MMVAE_TRY(launch_latent3_fwd(la, s));
    MMVAE_TRY(commit_fork(P, s));
    // ---- text decoder (forward, backward and its weight gradients) on the side stream, image decoder on main
    if (T != s) MMVAE_TRY(fork_to(P, T));
    TextDecArgs td = td_args(P, w.z_f32, 3, do_backward);
    td.keep = (training && io.gru_dropout) ? gk : nullptr; td.keep_scale = 1.f / (1.f - DROP_P);
    td.force_tokens = io.force_tokens;
    if (io.recon_text) td.words = io.recon_text;
    if (io.tokens) td.tokens_out = io.tokens;
    td.target = io.text; td.nll_sum = w.sums + 4; td.dwords = do_backward ? w.dwords : nullptr;
    for (int k = 0; k < 3; ++k) td.nll_coef[k] = sk[k] ? 0.f : io.lambda_yx[k] / (float)(B * TXT_T);
    if (const int half = mmvae_knob(K_dbg_text_rows_div)) td.R = max(16, td.R / half);      // measurement aid (garbage results): the text decoder on a fraction of its rows
    MMVAE_TRY(launch_text_decoder_fwd(td, T));
    if (do_backward) MMVAE_TRY(txt_dec_bwd(P, td, w.dwords, w.dz_txt, T));
    // decoders on 3B rows, BatchNorm statistics per pass; last layer fused with sigmoid + BCE (+ gradient)
    ConvTLastFwdArgs last{};
    last.target = io.image; last.recon = io.recon_image; last.dlogit = do_backward ? w.dlogit : nullptr; last.loss_sum = w.sums;
    for (int k = 0; k < 3; ++k) last.coef[k] = sk[k] ? 0.f : io.lambda_xy[k] / (float)(B * NPIX);
    // the last layer (no BatchNorm after it) of a trailing pass whose image term has weight 0 and whose reconstruction is
    // not asked for feeds nothing: multimnist/train.py:164-166 multiplies that pass's BCE by lambda_xy = 0
    int last_groups = 3;
    if (!io.recon_image)
        while (last_groups > 1 && last.coef[last_groups - 1] == 0.f) --last_groups;
    // image decoder backward runs for the leading groups with a non-zero image term (a pass with lambda_xy = 0 has exactly
    // zero gradient); the fused tail needs to know it already in the forward
    int img_groups = 3;
    while (img_groups > 0 && (io.lambda_xy[img_groups - 1] == 0.f || sk[img_groups - 1])) --img_groups;
    const bool fuse_tail = P.slab.pool != nullptr;
    MMVAE_TRY(dec_fwd(P, 3, training, &last, s, last_groups, fuse_tail ? (do_backward ? std::min(img_groups, last_groups) : 0) : -1, fuse));
    if (!do_backward) {
        MMVAE_TRY(edge(P, T, s));
        P.in_step = false;
        hipLaunchKernelGGL(sum_slots_kernel, dim3(1), dim3(64), 0, s, w.sums, io.sums);
        return mmvae_check_launch("sum_slots");
    }

    // =============================== backward ===============================
    // knob mm_wgrad_inline: the image path's weight gradients stay on the main stream, right behind the data gradient that made
    // their operands (no fork, no join, no contention with the main chain's kernels; 2: their partial copies summed by ONE launch
    // in front of the optimizer instead of one per layer)
    P.wgrad_forked = mmvae_knob(K_mm_wgrad_inline) == 0;
    int rc = MMVAE_OK;
    P.deferred.clear();
    P.defer_wgrad = false;
    if (img_groups > 0) rc = dec_bwd(P, w.dlogit, img_groups, w.dz_img, s, fuse_tail, fuse, 3, training);
    // ---- early optimizer part (mmvae_mm_step_io::early_adam): every gradient of image_decoder.* is complete on the weight-gradient stream (its
    //      last flush forked off the first layer's data gradient, which also closed the BatchNorm parameter gradients), text_decoder.*
    //      behind ev_txtgrads on the second-modality stream.  Their Adam update runs in the gap that stream has until the encoders'
    //      weight gradients arrive, beside the encoders' backward -- the optimizer launch behind the step shrinks to the encoders' ranges.
    if (io.early_adam && rc == MMVAE_OK && img_groups > 0 && fuse && fuse_tail && P.wgrad_forked && !serial && T != s && !io.dp_split &&
        io.defer_unpack && P.ev_txtgrads && P.side_pending.empty() && P.st_wgrad2 == P.st_wgrad && mmvae_knob(K_mm_early_adam)) {
        hipStream_t Wst = P.st_wgrad;
        AdamArgs ad{};
        const mmvae_early_adam& ea = *io.early_adam;
        ad.p = P.buf.params; ad.g = P.buf.grads; ad.m = ea.m; ad.v = ea.v; ad.n = P.nparams; ad.step = ea.state;
        ad.lr = ea.lr; ad.b1 = ea.beta1; ad.b2 = ea.beta2; ad.eps = ea.eps; ad.grad_scale = ea.grad_scale;
        ad.gmap = ea.gmap; ad.gpk = P.buf.gpk; ad.gpk_vec = P.buf.gpk_vec; ad.g_out = P.buf.grads;
        long long rg[8];
        ad.nr = mm_early_ranges(&P, rg, 4);
        for (int r = 0; r < ad.nr; ++r) { ad.roff[r] = rg[2 * r]; ad.rlen[r] = rg[2 * r + 1]; }
        ad.no_advance = 1;
        if (ad.nr > 0) {
            if (hipStreamWaitEvent(Wst, P.ev_txtgrads, 0) != hipSuccess) { mmvae_set_error("early optimizer part: %s", hipGetErrorString(hipGetLastError())); rc = MMVAE_EHIP; }
            if (rc == MMVAE_OK) rc = launch_adam(ad, Wst);
            if (rc == MMVAE_OK) *ea.ran = 1;
        }
    }
    if (rc == MMVAE_OK) {                            // dz of the text decoder
        const int k = mmvae_knob(K_dbg_skip_edges);
        if (P.ev_dz && T != s) {
            if (k != 1 && k != 3 && hipStreamWaitEvent(s, P.ev_dz, 0) != hipSuccess) {
                mmvae_set_error("stream join failed: %s", hipGetErrorString(hipGetLastError()));
                rc = MMVAE_EHIP;
            }
        } else {
            rc = edge(P, T, s);
        }
    }
    const bool dp_split = io.dp_split && !io.defer_unpack;
    if (dp_split && rc == MMVAE_OK) {
        // Data-parallel step: every gradient of image_decoder.* and text_decoder.* has been issued -- on s (which has just
        // joined T) and on the weight-gradient streams.  T is idle until the text encoder's backward: it waits for those
        // streams, scatters the early descriptors into the flat gradient buffer and marks the event the collective waits on.
        rc = edge(P, s, T);
        if (rc == MMVAE_OK && P.st_wgrad != T) rc = edge(P, P.st_wgrad, T);
        if (rc == MMVAE_OK && P.st_wgrad2 != P.st_wgrad && P.st_wgrad2 != T) rc = edge(P, P.st_wgrad2, T);
        if (rc == MMVAE_OK) rc = launch_wgrad_reduce(&P.slab, T);
        if (rc == MMVAE_OK)
            rc = plan_unpack(P, T, false, 1);
        if (rc == MMVAE_OK) {
            if (!P.ev_early) hipEventCreateWithFlags(&P.ev_early, hipEventDisableTiming);
            if (hipEventRecord(P.ev_early, T) != hipSuccess) { mmvae_set_error("early-gradient event failed"); rc = MMVAE_EHIP; }
        }
    }
    Latent3BwdArgs lb{};
    lb.f = la; lb.dz_a = w.dz_img; lb.dz_b = w.dz_txt;
    for (int k = 0; k < 3; ++k) lb.kl_coef[k] = sk[k] ? 0.f : io.kl_lambda / (float)B;
    lb.d_img_out_bf = w.d_encout; lb.ld_img_out_bf = P.lde; lb.d_img_bias = P.buf.grads + P.fc[2].b_off; lb.d_txt_out = w.d_txtout;
    lb.loss_slots = w.sums; lb.loss_out = io.sums;      // every loss term is final here (text-decoder NLL joined above)
    if (rc == MMVAE_OK) {
        arm_fork(P);                // the text encoder's backward and classifier.6's weight gradient fork off this kernel
        rc = launch_latent3_bwd(lb, s);
        if (rc == MMVAE_OK) rc = commit_fork(P, s);
    }
    if (rc == MMVAE_OK) rc = flush_wgrads(P, s);
    if (rc == MMVAE_OK && T != s) rc = fork_to(P, T);
    if (rc == MMVAE_OK) rc = txt_enc_bwd(P, io.text, w.d_txtout, T);
    if (rc == MMVAE_OK) rc = enc_bwd(P, w.d_encout, 2, m1, m2, enc_drop, s, fuse);
    P.wgrad_forked = false;
    P.in_step = false;
    MMVAE_TRY(rc);
    MMVAE_TRY(join_sides(P, T, s));
    MMVAE_TRY(launch_wgrad_reduce(&P.slab, s));
    if (dp_split) return plan_unpack(P, s, false, 0);
    if (!io.defer_unpack) MMVAE_TRY(plan_unpack(P, s, true));
    return MMVAE_OK;
}
int mm_wait_early_grads(MMPlan* P, hipStream_t s) {
    MMVAE_REQUIRE(P && P->ev_early, "mm_wait_early_grads: no dp_split step has run on this plan");
    if (hipStreamWaitEvent(s, P->ev_early, 0) != hipSuccess) {
        mmvae_set_error("mm_wait_early_grads: %s", hipGetErrorString(hipGetLastError()));
        return MMVAE_EHIP;
    }
    return MMVAE_OK;
}

// ---------------------------------------------------------------- image-only VAE (multimnist/model.py ImageVAE, multimnist/train_imageonly.py)
// The counterpart of img_tower.h tower_image_step on this family's own tower: zero_grad, ONE forward of B rows (encoder with one
// dropout variant and one BatchNorm update, the one-expert latent block -- no product of experts --, decoder with one BatchNorm
// group, sigmoid + BCE) and its backward, in the one-pass carve.  The launches are the module entry points' (the staged conv
// forms, conv1.hip's in-step form and the fused decoder tail's backward groups are built for 3 groups / 2 variants and stay
// with the 3-pass step); weight gradients go to the side stream.  Nothing of the text half is launched: its gradients stay at
// the zero of the prologue.
// The middle of that chain -- classifier.3, classifier.6, latent1 (+ finish), then upsample.0; backward latent1 (+ finish), two
// data gradients -- is launch latency on the critical path.  Where the latent size is compiled (mlp2_latent1_compiled) and the
// knob mm_image_waist is on, the waist pair of mlp_tail.hip replaces it: one launch per direction on the main chain.
// default of mm_image_waist per compiled size, from profiles/imageonly_mm_bench.txt: at n_latents = 20 the waist wins at B = 256 (0.541
// against 0.565 ms, spread 0.003) and ties at B = 128; at n_latents = 100, where the chain already has mlp2_fwd / mlp2_bwd, it does
// not win (B = 128: 0.494 against 0.485 ms, B = 256 a tie)
static int mm_image_waist_default(int D) { return D == 20 ? 1 : 0; }
// the encoder with its latent block, and their backward, either way; `tail_only`: classifier.3 onwards / down to classifier.0's output
// gradient, on the buffers an earlier step left in the workspace (mm_image_middle_replay)
struct ImageMiddle {
    bool waist; int training, enc_drop;
    const float* eps; const uint8_t *m1, *m2; float *mu, *logvar;
    const float* dz; float kl_coef; float* loss_out;
};
static Latent1Args image_latent_args(MMPlan& P, const ImageMiddle& m) {
    MMPlan::W& w = P.w;
    Latent1Args la{};
    la.B = P.B; la.D = P.D; la.enc_out = w.encout; la.eps = m.eps; la.mu = m.mu; la.logvar = m.logvar;
    la.z_f32 = w.z_f32; la.z_bf = w.z_bf; la.ldz = P.ldz; la.kl_sum = w.sums + 8; la.training = m.training;
    la.scratch = w.tmp_f32;         // (the module decoder's sigmoid-backward buffer: nobody else's in this step)
    return la;
}
static int image_middle_fwd(MMPlan& P, const ImageMiddle& m, const float* image, hipStream_t s, bool tail_only = false) {
    MMPlan::W& w = P.w;
    if (m.waist) {
        Mlp2Latent1FwdArgs wf{};
        wf.D = P.D; wf.ldz = P.ldz; wf.training = m.training; wf.eps = m.eps; wf.mu = m.mu; wf.logvar = m.logvar;
        wf.z_f32 = w.z_f32; wf.z_bf = w.z_bf; wf.scratch = reinterpret_cast<double*>(w.tmp_f32);
        return enc_fwd(P, image, 1, m.m1, m.m2, m.enc_drop, m.training, 1, w.encout, s, false, &wf, tail_only);
    }
    MMVAE_TRY(enc_fwd(P, image, 1, m.m1, m.m2, m.enc_drop, m.training, 1, w.encout, s, false, nullptr, tail_only));
    return launch_latent1_fwd(image_latent_args(P, m), s);
}
static int image_middle_bwd(MMPlan& P, const ImageMiddle& m, hipStream_t s, bool tail_only = false) {
    MMPlan::W& w = P.w;
    if (m.waist) {
        Mlp2Latent1BwdArgs wb{};
        wb.D = P.D; wb.training = m.training; wb.mu = m.mu; wb.logvar = m.logvar; wb.eps = m.eps; wb.dz = m.dz;
        wb.kl_coef = m.kl_coef; wb.scratch = reinterpret_cast<double*>(w.tmp_f32);
        return enc_bwd(P, w.d_encout, 1, m.m1, m.m2, m.enc_drop, s, false, &wb, m.loss_out, tail_only);
    }
    Latent1BwdArgs lb{};
    lb.f = image_latent_args(P, m); lb.dz = m.dz; lb.kl_coef = m.kl_coef;
    lb.d_enc_out = w.d_encout; lb.ld = P.lde; lb.d_bias = P.buf.grads + P.fc[2].b_off;
    lb.loss_slots = w.sums; lb.loss_out = m.loss_out;      // (BCE and KL sums are final here)
    MMVAE_TRY(launch_latent1_bwd(lb, s));
    return enc_bwd(P, w.d_encout, 1, m.m1, m.m2, m.enc_drop, s, false, nullptr, nullptr, tail_only);
}
static int mm_image_step_body(MMPlan* Pp, const mmvae_image_step_io& io, int training, int do_backward, hipStream_t s) {
    MMVAE_TRY(use_ws(Pp, io.ws, io.ws_bytes));
    MMPlan& P = *Pp;
    MMPlan::W& w = P.w;
    const int B = P.B, D = P.D;
    MMVAE_REQUIRE(io.image && io.sums, "image step: image/sums must be given");
    const int wk = mmvae_knob(K_mm_image_waist);          // 1 / 0: on / off where compiled; -1 (not set): the size's default
    ImageMiddle m{};
    m.waist = P.waist && (wk < 0 ? mm_image_waist_default(D) : wk) != 0;
    MMVAE_REQUIRE(launch_latent1_scratch_floats(B, D) <= (size_t)B * NPIX && 2 * mlp2_latent1_scratch_doubles(B, D) <= (size_t)B * NPIX,
                  "image step: no room for the latent block's partial sums");
    m.training = training; m.enc_drop = training && io.enc_dropout;
    m.eps = io.eps; m.m1 = io.enc_mask1; m.m2 = io.enc_mask2;
    StepBeginArgs sb{};
    sb.zero_ptr[0] = w.zero_begin; sb.zero_bytes[0] = w.zero_bytes;
    if (do_backward) {
        sb.zero_ptr[1] = P.buf.gpk; sb.zero_bytes[1] = (size_t)P.gk.mat_elems * sizeof(float);
        sb.zero_ptr[2] = P.buf.grads; sb.zero_bytes[2] = (size_t)(P.nparams / 4) * 16;
    }
    sb.p = DROP_P; sb.seed = io.seed; sb.step = io.step_counter;
    if (training && !m.eps) { sb.eps = w.eps; sb.n_eps = (long long)B * D; m.eps = w.eps; }
    if (m.enc_drop && !m.m1) { sb.mask[0] = w.m1; sb.n_mask[0] = (long long)B * 400; m.m1 = w.m1; }
    if (m.enc_drop && !m.m2) { sb.mask[1] = w.m2; sb.n_mask[1] = (long long)B * 200; m.m2 = w.m2; }
    MMVAE_TRY(launch_step_begin(sb, s));
    if (do_backward && P.nparams % 4 != 0)
        MMVAE_TRY(launch_fill_zero(P.buf.grads + (P.nparams / 4) * 4, (size_t)(P.nparams % 4) * sizeof(float), s));
    MMVAE_TRY(ensure_streams(P));
    P.in_step = true;               // (dec_bwd binds its forks to kernel completions: arm_fork / commit_fork)
    {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        P.capturing = hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
    }
    m.mu = io.mu ? io.mu : w.mu;
    m.logvar = io.logvar ? io.logvar : w.logvar;
    MMVAE_TRY(image_middle_fwd(P, m, io.image, s));
    ConvTLastFwdArgs last{};
    last.target = io.image; last.recon = io.recon_image; last.dlogit = do_backward ? w.dlogit : nullptr; last.loss_sum = w.sums;
    last.coef[0] = io.lambda_x / (float)(B * NPIX);
    MMVAE_TRY(dec_fwd(P, 1, training, &last, s));
    if (!do_backward) {
        P.in_step = false;
        if (m.waist)                // (the KL partials are folded here, behind the decoder: not between the waist and upsample.0)
            return launch_mlp2_latent1_finish(reinterpret_cast<double*>(w.tmp_f32), B, D, nullptr, w.sums, io.sums, s);
        hipLaunchKernelGGL(sum_slots_kernel, dim3(1), dim3(64), 0, s, w.sums, io.sums);
        return mmvae_check_launch("sum_slots");
    }
    // =============================== backward ===============================
    P.wgrad_forked = true;
    P.deferred.clear();
    P.defer_wgrad = false;
    int rc = MMVAE_OK;
    const bool img_term = io.lambda_x != 0.f;        // (a zero weight has exactly no gradient)
    if (img_term) rc = dec_bwd(P, w.dlogit, 1, w.dz_img, s);
    m.dz = img_term ? w.dz_img : nullptr; m.kl_coef = io.kl_lambda / (float)B; m.loss_out = io.sums;
    if (rc == MMVAE_OK) rc = image_middle_bwd(P, m, s);
    P.wgrad_forked = false;
    P.in_step = false;
    MMVAE_TRY(rc);
    MMVAE_TRY(join_sides(P, s, s));
    if (io.defer_unpack) return launch_wgrad_reduce(&P.slab, s);      // the packed gradients are complete; Adam gathers them
    return plan_unpack(P, s, true);
}
// Test aid (mm_bench_layer "image_step:waist_fwd" | "chain_fwd" | "waist_bwd" | "chain_bwd"): the middle of the image-only step again --
// classifier.3 to z, or dz back to classifier.0's output gradient -- with the waist or with the unfused chain, in training mode with
// dropout, on what a step that DREW its eps and masks (and got no mu / logvar buffers) left in its one-pass workspace, kl_lambda =
// 1e-3.  Two steps do not hand the middle the same bits (the conv towers' BatchNorm sums are fp32 atomics), two replays do.  The
// backward adds to the bias gradients of classifier.0 / .3 / .6 and writes `sums` (the workspace's loss slots summed) to loss_out.
static int mm_image_middle_replay(MMPlan* Pp, void* ws, size_t wsb, const std::string& what, hipStream_t s) {
    MMVAE_REQUIRE(what == "waist_fwd" || what == "chain_fwd" || what == "waist_bwd" || what == "chain_bwd", "bench_layer: unknown layer 'image_step:%s'", what.c_str());
    MMVAE_TRY(use_ws(Pp, ws, wsb));
    MMPlan& P = *Pp;
    MMPlan::W& w = P.w;
    ImageMiddle m{};
    m.waist = what.compare(0, 5, "waist") == 0;
    MMVAE_REQUIRE(!m.waist || P.waist, "bench_layer: no waist is compiled for n_latents = %d", P.D);
    m.training = 1; m.enc_drop = 1; m.eps = w.eps; m.m1 = w.m1; m.m2 = w.m2; m.mu = w.mu; m.logvar = w.logvar;
    m.dz = w.dz_img; m.kl_coef = 1e-3f / (float)P.B; m.loss_out = w.tmp_f32 + (size_t)P.B * NPIX - 16;
    if (what.compare(6, 3, "fwd") == 0) return image_middle_fwd(P, m, nullptr, s, true);
    MMVAE_TRY(image_middle_bwd(P, m, s, true));
    return launch_wgrad_reduce(&P.slab, s);
}
size_t mm_image_step_workspace_bytes(const MMPlan* P) { return P->ws_bytes_module; }
int mm_image_step(MMPlan* P, const mmvae_image_step_io& io, int training, int do_backward, hipStream_t s) {
    return plan_step(P, io, training, do_backward, s, mm_image_step_body);
}

// ---------------------------------------------------------------- granular module entry points (drop-in modules)
// Every call gets its own workspace (saved activations live there until the matching backward).
int mm_image_encoder_fwd(MMPlan* P, void* ws, size_t wsb, const float* image, const uint8_t* m1, const uint8_t* m2,
                         int training, float* out, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    MMPlan::W& w = P->w;
    MMVAE_TRY(launch_fill_zero(w.zero_begin, w.zero_bytes, s));
    return enc_fwd(*P, image, 1, m1, m2, training && m1 != nullptr, training, 1, out, s);
}
// bf16 copy of x [rows][cols] with row stride ld >= cols, pad columns zero
static __global__ void cast_rows_pad_kernel(const float* x, int rows, int cols, bf16* out, int ld) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * ld) return;
    int r = i / ld, c = i - r * ld;
    out[i] = (bf16)(c < cols ? x[(size_t)r * cols + c] : 0.0f);
}
int mm_image_encoder_bwd(MMPlan* P, void* ws, size_t wsb, const float* d_out, const uint8_t* m1, const uint8_t* m2, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    MMPlan::W& w = P->w;
    const int rows = P->B, D2 = 2 * P->D;
    MMVAE_TRY(plan_zero_gpk(*P, s));
    hipLaunchKernelGGL(cast_rows_pad_kernel, dim3(ceil_div(rows * P->lde, 256)), dim3(256), 0, s, d_out, rows, D2, w.d_encout, P->lde);
    hipLaunchKernelGGL(colsum_kernel, dim3(ceil_div(D2, 64)), dim3(64), 0, s, d_out, rows, D2, P->buf.grads + P->fc[2].b_off);
    MMVAE_TRY(mmvae_check_launch("image encoder bwd prologue"));
    MMVAE_TRY(enc_bwd(*P, w.d_encout, 1, m1, m2, m1 != nullptr, s));
    return plan_unpack(*P, s, true);
}
int mm_image_decoder_fwd(MMPlan* P, void* ws, size_t wsb, const float* z, int training, float* recon, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    MMPlan::W& w = P->w;
    const int rows = P->B;
    MMVAE_TRY(launch_fill_zero(w.zero_begin, w.zero_bytes, s));
    hipLaunchKernelGGL(cast_z_kernel, dim3(ceil_div(rows * P->ldz, 256)), dim3(256), 0, s, z, rows, P->D, w.z_bf, P->ldz);
    MMVAE_TRY(mmvae_check_launch("cast_z"));
    ConvTLastFwdArgs last{};
    last.recon = recon;
    return dec_fwd(*P, 1, training, &last, s);
}
int mm_image_decoder_bwd(MMPlan* P, void* ws, size_t wsb, const float* d_recon, const float* recon, float* dz, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    MMPlan::W& w = P->w;
    const int rows = P->B;
    MMVAE_TRY(plan_zero_gpk(*P, s));
    hipLaunchKernelGGL(sigmoid_bwd_kernel, dim3(ceil_div(rows * NPIX, 256)), dim3(256), 0, s, d_recon, recon, (long long)rows * NPIX, w.dlogit);
    MMVAE_TRY(mmvae_check_launch("sigmoid_bwd"));
    MMVAE_TRY(dec_bwd(*P, w.dlogit, 1, dz, s));
    return plan_unpack(*P, s, true);
}
int mm_text_encoder_fwd(MMPlan* P, void* ws, size_t wsb, const long long* text, float* out, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    TextEncArgs a = te_args(*P, text, out, true);
    return launch_text_encoder_fwd(a, s);
}
int mm_text_encoder_bwd(MMPlan* P, void* ws, size_t wsb, const long long* text, const float* d_out, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    MMVAE_TRY(plan_zero_gpk(*P, s));
    MMVAE_TRY(txt_enc_bwd(*P, text, d_out, s));
    return plan_unpack(*P, s, true);
}
int mm_text_decoder_fwd(MMPlan* P, void* ws, size_t wsb, const float* z, int training, const uint8_t* keep,
                        const long long* force_tokens, float* words, long long* tokens, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    TextDecArgs a = td_args(*P, z, 1, true);
    a.keep = training ? keep : nullptr; a.keep_scale = 1.f / (1.f - DROP_P);
    a.force_tokens = force_tokens; a.words = words; a.tokens_out = tokens;
    return launch_text_decoder_fwd(a, s);
}
int mm_text_decoder_bwd(MMPlan* P, void* ws, size_t wsb, const float* z, const uint8_t* keep, const long long* force_tokens,
                        const float* words, const long long* tokens, const float* d_words, float* dz, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    MMVAE_TRY(plan_zero_gpk(*P, s));
    TextDecArgs a = td_args(*P, z, 1, true);
    a.keep = keep; a.keep_scale = 1.f / (1.f - DROP_P);
    a.force_tokens = force_tokens; a.words = const_cast<float*>(words); a.tokens_out = const_cast<long long*>(tokens);
    MMVAE_TRY(txt_dec_bwd(*P, a, d_words, dz, s));
    return plan_unpack(*P, s, true);
}

// ---------------------------------------------------------------- importance-weighted evaluation (iw.h)
// Eval-mode decoders on the B*K particle rows z [B][K][D]: the image decoder ends in the scoring form of the fused tail (one
// log p(x|z) per row, against the row's own example), the text decoder writes its greedy log-softmax outputs.  No backward
// activations are kept and the BatchNorm running statistics are not touched.
// the image half: particles -> z_bf, eval-mode decoder, scoring tail (`who`: the entry point, for its messages)
static int iw_image_rows(MMPlan* P, void* ws, size_t wsb, const float* z, const float* image, int B, int K, float* loglik_x, hipStream_t s,
                         const char* who) {
    MMVAE_REQUIRE(B >= 1 && K >= 1 && (long long)B * K <= P->B, "%s: %d examples x %d particles exceed the plan's %d rows", who, B, K, P->B);
    MMVAE_TRY(use_ws(P, ws, wsb));
    MMPlan::W& w = P->w;
    const int rows = B * K;
    MMVAE_TRY(launch_fill_zero(w.zero_begin, w.zero_bytes, s));
    hipLaunchKernelGGL(cast_z_kernel, dim3(ceil_div(rows * P->ldz, 256)), dim3(256), 0, s, z, rows, P->D, w.z_bf, P->ldz);
    MMVAE_TRY(mmvae_check_launch("cast_z"));
    ConvTLastFwdArgs last{};
    last.target = image; last.loglik = loglik_x; last.rows_per_target = K; last.rows = rows;
    return dec_fwd(*P, 1, 0, &last, s, -1, 0);
}
int mm_iw_score(MMPlan* P, void* ws, size_t wsb, const float* z, const float* image, int B, int K, float* loglik_x, float* words,
                hipStream_t s) {
    MMVAE_REQUIRE(P && z && image && loglik_x && words, "mmvae_mm_iw_score: null argument");
    MMVAE_TRY(iw_image_rows(P, ws, wsb, z, image, B, K, loglik_x, s, "mmvae_mm_iw_score"));
    TextDecArgs a = td_args(*P, z, 1, false);
    a.R = B * K; a.words = words;
    return launch_text_decoder_fwd(a, s);
}
// log p(x | z) of the particle rows alone: the image-only VAE has no text decoder to run
int mm_iw_score_image(MMPlan* P, void* ws, size_t wsb, const float* z, const float* image, int B, int K, float* loglik_x, hipStream_t s) {
    MMVAE_REQUIRE(P && z && image && loglik_x, "mmvae_mm_iw_score_image: null argument");
    return iw_image_rows(P, ws, wsb, z, image, B, K, loglik_x, s, "mmvae_mm_iw_score_image");
}

// ---------------------------------------------------------------- test / profiling aid: replay one launch of the step (mm_bench_layer)
// The launches of mm_gemm / mm_wgrad under names, in the form the default training step runs them: training mode, the classifier on
// its 2 dropout variants with the keep flags in w.m1 / w.m2 (as drawn by the last step), the decoder with 3 passes forward and 2
// backward (2 of 3 passes carry an image gradient).  Statistics land in the (dead) accumulation buffers of the last step.  What the
// step writes into the caller's buffers or the flat gradient goes to tmp_f32 instead: the result of enc_fc3 and dec_up_dgrad, the
// column sums of enc_fc3_dgrad / enc_fc2_dgrad; enc_fc3_dgrad reads d_encout.  The weight gradients read the operands of the
// unfused layers (dr[l] / dq[l + 1]).
static bool layer_gemm(MMPlan& P, const std::string& name, GemmParams& g) {
    MMPlan::W& w = P.w;
    if (name == "enc_conv1") { g = mm_gemm(P, MM_ENC_CONV1, 0, 1); return true; }
    for (int l = 1; l < 4; ++l) {
        const std::string n = "enc_conv" + std::to_string(l + 1);
        if (name == n) { g = mm_gemm(P, MM_ENC_CONV, l, 1); return true; }
        if (name == n + "_dgrad") { g = mm_gemm(P, MM_ENC_CONV_DGRAD, l, 1); return true; }
    }
    if (name == "enc_fc1") { g = mm_gemm(P, MM_FC1, 0, 2, 1, w.m1); return true; }
    if (name == "enc_fc1_dgrad") { g = mm_gemm(P, MM_FC1_DGRAD, 0, 2); return true; }
    if (name == "enc_fc2") { g = mm_gemm(P, MM_FC2, 0, 2, 1, w.m2); return true; }
    if (name == "enc_fc3") { g = mm_gemm(P, MM_FC3, 0, 2, 1, nullptr, w.tmp_f32); return true; }
    if (name == "enc_fc3_dgrad") { g = mm_gemm(P, MM_FC3_DGRAD, 0, 2, 1, w.m2, w.d_encout, w.tmp_f32); return true; }
    if (name == "enc_fc2_dgrad") { g = mm_gemm(P, MM_FC2_DGRAD, 0, 2, 1, w.m1, nullptr, w.tmp_f32); return true; }
    if (name == "dec_up") { g = mm_gemm(P, MM_UP, 0, 3); return true; }
    if (name == "dec_up_dgrad") { g = mm_gemm(P, MM_UP_DGRAD, 0, 2, 1, nullptr, w.tmp_f32); return true; }
    for (int l = 0; l < 3; ++l) {
        const std::string n = "dec_convT" + std::to_string(l + 1);
        if (name == n) { g = mm_gemm(P, MM_DEC_CONVT, l, 3); return true; }
        if (name == n + "_dgrad") { g = mm_gemm(P, MM_DEC_CONVT_DGRAD, l, 2); return true; }
    }
    if (name == "dec_last_dgrad_gemm") { g = mm_gemm(P, MM_DEC_LAST_DGRAD, 3, 2); return true; }
    return false;
}
static bool layer_wgrad(MMPlan& P, const std::string& name, WgradParams& g) {
    const MMChains t = mm_chains(P.w);
    if (name == "enc_conv1_wgrad") { g = mm_wgrad(P, MM_W_ENC_CONV1, 0, 1); return true; }
    for (int l = 1; l < 4; ++l)
        if (name == "enc_conv" + std::to_string(l + 1) + "_wgrad") { g = mm_wgrad(P, MM_W_ENC_CONV, l, 1, t.dr[l]); return true; }
    for (int l = 0; l < 3; ++l)
        if (name == "dec_convT" + std::to_string(l + 1) + "_wgrad") { g = mm_wgrad(P, MM_W_DEC_CONVT, l, 2, t.dq[l + 1]); return true; }
    if (name == "dec_last_wgrad") { g = mm_wgrad(P, MM_W_DEC_LAST, 3, 2); return true; }
    return false;
}
// FLOPs of one launch (GemmParams or WgradParams)
template <class Params>
static double launch_flops(const Params& g) {
    double f = 0;
    for (int i = 0; i < g.c.nclasses; ++i) f += 2.0 * g.c.groups * g.cls[i].rows_per_group * (double)g.c.N * g.cls[i].K;
    return f;
}
int mm_bench_layer(MMPlan* P, void* ws, size_t wsb, const char* layer, int iters, hipStream_t s) {
    if (std::strncmp(layer, "image_step:", 11) == 0) {      // the middle of mm_image_step, on its one-pass workspace
        for (int i = 0; i < iters; ++i) MMVAE_TRY(mm_image_middle_replay(P, ws, wsb, layer + 11, s));
        return MMVAE_OK;
    }
    MMVAE_TRY(use_ws(P, ws, wsb, false));
    // fused decoder tail as in the training step (2 of 3 passes carry a gradient).  "dec_last_fused_reduce": followed by the sum of
    // its weight-gradient partials into the packed gradient (the step makes it on a side stream), and with the optional outputs
    // logits / recon / dlogit written to the workspace buffers of those names
    if (std::string(layer) == "dec_last_fused" || std::string(layer) == "dec_last_fused_reduce") {
        const bool reduce = std::string(layer) == "dec_last_fused_reduce";
        ConvTLastFwdArgs last{};
        last.target = (const float*)P->w.tmp_f32; last.loss_sum = P->w.sums;
        last.coef[0] = last.coef[1] = 1.f / (float)(P->B * NPIX);
        if (reduce) { last.logits = P->w.logits; last.recon = P->w.recon; }
        for (int i = 0; i < iters; ++i) {
            P->slab.reset(P->w.slab, P->w.slab_floats);
            MMVAE_TRY(fused_tail(*P, 3, 1, &last, 2, 2, s, reduce ? P->w.dlogit : nullptr));
            if (reduce) MMVAE_TRY(launch_wgrad_reduce(&P->slab, s));
            P->slab.jobs.clear(); P->slab.ring_jobs.clear();
        }
        return MMVAE_OK;
    }
    // conv1.hip's forms as the fused step launches them; the image batch is read from the first B * 2500 floats of tmp_f32
    if (std::string(layer) == "enc_conv1_mfma") {
        const PackDesc& d = P->pk.d[P->conv[0].pk_fwd[0]];
        for (int i = 0; i < iters; ++i)
            MMVAE_TRY(launch_conv1_fwd_mfma(P->w.tmp_f32, P->B, P->buf.packed + d.dst_off, d.Kpad, P->w.r1, P->w.a1, s));
        return MMVAE_OK;
    }
    if (std::string(layer) == "enc_conv1_wgrad_mfma") {       // float atomics into the packed gradient: no slab, no reduce launch
        const PackDesc& gd = P->gk.d[P->conv[0].gk[0]];
        for (int i = 0; i < iters; ++i)
            MMVAE_TRY(launch_conv1_wgrad_mfma(P->w.tmp_f32, P->B, P->w.d1e, P->buf.gpk + gd.dst_off, gd.Kpad, s));
        return MMVAE_OK;
    }
    WgradParams wg{};
    if (layer_wgrad(*P, layer, wg)) {         // kernel + its share of the slab reduction, as in the step
        for (int i = 0; i < iters; ++i) {
            P->slab.reset(P->w.slab, P->w.slab_floats);
            MMVAE_TRY(launch_wgrad(wg, s, &P->slab));
            MMVAE_TRY(launch_wgrad_reduce(&P->slab, s));
        }
        return MMVAE_OK;
    }
    GemmParams g{};
    MMVAE_REQUIRE(layer_gemm(*P, layer, g), "bench_layer: unknown layer '%s'", layer);
    for (int i = 0; i < iters; ++i) MMVAE_TRY(launch_gemm_gather(g, s));
    return MMVAE_OK;
}
double mm_layer_flops(const MMPlan* Pc, const char* layer) {
    MMPlan& P = *const_cast<MMPlan*>(Pc);
    GemmParams g{};
    WgradParams wg{};
    if (std::string(layer) == "dec_last_fused" || std::string(layer) == "dec_last_fused_reduce")
        return 3.0 * 2.0 * 2 * P.B * 625 * 16 * 32;      // forward + both gradients, 2 passes
    if (std::string(layer) == "enc_conv1_mfma" || std::string(layer) == "enc_conv1_wgrad_mfma") return 2.0 * P.B * 640 * 16 * 32;   // 20 tiles of 32 rows
    if (P.bound && layer_wgrad(P, layer, wg)) return launch_flops(wg);
    if (!P.bound || !layer_gemm(P, layer, g)) return -1.0;
    return launch_flops(g);
}
// FLOPs of a layer the way torch's FlopCounterMode counts the reference: 2 * out_pixels * taps * Cin * Cout for a
// Conv2d, 2 * in_pixels * taps * Cin * Cout for a ConvTranspose2d, the same number again for each of the two gradients --
// padded / cropped taps are NOT subtracted by the counter, zero-padded GEMM columns of this engine are not added.
double mm_layer_algo_flops(const MMPlan* Pc, const char* layer) {
    const MMPlan& P = *Pc;
    const std::string name = layer;
    const int B = P.B;
    auto conv = [&](const ConvL& L, int images) {
        const ConvGeom& g = L.g;
        const double pix = g.transposed ? (double)g.IH * g.IW : (double)g.OH * g.OW;
        return 2.0 * pix * g.KH * g.KW * g.Cin * g.Cout * images;
    };
    for (int l = 0; l < 4; ++l) {
        const std::string e = "enc_conv" + std::to_string(l + 1), d = "dec_convT" + std::to_string(l + 1);
        if (name == e || name == e + "_dgrad" || name == e + "_wgrad") return conv(P.conv[l], B);
        if (name == d) return conv(P.convT[l], 3 * B);
        if (name == d + "_dgrad" || name == d + "_wgrad") return conv(P.convT[l], 2 * B);
    }
    if (name == "dec_last_wgrad" || name == "dec_last_dgrad_gemm") return conv(P.convT[3], 2 * B);
    if (name == "dec_last_fused" || name == "dec_last_fused_reduce") return 3.0 * conv(P.convT[3], 2 * B);
    if (name == "enc_conv1_mfma" || name == "enc_conv1_wgrad_mfma") return conv(P.conv[0], B);
    return mm_layer_flops(Pc, layer);          // dense layers: no padding in the count
}
// Algorithmic bytes of one conv-shaped layer launch: every operand tensor read once and the result written once (bf16
// activations / gradients, bf16 packed weights; the weight gradient is fp32).  What the launch would move with perfect
// reuse -- the PMC traffic of the same launch (profiles/r02_traffic.json) is compared against it.  0: not a conv layer.
double mm_layer_algo_bytes(const MMPlan* Pc, const char* layer) {
    const MMPlan& P = *Pc;
    const std::string name = layer;
    const int B = P.B;
    auto conv = [&](const ConvL& L, int images, bool wgrad) {
        const ConvGeom& g = L.g;
        const double act = (double)images * ((double)g.IH * g.IW * g.Cin + (double)g.OH * g.OW * g.Cout) * 2.0;
        return act + (double)g.Cin * g.Cout * g.KH * g.KW * (wgrad ? 4.0 : 2.0);
    };
    for (int l = 0; l < 4; ++l) {
        const std::string e = "enc_conv" + std::to_string(l + 1), d = "dec_convT" + std::to_string(l + 1);
        if (name == e || name == e + "_dgrad") return conv(P.conv[l], B, false);
        if (name == e + "_wgrad") return conv(P.conv[l], B, true);
        if (name == d) return conv(P.convT[l], 3 * B, false);
        if (name == d + "_dgrad") return conv(P.convT[l], 2 * B, false);
        if (name == d + "_wgrad") return conv(P.convT[l], 2 * B, true);
    }
    // conv1.hip reads the fp32 image itself (no patch buffer) and writes the raw and the Swish copy / reads the gradient
    if (name == "enc_conv1_mfma") return (double)B * (2500 * 4.0 + 2 * 625 * 32 * 2.0) + 32 * 16 * 2.0;
    if (name == "enc_conv1_wgrad_mfma") return (double)B * (2500 * 4.0 + 625 * 32 * 2.0) + 32 * 16 * 4.0;
    // fused tail, 2 passes: raw input read, input gradient written, the fp32 target image read once per pass
    if (name == "dec_last_fused" || name == "dec_last_fused_reduce") return 2.0 * B * (2 * 625 * 32 * 2.0 + 2500 * 4.0) + 32 * 16 * 4.0;
    return 0.0;
}
// ---------------------------------------------------------------- test aid: byte offset of a named workspace buffer
int mm_debug_pack_stage(MMPlan* Pp, int stage, int* blocks, hipStream_t s) {
    MMPlan& P = *Pp;
    StepBeginArgs sb{};
    MMVAE_TRY(step_begin_with_pack(sb, P.buf.desc_dev, P.pk.d.data(), (int)P.pk.d.size(), P.buf.params, P.buf.packed, P.buf.packed_vec,
                                   stage < 0 ? 0u : 1u << stage));
    if (blocks) *blocks = sb.pack_blocks;
    return launch_step_begin(sb, s);
}
long long mm_debug_offset(MMPlan* P, const char* name) {
    Workspace ws((void*)0x1000, (size_t)1 << 40);
    // "image_step:<name>": in the one-pass carve of mm_image_step (and of the module entry points)
    const bool one_pass = std::strncmp(name, "image_step:", 11) == 0;
    if (one_pass) name += 11;
    P->carve_passes = one_pass ? 1 : 3;
    carve(*P, ws);
    P->carve_passes = 3;
    MMPlan::W& w = P->w;
    std::map<std::string, const void*> m = {
        {"patches1", w.patches1}, {"r1", w.r1}, {"r2", w.r2}, {"r3", w.r3}, {"r4", w.r4}, {"y1", w.y1}, {"y2", w.y2},
        {"encout", w.encout}, {"txtout", w.txtout}, {"z_bf", w.z_bf}, {"z_f32", w.z_f32}, {"u", w.u}, {"q1", w.q1}, {"q2", w.q2},
        {"q3", w.q3}, {"logits", w.logits}, {"dlogit", w.dlogit}, {"d3", w.d3}, {"d2", w.d2}, {"d1", w.d1}, {"du", w.du},
        {"dz_img", w.dz_img}, {"dz_txt", w.dz_txt}, {"d_encout", w.d_encout}, {"d_txtout", w.d_txtout}, {"dy2", w.dy2},
        {"dy1", w.dy1}, {"db4", w.db4}, {"dr4", w.dr4}, {"d3e", w.d3e}, {"d2e", w.d2e}, {"d1e", w.d1e},
        {"aff_d0", w.aff_d[0]}, {"aff_d1", w.aff_d[1]}, {"aff_d2", w.aff_d[2]}, {"st_d0", w.st_d[0]}, {"patches4", w.patches4},
        {"tmp_f32", w.tmp_f32}, {"aff_e0", w.aff_e[0]}, {"aff_e1", w.aff_e[1]}, {"aff_e2", w.aff_e[2]},
        {"eps", w.eps}, {"m1", w.m1}, {"m2", w.m2}, {"gkeep", w.gkeep},
        {"st_e0", w.st_e[0]}, {"st_e1", w.st_e[1]}, {"st_e2", w.st_e[2]}, {"st_d1", w.st_d[1]}, {"st_d2", w.st_d[2]},
        {"red_e0", w.red_e[0]}, {"red_e1", w.red_e[1]}, {"red_e2", w.red_e[2]},
        {"red_d0", w.red_d[0]}, {"red_d1", w.red_d[1]}, {"red_d2", w.red_d[2]},
        {"a1", w.a1}, {"a2", w.a2}, {"a3", w.a3}, {"aq1", w.aq1}, {"aq2", w.aq2}, {"aq3", w.aq3},
        {"a4", w.a4}, {"au", w.au}, {"ay1", w.ay1}, {"ay2", w.ay2}, {"slab", w.slab},
        {"mr_e0", w.mr_e[0]}, {"mr_e1", w.mr_e[1]}, {"mr_e2", w.mr_e[2]}, {"mr_d0", w.mr_d[0]}, {"mr_d1", w.mr_d[1]}, {"mr_d2", w.mr_d[2]},
        {"mu", w.mu}, {"logvar", w.logvar}, {"recon", w.recon}, {"sums", w.sums},
    };
    auto it = m.find(name);
    if (it == m.end()) return -1;
    return (long long)((const char*)it->second - (const char*)0x1000);
}
