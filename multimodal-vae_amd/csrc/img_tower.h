// Private: the image half shared by celeba.hip and coco.hip -- an im2col conv1 and three k4 convolutions with BatchNorm + Swish,
// classifier.0 over the NHWC feature map, the upsample Linear, three transposed convolutions with per-pass BatchNorm and the last
// C -> 3 transposed convolution through 48-column patches.  What differs between the families is data (TowerGeom and the
// ConvGeom of each layer); classifier tails, the fused decoder tail and the second modality stay in the family's file.
//
// ONE definition per launch: every GemmParams / WgradParams and the arguments of every stand-alone pass are built here, for the
// step (tower_enc_fwd / tower_enc_bwd / tower_dec_fwd / tower_dec_bwd) and for the replay of one launch on a test's own operands
// (<family>_bench_layer): a test cannot pass on a copy of the parameters that drifted from the step.
#pragma once
#include "plan_base.h"
#include "thin.h"
#include "iw.h"
#include "mmd.h"
#include "../../include/mmvae_hip.h"
#include <map>
#include <string>

struct TowerGeom {
    int img;            // image side (3 x img x img)
    int s1, c1;         // conv1 output side / channels == input of the last transposed convolution
    int fs, fc;         // feature map side / channels
    int feat;           // fs * fs * fc
    int hid;            // width of classifier.0
};

// workspace buffers of the tower; the family's W derives from it and carves them in its own order
struct TowerW {
    float2 *st_e[3], *red_e[3], *st_d[3], *red_d[3], *aff_e[3], *mr_e[3], *aff_d[3], *mr_d[3];
    bf16 *patches1, *r1, *r2, *r3, *r4, *a1, *a2, *a3, *a4, *y1, *ay1;
    bf16* z_bf;
    bf16 *u, *au, *q1, *q2, *q3, *aq1, *aq2, *aq3;
    float* dlogit;
    bf16 *patches4, *d3, *d2, *d1, *du;
    bf16 *dy1, *db4, *dr4, *d3e, *d2e, *d1e;
    float* slab; size_t slab_floats;
};

struct TowerPlan : PlanBase {
    int ldz;
    ConvL conv[4], convT[4];
    LinL fc1, up;
    int fc1_dgrad;                // dense [FEAT][hid] packing of classifier.0 for its input gradient
    BnL bn[6];                    // features.3 / .6 / .9, hallucinate.1 / .4 / .7
    TowerGeom geo;
    TowerW* tw;                   // the family's workspace struct
};

// the tensors along the two conv chains, by layer: raw / activated / gradient
struct TowerChains { bf16 *r[4], *a[4], *dr[4], *q[4], *aq[4], *dq[4]; };
inline TowerChains tower_chains(const TowerW& w) {
    return TowerChains{{w.r1, w.r2, w.r3, w.r4}, {w.a1, w.a2, w.a3, w.a4}, {w.d1e, w.d2e, w.d3e, w.dr4},
                       {w.u, w.q1, w.q2, w.q3}, {w.au, w.aq1, w.aq2, w.aq3}, {w.du, w.d1, w.d2, w.d3}};
}

// ================================================================== build
// BatchNorm table and the eight conv layers; enc[l] / dec[l]: geometry of features / hallucinate layer l.  Returns the offset of
// the next BatchNorm's running statistics.  The three build functions add their pack descriptors in call order.
inline long long tower_build_convs(TowerPlan& P, const ConvGeom* enc, const ConvGeom* dec) {
    static const char* const bnn[6] = {"image_encoder.features.3", "image_encoder.features.6", "image_encoder.features.9",
                                       "image_decoder.hallucinate.1", "image_decoder.hallucinate.4", "image_decoder.hallucinate.7"};
    static const char* const en[4] = {"image_encoder.features.0.weight", "image_encoder.features.2.weight",
                                      "image_encoder.features.5.weight", "image_encoder.features.8.weight"};
    static const char* const dn[4] = {"image_decoder.hallucinate.0.weight", "image_decoder.hallucinate.3.weight",
                                      "image_decoder.hallucinate.6.weight", "image_decoder.hallucinate.9.weight"};
    P.ldz = round_up(P.D + 1, 8);
    long long so = 0;
    for (int i = 0; i < 6; ++i) {
        const int c = i < 3 ? enc[i + 1].Cout : dec[i - 3].Cout;
        P.bn[i] = BnL{off(P, std::string(bnn[i]) + ".weight"), off(P, std::string(bnn[i]) + ".bias"), c, so, i};
        P.bn_names.push_back(bnn[i]); P.bn_list.push_back(P.bn[i]);
        so += 2 * c;
    }
    build_conv(P, P.conv[0], en[0], enc[0], -1, false, true, false);
    for (int l = 1; l < 4; ++l) build_conv(P, P.conv[l], en[l], enc[l], l - 1, true, false, false);
    for (int l = 0; l < 3; ++l) build_conv(P, P.convT[l], dn[l], dec[l], 3 + l, true, false, false);
    build_conv(P, P.convT[3], dn[3], dec[3], -1, true, false, true);
    return so;
}
// classifier.0 consumes the NCHW flatten c*fs*fs + y*fs + x of the (fc, fs, fs) map held here as NHWC [fs][fs][fc]
inline void tower_build_fc1(TowerPlan& P) {
    const TowerGeom& G = P.geo;
    const int pix = G.fs * G.fs;
    LinL& f = P.fc1;
    f.w_off = off(P, "image_encoder.classifier.0.weight"); f.b_off = off(P, "image_encoder.classifier.0.bias");
    f.N = G.hid; f.K = G.feat; f.pk_dgrad = -1;
    PackDesc d = pack_dense(f.w_off, G.hid, G.feat, npad_for(G.hid), G.feat, G.feat, 0);
    d.TW = G.fs; d.C = G.fc; d.s_ty = G.fs; d.s_tx = 1; d.s_c = pix;
    f.pk_fwd = P.pk.add(d);
    PackDesc gd = d; gd.Npad = round_up(G.hid, 64);
    f.gk = P.gk.add(gd);
    // input gradient as ONE dense GEMM: da[n][s*fc+c] = sum_j dy[n][j] * W[j][c*pix+s]
    PackDesc t = pack_dense(f.w_off, G.feat, G.hid, npad_for(G.feat), G.hid, 0, G.feat);
    t.NL = G.fc; t.s_nhi = 1; t.s_nlo = pix;
    P.fc1_dgrad = P.pk.add(t);
}
// upsample Linear(D, FEAT): output columns permuted to NHWC n' = s*fc + c  <->  row c*pix + s; bias folded
inline void tower_build_up(TowerPlan& P) {
    const TowerGeom& G = P.geo;
    const int pix = G.fs * G.fs, D = P.D;
    LinL& f = P.up;
    f.w_off = off(P, "image_decoder.upsample.0.weight"); f.b_off = off(P, "image_decoder.upsample.0.bias");
    f.N = G.feat; f.K = D;
    PackDesc d = pack_dense(f.w_off, G.feat, D, npad_for(G.feat), round_up(P.ldz, 64), 0, 1);
    d.NL = G.fc; d.s_nhi = D; d.s_nlo = pix * D;
    d.bias_off = f.b_off; d.b_nhi = 1; d.b_nlo = pix;
    f.pk_fwd = P.pk.add(d);
    PackDesc gd = d; f.gk = P.gk.add(gd);
    PackDesc t = pack_dense(f.w_off, D, G.feat, npad_for(D), G.feat, 1, 0);
    t.TW = pix; t.C = G.fc; t.s_ty = 0; t.s_tx = D; t.s_c = pix * D;
    f.pk_dgrad = P.pk.add(t);
}

// ================================================================== launch arguments
// l: layer index (conv[l] / convT[l]); n: row blocks -- dropout variants of the classifier, BatchNorm groups (passes) of the decoder.
enum TowerGemm { TW_ENC_CONV1, TW_ENC_CONV, TW_ENC_CONV_DGRAD, TW_FC1, TW_FC1_DGRAD, TW_UP, TW_UP_DGRAD, TW_DEC_CONVT, TW_DEC_CONVT_DGRAD,
                 TW_DEC_LAST_DGRAD };
enum TowerWgrad { TW_W_ENC_CONV1, TW_W_ENC_CONV, TW_W_FC1, TW_W_UP, TW_W_DEC_CONVT, TW_W_DEC_LAST };

// mask: keep flags of the classifier Dropout behind classifier.0 (TW_FC1) or null; training: column statistics of the conv
// layers; aux: TW_UP_DGRAD the fp32 result dz [n*B][D]
inline GemmParams tower_gemm(TowerPlan& P, TowerGemm kind, int l, int n, int training = 1, const uint8_t* mask = nullptr, const void* aux = nullptr) {
    TowerW& w = *P.tw;
    const TowerGeom& G = P.geo;
    const TowerChains t = tower_chains(w);
    const int B = P.B, rows = n * B, rows1 = B * G.s1 * G.s1;
    switch (kind) {
    case TW_ENC_CONV1: {   // conv1 + Swish (no BatchNorm): raw and activated outputs
        GatherPlan pl = dense_plan(rows1, 48, 48, G.c1);
        GemmParams g = gemm_of(P, pl, P.conv[0].pk_fwd, 1, rows1);
        g.c.A = w.patches1; g.out_bf = w.r1; g.ldo = G.c1; g.out_act_bf = w.a1; g.e_act = ACT_SWISH;
        return g;
    }
    case TW_ENC_CONV: {
        const ConvL& L = P.conv[l];
        GemmParams g = gemm_of(P, L.fwd, L.pk_fwd, 1, B, L.pk_fwd_f);
        g.c.A = t.a[l - 1];
        g.out_bf = t.r[l]; g.ldo = L.g.Cout;
        g.colstats = training ? w.st_e[l - 1] : nullptr;
        return g;
    }
    case TW_ENC_CONV_DGRAD: {
        const ConvL& L = P.conv[l];
        GemmParams d = gemm_of(P, L.dgrad, L.pk_dgrad, 1, B, L.pk_dgrad_f);
        d.c.A = t.dr[l]; d.out_bf = t.dr[l - 1]; d.ldo = L.g.Cin;
        d.d_r = t.r[l - 1]; d.d_ld = L.g.Cin; d.d_act = ACT_SWISH;
        if (l > 1) { d.d_affine = w.aff_e[l - 2]; d.d_meanrstd = w.mr_e[l - 2]; d.d_red = w.red_e[l - 2]; }
        return d;
    }
    case TW_FC1: {   // classifier.0 over the NHWC feature map (shared by the variants) + Swish + Dropout
        GatherPlan pl = plan_fwdform(G.fs, G.fs, 1, 1, G.fc, G.fs, G.fs, 1, 0, G.hid, 1, rows);
        GemmParams g = gemm_of(P, pl, &P.fc1.pk_fwd, 1, rows);
        g.c.A = w.a4; g.c.a_bcast_n = B;
        g.bias = P.buf.params + P.fc1.b_off; g.out_bf = w.y1; g.ldo = G.hid;
        g.out_act_bf = w.ay1; g.e_act = ACT_SWISH; if (mask) { g.e_mask = mask; g.e_mask_scale = 1.f / (1.f - DROP_P); }
        return g;
    }
    case TW_FC1_DGRAD: {   // classifier.0: the input gradient is one dense GEMM over NHWC columns
        GatherPlan pd = dense_plan(rows, G.hid, G.hid, G.feat);
        GemmParams d = gemm_of(P, pd, &P.fc1_dgrad, 1, rows);
        d.c.A = w.dy1; d.out_bf = w.db4; d.ldo = G.feat;
        d.d_r = w.r4; d.d_ld = G.feat; d.d_bcast_n = B; d.d_act = ACT_SWISH; d.d_cmod = G.fc;
        d.d_affine = w.aff_e[2]; d.d_meanrstd = w.mr_e[2]; d.d_red = w.red_e[2];
        return d;
    }
    case TW_UP: {
        GatherPlan pl = dense_plan(rows, P.ldz, P.ldz, G.feat);
        GemmParams g = gemm_of(P, pl, &P.up.pk_fwd, 1, rows);
        g.c.A = w.z_bf; g.out_bf = w.u; g.ldo = G.feat; g.out_act_bf = w.au; g.e_act = ACT_SWISH;
        return g;
    }
    case TW_UP_DGRAD: {
        GatherPlan pd = dense_plan(rows, G.feat, G.feat, P.D);
        GemmParams d = gemm_of(P, pd, &P.up.pk_dgrad, 1, rows);
        d.c.A = w.du; d.out_f = (float*)aux; d.ldo = P.D;
        return d;
    }
    case TW_DEC_CONVT: {
        const ConvL& L = P.convT[l];
        GemmParams g = gemm_of(P, L.fwd, L.pk_fwd, n, B, L.pk_fwd_f);
        g.c.A = t.aq[l];
        g.out_bf = t.q[l + 1]; g.ldo = L.g.Cout;
        g.colstats = training ? w.st_d[l] : nullptr;
        return g;
    }
    case TW_DEC_CONVT_DGRAD: {
        const ConvL& L = P.convT[l];
        GemmParams d = gemm_of(P, L.dgrad, L.pk_dgrad, n, B, L.pk_dgrad_f);
        d.c.A = t.dq[l + 1]; d.out_bf = t.dq[l]; d.ldo = L.g.Cin;
        d.d_r = t.q[l]; d.d_ld = L.g.Cin; d.d_act = ACT_SWISH;
        if (l > 0) { d.d_affine = w.aff_d[l - 1]; d.d_meanrstd = w.mr_d[l - 1]; d.d_red = w.red_d[l - 1]; }
        return d;
    }
    case TW_DEC_LAST_DGRAD: {   // input gradient = dense GEMM patches x W with d-Swish + BatchNorm-backward sums in the epilogue
        GatherPlan pd = dense_plan(rows1, 48, 48, G.c1);
        GemmParams d = gemm_of(P, pd, P.convT[3].pk_dgrad, n, rows1);
        d.c.A = w.patches4; d.out_bf = w.d3; d.ldo = G.c1;
        d.d_r = w.q3; d.d_ld = G.c1; d.d_act = ACT_SWISH; d.d_affine = w.aff_d[2]; d.d_meanrstd = w.mr_d[2]; d.d_red = w.red_d[2];
        return d;
    }
    }
    return GemmParams{};
}

inline WgradParams tower_wgrad(TowerPlan& P, TowerWgrad kind, int l, int n) {
    TowerW& w = *P.tw;
    const TowerGeom& G = P.geo;
    const TowerChains t = tower_chains(w);
    const int B = P.B, rows = n * B, rows1 = B * G.s1 * G.s1;
    switch (kind) {
    case TW_W_ENC_CONV1: {   // conv1 wgrad over the im2col patches
        GatherPlan pl = dense_plan(rows1, 48, 48, G.c1);
        WgradParams g = wgrad_of(P, pl, P.conv[0].gk, 1, rows1);
        g.c.A = w.patches1; g.P = w.d1e; g.ldp = G.c1;
        return g;
    }
    case TW_W_ENC_CONV: {
        const ConvL& L = P.conv[l];
        WgradParams g = wgrad_of(P, L.fwd, L.gk, 1, B);
        g.c.A = t.a[l - 1]; g.P = t.dr[l]; g.ldp = L.g.Cout;
        return g;
    }
    case TW_W_FC1: {   // classifier.0: wgrad gathers the shared feature map
        GatherPlan pl = plan_fwdform(G.fs, G.fs, 1, 1, G.fc, G.fs, G.fs, 1, 0, G.hid, 1, rows);
        WgradParams g = wgrad_of(P, pl, &P.fc1.gk, 1, rows);
        g.c.A = w.a4; g.c.a_bcast_n = B;
        g.P = w.dy1; g.ldp = G.hid;
        return g;
    }
    case TW_W_UP: {   // upsample Linear: weight (+ folded bias) gradient
        GatherPlan pl = dense_plan(rows, P.ldz, P.ldz, G.feat);
        WgradParams g = wgrad_of(P, pl, &P.up.gk, 1, rows);
        g.c.A = w.z_bf; g.P = w.du; g.ldp = G.feat;
        return g;
    }
    case TW_W_DEC_CONVT:
        return convT_wgrad(P, P.convT[l], n, B, t.aq[l], t.dq[l + 1]);
    case TW_W_DEC_LAST: {   // last transposed conv (c1 -> 3) through the im2col patches of dlogit (K = 16 taps x 3)
        GatherPlan pl = plan_fwdform(1, 1, G.s1, G.s1, 48, 1, 1, 1, 0, G.c1, n, B);   // rows (n, iy, ix), dense K=48
        WgradParams g = wgrad_of(P, pl, P.convT[3].gk, n, B);
        g.c.A = w.patches4; g.c.AH = G.s1; g.c.AW = G.s1; g.c.sy = g.c.sx = 1;
        g.P = w.aq3; g.ldp = G.c1;
        return g;
    }
    }
    return WgradParams{};
}

// ---- the stand-alone passes
// image [B][3][img][img] -> patches1 [B*s1*s1][48];  dlogit [groups*B][3][img][img] -> patches4 [groups*B*s1*s1][48]: the same
// kernel with the same arguments except the row count
inline int im2col_image(TowerPlan& P, const float* image, hipStream_t s) {
    const TowerGeom& G = P.geo;
    return launch_im2col_small(image, P.B, 3, G.img, G.img, 4, 4, 2, 1, G.s1, G.s1, P.tw->patches1, 48, s);
}
inline int im2col_dlogit(TowerPlan& P, const float* dlogit, int groups, hipStream_t s) {
    const TowerGeom& G = P.geo;
    return launch_im2col_small(dlogit, groups * P.B, 3, G.img, G.img, 4, 4, 2, 1, G.s1, G.s1, P.tw->patches4, 48, s);
}
// BatchNorm + Swish behind conv[l] (l = 1..3) / convT[l] (l = 0..2): tables, running statistics, activated tensor
inline int enc_bn_act(TowerPlan& P, int l, int bn_updates, int training, hipStream_t s) {
    TowerW& w = *P.tw;
    const TowerChains t = tower_chains(w);
    const ConvL& L = P.conv[l];
    const int rows = P.B * L.g.OH * L.g.OW;
    return bn_act(P, P.bn[L.bn], t.r[l], t.a[l], rows, rows, 1, w.st_e[l - 1], bn_updates, w.aff_e[l - 1], w.mr_e[l - 1], training, s);
}
inline int dec_bn_act(TowerPlan& P, int l, int groups, int training, hipStream_t s) {
    TowerW& w = *P.tw;
    const TowerChains t = tower_chains(w);
    const ConvL& L = P.convT[l];
    const int rpg = P.B * L.g.OH * L.g.OW;
    return bn_act(P, P.bn[L.bn], t.q[l + 1], t.aq[l + 1], groups * rpg, rpg, groups, w.st_d[l], 1, w.aff_d[l], w.mr_d[l], training, s);
}
// BatchNorm backward behind conv[l] / convT[l]; features.9 (l = 3) sums the gradients of the 2 classifier variants (db2)
inline BnBwdApplyArgs enc_bn_bwd_args(TowerPlan& P, int l, int variants) {
    TowerW& w = *P.tw;
    const TowerChains t = tower_chains(w);
    const int B = P.B;
    const ConvL& L = P.conv[l];
    const BnL& b = P.bn[L.bn];
    const int pix = L.g.OH * L.g.OW;
    BnBwdApplyArgs x{};
    x.db = (l == 3) ? w.db4 : t.dr[l];
    x.db2 = (l == 3 && variants == 2) ? w.db4 + (size_t)B * P.geo.feat : nullptr;
    x.r = t.r[l]; x.dr = t.dr[l]; x.rows = B * pix; x.C = L.g.Cout; x.ld = L.g.Cout; x.rows_per_group = B * pix; x.G = 1;
    x.red = w.red_e[l - 1]; x.meanrstd = w.mr_e[l - 1]; x.gamma = P.buf.params + b.w_off;
    x.dgamma = P.buf.grads + b.w_off; x.dbeta = P.buf.grads + b.b_off;
    return x;
}
inline BnBwdApplyArgs dec_bn_bwd_args(TowerPlan& P, int l, int groups) {
    TowerW& w = *P.tw;
    const TowerChains t = tower_chains(w);
    const int B = P.B, rows = groups * B;
    const ConvL& L = P.convT[l];
    const BnL& b = P.bn[L.bn];
    const int pix = L.g.OH * L.g.OW;
    BnBwdApplyArgs x{};
    x.db = t.dq[l + 1]; x.r = t.q[l + 1]; x.dr = t.dq[l + 1]; x.rows = rows * pix; x.C = L.g.Cout; x.ld = L.g.Cout;
    x.rows_per_group = B * pix; x.G = groups;
    x.red = w.red_d[l]; x.meanrstd = w.mr_d[l]; x.gamma = P.buf.params + b.w_off;
    x.dgamma = P.buf.grads + b.w_off; x.dbeta = P.buf.grads + b.b_off;
    return x;
}
// last transposed conv (c1 -> 3) + sigmoid + BCE: `last` carries the caller's target / outputs / loss weights
inline ConvTLastFwdArgs dec_last_args(TowerPlan& P, const ConvTLastFwdArgs& last, int groups) {
    const TowerGeom& G = P.geo;
    ConvTLastFwdArgs x = last;
    x.act = P.tw->aq3; x.w = P.buf.params + P.convT[3].w_off; x.G = groups; x.B = P.B; x.IH = G.s1; x.IW = G.s1; x.Cin = G.c1; x.Cout = 3;
    return x;
}

// Staging transforms of the fused step (gemm.h GatherTransform; B % 4 == 0, image-resident kernels only): `tr` is read by the
// launcher and must outlive the launch.
// kind 1: forward layer l stages Swish(BatchNorm(raw output of the layer below)) itself, writes that layer's tables, updates its
// running statistics and leaves the activated tensor behind for the weight gradient
inline void stage_fwd_enc(TowerPlan& P, int l, GemmParams& g, GatherTransform& tr, int bn_updates, int training) {
    TowerW& w = *P.tw;
    const TowerChains t = tower_chains(w);
    const ConvL& Lp = P.conv[l - 1];
    tr.kind = 1;
    tr.fin = bn_fin_args(P, P.bn[Lp.bn], P.B * Lp.g.OH * Lp.g.OW, 1, w.st_e[l - 2], bn_updates, w.aff_e[l - 2], w.mr_e[l - 2], training);
    tr.out = t.a[l - 1];
    g.c.A = t.r[l - 1]; g.tr = &tr;
}
inline void stage_fwd_dec(TowerPlan& P, int l, int groups, GemmParams& g, GatherTransform& tr, int training) {
    TowerW& w = *P.tw;
    const TowerChains t = tower_chains(w);
    const ConvL& Lp = P.convT[l - 1];
    tr.kind = 1;
    tr.fin = bn_fin_args(P, P.bn[Lp.bn], P.B * Lp.g.OH * Lp.g.OW, groups, w.st_d[l - 1], 1, w.aff_d[l - 1], w.mr_d[l - 1], training);
    tr.out = t.aq[l];
    g.c.A = t.q[l]; g.tr = &tr;
}
// kind 2: the data gradient of layer l applies the BatchNorm backward of the layer's own BatchNorm to db while staging it and
// writes dr back IN PLACE (a workgroup owns its images: each vector is read, then overwritten, by the same thread)
inline void stage_bwd_enc(TowerPlan& P, int l, GemmParams& d, GatherTransform& tr) {
    TowerW& w = *P.tw;
    const TowerChains t = tower_chains(w);
    const ConvL& L = P.conv[l];
    const BnL& b = P.bn[L.bn];
    tr.kind = 2; tr.r = t.r[l]; tr.red = w.red_e[l - 1]; tr.mr = w.mr_e[l - 1]; tr.gamma = P.buf.params + b.w_off;
    tr.dgamma = P.buf.grads + b.w_off; tr.dbeta = P.buf.grads + b.b_off;
    tr.inv_cnt = 1.f / (float)(P.B * L.g.OH * L.g.OW); tr.groups = 1; tr.out = t.dr[l];
    d.tr = &tr;
}
inline void stage_bwd_dec(TowerPlan& P, int l, int groups, GemmParams& d, GatherTransform& tr) {
    TowerW& w = *P.tw;
    const TowerChains t = tower_chains(w);
    const ConvL& L = P.convT[l];
    const BnL& b = P.bn[L.bn];
    tr.kind = 2; tr.r = t.q[l + 1]; tr.red = w.red_d[l]; tr.mr = w.mr_d[l]; tr.gamma = P.buf.params + b.w_off;
    tr.dgamma = P.buf.grads + b.w_off; tr.dbeta = P.buf.grads + b.b_off;
    tr.inv_cnt = 1.f / (float)(P.B * L.g.OH * L.g.OW); tr.groups = groups; tr.out = t.dq[l + 1];
    d.tr = &tr;
}

// ================================================================== the conv chains of the step
// fuse (CelebA's fused step, B % 4 == 0): the layers that run on the image-resident kernels (convres.hip) stage BatchNorm + Swish /
// the BatchNorm backward of their gathered operand themselves (GatherTransform) and leave the staged tensor behind for the
// weight gradients (GatherTransform::out) -- no bn_act / bn_bwd_apply launch in front of them.  The staged layers (features.5,
// hallucinate.3 / .6 forward; features.5 / .2, hallucinate.6 / .3 backward) are CelebA's: COCO passes fuse = false.

// image -> a4 (the activated feature map); the family's classifier follows
inline int tower_enc_fwd(TowerPlan& P, const float* image, int training, int bn_updates, hipStream_t s, bool fuse = false) {
    MMVAE_TRY(im2col_image(P, image, s));
    MMVAE_TRY(launch_gemm_gather(tower_gemm(P, TW_ENC_CONV1, 0, 1), s));
    for (int l = 1; l < 4; ++l) {
        GemmParams g = tower_gemm(P, TW_ENC_CONV, l, 1, training);
        GatherTransform tr{};
        if (fuse && l == 2) stage_fwd_enc(P, l, g, tr, bn_updates, training);     // features.5 stages a2 = Swish(BatchNorm(r2)) itself
        MMVAE_TRY(launch_gemm_gather(g, s));
        if (fuse && l == 1) continue;
        MMVAE_TRY(enc_bn_act(P, l, bn_updates, training, s));
    }
    return MMVAE_OK;
}
// db4 (the gradient of classifier.0's input, one block per variant) -> every conv gradient of the encoder
inline int tower_enc_bwd(TowerPlan& P, int variants, hipStream_t s, bool fuse = false) {
    for (int l = 3; l >= 1; --l) {
        const bool fl = fuse && l <= 2;       // BatchNorm backward inside the data gradient's staging, dr in place; the weight gradient follows it
        if (!fl) MMVAE_TRY(launch_bn_bwd_apply(enc_bn_bwd_args(P, l, variants), s));
        WgradParams gw = tower_wgrad(P, TW_W_ENC_CONV, l, 1);
        if (!fl) MMVAE_TRY(wgrad_async(P, gw, s));
        {
            GemmParams d = tower_gemm(P, TW_ENC_CONV_DGRAD, l, 1);
            GatherTransform tr{};
            if (fl) stage_bwd_enc(P, l, d, tr);
            MMVAE_TRY(launch_gemm_gather(d, s));
        }
        if (fl) MMVAE_TRY(wgrad_async(P, gw, s));
    }
    return wgrad_async(P, tower_wgrad(P, TW_W_ENC_CONV1, 0, 1), s);
}
// z_bf -> q3 (raw output of hallucinate.6); bn_last: its stand-alone BatchNorm + Swish pass into aq3 as well (not when the caller's
// own tail normalises q3 itself: CelebA's fused tail, the scoring tails of <family>_iw_score)
inline int tower_dec_fwd(TowerPlan& P, int groups, int training, bool bn_last, hipStream_t s, bool fuse = false) {
    MMVAE_TRY(launch_gemm_gather(tower_gemm(P, TW_UP, 0, groups), s));
    for (int l = 0; l < 3; ++l) {
        GemmParams g = tower_gemm(P, TW_DEC_CONVT, l, groups, training);
        GatherTransform tr{};
        if (fuse && l >= 1) stage_fwd_dec(P, l, groups, g, tr, training);     // hallucinate.3 / .6 stage Swish(BatchNorm(q[l])) themselves and leave aq[l] behind
        MMVAE_TRY(launch_gemm_gather(g, s));
        if (l == 2 && !bn_last) continue;
        if (fuse && l <= 1) continue;
        MMVAE_TRY(dec_bn_act(P, l, groups, training, s));
    }
    return MMVAE_OK;
}
// dlogit: fp32 NCHW [groups*B][3][img][img] (grad wrt the pre-sigmoid logits). Writes dz (fp32 [groups*B][D]).
// last_fused: d3, the BatchNorm-backward sums and the weight gradient of the last layer came out of the caller's fused tail
inline int tower_dec_bwd(TowerPlan& P, const float* dlogit, int groups, float* dz, hipStream_t s, bool last_fused = false, bool fuse = false) {
    if (!last_fused) {   // last transposed conv (c1 -> 3): both gradients go through the im2col patches of dlogit (K = 16 taps x 3)
        MMVAE_TRY(im2col_dlogit(P, dlogit, groups, s));
        MMVAE_TRY(launch_gemm_gather(tower_gemm(P, TW_DEC_LAST_DGRAD, 3, groups), s));
        MMVAE_TRY(wgrad_async(P, tower_wgrad(P, TW_W_DEC_LAST, 3, groups), s));
    }
    for (int l = 2; l >= 0; --l) {
        const bool fl = fuse && l >= 1;       // hallucinate.6 / .3: as in tower_enc_bwd
        if (!fl) MMVAE_TRY(launch_bn_bwd_apply(dec_bn_bwd_args(P, l, groups), s));
        WgradParams gw = tower_wgrad(P, TW_W_DEC_CONVT, l, groups);
        if (!fl) MMVAE_TRY(wgrad_async(P, gw, s));
        {
            GemmParams d = tower_gemm(P, TW_DEC_CONVT_DGRAD, l, groups);
            GatherTransform tr{};
            if (fl) stage_bwd_dec(P, l, groups, d, tr);
            MMVAE_TRY(launch_gemm_gather(d, s));
        }
        if (fl) MMVAE_TRY(wgrad_async(P, gw, s));
    }
    // upsample Linear: weight (+ folded bias) gradient and dz
    MMVAE_TRY(wgrad_async(P, tower_wgrad(P, TW_W_UP, 0, groups), s));
    return launch_gemm_gather(tower_gemm(P, TW_UP_DGRAD, 0, groups, 1, nullptr, dz), s);
}

// ================================================================== importance-weighted evaluation
// particles z [rows][D] -> z_bf; the decoder body runs the plan's rows: the ones past `rows` are defined (zero) and never scored
inline int tower_iw_particles(TowerPlan& P, const float* z, int rows, hipStream_t s) {
    bf16* z_bf = P.tw->z_bf;
    hipLaunchKernelGGL(cast_z_kernel, dim3(ceil_div(rows * P.ldz, 256)), dim3(256), 0, s, z, rows, P.D, z_bf, P.ldz);
    MMVAE_TRY(mmvae_check_launch("cast_z"));
    if (rows < P.B) MMVAE_TRY(launch_fill_zero(z_bf + (size_t)rows * P.ldz, (size_t)(P.B - rows) * P.ldz * sizeof(bf16), s));
    return MMVAE_OK;
}
// the scoring tail behind tower_dec_fwd(P, 1, 0, false, s): BatchNorm of hallucinate.7 from its running statistics
inline IwTailArgs tower_iw_tail_args(TowerPlan& P, const float* image, int rows, int K, float* loglik) {
    const BnL& b = P.bn[P.convT[2].bn];
    IwTailArgs t{};
    t.q3 = P.tw->q3; t.gamma = P.buf.params + b.w_off; t.beta = P.buf.params + b.b_off;
    t.rmean = P.buf.bn_stats + b.stat_off; t.rvar = t.rmean + b.C; t.eps = BN_EPS;
    t.act = ACT_SWISH; t.w = P.buf.params + P.convT[3].w_off; t.image = image; t.rows = rows; t.K = K; t.loglik = loglik;
    return t;
}

// ================================================================== the one-pass step of the image-only VAE
// celeba/train_imageonly.py:95-113, coco/train_imageonly.py: zero_grad, ONE forward of B rows (encoder with one dropout variant and
// one BatchNorm update, latent1 -- no product of experts --, decoder with one BatchNorm group, sigmoid + BCE) and its backward.  The
// workspace is the family's one-pass carve (the module entry points' one); the launches are the ones the module entry points run
// (the staged forms and CelebA's fused decoder tail are built for 3 groups / 2 variants and stay with the 3-pass step).  Weight
// gradients go to the two side streams as in the 3-pass step; nothing else leaves the main stream: there is no second modality.
// Fam (the family's classifier tail around the tower):
//   mask_width[2]                   widths of the classifier's Dropout layers (0: the family has no second one)
//   last_bias(P)                    offset of the bias of the classifier's last Linear in the flat buffers
//   enc_fwd(P, image, m1, m2, drop, training, out, s) / enc_bwd(P, d_out, m1, m2, drop, s)      one variant
//
// `lt` (optional): an extra loss term in the latent sample beside the reconstruction and the KL term -- the InfoVAE step's
// lambda * MMD(prior samples, z), coco/train_infovae.py:44-55.  It needs z, which is ready right behind the latent block, and its
// gradient is needed only by the latent block's backward; the decoder's forward and backward run in between.  So the sweep and its
// fold (mmd.h launch_mmd_dy: gradient for z alone) go to the plan's first side stream, which this step leaves idle (there is no second
// modality), and the main stream waits for them once, in front of the latent block's backward, which adds lt->dz to the decoder's dz
// (Latent1BwdArgs::dz2).  MMVAE_SERIAL: in order on the caller's stream.  Without `lt` the step launches what it always launched.
struct TowerLatentTerm {
    const float* samples;    // [B][D] prior samples, or null: drawn into `drawn` by the step's prologue on Philox stream `philox_stream`
    float* drawn;            // [B][D]
    unsigned philox_stream;
    float lambda;            // weight of the term (0: the value is still reported, no gradient)
    void* ws;                // mmd_dy_workspace_bytes(B, B, D) bytes, 8-byte aligned
    float* dz;               // [B][D]: lambda * dMMD/dz
    float* z_out;            // [B][D] or null: where z goes instead of the workspace
    int slot;                // first of the 4 loss slots {mean Kxx, mean Kyy, mean Kxy, MMD} (row 0 of the slot table, zero elsewhere)
};
template <class Plan, class Fam>
int tower_image_step(Plan& P, const mmvae_image_step_io& io, int training, int do_backward, hipStream_t s, const Fam& fam,
                     const TowerLatentTerm* lt = nullptr) {
    typename Plan::W& w = P.w;
    const TowerGeom& G = P.geo;
    const int B = P.B, D = P.D, npix = 3 * G.img * G.img;
    MMVAE_REQUIRE(io.image && io.sums, "image step: image/sums must be given");
    MMVAE_REQUIRE(launch_latent1_scratch_floats(B, D) <= (size_t)B * npix, "image step: no room for the latent block's partial sums");
    const float* eps = io.eps;
    const uint8_t *m1 = io.enc_mask1, *m2 = io.enc_mask2;
    StepBeginArgs sb{};
    sb.zero_ptr[0] = w.zero_begin; sb.zero_bytes[0] = w.zero_bytes;
    if (do_backward) {
        sb.zero_ptr[1] = P.buf.gpk; sb.zero_bytes[1] = (size_t)P.gk.mat_elems * sizeof(float);
        sb.zero_ptr[2] = P.buf.grads; sb.zero_bytes[2] = (size_t)(P.nparams / 4) * 16;
    }
    sb.p = DROP_P; sb.seed = io.seed; sb.step = io.step_counter;
    const int enc_drop = training && io.enc_dropout;
    if (training && !eps) { sb.eps = w.eps; sb.n_eps = (long long)B * D; eps = w.eps; }
    if (enc_drop && !m1) { sb.mask[0] = w.m1; sb.n_mask[0] = (long long)B * fam.mask_width[0]; m1 = w.m1; }
    if (enc_drop && fam.mask_width[1] && !m2) { sb.mask[1] = fam.m2(P); sb.n_mask[1] = (long long)B * fam.mask_width[1]; m2 = fam.m2(P); }
    const float* prior = nullptr;
    if (lt) {
        MMVAE_REQUIRE(B <= MMD_MAX_N && lt->ws && lt->dz && lt->drawn, "image step: the latent term needs its workspace and a batch of at most %d", (int)MMD_MAX_N);
        prior = lt->samples;
        if (!prior) { sb.normal2 = lt->drawn; sb.n_normal2 = (long long)B * D; sb.normal2_stream = lt->philox_stream; prior = lt->drawn; }
    }
    MMVAE_TRY(launch_step_begin(sb, s));
    if (do_backward && P.nparams % 4 != 0)
        MMVAE_TRY(launch_fill_zero(P.buf.grads + (P.nparams / 4) * 4, (size_t)(P.nparams % 4) * sizeof(float), s));
    MMVAE_TRY(ensure_streams(P));
    MMVAE_TRY(fam.enc_fwd(P, io.image, m1, m2, enc_drop, training, w.encout, s));
    Latent1Args la{};
    la.B = B; la.D = D; la.enc_out = w.encout; la.eps = eps;
    la.mu = io.mu ? io.mu : w.mu; la.logvar = io.logvar ? io.logvar : w.logvar;
    la.z_f32 = (lt && lt->z_out) ? lt->z_out : w.z_f32; la.z_bf = w.z_bf; la.ldz = P.ldz; la.kl_sum = w.sums + 8; la.training = training;
    la.scratch = w.tmp_f32;         // (the module decoder's sigmoid-backward buffer: nobody else's in this step)
    MMVAE_TRY(launch_latent1_fwd(la, s));
    hipStream_t Sm = s;             // where the latent term runs
    const bool lt_grad = lt && do_backward && lt->lambda != 0.f;        // (a zero weight has exactly no gradient)
    if (lt) {
        if (!mmvae_serial()) { Sm = P.st_text; MMVAE_TRY(edge(P, s, Sm)); }
        MMVAE_TRY(launch_mmd_dy(prior, B, la.z_f32, B, D, lt->ws, lt->lambda, w.sums + lt->slot, lt_grad ? lt->dz : nullptr, Sm));
    }
    ConvTLastFwdArgs last{};
    last.target = io.image; last.recon = io.recon_image; last.dlogit = do_backward ? w.dlogit : nullptr; last.loss_sum = w.sums;
    last.coef[0] = io.lambda_x / (float)(B * npix);
    MMVAE_TRY(tower_dec_fwd(P, 1, training, true, s));
    MMVAE_TRY(launch_convt_last_fwd(dec_last_args(P, last, 1), s));
    if (!do_backward) {
        if (Sm != s) MMVAE_TRY(edge(P, Sm, s));
        hipLaunchKernelGGL(sum_slots_kernel, dim3(1), dim3(64), 0, s, w.sums, io.sums);
        return mmvae_check_launch("sum_slots");
    }
    // =============================== backward ===============================
    P.wgrad_forked = true;
    int rc = MMVAE_OK;
    const bool img_term = io.lambda_x != 0.f;        // (a zero weight has exactly no gradient)
    if (img_term) rc = tower_dec_bwd(P, w.dlogit, 1, w.dz_img, s);
    if (rc == MMVAE_OK && Sm != s) rc = edge(P, Sm, s);      // the latent term's value and gradient
    Latent1BwdArgs lb{};
    lb.f = la; lb.dz = img_term ? w.dz_img : nullptr; lb.dz2 = lt_grad ? lt->dz : nullptr; lb.kl_coef = io.kl_lambda / (float)B;
    lb.d_enc_out = w.d_encout; lb.ld = 2 * D; lb.d_bias = P.buf.grads + fam.last_bias(P);
    lb.loss_slots = w.sums; lb.loss_out = io.sums;      // (BCE and KL sums are final here)
    if (rc == MMVAE_OK) rc = launch_latent1_bwd(lb, s);
    if (rc == MMVAE_OK) rc = fam.enc_bwd(P, w.d_encout, m1, m2, enc_drop, s);
    P.wgrad_forked = false;
    MMVAE_TRY(rc);
    MMVAE_TRY(join_sides(P, s, s));
    if (io.defer_unpack) return launch_wgrad_reduce(&P.slab, s);      // the packed gradients are complete; Adam gathers them
    return plan_unpack(P, s, true);
}

// ================================================================== test / profiling aids (<family>_bench_layer, <family>_debug_offset)
// The launches of tower_gemm / tower_wgrad under names: <layer>, <layer>_dgrad, <layer>_wgrad.  The classifier runs its 2 dropout
// variants, the decoder 3 passes forward and 3 backward (the default step).  m1: keep flags that take part in fc1, or null; dz:
// where up_dgrad writes.  staged (CelebA): also <layer>_staged / <layer>_dgrad_staged, the forms its default step runs at
// B % 4 == 0 (stage_fwd_* / stage_bwd_*; `tr` is theirs), with the running-statistics updates of the default step (2 encoder
// variants, 1 per decoder pass)
inline bool tower_named_gemm(TowerPlan& P, const std::string& name, const uint8_t* m1, float* dz, bool staged, GemmParams& g, GatherTransform& tr) {
    if (name == "enc_conv1") { g = tower_gemm(P, TW_ENC_CONV1, 0, 1); return true; }
    for (int l = 1; l < 4; ++l) {
        const std::string n = "enc_conv" + std::to_string(l + 1);
        if (name == n) { g = tower_gemm(P, TW_ENC_CONV, l, 1); return true; }
        if (name == n + "_dgrad") { g = tower_gemm(P, TW_ENC_CONV_DGRAD, l, 1); return true; }
    }
    if (name == "fc1") { g = tower_gemm(P, TW_FC1, 0, 2, 1, m1); return true; }
    if (name == "fc1_dgrad") { g = tower_gemm(P, TW_FC1_DGRAD, 0, 2); return true; }
    if (name == "up") { g = tower_gemm(P, TW_UP, 0, 3); return true; }
    if (name == "up_dgrad") { g = tower_gemm(P, TW_UP_DGRAD, 0, 3, 1, nullptr, dz); return true; }
    for (int l = 0; l < 3; ++l) {
        const std::string n = "dec_convT" + std::to_string(l + 1);
        if (name == n) { g = tower_gemm(P, TW_DEC_CONVT, l, 3); return true; }
        if (name == n + "_dgrad") { g = tower_gemm(P, TW_DEC_CONVT_DGRAD, l, 3); return true; }
    }
    if (name == "dec_last_dgrad_gemm") { g = tower_gemm(P, TW_DEC_LAST_DGRAD, 3, 3); return true; }
    if (!staged) return false;
    if (name == "enc_conv3_staged") { g = tower_gemm(P, TW_ENC_CONV, 2, 1); stage_fwd_enc(P, 2, g, tr, 2, 1); return true; }
    for (int l = 1; l < 3; ++l) {
        const std::string e = "enc_conv" + std::to_string(l + 1), d = "dec_convT" + std::to_string(l + 1);
        if (name == d + "_staged") { g = tower_gemm(P, TW_DEC_CONVT, l, 3); stage_fwd_dec(P, l, 3, g, tr, 1); return true; }
        if (name == e + "_dgrad_staged") { g = tower_gemm(P, TW_ENC_CONV_DGRAD, l, 1); stage_bwd_enc(P, l, g, tr); return true; }
        if (name == d + "_dgrad_staged") { g = tower_gemm(P, TW_DEC_CONVT_DGRAD, l, 3); stage_bwd_dec(P, l, 3, g, tr); return true; }
    }
    return false;
}
inline bool tower_named_wgrad(TowerPlan& P, const std::string& name, WgradParams& g) {
    if (name == "enc_conv1_wgrad") { g = tower_wgrad(P, TW_W_ENC_CONV1, 0, 1); return true; }
    for (int l = 1; l < 4; ++l)
        if (name == "enc_conv" + std::to_string(l + 1) + "_wgrad") { g = tower_wgrad(P, TW_W_ENC_CONV, l, 1); return true; }
    if (name == "fc1_wgrad") { g = tower_wgrad(P, TW_W_FC1, 0, 2); return true; }
    if (name == "up_wgrad") { g = tower_wgrad(P, TW_W_UP, 0, 3); return true; }
    for (int l = 0; l < 3; ++l)
        if (name == "dec_convT" + std::to_string(l + 1) + "_wgrad") { g = tower_wgrad(P, TW_W_DEC_CONVT, l, 3); return true; }
    if (name == "dec_last_wgrad") { g = tower_wgrad(P, TW_W_DEC_LAST, 3, 3); return true; }
    return false;
}
// a weight gradient + its share of the slab reduction, as in the step
inline int tower_replay_wgrad(TowerPlan& P, const WgradParams& wg, int iters, hipStream_t s) {
    for (int i = 0; i < iters; ++i) {
        P.slab.reset(P.tw->slab, P.tw->slab_floats);
        MMVAE_TRY(launch_wgrad(wg, s, &P.slab));
        MMVAE_TRY(launch_wgrad_reduce(&P.slab, s));
    }
    return MMVAE_OK;
}
// names of the tower's workspace buffers; the family adds its own and looks one up with tower_offset_of (-1 if unknown)
inline std::map<std::string, const void*> tower_debug_names(const TowerW& w) {
    std::map<std::string, const void*> m = {
        {"patches1", w.patches1}, {"r1", w.r1}, {"r2", w.r2}, {"r3", w.r3}, {"r4", w.r4},
        {"a1", w.a1}, {"a2", w.a2}, {"a3", w.a3}, {"a4", w.a4}, {"y1", w.y1}, {"ay1", w.ay1},
        {"z_bf", w.z_bf}, {"u", w.u}, {"au", w.au}, {"q1", w.q1}, {"q2", w.q2}, {"q3", w.q3},
        {"aq1", w.aq1}, {"aq2", w.aq2}, {"aq3", w.aq3}, {"dlogit", w.dlogit}, {"patches4", w.patches4},
        {"d3", w.d3}, {"d2", w.d2}, {"d1", w.d1}, {"du", w.du},
        {"dy1", w.dy1}, {"db4", w.db4}, {"dr4", w.dr4}, {"d3e", w.d3e}, {"d2e", w.d2e}, {"d1e", w.d1e}, {"slab", w.slab},
    };
    for (int i = 0; i < 3; ++i) {
        const std::string k = std::to_string(i);
        m["st_e" + k] = w.st_e[i]; m["st_d" + k] = w.st_d[i]; m["red_e" + k] = w.red_e[i]; m["red_d" + k] = w.red_d[i];
        m["aff_e" + k] = w.aff_e[i]; m["aff_d" + k] = w.aff_d[i]; m["mr_e" + k] = w.mr_e[i]; m["mr_d" + k] = w.mr_d[i];
    }
    return m;
}
inline long long tower_offset_of(const std::map<std::string, const void*>& m, const char* name, const void* base) {
    auto it = m.find(name);
    if (it == m.end()) return -1;
    return (long long)((const char*)it->second - (const char*)base);
}
