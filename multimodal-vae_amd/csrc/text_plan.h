// Host side of the MultiMNIST text path shared by the plans that run it: the MMVAE (multimnist.hip, hidden size 100, parameters
// text_encoder.* / text_decoder.*) and the text-only baseline (mmtext.hip, hidden size 50 or 100, parameters encoder.* / decoder.*).
// Parameter table, weight-pack descriptors (gate-major, transposed copies for the backward, weight-gradient targets), workspace
// carving and the argument structs / grouped weight-gradient launches of text.hip, all sized from the plan's hidden size.
//
// A plan that uses these templates has the members
//   int D, B, H, kx, kz;  const char *te_name, *td_name;      (parameter prefixes without the trailing dot)
//   TextGruIdx te_f, te_r, td0, td1;  int te_h2p, te_h2pT, g_te_h2p, td_z2h, td_z2hT, g_td_z2h, td_h2o, td_h2oT, g_td_h2o;
// and a workspace struct `w` with the pointers the carve_text_* functions fill.
// Include only from .hip translation units, behind plan_base.h.
#pragma once
#include "plan_base.h"
#include "text.h"

struct TextGruIdx { int wih, whh, wihT, whhT, g_wih, g_whh; long long bih, bhh; };

// ---- parameters, in state_dict order (multimnist/model.py:219-307)
template <class Plan>
void text_add_encoder_params(Plan& P) {
    const int D = P.D, H = P.H;
    const std::string n = P.te_name;
    auto gru = [&](const char* sfx) {
        add_param(P, n + ".gru.weight_ih_" + sfx, {3 * H, H}); add_param(P, n + ".gru.weight_hh_" + sfx, {3 * H, H});
        add_param(P, n + ".gru.bias_ih_" + sfx, {3 * H}); add_param(P, n + ".gru.bias_hh_" + sfx, {3 * H});
    };
    add_param(P, n + ".embed.weight", {TXT_V, H});
    gru("l0"); gru("l0_reverse");
    add_param(P, n + ".h2p.weight", {2 * D, H}); add_param(P, n + ".h2p.bias", {2 * D});
}
template <class Plan>
void text_add_decoder_params(Plan& P) {
    const int D = P.D, H = P.H;
    const std::string n = P.td_name;
    auto gru = [&](int inp, const char* sfx) {
        add_param(P, n + ".gru.weight_ih_" + sfx, {3 * H, inp}); add_param(P, n + ".gru.weight_hh_" + sfx, {3 * H, H});
        add_param(P, n + ".gru.bias_ih_" + sfx, {3 * H}); add_param(P, n + ".gru.bias_hh_" + sfx, {3 * H});
    };
    add_param(P, n + ".embed.weight", {TXT_V, H});
    add_param(P, n + ".z2h.weight", {H, D}); add_param(P, n + ".z2h.bias", {H});
    gru(H + D, "l0"); gru(H, "l1");
    add_param(P, n + ".h2o.weight", {TXT_V, H + D}); add_param(P, n + ".h2o.bias", {TXT_V});
}

// ---- packs of the row-tile kernels: [round16(N)][round32(K)] bf16 fragment-major, plus transposed copies for the backward
template <class Plan>
void text_build_packs(Plan& P) {
    const int D = P.D, H = P.H, HP = txt_hp(H), G3 = 3 * H;
    P.kz = round_up(D, 32); P.kx = txt_kx(H, D);
    auto rt = [&](long long w, int N, int K, bool transpose) {       // fragment-major: text.hip rowtile_gemm
        PackDesc d = transpose ? pack_dense(w, K, N, round_up(K, 16), round_up(N, 32), 1, K) : pack_dense(w, N, K, round_up(N, 16), round_up(K, 32), K, 1);
        d.frag = 1;
        return P.pk.add(d);
    };
    auto gw = [&](long long w, int N, int K, int Kc) {   // wgrad target: [round64(N)][round64(Kc)] with K valid columns
        return P.gk.add(pack_dense(w, N, K, round_up(N, 64), round_up(Kc, 64), K, 1));
    };
    auto grui = [&](TextGruIdx& g, const std::string& n, const char* sfx, int inp, int inp_k, bool need_hh) {
        const long long wih = off(P, n + ".weight_ih_" + sfx), whh = off(P, n + ".weight_hh_" + sfx);
        g.bih = off(P, n + ".bias_ih_" + sfx); g.bhh = off(P, n + ".bias_hh_" + sfx);
        g.wih = rt(wih, G3, inp, false); g.wihT = rt(wih, G3, inp, true);
        g.whh = rt(whh, G3, H, false); g.whhT = rt(whh, G3, H, true);
        g.g_wih = gw(wih, G3, inp, inp_k);
        g.g_whh = need_hh ? gw(whh, G3, H, HP) : -1;
    };
    const std::string te = P.te_name, td = P.td_name;
    grui(P.te_f, te + ".gru", "l0", H, HP, true);
    grui(P.te_r, te + ".gru", "l0_reverse", H, HP, false);       // (one step from h = 0: W_hh of the reverse direction has no gradient)
    {
        const long long w = off(P, te + ".h2p.weight");
        P.te_h2p = rt(w, 2 * D, H, false); P.te_h2pT = rt(w, 2 * D, H, true); P.g_te_h2p = gw(w, 2 * D, H, HP);
    }
    {
        const long long w = off(P, td + ".z2h.weight");
        P.td_z2h = rt(w, H, D, false); P.td_z2hT = rt(w, H, D, true); P.g_td_z2h = gw(w, H, D, P.kz);
    }
    grui(P.td0, td + ".gru", "l0", H + D, P.kx, true);
    grui(P.td1, td + ".gru", "l1", H, HP, true);
    {
        const long long w = off(P, td + ".h2o.weight");
        P.td_h2o = rt(w, TXT_V, H + D, false); P.td_h2oT = rt(w, TXT_V, H + D, true); P.g_td_h2o = gw(w, TXT_V, H + D, P.kx);
    }
}

// ---- workspace (B: encoder rows, R: decoder rows)
template <class W>
void carve_text_enc(W& w, Workspace& ws, size_t B, size_t D, int H) {
    const size_t HP = txt_hp(H);
    w.txtout = ws.take<float>(B * 2 * D);
    w.te_gates_f = ws.take<float>(4 * 5 * B * H); w.te_gates_r = ws.take<float>(5 * B * H);
    w.te_x = ws.take<bf16>(4 * B * HP); w.te_hprev = ws.take<bf16>(4 * B * HP); w.te_hsum = ws.take<bf16>(B * HP);
}
template <class W>
void carve_text_dec(W& w, Workspace& ws, size_t R, int H, int kx, int kz) {
    const size_t HP = txt_hp(H), GL = txt_gl(H);
    w.words = ws.take<float>(R * TXT_T * TXT_V); w.dwords = ws.take<float>(R * TXT_T * TXT_V); w.tokens = ws.take<long long>(R * TXT_T);
    w.td_gates = ws.take<float>(4 * 2 * 5 * R * H);
    w.td_x0 = ws.take<bf16>(4 * R * kx); w.td_hz = ws.take<bf16>(4 * R * kx);
    w.td_h0p = ws.take<bf16>(4 * R * HP); w.td_mid = ws.take<bf16>(4 * R * HP); w.td_h1p = ws.take<bf16>(4 * R * HP);
    w.td_zbf = ws.take<bf16>(R * kz);
    w.dgi0 = ws.take<bf16>(4 * R * GL); w.dgh0 = ws.take<bf16>(4 * R * GL);
    w.dgi1 = ws.take<bf16>(4 * R * GL); w.dgh1 = ws.take<bf16>(4 * R * GL);
    w.dlogit_bf = ws.take<bf16>(4 * R * 16); w.dhinit = ws.take<bf16>(R * txt_hn(H));
}
template <class W>
void carve_text_enc_bwd(W& w, Workspace& ws, size_t B, size_t D, int H) {
    const size_t GL = txt_gl(H);
    w.d_txtout = ws.take<float>(B * 2 * D);
    w.te_dout_bf = ws.take<bf16>(B * round_up(2 * (int)D, 8));
    w.te_dgi_f = ws.take<bf16>(4 * B * GL); w.te_dgh_f = ws.take<bf16>(4 * B * GL); w.te_dgi_r = ws.take<bf16>(B * GL);
}

// ---- kernel arguments
template <class Plan>
GruPacked text_gru_of(const Plan& P, const TextGruIdx& g) {
    GruPacked r{};
    r.wih = P.buf.packed + P.pk.d[g.wih].dst_off; r.kih = P.pk.d[g.wih].Kpad;
    r.whh = P.buf.packed + P.pk.d[g.whh].dst_off;
    r.wihT = P.buf.packed + P.pk.d[g.wihT].dst_off; r.nih = P.pk.d[g.wihT].Npad;
    r.whhT = P.buf.packed + P.pk.d[g.whhT].dst_off;
    r.bih = P.buf.params + g.bih; r.bhh = P.buf.params + g.bhh;
    return r;
}
template <class Plan>
TextEncArgs text_enc_args(Plan& P, const long long* text, float* out, bool save) {
    auto& w = P.w;
    const std::string n = P.te_name;
    TextEncArgs a{};
    a.H = P.H;
    a.B = P.B; a.D = P.D; a.tokens = text; a.embed = P.buf.params + off(P, n + ".embed.weight");
    a.fwd = text_gru_of(P, P.te_f); a.rev = text_gru_of(P, P.te_r);
    a.h2p = P.buf.packed + P.pk.d[P.te_h2p].dst_off; a.nh2p = P.pk.d[P.te_h2p].Npad;
    a.h2pT = P.buf.packed + P.pk.d[P.te_h2pT].dst_off;
    a.h2p_bias = P.buf.params + off(P, n + ".h2p.bias");
    a.out = out;
    if (save) { a.gates_f = w.te_gates_f; a.gates_r = w.te_gates_r; a.x_bf = w.te_x; a.hprev_bf = w.te_hprev; a.hsum_bf = w.te_hsum; }
    return a;
}
// the encoder's BPTT kernel and its four weight gradients as ONE grouped launch
template <class Plan>
int text_enc_bwd(Plan& P, const long long* text, const float* d_out, hipStream_t s) {
    auto& w = P.w;
    const int B = P.B, D2 = 2 * P.D, H = P.H, HP = txt_hp(H), G3 = 3 * H, GL = txt_gl(H);
    const std::string n = P.te_name;
    TextEncBwdArgs a{};
    a.f = text_enc_args(P, text, nullptr, true);
    a.d_out = d_out; a.d_out_bf = w.te_dout_bf;
    a.dgi_f = w.te_dgi_f; a.dgh_f = w.te_dgh_f; a.dgi_r = w.te_dgi_r;
    float* G = P.buf.grads;
    a.g_embed = G + off(P, n + ".embed.weight");
    a.g_bih_f = G + P.te_f.bih; a.g_bhh_f = G + P.te_f.bhh; a.g_bih_r = G + P.te_r.bih; a.g_bhh_r = G + P.te_r.bhh;
    a.g_h2p_bias = G + off(P, n + ".h2p.bias");
    MMVAE_TRY(launch_text_encoder_bwd(a, s));
    WgradParams list[4];
    int nl = 0;
    auto wg = [&](int gidx, const bf16* Pm, int N, int ldp, const bf16* Gm, int C, int rows) {
        GatherPlan pl = dense_plan(rows, C, C, N);
        WgradParams g = wgrad_of(P, pl, &gidx, 1, rows);
        g.c.A = Gm; g.P = Pm; g.ldp = ldp;
        list[nl++] = g;
    };
    wg(P.te_f.g_wih, w.te_dgi_f, G3, GL, w.te_x, HP, 4 * B);
    wg(P.te_f.g_whh, w.te_dgh_f, G3, GL, w.te_hprev, HP, 4 * B);
    wg(P.te_r.g_wih, w.te_dgi_r, G3, GL, w.te_x + (size_t)3 * B * HP, HP, B);
    wg(P.g_te_h2p, w.te_dout_bf, D2, round_up(D2, 8), w.te_hsum, HP, B);
    MMVAE_TRY(launch_wgrad_group(list, nl, s, &P.slab));
    return launch_wgrad_reduce(&P.slab, s, true);
}
template <class Plan>
TextDecArgs text_dec_args(Plan& P, const float* z, int groups, bool save) {
    auto& w = P.w;
    const std::string n = P.td_name;
    TextDecArgs a{};
    a.H = P.H;
    a.R = groups * P.B; a.D = P.D; a.rows_per_pass = P.B; a.z = z;
    a.embed = P.buf.params + off(P, n + ".embed.weight");
    a.z2h = P.buf.packed + P.pk.d[P.td_z2h].dst_off; a.kz = P.kz;
    a.z2hT = P.buf.packed + P.pk.d[P.td_z2hT].dst_off;
    a.z2h_bias = P.buf.params + off(P, n + ".z2h.bias");
    a.l0 = text_gru_of(P, P.td0); a.l1 = text_gru_of(P, P.td1);
    a.h2o = P.buf.packed + P.pk.d[P.td_h2o].dst_off; a.kx = P.kx;
    a.h2oT = P.buf.packed + P.pk.d[P.td_h2oT].dst_off;
    a.h2o_bias = P.buf.params + off(P, n + ".h2o.bias");
    a.words = w.words; a.tokens_out = w.tokens;
    if (save) {
        a.gates = w.td_gates; a.x0_bf = w.td_x0; a.h0p_bf = w.td_h0p; a.mid_bf = w.td_mid; a.h1p_bf = w.td_h1p;
        a.hz_bf = w.td_hz; a.z_bf = w.td_zbf;
    }
    return a;
}
template <class Plan>
TextDecBwdArgs text_dec_bwd_args(Plan& P, const TextDecArgs& f, const float* dwords, float* dz) {
    auto& w = P.w;
    const std::string n = P.td_name;
    TextDecBwdArgs a{};
    a.f = f; a.dwords = dwords; a.R_active = f.R; a.dz = dz;
    a.dgi0 = w.dgi0; a.dgh0 = w.dgh0; a.dgi1 = w.dgi1; a.dgh1 = w.dgh1; a.dlogit_bf = w.dlogit_bf; a.dhinit_bf = w.dhinit;
    float* G = P.buf.grads;
    a.g_embed = G + off(P, n + ".embed.weight");
    a.g_b[0] = G + P.td0.bih; a.g_b[1] = G + P.td0.bhh; a.g_b[2] = G + P.td1.bih; a.g_b[3] = G + P.td1.bhh;
    a.g_h2o_bias = G + off(P, n + ".h2o.bias"); a.g_z2h_bias = G + off(P, n + ".z2h.bias");
    return a;
}
// the six weight gradients of the text decoder: one grouped launch (128x128 tile class) + the thin h2o one
template <class Plan>
int text_dec_wgrads(Plan& P, int R, hipStream_t s) {
    auto& w = P.w;
    const int H = P.H, HP = txt_hp(H), G3 = 3 * H, GL = txt_gl(H);
    WgradParams list[6];
    int nl = 0;
    auto wg = [&](int gidx, const bf16* Pm, int N, int ldp, const bf16* Gm, int C, int rows) {
        GatherPlan pl = dense_plan(rows, C, C, N);
        WgradParams g = wgrad_of(P, pl, &gidx, 1, rows);
        g.c.A = Gm; g.P = Pm; g.ldp = ldp;
        list[nl++] = g;
    };
    wg(P.td0.g_wih, w.dgi0, G3, GL, w.td_x0, P.kx, 4 * R);
    wg(P.td0.g_whh, w.dgh0, G3, GL, w.td_h0p, HP, 4 * R);
    wg(P.td1.g_wih, w.dgi1, G3, GL, w.td_mid, HP, 4 * R);
    wg(P.td1.g_whh, w.dgh1, G3, GL, w.td_h1p, HP, 4 * R);
    wg(P.g_td_z2h, w.dhinit, H, txt_hn(H), w.td_zbf, P.kz, R);
    wg(P.g_td_h2o, w.dlogit_bf, TXT_V, 16, w.td_hz, P.kx, 4 * R);
    MMVAE_TRY(launch_wgrad_group(list, nl, s, &P.slab));
    return launch_wgrad_reduce(&P.slab, s, true);
}
