// Text-only VAE baseline of MultiMNIST: TextVAE of multimnist/model.py:123-147 (TextEncoder / TextDecoder at n_hiddens = 50, no
// product of experts) and the train() closure of multimnist/train_textonly.py:95-113 as one enqueue.
// The kernels are the MMVAE's text path (text.hip) instantiated for the plan's hidden size; parameter table, weight packs, workspace
// pieces and kernel arguments come from text_plan.h, shared with the MMVAE's plan.
#include "mmtext.h"
#include "plan_base.h"
#include "text_plan.h"

struct MMTextPlan : PlanBase {
    int H = 50, ldz = 0, kx = 0, kz = 0;
    const char *te_name = "encoder", *td_name = "decoder";
    TextGruIdx te_f, te_r, td0, td1;
    int te_h2p, te_h2pT, g_te_h2p, td_z2h, td_z2hT, g_td_z2h, td_h2o, td_h2oT, g_td_h2o;
    struct W {
        char* zero_begin; size_t zero_bytes;
        float* sums; float* dz_txt;
        uint8_t* gkeep;
        float *txtout, *te_gates_f, *te_gates_r; bf16 *te_x, *te_hprev, *te_hsum;
        float *eps, *mu, *logvar, *z_f32, *lat_scratch; bf16* z_bf;
        float *words, *dwords, *td_gates; long long* tokens;
        bf16 *td_x0, *td_h0p, *td_mid, *td_h1p, *td_hz, *td_zbf;
        bf16 *dgi0, *dgh0, *dgi1, *dgh1, *dlogit_bf, *dhinit;
        float* d_txtout; bf16* te_dout_bf; bf16 *te_dgi_f, *te_dgh_f, *te_dgi_r;
        float* slab; size_t slab_floats;
    } w;
};

namespace {

// One pass over B rows whatever PlanBase::carve_passes says: the step, the modules and the scorer share this carve
void carve(MMTextPlan& P, Workspace& ws) {
    MMTextPlan::W& w = P.w;
    const size_t B = P.B, D = P.D;
    char* z0 = ws.take<char>(0);
    w.sums = ws.take<float>(16 * MMVAE_LOSS_SLOTS);
    w.dz_txt = ws.take<float>(B * D);
    char* z1 = ws.take<char>(0);
    w.zero_begin = z0; w.zero_bytes = (size_t)(z1 - z0);
    w.gkeep = ws.take<uint8_t>(4 * B * P.H);
    carve_text_enc(w, ws, B, D, P.H);
    w.eps = ws.take<float>(B * D); w.mu = ws.take<float>(B * D); w.logvar = ws.take<float>(B * D);
    w.z_f32 = ws.take<float>(B * D); w.z_bf = ws.take<bf16>(B * P.ldz);
    w.lat_scratch = ws.take<float>(launch_latent1_scratch_floats((int)B, (int)D));
    carve_text_dec(w, ws, B, P.H, P.kx, P.kz);
    carve_text_enc_bwd(w, ws, B, D, P.H);
    // weight-gradient partial-tile slabs (written and read once per step, never zeroed): the size the MMVAE's one-pass carve gives them
    w.slab_floats = (size_t)16 << 20;
    w.slab = ws.take<float>(w.slab_floats);
}

int use_ws(MMTextPlan* P, void* ws, size_t bytes) { return plan_use_ws(P, ws, bytes, true, carve); }

int dec_bwd(MMTextPlan& P, const TextDecArgs& f, const float* dwords, float* dz, hipStream_t s) {
    const TextDecBwdArgs a = text_dec_bwd_args(P, f, dwords, dz);
    MMVAE_TRY(launch_text_decoder_bwd(a, s));
    return text_dec_wgrads(P, f.R, s);
}

int step_body(MMTextPlan* Pp, const mmvae_mm_text_step_io& io, int training, int do_backward, hipStream_t s) {
    MMVAE_TRY(use_ws(Pp, io.ws, io.ws_bytes));
    MMTextPlan& P = *Pp;
    MMTextPlan::W& w = P.w;
    const int B = P.B, D = P.D;
    MMVAE_REQUIRE(io.text && io.sums, "mmvae_mmtext_step: text/sums must be given");
    // ---- one prologue launch: zero the accumulators and the gradient buffers, draw eps / keep flags unless the caller injected them
    const float* eps = io.eps;
    const uint8_t* gk = io.gru_keep;
    StepBeginArgs sb{};
    sb.zero_ptr[0] = w.zero_begin; sb.zero_bytes[0] = w.zero_bytes;
    if (do_backward) {
        sb.zero_ptr[1] = P.buf.gpk; sb.zero_bytes[1] = (size_t)P.gk.mat_elems * sizeof(float);
        sb.zero_ptr[2] = P.buf.grads; sb.zero_bytes[2] = (size_t)(P.nparams / 4) * 16;     // tail (< 4 floats) below
    }
    sb.p = DROP_P; sb.seed = io.seed; sb.step = io.step_counter;
    if (training && !eps) { sb.eps = w.eps; sb.n_eps = (long long)B * D; eps = w.eps; }
    if (training && io.gru_dropout && !gk) { sb.mask[2] = w.gkeep; sb.n_mask[2] = (long long)4 * B * P.H; gk = w.gkeep; }
    if (!(training && io.gru_dropout)) gk = nullptr;
    if (io.pack_first)
        MMVAE_TRY(step_begin_with_pack(sb, P.buf.desc_dev, P.pk.d.data(), (int)P.pk.d.size(), P.buf.params, P.buf.packed, P.buf.packed_vec));
    MMVAE_TRY(launch_step_begin(sb, s));
    if (do_backward && P.nparams % 4 != 0)
        MMVAE_TRY(launch_fill_zero(P.buf.grads + (P.nparams / 4) * 4, (size_t)(P.nparams % 4) * sizeof(float), s));
    // ---- encoder, the one-expert latent block (mu | logvar are the encoder's halves bit for bit), decoder on ONE row group + NLL
    {
        TextEncArgs a = text_enc_args(P, io.text, w.txtout, do_backward != 0);
        MMVAE_TRY(launch_text_encoder_fwd(a, s));
    }
    Latent1Args la{};
    la.B = B; la.D = D; la.enc_out = w.txtout; la.eps = eps;
    la.mu = io.mu ? io.mu : w.mu; la.logvar = io.logvar ? io.logvar : w.logvar;
    la.z_f32 = w.z_f32; la.z_bf = w.z_bf; la.ldz = P.ldz; la.kl_sum = w.sums + 8; la.training = training;
    la.scratch = w.lat_scratch;
    MMVAE_TRY(launch_latent1_fwd(la, s));
    TextDecArgs td = text_dec_args(P, w.z_f32, 1, do_backward != 0);
    td.keep = gk; td.keep_scale = 1.f / (1.f - DROP_P);
    td.force_tokens = io.force_tokens;
    if (io.recon_text) td.words = io.recon_text;
    if (io.tokens) td.tokens_out = io.tokens;
    td.target = io.text; td.nll_sum = w.sums + 4; td.dwords = do_backward ? w.dwords : nullptr;
    td.nll_coef[0] = io.lambda_y / (float)(B * TXT_T);
    MMVAE_TRY(launch_text_decoder_fwd(td, s));
    if (do_backward) {
        MMVAE_TRY(dec_bwd(P, td, w.dwords, w.dz_txt, s));
        Latent1BwdF32Args lb{};
        lb.B = B; lb.D = D; lb.mu = la.mu; lb.logvar = la.logvar; lb.eps = eps; lb.dz = w.dz_txt; lb.training = training;
        lb.kl_coef = io.kl_lambda / (float)B; lb.d_enc_out = w.d_txtout; lb.ld = 2 * D;
        MMVAE_TRY(launch_latent1_bwd_f32(lb, s));
        MMVAE_TRY(text_enc_bwd(P, io.text, w.d_txtout, s));
        if (io.defer_unpack) MMVAE_TRY(launch_wgrad_reduce(&P.slab, s));      // the packed gradients are complete; Adam gathers them
        else MMVAE_TRY(plan_unpack(P, s, true));
    }
    hipLaunchKernelGGL(sum_slots_kernel, dim3(1), dim3(64), 0, s, w.sums, io.sums);
    return mmvae_check_launch("sum_slots");
}

}  // namespace

MMTextPlan* mmtext_create(int D, int H, int B) {
    if (D < 1 || D > 127 || B < 1) { mmvae_set_error("mmvae_mmtext_create: need 1 <= n_latents <= 127 and batch >= 1 (got %d, %d)", D, B); return nullptr; }
    if (H != 50 && H != TXT_H) {
        mmvae_set_error("mmvae_mmtext_create: n_hiddens = %d is not built: the text kernels are compiled for 50 and %d", H, TXT_H);
        return nullptr;
    }
    MMTextPlan* P = new MMTextPlan();
    P->D = D; P->B = B; P->H = H;
    P->ldz = round_up(D + 1, 8);
    text_add_encoder_params(*P);
    text_add_decoder_params(*P);
    text_build_packs(*P);
    plan_size_workspaces(*P, carve);
    return P;
}
void mmtext_destroy(MMTextPlan* P) { delete P; }
PlanBase* mmtext_base(MMTextPlan* P) { return P; }
int mmtext_hidden(const MMTextPlan* P) { return P ? P->H : 0; }

int mmtext_step(MMTextPlan* P, const mmvae_mm_text_step_io& io, int training, int do_backward, hipStream_t s) {
    return plan_step(P, io, training, do_backward, s, step_body);
}

// ---------------------------------------------------------------- granular module entry points (drop-in modules)
int mmtext_encoder_fwd(MMTextPlan* P, void* ws, size_t wsb, const long long* text, float* out, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    TextEncArgs a = text_enc_args(*P, text, out, true);
    return launch_text_encoder_fwd(a, s);
}
int mmtext_encoder_bwd(MMTextPlan* P, void* ws, size_t wsb, const long long* text, const float* d_out, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    MMVAE_TRY(plan_zero_gpk(*P, s));
    MMVAE_TRY(text_enc_bwd(*P, text, d_out, s));
    return plan_unpack(*P, s, true);
}
int mmtext_decoder_fwd(MMTextPlan* P, void* ws, size_t wsb, const float* z, int training, const uint8_t* keep, const long long* force_tokens,
                       float* words, long long* tokens, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    TextDecArgs a = text_dec_args(*P, z, 1, true);
    a.keep = training ? keep : nullptr; a.keep_scale = 1.f / (1.f - DROP_P);
    a.force_tokens = force_tokens; a.words = words; a.tokens_out = tokens;
    return launch_text_decoder_fwd(a, s);
}
int mmtext_decoder_bwd(MMTextPlan* P, void* ws, size_t wsb, const float* z, const uint8_t* keep, const long long* force_tokens,
                       const float* words, const long long* tokens, const float* d_words, float* dz, hipStream_t s) {
    MMVAE_TRY(use_ws(P, ws, wsb));
    MMVAE_TRY(plan_zero_gpk(*P, s));
    TextDecArgs a = text_dec_args(*P, z, 1, true);
    a.keep = keep; a.keep_scale = 1.f / (1.f - DROP_P);
    a.force_tokens = force_tokens; a.words = const_cast<float*>(words); a.tokens_out = const_cast<long long*>(tokens);
    MMVAE_TRY(dec_bwd(*P, a, d_words, dz, s));
    return plan_unpack(*P, s, true);
}

// ---------------------------------------------------------------- importance-weighted evaluation (iw.h)
// The eval-mode decoder on the B*K particle rows z [B][K][D]: its greedy log-softmax outputs, exactly the text half of mm_iw_score.
int mmtext_iw_score(MMTextPlan* P, void* ws, size_t wsb, const float* z, int B, int K, float* words, hipStream_t s) {
    MMVAE_REQUIRE(P && z && words, "mmvae_mmtext_iw_score: null argument");
    MMVAE_REQUIRE(B >= 1 && K >= 1 && (long long)B * K <= P->B,
                  "mmvae_mmtext_iw_score: %d examples x %d particles exceed the plan's %d rows", B, K, P->B);
    MMVAE_TRY(use_ws(P, ws, wsb));
    TextDecArgs a = text_dec_args(*P, z, 1, false);
    a.R = B * K; a.words = words;
    return launch_text_decoder_fwd(a, s);
}
