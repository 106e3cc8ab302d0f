// MultiMNIST text path (multimnist/model.py:219-307): persistent row-tile kernels, one launch per direction.
// Each workgroup owns 16 batch rows (rows are independent: no BatchNorm on this path) and runs the whole
// recurrence for them; every matmul is a 16-row MFMA tile against packed bf16 weights streamed from L2.
#pragma once
#include "common.h"

// The kernels are compiled for two hidden sizes: 100 (MultimodalVAE, multimnist/model.py:26,29) and 50 (the text-only baseline
// TextVAE, model.py:123-128).  Every size below follows from H; the TXT_* macros are the H = 100 values the MMVAE's plan uses.
constexpr int txt_hp(int H) { return (H + 31) / 32 * 32; }             // hidden size padded to an MFMA K multiple
constexpr int txt_hn(int H) { return (H + 15) / 16 * 16; }             // ... to an MFMA N tile (rows of the transposed packs)
constexpr int txt_gl(int H) { return (3 * H + 15) / 16 * 16; }         // 3*H gate columns padded to 16 (row stride)
constexpr int txt_gk(int H) { return (3 * H + 31) / 32 * 32; }         // ... padded to 32 (as a reduction dim)
constexpr int txt_kx(int H, int D) { return (H + D + 31) / 32 * 32; }  // the [c_in | z] operand of the decoder
#define TXT_H 100
#define TXT_HP txt_hp(TXT_H)
#define TXT_G3 (3 * TXT_H)
#define TXT_G3P txt_gl(TXT_H)
#define TXT_G3K txt_gk(TXT_H)
#define TXT_T 4            // max_length (multimnist/utils.py:14)
#define TXT_V 12           // n_characters

// (sizes in the comments below: HP = txt_hp(H), HN = txt_hn(H), GL = txt_gl(H), GK = txt_gk(H))
struct GruPacked {
    const bf16* wih;  int kih;    // [GL][kih]   (gate-major, K = input features padded to 32)
    const bf16* whh;              // [GL][HP]
    const bf16* wihT; int nih;    // [nih][GK]   transposed copy for backward (nih = input features padded to 16)
    const bf16* whhT;             // [HN][GK]
    const float* bih; const float* bhh;   // fp32 [3H]
};

struct TextEncArgs {
    int B, D;
    const long long* tokens;       // [B][4]
    const float* embed;            // [12][H] fp32
    GruPacked fwd, rev;
    const bf16* h2p;  int nh2p;    // [round16(2D)][HP]
    const bf16* h2pT;              // [HN][round32(2D)]
    const float* h2p_bias;         // [2D]
    float* out;                    // [B][2D]  (mu | logvar)
    // saved for backward (may be null in eval)
    float* gates_f;                // [4][5][B][H]  r,z,n,ghn,hprev
    float* gates_r;                // [5][B][H]
    bf16* x_bf;                    // [4][B][HP] embedded tokens
    bf16* hprev_bf;                // [4][B][HP]
    bf16* hsum_bf;                 // [B][HP]
    int H;                         // hidden size: 50 or 100 (the launcher dispatches on it)
};
int launch_text_encoder_fwd(const TextEncArgs& a, hipStream_t s);

struct TextEncBwdArgs {
    TextEncArgs f;
    const float* d_out;            // [B][2D]
    bf16* d_out_bf;                // [B][round8(2D)]  (P operand of the h2p wgrad)
    bf16* dgi_f; bf16* dgh_f;      // [4][B][GL]
    bf16* dgi_r;                   // [B][GL]
    float* g_embed;                // [12][H] +=
    float* g_bih_f; float* g_bhh_f; float* g_bih_r; float* g_bhh_r;   // [3H] +=
    float* g_h2p_bias;             // [2D] +=
};
int launch_text_encoder_bwd(const TextEncBwdArgs& a, hipStream_t s);

struct TextDecArgs {
    int R, D;                      // rows (= passes*B), latent size
    int rows_per_pass;             // B (for the per-pass NLL sums)
    const float* z;                // [R][D]
    const float* embed;            // [12][H]
    const bf16* z2h;  int kz;      // [HN][kz]  kz = round32(D)
    const bf16* z2hT;              // [round16(D)][HP]
    const float* z2h_bias;         // [H]
    GruPacked l0, l1;              // l0 input = H + D features
    const bf16* h2o;  int kx;      // [16][kx]   kx = txt_kx(H, D) = round32(H+D)
    const bf16* h2oT;              // [round16(H+D)][32]
    const float* h2o_bias;         // [12]
    const uint8_t* keep;           // [4][R][H] inter-layer dropout keep flags, null = no dropout
    float keep_scale;
    const long long* force_tokens; // [R][4] or null (test hook: overrides the greedy feedback)
    float* words;                  // [R][4][12] log-probs
    long long* tokens_out;         // [R][4] greedy argmax, may be null
    // fused NLL (multimnist/train.py:79): target tokens shared by all passes
    const long long* target;       // [rows_per_pass][4] or null
    float* nll_sum;                // [passes] += sum of -logp[target]
    float* dwords;                 // [R][4][12] = coef[pass] * dNLL/dlogp, or null
    float nll_coef[4];
    // saved for backward (null in eval)
    float* gates;                  // [4][2][5][R][H]
    bf16* x0_bf;                   // [4][R][kx]
    bf16* h0p_bf; bf16* mid_bf; bf16* h1p_bf;   // [4][R][HP]
    bf16* hz_bf;                   // [4][R][kx]
    bf16* z_bf;                    // [R][kz]
    unsigned long long* ts;        // measurement aid (knobs txt_ts_lo / txt_ts_hi, set by the launcher): s_memrealtime stamps of workgroup 0's phases, or null
    int H;                         // hidden size: 50 or 100 (the launcher dispatches on it; the weights-resident forward exists at 100 only)
};
int launch_text_decoder_fwd(const TextDecArgs& a, hipStream_t s);

struct TextDecBwdArgs {
    TextDecArgs f;
    const float* dwords;           // [R][4][12] grad wrt log-probs
    int R_active;                  // rows [0, R_active) carry gradient (text-only pass with lambda 0 never happens here)
    float* dz;                     // [R][D] out
    bf16* dgi0; bf16* dgh0; bf16* dgi1; bf16* dgh1;   // [4][R][GL]
    bf16* dlogit_bf;               // [4][R][16]
    bf16* dhinit_bf;               // [R][HN]
    float* g_embed;                // [12][H] +=
    float* g_b[4];                 // bih0, bhh0, bih1, bhh1  [3H] +=
    float* g_h2o_bias;             // [12] +=
    float* g_z2h_bias;             // [H] +=
};
int launch_text_decoder_bwd(const TextDecBwdArgs& a, hipStream_t s);
