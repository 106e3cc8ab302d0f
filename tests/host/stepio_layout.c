/* Prints sizeof and every offsetof of the step-io structs of include/mmvae_hip.h, compiled as C (the header's own language):
 * tests/test_cpu_host.py compares them with the ctypes mirrors in multimodal-vae_amd/_lib.py.
 * One line per struct: "<ctypes class> <sizeof> <field>:<offset> ..." in declaration order. */
#include <stddef.h>
#include <stdio.h>
#include "mmvae_hip.h"

#define BEGIN(cls, T) printf("%s %zu", cls, sizeof(T))
#define F(T, f) printf(" %s:%zu", #f, offsetof(T, f))
#define END() printf("\n")

int main(void) {
    BEGIN("StepIO", mmvae_mm_step_io);
#define M(f) F(mmvae_mm_step_io, f)
    M(ws); M(ws_bytes); M(step_counter); M(image); M(text); M(eps); M(enc_mask1); M(enc_mask2); M(gru_keep);
    M(enc_dropout); M(gru_dropout); M(force_tokens); M(kl_lambda); M(lambda_xy); M(lambda_yx); M(seed);
    M(sums); M(recon_image); M(recon_text); M(mu); M(logvar); M(tokens); M(pass_skip); M(defer_unpack);
    M(pack_first); M(dp_split); M(early_adam);
#undef M
    END();
    BEGIN("EarlyAdam", struct mmvae_early_adam);
#define M(f) F(struct mmvae_early_adam, f)
    M(m); M(v); M(state); M(lr); M(beta1); M(beta2); M(eps); M(grad_scale); M(gmap); M(ran);
#undef M
    END();
    BEGIN("MnistStepIO", mmvae_mnist_step_io);
#define M(f) F(mmvae_mnist_step_io, f)
    M(ws); M(ws_bytes); M(step_counter); M(image); M(label); M(eps); M(lambda_xy); M(lambda_yx); M(kl_coef); M(seed);
    M(sums); M(recon_image); M(recon_text); M(mu); M(logvar); M(pass_skip);
#undef M
    END();
    BEGIN("CelebaStepIO", mmvae_celeba_step_io);
#define M(f) F(mmvae_celeba_step_io, f)
    M(ws); M(ws_bytes); M(step_counter); M(image); M(attrs); M(eps); M(enc_mask); M(enc_dropout); M(kl_lambda);
    M(lambda_x); M(lambda_y); M(seed); M(sums); M(recon_image); M(recon_attrs); M(mu); M(logvar); M(pass_skip);
    M(defer_unpack);
#undef M
    END();
    BEGIN("CocoStepIO", mmvae_coco_step_io);
#define M(f) F(mmvae_coco_step_io, f)
    M(ws); M(ws_bytes); M(step_counter); M(image); M(text); M(sos); M(eps); M(enc_mask1); M(enc_mask2); M(gru_keep);
    M(enc_dropout); M(gru_dropout); M(kl_lambda); M(lambda_xy); M(lambda_yx); M(seed); M(sums); M(recon_image);
    M(recon_text); M(mu); M(logvar); M(pass_skip); M(defer_unpack); M(pack_first); M(optimizer_state);
#undef M
    END();
    return 0;
}
