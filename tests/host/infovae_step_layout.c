/* Prints sizeof and every offsetof of mmvae_infovae_step_io (include/mmvae_hip.h), compiled as C99 (the header's own language):
 * tests/test_cpu_infovae_step.py compares them with the ctypes mirror InfoVAEStepIO of multimodal-vae_amd/_lib.py, and the leading
 * fields with mmvae_image_step_io (the step hands them on to the image-only step).
 * One line: "<ctypes class> <sizeof> <field>:<offset> ..." in declaration order, then the same line for mmvae_image_step_io. */
#include <stddef.h>
#include <stdio.h>
#include "mmvae_hip.h"

#define F(f) printf(" %s:%zu", #f, offsetof(mmvae_infovae_step_io, f))
#define G(f) printf(" %s:%zu", #f, offsetof(mmvae_image_step_io, f))

int main(void) {
    printf("InfoVAEStepIO %zu", sizeof(mmvae_infovae_step_io));
    F(ws); F(ws_bytes); F(step_counter); F(image); F(eps); F(enc_mask1); F(enc_mask2); F(enc_dropout); F(kl_lambda); F(lambda_x);
    F(seed); F(sums); F(recon_image); F(mu); F(logvar); F(defer_unpack); F(true_samples); F(lambda_mmd); F(z);
    printf("\n");
    printf("ImageStepIO %zu", sizeof(mmvae_image_step_io));
    G(ws); G(ws_bytes); G(step_counter); G(image); G(eps); G(enc_mask1); G(enc_mask2); G(enc_dropout); G(kl_lambda); G(lambda_x);
    G(seed); G(sums); G(recon_image); G(mu); G(logvar); G(defer_unpack);
    printf("\n");
    printf("slots %d %d %d %d stream %d\n", MMVAE_SUM_MMD_KXX, MMVAE_SUM_MMD_KYY, MMVAE_SUM_MMD_KXY, MMVAE_SUM_MMD, MMVAE_TRUE_SAMPLES_STREAM);
    return 0;
}
