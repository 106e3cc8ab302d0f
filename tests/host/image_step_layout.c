/* Prints sizeof and every offsetof of mmvae_image_step_io (include/mmvae_hip.h), compiled as C99 (the header's own language):
 * tests/test_cpu_imageonly.py compares them with the ctypes mirror ImageStepIO of multimodal-vae_amd/_lib.py.
 * One line: "<ctypes class> <sizeof> <field>:<offset> ..." in declaration order. */
#include <stddef.h>
#include <stdio.h>
#include "mmvae_hip.h"

#define F(f) printf(" %s:%zu", #f, offsetof(mmvae_image_step_io, f))

int main(void) {
    printf("ImageStepIO %zu", sizeof(mmvae_image_step_io));
    F(ws); F(ws_bytes); F(step_counter); F(image); F(eps); F(enc_mask1); F(enc_mask2); F(enc_dropout); F(kl_lambda); F(lambda_x);
    F(seed); F(sums); F(recon_image); F(mu); F(logvar); F(defer_unpack);
    printf("\n");
    return 0;
}
