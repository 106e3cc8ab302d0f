/* Prints sizeof and every offsetof of mmvae_mm_text_step_io (include/mmvae_hip.h), compiled as C99 (the header's own language):
 * tests/test_cpu_textonly_mm.py compares them with the ctypes mirror MMTextStepIO of multimodal-vae_amd/_lib.py.
 * One line: "<ctypes class> <sizeof> <field>:<offset> ..." in declaration order. */
#include <stddef.h>
#include <stdio.h>
#include "mmvae_hip.h"

#define F(f) printf(" %s:%zu", #f, offsetof(mmvae_mm_text_step_io, f))

int main(void) {
    printf("MMTextStepIO %zu", sizeof(mmvae_mm_text_step_io));
    F(ws); F(ws_bytes); F(step_counter); F(text); F(eps); F(gru_keep); F(gru_dropout); F(force_tokens); F(kl_lambda); F(lambda_y);
    F(seed); F(sums); F(recon_text); F(mu); F(logvar); F(tokens); F(defer_unpack); F(pack_first);
    printf("\n");
    return 0;
}
