// Host program over multimodal-vae_amd/csrc/imgprep_core.h (tests/test_cpu_imgprep.py compiles it with the host compiler, sanitizers
// on): the header is plain C++17, and what it computes equals the numpy restatement (tests/imgprep_ref.py).
// usage: imgprep_core_check W H S   ->  "size ow oh x1 y1", then per axis (h: horizontal, v: vertical) and window index
//        "<axis> <index> <xmin> <n> <k_0> ... <k_n-1>"
#include <cstdio>
#include <cstdlib>

#include "imgprep_core.h"

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int w = atoi(argv[1]), h = atoi(argv[2]), S = atoi(argv[3]);
    if (!imgprep::sides_ok(h, w) || S < 1 || S > imgprep::MAX_OUT) return 3;
    int ow, oh;
    imgprep::scaled_size(w, h, S, &ow, &oh);
    const int first[2] = {imgprep::crop_offset(ow - S), imgprep::crop_offset(oh - S)};
    printf("size %d %d %d %d\n", ow, oh, first[0], first[1]);
    const int n_in[2] = {w, h}, n_out[2] = {ow, oh};
    for (int ax = 0; ax < 2; ++ax)
        for (int j = 0; j < S; ++j) {
            const imgprep::Span sp = imgprep::span_of(n_in[ax], n_out[ax], first[ax] + j);
            printf("%c %d %d %d", ax ? 'v' : 'h', first[ax] + j, sp.xmin, sp.n);
            for (int t = 0; t < sp.n; ++t) printf(" %d", imgprep::coef_at(n_in[ax], n_out[ax], first[ax] + j, sp.xmin, sp.ww, t));
            printf("\n");
        }
    // one line of pixels through clip8, at the extremes
    if (imgprep::clip8(-1) != 0 || imgprep::clip8((256 << imgprep::PRECISION_BITS)) != 255 || imgprep::clip8(7 << imgprep::PRECISION_BITS) != 7) return 4;
    return 0;
}
