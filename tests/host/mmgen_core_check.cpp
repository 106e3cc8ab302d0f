// Host program over multimodal-vae_amd/csrc/mmgen_core.h (tests/test_cpu_multimnist_gen.py compiles it with
// -fsanitize=address,undefined): prints the tables and the draws of a few hundred canvases, one record per line, for comparison with
// the numpy restatement (tests/multimnist_gen_ref.py).  usage: mmgen_core_check SEED FIRST N M
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mmgen_core.h"

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const uint64_t seed = strtoull(argv[1], nullptr, 10), first = strtoull(argv[2], nullptr, 10);
    const int n = atoi(argv[3]);
    const uint32_t M = (uint32_t)strtoul(argv[4], nullptr, 10);
    std::vector<int32_t> tab(mmgen::TABLE_WORDS);
    const int taps = mmgen::build_tables(tab.data());
    printf("taps %d words %d\n", taps, (int)mmgen::TABLE_WORDS);
    printf("table");
    for (int32_t v : tab) printf(" %d", v);
    printf("\n");
    const uint32_t* T = reinterpret_cast<const uint32_t*>(tab.data() + mmgen::T_OFFSET);
    const int flag_sets[] = {0, mmgen::F_NO_RESIZE, mmgen::F_NO_TRANSLATE, mmgen::F_FIXED | mmgen::F_REVERSE, mmgen::F_FIXED | mmgen::F_SCRAMBLE};
    for (int flags : flag_sets) {
        if (!mmgen::flags_ok(flags, 0, 4)) return 3;
        for (int i = 0; i < n; ++i) {
            const uint64_t c = first + (uint64_t)i;
            const mmgen::CanvasDraw cd = mmgen::draw_canvas(seed, c, 0, 4);
            int order[mmgen::MAX_DIGITS];
            mmgen::label_order(cd, flags, order);
            printf("canvas %d %llu %d %d %u order", flags, (unsigned long long)c, cd.k, cd.reverse, cd.scramble);
            for (int j = 0; j < cd.k; ++j) printf(" %d", order[j]);
            printf("\n");
            const int at[] = {0, 1, mmgen::MAX_ATTEMPTS - 1}, rd[] = {0, mmgen::MAX_REDRAWS - 1};
            for (int a : at)
                for (int j = 0; j < mmgen::MAX_DIGITS; ++j)
                    for (int t : rd) {
                        const mmgen::DigitDraw d = mmgen::draw_digit(seed, c, a, j, t, flags, M, T);
                        printf("digit %d %llu %d %d %d %d %d %d %d\n", flags, (unsigned long long)c, a, j, t, d.index, d.side, d.top, d.left);
                    }
        }
    }
    // the resize of one line through the table rows, as the kernels call it
    uint8_t line[mmgen::DIGIT];
    for (int x = 0; x < mmgen::DIGIT; ++x) line[x] = (uint8_t)((x * 37 + 11) & 255);
    for (int s = mmgen::SIDE_MIN; s <= mmgen::SIDE_MAX; ++s) {
        printf("line %d", s);
        for (int xx = 0; xx < s; ++xx) printf(" %d", mmgen::resample_at(line, 1, tab.data() + (s - mmgen::SIDE_MIN) * mmgen::SIDE_WORDS, xx));
        printf("\n");
    }
    printf("ok\n");
    return 0;
}
