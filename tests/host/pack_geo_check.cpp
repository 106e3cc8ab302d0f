// Host-side replay of the weight pack's index arithmetic (multimodal-vae_amd/csrc/pack_geo.h; the kernel is pack_block in
// elementwise.hip).  For a hand-written list of descriptors with the real layers' sizes it walks every block, wave and lane the
// way the kernel does and checks that
//   - every vector of the packed matrix is written exactly once, inside the matrix;
//   - what it holds is the element the ORIGINAL formula names (restated below as ref_src), the folded bias or zero;
//   - every read is inside the parameter tensor of the descriptor;
//   - every load instruction of a wave reads runs of at least 64 bytes.
// What "run" means, by kind of descriptor:
//   run assignment, all taps (step_t == 1):  the addresses of ONE load instruction (fixed j of the 8 channel loads), sorted, fall
//       into stretches of consecutive floats; each stretch is >= 64 B.
//   run assignment, stride-parity class (step_t == 2):  a class owns every second tap in y and x, the floats between them belong to
//       its sister classes and cannot be useful to this descriptor.  A run is a stretch whose neighbouring addresses are less than
//       64 B apart (no untouched 64-byte piece inside), and its span is >= 64 B.
//   row-major assignment (descriptors that are contiguous already, s_c == 1 or C < 8):  a lane's 8 loads are 8 consecutive
//       columns, so the unit is the wave's 8 loads together: their union falls into stretches of consecutive floats of >= 64 B
//       (or the whole row, where a row is shorter than that: conv1's 16 taps are exactly 64 B).
// The pack uses no LDS, so there is no LDS index to check.
#include "pack_geo.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures < 20) { std::printf("FAIL %s: ", name); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static int round_up(int a, int b) { return (a + b - 1) / b * b; }

// the formula of the pack before the run assignment existed, written out once more
static long long ref_src(const PackDesc& d, int n, int k) {
    const int nhi = n / d.NL, nlo = n % d.NL;
    const int tap = k / d.C, c = k % d.C;
    const int ty = tap / d.TW, tx = tap % d.TW;
    return d.src_off + (long long)nhi * d.s_nhi + (long long)nlo * d.s_nlo + (long long)(d.o_ty + ty * d.step_t) * d.s_ty +
           (long long)(d.o_tx + tx * d.step_t) * d.s_tx + (long long)c * d.s_c;
}

static PackDesc dense(long long src, int N, int K, int Npad, int Kpad, int s_n, int s_k) {      // layers.h pack_dense
    PackDesc x{};
    x.src_off = src; x.N = N; x.K = K; x.Npad = Npad; x.Kpad = Kpad;
    x.NL = N; x.s_nhi = 0; x.s_nlo = s_n;
    x.TW = 1; x.C = K; x.s_ty = 0; x.s_tx = 0; x.s_c = s_k; x.step_t = 1;
    x.bias_off = -1;
    return x;
}
static PackDesc conv(long long src, int N, int C, int TH, int TW, int Npad, int s_n, int s_c, int KW, int o_ty, int o_tx, int step) {   // pack_conv
    PackDesc x{};
    x.src_off = src; x.N = N; x.K = TH * TW * C; x.Npad = Npad; x.Kpad = round_up(x.K, 64);
    x.NL = N; x.s_nhi = 0; x.s_nlo = s_n;
    x.TW = TW; x.C = C; x.s_ty = KW; x.s_tx = 1; x.s_c = s_c; x.o_ty = o_ty; x.o_tx = o_tx; x.step_t = step;
    x.bias_off = -1;
    return x;
}

struct Case { const char* name; PackDesc d; long long p_lo, p_hi; bool expect_runs; long long b_lo, b_hi; };

static const long long ZERO = -1, UNSET = -2;

static void runs_of(std::vector<long long>& a, long long max_gap, const char* name, const char* what, long long min_bytes) {
    if (a.empty()) return;
    std::sort(a.begin(), a.end());
    a.erase(std::unique(a.begin(), a.end()), a.end());
    size_t s = 0;
    for (size_t i = 1; i <= a.size(); ++i)
        if (i == a.size() || a[i] - a[i - 1] > max_gap) {
            const long long bytes = (a[i - 1] - a[s] + 1) * 4;
            CHECK(bytes >= min_bytes, "%s: a run of %lld bytes at parameter %lld", what, bytes, a[s]);
            s = i;
        }
}

static void check(const Case& cs) {
    const char* name = cs.name;
    const PackDesc& d = cs.d;
    const int vpr = d.Kpad / 8, nb = pg_blocks(d);
    const long long elems = (long long)d.Npad * d.Kpad;
    std::vector<long long> got(elems, UNSET);
    std::vector<int> writes(elems / 8, 0);
    const PackRuns g = pg_runs(d);
    CHECK((g.ok != 0) == cs.expect_runs, "run assignment %d, expected %d", g.ok, (int)cs.expect_runs);
    auto read = [&](long long idx, bool bias) {
        const long long lo = bias ? cs.b_lo : cs.p_lo, hi = bias ? cs.b_hi : cs.p_hi;
        CHECK(idx >= lo && idx < hi, "read of parameter %lld outside [%lld, %lld)", idx, lo, hi);
        return idx;
    };
    auto store = [&](int n, int kv, const long long (&val)[8]) {
        CHECK(n >= 0 && n < d.Npad && kv >= 0 && kv < vpr, "vector (%d, %d) outside the matrix", n, kv);
        const long long e = pack_dst(d, n, kv);
        CHECK(e >= 0 && e + 8 <= elems && e % 8 == 0, "destination %lld outside the matrix", e);
        if (e < 0 || e + 8 > elems) return;
        ++writes[e / 8];
        // a fragment-major destination holds the same (n, k) elements in another order: file them under their (n, k)
        for (int j = 0; j < 8; ++j) got[(long long)n * d.Kpad + kv * 8 + j] = val[j];
        if (!d.frag) CHECK(e == (long long)n * d.Kpad + kv * 8, "row-major destination");
        else {
            const long long lane = 16 * (kv % 4) + n % 16, want = (((long long)(n / 16) * (d.Kpad / 32) + kv / 4) * 64 + lane) * 8;
            CHECK(e == want, "fragment-major destination %lld, expected %lld", e, want);
        }
    };
    const bool parity = d.step_t != 1;
    for (int lb = 0; lb < nb; ++lb) {
        if (g.ok) {
            for (int wave = 0; wave < PG_WAVES; ++wave)
                for (int task = pg_first_task(lb, wave); task < g.tasks; task += pg_task_step(nb)) {
                    std::vector<long long> addr[8];
                    for (int lane = 0; lane < PG_WAVE; ++lane) {
                        int n, tap, co;
                        if (!pg_runs_decode(g, task, lane, n, tap, co)) continue;
                        CHECK(n >= 0 && n < d.N && tap >= 0 && tap < g.T && co >= 0 && co < g.CO, "lane owns (%d, %d, %d)", n, tap, co);
                        const long long b = pack_src(d, n, tap * d.C + co * 8);
                        long long val[8];
                        for (int j = 0; j < 8; ++j) { val[j] = read(b + (long long)j * d.s_c, false); addr[j].push_back(val[j]); }
                        store(n, tap * g.CO + co, val);
                    }
                    for (int j = 0; j < 8; ++j) runs_of(addr[j], parity ? 15 : 1, name, "load instruction", 64);
                }
            for (int t = 0; t < PG_TPB; ++t)
                for (int i = lb * PG_TPB + t; i < g.zeros; i += nb * PG_TPB) {
                    int n, kv;
                    pg_zero_decode(d, g, i, n, kv);
                    const long long z[8] = {ZERO, ZERO, ZERO, ZERO, ZERO, ZERO, ZERO, ZERO};
                    store(n, kv, z);
                }
        } else {
            // the row-major assignment: thread t of block lb owns vector lb * 256 + t
            for (int wave = 0; wave < PG_WAVES; ++wave) {
                std::vector<long long> addr;
                for (int lane = 0; lane < PG_WAVE; ++lane) {
                    const int v = lb * PG_TPB + wave * PG_WAVE + lane;
                    if (v >= d.Npad * vpr) continue;
                    const int n = v / vpr, kv = v % vpr;
                    long long val[8];
                    for (int j = 0; j < 8; ++j) {
                        const int k = kv * 8 + j;
                        val[j] = ZERO;
                        if (n < d.N && k < d.K) { val[j] = read(pack_src(d, n, k), false); addr.push_back(val[j]); }
                        else if (n < d.N && k == d.K && d.bias_off >= 0) val[j] = read(pack_bias_src(d, n), true);
                    }
                    store(n, kv, val);
                }
                const long long row = (long long)d.K * 4;
                runs_of(addr, 1, name, "the 8 loads of a wave", row < 64 ? row : 64);
            }
        }
    }
    long long bad_w = 0, bad_v = 0;
    for (long long v = 0; v < elems / 8; ++v) bad_w += writes[v] != 1;
    CHECK(bad_w == 0, "%lld vectors not written exactly once", bad_w);
    for (int n = 0; n < d.Npad; ++n)
        for (int k = 0; k < d.Kpad; ++k) {
            long long want = ZERO;
            if (n < d.N && k < d.K) want = ref_src(d, n, k);
            else if (n < d.N && k == d.K && d.bias_off >= 0) want = d.bias_off + (long long)(n / d.NL) * d.b_nhi + (long long)(n % d.NL) * d.b_nlo;
            bad_v += got[(long long)n * d.Kpad + k] != want;
        }
    CHECK(bad_v == 0, "%lld elements hold another parameter than the original formula names (or a pad is not zero)", bad_v);
    std::printf("%-44s %s  blocks %4d  tasks %5d  unit %2d x %2d lanes  zero vectors %d\n", name, g.ok ? "runs     " : "row-major", nb, g.tasks,
                g.G, g.E, g.zeros);
}

int main() {
    std::vector<Case> cases;
    const long long base = 1000;        // the tensors do not start at parameter 0
    {   // Conv2d(32, 64, 4, 2, 1), weight (64, 32, 4, 4): forward form, row n = output channel, k = tap * 32 + input channel
        const int Cout = 64, Cin = 32, kk = 16;
        cases.push_back({"conv2d 32->64 k4 forward", conv(base, Cout, Cin, 4, 4, 64, Cin * kk, kk, 4, 0, 0, 1), base, base + Cout * Cin * kk, true, 0, 0});
        // its data gradient: rows = input channels, one descriptor per stride-parity class (2 x 2 of the 4 x 4 taps each)
        static const char* nm[4] = {"conv2d 32->64 k4 dgrad class 0", "conv2d 32->64 k4 dgrad class 1", "conv2d 32->64 k4 dgrad class 2", "conv2d 32->64 k4 dgrad class 3"};
        for (int ci = 0; ci < 4; ++ci) {
            const int ph = ci / 2, pw = ci % 2;
            cases.push_back({nm[ci], conv(base, Cin, Cout, 2, 2, 32, kk, Cin * kk, 4, (ph + 1) % 2, (pw + 1) % 2, 2), base, base + Cout * Cin * kk, true, 0, 0});
        }
        // fragment-major copy of a forward form: Conv2d(64, 128, 4, 2, 1)
        PackDesc f = conv(base, 128, 64, 4, 4, 128, 64 * kk, kk, 4, 0, 0, 1);
        f.frag = 1;
        cases.push_back({"conv2d 64->128 k4 forward, fragment-major", f, base, base + 128 * 64 * kk, true, 0, 0});
    }
    {   // ConvTranspose2d(64, 32, 5, 2, 2), weight (64, 32, 5, 5): forward = parity classes of 3x3, 3x2, 2x3, 2x2 taps, rows = output
        // channels; data gradient = forward form over all 25 taps, rows = input channels, K = 800 padded to 832
        const int Cin = 64, Cout = 32, kk = 25;
        static const char* nm[4] = {"convT 64->32 k5 forward class 0", "convT 64->32 k5 forward class 1", "convT 64->32 k5 forward class 2", "convT 64->32 k5 forward class 3"};
        for (int ci = 0; ci < 4; ++ci) {
            const int ph = ci / 2, pw = ci % 2, kh0 = (ph + 2) % 2, kw0 = (pw + 2) % 2;
            cases.push_back({nm[ci], conv(base, Cout, Cin, (5 - kh0 + 1) / 2, (5 - kw0 + 1) / 2, 32, kk, Cout * kk, 5, kh0, kw0, 2), base, base + Cin * Cout * kk, true, 0, 0});
        }
        cases.push_back({"convT 64->32 k5 dgrad (all taps)", conv(base, Cin, Cout, 5, 5, 64, Cout * kk, kk, 5, 0, 0, 1), base, base + Cin * Cout * kk, true, 0, 0});
    }
    {   // conv1: Conv2d(1, 32, 4, 2, 1) over im2col patches, C = 1, K = 16 padded to 64
        PackDesc d = dense(base, 32, 16, 32, 64, 16, 1);
        d.TW = 4; d.C = 1; d.s_ty = 4; d.s_tx = 1; d.s_c = 16;
        cases.push_back({"conv1 1->32 k4 (C = 1)", d, base, base + 32 * 16, false, 0, 0});
    }
    {   // upsample Linear(100, 1024) with NHWC-permuted rows (n = s * 256 + c <-> weight row c * 4 + s), bias folded into column 100, Kpad 128
        const int D = 100;
        PackDesc d = dense(base, 1024, D, 1024, 128, 0, 1);
        d.NL = 256; d.s_nhi = D; d.s_nlo = 4 * D;
        d.bias_off = 500000; d.b_nhi = 1; d.b_nlo = 4;
        cases.push_back({"linear 100->1024, bias column, Kpad > K", d, base, base + 1024 * D, false, 500000, 500000 + 1024});
        // its data gradient: the transpose, rows = the 100 latents padded to 128, k = s * 256 + c
        PackDesc t = dense(base, D, 1024, 128, 1024, 1, 0);
        t.TW = 4; t.C = 256; t.s_ty = 0; t.s_tx = D; t.s_c = 4 * D;
        cases.push_back({"linear 100->1024 transposed, Npad > N", t, base, base + 1024 * D, true, 0, 0});
        PackDesc t20 = dense(base, 20, 1024, 32, 1024, 1, 0);
        t20.TW = 4; t20.C = 256; t20.s_ty = 0; t20.s_tx = 20; t20.s_c = 80;
        cases.push_back({"linear 20->1024 transposed, Npad > N", t20, base, base + 1024 * 20, true, 0, 0});
    }
    {   // a GRU weight (600, 200) transposed into a fragment-major [208][608] operand of the row-tile kernels
        PackDesc d = dense(base, 200, 600, 208, 608, 1, 200);
        d.frag = 1;
        cases.push_back({"gru 200->600 transposed, fragment-major", d, base, base + 600 * 200, true, 0, 0});
    }
    {   // an fp32 vector destination
        PackDesc d = dense(base, 1, 100, 1, 104, 0, 1);
        d.is_f32 = 1;
        cases.push_back({"fp32 vector of 100", d, base, base + 100, false, 0, 0});
    }
    for (const Case& c : cases) check(c);
    std::printf("descriptors %zu\n", cases.size());
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
