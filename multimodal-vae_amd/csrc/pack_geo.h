// Geometry of the weight pack (elementwise.hip pack_block / pack_kernel / step_begin_kernel): the descriptor, the source and
// destination index of every packed element, and the assignment of destination vectors to lanes.  Plain C++17: the kernel and
// tests/host/pack_geo_check.cpp call the same functions.
//
// A packed matrix is [Npad][Kpad] bf16 (or fp32), written as 16-byte vectors of 8 consecutive columns; column k = tap * C + c.
// The old assignment (PackRuns::ok == 0, knob pack_runs = 0) gives thread t of a block the vector v = 256 * block + t in row-major
// (n, k / 8) order and lets it gather its 8 channels at stride s_c: for a conv weight every one of a wave's 64 x 8 loads is 4 bytes
// of a different cache line.  The run assignment keeps the set of vectors and their contents and changes only who owns which:
// the vectors with k < K are the grid (tap, n, c / 8); its three axes are ordered by their SOURCE stride, the lanes of a wave walk
// the axis with the smallest one, and a wave always takes whole extents of it ("units"), so that each of its 8 load instructions
// reads runs that are as long as the source allows:
//   Conv2d forward / ConvTranspose2d data-gradient form  (taps contiguous, 64 B for 4x4, 100 B for 5x5):   tap, c / 8, n
//   stride-parity classes (Conv2d data gradient, ConvTranspose2d forward: the class's taps of consecutive n):   tap, n, c / 8
//   transposed Linear (n contiguous):   n, tap, c / 8
// The 16-byte stores of the lanes that share a tap and differ in c / 8 are neighbours in the packed row, as before.
// An axis longer than a wave is cut into equal segments of at most 64 lanes.  The vectors of the pad columns (k >= K) and pad rows
// (n >= N) are zero; the threads of the descriptor's blocks share them in a second loop.
#pragma once

#if defined(__HIPCC__)
#define PG_HD __host__ __device__ inline
#else
#define PG_HD inline
#endif

struct PackDesc {
    long long dst_off;      // element offset in the packed buffer (bf16 units for matrices, float units for vectors)
    long long src_off;      // element offset in the flat fp32 parameter buffer
    int Npad, Kpad, N, K;   // packed matrix [Npad][Kpad]; entries outside [N][K] are zero
    int NL;                 // row n = n_hi*NL + n_lo
    int s_nhi, s_nlo;       // source strides of n_hi / n_lo
    int TW, C;              // column k = (ty*TW + tx)*C + c
    int s_ty, s_tx, s_c;    // source strides
    int o_ty, o_tx, step_t; // kernel index = o + t*step
    int is_f32;             // destination is fp32
    long long bias_off;     // >= 0: column K of every row holds a bias folded into the GEMM (operand column K == 1.0)
    int b_nhi, b_nlo;       // source strides of that bias vector
    int first_block;        // prefix sum of 256-thread blocks over the table
    int part;               // gradient descriptors: 1 = complete early in the step (decoders), 0 = with the encoders' backward;
                            // weight descriptors: the stage of the step that refreshes the copy (step_begin_with_pack), 0 = the prologue
    int frag;               // 1: MFMA-fragment-major destination -- 16-row tile nt, 32-column k-step ks: the 64 lanes' 8-element
                            // vectors (lane = 16*(k/8 % 4) + n % 16) are one contiguous 1 KB block at ((nt*(Kpad/32) + ks)*64 + lane)*8
};

constexpr int PG_TPB = 256, PG_WAVE = 64, PG_WAVES = PG_TPB / PG_WAVE;

// q = r / d, rem = r % d for 0 <= r < 2^23, 0 < d < 2^23 (float reciprocal, one correction step each way)
PG_HD int pg_divmod(int r, int d, int& rem) {
    int q = (int)((float)r * (1.0f / (float)d));
    rem = r - q * d;
    if (rem < 0) { --q; rem += d; }
    else if (rem >= d) { ++q; rem -= d; }
    return q;
}

PG_HD long long pg_vectors(const PackDesc& d) { return (long long)d.Npad * (d.Kpad / 8); }
PG_HD int pg_blocks(const PackDesc& d) { return (int)((pg_vectors(d) + PG_TPB - 1) / PG_TPB); }

// flat parameter index of packed element (n, k), k < K
PG_HD long long pack_src(const PackDesc& d, int n, int k) {
    int nhi = n / d.NL, nlo = n - nhi * d.NL;
    int tap = k / d.C, c = k - tap * d.C;
    int ty = tap / d.TW, tx = tap - ty * d.TW;
    return d.src_off + (long long)nhi * d.s_nhi + (long long)nlo * d.s_nlo +
           (long long)(d.o_ty + ty * d.step_t) * d.s_ty + (long long)(d.o_tx + tx * d.step_t) * d.s_tx + (long long)c * d.s_c;
}
// flat parameter index of the bias folded into column K of row n (bias_off >= 0)
PG_HD long long pack_bias_src(const PackDesc& d, int n) {
    int nhi = n / d.NL, nlo = n - nhi * d.NL;
    return d.bias_off + (long long)nhi * d.b_nhi + (long long)nlo * d.b_nlo;
}
// element offset (from dst_off) of the 8-column vector kv of row n
PG_HD long long pack_dst(const PackDesc& d, int n, int kv) {
    return d.frag ? ((long long)((n >> 4) * (d.Kpad >> 5) + (kv >> 2)) * 64 + (kv & 3) * 16 + (n & 15)) * 8 : (long long)n * d.Kpad + kv * 8;
}

enum { PG_TAP = 0, PG_N = 1, PG_CO = 2 };
struct PackRuns {
    int ok;                 // 0: the descriptor keeps the row-major assignment
    int T, CO;              // taps, channel octets: the vectors kv < T * CO of a row hold k < K
    int ax[3], ext[3];      // the axes (PG_TAP / PG_N / PG_CO) by ascending source stride, and their extents
                            // (rows: N, the pad rows are not part of the grid)
    int E, G, segs;         // a unit = E lanes along ax[0] (the extent, or one of `segs` equal segments of it); a wave takes G units at once
    int units, tasks;       // units = segs * ext[1] * ext[2]; tasks = wave-sized groups of G consecutive units
    int vpr, padv;          // vectors per packed row; zero vectors behind the K columns of a row
    int zrows, zeros;       // zero vectors: the zrows = (Npad - N) * vpr of the pad rows, then padv per row n < N
};

// |stride| as a sort key; an axis that does not move in the source goes last
PG_HD long long pg_stride_mag(long long s) { return s < 0 ? -s : (s == 0 ? (1ll << 40) : s); }

PG_HD PackRuns pg_runs(const PackDesc& d) {
    PackRuns r{};
    if (d.s_c == 1 || d.C < 8 || d.C % 8 != 0 || d.bias_off >= 0 || d.is_f32 || d.K <= 0 || d.K % d.C != 0 || d.TW < 1 || d.N < 1 || d.N > d.Npad) return r;
    r.T = d.K / d.C; r.CO = d.C / 8;
    if (r.T % d.TW != 0 || r.T > PG_WAVE) return r;
    const long long huge = 1ll << 40;
    long long st[3];
    st[PG_TAP] = r.T > 1 ? pg_stride_mag((long long)(d.TW > 1 ? d.s_tx : d.s_ty) * d.step_t) : huge;
    st[PG_N] = d.N > 1 ? pg_stride_mag(d.NL > 1 ? d.s_nlo : d.s_nhi) : huge;
    st[PG_CO] = r.CO > 1 ? pg_stride_mag(8ll * d.s_c) : huge;
    const int full[3] = {r.T, d.N, r.CO};
    int a0 = 0, a1 = 1, a2 = 2;         // three-element sort, stable
    if (st[a1] < st[a0]) { int t = a0; a0 = a1; a1 = t; }
    if (st[a2] < st[a1]) { int t = a1; a1 = a2; a2 = t; }
    if (st[a1] < st[a0]) { int t = a0; a0 = a1; a1 = t; }
    r.ax[0] = a0; r.ax[1] = a1; r.ax[2] = a2;
    for (int i = 0; i < 3; ++i) r.ext[i] = full[r.ax[i]];
    if (r.ext[0] <= PG_WAVE) { r.E = r.ext[0]; r.G = PG_WAVE / r.E; r.segs = 1; }
    else { r.segs = (r.ext[0] + PG_WAVE - 1) / PG_WAVE; r.E = (r.ext[0] + r.segs - 1) / r.segs; r.G = 1; }
    const long long units = (long long)r.segs * r.ext[1] * r.ext[2];
    if (units >= (1 << 23)) return r;
    r.units = (int)units; r.tasks = (r.units + r.G - 1) / r.G;
    r.vpr = d.Kpad / 8; r.padv = r.vpr - r.T * r.CO;
    r.zrows = (d.Npad - d.N) * r.vpr; r.zeros = r.zrows + d.N * r.padv;
    r.ok = 1;
    return r;
}

// the vector (n, tap, co) that lane `lane` of a wave owns in task `task`; false: the lane idles
PG_HD bool pg_runs_decode(const PackRuns& r, int task, int lane, int& n, int& tap, int& co) {
    int e;
    const int g = pg_divmod(lane, r.E, e);
    int u = task * r.G + g;
    if (g >= r.G || u >= r.units) return false;
    int idx[3], seg = 0;
    if (r.segs > 1) u = pg_divmod(u, r.segs, seg);
    idx[0] = seg * r.E + e;
    if (idx[0] >= r.ext[0]) return false;
    idx[2] = pg_divmod(u, r.ext[1], idx[1]);
    int out[3];
    for (int i = 0; i < 3; ++i) out[r.ax[i]] = idx[i];
    tap = out[PG_TAP]; n = out[PG_N]; co = out[PG_CO];
    return true;
}
// the i-th zero vector of the descriptor, 0 <= i < r.zeros
PG_HD void pg_zero_decode(const PackDesc& d, const PackRuns& r, int i, int& n, int& kv) {
    if (i < r.zrows) { n = d.N + pg_divmod(i, r.vpr, kv); return; }
    int p;
    n = pg_divmod(i - r.zrows, r.padv, p);
    kv = r.T * r.CO + p;
}
// the tasks of wave `wave` of the descriptor's block `lb` (of nb) are pg_first_task, + pg_task_step, ...; its threads' zero vectors
// lb * PG_TPB + thread, + nb * PG_TPB, ...
PG_HD int pg_first_task(int lb, int wave) { return lb * PG_WAVES + wave; }
PG_HD int pg_task_step(int nb) { return nb * PG_WAVES; }
