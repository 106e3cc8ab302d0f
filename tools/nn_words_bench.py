"""Rate of the nearest-word search (coco.WordTable.nearest: mmvae_nn_words_nearest) against a chunked torch.mm + argmin.

    python tools/nn_words_bench.py [--words 2196017] [--queries 102 6528] [--reps 5] [--chunk 65536] [--out profiles/nn_words_bench.txt]

For every query count N (default: 102 = one caption, 6528 = a batch of 64 captions) against V synthetic words (default: the
size of GloVe-840B), device events around ``--reps`` calls after a warm-up call (the method of tools/loglik_bench.py):
  * the fused call: one sweep of the table on the f32-input MFMA + merge; time per call, queries/s, achieved TFLOP/s of
    2 * 300 * N * V, its fraction of the 155 TFLOP/s fp32 matrix peak, and the table bytes / time (a floor: one pass);
  * the baseline a user could write without it: per vocabulary slice of ``--chunk`` words, ``torch.addmm(sqnorm, Q, W^T, alpha=-2)``
    and ``min(dim=1)``, the slice winners merged with ``torch.where`` (strict <, so the lower slice wins ties);
  * the ratio, and how many of the N winners the two agree on (they may differ on near-ties: another summation order).
Also the one-off cost of the table: mmvae_nn_words_norms.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = 155.0


def ev_time(fn, reps):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--words", type=int, default=2196017)
    ap.add_argument("--queries", type=int, nargs="+", default=[102, 6528])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "nn_words_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nn_words_bench: no GPU (the rates are only measured on the device)")
    from multimodal_vae_amd import coco as K
    from multimodal_vae_amd._lib import call, ptr
    dev = torch.device("cuda:0")
    V = args.words
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(V, 300, device=dev, generator=g).mul_(0.4)
    tab = K.WordTable.__new__(K.WordTable)                        # the table is generated on the device: no host copy to validate
    tab.itos, tab.stoi, tab.device, tab.vectors = range(V), {}, dev, W
    tab.sqnorm = torch.empty(V, dtype=torch.float32, device=dev)

    def norms():
        call("mmvae_nn_words_norms", ptr(W), V, 300, ptr(tab.sqnorm), None)
    t_norms = ev_time(norms, args.reps)
    lines = ["nn_words_bench: V = %d words x 300 fp32 (%.2f GB), %s, torch %s" %
             (V, V * 1200 / 1e9, torch.cuda.get_device_name(0), torch.__version__),
             "geometry (query tile, word tile, max splits) = %s" % (K.nn_words_geometry(),),
             "mmvae_nn_words_norms          %8.3f ms  (%.2f TB/s)" % (t_norms * 1e3, V * 1200 / t_norms / 1e12)]
    print(lines[-1]); sys.stdout.flush()
    sq = tab.sqnorm

    for N in args.queries:
        Q = torch.randn(N, 300, device=dev, generator=g).mul_(0.4)
        Q[: N // 2] = W[torch.randint(0, V, (N // 2,), device=dev, generator=g)] + 0.05 * torch.randn(N // 2, 300, device=dev, generator=g)
        flop = 2.0 * 300 * N * V
        res = {}

        def fused():
            res["fused"] = tab.nearest(Q)[0]

        def baseline():
            best = torch.full((N,), float("inf"), device=dev)
            arg = torch.zeros(N, dtype=torch.int64, device=dev)
            for v0 in range(0, V, args.chunk):
                s = torch.addmm(sq[v0:v0 + args.chunk], Q, W[v0:v0 + args.chunk].t(), alpha=-2.0)
                m = s.min(dim=1)
                better = m.values < best
                best = torch.where(better, m.values, best)
                arg = torch.where(better, m.indices + v0, arg)
            res["base"] = arg
        t_f = ev_time(fused, args.reps)
        t_b = ev_time(baseline, args.reps)
        agree = int((res["fused"] == res["base"]).sum())
        lines += ["N = %d queries (%.2f TFLOP per call), workspace %.2f MB" %
                  (N, flop / 1e12, call("mmvae_nn_words_workspace_bytes", N, V) / 1e6),
                  "  fused   mmvae_nn_words_nearest   %9.3f ms per call  %12.0f queries/s  %6.1f TFLOP/s = %4.1f %% of the %.0f TFLOP/s fp32 "
                  "matrix peak  (table pass alone: %.2f TB/s)" % (t_f * 1e3, N / t_f, flop / t_f / 1e12, 100 * flop / t_f / 1e12 / PEAK_TF,
                                                                  PEAK_TF, V * 1200 / t_f / 1e12),
                  "  baseline torch.addmm + min, slices of %d words  %9.3f ms per call  %12.0f queries/s  %6.1f TFLOP/s" %
                  (args.chunk, t_b * 1e3, N / t_b, flop / t_b / 1e12),
                  "  ratio baseline / fused  %.2fx  %s   same winner for %d of %d queries" %
                  (t_b / t_f, "" if t_f <= t_b else "(THE FUSED CALL IS SLOWER)", agree, N)]
        for l in lines[-4:]:
            print(l)
        sys.stdout.flush()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
