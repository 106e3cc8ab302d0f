"""Time of the exact t-SNE op (multimodal_vae_amd/tsne.py: csrc/tsne.hip) against the same algorithm in dense torch ops on the
same GPU.

    python tools/tsne_bench.py [--n 10000] [--dim 20] [--perplexity 40] [--n_iter 300] [--reps 5] [--out profiles/tsne_bench.txt]

Arms, on x (n, dim) on the device, ten unit-variance Gaussian clusters with centres ~ 4 N(0, 1):
  * joint_probabilities   the HIP op (row kernel with sklearn's search, symmetrisation, fold) / torch: ``cdist`` squared, the same
                          search for every row at once over the (n, n) matrix (one host look per step to see whether every row is
                          done), the same symmetrisation;
  * kl_grad               ONE gradient + KL: the HIP sweep and fold / torch: w from broadcast differences, two (n, n) x (n, 2)
                          products;
  * tsne                  ``--n_iter`` iterations from the same start: the HIP run (all iterations enqueued at once) / the torch
                          gradient above with the same update rule in torch ops.
Method: every arm is warmed up, then the two arms of a pair are timed in turn ``--reps`` times (A, B, A, B, ...), each timing a
device-event pair around the call (around 20 calls for ``kl_grad``, which is sub-millisecond); the median, the fastest and the
slowest are reported.  These are call times, launches and allocations included, not kernel times from a trace.  The byte bound
of the sweep is P read once (n * n * 4 bytes) at 6.29 TB/s, the copy rate measured on an MI355X; the share quoted is that time
over the call time (per iteration: the run's call time over n_iter).  The torch arms are the plain dense formulation, with
(n, n) and (n, n, 2) temporaries, not a tuned baseline, and are not bit-compatible with the op (other summation orders): the
results are compared, not equated.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12               # bytes / s, float4 copy measured on an MI355X
KL_GRAD_INNER = 20                # kl_grad calls per timed window (one call is half a millisecond)


def timed(fn, inner=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner, out


def interleaved(arms, reps, inner=1):
    """arms: {name: fn} -> ({name: (median, fastest, slowest) ms per call}, {name: last result}), the arms timed in turn, each
    timing one device-event pair around ``inner`` calls"""
    out = {}
    for k, fn in arms.items():
        out[k] = fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            ms, out[k] = timed(fn, inner)
            t[k].append(ms)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}, out


def fmt(t):
    return "%10.3f ms (fastest %.3f, slowest %.3f)" % t


# ------------------------------------------------------------------------------------------------------ the torch-ops baseline
def torch_joint_probabilities(x, perplexity):
    n = x.shape[0]
    d = torch.cdist(x, x).pow_(2)
    eye = torch.eye(n, dtype=torch.bool, device=x.device)
    d = d - d.masked_fill(eye, float("inf")).min(1, keepdim=True)[0]
    d.masked_fill_(eye, float("inf"))                              # exp(-beta inf) = 0: the diagonal drops out of every sum
    log_perp = float(torch.log(torch.tensor(float(perplexity))))
    beta = torch.ones(n, 1, device=x.device)
    bmin, bmax = torch.full_like(beta, -float("inf")), torch.full_like(beta, float("inf"))
    done = torch.zeros(n, 1, dtype=torch.bool, device=x.device)
    for _ in range(100):
        p = torch.exp(-beta * d)
        sp = p.sum(1, keepdim=True)
        h = torch.log(sp) + beta * torch.nan_to_num(d * p, nan=0.0, posinf=0.0).sum(1, keepdim=True) / sp
        diff = h - log_perp
        done |= diff.abs() <= 1e-5
        if bool(done.all()):
            break
        up, dn = ~done & (diff > 0), ~done & ~(diff > 0)
        bmin = torch.where(up, beta, bmin)
        bmax = torch.where(dn, beta, bmax)
        nb = torch.where(up, torch.where(torch.isinf(bmax), beta * 2, (beta + bmax) / 2),
                         torch.where(torch.isinf(bmin), beta / 2, (beta + bmin) / 2))
        beta = torch.where(done, beta, nb)
    p = torch.exp(-beta * d)
    p = p / p.sum(1, keepdim=True)
    P = ((p + p.t()) / (2.0 * n)).clamp_min_(1e-12).masked_fill_(eye, 0.0)
    return P, beta.squeeze(1)


def torch_kl_grad(P, y, exaggeration=1.0, plogp=None):
    n = y.shape[0]
    diff = y.unsqueeze(1) - y.unsqueeze(0)
    w = 1.0 / (1.0 + (diff * diff).sum(2))
    Z = w.sum(dtype=torch.float64) - n
    pw = P * w
    attr = pw.sum(1, keepdim=True) * y - pw @ y
    w2 = w * w
    rep = w2.sum(1, keepdim=True) * y - w2 @ y
    grad = 4.0 * (exaggeration * attr - rep / Z.float())
    if plogp is None:
        plogp = torch.xlogy(P, P).sum(dtype=torch.float64)
    kl = plogp - (P * torch.log(w)).sum(dtype=torch.float64) + torch.log(Z)
    return kl.float(), grad


def torch_tsne(P, y0, n_iter, learning_rate, early_exaggeration, exaggeration_iters):
    y, update, gains = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)
    plogp = torch.xlogy(P, P).sum(dtype=torch.float64)
    trace = []
    for k in range(n_iter):
        early = k < exaggeration_iters
        kl, grad = torch_kl_grad(P, y, early_exaggeration if early else 1.0, plogp)
        trace.append(kl)
        gains = torch.where(update * grad < 0, gains + 0.2, gains * 0.8).clamp_min_(0.01)
        update = (0.5 if early else 0.8) * update - learning_rate * gains * grad
        y = y + update
    return y, torch.stack(trace)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=20)
    ap.add_argument("--perplexity", type=float, default=40.0)
    ap.add_argument("--n_iter", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "tsne_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tsne_bench: no GPU (times are only measured on the device)")
    from multimodal_vae_amd import tsne as T
    from multimodal_vae_amd._lib import call
    dev = torch.device("cuda:0")
    n, dim = args.n, args.dim
    lines = ["tsne_bench: %s, torch %s; geometry (row tile, column tile, symmetrisation tile, row threads, max D) = %s; %d interleaved "
             "repetitions per arm, medians" % (torch.cuda.get_device_name(0), torch.__version__, T.tsne_geometry(), args.reps),
             "every time is a CALL time between device events (launches and allocations included), not a kernel time from a trace; the torch",
             "arms are the plain dense formulation (they materialise (n, n) and (n, n, 2) temporaries), not a tuned baseline",
             "n = %d, D = %d, perplexity %g: P is %.0f MB, workspace %.2f MB" % (n, dim, args.perplexity, n * n * 4 / 1e6,
                                                                             call("mmvae_tsne_workspace_bytes", n) / 1e6)]
    print("\n".join(lines)); sys.stdout.flush()

    def emit(*ls):
        lines.extend(ls)
        print("\n".join(ls)); sys.stdout.flush()

    g = torch.Generator(device=dev).manual_seed(0)                 # ten unit-variance clusters, like the latents of ten digits
    centres = 4.0 * torch.randn(10, dim, device=dev, generator=g)
    x = (centres[torch.randint(0, 10, (n,), device=dev, generator=g)] + torch.randn(n, dim, device=dev, generator=g)).contiguous()
    t, out = interleaved({"hip": lambda: T.joint_probabilities(x, args.perplexity),
                          "torch": lambda: torch_joint_probabilities(x, args.perplexity)}, args.reps)
    P, beta = out["hip"]
    Pt, beta_t = out["torch"]
    emit("joint_probabilities:",
         "  hip    %s" % fmt(t["hip"]),
         "  torch  %s   %.2fx the hip time%s" % (fmt(t["torch"]), t["torch"][0] / t["hip"][0], "" if t["torch"][0] >= t["hip"][0] else " (THE HIP OP IS SLOWER)"),
         "  max |P - P_torch| / max P %.1e, max |beta - beta_torch| / beta %.1e, sum P %.7f" %
         (float((P - Pt).abs().max() / P.max()), float(((beta - beta_t).abs() / beta).max()), float(P.sum(dtype=torch.float64))))
    del Pt, out
    torch.cuda.empty_cache()

    bound_ms = n * n * 4 / COPY_RATE * 1e3
    for scale in (1e-4, 10.0):
        y = T.initial_embedding(n, 0).to(dev) * (scale / 1e-4)
        t, out = interleaved({"hip": lambda: T.kl_grad(P, y, 12.0), "torch": lambda: torch_kl_grad(P, y, 12.0)}, args.reps, KL_GRAD_INNER)
        (kl, g), (klt, gt) = out["hip"], out["torch"]
        emit("kl_grad, y at scale %g (per call of %d in one timed window: the sweep with P log P, the fold, two allocations):" % (scale, KL_GRAD_INNER),
             "  hip    %s   %.1f G pairs/s; P read once takes %.3f ms: %.0f %% of the call" % (fmt(t["hip"]), n * n / t["hip"][0] / 1e6, bound_ms, 100 * bound_ms / t["hip"][0]),
             "  torch  %s   %.2fx the hip time%s" % (fmt(t["torch"]), t["torch"][0] / t["hip"][0], "" if t["torch"][0] >= t["hip"][0] else " (THE HIP OP IS SLOWER)"),
             "  |KL - KL_torch| %.1e, max |grad - grad_torch| / max |grad| %.1e" % (abs(float(kl) - float(klt)), float((g - gt).abs().max() / g.abs().max())))
        del out
        torch.cuda.empty_cache()

    y0 = T.initial_embedding(n, 0).to(dev)

    from multimodal_vae_amd._lib import ptr
    from multimodal_vae_amd._ops import stream as _stream
    ws = torch.empty(call("mmvae_tsne_workspace_bytes", n), dtype=torch.uint8, device=dev)

    def hip_run(n_iter=args.n_iter):
        yy, up, ga = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)
        trace = torch.empty(n_iter, device=dev)
        call("mmvae_tsne_run", ptr(P), n, ptr(yy), ptr(up), ptr(ga), 0, n_iter, 200.0, 12.0, 250, ptr(trace), ptr(ws), ws.numel(), _stream())
        return yy, trace
    y10, y10t = hip_run(10)[0], torch_tsne(P, y0, 10, 200.0, 12.0, 250)[0]
    dev10 = float((y10 - y10t).abs().max() / y10t.abs().max())
    t, out = interleaved({"hip": hip_run, "torch": lambda: torch_tsne(P, y0, args.n_iter, 200.0, 12.0, 250)}, max(3, args.reps // 2 + 1))
    (yh, th), (yt, tt) = out["hip"], out["torch"]
    per = t["hip"][0] / args.n_iter
    emit("%d iterations from one start (P given; learning rate 200, exaggeration 12 for 250 iterations):" % args.n_iter,
         "  hip    %s   %.4f ms per iteration (the call over %d: two launches each); P read once takes %.3f ms: %.0f %% of it" %
         (fmt(t["hip"]), per, args.n_iter, bound_ms, 100 * bound_ms / per),
         "  torch  %s   %.2fx the hip time%s" % (fmt(t["torch"]), t["torch"][0] / t["hip"][0], "" if t["torch"][0] >= t["hip"][0] else " (THE HIP OP IS SLOWER)"),
         "  KL first / last: hip %.4f / %.4f, torch %.4f / %.4f; embedding spread (std of y): hip %.3g, torch %.3g" %
         (float(th[0]), float(th[-1]), float(tt[0]), float(tt[-1]), float(yh.std()), float(yt.std())),
         "  after 10 iterations max |y - y_torch| / max |y_torch| = %.1e (the trajectories are chaotic: later states are not comparable point by point)" % dev10)
    t, _ = interleaved({"tsne": lambda: T.tsne(x, perplexity=args.perplexity, n_iter=args.n_iter)}, 3)
    emit("tsne(x) end to end (joint_probabilities + %d iterations): %s" % (args.n_iter, fmt(t["tsne"])))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
