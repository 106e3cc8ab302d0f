"""Time and accuracy of the fused MMD op (mmd.compute_mmd: mmvae_mmd, value + both gradients) against what a user could write in
torch ops, and of the InfoVAE training step with either MMD term.

    python tools/mmd_bench.py [--shapes 128,128,20 128,128,100 1024,1024,100 10000,10000,100] [--reps 9] [--out profiles/mmd_bench.txt]

Per shape (n_x, n_y, D), x ~ N(0, 1), y ~ 1.5 N(0, 1) + 0.3 on the device, each arm computes MMD and its gradient in x and in y:
  * fused     ``compute_mmd(x, y).backward()``: two launches, plus the multiply by the upstream scalar;
  * verbatim  the reference's formulation (coco/model.py:385-402: three expanded (n, m, D) tensors) with autograd, where those
              tensors and what autograd keeps of them fit in ``--verbatim_gb`` (default 24 GB);
  * cdist     the same quantity through ``torch.cdist`` over blocks of rows, ``exp(-d^2 / D^2)``, autograd.
Method: every arm is warmed up, then the arms are timed in turn ``--reps`` times (A, B, C, A, B, C, ...), each timing a device-event
pair around ``--inner`` calls; the median, the fastest and the slowest per call are reported.  The accuracy section is the error
of the op against float64 next to the error of the fp32 formulation on the CPU (the yardstick of tests/test_gpu_mmd.py).
The InfoVAE step is forward + loss + backward + Adam at B = 128, D = 100 (coco/train_infovae.py's defaults) on one fixed batch.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner                            # ms per call


def interleaved(arms, reps, inner):
    """arms: {name: fn} -> {name: (median, fastest, slowest) ms per call}, the arms timed in turn"""
    for fn in arms.values():
        fn(); fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            t[k].append(timed(fn, inner))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def formulation_kernel(x, y):
    n, m, D = x.shape[0], y.shape[0], x.shape[1]
    return torch.exp(-torch.mean(torch.pow(x.unsqueeze(1).expand(n, m, D) - y.unsqueeze(0).expand(n, m, D), 2), dim=2) / D)


def formulation_mmd(x, y):
    return formulation_kernel(x, x).mean() + formulation_kernel(y, y).mean() - 2 * formulation_kernel(x, y).mean()


def cdist_mmd(x, y, block_elems=1 << 24):
    D = x.shape[1]

    def kmean(a, b):
        rows = max(1, block_elems // b.shape[0])
        total = 0
        for i in range(0, a.shape[0], rows):
            d = torch.cdist(a[i:i + rows], b)
            total = total + torch.exp(-(d * d) / (D * D)).sum()
        return total / (a.shape[0] * b.shape[0])
    return kmean(x, x) + kmean(y, y) - 2 * kmean(x, y)


def fmt(t):
    return "%10.4f ms (fastest %.4f, slowest %.4f)" % t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, nargs="+", default=["128,128,20", "128,128,100", "1024,1024,100", "10000,10000,100"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--verbatim_gb", type=float, default=24.0)
    ap.add_argument("--accuracy", type=str, nargs="*", default=["128,128,100", "131,67,256", "2051,4099,100"])
    ap.add_argument("--no_step", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mmd_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mmd_bench: no GPU (times are only measured on the device)")
    from multimodal_vae_amd import coco as K, mmd
    from multimodal_vae_amd._lib import call
    dev = torch.device("cuda:0")
    lines = ["mmd_bench: %s, torch %s; geometry (row tile, column tile, max D) = %s; %d interleaved repetitions per arm, medians" %
             (torch.cuda.get_device_name(0), torch.__version__, mmd.mmd_geometry(), args.reps),
             "this tool ran alone in its process and started nothing else; the machine itself is shared",
             "value + both gradients, ms per call:"]
    print("\n".join(lines)); sys.stdout.flush()
    g = torch.Generator(device=dev).manual_seed(0)
    for shape in args.shapes:
        nx, ny, D = (int(v) for v in shape.split(","))
        x = torch.randn(nx, D, device=dev, generator=g).requires_grad_(True)
        y = (1.5 * torch.randn(ny, D, device=dev, generator=g) + 0.3).requires_grad_(True)
        res = {}
        mark = len(lines)

        def run(f, key):
            def go():
                x.grad = y.grad = None
                v = f(x, y)
                v.backward()
                res[key] = (v.detach(), x.grad, y.grad)
            return go
        arms = {"fused": run(mmd.compute_mmd, "fused")}
        pairs = float(nx + ny) ** 2 * D
        # the verbatim arm holds (a - b) and its square per kernel for the backward: ~2 tensors of 4 bytes per expanded element
        if pairs * 4 * 2.5 <= args.verbatim_gb * 1e9:
            arms["verbatim"] = run(formulation_mmd, "verbatim")
        arms["cdist"] = run(cdist_mmd, "cdist")
        inner = 20 if pairs < 1e9 else 2
        t = interleaved(arms, args.reps, inner)
        lines.append("(%d, %d, %d): workspace %.2f MB" % (nx, ny, D, call("mmvae_mmd_workspace_bytes", nx, ny, D) / 1e6))
        lines.append("  fused    compute_mmd + backward      %s   %.1f G pairs/s" % (fmt(t["fused"]), float(nx + ny) ** 2 / t["fused"][0] / 1e6))
        for k, label in (("verbatim", "reference formulation, autograd"), ("cdist", "torch.cdist blocks, autograd  ")):
            if k in t:
                rel = abs(float(res[k][0]) - float(res["fused"][0]))
                gd = float((res[k][1] - res["fused"][1]).abs().max() / res["fused"][1].abs().max())
                lines.append("  %-8s %s  %s   %.2fx the fused time%s   |MMD - fused| %.1e, dx max dev %.1e" %
                             (k, label, fmt(t[k]), t[k][0] / t["fused"][0], "" if t[k][0] >= t["fused"][0] else " (THE FUSED OP IS SLOWER)",
                              rel, gd))
            else:
                lines.append("  %-8s %s  does not fit: %.0f GB per expanded tensor" % (k, label, float(max(nx, ny)) ** 2 * D * 4 / 1e9))
        tv = interleaved({"value": lambda: mmd.mmd_terms(x.detach(), y.detach())}, args.reps, inner)
        lines.append("  fused    mmd_terms (value alone)     %s" % fmt(tv["value"]))
        for l in lines[mark:]:
            print(l)
        sys.stdout.flush()
        del x, y, res
        torch.cuda.empty_cache()

    if args.accuracy:
        import mmd_ref as R
        lines.append("accuracy against float64: error of the op / error of the fp32 formulation on the CPU (the tests' gate is 4x the latter)")
        for shape in args.accuracy:
            nx, ny, D = (int(v) for v in shape.split(","))
            c = R.real_case(nx, ny, D)
            xd, yd = c["x"].to(dev).requires_grad_(True), c["y"].to(dev).requires_grad_(True)
            mmd.compute_mmd(xd, yd).backward()
            terms = mmd.mmd_terms(xd.detach(), yd.detach())
            lines.append("  (%d, %d, %d): value %.2e / %.2e   dx %.2e / %.2e   dy %.2e / %.2e" %
                         (nx, ny, D, R.value_error(terms, c["ref"]["terms"]), c["yardstick"]["value"],
                          R.grad_error(xd.grad, c["ref"]["dx"]), c["yardstick"]["dx"], R.grad_error(yd.grad, c["ref"]["dy"]), c["yardstick"]["dy"]))
            print(lines[-1]); sys.stdout.flush()

    if not args.no_step:
        B, D = 128, 100
        torch.manual_seed(0)
        vae = K.InfoVAE(n_latents=D).cuda().train()
        opt = torch.optim.Adam(vae.parameters(), lr=1e-4)
        img = torch.rand(B, 3, 32, 32, device=dev, generator=g)
        from multimodal_vae_amd.modules import _BCEMeanFn

        def step(mmd_fn):
            def go():
                opt.zero_grad()
                recon, z = vae(img)
                true_samples = torch.randn(B, D, device=dev)
                loss = _BCEMeanFn.apply(recon.reshape(B, -1), img.reshape(B, -1)) + mmd_fn(true_samples, z)
                loss.backward()
                opt.step()
            return go
        t = interleaved({"fused": step(mmd.compute_mmd), "verbatim": step(formulation_mmd)}, args.reps, 10)
        lines += ["InfoVAE training step, B = %d, D = %d (forward, loss, backward, torch.optim.Adam), ms per step:" % (B, D),
                  "  MMD term on the fused op              %s" % fmt(t["fused"]),
                  "  MMD term as the reference formulation %s   %.2fx" % (fmt(t["verbatim"]), t["verbatim"][0] / t["fused"][0])]
        print("\n".join(lines[-3:]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
