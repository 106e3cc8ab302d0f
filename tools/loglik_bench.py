"""Rate of the importance-sampled evaluation (evaluate.iw_estimate / marginal_table) against a compute_nll-style loop.

    python tools/loglik_bench.py [--batch 64] [--particles 1000] [--loop_particles 100] [--batches 4] [--table_examples 10000]

Prints, at batch B:
  * particles/s of iw_estimate at K = --particles (whole batches, device-synchronised wall clock after a warm-up batch);
  * particles/s of the loop that evaluate.compute_nll runs (one image-decoder and one text-decoder module call per particle
    index, host BCE / NLL sums read back with float()), timed over a few batches at K = --loop_particles;
  * the ratio of the two rates;
  * the wall time of marginal_table (3 posteriors) on --table_examples synthetic examples at K = --particles;
  * the image decoder's algorithmic FLOPs per particle from the layer hooks (mmvae_mm_layer_algo_flops) and the achieved
    TFLOP/s of that count over the iw_estimate wall time (the text decoder and the rest of the chunk are inside the time, not
    in the count).
The model is the oracle's formula initialisation in eval mode; the data are synthetic MultiMNIST-shaped examples.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--particles", type=int, default=1000)
    ap.add_argument("--loop_particles", type=int, default=100)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--table_examples", type=int, default=10000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loglik_bench: no GPU (the rates are only measured on the device)")
    from multimodal_vae_amd import multimnist as M, data as Dd
    from multimodal_vae_amd._lib import call
    from multimodal_vae_amd.evaluate import iw_estimate, marginal_table, _proposal, iw_chunks, IW_ROWS
    from multimodal_vae_amd.multimnist import _BCEMeanFn, _NLLMeanFn
    from multimodal_vae_amd.utils import charlist_tensor
    from oracle import mmvae_ref as R
    dev = torch.device("cuda:0")
    D, B, K = 100, args.batch, args.particles
    vae = M.MultimodalVAE(D, use_cuda=True)
    vae.load_state_dict(R.formula_params("multimnist", D), strict=True)
    vae.cuda().eval()
    n = max(args.table_examples, B * (args.batches + 1))
    x, labels = Dd.synthetic_multimnist(n, seed=0)
    x = x.float().div_(255.0).view(-1, 1, 50, 50)
    t = torch.stack([charlist_tensor(l) for l in labels])
    batches = [(x[i:i + B].to(dev), t[i:i + B].to(dev)) for i in range(0, B * (args.batches + 1), B)]

    # ---- the new path: one iw_estimate per batch (joint posterior), batch 0 is the warm-up
    with torch.no_grad():
        props = [_proposal(vae, im, tx, "joint") for im, tx in batches]

        def run_new(i):
            return iw_estimate(vae, batches[i][0], batches[i][1], props[i][0], props[i][1], K, first_row=i * B)
        run_new(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(1, len(batches)):
            run_new(i)
        torch.cuda.synchronize()
        t_new = time.perf_counter() - t0
    rate_new = B * K * args.batches / t_new

    # ---- the compute_nll loop (evaluate.compute_nll's body at a fixed proposal), batch 0 is the warm-up
    Kl = args.loop_particles

    def run_loop(i):
        image, text = batches[i]
        mu, logvar = props[i]
        sample = torch.randn(Kl, D).cuda()
        z = sample.unsqueeze(0) * logvar.mul(0.5).exp().unsqueeze(1) + mu.unsqueeze(1)
        s = 0.0
        for k in range(Kl):
            zi = z[:, k].contiguous()
            ri = vae.decode_image(zi)
            rt = vae.decode_text(zi)
            s += float(_BCEMeanFn.apply(ri.reshape(B, -1), image.reshape(B, -1))) * image.numel()
            s += float(_NLLMeanFn.apply(rt.reshape(-1, rt.size(2)), text.reshape(-1))) * text.numel()
        return s
    with torch.no_grad():
        run_loop(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(1, len(batches)):
            run_loop(i)
        torch.cuda.synchronize()
        t_loop = time.perf_counter() - t0
    rate_loop = B * Kl * args.batches / t_loop

    # ---- FLOP count of the image decoder per particle from the layer hooks (they count 3 passes of the plan's rows)
    rows = max(nr * nk for _, nr, _, nk in iw_chunks(B, K, IW_ROWS))
    h = vae._core.state.plan(rows)
    names = ["dec_up", "dec_convT1", "dec_convT2", "dec_convT3", "dec_convT4"]
    per = {nm: call("mmvae_mm_layer_algo_flops", h, nm.encode()) / (3.0 * rows) for nm in names}
    flops_particle = sum(per.values())

    print("loglik_bench: B = %d, n_latents = %d, IW_ROWS = %d (rows per scoring call here: %d)" % (B, D, IW_ROWS, rows))
    print("iw_estimate        K = %4d  %d batches  %.3f s  %12.0f particles/s" % (K, args.batches, t_new, rate_new))
    print("compute_nll loop   K = %4d  %d batches  %.3f s  %12.0f particles/s" % (Kl, args.batches, t_loop, rate_loop))
    print("ratio              %.1fx" % (rate_new / rate_loop))
    print("image decoder algorithmic FLOPs per particle: %.2f MFLOP (%s)" %
          (flops_particle / 1e6, ", ".join("%s %.2f" % (k, v / 1e6) for k, v in per.items())))
    print("achieved           %.1f TFLOP/s (image decoder count over the iw_estimate wall time)" % (flops_particle * rate_new / 1e12))
    sys.stdout.flush()

    # ---- marginal_table on table_examples synthetic examples
    N = args.table_examples
    loader = [(x[i:i + B], t[i:i + B]) for i in range(0, N, B)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    table = marginal_table(vae, loader, n_particles=K, seed=0)
    torch.cuda.synchronize()
    t_table = time.perf_counter() - t0
    print("marginal_table     N = %d  K = %d  3 posteriors  %.1f s  (%.0f particles/s)" % (N, K, t_table, 3.0 * N * K / t_table))
    for post, r in table.items():
        print("  %-5s log p(x) >= %.3f  log p(y) >= %.3f  log p(x,y) >= %.3f  image NLL %.3f  text NLL %.3f  mean ESS %s" %
              (post, r["log_px"], r["log_py"], r["log_pxy"], r["image_nll"], r["text_nll"],
               " / ".join("%.2f" % v for v in r["ess"].double().mean(0).tolist())))


if __name__ == "__main__":
    main()
