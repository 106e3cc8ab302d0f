"""Rate of the importance-sampled evaluation (evaluate.iw_estimate / marginal_table) against a compute_nll-style loop.

    python tools/loglik_bench.py [--dataset multimnist|mnist|celeba|coco] [--batch 64] [--particles 1000] [--loop_particles 100] [--batches 4]
                                 [--table_examples 10000]

--dataset mnist (``main_mnist``): the fused fp32 scorer mmvae_mnist_iw_score against an unfused batched chain of the drop-in
decoder modules + torch ops, see there.  --dataset celeba (``main_celeba``): mmvae_celeba_iw_score against the unfused chain
``vae.image_decoder`` / ``vae.attrs_decoder`` + torch ops on the same particles, see there.  The rest of this text is the
MultiMNIST mode.

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


def main_mnist(args):
    """MNIST: particles/s of
      * ``iw_estimate`` on the fused scorer (mmvae_iw_particles -> mmvae_mnist_iw_score -> mmvae_iw_accumulate -> finalize);
      * the same pipeline with the scoring call replaced by the unfused batched chain a user could write without it: the image- and
        text-decoder module forwards called once on all rows of the chunk, then torch ops on what they return
        (-binary_cross_entropy(p, x) per element = x log p + (1 - x) log(1 - p) in ONE elementwise kernel, summed per row; the
        log-probabilities go to mmvae_iw_accumulate as they are).  Same particles, same chunks, same accumulator;
      * the two scoring steps alone on one chunk of particles (device events), and the TFLOP/s of the decoder's
        2 (D 200 + 200 400 + 400 784 + D 10 + 10 10) FLOP per particle over the fused kernel's time;
      * the per-particle loop of ``compute_nll_mnist``;
      * the wall time of ``marginal_table`` on --table_examples synthetic examples.
    The two iw pipelines alternate ``--repeats`` times after a warm-up of both; their log p^ are compared on the first batch."""
    import ctypes as C
    import torch.nn.functional as F
    from multimodal_vae_amd import mnist as M, data as Dd
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd.evaluate import (iw_estimate, marginal_table, compute_nll_mnist, _proposal, iw_chunks, IW_ROWS_MNIST)
    from oracle import mmvae_ref as R
    dev = torch.device("cuda:0")
    D, B, K = 20, args.batch, args.particles
    vae = M.MultimodalVAE(D)
    vae.load_state_dict(R.formula_params("mnist", D), strict=True)
    vae.cuda().eval()
    st = vae._core.sync(dev)
    n = max(args.table_examples, B * (args.batches + 1))
    x, t = Dd.synthetic_mnist(n, seed=0)
    x = x.float().div_(255.0).view(-1, 784)
    batches = [(x[i:i + B].to(dev), t[i:i + B].to(dev)) for i in range(0, B * (args.batches + 1), B)]
    f32 = dict(dtype=torch.float32, device=dev)
    flops_particle = 2.0 * (D * 200 + 200 * 400 + 400 * 784 + D * 10 + 10 * 10)

    def stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def unfused_score(z, image, nr, nk):
        """log p(x|z) (nr*nk,) and the log-probabilities (nr*nk, 10) from the decoder modules + torch ops."""
        p = vae.decode_image(z)
        words = vae.decode_text(z)
        lx = -F.binary_cross_entropy(p.view(nr, nk, 784), image.unsqueeze(1).expand(nr, nk, 784), reduction="none").sum(2)
        return lx.reshape(-1).contiguous(), words.contiguous()

    def run_unfused(i):
        image, label = batches[i]
        mu, lv = props[i]
        state = torch.empty(B, 3, 4, **f32)
        call("mmvae_iw_init", ptr(state), B, stream())
        for r0, nr, k0, nk in iw_chunks(B, K, IW_ROWS_MNIST):
            rows = nr * nk
            z, lr = torch.empty(rows, D, **f32), torch.empty(rows, **f32)
            call("mmvae_iw_particles", ptr(mu[r0:]), ptr(lv[r0:]), nr, D, nk, i * B + r0, k0, 0, None, ptr(z), ptr(lr), stream())
            lx, words = unfused_score(z, image[r0:r0 + nr], nr, nk)
            call("mmvae_iw_accumulate", ptr(lx), ptr(words), ptr(label[r0:]), 1, 10, ptr(lr), nr, nk, ptr(state[r0:]), None, stream())
        out = torch.empty(B, 8, **f32)
        call("mmvae_iw_finalize", ptr(state), B, K, ptr(out), stream())
        return out[:, 0:3]

    def run_fused(i):
        return iw_estimate(vae, batches[i][0], batches[i][1], props[i][0], props[i][1], K, first_row=i * B)["log_p"]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(1, len(batches)):
            fn(i)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    with torch.no_grad():
        props = [_proposal(vae, im, lb, "joint") for im, lb in batches]
        a, b = run_fused(0), run_unfused(0)                     # warm-up of both, and the same numbers from both
        torch.cuda.synchronize()
        diff = (a.double() - b.double()).abs().max(0).values.tolist()
        tf, tu = [], []
        for _ in range(args.repeats):
            tf.append(timed(run_fused))
            tu.append(timed(run_unfused))
    per = B * K * args.batches
    rate_f, rate_u = per / min(tf), per / min(tu)
    print("loglik_bench --dataset mnist: B = %d, K = %d, n_latents = %d, rows per scoring call <= %d, %d batches per timing" %
          (B, K, D, IW_ROWS_MNIST, args.batches))
    print("fused   vs unfused log p^ (x, y, xy) of batch 0: max abs difference %s" % " / ".join("%.2e" % v for v in diff))
    print("iw_estimate, fused scorer     %12.0f particles/s  (best of %s s)" % (rate_f, ", ".join("%.4f" % v for v in tf)))
    print("same pipeline, unfused chain  %12.0f particles/s  (best of %s s)" % (rate_u, ", ".join("%.4f" % v for v in tu)))
    print("ratio fused / unfused         %.2fx  %s" % (rate_f / rate_u, "" if rate_f >= rate_u else "(THE FUSED SCORER IS SLOWER)"))
    sys.stdout.flush()

    # ---- the scoring step alone on one chunk (device events, 10 calls each after a warm-up call)
    with torch.no_grad():
        r0, nr, k0, nk = iw_chunks(B, K, IW_ROWS_MNIST)[0]
        rows = nr * nk
        image = batches[1][0][r0:r0 + nr].contiguous()
        z, lr = torch.empty(rows, D, **f32), torch.empty(rows, **f32)
        call("mmvae_iw_particles", ptr(props[1][0]), ptr(props[1][1]), nr, D, nk, 0, 0, 0, None, ptr(z), ptr(lr), stream())
        lx, words = torch.empty(rows, **f32), torch.empty(rows, 10, **f32)

        def fused_score():
            call("mmvae_mnist_iw_score", st.plan(1), ptr(z), ptr(image), nr, nk, ptr(lx), ptr(words), stream())

        def ev_time(fn, reps=10):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / reps
        t_fs = ev_time(fused_score)
        t_us = ev_time(lambda: unfused_score(z, image, nr, nk))
    print("scoring step alone, %d rows:  fused kernel %.3f ms (%.1f TFLOP/s of %.3f MFLOP per particle, fp32 MFMA)   "
          "unfused chain %.3f ms   ratio %.2fx" % (rows, t_fs * 1e3, flops_particle * rows / t_fs / 1e12, flops_particle / 1e6,
                                                    t_us * 1e3, t_us / t_fs))
    print("achieved in iw_estimate       %.1f TFLOP/s (decoder count over the iw_estimate wall time)" % (flops_particle * rate_f / 1e12))
    sys.stdout.flush()

    # ---- the compute_nll_mnist loop (one decoder module call pair per particle index, host sums), batch 0 is the warm-up
    Kl = args.loop_particles
    cpu_batches = [(im.cpu(), lb.cpu()) for im, lb in batches]
    compute_nll_mnist(vae, cpu_batches[:1], n_samples=Kl, use_cuda=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    compute_nll_mnist(vae, cpu_batches[1:], n_samples=Kl, use_cuda=True)
    torch.cuda.synchronize()
    t_loop = time.perf_counter() - t0
    rate_loop = B * Kl * args.batches / t_loop
    print("compute_nll_mnist loop  K = %4d  %d batches  %.3f s  %12.0f particles/s   (fused iw_estimate: %.0fx)" %
          (Kl, args.batches, t_loop, rate_loop, rate_f / rate_loop))
    sys.stdout.flush()

    # ---- marginal_table on table_examples synthetic examples
    N = args.table_examples
    loader = [(x[i:i + B], t[i:i + B]) for i in range(0, N, B)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    table = marginal_table(vae, loader, n_particles=K, seed=0)
    torch.cuda.synchronize()
    t_table = time.perf_counter() - t0
    print("marginal_table     N = %d  K = %d  3 posteriors  %.2f s  (%.0f particles/s, %.1f TFLOP/s of the decoder count)" %
          (N, K, t_table, 3.0 * N * K / t_table, flops_particle * 3.0 * N * K / t_table / 1e12))
    for post, r in table.items():
        print("  %-5s log p(x) >= %.3f  log p(y) >= %.3f  log p(x,y) >= %.3f  image NLL %.3f  text NLL %.3f  mean ESS %s" %
              (post, r["log_px"], r["log_py"], r["log_pxy"], r["image_nll"], r["text_nll"],
               " / ".join("%.2f" % v for v in r["ess"].double().mean(0).tolist())))


def main_celeba(args):
    """CelebA: particles/s of
      * ``iw_estimate`` on mmvae_celeba_iw_score (particles -> bf16 decoder body -> scoring tail + fp32 attribute scorer ->
        accumulate -> finalize);
      * the same pipeline with the scoring call replaced by the unfused chain a user could write without it: ``vae.image_decoder``
        and ``vae.attrs_decoder`` called once on all rows of the chunk, then torch ops on the probabilities they return
        (-binary_cross_entropy per element, summed per row; (log(1 - p), log p) of the attributes as the words).  Same
        particles, same chunks of at most IW_ROWS_CELEBA rows, same accumulator;
      * the two scoring steps alone on one chunk (device events), and the TFLOP/s of the image decoder's algorithmic count
        (2 x multiply-adds of upsample + the four transposed convolutions) over the scoring call's time.
    The two pipelines alternate ``--repeats`` times after a warm-up of both; their log p^ are compared on the first batch."""
    import ctypes as C
    import torch.nn.functional as F
    from multimodal_vae_amd import celeba as M, data as Dd
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd.evaluate import iw_estimate, _proposal, iw_chunks, IW_ROWS_CELEBA
    from oracle import mmvae_ref as R
    dev = torch.device("cuda:0")
    D, B, K = 100, args.batch, args.particles
    vae = M.MultimodalVAE(D)
    vae.load_state_dict(R.formula_params("celeba", D), strict=True)
    vae.cuda().eval()
    st = vae._core.sync(dev)
    x, t = Dd.synthetic_celeba(B * (args.batches + 1), seed=0)
    x = x.float().div_(255.0)
    batches = [(x[i:i + B].to(dev), t[i:i + B].to(dev)) for i in range(0, B * (args.batches + 1), B)]
    f32 = dict(dtype=torch.float32, device=dev)
    # multiply-adds per particle: Linear(D, 6400), ConvTranspose2d 5x5x256 -> 8x8x128 (every input pixel meets all 16 taps),
    # 8x8x128 -> 16x16x64, 16x16x64 -> 32x32x32, 32x32x32 -> 64x64x3 (stride 2: 4 taps per output pixel)
    flops_particle = 2.0 * (D * 6400 + 25 * 256 * 128 * 16 + 256 * 128 * 64 * 4 + 1024 * 64 * 32 * 4 + 4096 * 32 * 3 * 4)

    def stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def unfused_score(z, image, nr, nk):
        """log p(x|z) (nr*nk,) and the words (nr*nk, 18, 2) from the decoder modules + torch ops."""
        p = vae.image_decoder(z)
        pa = vae.attrs_decoder(z)
        lx = -F.binary_cross_entropy(p.view(nr, nk, -1), image.reshape(nr, 1, -1).expand(nr, nk, 3 * 64 * 64), reduction="none").sum(2)
        words = torch.stack([torch.log1p(-pa), torch.log(pa)], 2)
        return lx.reshape(-1).contiguous(), words.contiguous()

    def run_unfused(i):
        image, attrs = batches[i]
        mu, lv = props[i]
        tgt = attrs.long().contiguous()
        state = torch.empty(B, 3, 4, **f32)
        call("mmvae_iw_init", ptr(state), B, stream())
        for r0, nr, k0, nk in iw_chunks(B, K, IW_ROWS_CELEBA):
            rows = nr * nk
            z, lr = torch.empty(rows, D, **f32), torch.empty(rows, **f32)
            call("mmvae_iw_particles", ptr(mu[r0:]), ptr(lv[r0:]), nr, D, nk, i * B + r0, k0, 0, None, ptr(z), ptr(lr), stream())
            lx, words = unfused_score(z, image[r0:r0 + nr], nr, nk)
            call("mmvae_iw_accumulate", ptr(lx), ptr(words), ptr(tgt[r0:]), 18, 2, ptr(lr), nr, nk, ptr(state[r0:]), None, stream())
        out = torch.empty(B, 8, **f32)
        call("mmvae_iw_finalize", ptr(state), B, K, ptr(out), stream())
        return out[:, 0:3]

    def run_fused(i):
        return iw_estimate(vae, batches[i][0], batches[i][1], props[i][0], props[i][1], K, first_row=i * B)["log_p"]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(1, len(batches)):
            fn(i)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    with torch.no_grad():
        props = [_proposal(vae, im, at, "joint") for im, at in batches]
        a, b = run_fused(0), run_unfused(0)                     # warm-up of both, and the same numbers from both
        torch.cuda.synchronize()
        diff = (a.double() - b.double()).abs().max(0).values.tolist()
        tf, tu = [], []
        for _ in range(args.repeats):
            tf.append(timed(run_fused))
            tu.append(timed(run_unfused))
    per = B * K * args.batches
    rate_f, rate_u = per / min(tf), per / min(tu)
    chunks = iw_chunks(B, K, IW_ROWS_CELEBA)
    print("loglik_bench --dataset celeba: B = %d, K = %d, n_latents = %d, %d scoring calls of <= %d rows per batch, %d batches per timing" %
          (B, K, D, len(chunks), IW_ROWS_CELEBA, args.batches))
    print("fused   vs unfused log p^ (x, y, xy) of batch 0: max abs difference %s" % " / ".join("%.2e" % v for v in diff))
    print("iw_estimate, mmvae_celeba_iw_score  %12.0f particles/s  (best of %s s)" % (rate_f, ", ".join("%.4f" % v for v in tf)))
    print("same pipeline, unfused chain        %12.0f particles/s  (best of %s s)" % (rate_u, ", ".join("%.4f" % v for v in tu)))
    print("ratio fused / unfused               %.2fx  %s" % (rate_f / rate_u, "" if rate_f >= rate_u else "(THE FUSED SCORER IS SLOWER)"))
    sys.stdout.flush()

    # ---- the scoring step alone on one chunk (device events, 10 calls each after a warm-up call)
    with torch.no_grad():
        r0, nr, k0, nk = chunks[0]
        rows = nr * nk
        image = batches[1][0][r0:r0 + nr].contiguous()
        z, lr = torch.empty(rows, D, **f32), torch.empty(rows, **f32)
        call("mmvae_iw_particles", ptr(props[1][0]), ptr(props[1][1]), nr, D, nk, 0, 0, 0, None, ptr(z), ptr(lr), stream())
        lx, words = torch.empty(rows, **f32), torch.empty(rows, 18, 2, **f32)
        h = st.plan(rows)
        wsb = call("mmvae_celeba_iw_workspace_bytes", h)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

        def fused_score():
            call("mmvae_celeba_iw_score", h, ptr(ws), wsb, ptr(z), ptr(image), nr, nk, ptr(lx), ptr(words), stream())

        def ev_time(fn, reps=10):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / reps
        t_fs = ev_time(fused_score)
        t_us = ev_time(lambda: unfused_score(z, image, nr, nk))
    print("scoring step alone, %d rows (workspace %.1f MiB):  mmvae_celeba_iw_score %.3f ms (%.1f TFLOP/s of %.2f MFLOP per particle, "
          "bf16 MFMA)   unfused chain %.3f ms   ratio %.2fx" % (rows, wsb / 2.0 ** 20, t_fs * 1e3, flops_particle * rows / t_fs / 1e12,
                                                                flops_particle / 1e6, t_us * 1e3, t_us / t_fs))
    print("achieved in iw_estimate             %.1f TFLOP/s (decoder count over the iw_estimate wall time)" % (flops_particle * rate_f / 1e12))


def main_coco(args):
    """COCO: particles/s of
      * ``iw_estimate`` on mmvae_coco_iw_score (particles -> bf16 image decoder body -> scoring tail, caption decoder -> squared
        error per row -> accumulate -> finalize);
      * the same pipeline with the scoring call replaced by the unfused chain a user could write without it: ``vae.image_decoder``
        and ``vae.text_decoder`` called once on all rows of the chunk, then torch ops on what they return (-binary_cross_entropy per
        element summed per row; the squared error against the captions summed per row, times -1/2).  Same particles, same chunks
        of at most IW_ROWS_COCO rows, same accumulator;
      * the two scoring steps alone on one chunk (device events);
      * the scoring tail alone (mmvae_coco_iw_tail on an IW_ROWS_COCO-row raw tensor) against its byte bound: the raw tensor read
        once, 32 KB per row, plus the row's image.
    The 102 sequential GRU steps of the caption decoder are in both pipelines and dominate both.  The two pipelines alternate
    ``--repeats`` times after a warm-up of both; their log p^ are compared on the first batch."""
    import ctypes as C
    import torch.nn.functional as F
    from multimodal_vae_amd import coco as M
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd.evaluate import iw_estimate, _proposal, iw_chunks, IW_ROWS_COCO
    from multimodal_vae_amd.train_coco import synthetic_coco
    from oracle import mmvae_ref as R
    dev = torch.device("cuda:0")
    D, B, K, T = 100, args.batch, args.particles, M.MAX_WORDS
    x, t, sos = synthetic_coco(B * (args.batches + 1), seed=0)
    vae = M.MultimodalVAE(D, sos=sos)
    vae.load_state_dict(R.formula_params("coco", D), strict=True)
    vae.cuda().eval()
    st = vae._core.sync(dev)
    x = x.float().div_(255.0)
    batches = [(x[i:i + B].to(dev), t[i:i + B].to(dev).contiguous()) for i in range(0, B * (args.batches + 1), B)]
    f32 = dict(dtype=torch.float32, device=dev)
    zeros = torch.zeros(B, 1, dtype=torch.int64, device=dev)

    def stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def unfused_score(z, image, text, nr, nk):
        """log p(x|z) (nr*nk,) and -SSE / 2 (nr*nk,) from the decoder modules + torch ops."""
        p = vae.image_decoder(z)
        y = vae.text_decoder(z)
        lx = -F.binary_cross_entropy(p.view(nr, nk, -1), image.reshape(nr, 1, -1).expand(nr, nk, 3 * 32 * 32), reduction="none").sum(2)
        ly = (y.view(nr, nk, T, 300) - text.view(nr, 1, T, 300)).pow(2).sum((2, 3)).mul(-0.5)
        return lx.reshape(-1).contiguous(), ly.reshape(-1).contiguous()

    def run_unfused(i):
        image, text = batches[i]
        mu, lv = props[i]
        state = torch.empty(B, 3, 4, **f32)
        call("mmvae_iw_init", ptr(state), B, stream())
        for r0, nr, k0, nk in iw_chunks(B, K, IW_ROWS_COCO):
            rows = nr * nk
            z, lr = torch.empty(rows, D, **f32), torch.empty(rows, **f32)
            call("mmvae_iw_particles", ptr(mu[r0:]), ptr(lv[r0:]), nr, D, nk, i * B + r0, k0, 0, None, ptr(z), ptr(lr), stream())
            lx, words = unfused_score(z, image[r0:r0 + nr], text[r0:r0 + nr], nr, nk)
            call("mmvae_iw_accumulate", ptr(lx), ptr(words), ptr(zeros[r0:]), 1, 1, ptr(lr), nr, nk, ptr(state[r0:]), None, stream())
        out = torch.empty(B, 8, **f32)
        call("mmvae_iw_finalize", ptr(state), B, K, ptr(out), stream())
        return out[:, 0:3]

    def run_fused(i):
        r = iw_estimate(vae, batches[i][0], batches[i][1], props[i][0], props[i][1], K, first_row=i * B)["log_p"].clone()
        r[:, 1:3] -= const                                      # (the unfused chain above carries no constant)
        return r

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(1, len(batches)):
            fn(i)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    from multimodal_vae_amd.evaluate import coco_text_constant
    const = coco_text_constant(T, 1.0)
    with torch.no_grad():
        props = [_proposal(vae, im, tx, "joint") for im, tx in batches]
        a, b = run_fused(0), run_unfused(0)                     # warm-up of both, and the same numbers from both
        torch.cuda.synchronize()
        diff = (a.double() - b.double()).abs().max(0).values.tolist()
        tf, tu = [], []
        for _ in range(args.repeats):
            tf.append(timed(run_fused))
            tu.append(timed(run_unfused))
    per = B * K * args.batches
    rate_f, rate_u = per / min(tf), per / min(tu)
    chunks = iw_chunks(B, K, IW_ROWS_COCO)
    print("loglik_bench --dataset coco: B = %d, K = %d, n_latents = %d, steps = %d, %d scoring calls of <= %d rows per batch, %d batches per timing" %
          (B, K, D, T, len(chunks), IW_ROWS_COCO, args.batches))
    print("fused   vs unfused log p^ (x, y, xy) of batch 0 (without the constant): max abs difference %s" % " / ".join("%.2e" % v for v in diff))
    print("iw_estimate, mmvae_coco_iw_score    %12.0f particles/s  (best of %s s)" % (rate_f, ", ".join("%.4f" % v for v in tf)))
    print("same pipeline, unfused chain        %12.0f particles/s  (best of %s s)" % (rate_u, ", ".join("%.4f" % v for v in tu)))
    print("ratio fused / unfused               %.2fx  %s" % (rate_f / rate_u, "" if rate_f >= rate_u else "(THE FUSED SCORER IS SLOWER)"))
    sys.stdout.flush()

    def ev_time(fn, reps=10):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    # ---- the scoring step alone on one chunk (device events, 10 calls each after a warm-up call)
    with torch.no_grad():
        r0, nr, k0, nk = chunks[0]
        rows = nr * nk
        image, text = batches[1][0][r0:r0 + nr].contiguous(), batches[1][1][r0:r0 + nr].contiguous()
        z, lr = torch.empty(rows, D, **f32), torch.empty(rows, **f32)
        call("mmvae_iw_particles", ptr(props[1][0]), ptr(props[1][1]), nr, D, nk, 0, 0, 0, None, ptr(z), ptr(lr), stream())
        lx, sse = torch.empty(rows, **f32), torch.empty(rows, **f32)
        h = st.plan(rows)
        wsb = call("mmvae_coco_iw_workspace_bytes", h)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        sosd = vae.text_decoder.sos.to(dev).contiguous()

        def fused_score():
            call("mmvae_coco_iw_score", h, ptr(ws), wsb, ptr(z), ptr(image), ptr(text), ptr(sosd), nr, nk, ptr(lx), ptr(sse), stream())
        t_fs = ev_time(fused_score)
        t_us = ev_time(lambda: unfused_score(z, image, text, nr, nk))
    print("scoring step alone, %d rows (workspace %.1f MiB):  mmvae_coco_iw_score %.3f ms   unfused chain %.3f ms   ratio %.2fx" %
          (rows, wsb / 2.0 ** 20, t_fs * 1e3, t_us * 1e3, t_us / t_fs))
    # ---- the scoring tail alone against its byte bound
    n = IW_ROWS_COCO
    g = torch.Generator().manual_seed(0)
    q3 = torch.randn(n, 16, 16, 64, generator=g).to(dev).to(torch.bfloat16).contiguous()
    aff = torch.tensor([1.0, 0.0]).repeat(64, 1).to(dev).contiguous()
    w = (torch.randn(64, 3, 4, 4, generator=g) * 0.05).to(dev).contiguous()
    img = torch.rand(n, 3, 32, 32, generator=g).to(dev).contiguous()
    ll = torch.empty(n, **f32)
    t_tail = ev_time(lambda: call("mmvae_coco_iw_tail", ptr(q3), ptr(aff), 1, ptr(w), ptr(img), n, 1, ptr(ll), None, stream()), reps=50)
    nbytes = n * (16 * 16 * 64 * 2 + 3 * 32 * 32 * 4)
    print("scoring tail alone, %d rows:  %.1f us, %.2f MB read once (raw tensor 32 KB + image 12 KB per row) = %.0f GB/s "
          "(50 calls back to back between device events; the inputs fit the cache)" % (n, t_tail * 1e6, nbytes / 1e6, nbytes / t_tail / 1e9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", choices=("multimnist", "mnist", "celeba", "coco"), default="multimnist")
    ap.add_argument("--repeats", type=int, default=3, help="mnist, celeba: alternations of the fused and the unfused pipeline")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--particles", type=int, default=1000)
    ap.add_argument("--loop_particles", type=int, default=100)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--table_examples", type=int, default=10000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loglik_bench: no GPU (the rates are only measured on the device)")
    if args.dataset == "mnist":
        return main_mnist(args)
    if args.dataset == "celeba":
        return main_celeba(args)
    if args.dataset == "coco":
        return main_coco(args)
    from multimodal_vae_amd import multimnist as M, data as Dd
    from multimodal_vae_amd._lib import call
    from multimodal_vae_amd.evaluate import iw_estimate, marginal_table, _proposal, iw_chunks, IW_ROWS
    from multimodal_vae_amd.modules import _BCEMeanFn, _NLLMeanFn
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
