"""``coco/train_textonly.py``-compatible driver of the uni-modal caption baseline.

The reference script's command line, printed lines, KL schedule (``:145-153``: 1e-3, or with ``--anneal_kl`` the next value of
1e-5 ... 1.0 every 5 epochs) and checkpoint dict (``state_dict``, ``best_loss``, ``n_latents``, ``optimizer``), with the batch loop
body (``:106-120``) replaced by ONE fused enqueue (``TextVAETrainer``: one pass over B rows, no product of experts, the image half
of the plan never launched) and the ``DataLoader`` by ``data.DeviceBatcher``.

    python -m multimodal_vae_amd.train_textonly --cuda --data ./data/coco
    python -m multimodal_vae_amd.train_textonly --cuda --epochs 2 --synthetic 4096 --synthetic_words 500   # no data files needed

One departure: ``--n_latents`` defaults to 100, not the reference's 200.  The COCO plan takes n_latents 4..124 in multiples of 4
(the operand padding of the caption kernels); 200 is refused on the host.

``--data DIR`` is the folder ``train_coco --data`` reads: ``captions.pt`` ((N,102,300) fp32) and ``sos.pt`` (the first tenth is the
test split).  The '<s>' vector comes from ``--sos FILE.pt``, else from the word table, else from ``DIR/sos.pt``.  With a word table
(``--words TABLE.pt`` as written by ``coco.save_word_table``, or ``--synthetic_words V``) each epoch writes
``sample_text_epochN.txt`` from ``vae.decoder.generate(z)`` of 64 prior samples (``:168-174``); without one the raw vectors go to
``sample_text_epochN.pt``.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

from .train_common import eval_epoch, kl_schedule, save_checkpoint, train_epoch
from .train_common import kl_lambdas as _kl_lambdas
from .train_imageonly import image_adam_state_dict as own_adam_state_dict

DEFAULT_N_LATENTS = 100      # reference: 200, outside the plan's 4..124
DEFAULT_KL_LAMBDA = 1e-3     # coco/train_textonly.py:145


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="text-only VAE baseline (coco/train_textonly.py) on the fused one-pass caption step")
    # the reference's flags, same names / defaults (coco/train_textonly.py:46-59) but for --n_latents
    parser.add_argument('--n_latents', type=int, default=DEFAULT_N_LATENTS,
                        help='size of the latent embedding (default: 100; the reference defaults to 200, which the caption kernels '
                             'do not take: 4..124 in multiples of 4)')
    parser.add_argument('--batch_size', type=int, default=64, metavar='N', help='input batch size for training (default: 64)')
    parser.add_argument('--epochs', type=int, default=20, metavar='N', help='number of epochs to train (default: 20)')
    parser.add_argument('--lr', type=float, default=1e-4, metavar='LR', help='learning rate (default: 1e-4)')
    parser.add_argument('--log_interval', type=int, default=10, metavar='N', help='how many batches to wait before logging training status (default: 10)')
    parser.add_argument('--anneal_kl', action='store_true', default=False, help='if True, use a fixed interval of doubling the KL term')
    parser.add_argument('--cuda', action='store_true', default=False, help='enables CUDA training')
    # additions, as train_imageonly
    parser.add_argument('--data', type=str, default='./data/coco', metavar='DIR', help='folder with captions.pt and sos.pt (as train_coco)')
    parser.add_argument('--synthetic', type=int, default=0, metavar='N', help='train on N synthetic captions instead of files')
    parser.add_argument('--out', type=str, default='./trained_models/text_only', help='checkpoint folder (reference: ./trained_models/text_only)')
    parser.add_argument('--results', type=str, default='./results/text_only', help='folder of the per-epoch sample dumps (off when empty)')
    parser.add_argument('--seed', type=int, default=1234)
    # where the '<s>' vector and the words of the sample captions come from
    parser.add_argument('--sos', type=str, default='', metavar='FILE.pt', help="the 300-d vector of '<s>' (default: the word table's, else DIR/sos.pt)")
    parser.add_argument('--words', type=str, default='', metavar='TABLE.pt', help='word table (coco.save_word_table): sample captions are written as text')
    parser.add_argument('--synthetic_words', type=int, default=0, metavar='V', help="a random table of V words (with '<s>' and '</s>') instead of --words")
    return parser


def kl_lambdas(epochs: int, anneal_kl: bool = False):
    """kl_lambda of epochs 1..epochs (coco/train_textonly.py:145-153): 1e-3, or with --anneal_kl the next value of
    1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0 every 5 epochs, the last one kept."""
    return _kl_lambdas(DEFAULT_KL_LAMBDA, kl_schedule(), epochs, anneal_kl)


def checkpoint_dict(vae, engine, best_loss, n_latents) -> dict:
    """coco/train_textonly.py:161-166; the optimizer state covers the TextVAE's own (caption) parameters only."""
    return {'state_dict': vae.state_dict(), 'best_loss': best_loss, 'n_latents': n_latents,
            'optimizer': own_adam_state_dict(vae, engine)}


def _load_captions(args):
    """(training captions, test captions, sos or None)"""
    if args.synthetic > 0:
        from .train_coco import synthetic_coco
        _, tr, sos = synthetic_coco(args.synthetic, seed=args.seed)
        _, te, _ = synthetic_coco(max(args.batch_size, args.synthetic // 6), seed=args.seed + 1)
        return tr, te, sos
    t = torch.as_tensor(torch.load(os.path.join(args.data, "captions.pt"), weights_only=False))
    sos_path = os.path.join(args.data, "sos.pt")
    sos = torch.as_tensor(torch.load(sos_path, weights_only=False)) if os.path.exists(sos_path) else None
    n_test = max(args.batch_size, len(t) // 10)          # as train_coco: the first tenth is the test split
    return t[n_test:], t[:n_test], sos


def main(argv=None) -> dict:
    args = build_parser().parse_args(argv)
    args.cuda = args.cuda and torch.cuda.is_available()
    if not args.cuda:
        raise SystemExit("this engine runs on a gfx950 GPU only: pass --cuda on a machine that has one (no CPU fallback)")
    from . import data as D
    from . import coco as M
    try:
        M.check_text_latents(args.n_latents)
    except M.MMVAEError as e:
        raise SystemExit(str(e))

    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(args.seed)
    tr_t, te_t, sos = _load_captions(args)
    for name, t in (("training", tr_t), ("test", te_t)):
        if t.dtype != torch.float32 or tuple(t.shape[1:]) != (M.MAX_WORDS, M.N_EMBEDDING):
            raise SystemExit("the %s captions must be float32 (N,%d,%d) (got %s %s)" % (name, M.MAX_WORDS, M.N_EMBEDDING, t.dtype, tuple(t.shape)))
        if len(t) < args.batch_size:
            raise SystemExit("the %s split has %d captions, fewer than one batch of %d (the fused plan takes whole batches)"
                             % (name, len(t), args.batch_size))
    words = None
    if args.words:
        words = M.load_word_table(args.words, dev)
    elif args.synthetic_words > 0:
        words = M.WordTable(*D.synthetic_word_table(args.synthetic_words, seed=args.seed), device=dev)
    if args.sos:
        sos = torch.as_tensor(torch.load(args.sos, weights_only=False))
    elif words is not None and words.get_word(M.SOS) is not None:
        sos = words.get_word(M.SOS).detach().cpu()
    if sos is None:
        raise SystemExit("no '<s>' vector: give --sos FILE.pt, a word table that has '<s>', or DIR/sos.pt")
    none = lambda t: torch.zeros(len(t), 1, 2, 2, dtype=torch.uint8)     # the batcher carries an image tensor: nothing reads it
    train_loader = D.DeviceBatcher(none(tr_t), tr_t, args.batch_size, dev, shuffle=True, seed=args.seed)
    test_loader = D.DeviceBatcher(none(te_t), te_t, args.batch_size, dev, shuffle=True, seed=args.seed + 7)

    vae = M.TextVAE(args.n_latents, use_cuda=True, words=words, sos=sos)
    vae.cuda()
    trainer = M.TextVAETrainer(vae, args.batch_size, lr=args.lr, kl_lambda=DEFAULT_KL_LAMBDA, seed=args.seed)

    def train(epoch, kl_lambda):
        vae.train()
        avg, = train_epoch(
            train_loader, lambda b: trainer(b[1], kl_lambda=kl_lambda).losses()[0], args.batch_size, args.log_interval,
            lambda seen, n_total, pct, avg: 'Train Epoch: {} [{}/{} ({:.0f}%)]\tLoss: {:.6f}'.format(epoch, seen, n_total, pct, *avg),
            len(train_loader) * args.batch_size)
        print('====> Epoch: {} Average loss: {:.4f}'.format(epoch, avg))
        return avg

    def test(kl_lambda):
        vae.eval()
        test_loss, = eval_epoch(test_loader, lambda b: trainer.evaluate(b[1], kl_lambda=kl_lambda).losses()[0], 1, dev)
        print('====> Test set loss: {:.4f}'.format(test_loss))
        return test_loss

    best_loss = float(sys.maxsize)
    history = {"train": [], "test": [], "kl_lambda": []}
    schedule = kl_lambdas(args.epochs, args.anneal_kl)
    for epoch in range(1, args.epochs + 1):
        kl_lambda = schedule[epoch - 1]
        history["kl_lambda"].append(kl_lambda)
        history["train"].append(train(epoch, kl_lambda))
        loss = test(kl_lambda)
        history["test"].append(loss)
        is_best = loss < best_loss
        best_loss = min(loss, best_loss)
        save_checkpoint(checkpoint_dict(vae, trainer.engine, best_loss, args.n_latents), is_best, folder=args.out)
        if args.results:
            os.makedirs(args.results, exist_ok=True)
            sample = torch.randn(64, args.n_latents, device=dev)
            vae.eval()
            with torch.no_grad():
                if words is not None:
                    with open(os.path.join(args.results, 'sample_text_epoch%d.txt' % epoch), 'w') as fp:
                        fp.writelines(s + '\n' for s in vae.decoder.generate(sample))
                else:
                    torch.save(vae.decoder.generate_vector(sample).cpu(), os.path.join(args.results, 'sample_text_epoch%d.pt' % epoch))
    return history


if __name__ == "__main__":
    main()
