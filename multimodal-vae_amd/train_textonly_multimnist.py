"""``train_textonly.py``-compatible driver of the MultiMNIST text-only VAE baseline on the MI355X engine.

Mirrors the command line, KL schedule, meters, checkpoint dict and epoch loop of the reference's ``multimnist/train_textonly.py``
(flags ``:48-61``, ``train()`` ``:95-115``, ``test()`` ``:118-131``, KL schedule ``:134-142``, checkpoint dict ``:150-155``), with the
batch loop body replaced by ONE fused enqueue (``multimnist.TextVAETrainer``: the text kernels at hidden size 50).

    python -m multimodal_vae_amd.train_textonly_multimnist --cuda --epochs 2 --synthetic 4096     # no data files needed
    python -m multimodal_vae_amd.train_textonly_multimnist --cuda --data ./data                    # labels of processed/*.pt
    python -m multimodal_vae_amd.train_textonly_multimnist --cuda --generate --mnist_train A.pt --mnist_test B.pt

Only the labels of a data set are used.  Deliberate differences: a fixed batch size (the ragged last batch of an epoch is dropped: a
fused plan is built per batch size); loss values are read back every ``--log_interval`` batches only; ``sample_text_epochN.txt`` holds the
greedy tokens, one string per line (the reference's ``generate`` samples ``torch.multinomial`` from log-probabilities, which a modern
torch rejects; ``TextDecoder.generate`` keeps doing so).
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

from .train_common import (adam_state_dict, add_generate_flags, eval_epoch, kl_lambdas, kl_schedule, mnist_digit_sources, save_checkpoint,
                           train_epoch)


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser()
    # the reference's flags, same names / defaults (multimnist/train_textonly.py:48-61)
    parser.add_argument('--n_latents', type=int, default=100, help='size of the latent embedding')
    parser.add_argument('--batch_size', type=int, default=128, metavar='N', help='input batch size for training (default: 128)')
    parser.add_argument('--epochs', type=int, default=20, metavar='N', help='number of epochs to train (default: 20)')
    parser.add_argument('--lr', type=float, default=1e-3, metavar='LR', help='learning rate (default: 1e-3)')
    parser.add_argument('--log_interval', type=int, default=10, metavar='N', help='how many batches to wait before logging training status')
    parser.add_argument('--anneal_kl', action='store_true', default=False, help='if True, use a fixed interval of doubling the KL term')
    parser.add_argument('--cuda', action='store_true', default=False, help='enables CUDA training')
    # additions
    parser.add_argument('--data', type=str, default='./data', help="root of the reference's processed/{training,test}.pt (labels only)")
    parser.add_argument('--synthetic', type=int, default=0, metavar='N', help='train on the labels of N synthetic samples instead of files')
    parser.add_argument('--out', type=str, default='./trained_models/text_only', help='checkpoint folder')
    parser.add_argument('--results', type=str, default='./results/text_only', help='folder of the per-epoch text samples')
    parser.add_argument('--seed', type=int, default=1234)
    add_generate_flags(parser, 'labels of canvases generated on the device: --mnist_train / --mnist_test, or synthetic digits with --synthetic N')
    return parser


class LabelBatcher:
    """Fixed-size batches of an int64 (N, 4) label tensor kept on the device; a fresh permutation per epoch."""

    def __init__(self, text: torch.Tensor, batch_size: int, device: torch.device, shuffle: bool = True, seed: int = 0):
        self.text = text.to(device=device, dtype=torch.int64).contiguous()
        self.B, self.shuffle = int(batch_size), shuffle
        self.gen = torch.Generator().manual_seed(int(seed))

    def __len__(self) -> int:
        return self.text.shape[0] // self.B

    def __iter__(self):
        n = len(self)
        order = torch.randperm(self.text.shape[0], generator=self.gen) if self.shuffle else torch.arange(self.text.shape[0])
        order = order.to(self.text.device)
        for b in range(n):
            yield self.text[order[b * self.B:(b + 1) * self.B]].contiguous()


class _StreamLabels:
    """The labels of a ``MultiMNISTStream`` (the canvases are generated and dropped)."""

    def __init__(self, stream):
        self.stream = stream

    def __len__(self) -> int:
        return len(self.stream)

    def __iter__(self):
        for _, text in self.stream:
            yield text


def checkpoint_dict(vae, engine, best_loss: float, n_latents: int) -> dict:
    """multimnist/train_textonly.py:150-155: four keys, the optimizer in ``torch.optim.Adam.state_dict()`` layout."""
    return {'state_dict': vae.state_dict(), 'best_loss': best_loss, 'n_latents': n_latents, 'optimizer': adam_state_dict(vae, engine)}


def main(argv=None) -> dict:
    args = build_parser().parse_args(argv)
    args.cuda = args.cuda and torch.cuda.is_available()
    if not args.cuda:
        raise SystemExit("this engine runs on a gfx950 GPU only: pass --cuda on a machine that has one (no CPU fallback)")
    from . import data as D
    from .multimnist import TextVAE, TextVAETrainer
    from .utils import charlist_tensor, tensor_to_string

    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(args.seed)
    if args.generate:
        from . import multimnist_gen as G
        mn_tr, mn_te = mnist_digit_sources(args)
        train_loader = _StreamLabels(G.MultiMNISTStream(mn_tr[0], mn_tr[1], args.batch_size, dev, epoch_size=args.epoch_size, seed=args.seed,
                                                        min_digits=args.min_digits, max_digits=args.max_digits))
        n_test = max(args.batch_size, min(10000, args.epoch_size // 6))
        _, te_t = G.generate(mn_te[0].to(dev).contiguous(), mn_te[1].to(dev, torch.int64).contiguous(), n_test, seed=args.seed + 7,
                             min_digits=args.min_digits, max_digits=args.max_digits)
        n_train = len(train_loader) * args.batch_size
    else:
        if args.synthetic > 0:
            n_test = max(args.batch_size, args.synthetic // 6)
            _, tr_y = D.synthetic_multimnist(args.synthetic, seed=args.seed)
            _, te_y = D.synthetic_multimnist(n_test, seed=args.seed + 1)
            tr_t = torch.stack([charlist_tensor(l) for l in tr_y]); te_t = torch.stack([charlist_tensor(l) for l in te_y])
        else:
            _, tr_t = D.load_multimnist(args.data, train=True)
            _, te_t = D.load_multimnist(args.data, train=False)
        train_loader = LabelBatcher(tr_t, args.batch_size, dev, shuffle=True, seed=args.seed)
        n_train = len(tr_t)
    test_loader = LabelBatcher(te_t, args.batch_size, dev, shuffle=True, seed=args.seed + 7)
    if len(train_loader) == 0 or len(test_loader) == 0:
        import warnings
        warnings.warn("%d training / %d test samples give no full batch of %d: nothing to do in that phase"
                      % (n_train, len(te_t), args.batch_size))

    vae = TextVAE(args.n_latents, use_cuda=True).cuda()
    trainer = TextVAETrainer(vae, args.batch_size, lr=args.lr, kl_lambda=1e-3, seed=args.seed)

    def train(epoch, kl_lambda):
        vae.train()
        avg, = train_epoch(
            train_loader, lambda text: trainer(text, kl_lambda=kl_lambda).losses()[0:1], args.batch_size, args.log_interval,
            lambda seen, n_total, pct, avg: 'Train Epoch: {} [{}/{} ({:.0f}%)]\tLoss: {:.6f}'.format(epoch, seen, n_total, pct, *avg),
            n_train)            # (the reference prints the size of the data set, not batches times batch size)
        print('====> Epoch: {} Average loss: {:.4f}'.format(epoch, avg))
        return avg

    def test(kl_lambda):
        vae.eval()
        test_loss, = eval_epoch(test_loader, lambda text: trainer.evaluate(text, kl_lambda=kl_lambda).losses()[0:1], 1, dev)
        print('====> Test set loss: {:.4f}'.format(test_loss))
        return test_loss

    schedule = kl_lambdas(1e-3, kl_schedule(), args.epochs, args.anneal_kl)
    best_loss = float(sys.maxsize)
    history = {"train": [], "test": []}
    for epoch in range(1, args.epochs + 1):
        kl_lambda = schedule[epoch - 1]
        history["train"].append(train(epoch, kl_lambda))
        loss = test(kl_lambda)
        history["test"].append(loss)
        is_best = loss < best_loss
        best_loss = min(loss, best_loss)
        save_checkpoint(checkpoint_dict(vae, trainer.engine, best_loss, args.n_latents), is_best, folder=args.out)
        os.makedirs(args.results, exist_ok=True)
        sample = torch.randn(64, args.n_latents, device=dev)
        vae.eval()
        with torch.no_grad():
            words = vae.decoder(sample)                              # (64, 4, 12) log-probs
        text_sample = words.argmax(dim=2).cpu()
        with open(os.path.join(args.results, 'sample_text_epoch%d.txt' % epoch), 'w') as fp:
            for i in range(text_sample.size(0)):
                fp.write('%s\n' % tensor_to_string(text_sample[i]))
    return history


if __name__ == "__main__":
    main()
