"""``train.py``-compatible driver for the MI355X engine.

Mirrors the command line, schedules, meters, checkpoint format and epoch loop of the reference's
``multimnist/train.py`` (flags ``:91-110``, ``AverageMeter`` ``:26-42``, ``save_checkpoint``/``load_checkpoint``
``:44-66``, LR schedule ``:132-137``, KL schedule ``:226-233``, ``train()`` ``:140-183``, ``test()`` ``:185-224``,
checkpoint dict ``:243-251``), with the batch loop body replaced by ONE fused enqueue (``FusedTrainer``).

    python -m multimodal_vae_amd.train --cuda --epochs 2 --synthetic 4096          # no data files needed
    python -m multimodal_vae_amd.train --cuda --data ./data                         # the reference's processed/*.pt
    python -m multimodal_vae_amd.train --cuda --generate --mnist_train A.pt --mnist_test B.pt   # fresh canvases made on the device

Differences that are deliberate: the loader is ``data.DeviceBatcher`` (uint8 H2D + on-device ToTensor, fixed batch
size: the ragged last batch of an epoch is dropped because a fused plan is built per batch size); loss values are read
back every ``--log_interval`` batches only (the reference synchronises three times per batch); sample dumps are written
only when ``--results`` is given (torchvision is not a dependency).
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

from .train_common import (AverageMeter, adam_state_dict, add_generate_flags, eval_epoch, kl_lambdas, kl_schedule,  # noqa: F401
                           mnist_digit_sources, save_checkpoint, train_epoch)

DEFAULT_N_LATENTS = 100


def load_checkpoint(file_path, use_cuda=False):
    """multimnist/train.py:52-66: rebuilds a MultimodalVAE from a checkpoint written by either code base."""
    from .core import load_vae_checkpoint
    from .multimnist import MultimodalVAE
    return load_vae_checkpoint(file_path, MultimodalVAE, use_cuda, DEFAULT_N_LATENTS, use_cuda=use_cuda)


def adjusted_lr(base_lr: float, epoch: int) -> float:
    """multimnist/train.py:132-137"""
    return base_lr * (0.1 ** (epoch // 5))


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser()
    # the reference's flags, same names / defaults (multimnist/train.py:91-108)
    parser.add_argument('--n_latents', type=int, default=100, help='size of the latent embedding (default: 100)')
    parser.add_argument('--batch_size', type=int, default=128, metavar='N', help='input batch size for training (default: 128)')
    parser.add_argument('--epochs', type=int, default=20, metavar='N', help='number of epochs to train (default: 20)')
    parser.add_argument('--lr', type=float, default=1e-3, metavar='LR', help='learning rate (default: 1e-3)')
    parser.add_argument('--log_interval', type=int, default=10, metavar='N', help='how many batches to wait before logging training status')
    parser.add_argument('--anneal_kl', action='store_true', default=False, help='if True, use a fixed interval of doubling the KL term')
    parser.add_argument('--anneal_lr', action='store_true', default=False, help='If True, half learning rate every 5 epochs')
    parser.add_argument('--cuda', action='store_true', default=False, help='enables CUDA training')
    # additions
    parser.add_argument('--data', type=str, default='./data', help="root of the reference's processed/{training,test}.pt")
    parser.add_argument('--synthetic', type=int, default=0, metavar='N', help='train on N synthetic MultiMNIST-shaped samples instead of files')
    parser.add_argument('--out', type=str, default='./trained_models', help='checkpoint folder (reference: ./trained_models)')
    parser.add_argument('--results', type=str, default='', help='folder for per-epoch sample dumps (off when empty)')
    parser.add_argument('--seed', type=int, default=1234)
    # fresh canvases made on the device at every step (multimnist_gen.MultiMNISTStream) instead of a dataset file
    add_generate_flags(parser, 'train on canvases generated on the device from MNIST digits: --mnist_train / --mnist_test, or synthetic digits with --synthetic N')
    return parser


def main(argv=None) -> dict:
    """Single GPU: ``python -m multimodal_vae_amd.train --cuda ...``.  Data parallel (BASELINE configuration 4, one process
    per GPU): ``python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 -m
    multimodal_vae_amd.train --cuda ...`` -- every rank trains on its own shard of the training set with the per-GPU
    ``--batch_size``, gradients are summed over RCCL (1/world inside Adam), rank 0 prints and writes checkpoints, the
    BatchNorm running statistics are averaged over the ranks before every test pass / checkpoint."""
    from . import dp
    dp.ensure_ipc_env()                  # before the first GPU call (torch.cuda.is_available() below is one)
    args = build_parser().parse_args(argv)
    args.cuda = args.cuda and torch.cuda.is_available()
    if not args.cuda:
        raise SystemExit("this engine runs on a gfx950 GPU only: pass --cuda on a machine that has one (no CPU fallback)")
    from . import data as D
    from .multimnist import FusedTrainer, MultimodalVAE
    from .utils import tensor_to_string

    world, local = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        torch.cuda.set_device(local)
    dev = torch.device("cuda", torch.cuda.current_device())
    rank, world, _ = dp.init_distributed("nccl", dev)
    chief = rank == 0
    if not chief:
        global print
        print = lambda *a, **k: None     # noqa: E731  (rank 0 reports)
    torch.manual_seed(args.seed)
    gen_stream = None
    if args.generate:
        # training canvases are made on the device, one kernel in front of every step and never the same twice; the test set is
        # generated once, from the test digits, and goes through the usual loader
        from . import multimnist_gen as G
        mn_tr, mn_te = mnist_digit_sources(args)
        gen_stream = G.MultiMNISTStream(mn_tr[0], mn_tr[1], args.batch_size, dev, epoch_size=args.epoch_size // world,
                                        seed=dp.rank_seed(args.seed, rank), min_digits=args.min_digits, max_digits=args.max_digits)
        n_test = max(args.batch_size * world, min(10000, args.epoch_size // 6))
        te_x, te_t = G.generate(mn_te[0].to(dev).contiguous(), mn_te[1].to(dev, torch.int64).contiguous(), n_test, seed=args.seed + 7,
                                min_digits=args.min_digits, max_digits=args.max_digits)
        te_x, te_t = te_x.cpu(), te_t.cpu()
        tr_x, tr_t = te_x[:0], te_t[:0]          # (nothing is loaded for training)
    elif args.synthetic > 0:
        n_test = max(args.batch_size, args.synthetic // 6)
        tr_x, tr_y = D.synthetic_multimnist(args.synthetic, seed=args.seed)
        te_x, te_y = D.synthetic_multimnist(n_test, seed=args.seed + 1)
        from .utils import charlist_tensor
        tr_t = torch.stack([charlist_tensor(l) for l in tr_y]); te_t = torch.stack([charlist_tensor(l) for l in te_y])
    else:
        tr_x, tr_t = D.load_multimnist(args.data, train=True)
        te_x, te_t = D.load_multimnist(args.data, train=False)
    if world > 1:                        # rank r trains / tests on samples r, r + world, ... (equal shard sizes)
        n_tr, n_te = len(tr_x) // world * world, len(te_x) // world * world
        tr_x, tr_t, te_x, te_t = (t.contiguous() for t in (tr_x[rank:n_tr:world], tr_t[rank:n_tr:world],
                                                           te_x[rank:n_te:world], te_t[rank:n_te:world]))
    train_loader = gen_stream if gen_stream is not None else \
        D.DeviceBatcher(tr_x, tr_t, args.batch_size, dev, shuffle=True, seed=dp.rank_seed(args.seed, rank))
    test_loader = D.DeviceBatcher(te_x, te_t, args.batch_size, dev, shuffle=True, seed=dp.rank_seed(args.seed + 7, rank))

    if len(train_loader) == 0 or len(test_loader) == 0:
        import warnings
        warnings.warn("rank %d: %d training / %d test samples give no full batch of %d: nothing to do in that phase"
                      % (rank, len(tr_x), len(te_x), args.batch_size))

    vae = MultimodalVAE(args.n_latents, use_cuda=True).cuda()
    trainer = FusedTrainer(vae, args.batch_size, lr=args.lr, kl_lambda=1e-3, seed=dp.rank_seed(args.seed, rank), world_size=world,
                           all_reduce=dp.GradAllReduce() if world > 1 else None)
    state = trainer.engine.state
    dp.broadcast_flat(state.params)      # identical replicas (every rank seeds the same initialisation anyway)
    dp.broadcast_flat(state.bn_stats)
    if world > 1:
        state.pack_weights()

    def train(epoch, kl_lambda):
        vae.train()
        avgs = train_epoch(
            train_loader, lambda b: trainer(b[0], b[1], kl_lambda=kl_lambda).losses(), args.batch_size, args.log_interval,
            lambda seen, n_total, pct, avg: 'Train Epoch: {} [{}/{} ({:.0f}%)]\tJoint Loss: {:.6f}\tImage Loss: {:.6f}\tText Loss: {:.6f}'.format(
                epoch, seen, n_total, pct, *avg),
            len(train_loader) * args.batch_size, 3, log=print)          # (this module's print: rank 0 reports)
        print('====> Epoch: {}\tJoint loss: {:.4f}\tImage loss: {:.4f}\tText loss: {:.4f}'.format(epoch, *avgs))
        return avgs

    def ranks_average(acc):
        if world > 1:
            torch.distributed.all_reduce(acc)
            acc = acc / world
        return acc

    def test(kl_lambda):
        vae.eval()
        dp.sync_bn_buffers(state.bn_stats, state.bn_nbt)     # eval (and the checkpoint below) see the ranks' average
        j, i, t = eval_epoch(test_loader, lambda b: trainer.evaluate(b[0], b[1], kl_lambda=kl_lambda).losses(), 3, dev, ranks_average)
        print('====> Test Epoch\tJoint loss: {:.4f}\tImage loss: {:.4f}\tText loss:{:.4f}'.format(j, i, t))
        return j + i + t, (j, i, t)

    # everything allocated so far lives for the whole run: keep the cyclic collector from re-scanning it in the enqueue
    # thread (a generational collection there stalls the GPU for milliseconds; bench.py: 0.959 -> 0.940 ms per step)
    import gc
    gc.collect()
    gc.freeze()
    schedule = kl_lambdas(1e-3, kl_schedule(), args.epochs, args.anneal_kl)
    best_loss = float(sys.maxsize)
    history = {"train": [], "test": []}
    for epoch in range(1, args.epochs + 1):
        kl_lambda = schedule[epoch - 1]
        history["train"].append(train(epoch, kl_lambda))
        loss, (joint_loss, image_loss, text_loss) = test(kl_lambda)
        history["test"].append((joint_loss, image_loss, text_loss))
        if args.anneal_lr:
            trainer.engine.lr = adjusted_lr(args.lr, epoch)
            print('learning rate: {:.4f}'.format(trainer.engine.lr))
        is_best = loss < best_loss
        best_loss = min(loss, best_loss)
        eng = trainer.engine
        if chief:
            save_checkpoint({
                'state_dict': vae.state_dict(),
                'best_loss': best_loss,
                'joint_loss': joint_loss,
                'image_loss': image_loss,
                'text_loss': text_loss,
                'n_latents': args.n_latents,
                # torch.optim.Adam.state_dict() layout, so that optim.Adam(...).load_state_dict() accepts it
                'optimizer': adam_state_dict(vae, eng),
            }, is_best, folder=args.out)
        if args.results and chief:
            os.makedirs(args.results, exist_ok=True)
            sample = torch.randn(64, args.n_latents, device=dev)
            vae.eval()
            with torch.no_grad():
                image_sample = vae.image_decoder(sample).cpu()
                words = vae.text_decoder(sample)                       # (64, 4, 12) log-probs
            torch.save(image_sample.view(64, 1, 50, 50), os.path.join(args.results, 'sample_image_epoch%d.pt' % epoch))
            # the reference samples torch.multinomial from LOG-probabilities (multimnist/model.py:290-296), which modern
            # torch rejects; the dump uses the greedy path the decoder itself feeds back
            text_sample = words.argmax(dim=2).cpu()
            with open(os.path.join(args.results, 'sample_text_epoch%d.txt' % epoch), 'w') as fp:
                for i in range(text_sample.size(0)):
                    fp.write('%s\n' % tensor_to_string(text_sample[i]))
    if world > 1:
        dp.barrier(dev)
        torch.distributed.destroy_process_group()
    return history


if __name__ == "__main__":
    main()
