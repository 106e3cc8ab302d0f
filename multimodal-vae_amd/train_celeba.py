"""``celeba/train.py``-compatible driver for the MI355X engine.

Mirrors the command line (``celeba/train.py:86-99``: ``--n_latents 100 --batch_size 128 --epochs 20 --lr 1e-3 --log_interval 10
--cuda``), the epoch loop, the printed lines and the checkpoint dict (``:204-219``) of the reference, with the batch loop body
(``:130-154``) replaced by ONE fused enqueue (``celeba.FusedTrainer``) and the ``DataLoader`` by ``data.DeviceBatcher``; ToTensor runs
on the device.  As the reference does, it trains on ``train`` and tests on ``val``.

    python -m multimodal_vae_amd.make_celeba --root ./data                        # once: celeba_{train,val,test}.pt
    python -m multimodal_vae_amd.train_celeba --cuda --data ./data
    python -m multimodal_vae_amd.train_celeba --cuda --epochs 2 --synthetic 4096  # no data files needed

``--anneal_kl`` is the KL schedule of the other drivers (``multimnist/train.py``); the reference's CelebA script keeps 1e-3.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

from .train_common import adam_state_dict, eval_epoch, kl_lambdas, kl_schedule, save_checkpoint, train_epoch


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser()
    # the reference's flags, same names / defaults (celeba/train.py:86-99)
    parser.add_argument('--n_latents', type=int, default=100, help='size of the latent embedding (default: 100)')
    parser.add_argument('--batch_size', type=int, default=128, metavar='N', help='input batch size for training (default: 128)')
    parser.add_argument('--epochs', type=int, default=20, metavar='N', help='number of epochs to train (default: 20)')
    parser.add_argument('--lr', type=float, default=1e-3, metavar='LR', help='learning rate (default: 1e-3)')
    parser.add_argument('--log_interval', type=int, default=10, metavar='N', help='how many batches to wait before logging training status')
    parser.add_argument('--cuda', action='store_true', default=False, help='enables CUDA training')
    # additions
    parser.add_argument('--anneal_kl', action='store_true', default=False, help='if True, use a fixed interval of doubling the KL term')
    parser.add_argument('--data', type=str, default='./data', metavar='DIR', help='folder with celeba_train.pt and celeba_val.pt (make_celeba)')
    parser.add_argument('--synthetic', type=int, default=0, metavar='N', help='train on N synthetic CelebA-shaped samples instead of files')
    parser.add_argument('--out', type=str, default='./trained_models', help='checkpoint folder (reference: ./trained_models)')
    parser.add_argument('--results', type=str, default='', help='folder for per-epoch sample dumps (off when empty)')
    parser.add_argument('--seed', type=int, default=1234)
    return parser


def main(argv=None) -> dict:
    args = build_parser().parse_args(argv)
    args.cuda = args.cuda and torch.cuda.is_available()
    if not args.cuda:
        raise SystemExit("this engine runs on a gfx950 GPU only: pass --cuda on a machine that has one (no CPU fallback)")
    from . import data as D
    from .celeba import FusedTrainer, MultimodalVAE, tensor_to_attributes
    from .evaluate import load_celeba_eval_file

    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(args.seed)
    if args.synthetic > 0:
        tr_x, tr_a = D.synthetic_celeba(args.synthetic, seed=args.seed)
        te_x, te_a = D.synthetic_celeba(max(args.batch_size, args.synthetic // 6), seed=args.seed + 1)
    else:
        tr_x, tr_a = load_celeba_eval_file(os.path.join(args.data, "celeba_train.pt"))
        te_x, te_a = load_celeba_eval_file(os.path.join(args.data, "celeba_val.pt"))
    for name, x in (("training", tr_x), ("test (val)", te_x)):
        if len(x) < args.batch_size:
            raise SystemExit("the %s split has %d images, fewer than one batch of %d (the fused plan takes whole batches)"
                             % (name, len(x), args.batch_size))
    train_loader = D.DeviceBatcher(tr_x, tr_a, args.batch_size, dev, shuffle=True, seed=args.seed)
    test_loader = D.DeviceBatcher(te_x, te_a, args.batch_size, dev, shuffle=True, seed=args.seed + 7)

    vae = MultimodalVAE(args.n_latents, use_cuda=True)
    vae.weight_init(mean=0.0, std=0.02)
    vae.cuda()
    trainer = FusedTrainer(vae, args.batch_size, lr=args.lr, kl_lambda=1e-3, seed=args.seed)

    def train(epoch, kl_lambda):
        vae.train()
        avgs = train_epoch(
            train_loader, lambda b: trainer(b[0], b[1], kl_lambda=kl_lambda).losses(), args.batch_size, args.log_interval,
            lambda seen, n_total, pct, avg: 'Train Epoch: {} [{}/{} ({:.0f}%)]\tJoint Loss: {:.6f}\tImage Loss: {:.6f}\tAttrs Loss: {:.6f}'.format(
                epoch, seen, n_total, pct, *avg),
            len(train_loader) * args.batch_size, 3)
        print('====> Epoch: {}\tJoint loss: {:.4f}\tImage loss: {:.4f}\tAttrs loss: {:.4f}'.format(epoch, *avgs))
        return avgs

    def test(kl_lambda):
        vae.eval()
        j, i, a = eval_epoch(test_loader, lambda b: trainer.evaluate(b[0], b[1], kl_lambda=kl_lambda).losses(), 3, dev)
        print('====> Test Epoch\tJoint loss: {:.4f}\tImage loss: {:.4f}\tAttrs loss:{:.4f}'.format(j, i, a))
        return j + i + a, (j, i, a)

    # everything allocated so far lives for the whole run: keep the cyclic collector from re-scanning it in the enqueue thread
    import gc
    gc.collect()
    gc.freeze()
    schedule = kl_lambdas(1e-3, kl_schedule(), args.epochs, args.anneal_kl)
    best_loss = float(sys.maxsize)
    history = {"train": [], "test": []}
    for epoch in range(1, args.epochs + 1):
        kl_lambda = schedule[epoch - 1]
        history["train"].append(train(epoch, kl_lambda))
        loss, (joint_loss, image_loss, attrs_loss) = test(kl_lambda)
        history["test"].append((joint_loss, image_loss, attrs_loss))
        is_best = loss < best_loss
        best_loss = min(loss, best_loss)
        save_checkpoint({
            'state_dict': vae.state_dict(),
            'best_loss': best_loss,
            'joint_loss': joint_loss,
            'image_loss': image_loss,
            'attrs_loss': attrs_loss,
            'n_latents': args.n_latents,
            'optimizer': adam_state_dict(vae, trainer.engine),
        }, is_best, folder=args.out)
        if args.results:
            # celeba/train.py:221-238, the tensor instead of a PNG grid (no torchvision here)
            os.makedirs(args.results, exist_ok=True)
            sample = torch.randn(64, args.n_latents, device=dev)
            vae.eval()
            with torch.no_grad():
                torch.save(vae.image_decoder(sample).cpu().view(64, 3, 64, 64), os.path.join(args.results, 'sample_image_epoch%d.pt' % epoch))
                attrs_sample = vae.attrs_decoder(sample).cpu()
            with open(os.path.join(args.results, 'sample_attrs_epoch%d.txt' % epoch), 'w') as fp:
                for row in attrs_sample:
                    fp.write('%s\n' % ','.join(tensor_to_attributes(row)))
    return history


if __name__ == "__main__":
    main()
