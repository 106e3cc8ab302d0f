"""``mnist/train_infovae.py``-compatible driver: the MMD-regularised convolutional InfoVAE on MNIST.

Mirrors the command line (``mnist/train_infovae.py:81-93``: ``--n_latents 20 --batch_size 128 --epochs 20 --lr 1e-3 --log_interval 10
--cuda``), the train / test loops with their printed lines (``:115-155``) and the checkpoint dict (``:166-171``: ``state_dict``,
``best_loss``, ``n_latents``, ``optimizer``) of the reference.  The model is ``mnist.InfoVAE``, a plain torch module that trains
through autograd wherever torch runs; the loss is ``mnist.infovae_loss`` (mean squared error + MMD against N(0, I)).

    python -m multimodal_vae_amd.train_infovae_mnist --cuda --conv_backend hip --epochs 2 --synthetic 4096      # no data files needed

``--conv_backend hip`` (needs ``--cuda``) runs each of the four bias-free 4 x 4 stride-2 convolutions with its activation as one
``conv4s2.down4s2`` / ``up4s2`` call: forward, data gradient and weight gradient on bf16 MFMA with fp32 accumulation.  The four
``nn.Linear`` layers, the loss and Adam stay torch ops (on the device the MMD term is the fused op of ``mmd.py``); the checkpoint has
the same ``state_dict`` under either backend.

``--fused`` (needs ``--cuda``) trains ``mnist.FusedInfoVAE`` with ``mnist.InfoVAETrainer``: the batch loop body is ONE enqueue
(csrc/infovae_mnist.hip: the convolutions above, the four Linears on the fp32 MFMA, the loss tail, the MMD sweep beside the decoder,
every gradient) plus one Adam launch.  Same printed lines, checkpoint dict and samples; the fused plan takes whole batches, so a
trailing partial batch of an epoch is left out.  The module route stays the default.

Data: ``--data FILE.pt`` is ``(uint8 (N,28,28), int64 labels (N,))``, the file ``evaluate loglik --dataset mnist`` reads (torchvision's
``processed/training.pt``); the last tenth (at least one batch) is held out for ``test()``.  Or ``--synthetic N``.  Checkpoints go to
``--out``/infovae (the reference: ./trained_models/infovae), per-epoch ``vae.decode(randn(64, n_latents))`` to ``--results`` as
``sample_epoch%d.pt`` ((64,1,28,28) float; torchvision's PNG grid is not a dependency).
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

from .mnist import INFOVAE_BACKENDS, InfoVAE, infovae_loss, set_infovae_backend
from .train import AverageMeter, save_checkpoint


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser()
    # the reference's flags, same names / defaults (mnist/train_infovae.py:81-93)
    parser.add_argument('--n_latents', type=int, default=20, help='size of the latent embedding')
    parser.add_argument('--batch_size', type=int, default=128, metavar='N', help='input batch size for training (default: 128)')
    parser.add_argument('--epochs', type=int, default=20, metavar='N', help='number of epochs to train (default: 20)')
    parser.add_argument('--lr', type=float, default=1e-3, metavar='LR', help='learning rate (default: 1e-3)')
    parser.add_argument('--log_interval', type=int, default=10, metavar='N', help='how many batches to wait before logging training status')
    parser.add_argument('--cuda', action='store_true', default=False, help='enables CUDA training')
    # additions
    parser.add_argument('--conv_backend', choices=INFOVAE_BACKENDS, default='torch',
                        help='convolutions through torch ops or through the HIP 4 x 4 stride-2 op (hip needs --cuda; default: torch)')
    parser.add_argument('--fused', action='store_true', default=False,
                        help='the whole training step as one enqueue of HIP kernels (mnist.FusedInfoVAE + InfoVAETrainer; needs --cuda)')
    parser.add_argument('--data', type=str, default='', metavar='FILE.pt', help='(uint8 images (N,28,28), int64 labels (N,))')
    parser.add_argument('--synthetic', type=int, default=0, metavar='N', help='train on N synthetic MNIST-shaped images instead of a file')
    parser.add_argument('--out', type=str, default='./trained_models', help='checkpoints go to OUT/infovae (reference: ./trained_models/infovae)')
    parser.add_argument('--results', type=str, default='', metavar='DIR', help='folder for per-epoch sample dumps (off when empty)')
    parser.add_argument('--seed', type=int, default=1234)
    return parser


def resolve(args):
    if args.conv_backend == 'hip' and not (args.cuda and torch.cuda.is_available()):
        raise SystemExit('--conv_backend hip runs on the GPU only: pass --cuda on a machine with a gfx950 device (there is no CPU fallback)')
    if args.fused and not (args.cuda and torch.cuda.is_available()):
        raise SystemExit('--fused runs on the GPU only: pass --cuda on a machine with a gfx950 device (there is no CPU fallback)')
    args.cuda = args.cuda and torch.cuda.is_available()
    return args


def train_step(vae, optimizer, data, true_samples=None):
    """one optimisation step on a batch (B,1,28,28) in [0, 1] (mnist/train_infovae.py:123-130); -> the loss, a 0-d tensor"""
    optimizer.zero_grad()
    recon_data, z = vae(data)
    loss = infovae_loss(recon_data, data, z, true_samples)
    loss.backward()
    optimizer.step()
    return loss.detach()


def load_images(args):
    """-> (train, test) uint8 (N,28,28)"""
    from . import data as D
    if args.synthetic > 0:
        return D.synthetic_mnist(args.synthetic, seed=args.seed)[0], D.synthetic_mnist(max(args.batch_size, args.synthetic // 6), seed=args.seed + 1)[0]
    if not args.data:
        raise SystemExit('give --data FILE.pt or --synthetic N')
    x = torch.load(args.data, weights_only=False)[0]
    if x.dtype != torch.uint8 or x.dim() != 3 or tuple(x.shape[1:]) != (28, 28):
        raise ValueError('--data: images must be uint8 (N,28,28) (got %s %s)' % (x.dtype, tuple(x.shape)))
    n_test = max(args.batch_size, len(x) // 10)
    return x[:-n_test], x[-n_test:]


def main(argv=None) -> dict:
    args = resolve(build_parser().parse_args(argv))
    torch.manual_seed(args.seed)
    dev = torch.device('cuda', torch.cuda.current_device()) if args.cuda else torch.device('cpu')
    tr, te = (t.to(dev) for t in load_images(args))                # uint8, resident on the device; a batch is a gather + ToTensor
    gen = torch.Generator().manual_seed(args.seed)

    def batches(images):
        order = torch.randperm(len(images), generator=gen).to(dev)
        for i in range(0, len(images), args.batch_size):
            yield images[order[i:i + args.batch_size]].float().div_(255.0).unsqueeze(1)

    if args.fused:
        from .mnist import FusedInfoVAE, InfoVAETrainer
        from .train_common import adam_state_dict
        if min(len(tr), len(te)) < args.batch_size:
            raise SystemExit('a split has fewer images than one batch of %d (the fused plan takes whole batches)' % args.batch_size)
        vae = FusedInfoVAE(n_latents=args.n_latents).to(dev)
        trainer = InfoVAETrainer(vae, args.batch_size, lr=args.lr, seed=args.seed)
        whole = lambda it: (b for b in it if len(b) == args.batch_size)
        step = lambda data: trainer(data).total()
        test_loss_of = lambda data: trainer.evaluate(data).total()
        optimizer_state = lambda: adam_state_dict(vae, trainer.engine)
    else:
        vae = set_infovae_backend(InfoVAE(n_latents=args.n_latents), args.conv_backend).to(dev)
        optimizer = torch.optim.Adam(vae.parameters(), lr=args.lr)
        whole = lambda it: it
        step = lambda data: train_step(vae, optimizer, data)

        def test_loss_of(data):
            recon_data, z = vae(data)
            return infovae_loss(recon_data, data, z)
        optimizer_state = optimizer.state_dict
    n_batches = (len(tr) + args.batch_size - 1) // args.batch_size

    def train(epoch):
        vae.train()
        loss_meter = AverageMeter()
        pending = []

        def drain():
            for v, n in pending:                                   # one wait per log interval, not one per batch
                loss_meter.update(float(v), n)
            pending.clear()

        for batch_idx, data in enumerate(whole(batches(tr))):
            pending.append((step(data), len(data)))
            if batch_idx % args.log_interval == 0:
                drain()
                print('Train Epoch: {} [{}/{} ({:.0f}%)]\tLoss: {:.6f}'.format(
                    epoch, batch_idx * len(data), len(tr), 100. * batch_idx / n_batches, loss_meter.avg))
        drain()
        print('====> Epoch: {}\tLoss: {:.4f}'.format(epoch, loss_meter.avg))
        return loss_meter.avg

    @torch.no_grad()
    def test():
        vae.eval()
        test_loss, n = torch.zeros((), device=dev), 0
        for data in whole(batches(te)):
            test_loss += test_loss_of(data)
            n += 1
        test_loss = float(test_loss) / n
        print('====> Test Epoch\tLoss: {:.4f}'.format(test_loss))
        return test_loss

    folder = os.path.join(args.out, 'infovae')
    os.makedirs(folder, exist_ok=True)
    best_loss = float(sys.maxsize)
    history = {"train": [], "test": []}
    for epoch in range(1, args.epochs + 1):
        history["train"].append(train(epoch))
        loss = test()
        history["test"].append(loss)
        is_best = loss < best_loss
        best_loss = min(loss, best_loss)
        save_checkpoint({
            'state_dict': vae.state_dict(),
            'best_loss': best_loss,
            'n_latents': args.n_latents,
            'optimizer': optimizer_state(),
        }, is_best, folder=folder)
        if args.results:
            os.makedirs(args.results, exist_ok=True)
            vae.eval()
            with torch.no_grad():
                sample = vae.decode(torch.randn(64, args.n_latents, device=dev))
            torch.save(sample.cpu().view(64, 1, 28, 28), os.path.join(args.results, 'sample_epoch%d.pt' % epoch))
    history["checkpoint"] = os.path.join(folder, 'checkpoint.pth.tar')
    return history


if __name__ == "__main__":
    main()
