"""``coco/train_infovae.py``-compatible driver: the MMD-regularised InfoVAE on COCO images.

Mirrors the command line (``coco/train_infovae.py:61-72``: ``--n_latents 100 --batch_size 128 --epochs 10 --lr 1e-4
--log_interval 10 --cuda``), the train / test loops with their printed lines (``:113-147``) and the checkpoint dict
(``:158-163``: ``state_dict``, ``best_loss``, ``n_latents``, ``optimizer``) of the reference.  The model is ``coco.InfoVAE`` (the HIP
image encoder and decoder), the loss ``coco.infovae_loss`` (BCE kernel + the fused MMD op), the optimizer ``torch.optim.Adam`` over
the module's own parameters, as in the reference.  With ``--fused`` the model is ``coco.FusedInfoVAE`` and the batch loop body is ONE
enqueue (``coco.InfoVAETrainer``: the one-pass image step with the MMD sweep beside the decoder and the packed-gradient Adam): the
same flags, printed lines, samples and checkpoint keys; whole batches only (a short last batch is dropped, the plan has one size).

    python -m multimodal_vae_amd.train_infovae --cuda --epochs 2 --synthetic 4096      # no data files needed
    python -m multimodal_vae_amd.train_infovae --cuda --fused --epochs 2 --synthetic 4096

Inputs, as ``train_coco``: ``--data DIR`` with ``images_u8.pt`` ((N,3,32,32) uint8: Scale(32) + CenterCrop(32); the captions are
not read) or ``--synthetic N``.  The images stay on the device as uint8; a batch is a gather of a device permutation + ToTensor.
Checkpoints go to ``--out``/infovae (the reference: ./trained_models/infovae), per-epoch samples of ``vae.decode`` to
``--results`` as ``sample_epoch%d.pt`` ((64,3,32,32) float; torchvision's PNG grid is not a dependency).
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

from .train import AverageMeter, save_checkpoint
from .train_common import adam_state_dict, eval_epoch, train_epoch


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser()
    # the reference's flags, same names / defaults (coco/train_infovae.py:61-72)
    parser.add_argument('--n_latents', type=int, default=100, help='size of the latent embedding (default: 100)')
    parser.add_argument('--batch_size', type=int, default=128, metavar='N', help='input batch size for training (default: 128)')
    parser.add_argument('--epochs', type=int, default=10, metavar='N', help='number of epochs to train (default: 10)')
    parser.add_argument('--lr', type=float, default=1e-4, metavar='LR', help='learning rate (default: 1e-4)')
    parser.add_argument('--log_interval', type=int, default=10, metavar='N', help='how many batches to wait before logging training status (default: 10)')
    parser.add_argument('--cuda', action='store_true', default=False, help='enables CUDA training')
    # additions, with their meaning in train_coco
    parser.add_argument('--data', type=str, default='./data/coco', help='folder with images_u8.pt')
    parser.add_argument('--synthetic', type=int, default=0, metavar='N', help='train on N synthetic COCO-shaped images instead of files')
    parser.add_argument('--out', type=str, default='./trained_models', help='checkpoints go to OUT/infovae (reference: ./trained_models/infovae)')
    parser.add_argument('--results', type=str, default='', help='folder for per-epoch sample dumps (off when empty)')
    parser.add_argument('--seed', type=int, default=1234)
    parser.add_argument('--fused', action='store_true', default=False,
                        help='train a FusedInfoVAE with the one-enqueue step (InfoVAETrainer) instead of modules + torch.optim.Adam')
    return parser


def load_checkpoint(file_path, use_cuda=False, fused=False):
    """coco/train_infovae.py:30-41: rebuilds an InfoVAE (``fused``: a FusedInfoVAE) from the checkpoint dict this driver writes on
    either route, or the reference's: the two classes have the same state-dict keys."""
    from .coco import FusedInfoVAE, InfoVAE
    checkpoint = torch.load(file_path, map_location=None if use_cuda else 'cpu', weights_only=False)
    vae = (FusedInfoVAE if fused else InfoVAE)(n_latents=checkpoint['n_latents'])
    vae.load_state_dict(checkpoint['state_dict'])
    if use_cuda:
        vae.cuda()
    return vae


class _DeviceImages:
    """(N,3,32,32) uint8 images resident on the device -> fp32 batches in [0, 1] (ToTensor), shuffled per epoch from ``seed``.
    The last batch may be short, as with the reference's DataLoader."""

    def __init__(self, images_u8: torch.Tensor, batch_size: int, device, shuffle=True, seed=0):
        assert images_u8.dtype == torch.uint8 and tuple(images_u8.shape[1:]) == (3, 32, 32), "expected (N,3,32,32) uint8 images"
        self.images = images_u8.to(device)
        self.B, self.shuffle, self.epoch = int(batch_size), shuffle, 0
        self.gen = torch.Generator().manual_seed(seed)

    def __len__(self):
        return (len(self.images) + self.B - 1) // self.B

    @property
    def n(self):
        return len(self.images)

    def __iter__(self):
        n = len(self.images)
        order = (torch.randperm(n, generator=self.gen) if self.shuffle else torch.arange(n)).to(self.images.device)
        for i in range(0, n, self.B):
            yield self.images[order[i:i + self.B]].float().div_(255.0)


def main(argv=None) -> dict:
    args = build_parser().parse_args(argv)
    args.cuda = args.cuda and torch.cuda.is_available()
    if not args.cuda:
        raise SystemExit("this engine runs on a gfx950 GPU only: pass --cuda on a machine that has one (no CPU fallback)")
    from .train_coco import synthetic_coco

    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(args.seed)
    if args.synthetic > 0:
        n_test = max(args.batch_size, args.synthetic // 6)
        tr_x = synthetic_coco(args.synthetic, seed=args.seed)[0]
        te_x = synthetic_coco(n_test, seed=args.seed + 1)[0]
    else:
        tr_x = torch.load(os.path.join(args.data, "images_u8.pt"))
        n_test = max(args.batch_size, len(tr_x) // 10)
        te_x, tr_x = tr_x[:n_test], tr_x[n_test:]
    vae, train, test, optimizer_state = (_fused_route if args.fused else _module_route)(args, dev, tr_x, te_x)

    folder = os.path.join(args.out, 'infovae')
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
            sample = torch.randn(64, args.n_latents, device=dev)
            vae.eval()
            with torch.no_grad():
                torch.save(vae.decode(sample).cpu().view(64, 3, 32, 32), os.path.join(args.results, 'sample_epoch%d.pt' % epoch))
    history["checkpoint"] = os.path.join(folder, 'checkpoint.pth.tar')
    return history


def _module_route(args, dev, tr_x, te_x):
    """-> (vae, train(epoch), test(), optimizer_state()): ``InfoVAE`` + ``infovae_loss`` + ``torch.optim.Adam``, as the reference."""
    from .coco import InfoVAE, infovae_loss
    train_loader = _DeviceImages(tr_x, args.batch_size, dev, shuffle=True, seed=args.seed)
    test_loader = _DeviceImages(te_x, args.batch_size, dev, shuffle=True, seed=args.seed + 7)

    vae = InfoVAE(n_latents=args.n_latents).cuda()
    optimizer = torch.optim.Adam(vae.parameters(), lr=args.lr)

    def train(epoch):
        vae.train()
        loss_meter = AverageMeter()
        pending = []

        def drain():
            for v, n in pending:                                   # one wait per log interval, not one per batch
                loss_meter.update(float(v), n)
            pending.clear()

        for batch_idx, data in enumerate(train_loader):
            optimizer.zero_grad()
            recon_data, z = vae(data)
            loss = infovae_loss(recon_data, data, z)
            pending.append((loss.detach(), len(data)))
            loss.backward()
            optimizer.step()
            if batch_idx % args.log_interval == 0:
                drain()
                print('Train Epoch: {} [{}/{} ({:.0f}%)]\tLoss: {:.6f}'.format(
                    epoch, batch_idx * len(data), train_loader.n, 100. * batch_idx / len(train_loader), loss_meter.avg))
        drain()
        print('====> Epoch: {} Average loss: {:.4f}'.format(epoch, loss_meter.avg))
        return loss_meter.avg

    @torch.no_grad()
    def test():
        vae.eval()
        test_loss = torch.zeros((), device=dev)
        for data in test_loader:
            recon_data, z = vae(data)
            test_loss += infovae_loss(recon_data, data, z)
        test_loss = float(test_loss) / len(test_loader)
        print('====> Test set loss: {:.4f}'.format(test_loss))
        return test_loss

    return vae, train, test, optimizer.state_dict


def _fused_route(args, dev, tr_x, te_x):
    """-> (vae, train(epoch), test(), optimizer_state()): ``InfoVAETrainer`` on a ``FusedInfoVAE``, one enqueue per batch."""
    from . import data as D
    from .coco import FusedInfoVAE, InfoVAETrainer
    for name, x in (("training", tr_x), ("test", te_x)):
        if len(x) < args.batch_size:
            raise SystemExit("the %s split has %d images, fewer than one batch of %d (the fused plan takes whole batches)"
                             % (name, len(x), args.batch_size))
    none = lambda x: torch.zeros(len(x), dtype=torch.int64)          # the batcher carries a second tensor: nothing reads it
    train_loader = D.DeviceBatcher(tr_x, none(tr_x), args.batch_size, dev, shuffle=True, seed=args.seed)
    test_loader = D.DeviceBatcher(te_x, none(te_x), args.batch_size, dev, shuffle=True, seed=args.seed + 7)
    vae = FusedInfoVAE(n_latents=args.n_latents).cuda()
    trainer = InfoVAETrainer(vae, args.batch_size, lr=args.lr, seed=args.seed)

    def train(epoch):
        vae.train()
        avg, = train_epoch(
            train_loader, lambda b: trainer(b[0]).total(), args.batch_size, args.log_interval,
            lambda seen, n_total, pct, avg: 'Train Epoch: {} [{}/{} ({:.0f}%)]\tLoss: {:.6f}'.format(epoch, seen, n_total, pct, *avg),
            len(train_loader) * args.batch_size)
        print('====> Epoch: {} Average loss: {:.4f}'.format(epoch, avg))
        return avg

    def test():
        vae.eval()
        test_loss, = eval_epoch(test_loader, lambda b: trainer.evaluate(b[0]).total(), 1, dev)
        print('====> Test set loss: {:.4f}'.format(test_loss))
        return test_loss

    return vae, train, test, lambda: adam_state_dict(vae, trainer.engine, own_only=True)


if __name__ == "__main__":
    main()
