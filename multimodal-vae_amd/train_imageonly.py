"""``celeba/train_imageonly.py`` / ``coco/train_imageonly.py`` / ``multimnist/train_imageonly.py`` /
``mnist/imageonly/train_imageonly.py``-compatible driver of the uni-modal image baselines.

Per data set the reference script's command line, defaults, printed lines, KL schedule and checkpoint dict (``state_dict``,
``best_loss``, ``n_latents``, ``optimizer``), with the batch loop body replaced by ONE fused enqueue (``ImageVAETrainer``: one pass
over B rows, no product of experts) and the ``DataLoader`` by ``data.DeviceBatcher``:

    celeba (celeba/train_imageonly.py:57-70,141-153): --n_latents 100 --lr 1e-3, kl_lambda 1e-3 throughout
    coco   (coco/train_imageonly.py:45-60,141-162):   --n_latents 20 --lr 1e-4 [--anneal_kl], kl_lambda 5e-4, or with --anneal_kl
                                                      1e-5, 1e-4, 1e-3 advancing every 5 epochs
    multimnist (multimnist/train_imageonly.py:46-60,131-139): --n_latents 20 --lr 1e-3 [--anneal_kl], kl_lambda 1e-3, or with
                                                      --anneal_kl 1e-5 ... 1.0 advancing every 5 epochs; test loss = mean over batches
    mnist  (mnist/imageonly/train_imageonly.py:60-71,77-89): --n_latents 20 --lr 1e-3 --epochs 20, loss (BCE + KLD / 784) / B throughout,
                                                      checkpoints in ./trained_models, ``sample_image.pt`` (64 prior samples) in ./results
                                                      whenever the test loss reaches a new best

    python -m multimodal_vae_amd.train_imageonly --dataset celeba --cuda --data ./data
    python -m multimodal_vae_amd.train_imageonly --dataset coco --cuda --epochs 2 --synthetic 4096   # no data files needed
    python -m multimodal_vae_amd.train_imageonly --dataset multimnist --cuda --data ./data           # images of processed/*.pt
    python -m multimodal_vae_amd.train_imageonly --dataset multimnist --cuda --generate --mnist_train A.pt --mnist_test B.pt
    python -m multimodal_vae_amd.train_imageonly --dataset mnist --cuda --data mnist_train.pt [--test_data mnist_test.pt]

After each epoch 64 prior samples are written as ``sample_image_epochN.pt`` (the tensor, not a PNG grid: no torchvision here).
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

from .train_common import add_generate_flags, adam_state_dict, eval_epoch, kl_schedule, mnist_digit_sources, save_checkpoint, train_epoch
from .train_common import kl_lambdas as _kl_lambdas

DATASETS = {
    #          n_latents  lr    kl_lambda  side
    "celeba": (100, 1e-3, 1e-3, 64),
    "coco": (20, 1e-4, 5e-4, 32),
    "multimnist": (20, 1e-3, 1e-3, 50),
    "mnist": (20, 1e-3, 1.0 / 784, 28),         # (BCE + KLD / 784) / B: the 1 / B sits in the trainer's lambda_x
}
CHANNELS = {"celeba": 3, "coco": 3, "multimnist": 1, "mnist": 1}
# epochs, checkpoint folder, results folder where the reference script's differ from the others' (mnist/imageonly/train_imageonly.py:81,92-96)
FOLDERS = {"mnist": (20, './trained_models', './results')}
COCO_KL_SCHEDULE = (1e-5, 1e-4, 1e-3)       # coco/train_imageonly.py:142
KL_SCHEDULES = {"coco": COCO_KL_SCHEDULE, "multimnist": tuple(kl_schedule())}      # multimnist/train_imageonly.py:132


def build_parser(dataset: str) -> argparse.ArgumentParser:
    n_latents, lr, _, _ = DATASETS[dataset]
    epochs, out, results = FOLDERS.get(dataset, (10, './trained_models/image_only', './results/image_only'))
    parser = argparse.ArgumentParser()
    parser.add_argument('--dataset', choices=sorted(DATASETS), default=dataset)
    # the reference's flags, same names / defaults
    parser.add_argument('--n_latents', type=int, default=n_latents, help='size of the latent embedding')
    parser.add_argument('--batch_size', type=int, default=128, metavar='N', help='input batch size for training (default: 128)')
    parser.add_argument('--epochs', type=int, default=epochs, metavar='N', help='number of epochs to train (default: %d)' % epochs)
    parser.add_argument('--lr', type=float, default=lr, metavar='LR', help='learning rate (default: %g)' % lr)
    parser.add_argument('--log_interval', type=int, default=10, metavar='N', help='how many batches to wait before logging training status')
    if dataset in KL_SCHEDULES:
        parser.add_argument('--anneal_kl', action='store_true', default=False, help='if True, use a fixed interval of doubling the KL term')
    parser.add_argument('--cuda', action='store_true', default=False, help='enables CUDA training')
    # additions, as train_celeba / train_coco
    parser.add_argument('--data', type=str, default='./data', metavar='DIR',
                        help='celeba: folder with celeba_{train,val}.pt (make_celeba); coco: folder with images_u8.pt (as train_coco); '
                             "multimnist: root of the reference's processed/{training,test}.pt (images only); "
                             'mnist: a .pt FILE holding (uint8 (N,28,28), int64 (N,)), the file `evaluate loglik --dataset mnist` reads')
    parser.add_argument('--synthetic', type=int, default=0, metavar='N', help='train on N synthetic samples instead of files')
    parser.add_argument('--out', type=str, default=out, help='checkpoint folder (reference: %s)' % out)
    parser.add_argument('--results', type=str, default=results, help='folder of the sample dumps (off when empty)')
    parser.add_argument('--seed', type=int, default=1234)
    if dataset == "multimnist":         # as train.py / train_textonly_multimnist.py
        add_generate_flags(parser, 'canvases generated on the device: --mnist_train / --mnist_test, or synthetic digits with --synthetic N')
    if dataset == "mnist":
        parser.add_argument('--test_data', type=str, default='', metavar='FILE',
                            help='the test split, same layout as --data (default: the first tenth of --data is held out)')
    return parser


def dataset_of(argv) -> str:
    """The value of ``--dataset`` (it selects the other flags' defaults, so it is looked at first)."""
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument('--dataset', choices=sorted(DATASETS), default='celeba')
    return pre.parse_known_args(argv)[0].dataset


def kl_lambdas(dataset: str, epochs: int, anneal_kl: bool = False):
    """kl_lambda of epochs 1..epochs.  celeba: loss_function's default throughout (celeba/train_imageonly.py:42,114); coco: 5e-4, or
    with --anneal_kl the next value of 1e-5, 1e-4, 1e-3 every 5 epochs, the last one kept (coco/train_imageonly.py:141-149); multimnist:
    1e-3, or with --anneal_kl the next value of 1e-5 ... 1.0 every 5 epochs (multimnist/train_imageonly.py:131-139)."""
    return _kl_lambdas(DATASETS[dataset][2], KL_SCHEDULES.get(dataset, ()), epochs, anneal_kl)


def image_adam_state_dict(vae, engine) -> dict:
    """The engine's flat Adam moments of the uni-modal model's own parameters as a ``torch.optim.Adam.state_dict()``."""
    return adam_state_dict(vae, engine, own_only=True)


def checkpoint_dict(vae, engine, best_loss, n_latents) -> dict:
    """celeba/train_imageonly.py:148-153"""
    return {'state_dict': vae.state_dict(), 'best_loss': best_loss, 'n_latents': n_latents,
            'optimizer': image_adam_state_dict(vae, engine)}


class _StreamImages:
    """The canvases of a ``MultiMNISTStream`` (the labels are generated and dropped)."""

    def __init__(self, stream):
        self.stream = stream

    def __len__(self) -> int:
        return len(self.stream)

    def __iter__(self):
        for image, _ in self.stream:
            yield image, None


def _multimnist_loaders(args, dev):
    """(train_loader, test images) of the MultiMNIST baseline: only the images of a data set are read."""
    from . import data as D
    if args.generate:
        from . import multimnist_gen as G
        mn_tr, mn_te = mnist_digit_sources(args)
        stream = G.MultiMNISTStream(mn_tr[0], mn_tr[1], args.batch_size, dev, epoch_size=args.epoch_size, seed=args.seed,
                                    min_digits=args.min_digits, max_digits=args.max_digits)
        n_test = max(args.batch_size, min(10000, args.epoch_size // 6))
        te_x, _ = G.generate(mn_te[0].to(dev).contiguous(), mn_te[1].to(dev, torch.int64).contiguous(), n_test, seed=args.seed + 7,
                             min_digits=args.min_digits, max_digits=args.max_digits)
        return _StreamImages(stream), te_x.cpu()
    if args.synthetic > 0:
        return (D.synthetic_multimnist(args.synthetic, seed=args.seed)[0],
                D.synthetic_multimnist(max(args.batch_size, args.synthetic // 6), seed=args.seed + 1)[0])
    return D.load_multimnist(args.data, train=True)[0], D.load_multimnist(args.data, train=False)[0]


def _load_images(args):
    from . import data as D
    if args.dataset == "mnist":         # only the images are read
        if args.synthetic > 0:
            return (D.synthetic_mnist(args.synthetic, seed=args.seed)[0],
                    D.synthetic_mnist(max(args.batch_size, args.synthetic // 6), seed=args.seed + 1)[0])
        from .make_multimnist import load_mnist_pt
        if not os.path.isfile(args.data):
            raise SystemExit("--dataset mnist: --data must name a .pt file holding (uint8 (N,28,28), int64 (N,)), or give --synthetic N")
        x = load_mnist_pt(args.data)[0]
        if args.test_data:
            return x, load_mnist_pt(args.test_data)[0]
        n_test = max(args.batch_size, len(x) // 10)
        return x[n_test:], x[:n_test]
    if args.dataset == "celeba":
        from .evaluate import load_celeba_eval_file
        if args.synthetic > 0:
            return (D.synthetic_celeba(args.synthetic, seed=args.seed)[0],
                    D.synthetic_celeba(max(args.batch_size, args.synthetic // 6), seed=args.seed + 1)[0])
        return (load_celeba_eval_file(os.path.join(args.data, "celeba_train.pt"))[0],
                load_celeba_eval_file(os.path.join(args.data, "celeba_val.pt"))[0])
    from .train_coco import synthetic_coco
    if args.synthetic > 0:
        return (synthetic_coco(args.synthetic, seed=args.seed)[0],
                synthetic_coco(max(args.batch_size, args.synthetic // 6), seed=args.seed + 1)[0])
    x = torch.as_tensor(torch.load(os.path.join(args.data, "images_u8.pt"), weights_only=False))      # as train_coco: the first tenth is the test split
    n_test = max(args.batch_size, len(x) // 10)
    return x[n_test:], x[:n_test]


def main(argv=None) -> dict:
    argv = sys.argv[1:] if argv is None else list(argv)
    args = build_parser(dataset_of(argv)).parse_args(argv)
    args.cuda = args.cuda and torch.cuda.is_available()
    if not args.cuda:
        raise SystemExit("this engine runs on a gfx950 GPU only: pass --cuda on a machine that has one (no CPU fallback)")
    import importlib
    from . import data as D
    M = importlib.import_module("." + args.dataset, __package__)
    side, channels = DATASETS[args.dataset][3], CHANNELS[args.dataset]

    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(args.seed)
    tr_x, te_x = _multimnist_loaders(args, dev) if args.dataset == "multimnist" else _load_images(args)
    stream = tr_x if isinstance(tr_x, _StreamImages) else None
    ishape = (side, side) if channels == 1 else (channels, side, side)       # MultiMNIST files hold (N,50,50): the batcher adds the channel
    for name, x in (("training", tr_x), ("test (val)", te_x)):
        if x is stream:
            continue
        if x.dtype != torch.uint8 or tuple(x.shape[1:]) != ishape:
            raise SystemExit("the %s images must be uint8 %s (got %s %s)" % (name, ("N",) + ishape, x.dtype, tuple(x.shape)))
        if len(x) < args.batch_size:
            raise SystemExit("the %s split has %d images, fewer than one batch of %d (the fused plan takes whole batches)"
                             % (name, len(x), args.batch_size))
    none = lambda x: torch.zeros(len(x), dtype=torch.int64)          # the batcher carries a second tensor: nothing reads it
    train_loader = stream if stream is not None else D.DeviceBatcher(tr_x, none(tr_x), args.batch_size, dev, shuffle=True, seed=args.seed)
    test_loader = D.DeviceBatcher(te_x, none(te_x), args.batch_size, dev, shuffle=True, seed=args.seed + 7)

    vae = M.ImageVAE(n_latents=args.n_latents)
    if args.dataset == "celeba":
        vae.weight_init(mean=0.0, std=0.02)
    vae.cuda()
    trainer = M.ImageVAETrainer(vae, args.batch_size, lr=args.lr, kl_lambda=DATASETS[args.dataset][2], seed=args.seed)

    def train(epoch, kl_lambda):
        if args.dataset in KL_SCHEDULES:
            print('Using KL Lambda: {}'.format(kl_lambda))
        vae.train()
        avg, = train_epoch(
            train_loader, lambda b: trainer(b[0], kl_lambda=kl_lambda).losses()[0], args.batch_size, args.log_interval,
            lambda seen, n_total, pct, avg: 'Train Epoch: {} [{}/{} ({:.0f}%)]\tLoss: {:.6f}'.format(epoch, seen, n_total, pct, *avg),
            len(train_loader) * args.batch_size)
        print('====> Epoch: {} Average loss: {:.4f}'.format(epoch, avg))
        return avg

    def test(kl_lambda):
        vae.eval()
        test_loss, = eval_epoch(test_loader, lambda b: trainer.evaluate(b[0], kl_lambda=kl_lambda).losses()[0], 1, dev)
        print('====> Test set loss: {:.4f}'.format(test_loss))
        return test_loss

    best_loss = float(sys.maxsize)
    history = {"train": [], "test": [], "kl_lambda": []}
    schedule = kl_lambdas(args.dataset, args.epochs, bool(getattr(args, "anneal_kl", False)))
    for epoch in range(1, args.epochs + 1):
        kl_lambda = schedule[epoch - 1]
        history["kl_lambda"].append(kl_lambda)
        history["train"].append(train(epoch, kl_lambda))
        loss = test(kl_lambda)
        history["test"].append(loss)
        is_best = loss < best_loss
        best_loss = min(loss, best_loss)
        save_checkpoint(checkpoint_dict(vae, trainer.engine, best_loss, args.n_latents), is_best, folder=args.out)
        if args.results and args.dataset == "mnist":      # mnist/imageonly/train_imageonly.py:166-173: on a new best only; n_latents columns
            if is_best:
                os.makedirs(args.results, exist_ok=True)
                vae.eval()
                with torch.no_grad():
                    torch.save(vae.decode(torch.randn(64, args.n_latents, device=dev)).cpu().view(64, 1, 28, 28),
                               os.path.join(args.results, 'sample_image.pt'))
        elif args.results:
            os.makedirs(args.results, exist_ok=True)
            sample = torch.randn(64, args.n_latents, device=dev)
            vae.eval()
            with torch.no_grad():
                torch.save(vae.decode(sample).cpu().view(64, channels, side, side), os.path.join(args.results, 'sample_image_epoch%d.pt' % epoch))
    return history


if __name__ == "__main__":
    main()
