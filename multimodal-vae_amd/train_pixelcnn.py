"""``mnist/train_pixelcnn.py`` and ``coco/train_pixelcnn.py`` in one script::

    python -m multimodal_vae_amd.train_pixelcnn --dataset mnist --gated --cuda --synthetic 2048      # no data files needed
    python -m multimodal_vae_amd.train_pixelcnn --dataset coco --cuda --data ./data/coco_pixel

Training is the reference's: Adam with ``weight_decay=1e-4``, gradient norm clipped at 1, target ``(data * (out_dims - 1)).long()``,
cross entropy over every (sample, channel, pixel); the best model so far triggers ``generate``.  The models are plain torch modules
and train through autograd wherever torch runs.  ``generate`` is the one-launch incremental sampler (``pixelcnn.generate``) when the
model is on the device; on the CPU it is skipped (there is no CPU sampler).

``--conv_backend hip`` (needs ``--cuda``) trains through ``pixelcnn.causal_conv2d``: every convolution's forward, data gradient and
weight gradient on bf16 MFMA with fp32 accumulation, only the taps that exist.  Gates, ReLUs, residual adds, the cross entropy and
Adam stay torch ops; ``test()`` and ``generate`` work with either backend and the checkpoint has the same ``state_dict``.  The
gradient of masked weight cells is exactly 0 there (torch gives them one that ``clip_grad_norm_`` counts), so the clipped norm is
taken over the taps that exist.

``--head hip`` (needs ``--cuda``) computes the loss through ``pixelcnn.head_nll``: the output head ``conv4`` and the cross entropy
as one fused device op, forward and backward, that never writes the logits to memory; the loss is ``nll(...).mean()`` in training
and in ``test()``.  It is independent of ``--conv_backend``; the default stays ``torch``.

Defaults follow the dataset's reference script: ``--out_dims`` 8 and 28 x 28 for mnist (``--rgb`` triples the channel), ``--out_dims``
256, ``--image_size`` 32, three channels and the gated model for coco (``--cifar`` only renames the output folder there).  One
deliberate difference: the MNIST script passes ``(data_channels, out_dims)`` positionally into ``(n_blocks, data_channels)`` and
cannot run; this one passes keywords.

Data: ``--data DIR`` holds ``train.pt`` and ``test.pt``, uint8 tensors (N, C, H, W); or ``--synthetic N``.
"""
import argparse
import os
import sys

import torch
import torch.optim as optim

from .pixelcnn import (CONV_BACKENDS, HEADS, GatedPixelCNN, MMVAEError, PixelCNN, check_head, cross_entropy_by_dim, nll, quantisize,
                       save_checkpoint, set_conv_backend)


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--dataset', choices=['mnist', 'coco'], default='mnist')
    parser.add_argument('--cifar', action='store_true', default=False, help='coco: train on CIFAR if set (default: False)')
    parser.add_argument('--rgb', action='store_true', default=False, help='mnist: convert MNIST to RGB form (default: False)')
    parser.add_argument('--gated', action='store_true', default=False, help='mnist: GatedPixelCNN instead of PixelCNN (coco always)')
    parser.add_argument('--n_blocks', type=int, default=15, metavar='N', help='number of blocks (default: 15)')
    parser.add_argument('--hid_dims', type=int, default=128, metavar='N', help='hidden channels (default: 128)')
    parser.add_argument('--out_dims', type=int, default=None, metavar='N', help='2|4|8|16|...|256 (default: mnist 8, coco 256)')
    parser.add_argument('--image_size', type=int, default=None, metavar='N', help='side of the images (default: mnist 28, coco 32)')
    parser.add_argument('--batch_size', type=int, default=32, metavar='N', help='input batch size for training (default: 32)')
    parser.add_argument('--epochs', type=int, default=10, metavar='N', help='number of epochs to train (default: 10)')
    parser.add_argument('--lr', type=float, default=1e-3, metavar='LR', help='learning rate (default: 1e-3)')
    parser.add_argument('--log_interval', type=int, default=10, metavar='N', help='batches between log lines (default: 10)')
    parser.add_argument('--cuda', action='store_true', default=False, help='enables GPU training (default: False)')
    parser.add_argument('--conv_backend', choices=CONV_BACKENDS, default='torch',
                        help='convolutions through torch ops or through the HIP causal convolution (hip needs --cuda; default: torch)')
    parser.add_argument('--head', choices=HEADS, default='torch',
                        help='conv4 + cross entropy as torch ops or as the fused HIP head (hip needs --cuda; default: torch)')
    parser.add_argument('--synthetic', type=int, default=0, metavar='N', help='train on N synthetic images instead of files')
    parser.add_argument('--data', default='./data', help='folder with train.pt / test.pt, uint8 (N, C, H, W)')
    parser.add_argument('--seed', type=int, default=0)
    return parser


def resolve(args):
    """fills the per-dataset defaults in; -> args"""
    coco = args.dataset == 'coco'
    if args.out_dims is None:
        args.out_dims = 256 if coco else 8
    if args.image_size is None:
        args.image_size = 32 if coco else 28
    args.data_channels = 3 if (coco or args.rgb) else 1
    args.gated = args.gated or coco
    args.folder_name = ('pixel_cifar' if args.cifar else 'pixel_cnn') if coco else 'pixel_cnn'
    if args.conv_backend == 'hip' and not (args.cuda and torch.cuda.is_available()):
        raise SystemExit('--conv_backend hip runs on the GPU only: pass --cuda on a machine with a gfx950 device (there is no CPU fallback)')
    if args.head == 'hip' and not (args.cuda and torch.cuda.is_available()):
        raise SystemExit('--head hip runs on the GPU only: pass --cuda on a machine with a gfx950 device (there is no CPU fallback)')
    args.cuda = args.cuda and torch.cuda.is_available()
    assert 1 < args.out_dims <= 256
    return args


def build_model(args):
    cls = GatedPixelCNN if args.gated else PixelCNN
    model = cls(n_blocks=args.n_blocks, data_channels=args.data_channels, hid_dims=args.hid_dims, out_dims=args.out_dims)
    try:
        check_head(model, getattr(args, 'head', 'torch'), '--head')
    except MMVAEError as e:
        raise SystemExit(str(e))
    return set_conv_backend(model, getattr(args, 'conv_backend', 'torch'))


def preprocess(u8, out_dims):
    """uint8 (N, C, H, W) -> float32 in [0, 1], quantised to out_dims levels / (out_dims - 1) when out_dims < 256"""
    x = u8.float() / 255.0
    if out_dims < 256:
        x = torch.from_numpy(quantisize(x.numpy(), out_dims).astype('f')) / (out_dims - 1)
    return x


def synthetic_images(n, channels, size, seed=0):
    """smooth random blobs, uint8 (n, channels, size, size)"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(n, channels, max(2, size // 4), max(2, size // 4), generator=g)
    x = torch.nn.functional.interpolate(low, size=(size, size), mode='bilinear', align_corners=False)
    return (x * 255).round().clamp(0, 255).to(torch.uint8)


def batch_loss(model, data, out_dims, head="torch"):
    """mean cross entropy over every (sample, channel, pixel) of a batch in [0, 1]"""
    target = (data * (out_dims - 1)).long()
    if head == "hip":
        return nll(model, data, target, head="hip").mean()
    return cross_entropy_by_dim(model(data), target)


def train_step(model, optimizer, data, out_dims, head="torch"):
    """one optimisation step on a batch in [0, 1]; -> (loss, gradient norm after clipping)"""
    optimizer.zero_grad()
    loss = batch_loss(model, data, out_dims, head)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(model.parameters(), 1.)
    norm = torch.sqrt(sum(p.grad.double().pow(2).sum() for p in model.parameters() if p.grad is not None))
    optimizer.step()
    return float(loss.detach()), float(norm)


def main(argv=None):
    args = resolve(build_parser().parse_args(argv))
    torch.manual_seed(args.seed)
    for d in ('./trained_models/%s' % args.folder_name, './results/%s' % args.folder_name):
        os.makedirs(d, exist_ok=True)
    if args.synthetic > 0:
        tr = synthetic_images(args.synthetic, args.data_channels, args.image_size, args.seed)
        te = synthetic_images(max(args.batch_size, args.synthetic // 6), args.data_channels, args.image_size, args.seed + 1)
    else:
        tr, te = (torch.load(os.path.join(args.data, f)) for f in ('train.pt', 'test.pt'))
        if args.rgb and tr.shape[1] == 1:
            tr, te = tr.repeat(1, 3, 1, 1), te.repeat(1, 3, 1, 1)
    tr, te = preprocess(tr, args.out_dims), preprocess(te, args.out_dims)
    dev = torch.device('cuda' if args.cuda else 'cpu')
    model = build_model(args).to(dev)
    optimizer = optim.Adam(model.parameters(), lr=args.lr, weight_decay=1e-4)

    def train(epoch):
        model.train()
        perm = torch.randperm(len(tr))
        total, seen = 0.0, 0
        for batch_idx in range(0, (len(tr) + args.batch_size - 1) // args.batch_size):
            data = tr[perm[batch_idx * args.batch_size:(batch_idx + 1) * args.batch_size]].to(dev)
            loss, _ = train_step(model, optimizer, data, args.out_dims, args.head)
            total, seen = total + loss * len(data), seen + len(data)
            if batch_idx % args.log_interval == 0:
                print('Train Epoch: {} [{}/{}]\tLoss: {:.6f}'.format(epoch, seen, len(tr), total / seen))
        print('====> Epoch: {}\tLoss: {:.4f}'.format(epoch, total / seen))

    @torch.no_grad()
    def test():
        model.eval()
        total = 0.0
        for k in range(0, len(te), args.batch_size):
            data = te[k:k + args.batch_size].to(dev)
            total += float(batch_loss(model, data, args.out_dims, args.head)) * len(data)
        print('====> Test Epoch\tLoss: {:.4f}'.format(total / len(te)))
        return total / len(te)

    def generate(epoch):
        if dev.type != 'cuda':
            print('generate: skipped, the sampler is device-only')
            return
        from .evaluate import sample_pixelcnn
        model.eval()
        image = sample_pixelcnn(model, 64, args.image_size, args.image_size, seed=epoch)
        torch.save(image.cpu(), './results/{}/sample_{}.pt'.format(args.folder_name, epoch))    # no torchvision here: the tensor

    best_loss = sys.maxsize
    for epoch in range(args.epochs):
        train(epoch)
        loss = test()
        is_best = loss < best_loss
        best_loss = min(loss, best_loss)
        save_checkpoint({
            'state_dict': model.state_dict(), 'best_loss': best_loss, 'optimizer': optimizer.state_dict(), 'gated': args.gated,
            'n_blocks': args.n_blocks, 'data_channels': args.data_channels, 'hid_dims': args.hid_dims, 'out_dims': args.out_dims,
            'height': args.image_size, 'width': args.image_size, 'conv_backend': args.conv_backend, 'head': args.head,
        }, is_best, folder='./trained_models/%s' % args.folder_name)
        if is_best:
            generate(epoch)


if __name__ == "__main__":
    main()
