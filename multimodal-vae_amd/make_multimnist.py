"""``multimnist/datasets.py``'s command line on the device generator (``multimnist_gen``): writes ``<out>/processed/{training,test}.pt``
in the reference's format, which ``train.py --data <out>`` reads.

    python -m multimodal_vae_amd.make_multimnist --mnist_train MNIST/processed/training.pt --mnist_test MNIST/processed/test.pt
    python -m multimodal_vae_amd.make_multimnist --synthetic_mnist 4096 --out ./data          # no MNIST files needed

The MNIST files are torchvision's ``(uint8 (N,28,28), int64 (N,))`` pairs.  The reference's flags keep their names and meaning
(``datasets.py:281-313``).  The canvases have the reference's distribution; its numpy random stream is not reproduced.
"""
from __future__ import annotations

import argparse

import torch


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser()
    # the reference's flags (multimnist/datasets.py:281-297)
    parser.add_argument('--min_digits', type=int, default=0, help='minimum number of digits to add to an image')
    parser.add_argument('--max_digits', type=int, default=2, help='maximum number of digits to add to an image')
    parser.add_argument('--no_resize', action='store_true', default=False, help='if True, fix the image to be MNIST size')
    parser.add_argument('--no_translate', action='store_true', default=False, help='if True, fix the image to be in the center')
    parser.add_argument('--fixed', action='store_true', default=False, help='If True, ignore resize/translate options and generate')
    parser.add_argument('--scramble', action='store_true', default=False, help='If True, scramble labels and generate. Only does something if fixed is True.')
    parser.add_argument('--reverse', action='store_true', default=False, help='If True, reverse flips the labels i.e. 4321 instead of 1234 with 0.5 probability.')
    parser.add_argument('--no_repeat', action='store_true', default=False, help='If True, do not generate images with multiple of the same label.')
    # additions
    parser.add_argument('--mnist_train', type=str, default='', help="MNIST training split: a .pt file holding (uint8 (N,28,28), int64 (N,))")
    parser.add_argument('--mnist_test', type=str, default='', help='MNIST test split, same layout')
    parser.add_argument('--synthetic_mnist', type=int, default=0, metavar='N', help='use N synthetic MNIST-shaped digits per split instead of files')
    parser.add_argument('--out', type=str, default='./data', help='root of processed/{training,test}.pt (default: ./data)')
    parser.add_argument('--n_train', type=int, default=60000, help='training canvases (reference: 60000)')
    parser.add_argument('--n_test', type=int, default=10000, help='test canvases (reference: 10000)')
    parser.add_argument('--seed', type=int, default=0)
    return parser


def mode_of(args) -> dict:
    """the generator's mode arguments from the reference's flags (the command line's --max_digits default of 2 applies to both modes,
    ``datasets.py:284``)"""
    return dict(fixed=args.fixed, resize=not args.no_resize, translate=not args.no_translate, min_digits=args.min_digits,
                max_digits=args.max_digits, reverse=args.reverse, scramble=args.scramble, no_repeat=args.no_repeat)


def load_mnist_pt(path: str):
    digits, labels = torch.load(path, weights_only=False)
    return torch.as_tensor(digits, dtype=torch.uint8), torch.as_tensor(labels, dtype=torch.int64)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("the generator runs on a gfx950 GPU only (no CPU fallback)")
    from . import data as D
    from . import multimnist_gen as G
    if args.synthetic_mnist > 0:
        train, test = D.synthetic_mnist(args.synthetic_mnist, seed=args.seed), D.synthetic_mnist(args.synthetic_mnist, seed=args.seed + 1)
    elif args.mnist_train and args.mnist_test:
        train, test = load_mnist_pt(args.mnist_train), load_mnist_pt(args.mnist_test)
    else:
        raise SystemExit("give --mnist_train FILE.pt and --mnist_test FILE.pt, or --synthetic_mnist N")
    if args.reverse and args.scramble:
        print('Found --reversed and --scrambling. Overriding --reversed.')
    paths = G.make_dataset(args.out, train, test, n_train=args.n_train, n_test=args.n_test, seed=args.seed, **mode_of(args))
    print("wrote %s (%d canvases) and %s (%d canvases)" % (paths[0], args.n_train, paths[1], args.n_test))
    return paths


if __name__ == "__main__":
    main()
