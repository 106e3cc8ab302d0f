"""Builds the CelebA dataset files of this engine from the reference's data layout (``celeba/datasets.py``, ``celeba/train.py:102-104``):

    python -m multimodal_vae_amd.make_celeba --root ./data                  # img_align_celeba/, Eval/, Anno/ below ./data
    python -m multimodal_vae_amd.make_celeba --synthetic 4096 --out ./data  # needs neither files nor Pillow

writes ``<out>/celeba_{train,val,test}.pt``, each ``(uint8 (N,3,64,64), float32 (N,18))`` -- the layout ``evaluate loglik_celeba
--data`` and ``train_celeba --data`` read.  The images are decoded with Pillow (``convert('RGB')``) on a thread pool, packed per chunk
and preprocessed on the device by ``imgprep.scale_center_crop`` (Scale(64) + CenterCrop(64), bit for bit the reference's transforms);
``ToTensor``'s division by 255 happens where the file is read.

Attributes: the rows of ``Anno/list_attr_celeba.txt`` that belong to the partition's own images, -1 -> 0, the 18 columns of
``ATTR_IX_TO_KEEP``.  The reference's ``load_attributes`` (celeba/datasets.py:81-97) appends EVERY row of the file whatever the
partition, so image i of ``val`` / ``test`` gets the attributes of the file's i-th image (a training image); what it means to do, the
partition's own rows, is what is built here.
"""
from __future__ import annotations

import argparse
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

VALID_PARTITIONS = {'train': 0, 'val': 1, 'test': 2}
SIZE = 64
MAX_WORKERS = 16


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser()
    parser.add_argument('--root', type=str, default='./data', help='folder with img_align_celeba/, Eval/list_eval_partition.txt, Anno/list_attr_celeba.txt')
    parser.add_argument('--out', type=str, default=None, metavar='DIR', help='where celeba_{train,val,test}.pt go (default: --root)')
    parser.add_argument('--partitions', type=str, nargs='+', default=['train', 'val', 'test'], choices=sorted(VALID_PARTITIONS, key=VALID_PARTITIONS.get))
    parser.add_argument('--chunk', type=int, default=4096, help='images per launch of the preprocessing kernel')
    parser.add_argument('--workers', type=int, default=8, help='decoding threads (at most %d)' % MAX_WORKERS)
    parser.add_argument('--synthetic', type=int, default=0, metavar='N', help='N synthetic 218 x 178 images per partition instead of files')
    parser.add_argument('--seed', type=int, default=0, help='seed of the synthetic images')
    return parser


def load_eval_partition(path: str, partition: str):
    """celeba/datasets.py:69-78 -> the file names of the partition, in the file's order"""
    names = []
    with open(path) as fp:
        for row in fp:
            row = row.split()
            if len(row) == 2 and int(row[1]) == VALID_PARTITIONS[partition]:
                names.append(row[0])
    return names


def load_attribute_file(path: str):
    """``Anno/list_attr_celeba.txt`` (a count line, a line of 40 names, then ``name v0 .. v39`` rows of -1 / 1) ->
    {file name: int64 (40,) row}.  The name line must be CelebA's own column order."""
    from .celeba import ATTR_NAMES
    with open(path) as fp:
        rows = fp.readlines()
    header = rows[1].split()
    if header != list(ATTR_NAMES):
        raise ValueError("%s: the attribute names of line 2 are not CelebA's 40 columns in their order" % path)
    table = {}
    for ix, row in enumerate(rows[2:]):
        row = row.split()
        if not row:
            continue
        if len(row) != 41:
            raise ValueError("%s: row %d has %d fields, need a name and 40 values" % (path, ix + 3, len(row)))
        table[row[0]] = np.array(row[1:], dtype=np.int64)
    return table


def partition_attributes(table, names) -> torch.Tensor:
    """the partition's own rows, -1 -> 0, columns ATTR_IX_TO_KEEP -> float32 (N,18)"""
    from .celeba import ATTR_IX_TO_KEEP
    missing = [n for n in names if n not in table]
    if missing:
        raise ValueError("no attribute row for %d images of the partition, e.g. %s" % (len(missing), missing[0]))
    a = np.stack([table[n] for n in names]) if names else np.zeros((0, 40), dtype=np.int64)
    a = np.where(a < 0, 0, a)
    return torch.from_numpy(a[:, ATTR_IX_TO_KEEP].astype(np.float32))


def decode_rgb(path: str) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert('RGB'))


def preprocess(arrays_of, n: int, chunk: int, device) -> torch.Tensor:
    """``arrays_of(lo, hi)`` -> the decoded images lo .. hi - 1; -> uint8 (n,3,64,64) on the host, ``chunk`` images per launch"""
    from . import imgprep
    out = torch.empty((n, 3, SIZE, SIZE), dtype=torch.uint8)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        out[lo:hi] = imgprep.scale_center_crop(arrays_of(lo, hi), SIZE, out="u8", device=device).cpu()
    return out


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("the preprocessing runs on a gfx950 GPU only (no CPU fallback)")
    if args.chunk < 1:
        raise SystemExit("--chunk must be at least 1")
    from . import data as D
    dev = torch.device("cuda", torch.cuda.current_device())
    out_dir = args.out or args.root
    os.makedirs(out_dir, exist_ok=True)
    workers = max(1, min(int(args.workers), MAX_WORKERS))
    table = None if args.synthetic > 0 else load_attribute_file(os.path.join(args.root, 'Anno', 'list_attr_celeba.txt'))
    paths = []
    with ThreadPoolExecutor(max_workers=workers) as pool:
        for part in args.partitions:
            if args.synthetic > 0:
                raw, rows = D.synthetic_celeba_raw(args.synthetic, seed=args.seed + VALID_PARTITIONS[part])
                names = ['%06d.jpg' % i for i in range(len(raw))]
                attrs = partition_attributes(dict(zip(names, rows.numpy())), names)
                images = preprocess(lambda lo, hi: raw[lo:hi], len(raw), args.chunk, dev)
            else:
                names = load_eval_partition(os.path.join(args.root, 'Eval', 'list_eval_partition.txt'), part)
                attrs = partition_attributes(table, names)
                files = [os.path.join(args.root, 'img_align_celeba', n) for n in names]
                images = preprocess(lambda lo, hi: list(pool.map(decode_rgb, files[lo:hi])), len(files), args.chunk, dev)
            path = os.path.join(out_dir, 'celeba_%s.pt' % part)
            torch.save((images, attrs), path)
            print("wrote %s: %d images" % (path, len(images)))
            paths.append(path)
    return paths


if __name__ == "__main__":
    main()
