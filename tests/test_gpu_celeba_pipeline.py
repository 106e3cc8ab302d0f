"""CelebA from the dataset to a checkpoint (make_celeba.py, train_celeba.py, evaluate.sample_celeba): the builder's files against the
numpy restatement of the preprocessing (tests/imgprep_ref.py) on synthetic arrays and on a small fake CelebA tree of lossless PNGs,
one epoch of the train driver on those files, the checkpoint through ``celeba.load_checkpoint`` and ``evaluate loglik_celeba``, and
the sampler's four modes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imgprep_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CHECKPOINT_KEYS = {'state_dict', 'best_loss', 'joint_loss', 'image_loss', 'attrs_loss', 'n_latents', 'optimizer'}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """make_celeba --synthetic 96, then one epoch of train_celeba on its files"""
    _need_gpu()
    from multimodal_vae_amd import make_celeba as M, train_celeba as T
    root = tmp_path_factory.mktemp("celeba")
    paths = M.main(['--synthetic', '96', '--out', str(root), '--chunk', '40', '--seed', '3'])
    history = T.main(['--data', str(root), '--epochs', '1', '--batch_size', '32', '--cuda', '--out', str(root / 'models')])
    return root, paths, history


def test_synthetic_files_equal_the_restatement(built):
    from multimodal_vae_amd import celeba as C, data as D, make_celeba as M
    root, paths, _ = built
    assert [os.path.basename(p) for p in paths] == ['celeba_train.pt', 'celeba_val.pt', 'celeba_test.pt']
    for part, path in zip(('train', 'val', 'test'), paths):
        x, a = torch.load(path, weights_only=False)
        assert x.dtype == torch.uint8 and tuple(x.shape) == (96, 3, 64, 64) and a.dtype == torch.float32 and tuple(a.shape) == (96, 18)
        raw, rows = D.synthetic_celeba_raw(96, seed=3 + M.VALID_PARTITIONS[part])
        for i in range(0, 96, 5):                                 # (every chunk of 40 is met)
            assert (x[i].numpy() == R.scale_crop(raw[i], 64)).all(), (part, i)
        assert (a.numpy() == np.maximum(rows.numpy(), 0)[:, C.ATTR_IX_TO_KEEP]).all()


def test_fake_celeba_tree(tmp_path):
    _need_gpu()
    Image = pytest.importorskip("PIL.Image")
    from multimodal_vae_amd import celeba as C, make_celeba as M
    rng = np.random.default_rng(21)
    names = ['%06d.png' % (i + 1) for i in range(6)]
    part = [0, 1, 0, 2, 0, 1]
    rows = np.where(rng.random((6, 40)) < 0.5, 1, -1)
    os.makedirs(tmp_path / 'img_align_celeba')
    os.makedirs(tmp_path / 'Eval')
    os.makedirs(tmp_path / 'Anno')
    raw = [R.random_image(rng, 178, 218) for _ in names]
    for n, im in zip(names, raw):
        Image.fromarray(im).save(str(tmp_path / 'img_align_celeba' / n))          # PNG: lossless
    with open(tmp_path / 'Eval' / 'list_eval_partition.txt', 'w') as fp:
        fp.writelines('%s %d\n' % (n, p) for n, p in zip(names, part))
    with open(tmp_path / 'Anno' / 'list_attr_celeba.txt', 'w') as fp:
        fp.write('6\n%s\n' % ' '.join(C.ATTR_NAMES))
        fp.writelines('%s %s\n' % (n, ' '.join(str(v) for v in r)) for n, r in zip(names, rows))
    M.main(['--root', str(tmp_path), '--out', str(tmp_path / 'out'), '--workers', '2'])
    for pname, pid in M.VALID_PARTITIONS.items():
        x, a = torch.load(str(tmp_path / 'out' / ('celeba_%s.pt' % pname)), weights_only=False)
        ix = [i for i, p in enumerate(part) if p == pid]
        assert tuple(x.shape) == (len(ix), 3, 64, 64) and x.dtype == torch.uint8
        for j, i in enumerate(ix):
            assert (x[j].numpy() == R.scale_crop(raw[i], 64)).all(), (pname, i)
        # the partition's OWN rows (the reference takes the file's first rows whatever the partition)
        assert (a.numpy() == np.maximum(rows[ix], 0)[:, C.ATTR_IX_TO_KEEP]).all()


def test_train_driver_checkpoint(built):
    from multimodal_vae_amd import celeba as C
    root, _, history = built
    assert len(history["train"]) == 1 and len(history["test"]) == 1
    assert all(np.isfinite(v) for v in history["train"][0] + tuple(history["test"][0]))
    for name in ('checkpoint.pth.tar', 'model_best.pth.tar'):
        ck = torch.load(str(root / 'models' / name), map_location='cpu', weights_only=False)
        assert set(ck) == CHECKPOINT_KEYS and ck['n_latents'] == 100
        assert set(ck['state_dict']) == set(C.MultimodalVAE(100).state_dict())
        assert all(np.isfinite(ck[k]) for k in ('best_loss', 'joint_loss', 'image_loss', 'attrs_loss'))
    vae = C.load_checkpoint(str(root / 'models' / 'model_best.pth.tar'), use_cuda=True)
    assert isinstance(vae, C.MultimodalVAE) and vae.n_latents == 100


def test_loglik_celeba_reads_the_files(built):
    from multimodal_vae_amd import evaluate as E
    root, _, _ = built
    table = E.main(['loglik_celeba', str(root / 'models' / 'model_best.pth.tar'), '--data', str(root / 'celeba_test.pt'), '--n_samples', '8'])
    r = table["joint"]
    assert r["n"] == 96 and all(np.isfinite(r[k]) for k in ("log_px", "log_py", "log_pxy"))


def test_sample_celeba_four_modes(built, tmp_path):
    from multimodal_vae_amd import celeba as C, evaluate as E
    root, _, _ = built
    kept = {C.IX_TO_ATTR_DICT[i] for i in C.ATTR_IX_TO_KEEP}
    vae = C.load_checkpoint(str(root / 'models' / 'model_best.pth.tar'), use_cuda=True)
    image = E.fetch_celeba_image(str(root / 'celeba_train.pt'), 'Bald', seed=1)
    assert tuple(image.shape) == (1, 3, 64, 64) and 0.0 <= float(image.min()) and float(image.max()) <= 1.0
    attrs = C.attrs_from_names('Male,Smiling')
    for im, at in ((None, None), (image, None), (None, attrs), (image, attrs)):
        x, names = E.sample_celeba(vae, n_samples=5, image=im, attrs=at, seed=2)
        assert tuple(x.shape) == (5, 3, 64, 64) and x.dtype == torch.float32 and bool(torch.isfinite(x).all())
        assert 0.0 <= float(x.min()) and float(x.max()) <= 1.0
        assert len(names) == 5 and all(isinstance(row, list) and set(row) <= kept for row in names)
    x1, n1 = E.sample_celeba(vae, 5, image, attrs, seed=2)
    x2, n2 = E.sample_celeba(vae, 5, image, attrs, seed=2)
    assert torch.equal(x1, x2) and n1 == n2
    # the command line: mode 4
    E.main(['sample_celeba', str(root / 'models' / 'model_best.pth.tar'), '--condition_on_image', 'Bald', '--data', str(root / 'celeba_train.pt'),
            '--condition_on_attrs', 'Male', '--n_samples', '4', '--out', str(tmp_path / 'res'), '--seed', '1'])
    assert tuple(torch.load(str(tmp_path / 'res' / 'sample_image.pt')).shape) == (4, 3, 64, 64)
    with open(tmp_path / 'res' / 'sample_attrs.txt') as fp:
        lines = fp.read().split('\n')[:-1]
    assert len(lines) == 4 and all(set(v for v in l.split(',') if v) <= kept for l in lines)
    with pytest.raises(ValueError, match="not a CelebA attribute"):
        E.main(['sample_celeba', 'nothing', '--condition_on_attrs', 'Beard'])
