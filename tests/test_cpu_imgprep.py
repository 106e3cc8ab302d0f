"""Scale + CenterCrop preprocessing, the parts that need no GPU (multimodal-vae_amd/csrc/imgprep_core.h, imgprep.py, make_celeba.py,
train_celeba.py, celeba.py's attribute tables): the numpy restatement (tests/imgprep_ref.py) against live Pillow and against a recorded
Pillow fixture, the library's host build of the kernel's coefficient functions against the restatement, the small functions and
parsers, and a check that the case list of the GPU test does notice the mistakes an ``==`` test is there to catch."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imgprep_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    images = R.case_images(0)
    return images, [R.scale_crop(im, S) for (_, _, S), im in zip(R.CASES, images)]


def test_case_list_is_the_stated_one():
    assert len(R.NAMED_CASES) == 16 and len(R.GRID_CASES) == 80 and len(set(R.CASES)) == 96
    assert (178, 218, 64) in R.CASES and (1300, 2000, 64) in R.CASES and (3, 1000, 64) in R.CASES
    assert R.scaled_size(3, 1000, 64) == (64, 21333)


def test_restatement_against_live_pillow(cases):
    Image = pytest.importorskip("PIL.Image")
    images, want = cases
    for (w, h, S), im, mine in zip(R.CASES, images, want):
        ow, oh = R.scaled_size(w, h, S)
        full = np.asarray(Image.fromarray(im).resize((ow, oh), Image.BILINEAR))
        x1, y1 = R.crop_offset(ow - S), R.crop_offset(oh - S)
        assert (full[y1:y1 + S, x1:x1 + S].transpose(2, 0, 1) == mine).all(), (w, h, S)
        if ow * oh <= 200000:                                     # the whole resize too, where it is small
            assert (R.resize_full(im, ow, oh) == full).all(), (w, h, S)


def test_restatement_against_recorded_pillow(cases, golden_dir):
    """tools/record_pillow_scale_crop.py wrote the outputs; the inputs come from the seed"""
    z = np.load(os.path.join(golden_dir, "pillow_scale_crop.npz"))
    assert [tuple(int(v) for v in c) for c in z["cases"]] == R.CASES and int(z["seed"]) == 0
    _, want = cases
    for k, mine in enumerate(want):
        assert (z["out_%03d" % k] == mine).all(), R.CASES[k]


def _axes():
    """every (n_in, n_out, first index, count) the case list produces"""
    axes = set()
    for (w, h, S) in R.CASES:
        ow, oh = R.scaled_size(w, h, S)
        axes.add((w, ow, R.crop_offset(ow - S), S))
        axes.add((h, oh, R.crop_offset(oh - S), S))
    return sorted(axes)


def test_host_coefficient_builder_equals_restatement():
    """mmvae_imgprep_coeffs runs the kernel's own span_of / coef_at, compiled for the host"""
    from multimodal_vae_amd import imgprep as I
    assert I.imgprep_geometry() == (8192, 128, 22)
    for (n_in, n_out, first, count) in _axes():
        xmin, taps, coefs = I.coefficients(n_in, n_out, first, count)
        rows = R.coeffs(n_in, n_out, first, count)
        assert xmin.tolist() == [r[0] for r in rows] and taps.tolist() == [len(r[1]) for r in rows], (n_in, n_out)
        for j, (_, k) in enumerate(rows):
            assert coefs[j, :len(k)].tolist() == k and not coefs[j, len(k):].any(), (n_in, n_out, first + j)


def test_core_header_as_a_host_program_under_sanitizers(tmp_path):
    """csrc/imgprep_core.h is plain C++17: tests/host/imgprep_core_check.cpp (its own main) prints the scaled size, the crop offsets and
    the coefficient rows of both axes under -fsanitize=address,undefined; what it prints equals the numpy restatement"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "imgprep_core_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "multimodal-vae_amd", "csrc"), os.path.join(ROOT, "tests", "host", "imgprep_core_check.cpp"), "-o", exe],
                   check=True)
    for (w, h, S) in [(178, 218, 64), (640, 480, 32), (20, 30, 32), (65, 64, 64), (1, 1, 32), (3, 1000, 64), (1300, 2000, 64), (8192, 8191, 128),
                      (8192, 4097, 1)]:
        r = subprocess.run([exe, str(w), str(h), str(S)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.strip().split("\n")
        ow, oh = R.scaled_size(w, h, S)
        x1, y1 = R.crop_offset(ow - S), R.crop_offset(oh - S)
        assert lines[0] == "size %d %d %d %d" % (ow, oh, x1, y1)
        want = [("h", x1 + j, xmin, k) for j, (xmin, k) in enumerate(R.coeffs(w, ow, x1, S))] + \
               [("v", y1 + j, xmin, k) for j, (xmin, k) in enumerate(R.coeffs(h, oh, y1, S))]
        assert len(lines) == 1 + len(want)
        for ln, (ax, idx, xmin, k) in zip(lines[1:], want):
            assert ln == " ".join([ax] + [str(v) for v in [idx, xmin, len(k)] + k]), (w, h, S, ln)
    assert subprocess.run([exe, "0", "5", "32"]).returncode == 3


def test_host_layout_and_refusals():
    from multimodal_vae_amd._lib import MMVAEError, call
    from multimodal_vae_amd import imgprep as I
    v = [ctypes.c_int() for _ in range(4)]
    for (w, h, S) in R.CASES:
        call("mmvae_imgprep_layout", h, w, S, *[ctypes.byref(a) for a in v])
        ow, oh = R.scaled_size(w, h, S)
        assert [a.value for a in v] == [ow, oh, R.crop_offset(ow - S), R.crop_offset(oh - S)]
        assert I.scaled_size(w, h, S) == (ow, oh)
    for args in ((0, 10, 32), (10, 8193, 32), (10, 10, 0), (10, 10, 129)):
        with pytest.raises(MMVAEError):
            call("mmvae_imgprep_layout", *args, *[ctypes.byref(a) for a in v])
    with pytest.raises(MMVAEError):
        call("mmvae_imgprep_geometry", None, None, None)
    # the pointer checks of scale_crop come before any launch: they answer without a GPU
    p = ctypes.c_void_p(16)
    for a in ((None, 0, p, p, p, 1, 32, p, None, p), (p, 0, p, p, p, 1, 0, p, None, p), (p, 0, p, p, p, 1, 32, None, None, p),
              (p, 0, p, p, p, 1, 32, p, None, None)):
        with pytest.raises(MMVAEError, match=r"failed \(-1\)"):
            call("mmvae_imgprep_scale_crop", *a, None)


def test_scaled_size_and_crop_offset():
    from multimodal_vae_amd import imgprep as I
    assert I.scaled_size(178, 218, 64) == (64, 78) and I.scaled_size(640, 480, 32) == (42, 32) and I.scaled_size(64, 64, 64) == (64, 64)
    assert I.scaled_size(65, 64, 64) == (65, 64) and I.scaled_size(97, 64, 64) == (97, 64)
    # int(size * h / w) with Python's float division, as the transform computes it
    for (w, h, S) in R.CASES + [(8191, 8192, 128), (8192, 8191, 127), (7, 8192, 3), (4097, 8192, 1)]:
        assert I.scaled_size(w, h, S) == ((S, int(S * h / w)) if w <= h else (int(S * w / h), S))
    # int(round(d / 2.)) under Python 2: halves go away from zero; an odd difference shows it (ow - S = 1 and = 33)
    assert [I.crop_offset(d) for d in (0, 1, 2, 3, 14, 33)] == [0, 1, 1, 2, 7, 17]
    assert [R.crop_offset(d) for d in (0, 1, 2, 3, 14, 33)] == [0, 1, 1, 2, 7, 17]
    assert I.crop_offset(65 - 64) == 1 and I.crop_offset(97 - 64) == 17


def test_pack_images_layout():
    from multimodal_vae_amd import imgprep as I
    from multimodal_vae_amd._lib import MMVAEError
    rng = np.random.default_rng(3)
    ims = [R.random_image(rng, 5, 7), R.random_image(rng, 1, 1), R.random_image(rng, 9, 2)]
    pixels, offsets, heights, widths = I.pack_images(ims)
    assert heights.tolist() == [7, 1, 2] and widths.tolist() == [5, 1, 9] and offsets.tolist() == [0, 112, 128]
    assert pixels.dtype == torch.uint8 and offsets.dtype == torch.int64 and heights.dtype == torch.int32
    for im, o in zip(ims, offsets.tolist()):
        assert (pixels[o:o + im.size].numpy() == im.reshape(-1)).all()
    I.check_descriptors(pixels.numel(), offsets, heights, widths)
    with pytest.raises(MMVAEError, match="image 2"):
        I.check_descriptors(128 + 53, offsets, heights, widths)
    with pytest.raises(MMVAEError, match="image 0"):
        I.pack_images([np.zeros((4, 4), dtype=np.uint8)])


def test_attribute_tables_round_trip():
    from multimodal_vae_amd import celeba as C
    assert len(C.ATTR_NAMES) == 40 and len(C.ATTR_IX_TO_KEEP) == 18 == C.N_ATTRS
    assert C.ATTR_TO_IX_DICT['5_o_Clock_Shadow'] == 0 and C.ATTR_TO_IX_DICT['Male'] == 20 and C.ATTR_TO_IX_DICT['Young'] == 39
    assert all(C.IX_TO_ATTR_DICT[C.ATTR_TO_IX_DICT[n]] == n for n in C.ATTR_NAMES)
    kept = [C.IX_TO_ATTR_DICT[i] for i in C.ATTR_IX_TO_KEEP]
    assert kept[0] == 'Bald' and kept[-1] == 'Wearing_Hat' and 'Smiling' in kept and 'Young' not in kept
    a = C.attrs_from_names('Male,Smiling')
    assert a.shape == (1, 18) and a.sum() == 2 and C.tensor_to_attributes(a[0]) == ['Male', 'Smiling']
    assert C.tensor_to_attributes(C.attrs_from_names(['Bald'])[0] * 0.7) == ['Bald']
    assert C.tensor_to_attributes(torch.full((18,), 0.4)) == []
    for name in kept:
        assert C.tensor_to_attributes(C.attrs_from_names(name)[0]) == [name]
    with pytest.raises(ValueError, match="not a CelebA attribute"):
        C.attrs_from_names('Beard')
    with pytest.raises(ValueError, match="keeps"):
        C.attrs_from_names('Young')


def test_attribute_file_parser(tmp_path):
    from multimodal_vae_amd import celeba as C, make_celeba as M
    rng = np.random.default_rng(11)
    names = ['%06d.jpg' % (i + 1) for i in range(6)]
    rows = np.where(rng.random((6, 40)) < 0.5, 1, -1)
    part = [0, 1, 0, 2, 1, 0]
    with open(tmp_path / 'attr.txt', 'w') as fp:
        fp.write('6\n%s\n' % ' '.join(C.ATTR_NAMES))
        for n, r in zip(names, rows):
            fp.write('%s  %s\n' % (n, ' '.join('%2d' % v for v in r)))
    with open(tmp_path / 'part.txt', 'w') as fp:
        for n, p in zip(names, part):
            fp.write('%s %d\n' % (n, p))
    table = M.load_attribute_file(str(tmp_path / 'attr.txt'))
    assert sorted(table) == names
    for pname, pid in M.VALID_PARTITIONS.items():
        mine = M.load_eval_partition(str(tmp_path / 'part.txt'), pname)
        assert mine == [n for n, p in zip(names, part) if p == pid]
        a = M.partition_attributes(table, mine)
        want = np.maximum(rows[[i for i, p in enumerate(part) if p == pid]], 0)[:, C.ATTR_IX_TO_KEEP]
        assert a.dtype == torch.float32 and a.shape == (len(mine), 18) and (a.numpy() == want).all()
    with pytest.raises(ValueError, match="no attribute row"):
        M.partition_attributes(table, ['999999.jpg'])
    with open(tmp_path / 'bad.txt', 'w') as fp:
        fp.write('1\n%s\n' % ' '.join(reversed(C.ATTR_NAMES)))
    with pytest.raises(ValueError, match="order"):
        M.load_attribute_file(str(tmp_path / 'bad.txt'))


def test_synthetic_raw_is_seeded():
    from multimodal_vae_amd import data as D
    a, ra = D.synthetic_celeba_raw(3, seed=4)
    b, rb = D.synthetic_celeba_raw(3, seed=4)
    c, _ = D.synthetic_celeba_raw(3, seed=5)
    assert len(a) == 3 and all(im.shape == (218, 178, 3) and im.dtype == np.uint8 for im in a)
    assert all((x == y).all() for x, y in zip(a, b)) and torch.equal(ra, rb) and any((x != y).any() for x, y in zip(a, c))
    assert ra.shape == (3, 40) and ra.dtype == torch.int64 and set(ra.unique().tolist()) <= {-1, 1}


def test_argument_parsers():
    from multimodal_vae_amd import evaluate as E, make_celeba as M, train_celeba as T
    a = M.build_parser().parse_args([])
    assert (a.root, a.out, a.partitions, a.chunk, a.workers, a.synthetic, a.seed) == ('./data', None, ['train', 'val', 'test'], 4096, 8, 0, 0)
    a = M.build_parser().parse_args(['--synthetic', '96', '--out', 'x', '--partitions', 'val', 'test'])
    assert a.synthetic == 96 and a.out == 'x' and a.partitions == ['val', 'test']
    with pytest.raises(SystemExit):
        M.build_parser().parse_args(['--partitions', 'dev'])
    a = T.build_parser().parse_args([])                          # celeba/train.py:86-99
    assert (a.n_latents, a.batch_size, a.epochs, a.lr, a.log_interval, a.cuda) == (100, 128, 20, 1e-3, 10, False)
    a = T.build_parser().parse_args(['--data', 'd', '--epochs', '1', '--batch_size', '32', '--cuda', '--anneal_kl', '--synthetic', '64'])
    assert (a.data, a.epochs, a.batch_size, a.cuda, a.anneal_kl, a.synthetic) == ('d', 1, 32, True, True, 64)
    a = E._parser().parse_args(['sample_celeba', 'ck', '--condition_on_image', 'Male', '--data', 'f.pt', '--condition_on_attrs', 'Bald,Smiling'])
    assert (a.cmd, a.model_path, a.condition_on_image, a.data, a.condition_on_attrs, a.n_samples, a.out, a.seed) == \
        ('sample_celeba', 'ck', 'Male', 'f.pt', 'Bald,Smiling', 64, './results', 0)


def test_the_case_list_sees_the_mistakes(cases):
    """a dropped last tap, the passes in the other order and a crop offset of d // 2 each change the restatement's output on the case
    list: an ``==`` test over these cases cannot pass by accident"""
    images, want = cases
    for kw in (dict(drop_last_tap=True), dict(vertical_first=True), dict(crop=lambda d: d // 2)):
        changed = [c for c, im, w in zip(R.CASES, images, want) if c != (1300, 2000, 64) and (R.scale_crop(im, c[2], **kw) != w).any()]
        assert len(changed) >= 10, (kw, changed)
    # the band loop's case on its own: the two cheap mistakes
    k = R.CASES.index((1300, 2000, 64))
    assert (R.scale_crop(images[k], 64, drop_last_tap=True) != want[k]).any()
    # an odd crop difference is what tells (d + 1) // 2 from d // 2
    k = R.CASES.index((65, 64, 64))
    assert (R.scale_crop(images[k], 64, crop=lambda d: d // 2) != want[k]).any()
