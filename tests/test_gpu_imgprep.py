"""Scale + CenterCrop + ToTensor on the device (multimodal-vae_amd/csrc/imgprep.hip, imgprep.py) against the numpy restatement
(tests/imgprep_ref.py, itself checked against Pillow in tests/test_cpu_imgprep.py).  Integer arithmetic throughout, so every
comparison is ``==``: the case list in ONE ragged call and each image alone (a batch changes nothing), flat and checkerboard inputs,
the float output, determinism, descriptors the kernel must refuse, and the host-side checks of the C entry."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imgprep_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _I():
    from multimodal_vae_amd import imgprep as I
    return I


@pytest.fixture(scope="module")
def cases():
    """(images, expected (3,S,S) uint8 per case): the reference is computed once and left unchanged"""
    images = R.case_images(0)
    want = [R.scale_crop(im, S) for (_, _, S), im in zip(R.CASES, images)]
    return images, want


def _by_size(cases):
    images, want = cases
    groups = {}
    for k, (_, _, S) in enumerate(R.CASES):
        groups.setdefault(S, []).append(k)
    return images, want, groups


def test_ragged_batch_equals_reference(cases):
    """every case of a side in one launch (the two sides of the list are two launches: S is an argument of the call)"""
    dev, I = _dev(), _I()
    images, want, groups = _by_size(cases)
    assert sorted(groups) == [32, 64]
    for S, ks in groups.items():
        got = I.scale_center_crop([images[k] for k in ks], S, out="u8", device=dev).cpu().numpy()
        assert got.shape == (len(ks), 3, S, S) and got.dtype == np.uint8
        for j, k in enumerate(ks):
            assert (got[j] == want[k]).all(), "case %s in the batch: %d bytes differ" % (R.CASES[k], int((got[j] != want[k]).sum()))


def test_each_image_alone_equals_reference(cases):
    dev, I = _dev(), _I()
    images, want = cases
    for k, (w, h, S) in enumerate(R.CASES):
        got = I.scale_center_crop([images[k]], S, out="u8", device=dev).cpu().numpy()
        assert (got[0] == want[k]).all(), "case %s alone: %d bytes differ" % ((w, h, S), int((got[0] != want[k]).sum()))


def test_flat_and_checkerboard():
    dev, I = _dev(), _I()
    flat = np.full((218, 178, 3), 255, dtype=np.uint8)
    yy, xx = np.mgrid[0:218, 0:178]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    got = I.scale_center_crop([flat, board], 64, out="u8", device=dev).cpu().numpy()
    assert (got[0] == 255).all()
    assert (got[0] == R.scale_crop(flat, 64)).all() and (got[1] == R.scale_crop(board, 64)).all()


def test_float_output_and_determinism(cases):
    dev, I = _dev(), _I()
    images, want, groups = _by_size(cases)
    ks = groups[64]
    batch = [images[k] for k in ks]
    f1 = I.scale_center_crop(batch, 64, out="f32", device=dev)
    f2 = I.scale_center_crop(batch, 64, out="f32", device=dev)
    u1 = I.scale_center_crop(batch, 64, out="u8", device=dev)
    u2 = I.scale_center_crop(batch, 64, out="u8", device=dev)
    assert f1.dtype == torch.float32 and torch.equal(f1, f2) and torch.equal(u1, u2)
    # the IEEE quotient (numpy on the host; a device-side torch division by a scalar multiplies by the rounded reciprocal)
    expect = np.stack([want[k] for k in ks]).astype(np.float32) / np.float32(255)
    assert (f1.cpu().numpy().view(np.uint32) == expect.view(np.uint32)).all()


def _raw_call(dev, pixels, declared_bytes, offsets, heights, widths, S, want_u8=True, want_f32=False):
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd._ops import stream
    n = len(offsets)
    d = [torch.as_tensor(v, dtype=dt).to(dev) for v, dt in ((offsets, torch.int64), (heights, torch.int32), (widths, torch.int32))]
    u8 = torch.full((n, 3, S, S), 7, dtype=torch.uint8, device=dev) if want_u8 else None
    f32 = torch.full((n, 3, S, S), 7.0, dtype=torch.float32, device=dev) if want_f32 else None
    status = torch.full((n,), 99, dtype=torch.int32, device=dev)
    call("mmvae_imgprep_scale_crop", ptr(pixels), int(declared_bytes), ptr(d[0]), ptr(d[1]), ptr(d[2]), n, S, ptr(u8), ptr(f32), ptr(status), stream())
    torch.cuda.synchronize()
    return u8, f32, status.cpu().tolist()


def test_kernel_refuses_unusable_descriptors():
    """h = 0, w = max_side + 1 and a span past the declared pixels_bytes: status -1 and zeros, neighbours exact.  The declared size is
    smaller than the allocation, so a kernel without the guard would read valid memory and merely fail the comparison."""
    dev, I = _dev(), _I()
    max_side = I.imgprep_geometry()[0]
    rng = np.random.default_rng(5)
    good = [R.random_image(rng, 40, 50), R.random_image(rng, 61, 33), R.random_image(rng, 30, 30)]
    pixels, offsets, heights, widths = I.pack_images(good)
    used = int(offsets[-1]) + good[-1].size
    # a real allocation well beyond what is declared: [good images | 64 KiB of further valid bytes]
    buf = torch.zeros(used + (64 << 10), dtype=torch.uint8)
    buf[:used] = pixels[:used]
    buf[used:] = torch.from_numpy(rng.integers(0, 256, size=64 << 10, dtype=np.uint8))
    d_buf = buf.to(dev)
    offs = [int(offsets[0]), 0, int(offsets[1]), 0, int(offsets[2]), used - 100]
    hs = [50, 0, 33, 20, 30, 60]
    ws = [40, 20, 61, max_side + 1, 30, 60]                      # the last one spans used - 100 + 10800 > used
    u8, f32, status = _raw_call(dev, d_buf, used, offs, hs, ws, 32, want_u8=True, want_f32=True)
    assert status == [0, -1, 0, -1, 0, -1]
    got, gotf = u8.cpu().numpy(), f32.cpu().numpy()
    for j, im in ((0, good[0]), (2, good[1]), (4, good[2])):
        assert (got[j] == R.scale_crop(im, 32)).all()
        assert (gotf[j] == got[j].astype(np.float32) / np.float32(255)).all()
    for j in (1, 3, 5):
        assert (got[j] == 0).all() and (gotf[j] == 0).all()
    # the same last image is fine once the declared size covers it
    _, _, status = _raw_call(dev, d_buf, used + (64 << 10), offs, hs, ws, 32)
    assert status == [0, -1, 0, -1, 0, 0]
    # a negative offset
    _, _, status = _raw_call(dev, d_buf, used, [-16, 0], [10, 50], [10, 40], 32)
    assert status == [-1, 0]


def test_wrapper_names_the_refused_image():
    dev, I = _dev(), _I()
    from multimodal_vae_amd._lib import MMVAEError
    rng = np.random.default_rng(6)
    pixels, offsets, heights, widths = I.pack_images([R.random_image(rng, 20, 20), R.random_image(rng, 24, 20)])
    heights = heights.clone()
    heights[1] = 4000                                            # its span leaves the buffer
    with pytest.raises(MMVAEError, match="image 1"):
        I.scale_center_crop((pixels, offsets, heights, widths), 32, device=dev)
    with pytest.raises(MMVAEError, match="size"):
        I.scale_center_crop([R.random_image(rng, 20, 20)], 0, device=dev)
    assert I.scale_center_crop([], 32, device=dev).shape == (0, 3, 32, 32)


def test_host_checks_launch_nothing():
    dev = _dev()
    from multimodal_vae_amd._lib import MMVAEError, call, ptr
    p = torch.zeros(4096, dtype=torch.uint8, device=dev)
    o = torch.zeros(1, dtype=torch.int64, device=dev)
    hw = torch.full((1,), 8, dtype=torch.int32, device=dev)
    out = torch.full((3 * 32 * 32,), 7, dtype=torch.uint8, device=dev)
    st = torch.full((1,), 99, dtype=torch.int32, device=dev)

    def go(S=32, u8=out, f32=None, status=st, n=1, nbytes=4096):
        return call("mmvae_imgprep_scale_crop", ptr(p), nbytes, ptr(o), ptr(hw), ptr(hw), n, S, ptr(u8), ptr(f32), ptr(status), None)
    for kw in (dict(S=0), dict(S=129), dict(u8=None, f32=None), dict(status=None), dict(n=-1), dict(nbytes=-1)):
        with pytest.raises(MMVAEError, match=r"failed \(-1\)"):   # MMVAE_EINVAL
            go(**kw)
    torch.cuda.synchronize()
    assert int(st[0]) == 99 and bool((out == 7).all())            # nothing ran
    assert go(n=0) == 0
    torch.cuda.synchronize()
    assert int(st[0]) == 99
    assert go() == 0
    torch.cuda.synchronize()
    assert int(st[0]) == 0 and bool((out == 0).all())             # the 8 x 8 zeros image, scaled
