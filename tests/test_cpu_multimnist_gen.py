"""MultiMNIST generator, the parts that need no GPU (multimodal-vae_amd/csrc/mmgen_core.h, multimnist_gen.py): the restated Pillow
resize against a recorded fixture (tools/record_pillow_resize.py) and against live Pillow, the host table builder against the numpy
restatement, the side distribution against the reference's ``int(28 * (1 / (0.1 * randn() + 1.3)))``, the wrappers' refusals, the
conditions the GPU tests' inputs have to meet (asserted on the reference alone), and the header itself as a stand-alone host program
under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multimnist_gen_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pillow_bilinear_28.npz")


def test_restated_resize_equals_recorded_pillow():
    z = np.load(GOLDEN)
    assert list(z["sides"]) == list(range(R.SIDE_MIN, R.SIDE_MAX + 1)) and str(z["pillow_version"])
    for s in z["sides"]:
        want = z["side_%d" % s]
        for i, im in enumerate(z["images"]):
            assert np.array_equal(R.resize(im, int(s)), want[i]), (int(s), i)


def test_restated_resize_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(5)
    imgs = [rng.randint(0, 256, (28, 28)).astype(np.uint8), np.full((28, 28), 255, np.uint8),
            np.where(rng.rand(28, 28) < 0.08, 255, 0).astype(np.uint8)]
    for s in range(1, 50):                               # beyond the generator's sides too: the restatement is Pillow's, not a fit
        for i, im in enumerate(imgs):
            want = np.asarray(Image.fromarray(im, "L").resize((s, s), Image.BILINEAR))
            assert np.array_equal(R.resize(im, s), want), (s, i)


def test_identity_at_28():
    im = np.random.RandomState(1).randint(0, 256, (28, 28)).astype(np.uint8)
    assert np.array_equal(R.resize(im, 28), im)          # no_resize may share the resize path


def test_host_tables_equal_numpy_tables():
    from multimodal_vae_amd import multimnist_gen as G
    lo, hi, taps, attempts, redraws, canvas = G.mmgen_geometry()
    assert (lo, hi, taps, attempts, redraws, canvas) == (R.SIDE_MIN, R.SIDE_MAX, R.MAX_TAPS, R.MAX_ATTEMPTS, R.MAX_REDRAWS, R.CANVAS)
    got = G.build_tables().numpy()
    want = R.tables()
    assert got.shape == want.shape == (R.TABLE_WORDS,) and np.array_equal(got, want)
    counts = want[:R.T_OFFSET].reshape(R.N_SIDES, R.SIDE_MAX, R.COEF_WORDS)[:, :, 1]
    assert 1 <= counts.max() <= R.MAX_TAPS               # the tap bound
    for s in range(R.SIDE_MIN, R.SIDE_MAX + 1):
        assert (counts[s - R.SIDE_MIN, :s] >= 1).all() and (counts[s - R.SIDE_MIN, s:] == 0).all()
    T = want[R.T_OFFSET:].view(np.uint32)
    assert (np.diff(T.astype(np.int64)) >= 0).all() and T[-1] == 0xffffffff


def test_side_frequencies_match_the_reference_distribution():
    n = 200000
    got = R.side_of(R.philox(3, np.arange(n), 1)[:, 1])
    rng = np.random.RandomState(681307)
    want = (28 * (1.0 / (0.1 * rng.randn(n) + 1.3))).astype(int)
    assert got.min() >= R.SIDE_MIN and got.max() <= R.SIDE_MAX and want.min() >= R.SIDE_MIN and want.max() <= R.SIDE_MAX
    for s in range(R.SIDE_MIN, R.SIDE_MAX + 1):
        a, b = int((got == s).sum()), int((want == s).sum())
        p = (a + b) / (2.0 * n)
        sd = np.sqrt(2.0 * n * p * (1.0 - p))            # of the difference of two binomial counts
        assert abs(a - b) <= 5.0 * sd + 1e-9, (s, a, b)


def test_wrappers_refuse_before_anything_is_launched():
    from multimodal_vae_amd import MMVAEError
    from multimodal_vae_amd import multimnist_gen as G
    d, l = torch.zeros(4, 28, 28, dtype=torch.uint8), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(MMVAEError, match="no CPU fallback"):
        G.generate(d, l, 3)
    with pytest.raises(MMVAEError, match="no CPU fallback"):
        G.render(d, torch.zeros(1, 4, 4, dtype=torch.int32))
    for bad in ("no_repeat", "scramble", "reverse"):
        with pytest.raises(MMVAEError, match="%s needs fixed" % bad):
            G.generate(d, l, 3, **{bad: True})
        with pytest.raises(MMVAEError, match="%s needs fixed" % bad):
            G.MultiMNISTStream(d, l, 2, "cpu", **{bad: True})
    for lo, hi in ((-1, 2), (3, 2), (0, 5)):
        with pytest.raises(MMVAEError, match="min <= max <= 4"):
            G.generate(d, l, 3, min_digits=lo, max_digits=hi)
    assert G.mode_flags(fixed=True, reverse=True, scramble=True)[0] == G.F_FIXED | G.F_SCRAMBLE      # datasets.py:311-313
    assert G.mode_flags(resize=False, translate=False) == (G.F_NO_RESIZE | G.F_NO_TRANSLATE, 0, 2)


def test_c_abi_refuses_bad_arguments_without_a_gpu():
    import ctypes as C
    from multimodal_vae_amd import MMVAEError
    from multimodal_vae_amd._lib import call
    p = C.c_void_p(4096)                                  # never dereferenced: every call below is refused first
    ok = dict(digits=p, labels=p, M=4, tables=p, flags=0, lo=0, hi=2, n=1, u8=p, f32=None, text=p)

    def gen(**kw):
        a = dict(ok, **kw)
        return call("mmvae_mmgen_generate", a["digits"], a["labels"], a["M"], a["tables"], a["flags"], a["lo"], a["hi"], 0, 0, a["n"], a["u8"], a["f32"],
                    a["text"], None, None, None, None)
    for kw in (dict(digits=None), dict(labels=None), dict(tables=None), dict(text=None), dict(u8=None), dict(M=0), dict(n=-1), dict(hi=5),
               dict(lo=3), dict(lo=-1), dict(flags=8), dict(flags=16), dict(flags=32), dict(flags=64), dict(digits=C.c_void_p(4097)),
               dict(u8=None, f32=C.c_void_p(4100))):
        with pytest.raises(MMVAEError):
            gen(**kw)
    with pytest.raises(MMVAEError):
        call("mmvae_mmgen_render", p, 4, p, None, 1, p, None, p, None)
    with pytest.raises(MMVAEError):
        call("mmvae_mmgen_render", p, 4, p, p, 1, p, None, None, None)
    with pytest.raises(MMVAEError):
        call("mmvae_mmgen_build_tables", None)


def test_conditions_on_the_gpu_tests_inputs():
    """what makes the GPU comparison meaningful, on the reference alone: the 257-canvas case retries often but stays far from the
    attempt bound; no case has a failed canvas; the crafted fixed-mode case does retry"""
    attempts = R.case("random_0_4")[5][3]
    assert len(attempts) == 257 and attempts.min() >= 1 and attempts.max() <= 32
    assert int((attempts >= 2).sum()) >= 16 and int((attempts >= 3).sum()) >= 1
    for name in R.CASES:
        d, l, n, seed, mode, (images, text, params, att) = R.case(name)
        assert att.min() >= 1 and att.max() <= 48, name
        k = (params[:, :, 0] >= 0).sum(1)
        assert k.min() == mode["min_digits"] and k.max() == mode["max_digits"], name
        assert ((text != R.FILL).sum(1) == k).all()
    assert int((R.case("fixed_crafted")[5][3] >= 2).sum()) >= 4
    p = R.case("random_0_4")[5][2]
    sides = p[:, :, 1][p[:, :, 0] >= 0]
    assert sides.min() <= 19 and sides.max() >= 25       # both the shrinking and the (nearly) unscaled end
    # fixed mode: labels of a no_repeat canvas are distinct; reverse and scramble do permute some canvas
    _, l, _, _, _, (_, text, params, _) = R.case("fixed_no_repeat")
    for row in text:
        digs = [v for v in row if v != R.FILL]
        assert len(set(digs)) == len(digs)
    for name in ("fixed_reverse", "fixed_scramble"):
        _, l, _, _, _, (_, text, params, _) = R.case(name)
        plain = np.where(params[:, :, 0] >= 0, l[np.maximum(params[:, :, 0], 0)], R.FILL)
        assert (plain != text).any(1).sum() >= 4 and (np.sort(plain, 1) == np.sort(text, 1)).all(), name


def test_core_header_as_a_host_program_under_sanitizers(tmp_path):
    """csrc/mmgen_core.h is plain C++17: tests/host/mmgen_core_check.cpp (its own main) builds the tables and draws a few hundred
    canvases with it under -fsanitize=address,undefined; what it prints equals the numpy restatement"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "mmgen_core_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "multimodal-vae_amd", "csrc"), os.path.join(ROOT, "tests", "host", "mmgen_core_check.cpp"), "-o", exe], check=True)
    seed, first, n, M = 0x1234567890, (1 << 32) - 100, 200, 60000
    r = subprocess.run([exe, str(seed), str(first), str(n), str(M)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    most = int(R.tables()[:R.T_OFFSET].reshape(-1, R.COEF_WORDS)[:, 1].max())
    assert lines[-1] == "ok" and lines[0] == "taps %d words %d" % (most, R.TABLE_WORDS) and most <= R.MAX_TAPS
    assert np.array_equal(np.array(lines[1].split()[1:], dtype=np.int64), R.tables().astype(np.int64))
    n_canvas = n_digit = n_line = 0
    for ln in lines[2:-1]:
        w = ln.split()
        if w[0] == "canvas":
            flags, c, k, rev, scr = (int(v) for v in w[1:6])
            rr = R.philox(seed, c, 0)
            assert k == int(R.mulhi(rr[0], 5)) and rev == int(rr[1]) >> 31 and scr == int(R.mulhi(rr[2], [1, 1, 2, 6, 24][k])), ln
            assert [int(v) for v in w[7:]] == R.label_order(k, rev, scr, flags), ln
            n_canvas += 1
        elif w[0] == "digit":
            flags, c, a, j, t = (int(v) for v in w[1:6])
            assert tuple(int(v) for v in w[6:]) == R.draw_digit(seed, c, a, j, t, flags, M), ln
            n_digit += 1
        else:
            assert w[0] == "line"
            s = int(w[1])
            line = ((np.arange(28) * 37 + 11) & 255).astype(np.uint8)
            assert np.array_equal(np.array(w[2:], dtype=np.int64), R._pass(line[None], R.dense(s))[0]), ln
            n_line += 1
    assert (n_canvas, n_digit, n_line) == (5 * n, 5 * n * 24, R.N_SIDES)
