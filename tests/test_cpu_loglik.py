"""Host side of the importance-sampled evaluation: the loglik command line and the particle-chunk planner."""
import itertools

import pytest


def test_loglik_parser_keeps_the_reference_flags():
    from multimodal_vae_amd.evaluate import _parser
    a = _parser().parse_args(["loglik", "model.pth.tar"])
    assert a.cmd == "loglik" and a.model_path == "model.pth.tar"
    # multimnist/loglikelihood.py: --image_only, --text_only, --n_samples 100, --cuda
    assert (a.image_only, a.text_only, a.all, a.n_samples, a.cuda) == (False, False, False, 100, False)
    assert (a.batch_size, a.data, a.synthetic, a.seed, a.json) == (64, "./data", 0, 0, None)
    a = _parser().parse_args(["loglik", "m", "--image_only", "--n_samples", "1000", "--cuda", "--batch_size", "32",
                              "--synthetic", "10", "--seed", "4", "--json", "o.json"])
    assert (a.image_only, a.n_samples, a.cuda, a.batch_size, a.synthetic, a.seed, a.json) == (True, 1000, True, 32, 10, 4, "o.json")
    assert _parser().parse_args(["loglik", "m", "--text_only"]).text_only
    assert _parser().parse_args(["loglik", "m", "--all"]).all
    for bad in (["--image_only", "--text_only"], ["--all", "--image_only"], ["--data", "d", "--synthetic", "3"]):
        with pytest.raises(SystemExit):
            _parser().parse_args(["loglik", "m"] + bad)
    s = _parser().parse_args(["sample", "m"])                     # the sample subcommand is unchanged
    assert (s.cmd, s.n_samples, s.out) == ("sample", 64, "./results")


@pytest.mark.parametrize("B,K,cap", list(itertools.product((1, 3, 13, 64, 100), (1, 7, 64, 1000), (1, 5, 64, 100, 4096))))
def test_iw_chunks_cover_every_pair_once(B, K, cap):
    from multimodal_vae_amd.evaluate import iw_chunks
    seen = set()
    for r0, nr, k0, nk in iw_chunks(B, K, cap):
        assert nr >= 1 and nk >= 1 and nr * nk <= cap
        for pair in itertools.product(range(r0, r0 + nr), range(k0, k0 + nk)):
            assert pair not in seen, pair
            seen.add(pair)
    assert len(seen) == B * K and all(0 <= b < B and 0 <= k < K for b, k in seen)


def test_iw_chunks_use_the_capacity():
    from multimodal_vae_amd.evaluate import iw_chunks
    ch = iw_chunks(64, 1000, 4096)
    assert len(ch) == 16 and all(nr == 64 for _, nr, _, _ in ch)            # 64 particles per call at most: 16 calls
    assert iw_chunks(16, 1000, 4096) == [(0, 16, k0, 250) for k0 in range(0, 1000, 250)]
    assert iw_chunks(10, 3, 1) == [(r, 1, k, 1) for r in range(10) for k in range(3)]
    with pytest.raises(ValueError):
        iw_chunks(0, 1, 1)
