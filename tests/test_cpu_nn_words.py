"""Host side of the nearest-word decoding (no GPU): the reference code of tests/nn_words_ref.py checks itself, coco.WordTable's
host logic runs behind a stub search, and the C boundary refuses bad arguments before it would launch anything."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nn_words_ref as R  # noqa: E402


# ------------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("kind", ["near", "rand"])
def test_gate_exceeds_the_error_of_cpu_fp32_and_the_inputs_meet_their_premises(kind):
    W, idx, Qn, Qr = R.real_inputs()
    Q = Qn if kind == "near" else Qr
    d2 = R.real_d2(kind)
    s32 = (W * W).sum(1)[None, :] - 2.0 * (Q @ W.t())             # torch's own fp32 score on the CPU
    s64 = (W.double() ** 2).sum(1)[None, :] - 2.0 * (Q.double() @ W.double().t())
    qn, wn = Q.double().norm(dim=1)[:, None], W.double().norm(dim=1)[None, :]
    E = R.GATE_C * (wn * wn + 2 * qn * wn)
    assert float(((s32.double() - s64).abs() / E).max()) < 1.0
    j = R.judge(Q, W, s32.argmin(1), d2)
    assert j["wrong_decided"] == 0 and j["regret_ratio"] <= 1.0 and j["undecided_share"] <= 0.05
    if kind == "near":
        assert torch.equal(j["best"], idx) and j["min_gap_ratio"] > 1e4
    # closest(vec, 10) on the first two queries: the float64 top 11 are further apart than twice the distance bound
    t = torch.topk(d2[:2].sqrt(), 11, dim=1, largest=False).values
    assert float((t[:, 1:] - t[:, :-1]).min()) > 2 * (R.DIST_RTOL * float(t.max()) + R.DIST_ATOL)


def test_reference_tie_rule_and_integer_distances():
    d2 = torch.tensor([[3.0, 1.0, 1.0, 2.0], [0.0, 0.0, 0.0, 0.0], [5.0, 4.0, 3.0, 3.0]], dtype=torch.float64)
    assert R.argmin_lowest(d2).tolist() == [1, 0, 2]
    A, B, Cc = R.int_tables(70, 32, 64)
    assert R.duplicate_rows(70, 32, 64) == [31, 32, 64, 69]
    assert torch.allclose(R.sqdist64_int(A[:9], B), R.sqdist64(A[:9], B), rtol=1e-13, atol=0)   # the expansion is exact on integers
    q = A[3:4]
    assert R.argmin_lowest(R.sqdist64_int(q, B)).item() == 3 and R.argmin_lowest(R.sqdist64_int(q, Cc)).item() == 31
    ints = torch.arange(0, 4801, dtype=torch.float64)             # every distance^2 the exact regime can produce (300 * 16)
    roots = R.sqrt_f32_of_int(ints)
    assert roots.dtype == torch.float32 and roots[1206].item() == float.fromhex("0x1.15d1f2p+5") and roots[4].item() == 2.0
    lo, hi = torch.nextafter(roots, torch.zeros(())).double(), torch.nextafter(roots, torch.full((), 1e9)).double()
    err = (roots.double() ** 2 - ints).abs()                      # nearer to the integer than either neighbour's square
    assert bool((err[1:] <= (lo[1:] ** 2 - ints[1:]).abs()).all() and (err <= (hi ** 2 - ints).abs()).all())
    j = R.judge(q, B, torch.tensor([31]))
    assert not bool(j["decided"][0]) and j["regret_ratio"] == 0.0 and j["wrong_decided"] == 0


# ------------------------------------------------------------------------------------------------------ WordTable, host logic
def small_table():
    from multimodal_vae_amd import coco as K, data as D
    vectors, itos = D.synthetic_word_table(40, seed=2)
    return K.WordTable(vectors, itos), vectors, itos


def stub_search(tab):
    """Replaces the device search of a host-only table with float64 on the CPU (test scaffolding, not a fallback)."""
    def nearest(vecs):
        d2 = R.sqdist64(torch.as_tensor(vecs).reshape(-1, R.DIM).float().cpu(), tab.vectors)
        i = R.argmin_lowest(d2)
        return i, d2[torch.arange(len(i)), i].sqrt().float()

    def dists(vecs):
        return R.sqdist64(torch.as_tensor(vecs).reshape(-1, R.DIM).float().cpu(), tab.vectors).sqrt().float()
    tab.nearest, tab.dists = nearest, dists
    return tab


def test_synthetic_table_and_file_round_trip(tmp_path):
    from multimodal_vae_amd import coco as K, data as D
    vectors, itos = D.synthetic_word_table(40, seed=2)
    assert vectors.shape == (40, 300) and vectors.dtype == torch.float32 and 0.35 < float(vectors.std()) < 0.45
    assert itos[:3] == ['<s>', '</s>', 'w0'] and itos[-1] == 'w37' and len(set(itos)) == 40
    assert torch.equal(D.synthetic_word_table(40, seed=2)[0], vectors)
    with pytest.raises(ValueError):
        D.synthetic_word_table(2)
    path = str(tmp_path / "table.pt")
    K.save_word_table(path, vectors, itos)
    raw = torch.load(path, weights_only=True)
    assert isinstance(raw, tuple) and raw[0].dtype == torch.float32 and tuple(raw[0].shape) == (40, 300) and raw[1] == itos
    tab = K.load_word_table(path)
    assert tab.itos == itos and torch.equal(tab.vectors, vectors) and len(tab) == 40 and tab.device is None
    assert torch.equal(tab.get_word('w5'), vectors[7]) and tab.get_word('nope') is None
    assert tab.stoi['</s>'] == 1


def test_word_table_refusals(tmp_path):
    from multimodal_vae_amd import coco as K, MMVAEError
    tab, vectors, itos = small_table()
    bad = vectors.clone()
    bad[5, 7] = float('nan')
    with pytest.raises(MMVAEError, match="non-finite"):
        K.WordTable(bad, itos)
    bad[5, 7] = float('inf')
    with pytest.raises(MMVAEError, match="non-finite"):
        K.WordTable(bad, itos)
    with pytest.raises(MMVAEError, match="duplicate"):
        K.WordTable(vectors, itos[:-1] + [itos[0]])
    with pytest.raises(MMVAEError, match="39 words for 40"):
        K.WordTable(vectors, itos[:-1])
    with pytest.raises(MMVAEError, match=r"\(V, 300\)"):
        K.WordTable(vectors[:, :299], itos)
    with pytest.raises(MMVAEError, match="float32"):
        K.WordTable(vectors.double(), itos)
    with pytest.raises(MMVAEError, match="duplicate"):
        K.save_word_table(str(tmp_path / "t.pt"), vectors, itos[:-1] + [itos[0]])
    assert not os.path.exists(str(tmp_path / "t.pt"))
    with pytest.raises(MMVAEError, match="no CPU fallback"):      # a host-only table does not search
        tab.nearest(vectors[:2])
    with pytest.raises(MMVAEError, match="GPU only"):
        K.WordTable(vectors, itos, device="cpu")


def test_embed():
    from multimodal_vae_amd import coco as K
    tab, vectors, itos = small_table()
    e = tab.embed("w1 zebra w2")
    assert e.shape == (102, 300) and e.dtype == torch.float32
    assert torch.equal(e[0], vectors[0]) and torch.equal(e[1], vectors[3]) and not e[2].any()
    assert torch.equal(e[3], vectors[4]) and torch.equal(e[4], vectors[1]) and not e[5:].any()
    long = tab.embed(" ".join(["w3"] * 150))                      # truncation to 100 words: <s> + 100 + </s>
    assert torch.equal(long[0], vectors[0]) and torch.equal(long[101], vectors[1])
    assert all(torch.equal(long[i], vectors[5]) for i in (1, 50, 100))
    assert not tab.embed("")[2:].any() and torch.equal(tab.embed("")[1], vectors[1])
    assert torch.equal(tab.embed("w1,w2", tokenizer=lambda s: s.split(","))[2], vectors[4])
    assert (K.SOS, K.EOS, K.MAX_WORDS) == ('<s>', '</s>', 102)


def test_closest_closest_batch_and_analogy_behind_a_stub():
    tab, vectors, itos = small_table()
    stub_search(tab)
    q = vectors[[9, 1, 30]] + 0.01
    assert tab.closest_batch(q) == [itos[9], itos[1], itos[30]]
    found = tab.closest(vectors[9] + 0.01, 4)
    assert len(found) == 4 and found[0][0] == itos[9] and [d for _, d in found] == sorted(d for _, d in found)
    assert abs(found[0][1] - 0.01 * 300 ** 0.5) < 1e-5
    assert len(tab.closest(vectors[0], 100)) == 40
    # analogy: w2 - w1 + w3 with w1 == w3 is w2 itself: it comes first unfiltered and is dropped when filtered
    full = tab.analogy('w4', 'w7', 'w4', n=5, filter_given=False)
    assert len(full) == 5 and full[0][0] == 'w7'
    kept = tab.analogy('w4', 'w7', 'w4', n=5)
    assert len(kept) == 5 and not {'w4', 'w7'} & {w for w, _ in kept}
    assert [w for w, _ in kept] == [w for w, _ in tab.analogy('w4', 'w7', 'w4', n=8, filter_given=False) if w not in ('w4', 'w7')][:5]
    with pytest.raises(KeyError):
        tab.analogy('w4', 'nope', 'w4')


def test_sentence_assembly_and_stop_at_eos():
    from multimodal_vae_amd import coco as K
    strings = ['a', 'b', '</s>', 'c', '</s>', 'd', 'e', 'f', 'g', 'h', 'i', 'j']
    assert K.assemble_sentences(strings, 3, 4) == ['a b </s> c', '</s> d e f', 'g h i j']
    assert K.assemble_sentences(strings, 3, 4, stop_at_eos=True) == ['a b', '', 'g h i j']
    assert K.assemble_sentences(strings, 2, 6, stop_at_eos=True) == ['a b', 'e f g h i j']
    with pytest.raises(AssertionError):
        K.assemble_sentences(strings, 5, 2)


def test_generate_assembles_the_words_of_forward_behind_a_stub():
    from multimodal_vae_amd import coco as K
    tab, vectors, itos = small_table()
    stub_search(tab)
    dec = K.TextDecoder(20, words=tab, steps=5)
    assert torch.equal(dec.sos, vectors[0])                       # sos defaults to the table's '<s>'
    rows = [3, 9, 1, 30, 4, 1, 8, 8, 8, 8]
    dec.forward = lambda z: vectors[rows].reshape(2, 5, 300)      # the device forward, replaced by known vectors
    assert dec.generate(torch.zeros(2, 20)) == ['w1 w7 </s> w28 w2', '</s> w6 w6 w6 w6']
    assert dec.generate(torch.zeros(2, 20), stop_at_eos=True) == ['w1 w7', '']


def test_model_wiring_keeps_the_state_dict_and_the_old_refusals():
    from multimodal_vae_amd import coco as K, MMVAEError
    tab, vectors, itos = small_table()
    plain = K.MultimodalVAE(20, sos=vectors[0])
    wired = K.MultimodalVAE(20, words=tab)
    assert list(plain.state_dict().keys()) == list(wired.state_dict().keys())
    assert [n for n, _ in plain.named_buffers()] == [n for n, _ in wired.named_buffers()]
    assert wired.text_decoder.words is tab and torch.equal(wired.text_decoder.sos, vectors[0])
    other = K.MultimodalVAE(20, sos=vectors[7], words=tab)        # an explicit sos wins
    assert torch.equal(other.text_decoder.sos, vectors[7])
    with pytest.raises(MMVAEError) as e:
        plain.text_decoder.generate(torch.zeros(1, 20))
    assert str(e.value) == ("TextDecoder.generate (coco/model.py:290-306) decodes vectors to words through the GloVe table, "
                            "which is not part of this engine; use generate_vector")
    with pytest.raises(MMVAEError, match="TextDecoder needs sos="):
        K.MultimodalVAE(20)
    no_sos = K.WordTable(vectors[2:], itos[2:])
    with pytest.raises(MMVAEError, match="has no '<s>'"):
        K.MultimodalVAE(20, words=no_sos)


def test_sample_coco_parser():
    from multimodal_vae_amd.evaluate import _parser
    p = _parser()
    a = p.parse_args(["sample_coco", "ck.pth.tar", "--words", "table.pt"])
    assert (a.cmd, a.model_path, a.words, a.synthetic_words, a.n_samples, a.condition_on_image, a.condition_on_text, a.out, a.seed) == \
        ("sample_coco", "ck.pth.tar", "table.pt", 0, 64, None, None, "./results", 0)
    a = p.parse_args(["sample_coco", "ck", "--synthetic_words", "5000", "--n_samples", "3", "--condition_on_text", "a man riding a wave",
                      "--condition_on_image", "im.pt", "--out", "o", "--seed", "4", "--stop_at_eos"])
    assert (a.synthetic_words, a.n_samples, a.condition_on_text, a.condition_on_image, a.out, a.seed, a.stop_at_eos) == \
        (5000, 3, "a man riding a wave", "im.pt", "o", 4, True)
    for bad in (["sample_coco", "ck"], ["sample_coco", "ck", "--words", "t.pt", "--synthetic_words", "5"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    a = p.parse_args(["sample", "m.pth.tar"])                      # the existing subcommands parse as before
    assert a.cmd == "sample" and a.n_samples == 64 and not hasattr(a, "words")


# ------------------------------------------------------------------------------------------------------ the C boundary
def test_c_boundary_refuses_before_it_launches():
    """Every refusal is decided on the host from the arguments alone, so it can be seen without a device: the pointers here are
    host dummies that a launch would fault on."""
    from multimodal_vae_amd import coco as K
    from multimodal_vae_amd._lib import MMVAEError, SIGNATURES, call, load
    lib = load()
    TQ, TV, S = K.nn_words_geometry()
    assert TQ % 32 == 0 and TQ >= 32 and TV >= 1 and S >= 1
    dummy = (C.c_float * 16)()
    p = C.cast(dummy, C.c_void_p)
    assert len(SIGNATURES["mmvae_nn_words_nearest"][1]) == 11 and len(SIGNATURES["mmvae_nn_words_dists"][1]) == 7
    need = call("mmvae_nn_words_workspace_bytes", 102, 2196017)
    assert need >= 102 * 8 and call("mmvae_nn_words_workspace_bytes", 6528, 2196017) >= 6528 * 8
    assert call("mmvae_nn_words_workspace_bytes", 0, 5) == 0 and call("mmvae_nn_words_workspace_bytes", 5, 0) == 0
    cases = [
        ("mmvae_nn_words_norms", [None, 5, 300, p, None], "null"),
        ("mmvae_nn_words_norms", [p, 5, 300, None, None], "null"),
        ("mmvae_nn_words_norms", [p, 0, 300, p, None], "n_words"),
        ("mmvae_nn_words_norms", [p, 5, 128, p, None], "dim = 128"),
        ("mmvae_nn_words_nearest", [None, 2, p, p, 5, 300, p, need, p, p, None], "null"),
        ("mmvae_nn_words_nearest", [p, 2, None, p, 5, 300, p, need, p, p, None], "null"),
        ("mmvae_nn_words_nearest", [p, 2, p, None, 5, 300, p, need, p, p, None], "null"),
        ("mmvae_nn_words_nearest", [p, 2, p, p, 5, 300, None, need, p, p, None], "null"),
        ("mmvae_nn_words_nearest", [p, 2, p, p, 5, 300, p, need, None, p, None], "null"),
        ("mmvae_nn_words_nearest", [p, 2, p, p, 5, 300, p, need, p, None, None], "null"),
        ("mmvae_nn_words_nearest", [p, 0, p, p, 5, 300, p, need, p, p, None], "n_queries = 0"),
        ("mmvae_nn_words_nearest", [p, 2, p, p, 0, 300, p, need, p, p, None], "n_words = 0"),
        ("mmvae_nn_words_nearest", [p, 2, p, p, 5, 50, p, need, p, p, None], "dim = 50"),
        ("mmvae_nn_words_nearest", [p, 102, p, p, 2196017, 300, p, need - 1, p, p, None], "workspace too small"),
        ("mmvae_nn_words_dists", [None, 2, p, 5, 300, p, None], "null"),
        ("mmvae_nn_words_dists", [p, 2, None, 5, 300, p, None], "null"),
        ("mmvae_nn_words_dists", [p, 2, p, 5, 300, None, None], "null"),
        ("mmvae_nn_words_dists", [p, 0, p, 5, 300, p, None], "n_queries = 0"),
        ("mmvae_nn_words_dists", [p, 9, p, 5, 300, p, None], "n_queries = 9"),
        ("mmvae_nn_words_dists", [p, 2, p, 0, 300, p, None], "n_words = 0"),
        ("mmvae_nn_words_dists", [p, 2, p, 5, 299, p, None], "dim = 299"),
    ]
    for name, args, words in cases:
        with pytest.raises(MMVAEError, match=words):
            call(name, *args)
        assert words.encode() in lib.mmvae_last_error()
