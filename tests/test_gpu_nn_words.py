"""Nearest-word search on the device (csrc/nn_words.hip through coco.WordTable and the C entry points) against float64.

The shapes come from mmvae_nn_words_geometry (TQ query rows per workgroup, TV words per vocabulary tile, at most S splits), so
the edges are the kernel's own.  Reference, gate and inputs: tests/nn_words_ref.py.

The real-valued tests print their figures (undecided share, mismatches, worst regret / gate, worst relative distance error)
before they assert; run with -s to see them.  DESIGN.md section 4.2d records them.
"""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nn_words_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def geometry():
    from multimodal_vae_amd.coco import nn_words_geometry
    return nn_words_geometry()


def splits(N, V):
    """The documented split rule of include/mmvae_hip.h -> (S, first tile of every split)."""
    TQ, TV, MS = geometry()
    T = -(-V // TV)
    S = max(1, min(MS, T, 1024 // -(-N // TQ)))
    return S, [T * s // S for s in range(S)]


def table_of(W):
    from multimodal_vae_amd.coco import WordTable
    return WordTable(W, ["w%d" % i for i in range(W.shape[0])], device=DEV)


@functools.lru_cache(maxsize=None)
def real_table():
    return table_of(R.real_inputs()[0])


def nearest(tab, Q):
    i, d = tab.nearest(Q)
    torch.cuda.synchronize()
    return i.cpu(), d.cpu()


# ------------------------------------------------------------------------------------------------------ 1. exact regime
def exact_shapes():
    TQ, TV, S = geometry()
    return [1, TQ - 1, TQ, TQ + 1, 2 * TQ + 3], [1, 5, TV - 1, TV, TV + 1, S * TV + 1, 2 * S * TV + 7]


def winner_rows(N, V):
    """row 0, TV-1, TV, V-1, row 3 and both sides of every split boundary of this shape (as far as they exist)."""
    TV = geometry()[1]
    rows = [0, TV - 1, TV, V - 1, 3]
    for t in splits(N, V)[1][1:]:
        rows += [t * TV - 1, t * TV]
    seen, out = set(), []
    for r in rows:
        if 0 <= r < V and r not in seen:
            seen.add(r)
            out.append(r)
    return out


def check_exact(W, Q, what):
    ref = R.sqdist64_int(Q, W)
    want = R.argmin_lowest(ref)
    got, dist = nearest(table_of(W), Q)
    assert torch.equal(got, want), (what, (got != want).nonzero().flatten()[:8].tolist())
    rows = torch.arange(Q.shape[0])
    assert torch.equal(dist, R.sqrt_f32_of_int(ref[rows, want])), what
    return got


def _ids():
    return ["N%d-V%d" % (n, v) for n in range(5) for v in range(7)]


@pytest.mark.parametrize("ni,vi", [(n, v) for n in range(5) for v in range(7)], ids=_ids())
def test_exact_regime_every_shape(ni, vi):
    """Integer entries in {-2..2}: index torch.equal to the float64 lowest-index arg-min, dist == sqrt of the exact integer.
    Queries: copies of the winner rows (distance 0), then integer rows of their own; cut to N."""
    Ns, Vs = exact_shapes()
    N, V = Ns[ni], Vs[vi]
    TV = geometry()[1]
    S, first = splits(N, V)
    A, B, Cc = R.int_tables(V, TV, first[-1] * TV)
    win = winner_rows(N, V)
    Q = torch.cat([A[win], R.int_rows(N, 5)])[:N].contiguous()
    got = check_exact(A, Q, "distinct rows")
    k = min(N, len(win))
    assert got[:k].tolist() == win[:k]                           # a copy of a row of a table of distinct rows finds that row
    # duplicates: table B holds row 3's value at 3 and at the duplicate rows, table C only at the duplicate rows
    dup = R.duplicate_rows(V, TV, first[-1] * TV)
    if V > 3:
        Qd = A[3].expand(N, R.DIM).contiguous()
        assert check_exact(B, Qd, "duplicates, lowest copy at 3").tolist() == [3] * N
        if dup:
            assert check_exact(Cc, Qd, "duplicates, lowest copy at %d" % dup[0]).tolist() == [dup[0]] * N
    check_exact(B, Q, "table with duplicates")


def test_exact_regime_every_tile_boundary():
    """V = S TV + 1: a winner on both sides of EVERY tile boundary (a split boundary is one of them whatever the split
    count), in one call and in calls of other query counts, which split the vocabulary differently."""
    TQ, TV, S = geometry()
    V = S * TV + 1
    A = R.int_tables(V, TV, splits(1, V)[1][-1] * TV)[0]
    rows = torch.tensor([r for t in range(1, S + 1) for r in (t * TV - 1, t * TV)] + [0, V - 1])
    Q = A[rows].contiguous()
    tab = table_of(A)
    got, dist = nearest(tab, Q)
    assert torch.equal(got, rows) and not dist.any()
    for n in (1, TQ + 1, 4 * TQ):                                # 512, 512 and 256 splits
        g, d = nearest(tab, Q[:n])
        assert torch.equal(g, rows[:n]) and not d.any()


# ------------------------------------------------------------------------------------------------------ 2, 3. real values
def test_near_construction_returns_the_planted_word():
    W, idx, Q, _ = R.real_inputs()
    d2 = R.real_d2("near")
    got, dist = nearest(real_table(), Q)
    j = R.judge(Q, W, got, d2)
    ok, worst = R.dist_within_bound(dist, d2[torch.arange(len(idx)), got])
    print("near construction: equal %d / %d, min gap / gate %.0f, worst relative distance error %.3g" %
          (int((got == idx).sum()), len(idx), j["min_gap_ratio"], worst))
    assert j["min_gap_ratio"] > 1e4                              # the premise: no conforming fp32 ranking can differ
    assert torch.equal(got, idx)
    assert ok, worst


def test_random_queries_within_the_gate():
    W, _, _, Q = R.real_inputs()
    d2 = R.real_d2("rand")
    got, dist = nearest(real_table(), Q)
    j = R.judge(Q, W, got, d2)
    ok, worst = R.dist_within_bound(dist, d2[torch.arange(Q.shape[0]), got])
    print("random queries: undecided share %.4f, mismatches %d (decided: %d), worst regret / gate %.3g, min gap / gate %.3g, "
          "worst relative distance error %.3g" % (j["undecided_share"], int((got != j["best"]).sum()), j["wrong_decided"],
                                                  j["regret_ratio"], j["min_gap_ratio"], worst))
    assert j["undecided_share"] <= 0.05
    assert j["wrong_decided"] == 0
    assert j["regret_ratio"] <= 1.0
    assert ok, worst


# ------------------------------------------------------------------------------------------------------ 4. two implementations
@pytest.mark.parametrize("kind", ["near", "rand"])
def test_dists_kernel_agrees_with_float64_and_with_nearest(kind):
    W, _, Qn, Qr = R.real_inputs()
    Q = (Qn if kind == "near" else Qr)[:8].contiguous()
    d2 = R.real_d2(kind)[:8]
    tab = real_table()
    rows = tab.dists(Q)
    torch.cuda.synchronize()
    ok, worst = R.dist_within_bound(rows, d2)
    print("dists rows (%s): worst relative error %.3g" % (kind, worst))
    assert rows.shape == (8, R.REAL_V) and ok, worst
    got, dist = nearest(tab, Q)
    top = torch.topk(rows, 1, dim=1, largest=False)
    assert torch.equal(top.indices[:, 0].cpu(), got)
    assert torch.equal(top.values[:, 0].cpu(), dist)             # one summation order for the distance, whoever computes it
    for i in range(2):
        found = tab.closest(Q[i], 10)
        ds = [d for _, d in found]
        assert ds == sorted(ds) and len(found) == 10
        want = torch.topk(d2[i], 10, largest=False, sorted=True).indices.tolist()
        assert [w for w, _ in found] == ["w%d" % k for k in want]


# ------------------------------------------------------------------------------------------------------ 5. independence
def test_same_call_twice_is_bit_equal_and_rows_do_not_depend_on_the_batch():
    TQ, TV, S = geometry()
    W, _, Qn, Qr = R.real_inputs()
    N = 2 * TQ + 3
    Q = torch.cat([Qr, Qn])[:N].contiguous()
    tab = real_table()
    i1, d1 = nearest(tab, Q)
    i2, d2 = nearest(tab, Q)
    assert torch.equal(i1, i2) and torch.equal(d1.view(torch.int32), d2.view(torch.int32))
    for r in (0, 31, 32, TQ - 1, TQ, 2 * TQ - 1, 2 * TQ, N - 1):
        i, d = nearest(tab, Q[r:r + 1])
        assert i.item() == i1[r].item() and torch.equal(d.view(torch.int32), d1[r:r + 1].view(torch.int32)), r
    i3, d3 = nearest(tab, Q[5:5 + TQ + 1])                      # another query count: another split of the vocabulary
    assert torch.equal(i3, i1[5:5 + TQ + 1]) and torch.equal(d3.view(torch.int32), d1[5:5 + TQ + 1].view(torch.int32))


def test_all_zero_query_block_returns_the_smallest_norm_word():
    TQ, TV, S = geometry()
    V = 3 * TV + 5
    A = R.int_tables(V, TV, splits(1, V)[1][-1] * TV)[0].clone()
    A[TV + 2] = 0.0
    A[TV + 2, 0] = 1.0                                           # the smallest norm, twice: the lower index wins
    A[2 * TV + 1] = A[TV + 2]
    Q = torch.cat([torch.zeros(TQ, R.DIM), R.int_rows(3, 9)])    # a whole query block of caption padding, then 3 live rows
    got = check_exact(A, Q, "zero rows")
    assert got[:TQ].tolist() == [TV + 2] * TQ


# ------------------------------------------------------------------------------------------------------ 6. large offsets
def test_table_past_4_gib():
    """V = 3,600,000 rows of 1200 bytes = 4.32 GB: byte offsets cross 2^31 and 2^32.  Planted queries = a row + 0.01 randn
    (random rows lie about 24 apart, the perturbation about 0.17), so the expected index needs no CPU reference."""
    from multimodal_vae_amd._lib import call, ptr
    V = 3_600_000
    r31, r32 = 2 ** 31 // 1200, 2 ** 32 // 1200
    rows = torch.tensor([0, r31 - 1, r31, r31 + 1, r32 - 1, r32, r32 + 1, V - 1])
    g = torch.Generator(device=DEV).manual_seed(3)
    W = torch.randn(V, R.DIM, device=DEV, generator=g).mul_(0.4)
    Q = (W[rows.to(DEV)] + 0.01 * torch.randn(8, R.DIM, device=DEV, generator=g)).contiguous()
    sq = torch.empty(V, dtype=torch.float32, device=DEV)
    index = torch.empty(8, dtype=torch.int64, device=DEV)
    dist = torch.empty(8, dtype=torch.float32, device=DEV)
    wsb = call("mmvae_nn_words_workspace_bytes", 8, V)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    call("mmvae_nn_words_norms", ptr(W), V, R.DIM, ptr(sq), None)
    call("mmvae_nn_words_nearest", ptr(Q), 8, ptr(W), ptr(sq), V, R.DIM, ptr(ws), wsb, ptr(index), ptr(dist), None)
    all_d = torch.empty(8, V, dtype=torch.float32, device=DEV)
    call("mmvae_nn_words_dists", ptr(Q), 8, ptr(W), V, R.DIM, ptr(all_d), None)
    torch.cuda.synchronize()
    planted = W[rows.to(DEV)].cpu()
    norms = sq[rows.to(DEV)].cpu()
    amin = all_d.argmin(dim=1).cpu()
    d_planted = all_d[torch.arange(8, device=DEV), rows.to(DEV)].cpu()
    got, dist = index.cpu(), dist.cpu()
    del W, sq, all_d, ws
    torch.cuda.empty_cache()
    assert torch.equal(got, rows), got.tolist()
    assert torch.equal(amin, rows), amin.tolist()
    ref = (Q.cpu().double() - planted.double()).pow(2).sum(1)
    assert R.dist_within_bound(dist, ref)[0] and torch.equal(d_planted, dist)
    n64 = planted.double().pow(2).sum(1)
    assert ((norms.double() - n64).abs() <= R.GATE_C * n64).all()  # a 300-term fp32 sum of squares: < 302 roundings


# ------------------------------------------------------------------------------------------------------ 7. boundary
def test_refused_arguments_launch_nothing_and_the_workspace_is_enough():
    from multimodal_vae_amd._lib import MMVAEError, call, ptr
    TQ, TV, S = geometry()
    V, N = 2 * TV + 1, 3
    A = R.int_tables(V, TV, splits(1, V)[1][-1] * TV)[0]
    W, Q = A.to(DEV), A[:N].to(DEV).contiguous()
    sq = torch.full((V,), -7.0, device=DEV)
    index = torch.full((N,), -7, dtype=torch.int64, device=DEV)
    dist = torch.full((N,), -7.0, device=DEV)
    all_d = torch.full((N, V), -7.0, device=DEV)
    wsb = call("mmvae_nn_words_workspace_bytes", N, V)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    good_norms = [ptr(W), V, R.DIM, ptr(sq), None]
    good_near = [ptr(Q), N, ptr(W), ptr(sq), V, R.DIM, ptr(ws), wsb, ptr(index), ptr(dist), None]
    good_dists = [ptr(Q), N, ptr(W), V, R.DIM, ptr(all_d), None]

    def refused(name, good, pos, value):
        args = list(good)
        args[pos] = value
        with pytest.raises(MMVAEError):
            call(name, *args)

    for pos in (0, 3):
        refused("mmvae_nn_words_norms", good_norms, pos, None)
    refused("mmvae_nn_words_norms", good_norms, 1, 0)
    refused("mmvae_nn_words_norms", good_norms, 2, 299)
    for pos in (0, 2, 3, 6, 8, 9):
        refused("mmvae_nn_words_nearest", good_near, pos, None)
    for pos, value in ((1, 0), (1, -1), (4, 0), (5, 304), (7, wsb - 1), (7, 0)):
        refused("mmvae_nn_words_nearest", good_near, pos, value)
    for pos in (0, 2, 5):
        refused("mmvae_nn_words_dists", good_dists, pos, None)
    for pos, value in ((1, 0), (1, 9), (3, 0), (4, 301)):
        refused("mmvae_nn_words_dists", good_dists, pos, value)
    assert call("mmvae_nn_words_workspace_bytes", 0, V) == 0 and call("mmvae_nn_words_workspace_bytes", N, 0) == 0
    torch.cuda.synchronize()
    for t in (sq, dist, all_d):
        assert bool((t == -7.0).all())                           # nothing ran
    assert bool((index == -7).all()) and not ws.any()
    # the workspace the library asks for is enough: a canary behind it stays intact at the shapes of the tests above
    Ns, Vs = exact_shapes()
    for n, v in [(Ns[-1], Vs[-1]), (Ns[0], Vs[-2]), (4 * TQ, Vs[-2]), (R.REAL_N, R.REAL_V), (1, 1)]:
        need = call("mmvae_nn_words_workspace_bytes", n, v)
        s_used = splits(n, v)[0]
        assert need >= s_used * n * 8                            # one (score, index) pair per (query, split)
        buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
        Wt = R.int_rows(v, 11).to(DEV)
        Qt = R.int_rows(n, 12).to(DEV)
        sqt = torch.empty(v, device=DEV)
        it = torch.empty(n, dtype=torch.int64, device=DEV)
        dt = torch.empty(n, device=DEV)
        call("mmvae_nn_words_norms", ptr(Wt), v, R.DIM, ptr(sqt), None)
        call("mmvae_nn_words_nearest", ptr(Qt), n, ptr(Wt), ptr(sqt), v, R.DIM, ptr(buf), need, ptr(it), ptr(dt), None)
        torch.cuda.synchronize()
        assert bool((buf[need:] == 0xA5).all()), (n, v)
        assert torch.equal(it.cpu(), R.argmin_lowest(R.sqdist64_int(Qt.cpu(), Wt.cpu())))


# ------------------------------------------------------------------------------------------------------ 8. end to end
@functools.lru_cache(maxsize=None)
def small_model():
    from multimodal_vae_amd import coco as K, data as D
    torch.manual_seed(0)
    vectors, itos = D.synthetic_word_table(5000, seed=0)
    words = K.WordTable(vectors, itos, device=DEV)
    vae = K.MultimodalVAE(n_latents=20, words=words).to(DEV).eval()
    return vae, words, vectors


def test_generate_is_the_float64_argmin_of_forward():
    vae, words, vectors = small_model()
    z = torch.randn(3, 20, generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        vecs = vae.text_decoder(z)
        sentences = vae.text_decoder.generate(z)
    torch.cuda.synchronize()
    T = vae.steps
    assert len(sentences) == 3 and all(len(s.split(' ')) == T for s in sentences)
    Q = vecs.reshape(-1, R.DIM).cpu()
    got = torch.tensor([words.stoi[w] for s in sentences for w in s.split(' ')])
    j = R.judge(Q, vectors, got)
    print("end to end: undecided share %.4f of %d positions, mismatches %d, worst regret / gate %.3g" %
          (j["undecided_share"], Q.shape[0], int((got != j["best"]).sum()), j["regret_ratio"]))
    assert j["undecided_share"] <= 0.05 and j["wrong_decided"] == 0 and j["regret_ratio"] <= 1.0
    cut = vae.text_decoder.generate(z, stop_at_eos=True)
    for full, short in zip(sentences, cut):
        ws = full.split(' ')
        assert short == ' '.join(ws[:ws.index('</s>')] if '</s>' in ws else ws)


def test_sample_coco_command_writes_captions(tmp_path):
    from multimodal_vae_amd import evaluate as E
    vae, _, _ = small_model()
    ck = str(tmp_path / "checkpoint.pth.tar")
    torch.save({"state_dict": vae.state_dict(), "n_latents": 20}, ck)
    out = str(tmp_path / "results")
    E._main(["sample_coco", ck, "--synthetic_words", "5000", "--n_samples", "4", "--out", out])
    lines = open(os.path.join(out, "sample_text.txt")).read().splitlines()
    assert len(lines) == 4 and all(len(l.split(' ')) == 102 for l in lines)
    assert tuple(torch.load(os.path.join(out, "sample_image.pt")).shape) == (4, 3, 32, 32)
    E._main(["sample_coco", ck, "--synthetic_words", "5000", "--n_samples", "2", "--out", out,
             "--condition_on_text", "w1 w2 w3 not-a-word"])
    assert len(open(os.path.join(out, "sample_text.txt")).read().splitlines()) == 2
