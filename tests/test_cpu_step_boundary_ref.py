"""CPU checks of tests/step_boundary_ref.py: Philox4x32-10 reproduces the published known-answer vectors, the Adam reference is
torch.optim.Adam on float64 tensors, the float32 emulation passes every gate the GPU test uses at every case the GPU test uses, and
every entry of FAULTS fails one of them at those cases."""
import numpy as np
import pytest
import torch

import step_boundary_ref as S


# ---------------------------------------------------------------------------------------------- Philox
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    assert " ".join("%08x" % int(w[0]) for w in S.philox4x32_10(ctr, key)) == want
    # vectorised: the same counter among others gives the same words
    c0 = np.array([1, ctr[0], 2], dtype=np.uint64)
    got = S.philox4x32_10((c0, ctr[1], ctr[2], ctr[3]), key)
    assert " ".join("%08x" % int(w[1]) for w in got) == want


def test_u01_edges_and_the_pinned_tie():
    """u01 in fp32: the largest word rounds to exactly 1.0, the smallest is 2^-25 (never 0: the logarithm is finite); the pinned tie
    case holds a draw equal to p, and only there ">" and ">=" differ"""
    u = S.u01(np.array([0, 0xFF, 0x100, 0x80000000, 0xFFFFFFFF], dtype=np.uint64))
    assert u.dtype == np.float32 and list(u) == [2.0 ** -25, 2.0 ** -25, 1.5 * 2.0 ** -24, 0.5, 1.0]
    T = S.TIE
    assert list(S.find_tie(T["seed"], T["step"], T["stream"], T["n"], T["p"])) == [T["index"]]
    a = S.keep_mask(T["seed"], T["step"], T["stream"], T["n"], T["p"])
    b = S.keep_mask(T["seed"], T["step"], T["stream"], T["n"], T["p"], "gt_for_ge")
    assert list(np.nonzero(a != b)[0]) == [T["index"]] and a[T["index"]] == 1
    for n, seed, step, stream in S.draw_cases():               # none of the ordinary cases has a tie: their masks do not see the fault
        if n <= 1023:
            assert all(len(S.find_tie(seed, step, stream, n, p)) == 0 for p in S.MASK_P[1:3])


def test_draw_cases_cover_what_they_claim():
    cases = S.draw_cases()
    assert {c[0] for c in cases} == set(S.DRAW_N)
    for n in S.DRAW_N:
        mine = [c for c in cases if c[0] == n]
        assert {c[1] for c in mine} == set(S.DRAW_SEEDS) and {c[2] for c in mine} == set(S.DRAW_STEPS) and {c[3] for c in mine} == set(S.DRAW_STREAMS)
    # a null step pointer is step 0; the streams, the steps and the seed's halves all reach the words
    w = lambda *a: S.draw_words(*a, 8)
    assert np.array_equal(w(5, None, 1), w(5, 0, 1))
    distinct = [w(5, 0, 1), w(5, 0, 2), w(5, 1, 1), w(5 + 2 ** 32, 0, 1), w(5, 2 ** 33 + 5, 1), w(5, 5, 1)]
    assert all(not np.array_equal(a, b) for i, a in enumerate(distinct) for b in distinct[:i])


# ---------------------------------------------------------------------------------------------- Adam reference == torch.optim.Adam
@pytest.mark.parametrize("hyper", S.HYPER)
@pytest.mark.parametrize("scale", S.SCALES)
def test_adam_reference_is_torch_optim_adam(hyper, scale):
    """three steps from zero moments, float64, the hyper-parameters as the fp32 values the kernel receives (rtol 1e-12)"""
    n = 257
    L = S.adam_inputs(n, hyper, 0, scale)
    L = L._replace(m=np.zeros_like(L.m), v=np.zeros_like(L.v))               # torch's state starts at zero (no m != 0, v = 0 block)
    lr, b1, b2, eps, s = (float(x) for x in S.f32_hyper(hyper, scale))
    p = torch.from_numpy(L.p.astype(np.float64)).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    rng = np.random.default_rng(5)
    for step in range(3):
        g = (L.g * rng.uniform(0.5, 2.0, n)).astype(np.float32)
        L = L._replace(g=g)
        r = S.adam_launch(L, np.float64)
        p.grad = torch.from_numpy(g.astype(np.float64) * s)
        opt.step()
        st = opt.state[p]
        # rtol 1e-12 of each value; of |p_old| + |dp| for the parameter, which is a difference that may cancel
        p_mag = torch.from_numpy(np.abs(L.p.astype(np.float64))) + (torch.from_numpy(L.p.astype(np.float64)) - p.detach()).abs()
        for name, got, want, mag in (("p", r["p"], p.detach(), p_mag), ("m", r["m"], st["exp_avg"], st["exp_avg"].abs()),
                                     ("v", r["v"], st["exp_avg_sq"], st["exp_avg_sq"])):
            assert bool(((torch.from_numpy(got) - want).abs() <= 1e-12 * mag).all()), (name, step, hyper)
        assert r["counter"] == step + 1 == int(st["step"])
        # carried in float64: the next step starts from the unrounded state (p, m, v are Launch fields of any float dtype)
        L = L._replace(p=r["p"], m=r["m"], v=r["v"], counter=r["counter"])


# ---------------------------------------------------------------------------------------------- the emulation passes, the faults do not
def _adam_launches():
    """every launch the GPU module makes, as (tag, Launch)"""
    for n, hyper, counter, scale in S.adam_cases():
        yield "whole n=%d" % n, S.adam_inputs(n, hyper, counter, scale)
    for L in S.range_launches():
        yield "ranges %s advance=%d" % (L.ranges, L.advance), L
    yield "packed", S.packed_base(S.HYPER[1], 1, 1.0 / 3.0)
    for name, L in S.void_launches():
        yield "void " + name, L
    first = S.packed_base()._replace(ranges=S.PARTITION[0], advance=0)
    yield "partition 1", first
    yield "partition 2", S.carry(first, S.emulate_adam(first), ranges=S.PARTITION[1], advance=1)


def _read(out, L):
    """an emulation's result in the form the GPU test reads a launch back"""
    got = {k: np.asarray(out[k], dtype=np.float32) for k in ("p", "m", "v")}
    got.update(counter=out["counter"], skip=out["skip"])
    if L.gmap is not None:
        got["g_out"] = out["g_out"]
    return got


def test_fault_free_adam_emulation_passes_every_gate():
    worst = {}
    for tag, L in _adam_launches():
        recs = S.gate_adam(_read(S.emulate_adam(L), L), L)
        assert not S.violations(recs), (tag, S.violations(recs))
        for r in recs:
            worst[r.name] = max(worst.get(r.name, 0.0), r.err / r.gate if r.gate else r.err)
    print("adam emulation, worst error / gate:", {k: "%.2f" % v for k, v in worst.items()})


@pytest.mark.parametrize("fault", S.ADAM_FAULTS)
def test_every_adam_fault_is_caught(fault):
    caught = [tag for tag, L in _adam_launches() if S.violations(S.gate_adam(_read(S.emulate_adam(L, fault), L), L))]
    print(fault, "caught at", len(caught), "launches, first:", caught[:2])
    assert caught, fault


def test_partition_equals_one_whole_launch():
    """two launches whose ranges partition [0, n) (advance 0, then 1) leave what one whole launch leaves, and count one step"""
    base = S.packed_base()
    whole = S.emulate_adam(base)
    first = base._replace(ranges=S.PARTITION[0], advance=0)
    a = S.emulate_adam(first)
    b = S.emulate_adam(S.carry(first, a, ranges=S.PARTITION[1], advance=1))
    assert a["counter"] == 2 and b["counter"] == 3 == whole["counter"]
    assert all(np.array_equal(b[k], whole[k]) for k in ("p", "m", "v", "g_out"))
    cover = np.zeros(S.RANGE_N, dtype=int)
    for o, l in S.PARTITION[0] + S.PARTITION[1]:
        cover[o:o + l] += 1
    assert (cover == 1).all()


def _draw_gates(fault=None):
    """(tag, violations) of every draw check the GPU module makes, on the emulation"""
    for n, seed, step, stream in S.draw_cases():
        tag = "n=%d seed=%#x step=%s stream=%#x" % (n, seed, step, stream)
        yield "normal " + tag, S.violations(S.gate_normals(S.emulate_normals(seed, step, stream, n, fault), seed, step, stream, n))
        for p in S.MASK_P:
            yield "mask p=%g " % p + tag, S.violations(S.gate_mask(S.emulate_mask(seed, step, stream, n, p, fault), seed, step, stream, n, p))
    T = S.TIE
    yield "mask tie", S.violations(S.gate_mask(S.emulate_mask(T["seed"], T["step"], T["stream"], T["n"], T["p"], fault), T["seed"],
                                               T["step"], T["stream"], T["n"], T["p"]))


def test_fault_free_draw_emulation_passes_every_gate():
    bad = [(tag, v) for tag, v in _draw_gates() if v]
    assert not bad, bad[:3]


@pytest.mark.parametrize("fault", S.DRAW_FAULTS)
def test_every_draw_fault_is_caught(fault):
    caught = [tag for tag, v in _draw_gates(fault) if v]
    print(fault, "caught at", len(caught), "checks, first:", caught[:2])
    assert caught, fault


def test_fault_list_is_the_issue_s():
    assert len(S.FAULTS) == 15 == len(set(S.FAULTS))
