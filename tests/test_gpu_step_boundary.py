"""GPU tests of the kernels at the step boundary (csrc/elementwise.hip): the optimizer (adam_kernel through mmvae_adam_step, _packed and
_packed_ranges), the Philox draws (mmvae_normal, mmvae_keep_mask and the prologue of a real MultiMNIST step), every family's gradient
map against the pack it inverts and against the family's own unpack, and the exact feed kernels (mmvae_gather_rows, _u8_f32,
mmvae_u8_to_f32) -- against the references of tests/step_boundary_ref.py, whose gate functions these tests call
(tests/test_cpu_step_boundary_ref.py proves on the CPU that every gate notices every entry of FAULTS).

Gates (elementwise_ref.py): fp32 elements err / magnitude <= max(4 err32, 2^-22 = 2.38e-7), err32 the same figure of the float32 CPU
evaluation; everything else exact.  Every output is filled with 7.0, NaN or a mark before the call and has guard elements; every test
prints what it measured (run with -s; MMVAE_TOL_REPORT=1 adds the worst error / gate ratio of every record).

Measured on an MI355X, worst error / gate over all cases (error / gate in brackets): Adam m 0.25 (6.2e-8 / 2.5e-7), v 0.28 (1.4e-7 /
4.9e-7), dp 0.68 (1.6e-7 / 2.4e-7), dp past the parameter's rounding 0.59 (1.4e-7 / 2.4e-7), the same under adam_blocks 1, 2 and the
default; the range launches dp 0.27 (3.4e-6 / 1.2e-5: t = 3 with b2 = 0.999, where 1 - b2^t cancels in fp32 for kernel and baseline
alike).  Normal draws 0.48 (1.17e-7 of the radius against 4 err32 = 2.42e-7).  Masks, the step prologue, the gradient maps, the feed
kernels and every "untouched" comparison: exact.  Wall time of the module: 5.7 s (32 tests, the slowest 0.5 s).

What these tests found:
  * No arithmetic defect.  logf / sqrtf / cosf / sinf of draw_normals under -ffp-contract=fast stay at 0.48 of the gate (the expf
    artefact of tests/test_gpu_elementwise.py has no counterpart here): the bits of a draw did not change.  adam_kernel agrees with
    the float32 baseline to within its own roundings at every size, cap, counter and scale.
  * launch_adam took null p / g / m / v and n < 1 straight to a kernel that reads g[0]; launch_normal and launch_keep_mask checked
    nothing.  Now MMVAE_REQUIREs with a message (n = 0 for the two generators is OK and launches nothing; p outside [0, 1] or NaN is
    refused): test_launchers_refuse_null_and_empty.
  * The weight pack and the gradient map do not share a descriptor table (the gradient table has its own row pads and offsets and one
    copy per weight), so "pack_weights, then packed[gmap[i]] == params[i]" cannot hold.  The inverse is checked where it can: pack_block
    run over the GRADIENT table (mmvae_<family>_debug_pack_as_grads, a test aid) against unpack_kernel<true>'s map.  It holds for every
    family, and the pack writes nothing outside the map but zero pads.
  * No plan has an fp32 gradient pack (is_f32) any more: gpk_vec entries ("< -1") occur in no real map, the optimizer's branch for
    them is reached by the synthetic map only.  The MNIST fp32 plan writes its gradients straight into grads; its map points into a gpk
    that its step never fills (exactly 0, asserted), so a packed optimizer launch on it would add zeros -- harmless, and pinned.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import step_boundary_ref as S
from oracle import mmvae_ref as R

pytestmark = pytest.mark.gpu
REPORT = os.environ.get("MMVAE_TOL_REPORT") is not None
LEAD = 4                                          # guard elements in front of a buffer (16 bytes: the vectors stay aligned), S.GUARD behind


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _api():
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd._ops import stream
    return call, ptr, stream


class _Worst:
    """the worst error / gate per record name over a test's cases"""

    def __init__(self):
        self.w = {}

    def add(self, tag, recs):
        bad = S.violations(recs)
        assert not bad, (tag, bad, S.describe(recs))
        for r in recs:
            q = r.err / r.gate if r.gate else r.err
            if r.name not in self.w or q > self.w[r.name][0]:
                self.w[r.name] = (q, r.err, r.gate, tag)

    def show(self, title):
        exact = [name for name, w in self.w.items() if not w[2]]
        for name, (q, err, gate, tag) in self.w.items():
            if gate:
                print("%s: %s worst error / gate %.3f (%.3e / %.3e)%s" % (title, name, q, err, gate, " at " + tag if REPORT else ""))
        print("%s: exact in every case: %s" % (title, ", ".join(n.replace(" exact", "") for n in exact)))


def _guarded(dev, a, fill=7.0, dtype=None):
    """-> (buffer [LEAD + n + GUARD] on the device holding ``a`` between guards of ``fill``, pointer to element 0 of ``a``)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.full((LEAD + t.numel() + S.GUARD,), fill, dtype=t.dtype if dtype is None else dtype, device=dev)
    buf[LEAD:LEAD + t.numel()] = t.to(dev)
    return buf, ctypes.c_void_p(buf.data_ptr() + LEAD * buf.element_size())


def _guards_intact(buf, n, fill=7.0):
    g = torch.cat((buf[:LEAD], buf[LEAD + n:])).cpu()
    return S.rec_exact("guards", g, torch.full_like(g, fill))


# ====================================================================================================== the optimizer
def _adam_launch(dev, L, blocks=None):
    """one launch on ``L`` through the entry point its fields ask for -> what gate_adam takes (and the guard record)"""
    from multimodal_vae_amd._lib import knobs
    call, ptr, stream = _api()
    n = L.p.shape[0]
    bufs = {k: _guarded(dev, getattr(L, k)) for k in ("p", "g", "m", "v")}
    state = torch.tensor([L.counter, L.skip << 32], dtype=torch.int64, device=dev)
    lr, b1, b2, eps = (float(x) for x in L.hyper)
    hyper = (ptr(state), lr, b1, b2, eps, float(L.scale))
    head = tuple(bufs[k][1] for k in ("p", "g", "m", "v")) + (n,)
    if L.gmap is not None:
        gm, pk, vec = (torch.from_numpy(x).to(dev) for x in (L.gmap, L.gpk, L.gpk_vec))
        packed = (ptr(gm), ptr(pk), ptr(vec))
    if L.gmap is None:
        assert L.ranges is None and L.advance == 1
        name, args = "mmvae_adam_step", head + hyper
    elif L.ranges is None:
        assert L.advance == 1
        name, args = "mmvae_adam_step_packed", head + hyper + packed
    else:
        flat = [x for r in L.ranges for x in r]
        name, args = "mmvae_adam_step_packed_ranges", head + ((ctypes.c_longlong * len(flat))(*flat), len(L.ranges), int(L.advance)) + hyper + packed
    with knobs(**({} if blocks is None else {"adam_blocks": blocks})):
        call(name, *args, stream())
    torch.cuda.synchronize()
    got = {k: bufs[k][0][LEAD:LEAD + n].cpu().numpy() for k in ("p", "m", "v")}
    got.update(counter=int(state[0]), skip=int(state[1]))
    if L.gmap is not None:
        got["g_out"] = bufs["g"][0][LEAD:LEAD + n].cpu().numpy()
    else:
        assert np.array_equal(bufs["g"][0][LEAD:LEAD + n].cpu().numpy().view(np.uint32), L.g.view(np.uint32))      # read-only
    guards = [_guards_intact(bufs[k][0], n) for k in ("p", "g", "m", "v")]
    return got, guards


@pytest.mark.parametrize("blocks", S.ADAM_BLOCKS)
def test_adam_every_element(blocks):
    """mmvae_adam_step against float64 torch.optim.Adam arithmetic, element by element: n = 1 .. 4101 (one block covers 1024 elements
    per pass: the grid-stride loop, uneven shares and the scalar tail under a cap of 1 and 2 blocks), three hyper-parameter sets (one
    with b1 = 0), the counter preset to 0, 1, 2, 999, 99999 with consistent moments, grad_scale 1, 0.125, 1/3, gradients from 1e-9 to 10
    with exact zeros and a block with m != 0, v = 0."""
    dev = _dev()
    worst = _Worst()
    for n, hyper, counter, scale in S.adam_cases():
        L = S.adam_inputs(n, hyper, counter, scale)
        got, guards = _adam_launch(dev, L, blocks)
        worst.add("n=%d hyper=%s counter=%d scale=%g" % (n, hyper, counter, scale), S.gate_adam(got, L) + guards)
    worst.show("adam (adam_blocks=%s)" % blocks)


@pytest.mark.parametrize("blocks", (1, None))
def test_adam_ranges_and_no_advance(blocks):
    """mmvae_adam_step_packed_ranges on 4101 elements filled from marks: one range, an empty range, a range that ends in the tail at n,
    four ranges with an empty one, each with advance = 1 and 0; everything outside the ranges bit-equal to what it held, the written
    back gradient exact (a synthetic map with all three kinds of entry)"""
    dev = _dev()
    worst = _Worst()
    for L in S.range_launches():
        got, guards = _adam_launch(dev, L, blocks)
        worst.add("ranges=%s advance=%d" % (L.ranges, L.advance), S.gate_adam(got, L) + guards)
    worst.show("adam ranges (adam_blocks=%s)" % blocks)


def test_adam_partition_is_one_whole_launch():
    """two launches whose ranges partition [0, n) (advance 0, then 1) == one whole launch, bit for bit, and count one step"""
    dev = _dev()
    base = S.packed_base()
    whole, _ = _adam_launch(dev, base)
    first = base._replace(ranges=S.PARTITION[0], advance=0)
    a, _ = _adam_launch(dev, first)
    assert a["counter"] == base.counter
    b, _ = _adam_launch(dev, S.carry(first, a, ranges=S.PARTITION[1], advance=1))
    assert b["counter"] == whole["counter"] == base.counter + 1 and b["skip"] == 0
    for k in ("p", "m", "v", "g_out"):
        assert np.array_equal(b[k].view(np.uint32), whole[k].view(np.uint32)), k


def test_adam_packed_gradient():
    """mmvae_adam_step_packed with a synthetic map (entries >= 0, -1 and < -1, a 4-vector that mixes them, the scalar tail): the
    written-back gradient is g + gpk[...] / gpk_vec[...] as one fp32 add, and p, m, v are bit-equal to mmvae_adam_step on it"""
    dev = _dev()
    L = S.packed_base(S.HYPER[1], 1, 1.0 / 3.0)
    assert (L.gmap >= 0).any() and (L.gmap == -1).any() and (L.gmap < -1).any() and len({int(np.sign(x + 1)) for x in L.gmap[:4]}) == 3
    got, guards = _adam_launch(dev, L)
    recs = S.gate_adam(got, L) + guards
    assert not S.violations(recs), S.violations(recs)
    full = L.g.copy()
    pk, vec = L.gmap >= 0, L.gmap < -1
    full[pk] += L.gpk[L.gmap[pk]]
    full[vec] += L.gpk_vec[-L.gmap[vec] - 2]
    assert torch.equal(torch.from_numpy(got["g_out"]), torch.from_numpy(full))
    plain, _ = _adam_launch(dev, L._replace(g=full, gmap=None, gpk=None, gpk_vec=None))
    for k in ("p", "m", "v"):
        assert np.array_equal(plain[k].view(np.uint32), got[k].view(np.uint32)), k
    print("adam packed: %s" % S.describe(recs))


def test_adam_void_step_and_nan_gradient():
    """The void mark in g[0] (either sign) and the skip word leave p, m, v and the counter untouched and state[1] == 0; the next ordinary
    launch behaves as if nothing had happened.  A quiet NaN of any other payload (and the mark's own bits anywhere but in g[0]) is a
    gradient: exactly that element of p, m, v becomes NaN and the counter advances."""
    dev = _dev()
    for name, L in S.void_launches():
        got, guards = _adam_launch(dev, L)
        recs = S.gate_adam(got, L) + guards
        assert not S.violations(recs), (name, S.violations(recs))
        if name.startswith(("mark", "skip")):
            assert got["counter"] == L.counter and got["skip"] == 0
            for k in ("p", "m", "v"):
                assert np.array_equal(got[k].view(np.uint32), getattr(L, k).view(np.uint32)), (name, k)
            nxt = S.carry(L, got, g=S.adam_inputs(L.p.shape[0], L.hyper, L.counter, L.scale).g)     # the same step, an ordinary gradient
            got2, guards2 = _adam_launch(dev, nxt)
            recs2 = S.gate_adam(got2, nxt) + guards2
            assert not S.violations(recs2) and got2["counter"] == L.counter + 1, (name, S.violations(recs2))
        else:
            assert got["counter"] == L.counter + 1
            for k in ("p", "m", "v"):
                assert list(np.nonzero(np.isnan(got[k]))[0]) == [5], (name, k)
        print("adam %s: %s" % (name, S.describe(recs)))


def test_launchers_refuse_null_and_empty():
    """launch_adam, launch_normal and launch_keep_mask return an error with a message before anything is launched: null buffers, n < 1
    (Adam reads g[0]) / n < 0 (the generators; n = 0 is OK and launches nothing), p outside [0, 1] or NaN"""
    from multimodal_vae_amd._lib import MMVAEError
    call, ptr, stream = _api()
    dev = _dev()
    t = torch.full((64,), 7.0, device=dev)
    st = torch.zeros(2, dtype=torch.int64, device=dev)
    gm = torch.full((64,), -1, dtype=torch.int32, device=dev)
    rng = (ctypes.c_longlong * 2)(0, 8)
    p, s, h = ptr(t), ptr(st), (1e-3, 0.9, 0.999, 1e-8, 1.0)
    bad = [("mmvae_adam_step", (a, b, c, d, n, e) + h + (stream(),)) for a, b, c, d, n, e in
           ((None, p, p, p, 8, s), (p, None, p, p, 8, s), (p, p, None, p, 8, s), (p, p, p, None, 8, s), (p, p, p, p, 8, None),
            (p, p, p, p, 0, s), (p, p, p, p, -4, s))]
    bad += [("mmvae_adam_step_packed", (p, p, p, p, 0, s) + h + (ptr(gm), p, p, stream())),
            ("mmvae_adam_step_packed", (p, None, p, p, 8, s) + h + (ptr(gm), p, p, stream())),
            ("mmvae_adam_step_packed", (p, p, p, p, 8, s) + h + (None, p, p, stream())),
            ("mmvae_adam_step_packed_ranges", (None, p, p, p, 8, rng, 1, 1, s) + h + (ptr(gm), p, p, stream())),
            ("mmvae_adam_step_packed_ranges", (p, p, p, p, 4, rng, 1, 1, s) + h + (ptr(gm), p, p, stream())),          # range past n
            ("mmvae_normal", (None, 8, 1, None, 1, stream())), ("mmvae_normal", (p, -1, 1, None, 1, stream())),
            ("mmvae_keep_mask", (None, 8, 0.1, 1, None, 1, stream())), ("mmvae_keep_mask", (p, -1, 0.1, 1, None, 1, stream()))]
    bad += [("mmvae_keep_mask", (p, 8, q, 1, None, 1, stream())) for q in (-0.1, 1.5, float("nan"), float("inf"))]
    for name, args in bad:
        with pytest.raises(MMVAEError) as e:
            call(name, *args)
        assert len(str(e.value)) > 10, name
    call("mmvae_normal", p, 0, 1, None, 1, stream())
    call("mmvae_keep_mask", p, 0, 0.1, 1, None, 1, stream())
    torch.cuda.synchronize()
    assert float(t.min()) == 7.0 == float(t.max()) and int(st.abs().max()) == 0 and int(gm.max()) == -1


# ====================================================================================================== the draws
def _normal(dev, n, seed, step, stream_id):
    call, ptr, stream = _api()
    out = torch.full((n + S.GUARD,), float("nan"), device=dev)
    ctr = None if step is None else torch.tensor([step, 0], dtype=torch.int64, device=dev)
    call("mmvae_normal", ptr(out), n, ctypes.c_ulonglong(seed), ptr(ctr), stream_id, stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[n:]).all()) and (ctr is None or (int(ctr[0]), int(ctr[1])) == (step, 0))
    return out[:n].cpu()


def _mask(dev, n, p, seed, step, stream_id):
    call, ptr, stream = _api()
    out = torch.full((n + S.GUARD,), 7, dtype=torch.uint8, device=dev)
    ctr = None if step is None else torch.tensor([step, 0], dtype=torch.int64, device=dev)
    call("mmvae_keep_mask", ptr(out), n, p, ctypes.c_ulonglong(seed), ptr(ctr), stream_id, stream())
    torch.cuda.synchronize()
    assert bool((out[n:] == 7).all())
    return out[:n].cpu()


def test_normals_against_the_definition():
    """mmvae_normal, every element against float64 Box-Muller on the Philox words of the definition: n = 1 .. 524293 (the last one
    grid-strides), seeds with and without high bits, a null step pointer and counters 0, 1, 2^33 + 5, streams 1 .. 5 and 0xffffffff;
    an element depends on (key, stream, index) only: n = 5 is the prefix of n = 1023, bit for bit"""
    dev = _dev()
    worst = _Worst()
    runs = {}
    for n, seed, step, sid in S.draw_cases():
        got = _normal(dev, n, seed, step, sid)
        runs[(n, seed, step, sid)] = got
        worst.add("n=%d seed=%#x step=%s stream=%#x" % (n, seed, step, sid), S.gate_normals(got, seed, step, sid, n))
    pre = 0
    for (n, seed, step, sid), got in runs.items():
        if n == 5:
            assert torch.equal(got.view(torch.int32), runs[(1023, seed, step, sid)][:5].view(torch.int32))
            pre += 1
    assert pre == len(S.DRAW_SEEDS) * len(S.DRAW_STEPS) * len(S.DRAW_STREAMS)
    worst.show("normal")


def test_masks_are_the_definition_s_bytes():
    """mmvae_keep_mask == (u01 >= p) of the definition's words, byte for byte, at the cases of the normals, p = 0, 0.1, 0.5, 1.0 -- and at
    the pinned case where one draw EQUALS p (">" for ">=" flips exactly that byte)"""
    dev = _dev()
    ones = 0
    for n, seed, step, sid in S.draw_cases():
        for p in S.MASK_P:
            got = _mask(dev, n, p, seed, step, sid)
            bad = S.violations(S.gate_mask(got, seed, step, sid, n, p))
            assert not bad, (n, seed, step, sid, p, bad)
            ones += int(got.sum())
    T = S.TIE
    got = _mask(dev, T["n"], T["p"], T["seed"], T["step"], T["stream"])
    assert not S.violations(S.gate_mask(got, T["seed"], T["step"], T["stream"], T["n"], T["p"])) and int(got[T["index"]]) == 1
    print("keep masks: every byte equal (%d ones); the tie at element %d is kept" % (ones, T["index"]))


@pytest.mark.parametrize("counter", [0, 1])
def test_step_prologue_is_the_standalone_generators(counter):
    """the draws of a real MultiMNIST fused step (B = 8, nothing injected), read back from the workspace: eps is mmvae_normal on stream 1,
    the three keep masks are mmvae_keep_mask on streams 2, 3, 4 at the step's p = 0.1, for the step's seed and counter, bit for bit --
    with the two tests above, the timed path is tied to the definition"""
    from multimodal_vae_amd.core import FusedELBOStep, MultimnistState
    from multimodal_vae_amd.init import default_init_
    from multimodal_vae_amd._lib import call
    dev = _dev()
    B, D, seed = 8, 100, 0x5EED00000000 + 1234
    st = MultimnistState(D, dev); default_init_(st, 3)
    image, text = R.formula_inputs("multimnist", B)
    eng = FusedELBOStep(st, B, seed=seed)
    eng.adam_state[0] = counter
    eng.forward_backward(image.to(dev), text.to(dev), True, False)
    torch.cuda.synchronize()
    for name, n, sid in (("eps", 3 * B * D, 1), ("m1", 2 * B * 400, 2), ("m2", 2 * B * 200, 3), ("gkeep", 4 * 3 * B * 100, 4)):
        off = call("mmvae_mm_debug_offset", eng.h, name.encode())
        assert off >= 0
        if name == "eps":
            got, want = eng.ws[off:off + 4 * n].view(torch.int32).cpu(), _normal(dev, n, seed, counter, sid).view(torch.int32)
            assert not S.violations(S.gate_normals(eng.ws[off:off + 4 * n].view(torch.float32).cpu(), seed, counter, sid, n))
        else:
            got, want = eng.ws[off:off + n].cpu(), _mask(dev, n, 0.1, seed, counter, sid)
            assert not S.violations(S.gate_mask(got, seed, counter, sid, n, 0.1))
        assert torch.equal(got, want), name
    assert int(eng.adam_state[0]) == counter


# ====================================================================================================== the gradient map
FAMILIES = ("mm20", "mm100", "celeba", "coco", "mmtext", "mnist_fp32", "mnist_bf16")


def _family(name, dev, B=8):
    """-> (state, engine, the step's inputs on the device)"""
    from multimodal_vae_amd import core
    from multimodal_vae_amd.init import default_init_
    if name in ("mm20", "mm100"):
        st = core.MultimnistState(int(name[2:]), dev)
        eng, (a, b) = core.FusedELBOStep(st, B, seed=3), R.formula_inputs("multimnist", B)
    elif name == "celeba":
        st = core.CelebaState(100, dev)
        eng, (a, b) = core.FusedCelebaStep(st, B, seed=3), R.formula_inputs("celeba", B)
    elif name == "coco":
        st = core.CocoState(100, dev, 8)
        eng, (a, b) = core.FusedCocoStep(st, B, R.formula_sos(), seed=3), R.formula_inputs("coco", B)
        b = b[:, :8]
    elif name == "mmtext":
        st = core.MultimnistTextState(100, dev, 50)
        eng, a, b = core.FusedMMTextStep(st, B, seed=3), None, R.formula_inputs("multimnist", B)[1]
    else:
        st = core.MnistState(20, dev, precision=name[6:])
        eng, (a, b) = core.FusedMnistStep(st, B, seed=3), R.formula_inputs("mnist", B)
        a = a.reshape(B, 784)
    default_init_(st, 5)
    st.pack_weights()
    return st, eng, tuple(x.to(dev).contiguous() for x in (a, b) if x is not None)


def _gdesc(st):
    from test_gpu_pack_runs import DESC
    return np.frombuffer(st._desc[1].cpu().numpy().tobytes(), dtype=DESC)


@pytest.mark.parametrize("family", FAMILIES)
def test_grad_map_structure_and_inverse_of_the_pack(family):
    """mmvae_<family>_grad_map.  Structure: every value >= 0 occurs once and lies inside gpk, every value < -1 decodes to a distinct
    index inside gpk_vec, and the number of mapped parameters is what the gradient descriptor table covers (N K plus its folded
    biases).  Inverse of the pack: pack_block run over the gradient descriptor table (mmvae_<family>_debug_pack_as_grads -- the weight
    pack itself has another table: other row pads, other offsets, more copies) puts parameter i where the map, built by
    unpack_kernel<true>, says its gradient lives -- bf16-representable random values, two independent seeds; and it puts nothing else
    anywhere (every other packed element is a zero pad)."""
    call, ptr, stream = _api()
    dev = _dev()
    st, _, _ = _family(family, dev)
    gmap = st.grad_map().cpu().long()
    mat, vec = gmap[gmap >= 0], -gmap[gmap < -1] - 2
    assert mat.numel() > 0 and mat.unique().numel() == mat.numel() and int(mat.max()) < st.gpk.numel()
    assert vec.unique().numel() == vec.numel() and (vec.numel() == 0 or int(vec.max()) < st.gpk_vec.numel())
    d = _gdesc(st)
    covered = int((d["N"].astype(np.int64) * (d["K"] + (d["bias_off"] >= 0))).sum())
    assert mat.numel() + vec.numel() == covered, (mat.numel(), vec.numel(), covered)
    f32_rows = int((d["N"].astype(np.int64) * (d["K"] + (d["bias_off"] >= 0)) * (d["is_f32"] != 0)).sum())
    assert vec.numel() == f32_rows
    # (no plan of the library has an fp32 gradient pack today -- vec is empty everywhere, the MNIST fp32 plan included: the map's and the
    # optimizer's "< -1" branch is reached through the synthetic map of test_adam_packed_gradient only)
    for seed in (11, 12):
        g = torch.Generator().manual_seed(seed)
        vals = torch.randn(st.nparams, generator=g).to(torch.bfloat16).float()
        vals[vals == 0] = 1.0
        out_bf = torch.full((st.gpk.numel() + S.GUARD,), 7.0, dtype=torch.bfloat16, device=dev)
        out_vec = torch.full((st.gpk_vec.numel() + S.GUARD,), 7.0, device=dev)
        vd = vals.to(dev)
        call("mmvae_%s_debug_pack_as_grads" % st.API, st.plan(1), ptr(vd), ptr(out_bf), ptr(out_vec), stream())
        torch.cuda.synchronize()
        assert float(out_bf[st.gpk.numel():].float().min()) == 7.0 == float(out_bf[st.gpk.numel():].float().max())
        assert float(out_vec[st.gpk_vec.numel():].min()) == 7.0 == float(out_vec[st.gpk_vec.numel():].max())
        pb, pv = out_bf[:st.gpk.numel()].float().cpu(), out_vec[:st.gpk_vec.numel()].cpu()
        assert torch.equal(pb[mat], vals[gmap >= 0]), (family, seed)
        assert torch.equal(pv[vec], vals[gmap < -1]), (family, seed)
        # nothing else: the places the pack wrote a parameter to are exactly the map's (the table's own extent; behind it the fill stays)
        assert int(((pb != 0) & (pb != 7.0)).sum()) == mat.numel() and int(((pv != 0) & (pv != 7.0)).sum()) == vec.numel()
    print("%s: %d parameters, %d through gpk, %d through gpk_vec, %d direct" % (family, st.nparams, mat.numel(), vec.numel(), int((gmap == -1).sum())))


@pytest.mark.parametrize("family", FAMILIES)
def test_grad_map_gather_equals_the_family_s_unpack(family):
    """One real step (B = 8, the family's default: its own unpack completes ``grads``), then the packed gradients it left in gpk /
    gpk_vec gathered through the map by mmvae_adam_step_packed into a gradient whose mapped entries were zeroed: the written-back
    gradient equals the step's under torch.equal, and p, m, v are bit-equal to mmvae_adam_step on the step's gradient.
    The MNIST fp32 plan is the exception the test pins down: its step writes every gradient straight into ``grads`` and never fills
    gpk (which stays exactly 0), so the packed optimizer on its map adds zeros: the complete gradient goes in and comes out unchanged."""
    call, ptr, stream = _api()
    dev = _dev()
    st, eng, inputs = _family(family, dev)
    eng.forward_backward(*inputs, True, True)
    torch.cuda.synchronize()
    gmap = st.grad_map()
    mapped = gmap != -1
    full = st.grads.clone()
    assert bool(torch.isfinite(full).all()) and float((full[mapped] != 0).float().mean()) > 0.5
    direct = family == "mnist_fp32"
    assert (float(st.gpk.abs().max()) == 0.0) == direct and float(st.gpk_vec.abs().max()) == 0.0
    n = st.nparams
    g = torch.Generator().manual_seed(2)
    m0, v0 = (0.01 * torch.randn(n, generator=g)).to(dev), (1e-4 * torch.rand(n, generator=g)).to(dev)
    res = []
    for packed in (False, True):
        grad = full.clone()
        if packed and not direct:
            grad[mapped] = 0.0
        p, m, v = st.params.clone(), m0.clone(), v0.clone()
        state = torch.tensor([4, 0], dtype=torch.int64, device=dev)
        args = (ptr(p), ptr(grad), ptr(m), ptr(v), n, ptr(state), 1e-3, 0.9, 0.999, 1e-8, 0.5)
        if packed:
            call("mmvae_adam_step_packed", *args, ptr(gmap), ptr(st.gpk), ptr(st.gpk_vec), stream())
        else:
            call("mmvae_adam_step", *args, stream())
        torch.cuda.synchronize()
        assert (int(state[0]), int(state[1])) == (5, 0)
        res.append((grad, p, m, v))
    assert torch.equal(res[1][0], full), family
    for a, b in zip(res[0][1:], res[1][1:]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), family
    print("%s: %d of %d gradient elements gathered through the map equal the step's own unpack" % (family, int(mapped.sum()), n))


def test_mnist_infovae_keeps_no_map():
    from multimodal_vae_amd import core
    from multimodal_vae_amd._lib import MMVAEError
    with pytest.raises(MMVAEError):
        core.MnistInfoVAEState(20, _dev()).grad_map()


# ====================================================================================================== the feed kernels
def _indices(rows, n_src):
    """repeated, reversed and out-of-order source rows"""
    g = torch.Generator().manual_seed(rows)
    idx = torch.randint(0, n_src, (rows,), generator=g)
    if rows >= 3:
        idx[0], idx[1], idx[2] = n_src - 1, n_src - 1, 0
    if rows >= 300:
        idx[100:200] = torch.arange(n_src - 1, n_src - 101, -1) % n_src
    return idx


@pytest.mark.parametrize("pinned", [False, True])
def test_gather_rows(pinned):
    """mmvae_gather_rows == src[idx], byte for byte: rows of 16, 48, 32768 (one part), 32784 (two) and 65552 bytes (three parts with an
    uneven last share) through the 16-byte kernel, 4, 20 and 2500 bytes through the 4-byte kernel; 1, 3 and (rows under 7 KB) 300 rows
    with repeated, reversed and out-of-order indices; the source in device memory and in pinned host memory; guard rows on both sides of dst"""
    call, ptr, stream = _api()
    dev = _dev()
    n_src = 7
    for row_bytes in (16, 48, 32768, 32784, 65552, 4, 20, 2500):
        g = torch.Generator().manual_seed(row_bytes)
        src = torch.randint(0, 256, (n_src, row_bytes), dtype=torch.uint8, generator=g)
        src_d = src.pin_memory() if pinned else src.to(dev)
        for rows in (r for r in (1, 3, 300) if (r + 2) * row_bytes <= 2 << 20):        # (no buffer of these tests is larger than 2 MB)
            idx = _indices(rows, n_src)
            idx_d = idx.pin_memory() if pinned else idx.to(dev)
            dst = torch.full((rows + 2, row_bytes), 0xA5, dtype=torch.uint8, device=dev)
            call("mmvae_gather_rows", ptr(src_d), ptr(idx_d), rows, row_bytes, ctypes.c_void_p(dst.data_ptr() + row_bytes), stream())
            torch.cuda.synchronize()
            assert torch.equal(dst[1:rows + 1].cpu(), src[idx]), (row_bytes, rows)
            assert bool((dst[0] == 0xA5).all()) and bool((dst[rows + 1] == 0xA5).all()), (row_bytes, rows)


def test_u8_to_f32_and_gather_rows_u8_f32():
    """ToTensor on the device: all 256 byte values, denominators 255 and 256, bit-equal to x.float() / denom; mmvae_u8_to_f32 at n = 1,
    15, 16, 17, 4097, mmvae_gather_rows_u8_f32 at rows of 4 and 2500 elements (1, 3, 300 rows); guards behind (and rows around) dst"""
    call, ptr, stream = _api()
    dev = _dev()
    for denom in (255.0, 256.0):
        for n in (1, 15, 16, 17, 4097):
            x = (torch.arange(n) * 37 % 256).to(torch.uint8) if n >= 256 else torch.randint(0, 256, (n,), dtype=torch.uint8, generator=torch.Generator().manual_seed(n))
            dst = torch.full((n + S.GUARD,), float("nan"), device=dev)
            xd = x.to(dev)
            call("mmvae_u8_to_f32", ptr(xd), n, denom, ptr(dst), stream())
            torch.cuda.synchronize()
            assert torch.equal(dst[:n].cpu().view(torch.int32), (x.float() / denom).view(torch.int32)) and bool(torch.isnan(dst[n:]).all()), (n, denom)
        assert set((torch.arange(4097) * 37 % 256).tolist()) == set(range(256))
        for row_elems in (4, 2500):
            src = (torch.arange(8 * row_elems) * 37 % 256).to(torch.uint8).view(8, row_elems)
            if row_elems == 4:
                src = torch.arange(256, dtype=torch.uint8).view(64, 4)                      # all 256 values in rows of 4
            src_d = src.to(dev)
            for rows in (1, 3, 300):
                idx = _indices(rows, src.shape[0])
                idx_d = idx.to(dev)
                lead = (row_elems + 3) // 4 * 4                                             # dst stays 16-byte aligned
                dst = torch.full((lead + (rows + 1) * row_elems,), float("nan"), device=dev)
                call("mmvae_gather_rows_u8_f32", ptr(src_d), ptr(idx_d), rows, row_elems, denom, ctypes.c_void_p(dst.data_ptr() + 4 * lead), stream())
                torch.cuda.synchronize()
                got = dst[lead:lead + rows * row_elems].view(rows, row_elems).cpu()
                assert torch.equal(got.view(torch.int32), (src[idx].float() / denom).view(torch.int32)), (row_elems, rows, denom)
                assert bool(torch.isnan(dst[:lead]).all()) and bool(torch.isnan(dst[lead + rows * row_elems:]).all())


def test_feed_kernels_refuse():
    """a row of 6 bytes, a misaligned destination and rows = 0 come back as errors with a message; nothing is written"""
    from multimodal_vae_amd._lib import MMVAEError
    call, ptr, stream = _api()
    dev = _dev()
    src = torch.zeros(4096, dtype=torch.uint8, device=dev)
    dst = torch.full((4096,), 0xA5, dtype=torch.uint8, device=dev)
    idx = torch.zeros(4, dtype=torch.int64, device=dev)
    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
    bad = [("mmvae_gather_rows", (ptr(src), ptr(idx), 2, 6, ptr(dst), stream())),
           ("mmvae_gather_rows", (ptr(src), ptr(idx), 2, 16, off(dst, 4), stream())),
           ("mmvae_gather_rows", (ptr(src), ptr(idx), 2, 20, off(dst, 2), stream())),
           ("mmvae_gather_rows", (ptr(src), ptr(idx), 0, 16, ptr(dst), stream())),
           ("mmvae_gather_rows", (ptr(src), None, 2, 16, ptr(dst), stream())),
           ("mmvae_gather_rows_u8_f32", (ptr(src), ptr(idx), 2, 6, 255.0, ptr(dst), stream())),
           ("mmvae_gather_rows_u8_f32", (ptr(src), ptr(idx), 2, 8, 255.0, off(dst, 4), stream())),
           ("mmvae_gather_rows_u8_f32", (ptr(src), ptr(idx), 0, 8, 255.0, ptr(dst), stream())),
           ("mmvae_u8_to_f32", (None, 8, 255.0, ptr(dst), stream())), ("mmvae_u8_to_f32", (ptr(src), -1, 255.0, ptr(dst), stream()))]
    for name, args in bad:
        with pytest.raises(MMVAEError) as e:
            call(name, *args)
        assert len(str(e.value)) > 10, name
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all())
