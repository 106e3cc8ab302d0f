"""The weight refresh (csrc/elementwise.hip pack_block, csrc/pack_geo.h) under its two lane assignments and in the staged prologue of
the fused MultiMNIST step.

Knob ``pack_runs`` = 1 (default) lets the lanes of a wave walk the source's contiguous direction, 0 is the row-major assignment it
replaced; both write the same elements, so the packed buffers must be equal BIT FOR BIT for every family that packs.  Parameters
are random, mixed with values exactly half-way between two bf16 numbers (the rounding ties) and with +-0.

The staged prologue issues three launches whose grids hold only the workgroups of their own descriptors: after one step the whole
buffer equals a full pack of the step's starting parameters, and each stage's launch alone (mmvae_mm_debug_pack_stage) changes
exactly the bytes of the descriptors of its stage.  Plans at B = 8: the packs do not depend on the batch and 8 is the smallest
batch of the fused step."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MARK = 0x7FC1       # a bf16 NaN with a payload: no pack of finite parameters writes it

# struct PackDesc (csrc/pack_geo.h), natural C alignment
DESC = np.dtype([("dst_off", "<i8"), ("src_off", "<i8"), ("Npad", "<i4"), ("Kpad", "<i4"), ("N", "<i4"), ("K", "<i4"), ("NL", "<i4"),
                 ("s_nhi", "<i4"), ("s_nlo", "<i4"), ("TW", "<i4"), ("C", "<i4"), ("s_ty", "<i4"), ("s_tx", "<i4"), ("s_c", "<i4"),
                 ("o_ty", "<i4"), ("o_tx", "<i4"), ("step_t", "<i4"), ("is_f32", "<i4"), ("bias_off", "<i8"), ("b_nhi", "<i4"),
                 ("b_nlo", "<i4"), ("first_block", "<i4"), ("part", "<i4"), ("frag", "<i4")], align=True)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _tricky_params(st, seed):
    """random weights; a third sit on a bf16 rounding tie (low 16 bits 0x8000), some are +0 / -0"""
    g = torch.Generator().manual_seed(seed)
    bits = (torch.randn(st.nparams, generator=g) * 0.1).view(torch.int32)
    kind = torch.randint(0, 12, (st.nparams,), generator=g)
    tie = (bits & -65536) | 0x8000
    bits = torch.where(kind < 4, tie, bits)
    bits = torch.where(kind == 4, torch.zeros_like(bits), bits)
    bits = torch.where(kind == 5, torch.full_like(bits, -2 ** 31), bits)
    st.params.copy_(bits.view(torch.float32).to(st.device))


def _mark(st):
    st.packed.view(torch.int16).fill_(MARK)
    st.packed_vec.view(torch.int32).fill_(0x7FC00001)


def _pack(st, h, runs):
    """one full pack through the family's own entry point, on the plan h, under pack_runs = runs"""
    from multimodal_vae_amd._lib import knobs
    from multimodal_vae_amd.core import _stream
    with knobs(pack_runs=runs):
        _mark(st)
        st._c("pack_weights", h, _stream())
        torch.cuda.synchronize()
    return st.packed.view(torch.int16).clone(), st.packed_vec.view(torch.int32).clone()


def _make(family, dev):
    from multimodal_vae_amd import core
    if family == "mm20":
        return core.MultimnistState(20, dev)
    if family == "mm100":
        return core.MultimnistState(100, dev)
    if family == "celeba":
        return core.CelebaState(100, dev)
    if family == "coco":
        return core.CocoState(100, dev, 8)
    return core.MultimnistTextState(100, dev, 50)


@pytest.mark.parametrize("family", ["mm20", "mm100", "celeba", "coco", "mmtext"])
def test_both_assignments_pack_the_same_bits(family):
    dev = _dev()
    st = _make(family, dev)
    _tricky_params(st, 17)
    h = st.plan(8)
    old, oldv = _pack(st, h, 0)
    new, newv = _pack(st, h, 1)
    assert int((old == MARK).sum()) == 0          # the reference itself wrote every element
    assert torch.equal(new, old), int((new != old).sum())
    assert torch.equal(newv, oldv)
    assert int((old != 0).sum()) > st.nparams // 4    # (and it is a pack of these parameters, not an empty buffer)


def _stage_launch(st, h, stage):
    from multimodal_vae_amd._lib import load
    from multimodal_vae_amd.core import _stream
    fn = load().mmvae_mm_debug_pack_stage
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p]
    blocks = C.c_int(-1)
    assert fn(h, stage, C.byref(blocks), _stream()) == 0
    torch.cuda.synchronize()
    return blocks.value


@pytest.mark.parametrize("runs", [1, 0])
def test_each_stage_launch_packs_its_own_descriptors_only(runs):
    from multimodal_vae_amd._lib import knobs
    from multimodal_vae_amd.core import MultimnistState
    dev = _dev()
    st = MultimnistState(100, dev)
    _tricky_params(st, 23)
    h = st.plan(8)
    ref, _ = _pack(st, h, 0)
    desc = np.frombuffer(st._desc[0].cpu().numpy().tobytes(), dtype=DESC)
    assert desc.nbytes == st._desc[0].numel() and set(desc["part"]) == {0, 1, 2} and not desc["is_f32"].any()
    nblk = (desc["Npad"].astype(np.int64) * (desc["Kpad"] // 8) + 255) // 256
    owner = torch.full((st.packed.numel(),), -1, dtype=torch.int8)
    for d in desc:
        owner[int(d["dst_off"]):int(d["dst_off"]) + int(d["Npad"]) * int(d["Kpad"])] = int(d["part"])
    assert int((owner < 0).sum()) == 0
    owner = owner.to(dev)
    with knobs(pack_runs=runs):
        for stage in (0, 1, 2, -1):
            _mark(st)
            blocks = _stage_launch(st, h, stage)
            got = st.packed.view(torch.int16)
            mine = owner == stage if stage >= 0 else owner >= 0
            assert blocks == int(nblk[desc["part"] == stage].sum() if stage >= 0 else nblk.sum())     # no workgroup of another stage
            assert torch.equal(got[mine], ref[mine]), stage
            assert bool((got[~mine] == MARK).all()), stage


@pytest.mark.parametrize("staged", [1, 0])
def test_step_with_pack_first_refreshes_the_whole_buffer(staged):
    from multimodal_vae_amd._lib import knobs
    from multimodal_vae_amd.core import FusedELBOStep, MultimnistState
    from multimodal_vae_amd.init import default_init_
    dev = _dev()
    B = 8
    rng = np.random.default_rng(3)
    img = torch.from_numpy((rng.random((B, 1, 50, 50)) < 0.2).astype(np.float32)).to(dev)
    txt = torch.from_numpy(rng.integers(0, 10, size=(B, 4)).astype(np.int64)).to(dev)
    st = MultimnistState(100, dev); default_init_(st, 21)
    eng = FusedELBOStep(st, B, lr=1e-2)
    with knobs(mm_stage_begin=staged):
        eng(img, txt)
        assert st.pack_pending
        p_start = st.params.clone()
        _mark(st)
        eng(img, txt)                              # the prologue packs p_start over the marks; then forward, backward, Adam
        torch.cuda.synchronize()
        got = st.packed.view(torch.int16).clone()
        p_end = st.params.clone()
        st.params.copy_(p_start)
        ref, _ = _pack(st, st.plan(B), 0)
        st.params.copy_(p_end); st.pack_pending = True
        assert torch.equal(got, ref), int((got != ref).sum())


def test_graph_replay_matches_eager_steps():
    """as test_training_reduces_loss_and_graph_matches_eager, at B = 8: twin engines, 4 eager steps against 2 eager (capture's
    warm-up) + 2 replays -- the captured prologue launches carry their stage grids.  rtol 2e-2 is that test's bound (float
    atomics: two runs of the same step differ by their summation order).  The packed buffer is marked before the last replay:
    its prologue rewrites every element."""
    from multimodal_vae_amd.core import FusedELBOStep, MultimnistState
    from multimodal_vae_amd.init import default_init_
    dev = _dev()
    B = 8
    rng = np.random.default_rng(0)
    img = torch.from_numpy((rng.random((B, 1, 50, 50)) < 0.15).astype(np.float32)).to(dev)
    txt = torch.from_numpy(rng.integers(0, 10, size=(B, 4)).astype(np.int64)).to(dev)
    sa = MultimnistState(100, dev); default_init_(sa, 11)
    sb = MultimnistState(100, dev); default_init_(sb, 11)
    ea, eb = FusedELBOStep(sa, B, seed=5), FusedELBOStep(sb, B, seed=5)
    for _ in range(4):
        la = ea(img, txt).losses().cpu().numpy()
    eb.capture(img, txt)
    eb.replay()
    torch.cuda.synchronize()
    _mark(sb)
    lb = eb.replay().losses().cpu().numpy()
    torch.cuda.synchronize()
    assert np.isfinite(la).all() and np.isfinite(lb).all()
    np.testing.assert_allclose(lb, la, rtol=2e-2)
    assert int((sb.packed.view(torch.int16) == MARK).sum()) == 0
