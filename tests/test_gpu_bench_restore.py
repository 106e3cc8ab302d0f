"""bench.py restarts its last timed step from the seeded initial state (training_state / restore_training_state): after k steps and
the restore, the next step must compute what a fresh engine's first step computes, up to the rounding of the step's float atomics.
A training-state buffer that a later change adds but leaves out of training_state() shows up here."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu
LR = 1e-3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _engine(wl, dev):
    """The engine, state and batch bench.py builds for `wl` on one GPU (default batch, n_latents 100, seed 1234)."""
    import multimodal_vae_amd  # noqa: F401
    from multimodal_vae_amd import core
    from multimodal_vae_amd.init import default_init_
    B, D, seed = bench.DEFAULT_BATCH[wl], 100, 1234
    if wl == "multimnist":
        st = core.MultimnistState(D, dev)
        default_init_(st, seed=seed)
        eng = core.FusedELBOStep(st, B, lr=LR, seed=seed)
    elif wl == "celeba":
        st = core.CelebaState(D, dev)
        default_init_(st, seed=seed)
        eng = core.FusedCelebaStep(st, B, lr=LR, seed=seed)
    else:
        st = core.CocoState(D, dev)
        default_init_(st, seed=seed)
        eng = core.FusedCocoStep(st, B, bench.synthetic_sos(), lr=LR, seed=seed)
    a, b = bench.synthetic_batch_for(wl, B, seed)
    return eng, a.to(dev).contiguous(), b.to(dev).contiguous()


def _after_step(eng, out):
    torch.cuda.synchronize()
    st = eng.state
    return (out.losses().cpu().double(), st.grads.double().clone(), eng.exp_avg.double().clone(), st.params.double().clone(),
            st.bn_stats.double().clone())


@pytest.mark.parametrize("wl", ["multimnist", "celeba", "coco"])
def test_restored_step_equals_a_fresh_first_step(wl):
    dev = _dev()
    fresh, a, b = _engine(wl, dev)
    p0 = fresh.state.params.double().clone()
    want = _after_step(fresh, fresh(a, b))
    del fresh

    eng, a, b = _engine(wl, dev)
    saved = [t.clone() for t in bench.training_state(eng)]
    for _ in range(3):
        eng(a, b)
    bench.restore_training_state(eng, saved)
    got = _after_step(eng, eng(a, b))

    losses, grads, m, params, bn = got
    w_losses, w_grads, w_m, w_params, w_bn = want
    torch.testing.assert_close(losses, w_losses, rtol=1e-4, atol=0)
    for name, x, y in (("grads", grads, w_grads), ("exp_avg", m, w_m), ("bn_stats", bn, w_bn)):
        err = (x - y).abs().max().item()
        assert err <= 2e-3 * y.abs().max().item(), (wl, name, err, y.abs().max().item())
    # Adam's first update is lr x sign(g): an element whose gradient is rounding noise may move by 2 lr the other way, every other
    # one matches.  A state buffer left out of the restore (moments, step count, parameters) moves most elements by O(lr).
    dp = (params - w_params).abs()
    assert dp.max().item() <= 2.2 * LR, (wl, dp.max().item())
    assert dp.mean().item() <= 0.2 * LR, (wl, dp.mean().item())
    assert (w_params - p0).abs().mean().item() > 0.5 * LR           # the step did update the parameters
