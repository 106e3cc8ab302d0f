"""GPU tests of the fused MMD op (csrc/mmd.hip) against float64 (tests/mmd_ref.py).

Exact cases: with every row the same vector all kernel values are 1, with one row offset by 30 in every coordinate its kernel values
underflow to exactly 0 (exp(-225)); the three means are then ratios of integers, computed here in float64 and rounded to fp32, and
the op must return exactly those bits -- n_x * n_y is above 2^24, so any fp32 fold fails.

Real-valued cases: the gate is 4 x the error of the reference's own formulation in fp32 torch ops on the CPU, on the same inputs,
against float64: |error| / (mean Kxx + mean Kyy + 2 mean Kxy) for the four terms, max |error| / max |gradient| for dx and dy.
tests/test_cpu_mmd.py shows that each of these gates sees a missing row tile, column tile or column split.

Measured on an MI355X (error of the op / yardstick; `pytest -s` prints them): see MEASURED below and profiles/mmd_bench.txt.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mmd_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

MEASURED = """
error of the op / yardstick (= error of the fp32 formulation on the CPU), both against float64; the gate is 4 x the yardstick
(n_x, n_y, D)          value                  dx                     dy
(1, 2, 20)             3.1e-08 / 3.1e-08      7.5e-08 / 7.8e-08      8.7e-08 / 2.1e-07
(2, 1, 21)             2.2e-08 / 8.7e-09      6.3e-08 / 9.4e-08      7.7e-08 / 4.9e-08
(31, 64, 100)          8.1e-09 / 1.4e-08      2.2e-07 / 7.3e-07      3.9e-07 / 7.8e-07
(32, 63, 1)            7.9e-09 / 5.9e-08      8.3e-08 / 1.4e-07      9.1e-08 / 2.1e-07
(33, 65, 2)            7.9e-09 / 1.9e-08      1.1e-07 / 1.3e-07      9.5e-08 / 2.1e-07
(63, 32, 256)          3.4e-09 / 3.4e-09      2.0e-07 / 5.4e-07      3.3e-07 / 1.1e-06
(64, 31, 20)           8.8e-09 / 2.6e-08      2.0e-07 / 4.7e-07      1.8e-07 / 6.5e-07
(65, 33, 100)          6.3e-09 / 5.9e-08      2.0e-07 / 6.1e-07      2.0e-07 / 8.4e-07
(67, 131, 21)          7.7e-09 / 1.1e-08      1.4e-07 / 6.6e-07      2.0e-07 / 8.8e-07
(131, 67, 256)         7.3e-09 / 2.5e-08      1.9e-07 / 7.7e-07      2.9e-07 / 1.1e-06
(70, 70, 20) same      2.2e-09 / 1.4e-08      0 / 1.6e-07            0 / 1.6e-07
(2051, 4099, 100)      3.5e-09 / 3.5e-09      1.3e-07 / 2.0e-06      1.9e-07 / 1.5e-06
The largest ratio is 2.5 (the value at (2, 1, 21): 1.4 ulp of one mean against 0.6 ulp by chance); where both figures agree the
error is the rounding of the exact result to fp32.  compute_kernel, largest elementwise error / yardstick: 3.5e-08 / 3.5e-08,
4.6e-08 / 5.0e-08, 3.3e-08 / 3.4e-08.
"""


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _geometry():
    from multimodal_vae_amd.mmd import mmd_geometry
    return mmd_geometry()


def _report(label, **kw):
    print("MMD %-34s %s" % (label, "  ".join("%s %.3e" % (k, v) for k, v in kw.items())))


def _op(x, y, dev, grad=True):
    """-> (terms (4,), dx, dy) through the C boundary with a workspace of the test's own"""
    from multimodal_vae_amd._lib import call, ptr
    xd = x.to(dev).contiguous()
    yd = xd if y is x else y.to(dev).contiguous()
    need = call("mmvae_mmd_workspace_bytes", xd.shape[0], yd.shape[0], xd.shape[1])
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(4, device=dev)
    dx, dy = (torch.empty_like(xd), torch.empty_like(yd)) if grad else (None, None)
    call("mmvae_mmd", ptr(xd), xd.shape[0], ptr(yd), yd.shape[0], xd.shape[1], ptr(ws), need, ptr(out), ptr(dx), ptr(dy),
         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return out, dx, dy, ws


# ------------------------------------------------------------------------------------------------------ exact cases
NX, NY, DX = 4099, 4100, 4


def _exact_inputs(outlier):
    base = torch.tensor([1.0, -2.0, 3.0, 0.5])
    x, y = base.repeat(NX, 1), base.repeat(NY, 1)
    if outlier is not None:
        (x if outlier[0] == "x" else y)[outlier[1]] += 30.0
    return x, y


def _exact_terms(outlier):
    """the float64 means of 0 / 1 kernel values (ratios of integers) and MMD, rounded to fp32 once"""
    nx, ny = np.float64(NX), np.float64(NY)
    sxx, syy, sxy = nx * nx, ny * ny, nx * ny
    if outlier is not None and outlier[0] == "x":
        sxx, sxy = (nx - 1) * (nx - 1) + 1, (nx - 1) * ny
    if outlier is not None and outlier[0] == "y":
        syy, sxy = (ny - 1) * (ny - 1) + 1, nx * (ny - 1)
    kxx, kyy, kxy = sxx / (nx * nx), syy / (ny * ny), sxy / (nx * ny)
    return torch.tensor([kxx, kyy, kxy, (kxx + kyy) - 2.0 * kxy], dtype=torch.float64).float()


def test_exact_means_of_identical_rows():
    dev = _dev()
    assert NX * NY > 2 ** 24
    out, dx, dy, _ = _op(*_exact_inputs(None), dev)
    assert out.cpu().tolist() == [1.0, 1.0, 1.0, 0.0]
    assert int(torch.count_nonzero(dx)) == 0 and int(torch.count_nonzero(dy)) == 0


def _outlier_positions():
    rt, ct, _ = _geometry()
    pos = []
    for cls, n in (("x", NX), ("y", NY)):
        rtx, rty, tx, ty, sx, sy = R.split_rule(NX, NY, rt, ct)
        tiles, splits = (tx, sx) if cls == "x" else (ty, sy)
        assert splits >= 3
        lo, hi = R.split_rows(tiles, splits, 1, ct, n)              # the second column split of the class
        last_lo, _ = R.split_rows(tiles, splits, splits - 1, ct, n)
        for i in sorted({0, ct - 1, ct, rt - 1, rt, lo - 1, lo, hi - 1, hi, last_lo, n - 1}):
            pos.append((cls, i))
    return pos


def test_exact_counts_with_one_outlier_row():
    dev = _dev()
    for outlier in _outlier_positions():
        out, dx, dy, _ = _op(*_exact_inputs(outlier), dev)
        want = _exact_terms(outlier)
        assert torch.equal(out.cpu(), want), (outlier, out.cpu().tolist(), want.tolist())
        # k is 1 where d = 0 and 0 where d = +-30: every gradient entry is an exact zero
        assert int(torch.count_nonzero(dx)) == 0 and int(torch.count_nonzero(dy)) == 0, outlier


# ------------------------------------------------------------------------------------------------------ real-valued inputs
def _real_shapes():
    """Every size of {1, 2, tile - 1, tile, tile + 1, 2 tile + 3} for the row tile and for the column tile appears as n_x and as
    n_y, n_x != n_y, and every D of {1, 2, 20, 21, 100, max_dim} appears."""
    rt, ct, md = 64, 32, 256                                       # checked against mmvae_mmd_geometry in the test
    return [(1, 2, 20), (2, 1, 21), (ct - 1, rt, 100), (ct, rt - 1, 1), (ct + 1, rt + 1, 2), (rt - 1, ct, md), (rt, ct - 1, 20),
            (rt + 1, ct + 1, 100), (2 * ct + 3, 2 * rt + 3, 21), (2 * rt + 3, 2 * ct + 3, md)]


def test_real_shapes_cover_the_geometry():
    rt, ct, md = _geometry()
    shapes = _real_shapes()
    sizes = {1, 2, rt - 1, rt, rt + 1, 2 * rt + 3, ct - 1, ct, ct + 1, 2 * ct + 3}
    assert {s[0] for s in shapes} == sizes and {s[1] for s in shapes} == sizes and all(s[0] != s[1] for s in shapes)
    assert {s[2] for s in shapes} == {1, 2, 20, 21, 100, md}


def _check_real(nx, ny, D, same, dev):
    c = R.real_case(nx, ny, D, same)
    out, dx, dy, _ = _op(c["x"], c["y"], dev)
    yard, ref = c["yardstick"], c["ref"]
    if same:                                                       # what autograd leaves on the one tensor: dx + dy, against zero
        dx = dy = dx + dy
    err = {"value": R.value_error(out, ref["terms"]), "dx": R.grad_error(dx, ref["dx"], c["scale"]),
           "dy": R.grad_error(dy, ref["dy"], c["scale"])}
    _report("(%d, %d, %d)%s" % (nx, ny, D, " same" if same else ""), **{k: err[k] for k in err}, **{"yard_" + k: yard[k] for k in yard})
    for k in err:
        assert err[k] <= R.GATE_FACTOR * yard[k], (k, err[k], yard[k])


@pytest.mark.parametrize("nx,ny,D", _real_shapes())
def test_real_valued_inputs(nx, ny, D):
    _check_real(nx, ny, D, False, _dev())


def test_real_valued_inputs_same_tensor():
    _check_real(70, 70, 20, True, _dev())


def test_real_valued_inputs_across_several_splits():
    rt, ct, _ = _geometry()
    assert min(R.split_rule(2051, 4099, rt, ct)[4:]) >= 3
    _check_real(2051, 4099, 100, False, _dev())


# ------------------------------------------------------------------------------------------------------ other checks
@pytest.mark.parametrize("nx,ny,D", [(65, 33, 100), (3, 131, 21), (40, 40, 256)])
def test_compute_kernel_elementwise(nx, ny, D):
    from multimodal_vae_amd.mmd import compute_kernel
    dev = _dev()
    x, y = R.real_inputs(nx, ny, D)
    k64 = R.kernel64(x, y)
    yard = float((R.formulation_kernel(x, y).double() - k64).abs().max())
    k = compute_kernel(x.to(dev), y.to(dev))
    assert k.shape == (nx, ny) and k.dtype == torch.float32 and not k.requires_grad
    err = float((k.double().cpu() - k64).abs().max())
    _report("kernel (%d, %d, %d)" % (nx, ny, D), err=err, yard=yard)
    assert err <= R.GATE_FACTOR * yard
    kk = compute_kernel(x.to(dev), x.to(dev))
    assert torch.equal(torch.diagonal(kk), torch.ones(nx, device=dev))
    # the fused op sums exactly these values: the mean of the matrix is its third term
    from multimodal_vae_amd.mmd import mmd_terms
    assert abs(float(mmd_terms(x.to(dev), y.to(dev))[2]) - float(k.double().mean())) < 1e-6


def test_two_calls_give_identical_bits():
    from multimodal_vae_amd._lib import call, ptr
    dev = _dev()
    x, y = R.real_inputs(300, 517, 100)
    out1, dx1, dy1, ws = _op(x, y, dev)
    xd, yd = x.to(dev), y.to(dev)
    ws.fill_(0xFF)                                                 # NaN in every float64 of the workspace
    out2, dx2, dy2 = torch.empty_like(out1), torch.empty_like(dx1), torch.empty_like(dy1)
    call("mmvae_mmd", ptr(xd), 300, ptr(yd), 517, 100, ptr(ws), ws.numel(), ptr(out2), ptr(dx2), ptr(dy2),
         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    for a, b in ((out1, out2), (dx1, dx2), (dy1, dy2)):
        assert bool(torch.isfinite(b).all()) and torch.equal(a.view(torch.int32), b.view(torch.int32))
    out3, _, _, _ = _op(x, y, dev, grad=False)                    # the value-only sweep sums the same pairs in the same order
    assert torch.equal(out1.view(torch.int32), out3.view(torch.int32))


def test_autograd_through_compute_mmd():
    from multimodal_vae_amd.mmd import compute_mmd, mmd_terms
    dev = _dev()
    c = R.real_case(65, 33, 100)
    x = c["x"].to(dev).requires_grad_(True)
    y = c["y"].to(dev).requires_grad_(True)
    mmd = compute_mmd(x, y)
    assert mmd.dim() == 0 and mmd.is_cuda and mmd.requires_grad
    (mmd * 2.5).backward()
    t64 = c["ref"]["terms"]
    assert abs(float(mmd) - float(t64[3])) / float(t64[0] + t64[1] + 2 * t64[2]) <= R.GATE_FACTOR * c["yardstick"]["value"]
    assert R.grad_error(x.grad / 2.5, c["ref"]["dx"]) <= R.GATE_FACTOR * c["yardstick"]["dx"]
    assert R.grad_error(y.grad / 2.5, c["ref"]["dy"]) <= R.GATE_FACTOR * c["yardstick"]["dy"]
    # one input only, and none
    y2 = c["y"].to(dev).requires_grad_(True)
    compute_mmd(c["x"].to(dev), y2).backward()
    assert R.grad_error(y2.grad, c["ref"]["dy"]) <= R.GATE_FACTOR * c["yardstick"]["dy"]
    t = mmd_terms(c["x"].to(dev), c["y"].to(dev))
    assert t.shape == (4,) and not t.requires_grad and float(t[3]) == float(mmd.detach())


def test_refusals_do_not_launch():
    from multimodal_vae_amd import MMVAEError, mmd
    from multimodal_vae_amd._lib import call, ptr
    dev = _dev()
    _, _, md = _geometry()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.zeros(4, 8, device=dev)
    out = torch.full((4,), 7.0, device=dev)
    need = call("mmvae_mmd_workspace_bytes", 4, 4, 8)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    for args in ([ptr(x), 4, ptr(x), 4, 0, ptr(ws), need, ptr(out), None, None, s],
                 [ptr(x), 4, ptr(x), 4, md + 1, ptr(ws), need, ptr(out), None, None, s],
                 [ptr(x), 0, ptr(x), 4, 8, ptr(ws), need, ptr(out), None, None, s],
                 [ptr(x), 4, ptr(x), 0, 8, ptr(ws), need, ptr(out), None, None, s],
                 [ptr(x), 4, ptr(x), 4, 8, ptr(ws), need - 1, ptr(out), None, None, s]):
        with pytest.raises(MMVAEError):
            call("mmvae_mmd", *args)
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [7.0] * 4                         # nothing ran
    for bad in (torch.zeros(4, 0, device=dev), torch.zeros(0, 8, device=dev), torch.zeros(4, md + 1, device=dev)):
        with pytest.raises(MMVAEError):
            mmd.compute_mmd(bad, bad)
    with pytest.raises(MMVAEError):
        mmd.compute_mmd(x, torch.zeros(4, 9, device=dev))
    with pytest.raises(MMVAEError):
        mmd.compute_mmd(x.double(), x.double())
