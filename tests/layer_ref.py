"""Layer-level reference and GPU harness of the MultiMNIST conv / transposed-conv kernels (tests/test_gpu_layers.py,
tests/test_cpu_layer_ref.py).

One layer of the step is replayed through mmvae_mm_bench_layer on operands the test wrote itself and compared with a float64
reference made here with torch.nn.functional.conv2d / conv_transpose2d and torch.autograd -- never with another engine kernel.
Operands are ternary {-1, 0, +1}: bf16 holds them exactly, every product is an integer and every fp32 partial sum stays below
2^24, so the result depends neither on the accumulation order nor on the rounding of the bf16 store and the comparison is
torch.equal.  The float epilogue of the data-gradient layers (Swish' and the BatchNorm-backward sums, csrc/gemm.h GemmParams
d_r / d_affine / d_meanrstd / d_red) is restated in float64 and gated by the precision of the formats alone.

The top half of this module needs no GPU (geometry table, operand generator, references); LayerHarness needs the MI355X."""
import ctypes
from collections import namedtuple

import torch
import torch.nn.functional as F

STAT_SLOTS = 16                 # MMVAE_STAT_SLOTS (csrc/common.h)
BATCHES = (7, 8, 12, 86, 88, 96, 256)
SEEDS = (0, 1)

# Geometry of multimnist/model.py:160-169 (image encoder features.*) and :199-208 (image decoder hallucinate.*), and the workspace
# buffers each engine layer reads and writes (csrc/multimnist.hip layer_gemm / layer_wgrad).  Activations are NHWC
# [image][y][x][channel].  gf / gb: BatchNorm groups (passes) of the forward and of the two gradient launches; a group is B images.
#   x / out / stats : forward operand, raw output, column statistics [gf][STAT_SLOTS][cout] (sum v, sum v^2)
#   dy / dx / r     : data gradient: gradient w.r.t. the raw output, result, saved raw tensor of the result's geometry
#   aff / mr / red  : (scale, shift) and (mean, rstd) tables [gb][cin] of the BatchNorm below, its sums [gb][STAT_SLOTS][cin]
Layer = namedtuple("Layer", "param transposed cin cout k stride pad ih oh gf gb x out stats dy dx r aff mr red x_density")
LAYERS = {
    "enc_conv2": Layer("image_encoder.features.2.weight", False, 32, 64, 4, 2, 1, 25, 12, 1, 1,
                       "a1", "r2", "st_e0", "d2e", "d1e", "r1", None, None, None, 0.5),
    "enc_conv3": Layer("image_encoder.features.5.weight", False, 64, 128, 4, 2, 1, 12, 6, 1, 1,
                       "a2", "r3", "st_e1", "d3e", "d2e", "r2", "aff_e0", "mr_e0", "red_e0", 0.5),
    "enc_conv4": Layer("image_encoder.features.8.weight", False, 128, 256, 4, 2, 0, 6, 2, 1, 1,
                       "a3", "r4", "st_e2", "dr4", "d3e", "r3", "aff_e1", "mr_e1", "red_e1", 0.5),
    "dec_convT1": Layer("image_decoder.hallucinate.0.weight", True, 256, 128, 4, 2, 0, 2, 6, 3, 2,
                        "au", "q1", "st_d0", "d1", "du", "u", None, None, None, 0.5),
    "dec_convT2": Layer("image_decoder.hallucinate.3.weight", True, 128, 64, 4, 2, 1, 6, 12, 3, 2,
                        "aq1", "q2", "st_d1", "d2", "d1", "q1", "aff_d0", "mr_d0", "red_d0", 0.5),
    # (activation density 1/4: at 768 images and density 1/2 a channel's sum of squares reaches 2.2e7 > 2^24)
    "dec_convT3": Layer("image_decoder.hallucinate.6.weight", True, 64, 32, 5, 2, 1, 12, 25, 3, 2,
                        "aq2", "q3", "st_d2", "d3", "d2", "q2", "aff_d1", "mr_d1", "red_d1", 0.25),
}
W_DENSITY = 0.25
G_DENSITY = 0.5

# every workspace name mmvae_mm_debug_offset knows (csrc/multimnist.hip): the end of a named buffer is bounded by the next of these
WS_NAMES = ("patches1 r1 r2 r3 r4 y1 y2 encout txtout z_bf z_f32 u q1 q2 q3 logits dlogit d3 d2 d1 du dz_img dz_txt d_encout "
            "d_txtout dy2 dy1 db4 dr4 d3e d2e d1e aff_d0 aff_d1 aff_d2 st_d0 patches4 tmp_f32 aff_e0 aff_e1 aff_e2 eps m1 m2 gkeep "
            "st_e0 st_e1 st_e2 st_d1 st_d2 red_e0 red_e1 red_e2 red_d0 red_d1 red_d2 a1 a2 a3 aq1 aq2 aq3 "
            "a4 au ay1 ay2 mr_e0 mr_e1 mr_e2 mr_d0 mr_d1 mr_d2 slab").split()


# ------------------------------------------------------------------------------------------------ operands
def gen(seed, *salt):
    g = torch.Generator()
    g.manual_seed(1000003 * seed + sum((i + 1) * 7919 * int(s) for i, s in enumerate(salt)) + 17)
    return g


def ternary(shape, density, g):
    """float64 tensor of {-1, 0, +1}, nonzero with probability `density`."""
    nz = torch.rand(shape, generator=g, dtype=torch.float32) < density
    sign = torch.randint(0, 2, shape, generator=g, dtype=torch.int8) * 2 - 1
    return (nz.to(torch.int8) * sign).double()


def weight_shape(L):
    return (L.cin, L.cout, L.k, L.k) if L.transposed else (L.cout, L.cin, L.k, L.k)


def layer_operands(name, nimg, seed):
    """(x [nimg][ih][ih][cin], w in the parameter's layout, dy [nimg][oh][oh][cout]) -- one draw per (layer, seed); the images of a
    smaller batch are a prefix of a larger one's only by accident, nothing relies on it."""
    L = LAYERS[name]
    idx = list(LAYERS).index(name)
    w = ternary(weight_shape(L), W_DENSITY, gen(seed, idx, 1))
    x = ternary((nimg, L.ih, L.ih, L.cin), L.x_density, gen(seed, idx, 2, nimg))
    dy = ternary((nimg, L.oh, L.oh, L.cout), G_DENSITY, gen(seed, idx, 3, nimg))
    return x, w, dy


def dyadic_tables(groups, C, g):
    """(scale, shift), (mean, rstd) tables [groups][C][2] of dyadic rationals: scale * r + shift and (r - mean) * rstd are exact in
    fp32 for r a multiple of 1/8 in [-4, 4]."""
    pick = lambda vals: torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), (groups, C), generator=g)]
    aff = torch.stack([pick([0.5, 1.0, 2.0, -1.0]), pick([-0.5, 0.0, 0.25, 1.0])], -1)
    mr = torch.stack([pick([-0.25, 0.0, 0.5]), pick([0.5, 1.0, 2.0])], -1)
    return aff, mr


def eighths(shape, g):
    """multiples of 1/8 in [-4, 4] (exact in bf16: |k| <= 32 needs 6 bits)"""
    return torch.randint(-32, 33, shape, generator=g).double() / 8


# ------------------------------------------------------------------------------------------------ float64 references
def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _op(L, x_nchw, w):
    if L.transposed:
        return F.conv_transpose2d(x_nchw, w, None, L.stride, L.pad)
    return F.conv2d(x_nchw, w, None, L.stride, L.pad)


def ref_forward(L, x, w):
    """raw layer output, NHWC float64"""
    out = _op(L, _nchw(x.double()), w.double())
    assert out.shape[2] == L.oh and out.shape[3] == L.oh and out.shape[1] == L.cout, out.shape
    return _nhwc(out)


def ref_colstats(out, groups):
    """[groups][cout][2]: (sum v, sum v^2) per BatchNorm group (a group = nimg / groups consecutive images)"""
    o = out.reshape(groups, -1, out.shape[-1])
    return torch.stack([o.sum(1), (o * o).sum(1)], -1)


def ref_wgrad(L, x, dy):
    """gradient of sum(out * dy) w.r.t. the weight, in the parameter's layout (torch.autograd, float64)"""
    w = torch.zeros(weight_shape(L), dtype=torch.float64, requires_grad=True)
    _op(L, _nchw(x.double()), w).backward(_nchw(dy.double()))
    return w.grad


def ref_dgrad_acc(L, dy, w):
    """gradient of sum(out * dy) w.r.t. the layer input, NHWC float64: the accumulator in front of the engine's epilogue"""
    x = torch.zeros((dy.shape[0], L.cin, L.ih, L.ih), dtype=torch.float64, requires_grad=True)
    _op(L, x, w.double()).backward(_nchw(dy.double()))
    return _nhwc(x.grad)


def dswish(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def ref_dgrad_epilogue(acc, r, aff, mr, groups):
    """csrc/gemm.h GemmParams, d-activation epilogue, in float64:  v = acc * Swish'(scale * r + shift);
    d_red += (sum v, sum v * xhat) with xhat = (r - mean) * rstd, summed per group and channel over the fp32 v (both kernels take
    the sums BEFORE the bf16 store: gemm_epi.h gemm_epilogue, convres_epi.h cr_epilogue_tile).
    acc, r: [nimg][h][w][C]; aff, mr: [groups][C][2] or None (identity / no sums).
    -> v, red [groups][C][2] or None, red_abs [groups][C][2] (sum of |terms|, what the gate scales with)"""
    C = acc.shape[-1]
    a = acc.double().reshape(groups, -1, C)
    rr = r.double().reshape(groups, -1, C)
    pre = rr if aff is None else rr * aff[:, None, :, 0] + aff[:, None, :, 1]
    v = a * dswish(pre)
    red = red_abs = None
    if mr is not None:
        t2 = v * ((rr - mr[:, None, :, 0]) * mr[:, None, :, 1])
        red = torch.stack([v.sum(1), t2.sum(1)], -1)
        red_abs = torch.stack([v.abs().sum(1), t2.abs().sum(1)], -1)
    return v.reshape(acc.shape), red, red_abs


def assert_exact_regime(out=None, dw=None, groups=1, what=""):
    """the conditions under which bf16 operands with fp32 accumulation give the float64 result bit for bit"""
    if out is not None:
        assert bool((out == out.round()).all()), what + ": non-integer output"
        assert float(out.abs().max()) <= 256, (what, float(out.abs().max()))
        ssq = ref_colstats(out, groups)[..., 1]
        assert float(ssq.max()) < 2 ** 24, (what, float(ssq.max()))
    if dw is not None:
        assert bool((dw == dw.round()).all()), what + ": non-integer weight gradient"
        assert float(dw.abs().max()) < 2 ** 24, (what, float(dw.abs().max()))


def assert_operand_coverage(ws, xs):
    """What 'over the seeds every weight position and every input pixel was nonzero at least once' means here: every tap (ky, kx)
    carries a nonzero weight for every input channel and for every output channel, and every pixel of every image a nonzero channel.
    Element by element a density of 1/4 cannot cover a weight tensor in two draws (9/16 of the elements stay zero); every single
    weight ELEMENT is reached by the weight-gradient comparison, whose result is dense, and by the one-hot packing test, whose
    weights are dense and distinct."""
    wnz = torch.stack([w != 0 for w in ws]).any(0)
    assert bool(wnz.any(0).all()) and bool(wnz.any(1).all()), "a (channel, tap) slice of the weights was zero in every seed"
    xnz = torch.stack([(x != 0).any(-1) for x in xs]).any(0)
    assert bool(xnz.all()), "an input pixel was zero in every channel in every seed"


def describe_mismatch(got, ref, limit=6):
    """first few indices and per-image counts of the elements that differ (got, ref: [nimg][h][w][C])"""
    bad = got.double().cpu() != ref.double().cpu()
    idx = torch.nonzero(bad)
    per_img = bad.reshape(bad.shape[0], -1).sum(1)
    imgs = torch.nonzero(per_img).reshape(-1)
    return "%d of %d elements differ; first [image, y, x, channel]: %s (got %s, want %s); images affected %d of %d, first %s, counts %s" % (
        int(bad.sum()), bad.numel(), idx[:limit].tolist(), got.double().cpu()[bad][:limit].tolist(), ref.double().cpu()[bad][:limit].tolist(),
        imgs.numel(), bad.shape[0], imgs[:limit].tolist(), per_img[imgs[:limit]].tolist())


# ------------------------------------------------------------------------------------------------ GPU harness
# the library's defaults of the knobs the tests set, restored after every test: csrc/convres.hip try_launch_convres ("convres" 1,
# "convres_alt" 0), csrc/wgrad_ring.hip try_launch_wgrad_ring ("wgrad_ring" 1), try_wr ("wr_pair" 0, "wr_atomic_kb" 256) -- a changed
# default there must be changed here (and in tests/test_gpu_wgrad_ring.py)
KNOB_DEFAULTS = {"convres": 1, "convres_alt": 0, "wgrad_ring": 1, "wr_atomic_kb": 256, "wr_pair": 0}
RECORDS = []        # (B, layer, knobs, [(tag, kernel)]) of every launch a harness made in this process: what the coverage test reads


class LayerHarness:
    """One MultiMNIST plan at batch B with a bound workspace (one ordinary step has run), whose layers the tests replay one at a
    time on operands of their own."""

    def __init__(self, B):
        import multimodal_vae_amd  # noqa: F401
        from multimodal_vae_amd._lib import call
        from multimodal_vae_amd.core import FusedELBOStep, MultimnistState
        from multimodal_vae_amd.init import default_init_
        from bench import synthetic_batch
        self.call = call
        self.B = B
        self.dev = torch.device("cuda:0")
        self.st = MultimnistState(100, self.dev)
        default_init_(self.st, 1234)
        img, txt = synthetic_batch(B, 1234)
        self.eng = FusedELBOStep(self.st, B)
        self.eng(img.to(self.dev), txt.to(self.dev))
        self.st.ensure_packed()
        torch.cuda.synchronize()
        self.sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.offsets = {}
        for n in WS_NAMES:
            off = call("mmvae_mm_debug_offset", self.eng.h, n.encode())
            assert off >= 0, "mmvae_mm_debug_offset does not know '%s'" % n
            self.offsets[n] = int(off)
        self._sorted = sorted(set(self.offsets.values())) + [self.eng.ws.numel()]
        self.gmap = self.st.grad_map().long()

    # ---- workspace
    def buf(self, name, numel, dtype):
        """view of `numel` elements of the named buffer; refuses an extent that reaches the next named buffer or the workspace end"""
        off = self.offsets[name]
        nbytes = numel * torch.empty((), dtype=dtype).element_size()
        limit = next(o for o in self._sorted if o > off)
        assert 0 <= off and off + nbytes <= limit <= self.eng.ws.numel(), (name, off, nbytes, limit)
        return self.eng.ws[off:off + nbytes].view(dtype)

    def put(self, name, t, dtype=torch.bfloat16):
        """writes tensor t (any shape) at the start of the named buffer; bf16 values must survive the conversion exactly"""
        src = t.to(dtype).contiguous()
        assert torch.equal(src.double(), t.double()), name + ": operand is not exact in " + str(dtype)
        self.buf(name, src.numel(), dtype).copy_(src.reshape(-1).to(self.dev))

    def zero(self, name, numel, dtype):
        self.buf(name, numel, dtype).zero_()

    def get(self, name, shape, dtype=torch.bfloat16):
        n = 1
        for s in shape:
            n *= s
        return self.buf(name, n, dtype).clone().reshape(shape)

    def stats(self, name, groups, C):
        """[groups][C][2] float64: a [groups][STAT_SLOTS][C] float2 table summed over its slots (each slot sum is an fp32 integer
        below 2^24 in the exact regime, so is their float64 sum)"""
        return self.buf(name, groups * STAT_SLOTS * C * 2, torch.float32).reshape(groups, STAT_SLOTS, C, 2).double().sum(1).cpu()

    # ---- weights
    def param_range(self, pname):
        for n, shape, off in self.st.table:
            if n == pname:
                numel = 1
                for s in shape:
                    numel *= s
                return off, numel, shape
        raise KeyError(pname)

    def set_weight(self, pname, w):
        """integer-valued weights into the flat fp32 parameters, then every packed form is rebuilt from them"""
        off, numel, shape = self.param_range(pname)
        assert tuple(w.shape) == tuple(shape), (pname, tuple(w.shape), shape)
        self.st.params[off:off + numel] = w.reshape(-1).float().to(self.dev)
        self.st.pack_weights()

    def packed_grad(self, pname):
        """(gradient of the parameter read through mmvae_mm_grad_map, max |gpk| over the elements the map gives to OTHER parameters)"""
        off, numel, shape = self.param_range(pname)
        m = self.gmap[off:off + numel]
        assert bool((m >= 0).all()), pname + ": not every element has a slot in the packed matrix gradient"
        assert int(m.unique().numel()) == numel, pname + ": two elements share a slot"
        gpk = self.st.gpk
        others = torch.cat([self.gmap[:off], self.gmap[off + numel:]])
        others = others[others >= 0]
        return gpk[m].reshape(shape).cpu(), float(gpk[others].abs().max())

    # ---- launch
    def set_knobs(self, **kn):
        for k, v in kn.items():
            self.call("mmvae_debug_set", k.encode(), int(v))

    def restore_knobs(self):
        self.set_knobs(**KNOB_DEFAULTS)

    def run(self, layer, **knobs):
        """one launch of the layer exactly as the step makes it; the kernels it ran are recorded (mmvae_debug_probe)"""
        self.set_knobs(**knobs)
        self.call("mmvae_debug_probe", 1)
        try:
            self.call("mmvae_mm_bench_layer", self.eng.h, self.eng.ws.data_ptr(), self.eng.ws.numel(), layer.encode(), 1, self.sp)
        finally:
            self.call("mmvae_debug_probe", 0)
        cap = 1 << 16
        text = ctypes.create_string_buffer(cap)
        self.call("mmvae_debug_probe_read", text, cap)
        torch.cuda.synchronize()
        launches = []
        for line in text.value.decode().splitlines():
            f = line.split("\t")
            launches.append((f[0], f[1]))
        RECORDS.append((self.B, layer, dict(knobs), launches))
        return launches
