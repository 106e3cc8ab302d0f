"""Layer-level reference and GPU harness of the MultiMNIST, CelebA and COCO conv / transposed-conv kernels (tests/test_gpu_layers.py,
tests/test_gpu_celeba_layers.py, tests/test_gpu_coco_layers.py, tests/test_cpu_layer_ref.py).

One layer of the step is replayed through mmvae_<family>_bench_layer on operands the test wrote itself and compared with a float64
reference made here with torch.nn.functional.conv2d / conv_transpose2d and torch.autograd -- never with another engine kernel.
Operands are ternary {-1, 0, +1}: bf16 holds them exactly, every product is an integer and every fp32 partial sum stays below
2^24, so the result depends neither on the accumulation order nor on the rounding of the bf16 store and the comparison is
torch.equal.  The float epilogue of the data-gradient layers (Swish' and the BatchNorm-backward sums, csrc/gemm.h GemmParams
d_r / d_affine / d_meanrstd / d_red) is restated in float64 and gated by the precision of the formats alone.

The top half of this module needs no GPU (geometry table, operand generator, references); LayerHarness needs the MI355X."""
import ctypes
import os
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

# CelebA: celeba/model.py:101-150 as restated in csrc/celeba.hip build() -- 64x64 images, encoder 32 -> 64 (32x32 -> 16x16),
# 64 -> 128 (16 -> 8), 128 -> 256 (k4 s1 p0, 8 -> 5); decoder 256 -> 128 (k4 s1 p0, 5 -> 8), 128 -> 64 (8 -> 16), 64 -> 32 (16 -> 32).
# The replayed decoder layers run 3 BatchNorm groups forward and backward (the default step: every image term has a gradient).
# Activation densities: the stride-1 transposed layer sums up to 16 taps x 256 channels into one output pixel (every other layer
# at most 4 x 128 / 16 x 128 with stride 2 / forward form) and the 32x32 output of hallucinate.6 holds 262144 elements per channel
# and group at B = 256: both take density 1/4 (tests/test_cpu_layer_ref.py asserts the regime for every batch and seed used).
BATCHES_CELEBA = (3, 4, 6, 8, 256)
LAYERS_CELEBA = {
    "enc_conv2": Layer("image_encoder.features.2.weight", False, 32, 64, 4, 2, 1, 32, 16, 1, 1,
                       "a1", "r2", "st_e0", "d2e", "d1e", "r1", None, None, None, 0.5),
    "enc_conv3": Layer("image_encoder.features.5.weight", False, 64, 128, 4, 2, 1, 16, 8, 1, 1,
                       "a2", "r3", "st_e1", "d3e", "d2e", "r2", "aff_e0", "mr_e0", "red_e0", 0.5),
    "enc_conv4": Layer("image_encoder.features.8.weight", False, 128, 256, 4, 1, 0, 8, 5, 1, 1,
                       "a3", "r4", "st_e2", "dr4", "d3e", "r3", "aff_e1", "mr_e1", "red_e1", 0.5),
    "dec_convT1": Layer("image_decoder.hallucinate.0.weight", True, 256, 128, 4, 1, 0, 5, 8, 3, 3,
                        "au", "q1", "st_d0", "d1", "du", "u", None, None, None, 0.25),
    "dec_convT2": Layer("image_decoder.hallucinate.3.weight", True, 128, 64, 4, 2, 1, 8, 16, 3, 3,
                        "aq1", "q2", "st_d1", "d2", "d1", "q1", "aff_d0", "mr_d0", "red_d0", 0.5),
    "dec_convT3": Layer("image_decoder.hallucinate.6.weight", True, 64, 32, 4, 2, 1, 16, 32, 3, 3,
                        "aq2", "q3", "st_d2", "d3", "d2", "q2", "aff_d1", "mr_d1", "red_d1", 0.25),
}
# every workspace name mmvae_celeba_debug_offset knows (csrc/celeba.hip)
WS_NAMES_CELEBA = ("patches1 r1 r2 r3 r4 a1 a2 a3 a4 y1 ay1 encout m1 z_bf z_f32 u au q1 q2 q3 aq1 aq2 aq3 dlogit patches4 d3 d2 d1 du "
                   "dz_img dz_att d_encout dy1 db4 dr4 d3e d2e d1e tmp_f32 slab st_e0 st_e1 st_e2 st_d0 st_d1 st_d2 red_e0 red_e1 red_e2 "
                   "red_d0 red_d1 red_d2 aff_e0 aff_e1 aff_e2 aff_d0 aff_d1 aff_d2 mr_e0 mr_e1 mr_e2 mr_d0 mr_d1 mr_d2").split()

# COCO: coco/model.py:157-208 as restated in csrc/coco.hip build() -- 32x32 images, every conv k4 s2 p1: encoder 64 -> 128 (16x16 -> 8x8),
# 128 -> 256 (8 -> 4), 256 -> 512 (4 -> 2); decoder 512 -> 256 (2 -> 4), 256 -> 128 (4 -> 8), 128 -> 64 (8 -> 16).  Buffer names: csrc/coco.hip
# layer_gemm / layer_wgrad.  The encoder runs 1 BatchNorm group, the replayed decoder 3 forward and backward (the default step).
# Activation density 1/2 everywhere: the longest sum is 9 valid taps x 256 channels (features.8 on the 4x4 map, and the data
# gradient of hallucinate.0) with variance 2304 / 8 = 288, and the largest sum of squares of a channel and group is that of
# hallucinate.6 at B = 256, 65536 elements of variance 64 = 4.2e6 < 2^24 (tests/test_cpu_layer_ref.py asserts the regime for every
# batch and seed used).
# Batches: derived in the docstring of tests/test_gpu_coco_layers.py.
BATCHES_COCO = (3, 4, 6, 8, 128, 256)
LAYERS_COCO = {
    "enc_conv2": Layer("image_encoder.features.2.weight", False, 64, 128, 4, 2, 1, 16, 8, 1, 1,
                       "a1", "r2", "st_e0", "d2e", "d1e", "r1", None, None, None, 0.5),
    "enc_conv3": Layer("image_encoder.features.5.weight", False, 128, 256, 4, 2, 1, 8, 4, 1, 1,
                       "a2", "r3", "st_e1", "d3e", "d2e", "r2", "aff_e0", "mr_e0", "red_e0", 0.5),
    "enc_conv4": Layer("image_encoder.features.8.weight", False, 256, 512, 4, 2, 1, 4, 2, 1, 1,
                       "a3", "r4", "st_e2", "dr4", "d3e", "r3", "aff_e1", "mr_e1", "red_e1", 0.5),
    "dec_convT1": Layer("image_decoder.hallucinate.0.weight", True, 512, 256, 4, 2, 1, 2, 4, 3, 3,
                        "au", "q1", "st_d0", "d1", "du", "u", None, None, None, 0.5),
    "dec_convT2": Layer("image_decoder.hallucinate.3.weight", True, 256, 128, 4, 2, 1, 4, 8, 3, 3,
                        "aq1", "q2", "st_d1", "d2", "d1", "q1", "aff_d0", "mr_d0", "red_d0", 0.5),
    "dec_convT3": Layer("image_decoder.hallucinate.6.weight", True, 128, 64, 4, 2, 1, 8, 16, 3, 3,
                        "aq2", "q3", "st_d2", "d3", "d2", "q2", "aff_d1", "mr_d1", "red_d1", 0.5),
}
# every workspace name mmvae_coco_debug_offset knows (csrc/coco.hip)
WS_NAMES_COCO = ("patches1 r1 r2 r3 r4 a1 a2 a3 a4 y1 ay1 y2 ay2 encout m1 m2 z_bf z_f32 u au q1 q2 q3 aq1 aq2 aq3 dlogit patches4 d3 d2 d1 "
                 "du dz_img d_encout dy2 dy1 db4 dr4 d3e d2e d1e tmp_f32 slab sums st_e0 st_e1 st_e2 st_d0 st_d1 st_d2 red_e0 red_e1 red_e2 "
                 "red_d0 red_d1 red_d2 aff_e0 aff_e1 aff_e2 aff_d0 aff_d1 aff_d2 mr_e0 mr_e1 mr_e2 mr_d0 mr_d1 mr_d2").split()
LOSS_SLOTS = 32                 # MMVAE_LOSS_SLOTS (csrc/common.h): the loss sums are [LOSS_SLOTS][16] floats, column g of every slot row

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


def layer_operands(name, nimg, seed, layers=None):
    """(x [nimg][ih][ih][cin], w in the parameter's layout, dy [nimg][oh][oh][cout]) -- one draw per (layer, seed); the images of a
    smaller batch are a prefix of a larger one's only by accident, nothing relies on it.  layers: the family's table (LAYERS)."""
    layers = LAYERS if layers is None else layers
    L = layers[name]
    idx = list(layers).index(name)
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
# (B, layer, knobs, [(tag, kernel)]) of every launch a harness of the family made in this process: what its coverage test reads
RECORDS = []
RECORDS_CELEBA = []
RECORDS_COCO = []


class LayerHarness:
    """One plan of a model family at batch B with a bound workspace (one ordinary step has run: the workspace is bound and the
    weights are packed), whose layers the tests replay one at a time on operands of their own.
    state_cls / engine_cls: the family's classes of multimodal_vae_amd.core (default: MultiMNIST); prefix: its mmvae_<prefix>_*
    entry points; ws_names: every name its debug_offset knows; workload: the family's synthetic batch of bench.py; records: the
    family's list of compared launches; n_latents: the latent size the plan is built at (the conv layers do not depend on it, the
    dense layers around the latent do); engine_args: what the engine's constructor takes behind (state, batch) -- COCO's sos."""

    def __init__(self, B, state_cls=None, engine_cls=None, prefix="mm", ws_names=None, workload="multimnist", records=None,
                 n_latents=100, engine_args=()):
        import multimodal_vae_amd  # noqa: F401
        from multimodal_vae_amd._lib import call
        from multimodal_vae_amd import core
        from multimodal_vae_amd.init import default_init_
        from bench import synthetic_batch_for
        self.call = call
        self.B = B
        self.n_latents = n_latents
        self.prefix = prefix
        self.records = RECORDS if records is None else records
        self.dev = torch.device("cuda:0")
        self.st = (state_cls or core.MultimnistState)(n_latents, self.dev)
        default_init_(self.st, 1234)
        a, b = synthetic_batch_for(workload, B, 1234)
        self.eng = (engine_cls or core.FusedELBOStep)(self.st, B, *engine_args)
        self.eng(a.to(self.dev), b.to(self.dev))
        self.st.ensure_packed()
        torch.cuda.synchronize()
        self.sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.offsets = {}
        for n in (WS_NAMES if ws_names is None else ws_names):
            off = call("mmvae_%s_debug_offset" % prefix, self.eng.h, n.encode())
            assert off >= 0, "mmvae_%s_debug_offset does not know '%s'" % (prefix, n)
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

    def packed_grad(self, pname, also=()):
        """(gradient of the parameter read through mmvae_<family>_grad_map, max |gpk| over the elements the map gives to OTHER
        parameters).  also: parameters whose packed gradient the same launch writes too (a bias folded into the packed weights)."""
        off, numel, shape = self.param_range(pname)
        m = self.gmap[off:off + numel]
        assert bool((m >= 0).all()), pname + ": not every element has a slot in the packed matrix gradient"
        assert int(m.unique().numel()) == numel, pname + ": two elements share a slot"
        gpk = self.st.gpk
        mine = torch.zeros(self.gmap.numel(), dtype=torch.bool, device=self.gmap.device)
        for n in (pname,) + tuple(also):
            o, k, _ = self.param_range(n)
            mine[o:o + k] = True
        others = self.gmap[~mine]
        others = others[others >= 0]
        return gpk[m].reshape(shape).cpu(), float(gpk[others].abs().max())

    # ---- launch
    def run(self, layer, **knobs):
        """one launch of the layer exactly as the step makes it, under the given library knobs (every other knob, and these behind
        the launch, at the default of csrc/knobs.h); the kernels it ran are recorded (mmvae_debug_probe)"""
        from multimodal_vae_amd._lib import knobs as lib_knobs
        self.call("mmvae_debug_probe", 1)
        try:
            with lib_knobs(**knobs):
                self.call("mmvae_%s_bench_layer" % self.prefix, self.eng.h, self.eng.ws.data_ptr(), self.eng.ws.numel(), layer.encode(), 1, self.sp)
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
        self.records.append((self.B, layer, dict(knobs), launches))
        return launches


# ------------------------------------------------------------------------------------------------ comparisons
# The checks of tests/test_gpu_celeba_layers.py (the same tiers and gates as tests/test_gpu_layers.py, whose docstring derives
# them), with the layer's table entry passed in.
REPORT = os.environ.get("MMVAE_TOL_REPORT") is not None       # print the worst error / gate ratio of every gated check


def check_forward(h, L, name, x, w, knob_sets, what):
    """Tier A: raw output and column statistics of a forward layer, torch.equal"""
    ref = ref_forward(L, x, w)
    assert_exact_regime(out=ref, groups=L.gf, what=what)
    ref_st = ref_colstats(ref, L.gf)
    h.set_weight(L.param, w)
    h.put(L.x, x)
    for knobs in knob_sets:
        h.zero(L.out, ref.numel(), torch.bfloat16)
        h.zero(L.stats, L.gf * STAT_SLOTS * L.cout * 2, torch.float32)
        launches = h.run(name, **knobs)
        got = h.get(L.out, ref.shape).double().cpu()
        assert torch.equal(got, ref), (what, knobs, launches, describe_mismatch(got, ref))
        st = h.stats(L.stats, L.gf, L.cout)
        assert torch.equal(st, ref_st), (what, knobs, launches, "column statistics: %d of %d differ, first [group, channel, 0 sum / 1 sum^2] %s"
                                         % (int((st != ref_st).sum()), st.numel(), torch.nonzero(st != ref_st)[:6].tolist()))


def check_wgrad(h, layer, pname, dw, knob_sets, what, also=()):
    """Tier A: the packed weight gradient of one parameter, exact, and nothing written into another parameter's slots.
    also: {parameter: its exact gradient} the same launch produces (a bias folded into the packed weights)"""
    also = dict(also)
    assert_exact_regime(dw=dw, what=what)
    assert float(dw.abs().max()) > 0
    for knobs in knob_sets:
        h.st.gpk.zero_()
        launches = h.run(layer, **knobs)
        for pn, want in [(pname, dw)] + list(also.items()):
            got, others = h.packed_grad(pn, [n for n in [pname] + list(also) if n != pn])
            bad = got.double() != want
            assert not bool(bad.any()), (what, pn, knobs, launches, "%d of %d elements differ, first %s: got %s want %s" % (
                int(bad.sum()), bad.numel(), torch.nonzero(bad)[:6].tolist(), got[bad][:6].tolist(), want[bad][:6].tolist()))
            assert others == 0.0, (what, knobs, "another parameter's packed gradient was written", others)


def gate_elements(got, ref, acc, what, extra=""):
    """Tier B: |got - ref| <= 2^-8 |ref| + 1e-5 |acc| per element"""
    got, gate = got.double().cpu(), 2.0 ** -8 * ref.abs() + 1e-5 * acc.abs()
    err = (got - ref).abs()
    bad = ~(err <= gate)
    if REPORT:
        print("TIERB %s: worst err/gate %.3f" % (what, float((err / gate.clamp_min(1e-30)).max())))
    assert not bool(bad.any()), (what, extra, "%d of %d outside the gate; first %s got %s want %s acc %s; rows affected %d" % (
        int(bad.sum()), bad.numel(), torch.nonzero(bad)[:6].tolist(), got[bad][:6].tolist(), ref[bad][:6].tolist(), acc[bad][:6].tolist(),
        int(bad.reshape(bad.shape[0], -1).any(1).sum())))


def gate_sums(got, ref, mag, what, extra=""):
    """Tier B: a sum of fp32 terms, |got - ref| <= 2^-16 sum |terms|"""
    err, gate = (got.double().cpu() - ref).abs(), 2.0 ** -16 * mag
    if REPORT:
        print("TIERB %s: sums worst err/gate %.3f" % (what, float((err / gate.clamp_min(1e-30)).max())))
    assert bool((err <= gate).all()), (what, extra, "first %s got %s want %s" % (
        torch.nonzero(err > gate)[:6].tolist(), got.double().cpu()[err > gate][:6].tolist(), ref[err > gate][:6].tolist()))


def check_exact(got, ref, what, limit=256):
    """Tier A on a dense layer: integer reference of magnitude <= limit (256: exact in bf16; 2^24: in fp32)"""
    got = got.double().cpu()
    assert bool((ref == ref.round()).all()) and float(ref.abs().max()) <= limit, (what, float(ref.abs().max()))
    bad = got != ref
    assert not bool(bad.any()), (what, "%d of %d elements differ; first %s got %s want %s; rows affected %d" % (
        int(bad.sum()), bad.numel(), torch.nonzero(bad)[:6].tolist(), got[bad][:6].tolist(), ref[bad][:6].tolist(),
        int(bad.reshape(bad.shape[0], -1).any(1).sum())))


def check_dgrad(h, L, name, dy, w, g, knob_sets, what):
    """Tier B: data gradient of a conv layer with the Swish' / BatchNorm-backward epilogue of the layer below; g: generator of the
    saved raw tensor and the tables"""
    acc = ref_dgrad_acc(L, dy, w)
    assert bool((acc == acc.round()).all()) and float(acc.abs().max()) <= 256, what
    r = eighths(acc.shape, g)
    aff, mr = dyadic_tables(L.gb, L.cin, g) if L.aff else (None, None)
    v, red, red_abs = ref_dgrad_epilogue(acc, r, aff, mr, L.gb)
    h.set_weight(L.param, w)
    h.put(L.dy, dy)
    h.put(L.r, r)
    if L.aff:
        h.put(L.aff, aff, torch.float32)
        h.put(L.mr, mr, torch.float32)
    for knobs in knob_sets:
        h.zero(L.dx, acc.numel(), torch.bfloat16)
        if L.red:
            h.zero(L.red, L.gb * STAT_SLOTS * L.cin * 2, torch.float32)
        launches = h.run(name + "_dgrad", **knobs)
        gate_elements(h.get(L.dx, acc.shape), v, acc, "%s %s" % (what, knobs), launches)
        if L.red:
            gate_sums(h.stats(L.red, L.gb, L.cin), red, red_abs, "%s %s d_red" % (what, knobs), launches)


# ------------------------------------------------------------------------------------------------ staged forms (fused step)
# csrc/gemm.h GatherTransform, csrc/convres.hip: kind 1 stages Swish(BatchNorm(raw)) of the layer's operand from the column
# statistics of the layer below; kind 2 stages the BatchNorm backward of the incoming gradient, in place.
BN_EPS = float(torch.tensor(1e-5, dtype=torch.float32))       # csrc/plan_base.h BN_EPS as the fp32 value the kernel adds
EPS32 = 2.0 ** -24                                            # one rounding of an fp32 operation, relative


def slot_stats(r, groups):
    """[groups][STAT_SLOTS][C][2] float64: (sum v, sum v^2) of r [nimg][h][w][C], the rows of a group dealt to the slots in
    STAT_SLOTS contiguous runs.  For r in eighths of magnitude <= 4 and at most 4096 rows per slot every entry is exact in fp32."""
    C = r.shape[-1]
    o = r.double().reshape(groups, STAT_SLOTS, -1, C)
    return torch.stack([o.sum(2), (o * o).sum(2)], -1)


def ref_bn_tables(stats, count, gamma, beta):
    """csrc/bn_dev.h bn_channel_tables in float64 from the slot table [groups][STAT_SLOTS][C][2] as written (fp32 values):
    -> scale, shift, mean, rstd, each [groups][C]"""
    s = stats.double().sum(1)
    mean = s[..., 0] / count
    var = (s[..., 1] / count - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + BN_EPS)
    scale = gamma.double()[None] * rstd
    return scale, beta.double()[None] - mean * scale, mean, rstd


def ref_stage_fwd(r, scale, shift, groups):
    """kind 1 by-product: Swish(scale * r + shift) per group and channel, float64, shape of r"""
    C = r.shape[-1]
    y = r.double().reshape(groups, -1, C) * scale[:, None] + shift[:, None]
    return (y * torch.sigmoid(y)).reshape(r.shape), y.reshape(r.shape)


def gate_stage_fwd(r, scale, shift, mean, beta, ref, groups):
    """Gate of the kind 1 by-product: one bf16 ulp of the stored value (2^-8 |ref|, either rounding) plus the fp32 error in front
    of the store, 32 roundings each relative to a quantity bounded by T = (|r| + |mean| + 4) |scale| + |beta| + 1:
    15 additions of the slot sums (|r| <= 4: their error reaches the mean by at most 15 eps * 4), 2 divisions by the count,
    3 operations of the variance (mean^2 << variance for the operands used: no cancellation), rsqrt, scale, 2 of the shift,
    2 of the affine, 5 of swish_fast (exponent scaling, exp, 1 +, reciprocal, product) = 31."""
    C = r.shape[-1]
    T = (r.double().abs().reshape(groups, -1, C) + mean.abs()[:, None] + 4) * scale.abs()[:, None] + beta.double().abs()[None, None] + 1
    return 2.0 ** -8 * ref.abs() + 32 * EPS32 * T.reshape(r.shape)


def ref_abs_terms(L, x, w):
    """sum of |terms| of every output element of the layer: the forward of |x| with |w|"""
    return ref_forward(L, x.double().abs(), w.double().abs())


def gate_stage_conv(L, ref, absterms):
    """Gate of a conv output whose operand is not integer-valued (the bf16 by-product): 2^-8 |ref| for the bf16 store plus
    K * 2^-24 * sum |terms| for K fp32 additions, K = taps x input channels of the layer"""
    return 2.0 ** -8 * ref.abs() + L.k * L.k * L.cin * EPS32 * absterms


def gate_stage_colstats(L, ref, absterms, groups):
    """Gate of the column statistics of such an output, summed from the fp32 accumulators BEFORE the store (convres_epi.h):
    per element e = K * 2^-24 * sum |terms|; sum v: sum e + 2^-16 sum |v|; sum v^2: sum (2 |v| e + e^2) + 2^-16 sum v^2"""
    C = ref.shape[-1]
    e = (L.k * L.k * L.cin * EPS32 * absterms).reshape(groups, -1, C)
    v = ref.reshape(groups, -1, C)
    return torch.stack([e.sum(1) + 2.0 ** -16 * v.abs().sum(1), (2 * v.abs() * e + e * e).sum(1) + 2.0 ** -16 * (v * v).sum(1)], -1)


def staged_bwd_operands(L, nimg, groups, count, g, integer_slots=True):
    """Operands of a kind 2 launch on which every coefficient and every dr = g db + cb r + c2 (csrc/convres.hip) lies on the
    2^-7 grid below 64: exact in fp32, so the in-place bf16 store is the only rounding of dr and the data gradient's fp32
    accumulation of the stored values (multiples of 2^-8: rounding to 8 bits only coarsens the grid) is exact again.
    -> db ternary, r eighths [nimg][oh][oh][cout]; red [groups][STAT_SLOTS][cout][2] with slot sums count * m1, count * m2
    (m1, m2 multiples of 1/4, spread unevenly over the slots); mr [groups][cout][2] dyadic; gamma [cout] in {1, 2, -1}
    integer_slots=False (the small COCO maps, count = 12 .. 48): the slot values are multiples of count / 64 instead of integers --
    dyadic and of magnitude <= count, so still exact in fp32 (the caller asserts it)"""
    C = L.cout
    db = ternary((nimg, L.oh, L.oh, C), G_DENSITY, g)
    r = eighths((nimg, L.oh, L.oh, C), g)
    pick = lambda vals, shape: torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), shape, generator=g)]
    m = pick([-1.0, -0.5, -0.25, 0.0, 0.25, 0.5, 1.0], (groups, C, 2))
    assert count % 64 == 0 or not integer_slots, count            # every slot value count * (multiple of 1/64) is an integer
    delta = torch.tensor([1.0, -1.0] * (STAT_SLOTS // 2), dtype=torch.float64)[None, :, None, None] / 64
    red = count * (m[:, None] / STAT_SLOTS + delta * torch.ones(groups, STAT_SLOTS, C, 2, dtype=torch.float64))
    mr = torch.stack([pick([-0.25, 0.0, 0.5], (groups, C)), pick([0.5, 1.0, 2.0], (groups, C))], -1)
    gamma = pick([1.0, 2.0, -1.0], (C,))
    return db, r, red, mr, gamma


def ref_bn_backward(db, r, red, mr, gamma, count, groups):
    """float64 BatchNorm backward as csrc/convres.hip TR 2 states it:  dr = g (db - m1 - xhat m2), g = gamma rstd, m1 / m2 = the
    group's sums of db / db xhat over the count, xhat = (r - mean) rstd;  dgamma = sum over groups of sum db xhat, dbeta = of sum db
    -> dr (shape of db), dgamma [C], dbeta [C], their sums of |slot values| [C] (what the 2^-16 gate scales with)"""
    C = db.shape[-1]
    s = red.double().sum(1)
    m1, m2 = s[..., 0] / count, s[..., 1] / count
    mean, rstd = mr[..., 0].double(), mr[..., 1].double()
    gg = gamma.double()[None] * rstd
    xhat = (r.double().reshape(groups, -1, C) - mean[:, None]) * rstd[:, None]
    dr = gg[:, None] * (db.double().reshape(groups, -1, C) - m1[:, None] - xhat * m2[:, None])
    mag = red.double().abs().sum((0, 1))
    return dr.reshape(db.shape), s[..., 1].sum(0), s[..., 0].sum(0), mag[..., 1], mag[..., 0]


def celeba_harness(B):
    """LayerHarness of the CelebA plan (csrc/celeba.hip celeba_bench_layer / celeba_debug_offset)"""
    from multimodal_vae_amd.core import CelebaState, FusedCelebaStep
    return LayerHarness(B, CelebaState, FusedCelebaStep, "celeba", WS_NAMES_CELEBA, "celeba", RECORDS_CELEBA)


# ------------------------------------------------------------------------------------------------ COCO (tests/test_gpu_coco_layers.py)
def coco_harness(B, n_latents=100):
    """LayerHarness of the COCO plan (csrc/coco.hip coco_bench_layer / coco_debug_offset); default caption length: the one warm-up
    step costs milliseconds"""
    from multimodal_vae_amd.core import CocoState, FusedCocoStep
    from bench import synthetic_sos
    return LayerHarness(B, CocoState, FusedCocoStep, "coco", WS_NAMES_COCO, "coco", RECORDS_COCO, n_latents, (synthetic_sos(),))


def patches_k4s2(img):
    """im2col of [n][3][H][H] for a 4x4 / stride 2 / padding 1 window: [n * (H/2)^2][48], column (ky * 4 + kx) * 3 + channel
    (csrc/elementwise.hip im2col_small_kernel; torch's unfold has the channel slowest), zeros where the window leaves the image"""
    n, H = img.shape[0], img.shape[-1]
    pix = (H // 2) ** 2
    u = F.unfold(img, 4, padding=1, stride=2).reshape(n, 3, 16, pix)
    return u.permute(0, 3, 2, 1).reshape(n * pix, 48).contiguous()


def slot_stats_any(r, groups):
    """slot_stats for any row count: the rows of a group dealt to the STAT_SLOTS slots in contiguous runs of near-equal length
    (empty slots hold zeros).  Exact in fp32 under the same condition (eighths, at most 4096 rows per slot)."""
    C = r.shape[-1]
    o = r.double().reshape(groups, -1, C)
    out = torch.zeros(groups, STAT_SLOTS, C, 2, dtype=torch.float64)
    for q, part in enumerate(torch.tensor_split(o, STAT_SLOTS, dim=1)):
        out[:, q, :, 0], out[:, q, :, 1] = part.sum(1), (part * part).sum(1)
    return out


BN_MOM32 = torch.tensor(0.1, dtype=torch.float32)           # csrc/plan_base.h BN_MOM as the fp32 value the kernel multiplies with
BN_KEEP32 = torch.tensor(1.0, dtype=torch.float32) - BN_MOM32  # ... and its (1.f - momentum), rounded once in fp32


def ref_bn_running(stats, count, rm0, rv0, updates):
    """csrc/bn_dev.h bn_running_update in float64: groups in pass order, `updates` momentum steps per group towards the group's
    mean and unbiased variance.  -> running_mean [C], running_var [C], max over groups of the unbiased variance [C]"""
    s = stats.double().sum(1)
    mean = s[..., 0] / count
    var = (s[..., 1] / count - mean * mean).clamp_min(0)
    unb = var * count / (count - 1.0)
    rm, rv = rm0.double().clone(), rv0.double().clone()
    keep, mom = float(BN_KEEP32), float(BN_MOM32)
    for g in range(stats.shape[0]):
        for _ in range(updates):
            rm = keep * rm + mom * mean[g]
            rv = keep * rv + mom * unb[g]
    return rm, rv, unb.max(0).values


def gate_bn_backward(db, r, red, mr, gamma, count, groups, ref):
    """Gate of the stand-alone BatchNorm backward's dr.  When the count is a power of two 1 / count is exact and, on the operands
    of staged_bwd_operands, so is every fp32 operation: one bf16 ulp, 2^-8 |ref| (the gate of the staged form).  Otherwise 1 / count
    is rounded and 8 fp32 roundings (the reciprocal, the two means, the two of xhat, its product with m2, the two subtractions; the
    products with gamma rstd are exact, both powers of two) each relative to at most T = |g| (|db| + |m1| + |xhat m2|) come on top."""
    gate = 2.0 ** -8 * ref.abs()
    if count & (count - 1):
        C = db.shape[-1]
        s = red.double().sum(1)
        m1, m2 = s[..., 0] / count, s[..., 1] / count
        xhat = (r.double().reshape(groups, -1, C) - mr[:, None, :, 0].double()) * mr[:, None, :, 1].double()
        T = (gamma.double()[None] * mr[..., 1].double()).abs()[:, None] * (db.double().abs().reshape(groups, -1, C) + m1.abs()[:, None] + (xhat * m2[:, None]).abs())
        gate = gate + 8 * EPS32 * T.reshape(ref.shape)
    return gate


# Last decoder layer (csrc/thin.hip convt_last_fwd_kernel): ConvTranspose2d(64, 3, 4, 2, 1) on bf16 operands with fp32 accumulation
# (exact on ternary operands), then per logit l:  p = rcp(1 + exp(-l)) on the hardware transcendentals,  dlogit = coef[g] (p - t),
# BCE term -(t max(log p, -100) + (1 - t) max(log(1 - p), -100)).  The gates below are multiples of one fp32 rounding (EPS32 = 2^-24)
# of the result's magnitude, and of 2^-16 sum |terms| for the sums; the multiples are at most 4 times the worst error / unit ratio
# measured against this float64 reference (docstring of tests/test_gpu_coco_layers.py): the reference defines the centre.
LAST_RECON_MULT = 24           # measured 7.65
LAST_DLOGIT_MULT = 24          # measured 6.81
LAST_SUM_MULT = 1.0 / 64       # measured 0.0049
LAST_X_DENSITY, LAST_W_DENSITY = 0.125, 0.125      # logit variance 4 taps x 64 channels / 64 = 4: |l| <= 8 is 4 sigma
LAST_TARGETS = (0.3125, 0.375, 0.625, 0.6875)      # exact in fp32; sigmoid(integer) stays >= 0.04 away from each: p - t does not cancel


def last_layer_coef(B):
    """the fp32 loss weights of the replay: (1, 1/2, 0) / (B * 3072), one fp32 division each"""
    lam = torch.tensor([1.0, 0.5, 0.0], dtype=torch.float32)
    return (lam / torch.tensor(float(B * 3072), dtype=torch.float32)).double()


def ref_dec_last(a3, w9, target, coef):
    """a3 [3B][16][16][64] NHWC, w9 (64, 3, 4, 4), target [B][3][32][32], coef [3] -> float64 logits, recon, dlogit (NCHW
    [3B][3][32][32]), BCE sums [3] and their sums of |terms| [3]"""
    G = 3
    logits = F.conv_transpose2d(_nchw(a3.double()), w9.double(), None, 2, 1)
    p = torch.sigmoid(logits)
    t = target.double().repeat(G, 1, 1, 1)
    dlogit = coef.double().repeat_interleave(logits.shape[0] // G)[:, None, None, None] * (p - t)
    lp = F.logsigmoid(logits).clamp_min(-100.0)
    lq = F.logsigmoid(-logits).clamp_min(-100.0)
    terms = -(t * lp + (1 - t) * lq)
    tg = terms.reshape(G, -1)
    return logits, p, dlogit, tg.sum(1), tg.abs().sum(1)


def assert_last_layer_regime(logits):
    """integer logits, at least 90 % of them in |l| <= 8 (where a logit off by 1 moves the sigmoid by more than 3e-4) and none
    beyond 14: there fp32 still resolves 1 - p = 8e-7 to 3 bits and neither BCE log reaches its clamp"""
    assert bool((logits == logits.round()).all())
    assert float((logits.abs() <= 8).double().mean()) >= 0.9, float((logits.abs() <= 8).double().mean())
    assert float(logits.abs().max()) <= 14, float(logits.abs().max())


def gate_last_layer(got, ref, mult, what, extra=""):
    """|got - ref| <= mult * 2^-24 * |ref| per element"""
    got = got.double().cpu()
    err, unit = (got - ref).abs(), EPS32 * ref.abs()
    if REPORT:
        nz = unit > 0
        print("LAST %s: worst err/(2^-24 |ref|) %.3f (gate %g)" % (what, float((err[nz] / unit[nz]).max()) if bool(nz.any()) else 0.0, mult))
    bad = ~(err <= mult * unit)
    assert not bool(bad.any()), (what, extra, "%d of %d outside the gate; first %s got %s want %s" % (
        int(bad.sum()), bad.numel(), torch.nonzero(bad)[:6].tolist(), got[bad][:6].tolist(), ref[bad][:6].tolist()))


def gate_last_sums(got, ref, mag, what, extra=""):
    """|got - ref| <= LAST_SUM_MULT * 2^-16 sum |terms|"""
    err, unit = (got.double().cpu() - ref).abs(), 2.0 ** -16 * mag
    if REPORT:
        print("LAST %s: sums worst err/(2^-16 sum|terms|) %.4f (gate %g)" % (what, float((err / unit.clamp_min(1e-30)).max()), LAST_SUM_MULT))
    assert bool((err <= LAST_SUM_MULT * unit).all()), (what, extra, got.tolist(), ref.tolist())
