"""GPU tests of the streaming kernels every step runs (csrc/elementwise.hip) on operands of their own, through the entry points that make
exactly the steps' launches: the 3-pass latent block, sigmoid + BCE, log-softmax + NLL, the BatchNorm triple, the embedding gather /
scatter, the column sums and the stand-alone latent / loss ops -- against the float64 references of tests/elementwise_ref.py, whose gate
functions these tests call (tests/test_cpu_elementwise_ref.py proves on the CPU that every gate notices every entry of FAULTS).

Gates (elementwise_ref.py): fp32 elements err / magnitude <= max(4 err32, 2^-22 = 2.38e-7) | bf16 elements 2^-8 = 3.9e-3 of the magnitude,
pads exact | sums through atomics 2 N 2^-24 sum|terms| | rstd 2^-22 (1 + mean^2 / var).  Every output is filled with 7.0 or NaN before the
call; every test prints what it measured (run with -s).  The figures in the docstrings are the worst over a test's cases on an MI355X.

What these tests found, and what was fixed for them (csrc/elementwise.hip):
  * expf under -ffp-contract=fast: the compiler fuses x * log2(e) of expf's range reduction into the subtraction of its rounded integer
    part, so the product's rounding error counts twice: up to |x| log2(e) 2^-24 relative.  The product of experts at logvar -11 .. -17
    measured 5.3e-7 .. 8.0e-7 of the magnitude in latent3_fwd's mu (gate 4 err32 = 4.9e-7 .. 5.2e-7), 6.9e-7 .. 1.2e-6 in mmvae_poe_fwd /
    _bwd (gates 5.1e-7 .. 1.0e-6), while torch's own exp on the same GPU gave 1.8e-7.  The kernels of that file now call exp_unfused
    (the same instructions, the product kept a value of its own); the same outputs then measured 1.3e-7 .. 2.9e-7.
  * logsoftmax_nll formed max + log(sum) first and subtracted it from the logit: at a logit spread of 200 the log-probs near 0 were off
    by 2.1e-6 absolute (the rounding of 100.002; gate 4.5e-7 .. 6.4e-7).  It now computes (logit - max) - log(sum) as torch does: 4.2e-7
    at the same row.
  * launch_bn_bwd_apply had no bound on G * C (its [G][C] float4 table is in LDS), several launchers took null or zero-sized arguments
    to the kernel: now refused with a message (test_wrappers_refuse_what_would_index_out_of_range).
"""
import ctypes
import itertools

import pytest
import torch

import elementwise_ref as E

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _api():
    from multimodal_vae_amd._lib import call, ptr
    from multimodal_vae_amd._ops import stream
    return call, ptr, stream


def _full(dev, shape, fill, dtype=torch.float32):
    return torch.full(shape, fill, dtype=dtype, device=dev)


def _coef(c):
    c = list(c) + [0.0] * (4 - len(c))
    return (ctypes.c_float * 4)(*c)


def _check(tag, recs):
    print("%s: %s" % (tag, E.describe(recs)))
    bad = E.violations(recs)
    assert not bad, (tag, bad)


def _same(a, b):
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


# ====================================================================================================== latent3 forward
def _l3_fwd(dev, inp, B, D, ldz, training, with_b, slots=None):
    call, ptr, stream = _api()
    if with_b:       # pass 1 is read from img_out_b: the second half of img_out must not be
        img = torch.cat((inp["img0"], torch.full((B, 2 * D), float("nan")))).to(dev)
        img_b = inp["img1"].to(dev)
    else:
        img, img_b = torch.cat((inp["img0"], inp["img1"])).to(dev), None
    txt, eps = inp["txt"].to(dev), inp["eps"].to(dev)
    mu, lv, z = (_full(dev, (3, B, D), float("nan")) for _ in range(3))
    zb = _full(dev, (3 * B + 1, ldz), 7.0, BF)                       # one guard row
    slots = _full(dev, (E.LOSS_SLOTS, 16), 0.0) if slots is None else slots
    call("mmvae_latent3_fwd", ptr(img), ptr(img_b), ptr(txt), ptr(eps) if training else None, B, D, int(training), ptr(mu), ptr(lv), ptr(z),
         ptr(zb), ldz, ptr(slots), stream())
    torch.cuda.synchronize()
    assert float(zb[3 * B].float().min()) == 7.0 == float(zb[3 * B].float().max())
    return dict(mu=mu.cpu(), logvar=lv.cpu(), z=z.cpu(), z_bf=zb[:3 * B].cpu(), kl=slots.double().sum(0)[:3].cpu(), slots=slots,
                mu_d=mu, lv_d=lv, z_d=z)


@pytest.mark.parametrize("B,D", E.L3_FWD_CASES + [E.L3_FWD_BIG])
def test_latent3_fwd(B, D):
    """mmvae_latent3_fwd against float64 (gates of the module docstring), with img_out_b null and given, training and eval (z == mu bit
    for bit), pads of z_bf exact in all three passes (column D = 1.0, the rest 0, a guard row untouched), KL sums folded over the 32
    slot rows (the other 13 columns stay exact zeros), "+=" into non-zero slots; the one-expert passes are what the reference says
    (logvar -20 reads -18.2 through the 1e-8), not the input halves.  (600, 100) is past the launcher's cap of 256 workgroups.
    mu / logvar / z against the chain mmvae_poe_fwd + mmvae_reparam_fwd on the same inputs: bit for bit, or, where contraction differs,
    within 2^-22 of the magnitude (printed which).
    Measured (gates in brackets): mu 1.3e-7 (4.9e-7), logvar 1.3e-7 (2.4e-7), z 1.1e-6 at (600, 100) (1.6e-6 = 4 err32), z_bf 3.89e-3
    (3.91e-3), KL sums 4.4e-8 of sum|terms| (4.8e-7 at (1, 1)), "+=" 3.3e-8 (9.5e-6).  Against the chain: equal bits at (1, 1); elsewhere the
    kernels differ by contraction (the templated experts are unrolled, the stand-alone loop is not): 1.8e-8 .. 2.3e-7 of the magnitude,
    under 2^-22 = 2.38e-7, and each side passes the float64 gate on its own (test_standalone_ops)."""
    call, ptr, stream = _api()
    dev = _dev()
    inp, ldz = E.latent3_inputs(B, D), E.ldz_of(D)
    assert all(float(inp[k][:, D:].min()) == -20.0 for k in ("img0", "img1"))
    first = None
    for with_b, training in itertools.product((False, True), (True, False)):
        got = _l3_fwd(dev, inp, B, D, ldz, training, with_b)
        _check("latent3_fwd (B=%d, D=%d, img_out_b=%d, training=%d)" % (B, D, with_b, training), E.gate_latent3_fwd(got, inp, ldz, training))
        assert float(got["slots"][:, 3:].abs().max()) == 0.0
        if training:
            if first is None:
                first = got
            else:                                                       # where pass 1 comes from changes no bit
                assert all(torch.equal(first[k], got[k]) for k in ("mu", "logvar", "z", "z_bf"))
    # "+=": the same call into slots that hold 3.0 everywhere
    r64 = E.latent3_fwd(inp)
    got2 = _l3_fwd(dev, inp, B, D, ldz, True, False, _full(dev, (E.LOSS_SLOTS, 16), 3.0))
    assert float((got2["slots"][:, 3:] - 3.0).abs().max()) == 0.0
    _check("latent3_fwd += (B=%d, D=%d)" % (B, D), [E.rec_sum("kl[%d] += " % k, got2["kl"][k], r64["kl"][k] + 96.0, r64["kl_abs"][k] + 96.0,
                                                              r64["kl_n"] + E.LOSS_SLOTS) for k in range(3)])
    # the chain of stand-alone ops
    n = B * D
    sp = lambda x: (x[:, :D].contiguous(), x[:, D:].contiguous())
    (m0, l0), (m1, l1), (mt, lt) = sp(inp["img0"]), sp(inp["img1"]), sp(inp["txt"])
    experts = [(torch.stack((m0, mt)), torch.stack((l0, lt))), (m1[None], l1[None]), (mt[None], lt[None])]
    worst = 0.0
    for k, (m, l) in enumerate(experts):
        md, ld_ = m.contiguous().to(dev), l.contiguous().to(dev)
        pm, plv, z = (_full(dev, (B, D), float("nan")) for _ in range(3))
        call("mmvae_poe_fwd", ptr(md), ptr(ld_), m.shape[0], n, ptr(pm), ptr(plv), stream())
        eps_k = inp["eps"][k].contiguous().to(dev)
        call("mmvae_reparam_fwd", ptr(pm), ptr(plv), ptr(eps_k), n, ptr(z), stream())
        for name, a in (("mu", pm), ("logvar", plv), ("z", z)):
            b = first[name][k]
            if not torch.equal(a.cpu(), b):
                worst = max(worst, E._err(a.cpu(), b.double(), r64[name + "_mag"][k]))
    print("latent3_fwd (B=%d, D=%d) vs poe_fwd + reparam_fwd: %s" % (B, D, "equal bits" if worst == 0.0 else
                                                                     "worst difference / magnitude %.3e" % worst))
    assert worst <= E.U22, worst


# ====================================================================================================== latent3 backward
def _l3_bwd(dev, inp, mu, lv, B, D, kc, form, training=True, use_a=True, use_b=True, txt="both", bias=True, slots=True, start=0.0,
            with_b=False):
    """one launch -> the dict gate_latent3_bwd takes.  Every output buffer has a guard row (or a guard half) filled with 7.0."""
    call, ptr, stream = _api()
    D2 = 2 * D
    d = {k: inp[k].to(dev) for k in ("txt", "eps", "dz_a", "dz_b")}
    if with_b:       # pass 1 is read from img_out_b: the second half of img_out holds NaN
        img, img_b = torch.cat((inp["img0"], torch.full((B, D2), float("nan")))).to(dev), inp["img1"].to(dev)
    else:
        img, img_b = torch.cat((inp["img0"], inp["img1"])).to(dev), None
    mu_d, lv_d = mu.to(dev), lv.to(dev)
    ldi = E.img_form_ld(form, D)
    LI = ldi or D2
    img_bf = _full(dev, (2 * B + 1, LI), 7.0, BF)
    img_f32 = _full(dev, (B + 1, D2), 7.0) if form == "f32_sum" else None
    t_f32 = _full(dev, (B + 1, D2), 7.0) if txt in ("f32", "both") else None
    t_bf = _full(dev, (B + 1, D2), 7.0, BF) if txt in ("bf", "both") else None
    b_img, b_txt = (_full(dev, (D2 + 1,), start) for _ in range(2)) if bias else (None, None)
    sl = (torch.arange(E.LOSS_SLOTS * 16, dtype=torch.float32, device=dev).view(E.LOSS_SLOTS, 16)).contiguous() if slots else None   # integers: any order of adding is exact
    lo = _full(dev, (16,), float("nan")) if slots else None
    call("mmvae_latent3_bwd", ptr(img), ptr(img_b), ptr(d["txt"]), ptr(mu_d), ptr(lv_d), ptr(d["eps"]) if training else None,
         ptr(d["dz_a"]) if use_a else None, ptr(d["dz_b"]) if use_b else None, B, D, int(training), kc[0], kc[1], kc[2],
         ptr(img_bf), ldi, int(form == "bf16_sum"), ptr(img_f32), ptr(b_img), ptr(t_f32), ptr(t_bf), ptr(b_txt), ptr(sl), ptr(lo), stream())
    torch.cuda.synchronize()
    got = {}
    seven = lambda t: float(t.float().min()) == 7.0 == float(t.float().max())
    if form == "f32_sum":
        got["d_img_f32"] = img_f32[:B].cpu()
        assert seven(img_f32[B:]) and seven(img_bf)                      # a form that is not asked for is not written
    elif form == "bf16_sum":
        got["d_img_bf"] = img_bf[:B].cpu()
        assert seven(img_bf[B:])
    else:
        got["d_img_bf"] = img_bf[:2 * B].cpu()
        assert seven(img_bf[2 * B:])
    if t_f32 is not None:
        got["d_txt"] = t_f32[:B].cpu()
        assert seven(t_f32[B:])
    if t_bf is not None:
        got["d_txt_bf"] = t_bf[:B].cpu()
        assert seven(t_bf[B:])
    if bias:
        got["d_img_bias"], got["d_txt_bias"] = b_img[:D2].cpu(), b_txt[:D2].cpu()
        assert float(b_img[D2]) == start == float(b_txt[D2])
    if slots:
        assert torch.equal(lo, sl.sum(0)), "loss_out != slots.sum(0)"
    return got


@pytest.mark.parametrize("D", E.L3_BWD_D)
@pytest.mark.parametrize("B", E.L3_BWD_B)
def test_latent3_bwd_shapes(B, D):
    """mmvae_latent3_bwd in the MultiMNIST form (two bf16 variants in a padded stride, both text outputs, both bias sums, the loss-slot
    fold) at every B whose row loop ends inside a workgroup and every D around the second column block; operands are the float64
    forward's mu / logvar rounded to fp32.  Pads exact zeros in both variants, guard rows untouched.
    Measured over this test and test_latent3_bwd_options: bf16 outputs 3.85e-3 (3.91e-3), d_txt 1.1e-7 (4.4e-7), d_img_f32 1.2e-7 (4.5e-7),
    bias sums (N = B) 9.6e-8 of sum|terms| at B = 3 (3.6e-7).  At B = 1 a "sum" is the element itself with the element's own rounding:
    the float32 CPU evaluation of the reference measures 1.9e-7 there against 2 B 2^-24 = 1.19e-7 (0.9e-7 .. 1.1e-7 at B = 3 .. 9, inside
    the plain bound), so that one case is floored by the fp32 element gate max(4 err32, 2^-22): kernel 1.3e-7 (image, gate 5.1e-7) and
    1.9e-7 (text, gate 7.5e-7)."""
    dev = _dev()
    inp = E.latent3_inputs(B, D)
    mu, lv = E.fwd_mu_logvar32(inp)
    got = _l3_bwd(dev, inp, mu, lv, B, D, E.KL_COEF, "bf16_two_padded")
    _check("latent3_bwd (B=%d, D=%d)" % (B, D), E.gate_latent3_bwd(got, inp, mu, lv, E.KL_COEF, "bf16_two_padded"))


L3_OPTIONS = [   # text outputs, bias sums, dz_a, dz_b, kl_coef, training, loss slots, start value of the bias sums
    dict(txt="both", bias=True, use_a=True, use_b=True, kc=E.KL_COEF, training=True, slots=True, start=0.0),
    dict(txt="both", bias=True, use_a=True, use_b=True, kc=E.KL_COEF, training=True, slots=True, start=0.0, with_b=True),
    dict(txt="f32", bias=False, use_a=True, use_b=False, kc=(E.KL_COEF[0], 0.0, E.KL_COEF[2]), training=True, slots=False, start=0.0),
    dict(txt="bf", bias=True, use_a=False, use_b=True, kc=E.KL_COEF, training=False, slots=True, start=0.25),
    dict(txt=None, bias=True, use_a=False, use_b=False, kc=(0.0, E.KL_COEF[1], 0.0), training=True, slots=False, start=0.0),
    dict(txt="both", bias=False, use_a=True, use_b=True, kc=E.KL_COEF, training=False, slots=False, start=0.0),
]


@pytest.mark.parametrize("form", E.IMG_FORMS)
def test_latent3_bwd_options(form):
    """Each of the four image-gradient forms of mmvae_latent3_bwd at (B, D) = (5, 65) -- a ragged row block and two column blocks --
    crossed with: the text outputs alone and together and absent, the bias sums present ("+=" into 0 and into 0.25) or null, dz_a / dz_b
    each null and both null, a zero kl_coef, eval mode, img_out_b given (the second half of img_out then holds NaN), loss_slots given (loss_out == slots.sum(0) exactly) or null.  A form that is not
    asked for is not written (the bf16 buffer under the fp32 form, the second half under the summed form)."""
    dev = _dev()
    B, D = E.L3_BWD_CROSS
    inp = E.latent3_inputs(B, D)
    mu, lv = E.fwd_mu_logvar32(inp)
    for o in L3_OPTIONS:
        got = _l3_bwd(dev, inp, mu, lv, B, D, o["kc"], form, o["training"], o["use_a"], o["use_b"], o["txt"], o["bias"], o["slots"], o["start"],
                      o.get("with_b", False))
        _check("latent3_bwd %s %s" % (form, {k: v for k, v in o.items() if k != "kc"}),
               E.gate_latent3_bwd(got, inp, mu, lv, o["kc"], form, o["training"], o["use_a"], o["use_b"], o["start"]))


# ====================================================================================================== sigmoid + BCE
@pytest.mark.parametrize("case", E.BCE_CASES)
@pytest.mark.parametrize("G", [1, 3])
def test_sigmoid_bce(G, case):
    """mmvae_sigmoid_bce: NHWC logits with a channel stride (pad channels hold NaN: never read), NCHW outputs, a zero coef for group 1,
    recon / dlogit each null, "+=" of the loss sums.  Ordinary logits against float64; +-20, +-40, +-100 against torch's float32
    sigmoid + F.binary_cross_entropy and its autograd (a term torch clamps to -100 is 100 here).
    Measured: recon 8.1e-8 (3.3e-7), dlogit 1.5e-7 (5.6e-7), loss sums 1.2e-7 of sum|terms| at the single element (2.4e-7).  The
    log(1 - p) term counts with the magnitude max(|log(1 - p)|, (1 + p) / (1 - p)) (elementwise_ref.py): with the plain magnitude
    max(|log|, 1), torch's own float32 sigmoid + F.binary_cross_entropy on the single element of group 2 at G = 3 (logit 2.80) measures
    2.70e-7 against 2 N 2^-24 = 2.38e-7 (the kernel 3.3e-7): the cancellation of 1 - p is in the reference's arithmetic itself."""
    call, ptr, stream = _api()
    dev = _dev()
    B, C, H, W, ldl = case
    logits, target = E.bce_inputs(G, B, C, H, W, ldl)
    ldev = logits.clone()
    ldev[..., C:] = float("nan")
    ldev, tdev = ldev.to(dev), target.to(dev)
    coef = E.BCE_COEF
    for want_recon, want_dl, start in ((True, True, 0.0), (False, True, 2.0), (True, False, 0.0)):
        recon = _full(dev, (G * B + 1, C, H, W), 7.0) if want_recon else None
        dl = _full(dev, (G * B + 1, C, H, W), 7.0) if want_dl else None
        loss = _full(dev, (G + 1,), start)
        call("mmvae_sigmoid_bce", ptr(ldev), ldl, ptr(tdev), G, B, C, H, W, _coef(coef[:G]), ptr(recon), ptr(dl), ptr(loss), stream())
        torch.cuda.synchronize()
        got = dict(loss=loss[:G].cpu())
        assert float(loss[G]) == start
        if want_recon:
            got["recon"] = recon[:G * B].cpu()
            assert float(recon[G * B].min()) == 7.0 == float(recon[G * B].max())
        if want_dl:
            got["dlogit"] = dl[:G * B].cpu()
            assert float(dl[G * B].min()) == 7.0 == float(dl[G * B].max())
            if G == 3:
                assert float(dl[B:2 * B].abs().max()) == 0.0              # the skipped pass
        _check("sigmoid_bce (G=%d, %s, recon=%d, dlogit=%d, start=%g)" % (G, case, want_recon, want_dl, start),
               E.gate_bce(got, logits, target, G, C, coef, start))


# ====================================================================================================== log-softmax + NLL
@pytest.mark.parametrize("rows_per_group", E.NLL_ROWS)
@pytest.mark.parametrize("classes", E.NLL_CLASSES)
def test_logsoftmax_nll(classes, rows_per_group):
    """mmvae_logsoftmax_nll at G = 3 with target_rows = rows_per_group (the target wraps), the wave path (64 rows per group) and the
    per-row path, the padded bf16 gradient and the fp32 gradient together and alone, a null target (log-probs only, nll slots
    untouched), a row with a logit spread of 200.
    Measured: words 4.2e-7 (6.4e-7; 2.1e-6 before the kernel subtracted the max first), dlogits_f32 2.2e-6 (6.3e-6 = 4 err32), dlogits_bf
    3.86e-3 (3.91e-3), NLL sums 2.5e-8 of sum|terms| (6.0e-7)."""
    call, ptr, stream = _api()
    dev = _dev()
    G, coef = 3, E.NLL_COEF
    logits, target = E.nll_inputs(G, rows_per_group, classes)
    rows, ld_d = G * rows_per_group, (classes + 7) // 8 * 8 + 8
    ldev, tdev = logits.to(dev), target.to(dev)
    for want_bf, want_f32, with_target in ((True, True, True), (True, False, True), (False, True, True), (False, False, False)):
        words = _full(dev, (rows + 1, classes), 7.0)
        slots = _full(dev, (E.LOSS_SLOTS, 16), 0.0 if with_target else float("nan"))
        dbf = _full(dev, (rows + 1, ld_d), 7.0, BF) if want_bf else None
        df = _full(dev, (rows + 1, classes), 7.0) if want_f32 else None
        call("mmvae_logsoftmax_nll", ptr(ldev), rows, classes, ptr(words), ptr(tdev) if with_target else None, rows_per_group, rows_per_group,
             ptr(slots), ptr(dbf), ld_d, ptr(df), _coef(coef), stream())
        torch.cuda.synchronize()
        got = dict(words=words[:rows].cpu())
        assert float(words[rows].min()) == 7.0 == float(words[rows].max())
        if with_target:
            got["nll"] = slots.double().sum(0)[:G].cpu()
            assert float(slots[:, G:].abs().max()) == 0.0
        else:
            assert bool(torch.isnan(slots).all())
        if want_bf:
            got["dlogits_bf"] = dbf[:rows].cpu()
            assert float(dbf[rows].float().min()) == 7.0 == float(dbf[rows].float().max())
        if want_f32:
            got["dlogits_f32"] = df[:rows].cpu()
            assert float(df[rows].min()) == 7.0 == float(df[rows].max())
        _check("logsoftmax_nll (classes=%d, rows/group=%d, bf16=%d, fp32=%d, target=%d)" % (classes, rows_per_group, want_bf, want_f32, with_target),
               E.gate_nll(got, logits, target if with_target else None, rows_per_group, coef))


# ====================================================================================================== BatchNorm triple
def _bn_fin(dev, inp, stats, training, updates, skip, fused, r_dev=None, ld=0, act=1):
    """bn_finalize (fused False) or bn_act (True) on fresh buffers -> tables, running buffers, nbt increment, activated output"""
    call, ptr, stream = _api()
    C, G, n = inp["C"], inp["G"], inp["rows_per_group"]
    aff, mr = _full(dev, (G, C, 2), float("nan")), _full(dev, (G, C, 2), float("nan"))
    rm, rv = inp["running_mean"].to(dev), inp["running_var"].to(dev)
    nbt = torch.full((1,), 5, dtype=torch.int64, device=dev)
    gamma, beta = inp["gamma"].to(dev), inp["beta"].to(dev)
    a = None
    tail = (ptr(stats), float(n), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt), updates, skip, ptr(aff), ptr(mr), E.BN_EPS, E.BN_MOM,
            int(training), stream())
    if fused:
        a = _full(dev, (G * n + 1, ld), 7.0, BF)
        call("mmvae_bn_act", ptr(r_dev), ptr(a), G * n, C, ld, n, G, act, *tail)
    else:
        call("mmvae_bn_finalize", tail[0], G, C, *tail[1:])
    torch.cuda.synchronize()
    return dict(affine=aff.cpu(), meanrstd=mr.cpu(), running_mean=rm.cpu(), running_var=rv.cpu(), nbt=int(nbt) - 5, a=a)


@pytest.mark.parametrize("rows_per_group", E.BN_ROWS)
@pytest.mark.parametrize("G", E.BN_G)
@pytest.mark.parametrize("C", E.BN_C)
def test_batchnorm_triple(C, G, rows_per_group):
    """mmvae_bn_finalize / mmvae_bn_act / mmvae_bn_bwd_apply on bf16 operands of their own, ld = C rounded up to 8 and 8 more.  stats /
    red are built in float64 from the bf16 r / db and spread unevenly over the 16 slots (some empty).  Channel 0 is constant within a
    group (the clamped variance must be exactly 0: rstd = rsqrt(eps)), the last channel has |mean| = 8 std (single-pass variance).
    updates_per_group in {1, 2} x skip_update_mask in {0, 0b010, 0b101}: num_batches_tracked moves by exactly the documented count;
    eval mode reads the running buffers and writes none.  bn_act: every activation code, its block-0 tables and both running-update
    paths equal bn_finalize's bit for bit, pad columns [C, 8 ceil(C/8)) zero and the columns behind them untouched.  bn_bwd_apply: db2
    present or null, dr aliasing db, dgamma / dbeta "+=" into 0 and into 0.5, or null.
    Measured: mean 5.5e-8 (2.4e-7), rstd / (1 + mean^2 / var) 1.2e-7 (2.38e-7: the single-pass variance keeps the cancellation bound, the
    constant channel's E[x^2] is a few ulp below mean^2 in the slot table, so only the clamp gives its exact 0), scale 1.6e-7 and shift
    1.2e-7 (4.8e-7), running mean 1.9e-7 (2.4e-7), running variance 0.81 of its per-channel gate max(2^-22 (1 + max_g mean^2 / var),
    4 err32 of the channel) at C = 64, G = 3, 2 updates (the float32 two-pass evaluation alone reaches 3.0e-7 / (1 + mean^2 / var) through
    the roundings of six momentum updates, above the bare 2.38e-7), a 3.85e-3 and dr 3.36e-3 (3.91e-3), dgamma 8.6e-8 and dbeta 4.4e-9 of sum|terms| (1.9e-6); bn_act's tables and
    running buffers equal bn_finalize's bit for bit in all 360 comparisons."""
    call, ptr, stream = _api()
    dev = _dev()
    n, rows = rows_per_group, G * rows_per_group
    c8 = (C + 7) // 8 * 8
    for ld in (c8, c8 + 8):
        inp = E.bn_inputs(C, ld, G, n)
        stats, r_dev = E.bn_stats(inp).to(dev), inp["r"].to(dev)
        tag = "bn (C=%d, ld=%d, G=%d, rows/group=%d)" % (C, ld, G, n)
        for updates, skip in itertools.product(E.BN_UPDATES, E.BN_SKIP):
            fin = _bn_fin(dev, inp, stats, True, updates, skip, False)
            _check("%s finalize updates=%d skip=%s" % (tag, updates, bin(skip)), E.gate_bn_tables(fin, inp, True, updates, skip))
            act = _bn_fin(dev, inp, stats, True, updates, skip, True, r_dev, ld)
            for k in ("affine", "meanrstd", "running_mean", "running_var"):
                assert torch.equal(fin[k], act[k]), (tag, k, "bn_act differs from bn_finalize")
            assert fin["nbt"] == act["nbt"]
        for code in E.ACTS:
            got = _bn_fin(dev, inp, stats, True, 1, 0, True, r_dev, ld, code)["a"]
            assert float(got[rows].float().min()) == 7.0 == float(got[rows].float().max())
            if ld > c8:
                assert float(got[:rows, c8:].float().min()) == 7.0 == float(got[:rows, c8:].float().max())
            _check("%s bn_act act=%d" % (tag, code), E.gate_bn_act(got[:rows], inp, code))
        for fused in (False, True):
            ev = _bn_fin(dev, inp, stats, False, 2, 0, fused, r_dev, ld, 2)
            assert torch.equal(ev["running_mean"], inp["running_mean"]) and torch.equal(ev["running_var"], inp["running_var"]) and ev["nbt"] == 0
            _check("%s eval fused=%d" % (tag, fused), E.gate_bn_tables(ev, inp, False))
            if fused:
                _check("%s eval bn_act" % tag, E.gate_bn_act(ev["a"][:rows], inp, 2, False))
        # ---- backward apply
        t64 = E.bn_tables(inp)
        mr = torch.stack((t64["mean"], t64["rstd"]), -1).float().contiguous().to(dev)
        gamma = inp["gamma"].to(dev)
        for use_db2, alias, start, with_params in ((False, False, 0.0, True), (True, True, 0.5, True), (True, False, 0.0, False)):
            red = E.bn_red(inp, use_db2).to(dev)
            db = torch.cat((inp["db"], torch.full((1, ld), 7.0, dtype=BF))).to(dev)
            db2 = inp["db2"].to(dev) if use_db2 else None
            dr = db if alias else _full(dev, (rows + 1, ld), 7.0, BF)
            dg, dbt = (_full(dev, (C + 1,), start) for _ in range(2)) if with_params else (None, None)
            call("mmvae_bn_bwd_apply", ptr(db), ptr(db2), ptr(r_dev), ptr(dr), rows, C, ld, n, G, ptr(red), ptr(mr), ptr(gamma), ptr(dg), ptr(dbt),
                 stream())
            torch.cuda.synchronize()
            got = dict(dr=dr[:rows].cpu())
            assert float(dr[rows].float().min()) == 7.0 == float(dr[rows].float().max())
            if with_params:
                got["dgamma"], got["dbeta"] = dg[:C].cpu(), dbt[:C].cpu()
                assert float(dg[C]) == start == float(dbt[C])
            _check("%s bwd db2=%d alias=%d start=%g" % (tag, use_db2, alias, start), E.gate_bn_bwd(got, inp, use_db2, start))


def test_bn_act_past_the_block_cap():
    """bn_act with more 8-column vectors than 2048 workgroups of 256 threads take in one sweep (C = 8, 2048 * 256 + 3 rows): the grid-stride
    loop's second sweep, against the same float64 reference."""
    dev = _dev()
    C, rows = 8, 2048 * 256 + 3
    inp = E.bn_inputs(C, 8, 1, rows)
    stats = E.bn_stats(inp).to(dev)
    got = _bn_fin(dev, inp, stats, True, 1, 0, True, inp["r"].to(dev), 8, 1)
    assert float(got["a"][rows].float().min()) == 7.0 == float(got["a"][rows].float().max())
    _check("bn_act past the cap", E.gate_bn_act(got["a"][:rows], inp, 1))


# ====================================================================================================== embedding, column sums
def test_embed_gather_scatter():
    """mmvae_embed_gather_stats at C = 50, ld = 56, rows = 3 x 37 with idx_rows = 37 (a group boundary inside a 64-row block): bf16 rows
    exact, pads zero, colstats folded over the 16 slots against float64 sums of the bf16 values (and null).  mmvae_embed_scatter_add
    with every row on one index (every atomic on one address), with distinct indices, and "+=" into a non-zero table.
    Measured: gathered rows exact; colstats 1.0e-7 of sum|terms| (4.4e-6), the scattered tables exact (sums of at most 111 bf16 values)."""
    call, ptr, stream = _api()
    dev = _dev()
    g = torch.Generator().manual_seed(77)
    C, ld, n, G, V = 50, 56, 37, 3, 61
    rows = G * n
    table, idx = torch.randn(V, C, generator=g), torch.randint(0, V, (n,), generator=g)
    x_ref, st, ab, nt = E.embed_ref(table, idx, rows, n, n, ld)
    table_d, idx_d = table.to(dev), idx.to(dev)
    for with_stats in (True, False):
        x = _full(dev, (rows + 1, ld), 7.0, BF)
        cs = _full(dev, (G, E.STAT_SLOTS, C, 2), 0.0) if with_stats else None
        call("mmvae_embed_gather_stats", ptr(table_d), C, ptr(idx_d), rows, n, n, ptr(x), ld, ptr(cs), stream())
        torch.cuda.synchronize()
        assert torch.equal(x[:rows].cpu(), x_ref) and float(x[rows].float().min()) == 7.0 == float(x[rows].float().max())
        if with_stats:
            _check("embed_gather colstats", [E.rec_sum("colstats", cs.double().sum(1).cpu(), st, ab, nt)])
    d = torch.zeros(rows, ld, dtype=BF)
    d[:, :C] = torch.randn(rows, C, generator=g).to(BF)
    d[:, C:] = 7.0                                                       # pad columns are never added
    d_d = d.to(dev)
    for name, ix, start in (("one index", torch.full((rows,), 9), 0.0), ("distinct", torch.randperm(rows, generator=g), 0.0),
                            ("wrapped +=", torch.arange(rows) % n, 1.5)):
        nrows_t = int(ix.max()) + 1
        gt, ix_d = _full(dev, (nrows_t + 1, C), start), ix.to(dev)
        call("mmvae_embed_scatter_add", ptr(d_d), ld, C, ptr(ix_d), rows, ptr(gt), stream())
        torch.cuda.synchronize()
        t, a, most = E.scatter_ref(d, ix, nrows_t, C)
        assert float(gt[nrows_t].min()) == start == float(gt[nrows_t].max())
        _check("embed_scatter %s" % name, [E.rec_sum("g_table", gt[:nrows_t].cpu(), t + start, a + abs(start), most + (1 if start else 0))])


def test_column_sums():
    """mmvae_colsum_f32 at (1, 1), (5, 10), (37, 65), (300, 784) and mmvae_colsum_bf16 at ld in {8, 24, 56, 2048} with cols < ld (at 24 one
    thread of the block has no vector, at 2048 there is one row lane), "+=" into 0 and into 0.5; the columns [cols, ld) are not added.
    Measured: colsum_f32 5.5e-8 of sum|terms| (6.0e-7 at 5 rows), colsum_bf16 3.3e-8 (4.4e-6 at 37 rows)."""
    call, ptr, stream = _api()
    dev = _dev()
    g = torch.Generator().manual_seed(78)
    for rows, cols in E.COLSUM_F32:
        x = torch.randn(rows, cols, generator=g) + 0.5
        x_d = x.to(dev)
        for start in (0.0, 0.5):
            out = _full(dev, (cols + 1,), start)
            call("mmvae_colsum_f32", ptr(x_d), rows, cols, ptr(out), stream())
            torch.cuda.synchronize()
            assert float(out[cols]) == start
            _check("colsum_f32 (%d, %d) start=%g" % (rows, cols, start), E.gate_colsum("colsum_f32", out[:cols].cpu(), x, start))
    for ld in E.COLSUM_BF16_LD:
        for rows in (1, 37, 300):
            cols = ld - 3
            x = (torch.randn(rows, ld, generator=g) + 0.5).to(BF)
            x_d = x.to(dev)
            for start in (0.0, 0.5):
                out = _full(dev, (ld + 1,), start)
                call("mmvae_colsum_bf16", ptr(x_d), ld, rows, cols, ptr(out), stream())
                torch.cuda.synchronize()
                assert float(out[cols:].min()) == start == float(out[cols:].max())
                _check("colsum_bf16 (ld=%d, rows=%d) start=%g" % (ld, rows, start), E.gate_colsum("colsum_bf16", out[:cols].cpu(), x[:, :cols], start))


def test_wrappers_refuse_what_would_index_out_of_range():
    """the launchers' checks: each call below would read or write out of range and must come back as an error with a message"""
    from multimodal_vae_amd._lib import MMVAEError
    call, ptr, stream = _api()
    dev = _dev()
    t = _full(dev, (4096,), 0.0)
    p = ptr(t)
    bad = [
        ("mmvae_bn_bwd_apply", (p, None, p, p, 6, 2049, 2056, 3, 2, p, p, p, None, None, stream())),          # G * C > 4096: LDS table
        ("mmvae_bn_bwd_apply", (p, None, p, p, 7, 8, 8, 3, 2, p, p, p, None, None, stream())),                # rows > G * rows_per_group
        ("mmvae_bn_act", (p, p, 7, 8, 8, 3, 2, 0, p, 3.0, p, p, None, None, None, 1, 0, None, None, 1e-5, 0.1, 1, stream())),
        ("mmvae_bn_act", (p, p, 6, 10, 8, 3, 2, 0, p, 3.0, p, p, None, None, None, 1, 0, None, None, 1e-5, 0.1, 1, stream())),   # ld < C
        ("mmvae_colsum_bf16", (p, 8, 4, 9, p, stream())),                                                     # cols > ld
        ("mmvae_colsum_f32", (p, 0, 4, p, stream())),
        ("mmvae_latent3_fwd", (p, None, p, None, 2, 4, 1, p, p, p, p, 8, p, stream())),                       # training without eps
        ("mmvae_latent3_fwd", (p, None, p, p, 2, 12, 1, p, p, p, p, 8, p, stream())),                         # ldz < D
        ("mmvae_latent3_bwd", (p, None, p, p, p, p, None, None, 2, 4, 1, 0.0, 0.0, 0.0, None, 0, 0, None, None, None, None, None, None, None,
                               stream())),                                                                    # no image gradient output
        ("mmvae_latent3_bwd", (p, None, p, p, p, p, None, None, 2, 4, 1, 0.0, 0.0, 0.0, p, 4, 0, None, None, None, None, None, None, None,
                               stream())),                                                                    # ld_img_out_bf < 2D
        ("mmvae_sigmoid_bce", (p, 1, p, 5, 1, 1, 2, 2, _coef((1.0,)), None, None, p, stream())),              # G > 4
        ("mmvae_sigmoid_bce", (p, 1, p, 1, 1, 2, 2, 2, _coef((1.0,)), None, None, p, stream())),              # ldl < C
        ("mmvae_logsoftmax_nll", (p, 10, 3, p, None, 0, 2, None, None, 0, None, _coef((1.0,)), stream())),    # 5 groups
        ("mmvae_logsoftmax_nll", (p, 4, 10, p, None, 0, 2, None, p, 8, None, _coef((1.0,)), stream())),       # ld_d < classes
        ("mmvae_embed_gather_stats", (p, 10, p, 4, 0, 2, p, 16, None, stream())),                             # idx_rows 0
        ("mmvae_embed_scatter_add", (p, 8, 10, p, 4, p, stream())),                                           # ld < C
    ]
    for name, args in bad:
        with pytest.raises(MMVAEError) as e:
            call(name, *args)
        assert len(str(e.value)) > 10, name
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


# ====================================================================================================== stand-alone ops
@pytest.mark.parametrize("n", E.STANDALONE_N)
def test_standalone_ops(n):
    """mmvae_poe_fwd / _bwd (M = 1, 2, 3), reparam, kl, bce, nll, mse forward and backward against float64 at n around the 256-thread
    block, with gscale present and null where the op has one; logvars over [-20, 2] with -20 exactly, probabilities that include exact
    0 and 1 (the -100 clamp and the 1e-12 clamp).
    Measured, closest to its gate first: poe_fwd logvar 1.7e-7 (2.4e-7), mse_bwd 1.2e-7 (2.4e-7), bce_bwd 1.2e-7 (3.2e-7), poe_bwd 2.9e-7
    (1.0e-6), reparam 1.4e-7 (5.0e-7), kl_bwd 7.1e-8 (2.9e-7), poe_fwd mu 1.4e-7 (5.2e-7); mse_fwd (N = n) 8.8e-8 of sum|terms| at n = 1
    (1.19e-7), the other sums under 0.4 of their gates; nll_bwd exact."""
    call, ptr, stream = _api()
    dev = _dev()
    g = torch.Generator().manual_seed(900 + n)
    F32 = torch.float32
    nanbuf = lambda *shape: _full(dev, shape, float("nan"))

    def lvs(M):
        lv = 22.0 * torch.rand(M, n, generator=g) - 20.0
        lv[:, 0] = -20.0
        return lv
    recs = []
    for M in (1, 2, 3):
        mu, lv, gm, gl = torch.randn(M, n, generator=g), lvs(M), torch.randn(n, generator=g), torch.randn(n, generator=g)
        om, ol, dm, dl = nanbuf(n), nanbuf(n), nanbuf(M, n), nanbuf(M, n)
        mu_d, lv_d, gm_d, gl_d = (t.to(dev) for t in (mu, lv, gm, gl))
        call("mmvae_poe_fwd", ptr(mu_d), ptr(lv_d), M, n, ptr(om), ptr(ol), stream())
        call("mmvae_poe_bwd", ptr(mu_d), ptr(lv_d), M, n, ptr(gm_d), ptr(gl_d), ptr(dm), ptr(dl), stream())
        r64, r32 = E.poe(mu, lv), E.poe(mu, lv, F32)
        recs += [E.rec_f32("poe_fwd mu M=%d" % M, om, r64[0], r64[2], r32[0]), E.rec_f32("poe_fwd logvar M=%d" % M, ol, r64[1], r64[3], r32[1])]
        b64, b32 = E.poe_bwd(mu, lv, gm, gl), E.poe_bwd(mu, lv, gm, gl, F32)
        recs += [E.rec_f32("poe_bwd d_mu M=%d" % M, dm, b64[0], b64[2], b32[0]), E.rec_f32("poe_bwd d_logvar M=%d" % M, dl, b64[1], b64[3], b32[1])]
    mu, lv, eps, dz = torch.randn(n, generator=g), lvs(1)[0], torch.randn(n, generator=g), torch.randn(n, generator=g)
    mu_d, lv_d, eps_d, dz_d = (t.to(dev) for t in (mu, lv, eps, dz))
    z, dm, dl = nanbuf(n), nanbuf(n), nanbuf(n)
    call("mmvae_reparam_fwd", ptr(mu_d), ptr(lv_d), ptr(eps_d), n, ptr(z), stream())
    call("mmvae_reparam_bwd", ptr(lv_d), ptr(eps_d), ptr(dz_d), n, ptr(dm), ptr(dl), stream())
    (z64, zm), (z32, _) = E.reparam(mu, lv, eps), E.reparam(mu, lv, eps, F32)
    b64, b32 = E.reparam_bwd(lv, eps, dz), E.reparam_bwd(lv, eps, dz, F32)
    assert torch.equal(dm.cpu(), dz)
    recs += [E.rec_f32("reparam_fwd", z, z64, zm, z32), E.rec_f32("reparam_bwd d_logvar", dl, b64[1], b64[3], b32[1])]
    gs = torch.tensor([0.625], device=dev)
    out = _full(dev, (2,), 0.0)
    call("mmvae_kl_fwd", ptr(mu_d), ptr(lv_d), n, ptr(out), stream())
    k64, kabs, kn = E.kl_terms(mu, lv)
    recs.append(E.rec_sum("kl_fwd", out[0], k64, kabs, kn))
    for scale, gp in ((1.0, None), (0.625, ptr(gs))):
        dm, dl = nanbuf(n), nanbuf(n)
        call("mmvae_kl_bwd", ptr(mu_d), ptr(lv_d), n, 0.37, gp, ptr(dm), ptr(dl), stream())
        b64, b32 = E.kl_bwd(mu, lv, 0.37 * scale), E.kl_bwd(mu, lv, 0.37 * scale, F32)
        recs += [E.rec_f32("kl_bwd d_mu gscale=%g" % scale, dm, b64[0], b64[2], b32[0]),
                 E.rec_f32("kl_bwd d_logvar gscale=%g" % scale, dl, b64[1], b64[3], b32[1])]
    # BCE on probabilities
    p, t = torch.rand(n, generator=g), torch.rand(n, generator=g)
    if n >= 255:
        p[:4] = torch.tensor([0.0, 0.0, 1.0, 1.0])
        t[:4] = torch.tensor([0.0, 1.0, 0.0, 1.0])
    out, p_d, t_d = _full(dev, (2,), 0.0), p.to(dev), t.to(dev)
    call("mmvae_bce_fwd", ptr(p_d), ptr(t_d), n, ptr(out), stream())
    s64, sabs, sn, d64, dmag = E.bce_probs(p, t)
    d32 = E.bce_probs(p, t, F32)[3]
    recs.append(E.rec_sum("bce_fwd", out[0], s64, sabs, sn))
    for scale, gp in ((1.0, None), (0.625, ptr(gs))):
        dp = nanbuf(n)
        call("mmvae_bce_bwd", ptr(p_d), ptr(t_d), n, 0.37, gp, ptr(dp), stream())
        recs.append(E.rec_f32("bce_bwd gscale=%g" % scale, dp, 0.37 * scale * d64, 0.37 * scale * dmag, 0.37 * scale * d32.double()))
    # NLL on log-probs
    classes = 7
    lp = torch.log_softmax(3 * torch.randn(n, classes, generator=g), 1)
    tg = torch.randint(0, classes, (n,), generator=g)
    out, lp_d, tg_d = _full(dev, (2,), 0.0), lp.to(dev), tg.to(dev)
    call("mmvae_nll_fwd", ptr(lp_d), ptr(tg_d), n, classes, ptr(out), stream())
    s64, sabs, sn = E.nll_picked(lp, tg)
    recs.append(E.rec_sum("nll_fwd", out[0], s64, sabs, sn))
    for scale, gp in ((1.0, None), (0.625, ptr(gs))):
        dlp = nanbuf(n, classes)
        call("mmvae_nll_bwd", ptr(tg_d), n, classes, 0.37, gp, ptr(dlp), stream())
        want = -(torch.tensor(0.37) * torch.tensor(scale)) * torch.nn.functional.one_hot(tg, classes).float()
        recs.append(E.rec_exact("nll_bwd gscale=%g" % scale, dlp, want))
    # MSE
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    out, a_d, b_d = _full(dev, (2,), 0.0), a.to(dev), b.to(dev)
    call("mmvae_mse_fwd", ptr(a_d), ptr(b_d), n, ptr(out), stream())
    s64, sabs, sn, d64, dmag = E.mse(a, b)
    d32 = E.mse(a, b, F32)[3]
    recs.append(E.rec_sum("mse_fwd", out[0], s64, sabs, sn))
    for scale, gp in ((1.0, None), (0.625, ptr(gs))):
        da = nanbuf(n)
        call("mmvae_mse_bwd", ptr(a_d), ptr(b_d), n, 0.37, gp, ptr(da), stream())
        recs.append(E.rec_f32("mse_bwd gscale=%g" % scale, da, 0.37 * scale * d64, 0.37 * scale * dmag, 0.37 * scale * d32.double()))
    torch.cuda.synchronize()
    _check("stand-alone ops (n=%d)" % n, recs)
