"""float64 references of MultiMNIST's uni-modal image VAE (multimnist/model.py:96-120, multimnist/train_imageonly.py:91-106).

1. The model and its loss, composed from the oracle's own functions: ``multimnist_image_encoder``, ``multimnist_image_decoder``,
   ``reparametrize`` and ``multimnist_loss`` with no text arguments.  There is NO product of experts: mu and logvar are the two
   halves of the encoder's output, untouched.
2. The one-expert waist (csrc/mlp_tail.hip, mlp2_latent1_fwd / _bwd) evaluated in float64 FROM THE OPERANDS THE KERNEL READS: the
   bf16 activation ``ay1``, the bf16-rounded weights, the fp32 biases, the keep masks, eps; backward: the fp32 mu / logvar / dz and
   the bf16 tensors the kernel itself wrote.  Each quantity comes with a per-element yardstick derived below from the number
   formats alone (``U32`` = 2^-24, ``UBF`` = 2^-8: the unit roundoffs of fp32 and bf16), never from what a kernel returned:

     y2      = ay1 W2^T + b2                     fp32 accumulation over K = 400: |err| <= (K + 2) U32 (|ay1| |W2|^T + |b2|) =: e2,
                                                 stored as bf16: + UBF |y2|
     ay2     = swish(y2) keep2 / (1 - p)         |swish'| <= 1.1: 1.1 e2 / (1 - p) + 8 U32 |ay2| (the fp32 evaluation), stored: + UBF |ay2|
     enc_out = bf16(ay2) W3^T + b3               the intermediate is rounded to bf16 before the second GEMM: da = 1.1 e2 / (1 - p) +
                                                 (UBF + 8 U32) |ay2| goes through |W3|: da |W3|^T, plus the fp32 accumulation over
                                                 K = 200: (K + 2) U32 (|ay2| |W3|^T + |b3|)            =: e_mu | e_lv
     z       = eps exp(lv / 2) + mu              e_mu + |eps| (exp((lv + e_lv) / 2) - exp(lv / 2)) + 8 U32 (|mu| + |eps| exp(lv / 2))
     z_bf    = bf16(z), column D = 1, pads 0     + UBF |z|; the pad columns are exact
     KL      = -sum(1 + lv - mu^2 - exp(lv)) / 2 sum(|mu| e_mu + e_mu^2 / 2 + e_lv / 2 + (exp(lv + e_lv) - exp(lv)) / 2)
                                                 + 8 U32 sum(1 + |lv| + mu^2 + exp(lv)) / 2 (fp32 terms; they are added in double)
     d_enc_out = bf16 of latent1_bwd's doubles   (UBF + 2 U32) |g|, pad columns exact
     d_bias    = column sums of those doubles    2 B U32 sum|g|  (the gate of test_latent1_alone)
     dy2     = (d_enc_out W3) swish'(y2) keep2 / (1 - p)     fp32 accumulation over K = 2 D, |swish'| <= 1.1:
                                                 e = (2 D + 2) U32 (|d| |W3|) 1.1 / (1 - p) + 8 U32 |dy2|, stored: + UBF |dy2|
     dy1     = (bf16(dy2) W2) swish'(y1) keep1 / (1 - p)     the same over K = 200, from the dy2 the kernel stored
     db2, db1 = column sums of the fp32 dy2, dy1 sum over the rows of e + B U32 sum|dy| (fp32 atomics, any order)
"""
import torch

from oracle import mmvae_ref as R
import imageonly_ref as IR

FAMILY = "multimnist"
MASK_WIDTHS = (400, 200)
U32, UBF = 2.0 ** -24, 2.0 ** -8
SW = 1.1                         # max |swish'| = 1.0998
TR = 16                          # rows of a waist workgroup


def image_names(D):
    return IR.image_names(FAMILY, D)


def state_dict_keys(D):
    """The keys of ``multimnist.ImageVAE(D).state_dict()`` (BatchNorm buffers behind the bias, nn.Module order)."""
    return IR.state_dict_keys(FAMILY, D)


def state_dict_shapes(D):
    """[key, shape] of the same state_dict, from the oracle's tables."""
    shapes = dict(R.param_table(FAMILY, D))
    bn = dict(R.bn_layers(FAMILY, D))
    out = []
    for k in state_dict_keys(D):
        n = "image_" + k
        if n in shapes:
            out.append([k, list(shapes[n])])
        else:
            pre, buf = n.rsplit(".", 1)
            out.append([k, [] if buf == "num_batches_tracked" else [bn[pre]]])
    return out


def params64(D, requires_grad=False):
    return IR.params64(FAMILY, D, requires_grad)


def forward(p, image, training, eps=None, masks=None, drop_p=R.DROP_P):
    """-> (recon, mu, logvar).  masks: a pair of keep masks (B,400), (B,200) or None."""
    o = R.multimnist_image_encoder(p, image.double(), training, None if masks is None else tuple(m.double() for m in masks), drop_p=drop_p)
    D = o.shape[1] // 2
    mu, logvar = o[:, :D], o[:, D:]
    z = R.reparametrize(mu, logvar, training, None if eps is None else eps.double())
    return R.multimnist_image_decoder(p, z, training), mu, logvar


def step_loss(p, image, training, eps=None, masks=None, drop_p=R.DROP_P, kl_lambda=1e-3):
    recon, mu, logvar = forward(p, image, training, eps, masks, drop_p)
    return R.multimnist_loss(mu, logvar, recon_image=recon, image=image.double(), kl_lambda=kl_lambda, lambda_xy=1.), (recon, mu, logvar)


# ================================================================================================ the waist
def bf(x):
    """the value a bf16 store keeps, as float64"""
    return x.to(torch.float32).to(torch.bfloat16).double()


def swish_grad(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def waist_inputs(B, D, seed=0):
    """Operands of the waist at the sizes of the image encoder's classifier: what the GPU test reads back from a step, drawn here."""
    g = torch.Generator().manual_seed(1000 * D + 10 * B + seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    keep = lambda *s: (torch.rand(*s, generator=g) >= R.DROP_P).double()
    y1 = bf(0.7 * r(B, 400))
    m1, m2 = keep(B, 400), keep(B, 200)
    return dict(y1=y1, ay1=bf(R.swish(y1) * m1 / (1 - R.DROP_P)), m1=m1, m2=m2,
                w2=bf(r(200, 400) / 20.0), b2=0.05 * r(200).float().double(), w3=bf(r(2 * D, 200) / 14.0), b3=0.05 * r(2 * D).float().double(),
                eps=r(B, D).float().double(), dz=(r(B, D) / 50.0).float().double(), kl_coef=1e-3 / B, training=True, drop=True)


def waist_forward(c):
    """float64 values and yardsticks of the forward's outputs from its operands ``c`` (see the module docstring)."""
    ms = 1.0 / (1 - R.DROP_P) if c["drop"] else 1.0
    keep = c["m2"] if c["drop"] else torch.ones_like(c["m2"])
    D = c["w3"].shape[0] // 2
    y2 = c["ay1"] @ c["w2"].t() + c["b2"]
    e2 = (400 + 2) * U32 * (c["ay1"].abs() @ c["w2"].abs().t() + c["b2"].abs())
    ay2 = R.swish(y2) * keep * ms
    da = SW * e2 * ms + (UBF + 8 * U32) * ay2.abs()
    enc = ay2 @ c["w3"].t() + c["b3"]
    e_enc = da @ c["w3"].abs().t() + (200 + 2) * U32 * (ay2.abs() @ c["w3"].abs().t() + c["b3"].abs())
    mu, lv, e_mu, e_lv = enc[:, :D], enc[:, D:], e_enc[:, :D], e_enc[:, D:]
    std = torch.exp(0.5 * lv)
    z = c["eps"] * std + mu if c["training"] else mu
    e_z = e_mu + 8 * U32 * mu.abs()
    if c["training"]:
        e_z = e_z + c["eps"].abs() * (torch.exp(0.5 * (lv + e_lv)) - std) + 8 * U32 * c["eps"].abs() * std
    kl = -0.5 * torch.sum(1 + lv - mu ** 2 - lv.exp())
    e_kl = torch.sum(mu.abs() * e_mu + 0.5 * e_mu ** 2 + 0.5 * e_lv + 0.5 * (torch.exp(lv + e_lv) - lv.exp())) \
        + 8 * U32 * 0.5 * torch.sum(1 + lv.abs() + mu ** 2 + lv.exp())
    ref = dict(y2=y2, ay2=ay2, encout=enc, mu=mu, logvar=lv, z=z, z_bf=z, kl=kl)
    st = lambda e, v: e + UBF * (v.abs() + e)          # a bf16 store of a value that carries the error e
    tol = dict(y2=st(e2, y2), ay2=st(SW * e2 * ms + 8 * U32 * ay2.abs(), ay2), encout=e_enc, mu=e_mu, logvar=e_lv, z=e_z, z_bf=st(e_z, z), kl=e_kl)
    return ref, tol


def waist_backward(c, f):
    """float64 values and yardsticks of the backward's outputs.  ``f``: what the forward left behind AS STORED (mu, logvar fp32; y2 bf16)
    and, for the second data gradient, the d_enc_out / dy2 the backward itself stored (``d_enc_out``, ``dy2``; absent: the float64
    values rounded to bf16, which is what a correct kernel stores up to its yardstick)."""
    ms = 1.0 / (1 - R.DROP_P) if c["drop"] else 1.0
    k2 = c["m2"] if c["drop"] else torch.ones_like(c["m2"])
    k1 = c["m1"] if c["drop"] else torch.ones_like(c["m1"])
    B, D = f["mu"].shape
    g = IR.latent1_bwd(f["mu"], f["logvar"], c["eps"], c["dz"], c["kl_coef"], c["training"])
    d = f.get("d_enc_out", bf(g))
    dy2 = (d @ c["w3"]) * swish_grad(f["y2"]) * k2 * ms
    e_dy2 = (2 * D + 2) * U32 * (d.abs() @ c["w3"].abs()) * SW * ms + 8 * U32 * dy2.abs()
    dy2s = f.get("dy2", bf(dy2))
    dy1 = (dy2s @ c["w2"]) * swish_grad(c["y1"]) * k1 * ms
    e_dy1 = (200 + 2) * U32 * (dy2s.abs() @ c["w2"].abs()) * SW * ms + 8 * U32 * dy1.abs()
    ref = dict(d_enc_out=g, d_bias=g.sum(0), dy2=dy2, dy1=dy1, db2=dy2.sum(0), db1=dy1.sum(0))
    tol = dict(d_enc_out=(UBF + 2 * U32) * g.abs(), d_bias=2 * B * U32 * g.abs().sum(0), dy2=e_dy2 + UBF * (dy2.abs() + e_dy2), dy1=e_dy1 + UBF * (dy1.abs() + e_dy1),
               db2=e_dy2.sum(0) + B * U32 * dy2.abs().sum(0), db1=e_dy1.sum(0) + B * U32 * dy1.abs().sum(0))
    return ref, tol


def violations(got, ref, tol):
    """{quantity: worst |got - ref| / yardstick} of every quantity of ``ref`` whose worst element exceeds its yardstick (a yardstick
    of 0 asks for equality), and the worst ratio of every quantity."""
    bad, ratios = {}, {}
    for k, r in ref.items():
        gk = torch.as_tensor(got[k]).double().reshape(r.shape)
        err, t = (gk - r).abs(), torch.as_tensor(tol[k]).double().expand_as(r)
        ratio = float(torch.where(t > 0, err / t.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))).max())
        ratios[k] = ratio
        if not ratio <= 1.0:
            bad[k] = ratio
    return bad, ratios


def pad_violations(z_bf, d_enc_out, D):
    """the pad columns as stored: column D of z_bf exactly 1, the columns behind it and those of d_enc_out past 2 D exactly 0"""
    bad = []
    if not bool((z_bf[:, D] == 1).all()):
        bad.append("z_bf[:, D] != 1")
    if z_bf.shape[1] > D + 1 and float(z_bf[:, D + 1:].abs().max()) != 0.0:
        bad.append("z_bf pads != 0")
    if d_enc_out.shape[1] > 2 * D and float(d_enc_out[:, 2 * D:].abs().max()) != 0.0:
        bad.append("d_enc_out pads != 0")
    return bad


FAULTS = ("eps", "kl_coef", "mask2", "last_block", "z_bf_one")


def emulate(c, ldz, lde, fault=None):
    """A stand-in for the kernel pair in the kernel's own arithmetic (fp32 GEMMs on the bf16 operands, bf16 stores), optionally with
    one of FAULTS: eps ignored (z = mu, no eps term in the gradient) | the kl_coef terms dropped | the second keep mask ignored | the
    last partial 16-row block left out (its outputs stay at the 0 the buffers held) | 0 instead of 1.0 in column D of z_bf."""
    f32 = lambda x: x.to(torch.float32)
    ms = (1.0 / (1 - R.DROP_P)) if c["drop"] else 1.0
    B, D = c["eps"].shape
    k2 = c["m2"] if c["drop"] and fault != "mask2" else torch.ones_like(c["m2"])
    k1 = c["m1"] if c["drop"] else torch.ones_like(c["m1"])
    y2 = f32(c["ay1"]) @ f32(c["w2"]).t() + f32(c["b2"])
    ay2 = f32(R.swish(y2.double()) * k2 * ms)
    enc = f32(bf(ay2)) @ f32(c["w3"]).t() + f32(c["b3"])
    mu, lv = enc[:, :D], enc[:, D:]
    training = c["training"] and fault != "eps"
    z = f32(c["eps"]) * torch.exp(0.5 * lv) + mu if training else mu.clone()
    z_bf = torch.zeros(B, ldz, dtype=torch.float64)
    z_bf[:, :D] = bf(z)
    z_bf[:, D] = 0.0 if fault == "z_bf_one" else 1.0
    kl = (-0.5 * (1.0 + lv - mu * mu - torch.exp(lv))).double().sum()
    kc = 0.0 if fault == "kl_coef" else c["kl_coef"]
    g = IR.latent1_bwd(mu, lv, c["eps"], c["dz"], kc, training)
    d = torch.zeros(B, lde, dtype=torch.float64)
    d[:, :2 * D] = bf(g)
    dy2 = (f32(d[:, :2 * D]) @ f32(c["w3"])) * f32(swish_grad(bf(y2)) * k2 * ms)
    dy1 = (f32(bf(dy2)) @ f32(c["w2"])) * f32(swish_grad(c["y1"]) * k1 * ms)
    out = dict(y2=bf(y2), ay2=bf(ay2), encout=enc.double(), mu=mu.double(), logvar=lv.double(), z=z.double(), z_bf=z_bf[:, :D], kl=kl,
               d_enc_out=d[:, :2 * D], d_bias=g.sum(0), dy2=bf(dy2), dy1=bf(dy1), db2=dy2.double().sum(0), db1=dy1.double().sum(0),
               z_bf_full=z_bf, d_enc_out_full=d)
    if fault == "last_block" and B % TR:
        r0 = B // TR * TR
        for k in ("y2", "ay2", "encout", "mu", "logvar", "z", "z_bf", "d_enc_out", "dy2", "dy1", "z_bf_full", "d_enc_out_full"):
            out[k] = out[k].clone()
            out[k][r0:] = 0.0
        out["kl"] = (-0.5 * (1.0 + lv[:r0] - mu[:r0] * mu[:r0] - torch.exp(lv[:r0]))).double().sum()
        out["d_bias"], out["db2"], out["db1"] = g[:r0].sum(0), dy2[:r0].double().sum(0), dy1[:r0].double().sum(0)
    return out


def check_waist(c, got, ldz=None, lde=None):
    """Every comparison of the waist at once: -> (list of failures, worst ratios).  ``got``: the quantities of ``emulate`` as the
    kernels (or the stand-in) stored them."""
    D = c["eps"].shape[1]
    fref, ftol = waist_forward(c)
    bad, ratios = violations(got, fref, ftol)
    stored = dict(mu=got["mu"].double(), logvar=got["logvar"].double(), y2=got["y2"].double())
    bref, btol = waist_backward(c, stored)
    b1, r1 = violations(got, {k: bref[k] for k in ("d_enc_out", "d_bias")}, btol)
    stored.update(d_enc_out=got["d_enc_out"].double(), dy2=got["dy2"].double())
    bref, btol = waist_backward(c, stored)
    b2, r2 = violations(got, {k: bref[k] for k in ("dy2", "dy1", "db2", "db1")}, btol)
    fails = ["%s %.3g x its yardstick" % kv for d in (bad, b1, b2) for kv in d.items()]
    fails += pad_violations(got["z_bf_full"].double(), got["d_enc_out_full"].double(), D)
    ratios.update(r1)
    ratios.update(r2)
    return fails, ratios
