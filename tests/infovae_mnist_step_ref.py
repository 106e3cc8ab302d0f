"""Yardsticks for the MNIST InfoVAE's fp32 Linear kernels and its one-enqueue step (csrc/infovae_mnist.hip), independent of the package.

``lin_layer``     one layer y = act(x W^T + b) with dx, dW, db in any dtype; the backward works from a SAVED OUTPUT, as the kernels do
``lin_reference`` the same in float64, in float32 (the yardstick E_f32) and the gates
``torch_step``    the reference formulation (mnist/model.py:238-279 + mnist/train_infovae.py:45-76) under torch autograd, in any dtype
``step``          the float64 restatement of ``mmvae_mnist_infovae_step``: activations between the convolutions and the two large
                  Linears channels-last, the (c, h, w) <-> (h, w, c) permutation explicit, the Linear backward written out from the
                  saved output; ``emulate``: the convolutions on bf16-rounded operands; ``fault``: what an implementation can get
                  wrong (FAULTS)
``step_yardsticks`` the GPU test's per-tensor gate: 2 E_emu + C_STEP E_f32
"""
import torch
import torch.nn.functional as F

import conv4s2_ref as C

PERM_P, PERM_C = 49, 128
ACTS = ("none", "relu", "leaky")
# (rows, N, K, perm): y [rows][N] = act(x [rows][K] W^T + b)
LAYER_SHAPES = [(1, 20, 1024, 0), (3, 1024, 2, 0), (65, 1024, 6272, 1), (5, 6272, 1024, 1), (17, 33, 1024, 0)]
STEP_SHAPES = [(1, 20), (4, 2), (9, 20), (65, 33)]          # (B, D)
STEP_LAMBDAS = (0.75, 2.5)                                  # lambda_x, lambda_mmd of the whole-step test: neither weight is 1
# The gates' multiples.  The kernels sum in another order than the CPU's float32 BLAS does, exact products either way.  MEASURED on the
# MI355X (profiles/infovae_mnist_step_bench.txt):
#   layers: the worst E_hip / max(E_f32, 2^-23 max |ref|) over the shapes, activations and outputs above is 2.22 (db of
#           (65, 1024, 6272, perm), relu: 65 terms on the MFMA's accumulator against torch's vectorised column sum; y, dx, dW stay
#           within 1.23); the multiple is 8, under 4 x of headroom, and the limit beyond which the kernel counts as wrong
#   step:   no tensor needs the float32 term, E_hip <= 2 E_emu alone at every shape (worst E_hip / (2 E_emu) = 0.59, z at B = 1;
#           E_hip follows E_emu to three digits wherever the convolutions' rounding dominates); C_STEP = 4 is the allowance for a
#           tensor that rounding hardly reaches, and the worst E_hip / gate is 0.50
LAYER_MEASURED, LAYER_FACTOR = 2.22, 8.0
STEP_MEASURED, C_STEP = 0.0, 4.0
FAULTS = ("perm_efc0", "perm_dfc2", "no_slope", "relu_sign_g", "no_db", "last_row", "mmd_dropped", "mmd_wrong_class", "lambda_mmd_ignored",
          "mse_no_784")
NAMES = ("encoder_conv.0.weight", "encoder_conv.2.weight", "encoder_fc.0.weight", "encoder_fc.0.bias", "encoder_fc.2.weight",
         "encoder_fc.2.bias", "decoder_fc.0.weight", "decoder_fc.0.bias", "decoder_fc.2.weight", "decoder_fc.2.bias",
         "decoder_conv.0.weight", "decoder_conv.2.weight")
DECODER = NAMES[6:]


def shapes_of(D):
    return [(64, 1, 4, 4), (128, 64, 4, 4), (1024, 6272), (1024,), (D, 1024), (D,), (1024, D), (1024,), (6272, 1024), (6272,),
            (128, 64, 4, 4), (64, 1, 4, 4)]


def formula_weights(D):
    """the fixture's formula over InfoVAE(n_latents=D)'s state_dict, float64"""
    return C.formula_state_dict(list(NAMES), shapes_of(D))


def to_cl(t):
    """[rows][c * 49 + p] -> [rows][p * 128 + c]: a (c, h, w) flattening as conv4s2 keeps it in memory"""
    return t.reshape(t.shape[0], PERM_C, PERM_P).transpose(1, 2).reshape(t.shape[0], -1)


def from_cl(t):
    return t.reshape(t.shape[0], PERM_P, PERM_C).transpose(1, 2).reshape(t.shape[0], -1)


# ------------------------------------------------------------------------------------------------------ one layer
def act(pre, kind, slope):
    if kind == "relu":
        return torch.where(pre > 0, pre, torch.zeros_like(pre))
    if kind == "leaky":
        return torch.where(pre > 0, pre, slope * pre)
    return pre


def gp(g, y, kind, slope, fault=None):
    """the gradient in front of the activation from the upstream gradient and the saved output"""
    on = (g if fault == "relu_sign_g" else y) > 0
    if kind == "relu":
        return torch.where(on, g, torch.zeros_like(g))
    if kind == "leaky":
        return torch.where(on, g, (0.0 if fault == "no_slope" else slope) * g)
    return g


def lin_layer(x, w, b, g, kind, slope, dtype, y=None):
    """{"y", "dx", "dw", "db"} in ``dtype``; the backward uses ``y`` (the saved output) when given, else this forward's own"""
    x, w, b, g = (t.to(dtype) for t in (x, w, b, g))
    out = act(x @ w.t() + b, kind, slope)
    q = gp(g, out if y is None else y.to(dtype), kind, slope)
    return {"y": out, "dx": q @ w, "dw": q.t() @ x, "db": q.sum(0)}


def lin_reference(x, w, b, g, kind, slope, y=None):
    """-> (float64 results, yardsticks E_f32, gates): gate = LAYER_FACTOR x max(E_f32, 2^-23 max |reference|).  Both backwards work
    from the same saved output: ``y`` (the kernel's own, float32) when given, else the float64 forward rounded to float32."""
    slope = C.slope32(slope)
    fwd = lin_layer(x, w, b, g, kind, slope, torch.float64)
    saved = fwd["y"].float() if y is None else y.float()
    ref = lin_layer(x, w, b, g, kind, slope, torch.float64, y=saved)
    f32 = lin_layer(x, w, b, g, kind, slope, torch.float32, y=saved)
    yard = {k: float((f32[k].double() - ref[k]).abs().max()) for k in ref}
    gates = {k: LAYER_FACTOR * max(yard[k], 2.0 ** -23 * float(ref[k].abs().max())) for k in ref}
    return ref, yard, gates


def lin_operands(shape, seed=0):
    """float32 x, w, b and an upstream gradient g, seeded; pre-activations of about unit scale, both signs"""
    rows, N, K, _ = shape
    gen = torch.Generator().manual_seed(4242 + seed)
    return (torch.randn(rows, K, generator=gen), torch.randn(N, K, generator=gen) / K ** 0.5, 0.3 * torch.randn(N, generator=gen),
            torch.randn(rows, N, generator=gen))


# ------------------------------------------------------------------------------------------------------ the step
def mmd_terms(x, y):
    def k(a, b):
        return torch.exp(-(a.unsqueeze(1) - b.unsqueeze(0)).pow(2).mean(dim=2) / a.shape[1])
    kxx, kyy, kxy = k(x, x).mean(), k(y, y).mean(), k(x, y).mean()
    return kxx, kyy, kxy, kxx + kyy - 2 * kxy


def _pack(recon, z, sse, terms, loss, grads):
    sums = torch.zeros(16, dtype=torch.float64)
    sums[0] = float(sse.detach())
    for i, t in enumerate(terms):
        sums[12 + i] = float(t.detach())
    return {"recon": recon.detach().double(), "z": z.detach().double(), "loss": float(loss), "sums": sums,
            "grads": None if grads is None else {k: v.detach().double() for k, v in grads.items()}}


def torch_step(sd, x, ts, lambda_x=1.0, lambda_mmd=1.0, dtype=torch.float64):
    """the reference formulation under autograd in ``dtype`` -> {"recon", "z", "loss", "sums", "grads"}"""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    x, ts = x.to(dtype), ts.to(dtype)
    recon, z = C.infovae_forward(leaves, x)
    terms = mmd_terms(ts, z)
    loss = lambda_x * F.mse_loss(recon, x) + lambda_mmd * terms[3]
    grads = torch.autograd.grad(loss, [leaves[k] for k in NAMES])
    return _pack(recon, z, (recon - x).pow(2).sum(), terms, loss.detach(), dict(zip(NAMES, grads)))


class _Lin(torch.autograd.Function):
    """act(x W^T + b) as the kernels compute it: ``perm`` "k" reads x channels-last, "n" writes y (and reads its gradient)
    channels-last; the backward from the saved output"""

    @staticmethod
    def forward(ctx, x, w, b, kind, slope, perm, fault, tag):
        drop = fault == "perm_" + tag
        xw = from_cl(x) if perm == "k" and not drop else x
        y = act(xw @ w.t() + b, kind, slope)
        out = to_cl(y) if perm == "n" and not drop else y
        ctx.save_for_backward(xw, w, out)
        ctx.cfg = (kind, slope, perm, fault, drop)
        return out.clone()

    @staticmethod
    def backward(ctx, g):
        xw, w, out = ctx.saved_tensors
        kind, slope, perm, fault, drop = ctx.cfg
        q = gp(g, out, kind, slope, fault)
        if perm == "n" and not drop:
            q = from_cl(q)
        dx = q @ w
        if perm == "k" and not drop:
            dx = to_cl(dx)
        rows = q.shape[0] - 1 if fault == "last_row" else q.shape[0]
        dw = q[:rows].t() @ xw[:rows]
        db = torch.zeros_like(q[0]) if fault == "no_db" else q.sum(0)
        return dx, dw, db, None, None, None, None, None


def step(sd, x, ts, lambda_x=1.0, lambda_mmd=1.0, emulate=False, fault=None):
    """float64 restatement of mmvae_mnist_infovae_step on float64 copies of ``sd`` -> {"recon", "z", "loss", "sums", "grads"}"""
    leaves = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    x, ts = x.double(), ts.double()
    B = x.shape[0]
    slope = C.slope32(0.1) if emulate else 0.1
    if emulate:
        h = C.qdown(C.qdown(x, leaves[NAMES[0]], "leaky", 0.1), leaves[NAMES[1]], "leaky", 0.1)
    else:
        h = F.leaky_relu(F.conv2d(F.leaky_relu(F.conv2d(x, leaves[NAMES[0]], stride=2, padding=1), 0.1), leaves[NAMES[1]], stride=2, padding=1), 0.1)
    h = h.permute(0, 2, 3, 1).reshape(B, PERM_P * PERM_C)                       # channels-last, as conv4s2 leaves it
    a1 = _Lin.apply(h, leaves[NAMES[2]], leaves[NAMES[3]], "leaky", slope, "k", fault, "efc0")
    z = _Lin.apply(a1, leaves[NAMES[4]], leaves[NAMES[5]], "none", 0.0, None, fault, "efc2")
    d1 = _Lin.apply(z, leaves[NAMES[6]], leaves[NAMES[7]], "relu", 0.0, None, fault, "dfc0")
    d2 = _Lin.apply(d1, leaves[NAMES[8]], leaves[NAMES[9]], "relu", 0.0, "n", fault, "dfc2")
    h = d2.reshape(B, 7, 7, PERM_C).permute(0, 3, 1, 2)
    if emulate:
        recon = C.qup(C.qup(h, leaves[NAMES[10]], "relu"), leaves[NAMES[11]], "sigmoid")
    else:
        recon = torch.sigmoid(F.conv_transpose2d(torch.relu(F.conv_transpose2d(h, leaves[NAMES[10]], stride=2, padding=1)),
                                                 leaves[NAMES[11]], stride=2, padding=1))
    sse = (recon - x).pow(2).sum()
    terms = mmd_terms(ts, z)
    loss = lambda_x * sse / (B * 784) + lambda_mmd * terms[3]
    # the objective whose gradient the step forms
    coef = lambda_x / B if fault == "mse_no_784" else lambda_x / (B * 784)
    lm = 1.0 if fault == "lambda_mmd_ignored" else lambda_mmd
    if fault == "mmd_dropped":
        term = terms[3].detach()
    elif fault == "mmd_wrong_class":                        # dMMD/d(prior samples) handed to z
        tsv = ts.clone().requires_grad_(True)
        (wrong,) = torch.autograd.grad(mmd_terms(tsv, z.detach())[3], tsv)
        term = (z * wrong).sum()
    else:
        term = terms[3]
    obj = coef * sse + lm * term
    grads = dict(zip(NAMES, torch.autograd.grad(obj, [leaves[k] for k in NAMES], allow_unused=True)))
    grads = {k: torch.zeros_like(leaves[k]) if v is None else v for k, v in grads.items()}
    return _pack(recon, z, sse, terms, loss.detach(), grads)


def tensors(out):
    """the per-tensor view the whole-step gate runs over: recon, z, loss and the 12 gradients"""
    t = {"recon": out["recon"], "z": out["z"], "loss": torch.tensor([out["loss"]], dtype=torch.float64)}
    t.update(out["grads"])
    return t


def step_yardsticks(sd32, x, ts, lambda_x, lambda_mmd):
    """-> (float64 reference, {tensor: E_emu}, {tensor: E_f32}, {tensor: gate}) for float32 weights ``sd32``"""
    ref = step(sd32, x, ts, lambda_x, lambda_mmd)
    emu = step(sd32, x, ts, lambda_x, lambda_mmd, emulate=True)
    f32 = torch_step(sd32, x, ts, lambda_x, lambda_mmd, torch.float32)
    r, e, f = tensors(ref), tensors(emu), tensors(f32)
    e_emu = {k: float((e[k] - r[k]).abs().max()) for k in r}
    e_f32 = {k: float((f[k] - r[k]).abs().max()) for k in r}
    gates = {k: 2 * e_emu[k] + C_STEP * e_f32[k] for k in r}
    return ref, e_emu, e_f32, gates
