"""float64 restatement of MNIST's uni-modal image VAE (mnist/model.py:188-232), its loss (mnist/imageonly/train_imageonly.py:60-71)
and one Adam step, in plain torch ops, and the gates the GPU tests hold the HIP step to.

    encoder: Linear(784,400) -> BatchNorm1d -> ReLU -> Linear(400,200) -> BatchNorm1d -> ReLU -> Linear(200, 2 D)
    mu | logvar = the two halves of the encoder's output (no product of experts: no 1e-8)
    z = mu + eps exp(logvar / 2) in train mode, mu in eval mode
    decoder: Linear(D,200) -> BatchNorm1d -> ReLU -> Linear(200,400) -> BatchNorm1d -> ReLU -> Linear(400,784) -> sigmoid
    loss = (mean over B * 784 elements of BCE + KLD / 784) / B,   KLD = -sum(1 + logvar - mu^2 - exp(logvar)) / 2

BatchNorm1d in train mode normalises with the biased batch variance and moves the running statistics by momentum 0.1 towards the
batch mean and the UNBIASED batch variance; in eval mode it normalises with the running statistics and leaves them alone.

``run`` evaluates all of it in a chosen dtype, with an optional ``fault`` (a dropped loss term, a dropped 1 / B, a dropped BatchNorm
update, ...): ``check`` -- the gates of tests/test_gpu_mnist.py for the same quantities -- must pass a float32 run of the same
formulas and must see every fault (tests/test_cpu_imageonly_mnist.py).  Parameter values come from the oracle's hash
(``formula_params("mnist", D)``: the image half of the MMVAE's table), inputs from ``formula_inputs`` / ``formula_eps``.
"""
import json
import math
import os

import torch

from oracle import mmvae_ref as R

BN_EPS, BN_MOM = 1e-5, 0.1
HALVES = (("encoder", "image_encoder.net."), ("decoder", "image_decoder.net."))
# Linear biases in front of a BatchNorm: the batch mean is subtracted, their exact gradient is 0 (tests/test_gpu_mnist.py:30-33)
PRE_BN_BIAS = ("image_encoder.net.0.bias", "image_encoder.net.3.bias", "image_decoder.net.0.bias", "image_decoder.net.3.bias")
BN_PREFIXES = ("image_encoder.net.1", "image_encoder.net.4", "image_decoder.net.1", "image_decoder.net.4")
FAULTS = ("no_kl", "no_bce", "no_1_over_B", "no_bn_update", "biased_running_var", "eval_draws_eps")
# (B, D) of the step tests: every batch size and every latent size the kernels branch on, once.  ReLU makes the gradient
# discontinuous where a BatchNorm output is 0, so a case is only a yardstick where every ReLU decision of the float64 run is out of
# reach of fp32 rounding: RELU_MARGIN is the least |BatchNorm output| a case may have (fp32 noise there is ~1e-6; at (23, 124) the
# formula inputs put one at 1.8e-6 and torch's own float32 run of these formulas then moves image_decoder.net.0.weight.grad by 1.5 %).
CASES = [(2, 20), (5, 124), (23, 4), (33, 20), (128, 20)]
RELU_MARGIN = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mnist_vae_keys.json")


def image_names(D):
    """The MMVAE plan's names of the image half, in table order (they lead the table)."""
    return [n for n, _ in R.param_table("mnist", D) if n.startswith(("image_encoder.", "image_decoder."))]


def recorded_keys():
    """[key, shape] of the reference's ``VAE(20).state_dict()`` (tests/golden/mnist_vae_keys.json, tools/record_mnist_vae_keys.py)"""
    with open(GOLDEN) as fp:
        return [(k, tuple(s)) for k, s in json.load(fp)["state_dict"]]


def plan_name(key):
    half, rest = key.split(".", 1)
    return dict(HALVES)[half] + rest


def params(D, dtype=torch.float64, requires_grad=False):
    """name -> tensor of the image half (parameters and BatchNorm buffers) under the plan's names"""
    p = R.formula_params("mnist", D)
    out = {}
    for n, v in p.items():
        if not n.startswith(("image_encoder.", "image_decoder.")):
            continue
        if v.dtype == torch.long:
            out[n] = v.clone()
        else:
            out[n] = v.detach().to(dtype).clone()
            if requires_grad and n in image_names(D):
                out[n].requires_grad_(True)
    return out


def _stack(p, x, pre, training, fault=None, margins=None):
    for lin, bn in ((0, 1), (3, 4)):
        y = x @ p["%s%d.weight" % (pre, lin)].t() + p["%s%d.bias" % (pre, lin)]
        rm, rv = p["%s%d.running_mean" % (pre, bn)], p["%s%d.running_var" % (pre, bn)]
        if training:
            n = y.shape[0]
            if n <= 1:
                raise ValueError("Expected more than 1 value per channel when training")
            mean = y.mean(0)
            var = ((y - mean) ** 2).mean(0)
            if fault != "no_bn_update":
                with torch.no_grad():
                    rm.mul_(1 - BN_MOM).add_(BN_MOM * mean)
                    rv.mul_(1 - BN_MOM).add_(BN_MOM * (var if fault == "biased_running_var" else var * n / (n - 1)))
                    p["%s%d.num_batches_tracked" % (pre, bn)] += 1
        else:
            mean, var = rm, rv
        a = (y - mean) / torch.sqrt(var + BN_EPS) * p["%s%d.weight" % (pre, bn)] + p["%s%d.bias" % (pre, bn)]
        if margins is not None:
            margins.append(float(a.detach().abs().min()))
        x = torch.relu(a)
    return x @ p[pre + "6.weight"].t() + p[pre + "6.bias"]


def forward(p, image, training, eps=None, fault=None, with_logits=False, margins=None):
    """-> (recon (B,784), mu, logvar[, the pre-sigmoid logits])"""
    dt = p["image_encoder.net.0.weight"].dtype
    o = _stack(p, image.reshape(-1, 784).to(dt), "image_encoder.net.", training, fault, margins)
    D = o.shape[1] // 2
    mu, logvar = o[:, :D], o[:, D:]
    z = mu + eps.to(dt) * torch.exp(0.5 * logvar) if (training or fault == "eval_draws_eps") and eps is not None else mu
    logits = _stack(p, z, "image_decoder.net.", training, fault, margins)
    return (torch.sigmoid(logits), mu, logvar) + ((logits,) if with_logits else ())


def kl_sum(mu, logvar):
    return -0.5 * torch.sum(1 + logvar - mu * mu - torch.exp(logvar))


def bce_mean(recon, x):
    """F.binary_cross_entropy: the mean over every element, each log clamped at -100"""
    x = x.reshape(recon.shape).to(recon.dtype)
    return -(x * torch.log(recon).clamp(min=-100) + (1 - x) * torch.log(1 - recon).clamp(min=-100)).mean()


def bce_mean_from_logits(logits, x):
    """The same mean from the pre-sigmoid logit l: softplus(l) - x l (equal to bce_mean wherever neither log is clamped, and without
    the cancellation of 1 - sigmoid(l) in a narrow format: the form the engine's sigmoid + BCE kernel evaluates)"""
    x = x.reshape(logits.shape).to(logits.dtype)
    return (torch.nn.functional.softplus(logits) - x * logits).mean()


def loss_function(recon, x, mu, logvar, fault=None, logits=None):
    B = recon.shape[0]
    bce = 0.0 if fault == "no_bce" else bce_mean(recon, x) if logits is None else bce_mean_from_logits(logits, x)
    kld = 0.0 if fault == "no_kl" else kl_sum(mu, logvar)
    total = bce + kld / 784
    return total if fault == "no_1_over_B" else total / B


def adam(p, g, step=1, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, m=None, v=None):
    """torch.optim.Adam's update of one tensor from zero (or given) moments -> (p', m', v')"""
    m = torch.zeros_like(p) if m is None else m
    v = torch.zeros_like(p) if v is None else v
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1 - b2 ** step) + eps
    return p - lr / (1 - b1 ** step) * m / denom, m, v


def inputs(B, D):
    return R.formula_inputs("mnist", B)[0].reshape(B, 784), R.formula_eps(B, D, 1)


def relu_margin(D, B, training=True):
    """The least |ReLU input| of the float64 forward on the test's inputs"""
    image, eps = inputs(B, D)
    margins = []
    with torch.no_grad():
        forward(params(D), image, training, eps, margins=margins)
    return min(margins)


def run(D, B, training=True, dtype=torch.float64, fault=None, lr=1e-3):
    """One step (train mode: forward, backward, one Adam update from zero moments; eval mode: the forward) -> dict of CPU tensors:
    loss, mu, logvar, recon, kl, grads {name}, params_after {name}, running {name}, nbt {prefix}."""
    image, eps = inputs(B, D)
    p = params(D, dtype, requires_grad=training)
    recon, mu, logvar, logits = forward(p, image, training, eps, fault, with_logits=True)
    # float64: the reference's literal formula; a narrower dtype stands in for the engine and takes the loss from the logits as it does
    loss = loss_function(recon, image, mu, logvar, fault, logits=None if dtype == torch.float64 else logits)
    out = dict(loss=float(loss.detach()), mu=mu.detach(), logvar=logvar.detach(), recon=recon.detach(), kl=float(kl_sum(mu, logvar).detach()))
    names = image_names(D)
    if training:
        loss.backward()
        grads = {n: (torch.zeros_like(p[n]) if p[n].grad is None else p[n].grad.detach().clone()) for n in names}      # (None: no path to the loss)
        out["grads"] = grads
        out["params_after"] = {n: adam(p[n].detach(), grads[n], lr=lr)[0] for n in names}
    out["running"] = {k: v.detach().clone() for k, v in p.items() if k.endswith(("running_mean", "running_var"))}
    out["nbt"] = {k[:-len(".num_batches_tracked")]: int(v) for k, v in p.items() if k.endswith("num_batches_tracked")}
    return out


def check(ref, got, training=True):
    """The gates tests/test_gpu_mnist.py applies to the fp32 plan, on ``got`` (same layout as ``run``'s result, any float dtype)
    against the float64 ``ref``.  -> (list of failed gates, {gate: worst measured / allowed})"""
    fails, ratios = [], {}

    def gate(name, err, allowed):
        r = float(err) / max(float(allowed), 1e-300)
        ratios[name] = max(ratios.get(name, 0.0), r)
        if not r <= 1.0:
            fails.append("%s: %.3e > %.3e" % (name, float(err), float(allowed)))

    d = lambda t: t.detach().double().cpu()
    gate("loss rtol 2e-5", abs(got["loss"] - ref["loss"]), 2e-5 * abs(ref["loss"]))
    gate("kl rtol 2e-5", abs(got["kl"] - ref["kl"]), 2e-5 * abs(ref["kl"]))
    gate("mu atol 1e-4", (d(got["mu"]) - ref["mu"]).abs().max(), 1e-4)
    gate("logvar atol 1e-4", (d(got["logvar"]) - ref["logvar"]).abs().max(), 1e-4)
    gate("recon atol 1e-5", (d(got["recon"]) - ref["recon"]).abs().max(), 1e-5)
    for k, v in ref["running"].items():
        e = (d(got["running"][k]) - v).abs()
        if k.endswith("running_mean"):
            gate("running_mean atol 1e-5", e.max(), 1e-5)
        else:
            gate("running_var rtol 1e-4 atol 1e-6", (e - 1e-4 * v.abs()).max(), 1e-6)
    for k, v in ref["nbt"].items():
        gate("num_batches_tracked", abs(int(got["nbt"][k]) - v), 0.5)
    if training:
        tot = math.sqrt(sum(float(g.double().pow(2).sum()) for g in ref["grads"].values()))
        for n, g in ref["grads"].items():
            gh = d(got["grads"][n])
            if n in PRE_BN_BIAS:
                gate("pre-BatchNorm bias gradient <= 1e-5", gh.abs().max(), 1e-5)
                continue
            gate("gradient " + n, (gh - g).norm(), 1e-3 * float(g.norm()) + 1e-6 * tot)
            pa, pr = d(got["params_after"][n]), ref["params_after"][n]
            gate("after Adam " + n, abs(float(pa.norm()) - float(pr.norm())), 1e-4 * float(pr.norm()) + 1e-6)
    return fails, ratios
