"""Float64 restatement of the MultiMNIST text-only VAE (multimnist/model.py:123-147 TextVAE: TextEncoder :219-247, TextDecoder
:250-307, reparametrize, loss_function of multimnist/train.py:69-87 with the text term alone) at ANY hidden size H, with the
bf16-operand emulation and the comparisons of tests/test_gpu_textonly_mm.py (on the MI355X) and tests/test_cpu_textonly_mm.py.

Parameters live under TextVAE's own names (``encoder.*`` / ``decoder.*``).  With ``rounded=True`` the restatement rounds to bf16
exactly the GEMM operands csrc/text.hip rounds (every weight matrix, the embedded token, the copies of the GRU states fed to W_hh,
the dropped-out layer-0 output, the ``[h1 | z]`` operand of the output projection and z); biases, gate math, softmax and all sums
stay float64.  The gate of a module comparison is GATE_FACTOR (tests/text_ref.py: 4) times what that emulation differs from the
unrounded result on the same inputs at the same H; nothing is taken from the engine.

``fault`` makes the restatement a stand-in engine with one defect, to show without a GPU that the comparisons see it:
  "last_column"  the decoder ignores latent column D-1
  "row16"        row 16 of every output is answered with row 0's
  "mask"         the keep masks are ignored
  "unit"         hidden unit H-1 of every GRU state is left out (a stale hidden-size bound)
Nothing here needs a GPU."""
import torch
import torch.nn.functional as F

from oracle import mmvae_ref as R
from text_ref import GATE_FACTOR, _RoundBf16, _affine, _ident, rel_l2

T = R.MAX_LENGTH
V = R.N_CHARACTERS
ENC, DEC = "encoder.", "decoder."
FAULTS = ("last_column", "row16", "mask", "unit")


def param_shapes(D, H):
    """TextVAE(D).state_dict() names and shapes at hidden size H, in order (multimnist/model.py:123-128, 223-231, 254-262)"""
    s = [(ENC + "embed.weight", (V, H))]
    for sfx in ("l0", "l0_reverse"):
        s += [(ENC + "gru.weight_ih_" + sfx, (3 * H, H)), (ENC + "gru.weight_hh_" + sfx, (3 * H, H)),
              (ENC + "gru.bias_ih_" + sfx, (3 * H,)), (ENC + "gru.bias_hh_" + sfx, (3 * H,))]
    s += [(ENC + "h2p.weight", (2 * D, H)), (ENC + "h2p.bias", (2 * D,)),
          (DEC + "embed.weight", (V, H)), (DEC + "z2h.weight", (H, D)), (DEC + "z2h.bias", (H,))]
    for sfx, inp in (("l0", H + D), ("l1", H)):
        s += [(DEC + "gru.weight_ih_" + sfx, (3 * H, inp)), (DEC + "gru.weight_hh_" + sfx, (3 * H, H)),
              (DEC + "gru.bias_ih_" + sfx, (3 * H,)), (DEC + "gru.bias_hh_" + sfx, (3 * H,))]
    s += [(DEC + "h2o.weight", (V, H + D)), (DEC + "h2o.bias", (V,))]
    return s


def make_params(D, H, seed=0, out_scale=1.0):
    """float32 parameters in PyTorch's default scales (uniform +-1/sqrt(fan) for GRU / Linear, N(0,1) embeddings).  ``out_scale``
    multiplies decoder.h2o.weight: wider logit margins for the free-running comparison."""
    g = torch.Generator().manual_seed(7000 + 17 * D + H + seed)
    P = {}
    for name, shape in param_shapes(D, H):
        if name.endswith("embed.weight"):
            P[name] = torch.randn(shape, generator=g)
        else:
            fan = H if ".gru." in name else (shape[1] if len(shape) == 2 else {ENC + "h2p.bias": H, DEC + "z2h.bias": D, DEC + "h2o.bias": H + D}[name])
            P[name] = (torch.rand(shape, generator=g) * 2 - 1) / fan ** 0.5
    P[DEC + "h2o.weight"] *= out_scale
    return P


def f64(P, requires_grad=False):
    return {k: v.detach().double().clone().requires_grad_(requires_grad) for k, v in P.items()}


def _gru_cell(x, h, w_ih, w_hh, b_ih, b_hh, q, rowwise, fault=None):
    H = h.shape[1]
    gi = _affine(q(x), q(w_ih), b_ih, rowwise)
    gh = _affine(q(h), q(w_hh), b_hh, rowwise)
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    out = (1 - z) * n + z * h
    if fault == "unit":
        m = torch.ones(H, dtype=out.dtype)
        m[H - 1] = 0
        out = out * m
    return out


def encoder(p, text, rounded=False, rowwise=False, fault=None):
    """TextEncoder.forward -> (B, 2D): embedding, bidirectional GRU, the last time step's two halves added, h2p"""
    q = _RoundBf16.apply if rounded else _ident
    g = ENC + "gru."
    H = p[ENC + "embed.weight"].shape[1]
    emb = p[ENC + "embed.weight"][text]
    h = emb.new_zeros(emb.shape[0], H)
    for t in range(T):
        h = _gru_cell(emb[:, t], h, p[g + "weight_ih_l0"], p[g + "weight_hh_l0"], p[g + "bias_ih_l0"], p[g + "bias_hh_l0"], q, rowwise, fault)
    hb = _gru_cell(emb[:, T - 1], emb.new_zeros(emb.shape[0], H), p[g + "weight_ih_l0_reverse"], p[g + "weight_hh_l0_reverse"],
                   p[g + "bias_ih_l0_reverse"], p[g + "bias_hh_l0_reverse"], q, rowwise, fault)
    return _affine(q(h + hb), q(p[ENC + "h2p.weight"]), p[ENC + "h2p.bias"], rowwise, True)


def decoder(p, z, keep=None, force_tokens=None, rounded=False, rowwise=False, fault=None):
    """TextDecoder.forward with the keep masks keep[t] (None: no dropout, eval mode) -> (log-probs (B,4,12), greedy tokens (B,4))"""
    q = _RoundBf16.apply if rounded else _ident
    g = DEC + "gru."
    if fault == "last_column":
        col = torch.ones(z.shape[1], dtype=z.dtype)
        col[-1] = 0
        z = z * col
    if fault == "mask":
        keep = None
    n = z.shape[0]
    c_in = torch.full((n,), R.SOS, dtype=torch.long)
    h0 = _affine(q(z), q(p[DEC + "z2h.weight"]), p[DEC + "z2h.bias"], rowwise, True)
    h = [h0, h0]
    words, toks = [], []
    for i in range(T):
        x = torch.cat((R.swish(p[DEC + "embed.weight"][c_in]), z), dim=1)
        h[0] = _gru_cell(x, h[0], p[g + "weight_ih_l0"], p[g + "weight_hh_l0"], p[g + "bias_ih_l0"], p[g + "bias_hh_l0"], q, rowwise, fault)
        mid = h[0]
        if keep is not None:
            mid = R.dropout(mid, True, keep[i])
        h[1] = _gru_cell(mid, h[1], p[g + "weight_ih_l1"], p[g + "weight_hh_l1"], p[g + "bias_ih_l1"], p[g + "bias_hh_l1"], q, rowwise, fault)
        o = _affine(q(torch.cat((h[1], z), dim=1)), q(p[DEC + "h2o.weight"]), p[DEC + "h2o.bias"], rowwise, True)
        lp = F.log_softmax(o, dim=1)
        words.append(lp)
        tok = lp.argmax(dim=1)
        toks.append(tok)
        c_in = tok if force_tokens is None else force_tokens[:, i]
    return torch.stack(words, dim=1), torch.stack(toks, dim=1)


def vae_loss(p, text, eps=None, keep=None, force_tokens=None, kl_lambda=1e-3, lambda_y=1.0, rounded=False):
    """TextVAE.forward + loss_function(mu, logvar, recon_text=, text=, kl_lambda=, lambda_yx=lambda_y) (train_textonly.py:104-106).
    ``eps`` None: eval mode (z = mu).  -> (loss, dict(mu, logvar, words, tokens, nll_sum, kl_sum))"""
    out = encoder(p, text, rounded)
    D = out.shape[1] // 2
    mu, logvar = out[:, :D], out[:, D:]
    z = mu if eps is None else eps * torch.exp(0.5 * logvar) + mu
    words, toks = decoder(p, z, keep, force_tokens, rounded)
    B = text.shape[0]
    nll_sum = -words.reshape(B * T, V).gather(1, text.reshape(-1, 1)).sum()
    kl_sum = -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp())
    loss = lambda_y * nll_sum / (B * T) + kl_lambda * kl_sum / B
    return loss, dict(mu=mu, logvar=logvar, words=words, tokens=toks, nll_sum=nll_sum, kl_sum=kl_sum)


def run_step(P32, text, eps, keep, force, kl_lambda=1e-3, lambda_y=1.0, rounded=False):
    """one training step's loss and gradients in float64 -> dict(loss, mu, logvar, words, tokens, nll_sum, kl_sum, grads)"""
    P = f64(P32, requires_grad=True)
    k = None if keep is None else [keep[t].double() for t in range(T)]
    loss, o = vae_loss(P, text, None if eps is None else eps.double(), k, force, kl_lambda, lambda_y, rounded)
    loss.backward()
    res = {n: (v.detach() if torch.is_tensor(v) else v) for n, v in o.items()}
    res["loss"] = float(loss.detach())
    res["grads"] = {n: (v.grad if v.grad is not None else torch.zeros_like(v)) for n, v in P.items()}
    return res


# ------------------------------------------------------------------------------------------------ module comparisons
def make_inputs(D, H, n=23, seed=0):
    g = torch.Generator().manual_seed(9100 + 131 * D + H + seed)
    return dict(
        z=torch.randn(n, D, generator=g),
        text=torch.randint(0, V, (n, T), generator=g),
        force=torch.randint(0, V, (n, T), generator=g),
        keep=(torch.rand(T, n, H, generator=g) >= R.DROP_P).to(torch.uint8),
        gw=torch.randn(n, T, V, generator=g),
        ge=torch.randn(n, 2 * D, generator=g))


def take_rows(inp, rows):
    rows = torch.as_tensor(rows, dtype=torch.long)
    out = {k: v[rows].contiguous() for k, v in inp.items() if k != "keep"}
    out["keep"] = inp["keep"][:, rows].contiguous()
    return out


def _row16(t, fault):
    if fault == "row16" and t.shape[0] > 16:
        t = t.clone()
        t[16] = t[0]
    return t


def run_forward(P32, inp, rounded=False, fault=None, free_running=False, rowwise=False, eval_mode=False):
    P = f64(P32)
    keep = None if eval_mode else [inp["keep"][t].double() for t in range(T)]
    with torch.no_grad():
        words, toks = decoder(P, inp["z"].double(), keep, None if free_running else inp["force"], rounded, rowwise, fault)
        enc = encoder(P, inp["text"], rounded, rowwise, fault)
    return dict(words=_row16(words, fault), tokens=_row16(toks, fault), encout=_row16(enc, fault))


def run_full(P32, inp, rounded=False, fault=None):
    """forward and backward of both modules (forced tokens, keep masks, the upstream gradients of ``inp``)"""
    P = f64(P32, requires_grad=True)
    z = inp["z"].double().requires_grad_(True)
    keep = [inp["keep"][t].double() for t in range(T)]
    words, toks = decoder(P, z, keep, inp["force"], rounded, False, fault)
    enc = encoder(P, inp["text"], rounded, False, fault)
    ((words * inp["gw"].double()).sum() + (enc * inp["ge"].double()).sum()).backward()
    return dict(words=_row16(words.detach(), fault), tokens=_row16(toks, fault), encout=_row16(enc.detach(), fault),
                dz=_row16(z.grad, fault), grads={k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in P.items()})


def errors(got, ref):
    """words and encoder output element-wise (max abs), dz and every parameter gradient by relative L2"""
    by = {k: rel_l2(got["grads"][k].cpu(), ref["grads"][k]) for k in ref["grads"] if float(ref["grads"][k].abs().max()) > 0}
    worst = max(by, key=by.get)
    return dict(words=float((got["words"].double().cpu() - ref["words"]).abs().max()),
                encout=float((got["encout"].double().cpu() - ref["encout"]).abs().max()),
                dz=rel_l2(got["dz"].cpu(), ref["dz"]), grads=by[worst], grads_worst=worst, grads_by_name=by)


def gates(P32, inp, ref=None):
    """GATE_FACTOR times the emulation's own distance from the unrounded result on these inputs -> (gates, reference, emulation errors)"""
    ref = run_full(P32, inp) if ref is None else ref
    e = errors(run_full(P32, inp, rounded=True), ref)
    return {k: GATE_FACTOR * e[k] for k in ("words", "encout", "dz", "grads")}, ref, e


def violations(got, ref, gate, what=""):
    e = errors(got, ref)
    bad = ["%s %s: %.3e > gate %.3e" % (what, k, e[k], gate[k]) for k in ("words", "encout", "dz") if not e[k] <= gate[k]]
    bad += ["%s grad %s: %.3e > gate %.3e" % (what, n, v, gate["grads"]) for n, v in e["grads_by_name"].items() if not v <= gate["grads"]]
    # a gradient that is exactly 0 in the reference (the reverse direction's W_hh: one step from h = 0) must be exactly 0
    bad += ["%s grad %s: must be exactly 0" % (what, n) for n, v in ref["grads"].items()
            if float(v.abs().max()) == 0 and float(got["grads"][n].abs().max()) != 0]
    return bad, e


def free_running_margin(P32, inp):
    """the smallest top-two log-prob margin over every (row, step) of the free-running float64 decoder (train-mode keep masks)"""
    w = run_forward(P32, inp, free_running=True)["words"]
    top = w.topk(2, dim=-1).values
    return float((top[..., 0] - top[..., 1]).min())


def wide_margin_inputs(P32, D, H, n=23, pool=600, seed=0):
    """Inputs for the free-running comparison: of ``pool`` candidate rows, the n whose smallest top-two margin over the four steps is
    widest in float64 (rows are independent, so a row's margin does not depend on its batch-mates)."""
    cand = make_inputs(D, H, pool, seed=seed + 1)
    w = run_forward(P32, cand, free_running=True)["words"]
    top = w.topk(2, dim=-1).values
    m = (top[..., 0] - top[..., 1]).min(dim=1).values
    rows = torch.argsort(m, descending=True)[:n].sort().values
    return take_rows(cand, rows.tolist())


def free_running_case(D, H, tries=8):
    """Parameters (h2o scaled by 8) and inputs of the free-running comparison, chosen from float64 alone: the first of ``tries``
    seeds whose smallest top-two margin is at least 10 x the words gate of those inputs.  -> (P, inputs, float64 result, margin,
    words gate); the caller asserts the condition"""
    for seed in range(tries):
        P = make_params(D, H, seed=seed, out_scale=8.0)
        inp = wide_margin_inputs(P, D, H, seed=seed)
        ref = run_forward(P, inp, free_running=True)
        emu = run_forward(P, inp, rounded=True, free_running=True)
        g_words = GATE_FACTOR * float((emu["words"] - ref["words"]).abs().max())
        margin = free_running_margin(P, inp)
        if margin >= 10 * g_words:
            break
    return P, inp, ref, margin, g_words


def row_independence_violations(forward, inp):
    """words, tokens and the encoder output of a row must be bit-for-bit the same whatever the batch around it: the full batch (23
    rows) against its first 16 rows, rows 16..22 moved to the front, a permutation, and single rows"""
    n = inp["z"].shape[0]
    full = forward(inp)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5)).tolist()
    cases = (("first 16 rows", list(range(16))), ("rows 16.. in front", list(range(16, n))), ("permutation", perm),
             ("row 0 alone", [0]), ("last row alone", [n - 1]), ("row 16 alone", [16]), ("sub-batch of 5", [n - 1, 5, 16, 0, 9]))
    bad = []
    for name, rows in cases:
        part = forward(take_rows(inp, rows))
        for k in ("words", "tokens", "encout"):
            a, b = part[k].cpu(), full[k].cpu()[torch.as_tensor(rows)]
            if not torch.equal(a, b):
                bad.append("%s: %s differs" % (name, k))
    return bad


def embed_into(P50, D, H_small=50, H_big=100):
    """The H_small parameters placed into an H_big model with every added row and column zero: the same function of (text, z).
    Gate-major weights: gate g's rows [g*H_small, (g+1)*H_small) go to [g*H_big, g*H_big + H_small).  -> (parameters, masks), masks
    1 where an entry is one of the added ones"""
    hs, hb = H_small, H_big
    Q, M = {}, {}

    def rows3(x):          # (3*hs, ...) -> (3*hb, ...)
        out = x.new_zeros((3 * hb,) + tuple(x.shape[1:]))
        for g in range(3):
            out[g * hb:g * hb + hs] = x[g * hs:(g + 1) * hs]
        return out

    def cols_h(x, tail=0):  # (..., hs + tail) -> (..., hb + tail): hidden columns first, then `tail` latent columns
        out = x.new_zeros(tuple(x.shape[:-1]) + (hb + tail,))
        out[..., :hs] = x[..., :hs]
        if tail:
            out[..., hb:] = x[..., hs:]
        return out

    for name, shape in param_shapes(D, hs):
        x = P50[name]
        if name.endswith("embed.weight"):
            y = cols_h(x)
        elif ".gru.weight_ih_l0" in name and name.startswith(DEC) and not name.endswith("reverse"):
            y = rows3(cols_h(x, D))
        elif ".gru.weight_" in name:
            y = rows3(cols_h(x))
        elif ".gru.bias_" in name:
            y = rows3(x)
        elif name == ENC + "h2p.weight":
            y = cols_h(x)
        elif name == DEC + "z2h.weight" or name == DEC + "z2h.bias":
            y = x.new_zeros((hb,) + tuple(x.shape[1:]))
            y[:hs] = x
        elif name == DEC + "h2o.weight":
            y = cols_h(x, D)
        else:
            y = x.clone()
        one = torch.ones_like(x)
        if name.endswith("embed.weight"):
            m = cols_h(one)
        elif ".gru.weight_ih_l0" in name and name.startswith(DEC) and not name.endswith("reverse"):
            m = rows3(cols_h(one, D))
        elif ".gru.weight_" in name:
            m = rows3(cols_h(one))
        elif ".gru.bias_" in name:
            m = rows3(one)
        elif name == ENC + "h2p.weight":
            m = cols_h(one)
        elif name == DEC + "z2h.weight" or name == DEC + "z2h.bias":
            m = one.new_zeros((hb,) + tuple(x.shape[1:]))
            m[:hs] = 1
        elif name == DEC + "h2o.weight":
            m = cols_h(one, D)
        else:
            m = one
        Q[name], M[name] = y, (m == 0)
    return Q, M


def extract_from(G100, M):
    """the entries of the big model's tensors that are NOT added ones, flattened, per name"""
    return {n: G100[n][~M[n]] for n in M}
