"""Float64 reference, bf16-operand emulation and comparisons of the MultiMNIST text encoder / decoder on their own
(tests/test_gpu_text_modules.py on the MI355X, tests/test_cpu_text_ref.py without one).

The reference is oracle.mmvae_ref.multimnist_text_encoder / multimnist_text_decoder on float64 parameters.  The emulation below
restates the two modules in float64 and, with ``rounded=True``, rounds to bf16 exactly the GEMM operands csrc/text.hip rounds:
every weight matrix, the embedded token x, the copies of the GRU states fed to W_hh (the fp32 state itself stays unrounded in
the gate math), the dropped-out layer-0 output ``mid``, the ``[h1 | z]`` operand of the output projection and z (in z2h, in
``[c_in | z]`` and in ``[h1 | z]``).  Biases, gate math, softmax and the accumulation stay float64.  With ``rounded=False`` it
is the oracle, operation for operation (tests/test_cpu_text_ref.py asserts equality).

The gate of a comparison comes from this side alone: GATE_FACTOR times what the emulation differs from the unrounded oracle on
the same inputs -- one factor of 2 for the backward's bf16-stored gate gradients (dgi, dgh, dlogit), which the emulation leaves
out, and the project's usual 2 over a measured figure.

``fault`` turns the emulation into a stand-in engine with one defect, to show on the CPU that the comparisons see it:
  "last_column"  the decoder ignores latent column D-1
  "row16"        row 16 of every output is answered with row 0's
  "mask3"        the keep mask of time step 3 is ignored
Nothing here needs a GPU."""
import torch
import torch.nn.functional as F

from oracle import mmvae_ref as R

SIZES = (1, 20, 32, 96, 99, 127)      # latent sizes of the MultiMNIST tests (what each selects: tests/test_gpu_latent_sizes.py)
B = 23                                # 16 + 7 rows: one full and one ragged row tile
H = 100
T = R.MAX_LENGTH
V = R.N_CHARACTERS
GATE_FACTOR = 4.0
ENC, DEC = "text_encoder.", "text_decoder."
FAULTS = ("last_column", "row16", "mask3")


class _RoundBf16(torch.autograd.Function):
    """value rounded to bf16, gradient passed through: the engine's backward GEMMs read the same rounded operand"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def _ident(x):
    return x


def rowwise_mm(x, w):
    """x @ w.t() as a per-row product and sum: the summation order of a row does not depend on how many rows there are
    (a BLAS gemm may block differently at another row count), so the result of a row is bit-for-bit independent of the batch"""
    return (x.unsqueeze(1) * w.unsqueeze(0)).sum(-1)


def _affine(x, w, b, rowwise, linear=False):
    """x w^T + b as the oracle writes it (F.linear for the Linear layers, x @ w.t() + b inside the GRU cell) or row by row"""
    if rowwise:
        return rowwise_mm(x, w) + b
    return F.linear(x, w, b) if linear else x @ w.t() + b


def _gru_cell(x, h, w_ih, w_hh, b_ih, b_hh, q, rowwise):
    gi = _affine(q(x), q(w_ih), b_ih, rowwise)
    gh = _affine(q(h), q(w_hh), b_hh, rowwise)
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return (1 - z) * n + z * h


def text_encoder(p, text, rounded=False, rowwise=False):
    """multimnist/model.py:237-247 -> (B, 2D)"""
    q = _RoundBf16.apply if rounded else _ident
    g = ENC + "gru."
    emb = p[ENC + "embed.weight"][text]
    h = emb.new_zeros(emb.shape[0], H)
    for t in range(T):
        h = _gru_cell(emb[:, t], h, p[g + "weight_ih_l0"], p[g + "weight_hh_l0"], p[g + "bias_ih_l0"], p[g + "bias_hh_l0"], q, rowwise)
    hb = _gru_cell(emb[:, T - 1], emb.new_zeros(emb.shape[0], H), p[g + "weight_ih_l0_reverse"], p[g + "weight_hh_l0_reverse"],
                   p[g + "bias_ih_l0_reverse"], p[g + "bias_hh_l0_reverse"], q, rowwise)
    return _affine(q(h + hb), q(p[ENC + "h2p.weight"]), p[ENC + "h2p.bias"], rowwise, True)


def text_decoder(p, z, keep=None, force_tokens=None, rounded=False, rowwise=False, fault=None):
    """multimnist/model.py:268-307 in train mode with the keep masks keep[t] (None: no dropout) -> (log-probs (B,4,12), greedy
    tokens (B,4))"""
    q = _RoundBf16.apply if rounded else _ident
    g = DEC + "gru."
    if fault == "last_column":
        col = torch.ones(z.shape[1], dtype=z.dtype)
        col[-1] = 0
        z = z * col
    n = z.shape[0]
    c_in = torch.full((n,), R.SOS, dtype=torch.long)
    h0 = _affine(q(z), q(p[DEC + "z2h.weight"]), p[DEC + "z2h.bias"], rowwise, True)
    h = [h0, h0]
    words, toks = [], []
    for i in range(T):
        x = torch.cat((R.swish(p[DEC + "embed.weight"][c_in]), z), dim=1)
        h[0] = _gru_cell(x, h[0], p[g + "weight_ih_l0"], p[g + "weight_hh_l0"], p[g + "bias_ih_l0"], p[g + "bias_hh_l0"], q, rowwise)
        mid = h[0]
        if keep is not None and not (fault == "mask3" and i == 3):
            mid = R.dropout(mid, True, keep[i])
        h[1] = _gru_cell(mid, h[1], p[g + "weight_ih_l1"], p[g + "weight_hh_l1"], p[g + "bias_ih_l1"], p[g + "bias_hh_l1"], q, rowwise)
        o = _affine(q(torch.cat((h[1], z), dim=1)), q(p[DEC + "h2o.weight"]), p[DEC + "h2o.bias"], rowwise, True)
        lp = F.log_softmax(o, dim=1)
        words.append(lp)
        tok = lp.argmax(dim=1)
        toks.append(tok)
        c_in = tok if force_tokens is None else force_tokens[:, i]
    return torch.stack(words, dim=1), torch.stack(toks, dim=1)


# ------------------------------------------------------------------------------------------------ parameters and inputs
def text_params(D):
    """the text_encoder.* / text_decoder.* tensors of the formula initialisation, float32 (what the engine is loaded with)"""
    P = R.formula_params("multimnist", D)
    return {k: v.clone() for k, v in P.items() if k.startswith((ENC, DEC))}


def f64(P, requires_grad=False):
    return {k: v.detach().double().clone().requires_grad_(requires_grad) for k, v in P.items()}


def single_column_params(P, D, col):
    """Every path from z into the decoder is cut except latent column `col`, and that one is scaled by 4: a kernel that drops the
    last k-step or the last column of its z operand returns the z-independent answer, O(1) away."""
    Q = {k: v.clone() for k, v in P.items()}
    for name, lo in ((DEC + "z2h.weight", 0), (DEC + "gru.weight_ih_l0", H), (DEC + "h2o.weight", H)):
        w = Q[name]
        kept = w[:, lo + col].clone() * 4
        w[:, lo:] = 0
        w[:, lo + col] = kept
    return Q


def make_inputs(D, n=B, seed=0):
    """float32 / integer inputs of one comparison: z, the encoder's tokens, forced fed-back tokens, keep masks of the four steps
    and upstream gradients on `words` and on the encoder output"""
    g = torch.Generator().manual_seed(9000 + 131 * D + seed)
    return dict(
        z=torch.randn(n, D, generator=g),
        text=torch.randint(0, V, (n, T), generator=g),
        force=torch.randint(0, V, (n, T), generator=g),
        keep=(torch.rand(T, n, H, generator=g) >= R.DROP_P).to(torch.uint8),
        gw=torch.randn(n, T, V, generator=g),
        ge=torch.randn(n, 2 * D, generator=g))


def take_rows(inp, rows):
    """the inputs of the given rows only, in the given order"""
    rows = torch.as_tensor(rows, dtype=torch.long)
    out = {k: v[rows].contiguous() for k, v in inp.items() if k != "keep"}
    out["keep"] = inp["keep"][:, rows].contiguous()
    return out


# ------------------------------------------------------------------------------------------------ the stand-in engine
def _row16(t, fault):
    if fault == "row16" and t.shape[0] > 16:
        t = t.clone()
        t[16] = t[0]
    return t


def run_forward(P32, inp, rounded=False, fault=None, free_running=False, rowwise=False):
    """forward of both modules in float64 -> dict(words, tokens, encout)"""
    P = f64(P32)
    keep = [inp["keep"][t].double() for t in range(T)]
    with torch.no_grad():
        words, toks = text_decoder(P, inp["z"].double(), keep, None if free_running else inp["force"], rounded, rowwise, fault)
        enc = text_encoder(P, inp["text"], rounded, rowwise)
    return dict(words=_row16(words, fault), tokens=_row16(toks, fault), encout=_row16(enc, fault))


def run_full(P32, inp, rounded=False, fault=None):
    """forward and backward of both modules in float64 (forced tokens, keep masks, the upstream gradients of `inp`)
    -> dict(words, tokens, encout, dz, grads {parameter name: gradient})"""
    P = f64(P32, requires_grad=True)
    z = inp["z"].double().requires_grad_(True)
    keep = [inp["keep"][t].double() for t in range(T)]
    words, toks = text_decoder(P, z, keep, inp["force"], rounded, False, fault)
    enc = text_encoder(P, inp["text"], rounded)
    ((words * inp["gw"].double()).sum() + (enc * inp["ge"].double()).sum()).backward()
    return dict(words=_row16(words.detach(), fault), tokens=_row16(toks, fault), encout=_row16(enc.detach(), fault),
                dz=_row16(z.grad, fault), grads={k: v.grad for k, v in P.items()})


# ------------------------------------------------------------------------------------------------ comparisons
def rel_l2(a, b):
    return float((a.double() - b.double()).norm()) / max(float(b.double().norm()), 1e-300)


def errors(got, ref):
    """what the comparisons measure: words and encoder output element-wise (max abs), dz and every parameter gradient by
    relative L2 (`grads`: the worst tensor; `grads_by_name`: each)"""
    by = {k: rel_l2(got["grads"][k].cpu(), ref["grads"][k]) for k in ref["grads"]}
    worst = max(by, key=by.get)
    return dict(words=float((got["words"].double().cpu() - ref["words"]).abs().max()),
                encout=float((got["encout"].double().cpu() - ref["encout"]).abs().max()),
                dz=rel_l2(got["dz"].cpu(), ref["dz"]), grads=by[worst], grads_worst=worst, grads_by_name=by)


def gates(P32, inp, ref=None):
    """GATE_FACTOR times the emulation's own distance from the unrounded oracle on these inputs -> (gates, oracle result)"""
    ref = run_full(P32, inp) if ref is None else ref
    e = errors(run_full(P32, inp, rounded=True), ref)
    return {k: GATE_FACTOR * e[k] for k in ("words", "encout", "dz", "grads")}, ref, e


def violations(got, ref, gate, what=""):
    """list of the comparisons `got` misses (empty: it passes)"""
    e = errors(got, ref)
    bad = ["%s %s: %.3e > gate %.3e" % (what, k, e[k], gate[k]) for k in ("words", "encout", "dz") if not e[k] <= gate[k]]
    bad += ["%s grad %s: %.3e > gate %.3e" % (what, n, v, gate["grads"]) for n, v in e["grads_by_name"].items() if not v <= gate["grads"]]
    return bad, e


def row_independence_violations(forward, inp):
    """The text path has no BatchNorm and an MFMA output element depends only on its own row of A, so `words`, the greedy tokens
    and the encoder output of a row must be bit-for-bit the same whatever the batch around it.  forward(inputs) -> dict(words,
    tokens, encout) for inputs of any row count.  Compared with the full batch of `inp` (23 rows): its first 16 rows alone, rows
    16..22 alone (moved to the front), a row permutation, and single rows with and without a batch-mate."""
    n = inp["z"].shape[0]
    assert n == B
    full = forward(inp)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5)).tolist()
    cases = (("first 16 rows", list(range(16))), ("rows 16..22 in front", list(range(16, n))), ("permutation", perm),
             ("row 0 alone", [0]), ("row 22 alone", [n - 1]), ("row 16 alone", [16]), ("rows 22, 5 as a pair", [n - 1, 5]))
    bad = []
    for name, rows in cases:
        part = forward(take_rows(inp, rows))
        for k in ("words", "tokens", "encout"):
            a, b = part[k].cpu(), full[k].cpu()[torch.as_tensor(rows)]
            if not torch.equal(a, b):
                diff = (a != b).reshape(len(rows), -1).any(1)
                bad.append("%s: %s differs in rows %s of the part" % (name, k, torch.nonzero(diff).reshape(-1).tolist()[:8]))
    return bad


def single_column_violations(run, P32, D, col, inp):
    """run(P, inputs) -> result of run_full's form on the parameters of single_column_params: `words` and dz[:, col] inside the
    gate of these parameters and inputs, every other column of dz exactly 0"""
    Q = single_column_params(P32, D, col)
    ref = run_full(Q, inp)
    emu = run_full(Q, inp, rounded=True)
    g_words = GATE_FACTOR * float((emu["words"] - ref["words"]).abs().max())
    g_dz = GATE_FACTOR * rel_l2(emu["dz"][:, col], ref["dz"][:, col])
    got = run(Q, inp)
    dz = got["dz"].double().cpu()
    e_words = float((got["words"].double().cpu() - ref["words"]).abs().max())
    e_dz = rel_l2(dz[:, col], ref["dz"][:, col])
    bad = []
    if not e_words <= g_words:
        bad.append("column %d kept: words %.3e > gate %.3e" % (col, e_words, g_words))
    if not e_dz <= g_dz:
        bad.append("column %d kept: dz[:, %d] %.3e > gate %.3e" % (col, col, e_dz, g_dz))
    others = torch.cat((dz[:, :col], dz[:, col + 1:]), 1)
    if others.numel() and not bool((others == 0).all()):
        bad.append("column %d kept: dz is nonzero in %d elements of the cut columns" % (col, int((others != 0).sum())))
    return bad, dict(words=e_words, dz=e_dz, gate_words=g_words, gate_dz=g_dz)
