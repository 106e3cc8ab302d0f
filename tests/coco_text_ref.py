"""Float64 reference, bf16-operand emulation, stand-in faults and comparisons of the COCO caption encoder / decoder on their own
(tests/test_gpu_coco_text_modules.py on the MI355X, tests/test_cpu_coco_text_ref.py without one).  Nothing here needs a GPU.

Reference: oracle.mmvae_ref.coco_text_encoder / coco_text_decoder on float64 copies of formula_params("coco", D), first input
formula_sos(), injected keep masks, random upstream gradients, backward by torch.autograd.

Emulation: the two modules restated in float64.  With ``rounded=False`` the three-exchange decoder and the encoder are the
oracle, operation for operation (equal bit for bit); the composed decoder is the same function written with W_comb (equal to
float64 rounding).  With ``rounded=True`` it rounds to bf16 exactly what the kernels round in the forward pass (the backward
kernels read the same rounded operands: value rounded, gradient passed through), by kernel of csrc/coco_text_bf16.hip:

  coco_dec_fwd_kernel, coco_dec_fwd_cl_kernel<4|8>  (form "three": one workgroup per block, cluster of 4, cluster of 8 with three
      exchanges): the input vector x[t] (xb: '<s>' at t = 0, then the previous output), the copies of h0 and h1 fed to W_hh0 /
      W_hh1 / W_ho (h0b, h1b; the fp32 state h0f / h1f stays unrounded in the gate math), the dropped-out layer-0 output mid
      (midb, rounded after the keep mask and its 1/0.9), and the five packed matrices W_ih0[:, :300], W_hh0, W_ih1, W_hh1,
      W_ho[:, :200].
  coco_dec_fwd_c8_kernel  (form "composed"): h0b, midb, h1b and W_hh0, W_ih1, W_hh1, W_ho[:, :200] as above.  x[t] is never
      formed for t >= 1: layer 0's input projection is W_comb h1b[t-1] + zi0p with W_comb = W_ih0[:, :300] W_ho[:, :200]
      composed in fp32 by coco_comb_kernel and THEN rounded; at t = 0 it is zi0 + sosv with sosv = W_ih0[:, :300] sos in fp32
      (coco_comb_kernel): neither '<s>' nor W_ih0 is rounded anywhere in this form's forward pass.
  fp32 `lin` launches of csrc/coco_text.hip, unrounded in every form: h(init) = z2h(z); zi0 = z W_ih0[:, 300:]^T + b_ih0;
      zo = z W_ho[:, 200:]^T + b_ho; zi0p = z wz^T + bz with wz = W_ih0[:, 300:] + W_ih0[:, :300] W_ho[:, 200:] and
      bz = b_ih0 + W_ih0[:, :300] b_ho (composed form); the encoder's reverse direction (one step from h = 0) and h2p.
  coco_enc_fwd_res_kernel (form "resident", B a multiple of 4): the copy of h fed to W_hh and W_hh; its input projection is one
      bf16 GEMM (launch_gemm_gather on text_tb_kernel's bf16 captions): the caption vectors and W_ih are rounded as well.
  coco_enc_fwd_kernel (form "streamed"): the copy of h fed to W_hh and W_hh; the input projection is an fp32 `lin`: unrounded.
Biases, gate math, state and accumulation stay float64.  The kernels' __expf / __frcp_rn (about 1e-6 relative) are not emulated.

Backward roundings.  The BPTT kernels (coco_dec_bwd_kernel, coco_dec_bwd_cl_kernel, coco_dec_bwd_c8_kernel, coco_enc_bwd_kernel,
coco_enc_bwd_res_kernel) store the gradients of the gate pre-activations as bf16 (dgi0/1, dgh0/1; the encoder's dgi, dgh) and
read them back as the operands of every product behind them (the hidden-state and feedback paths, the batched weight
gradients with the bias gradients in their 1.0 column, time_sum_bf16_kernel for the z-term of layer 0), and the total output
gradient dout as bf16 for dh1 and W_ho's weight gradient (its z-term and b_ho see the fp32 time sum).  The emulation rounds
these too, with a function that is the identity forward and rounds the gradient, placed on the two pre-activations of every
GRU cell and on the product W_ho h1.  They are in from the start, not added after a miss: at T = 1 the streamed encoder's
forward pass rounds nothing at all (h = 0, fp32 input projection), the forward-only emulation IS the oracle there and its gate
would be zero, while the kernel rounds dgi and dgh like at every other T.  Still left to the factor: the bf16 copies of operands
the forward pass did not round but a weight gradient reads rounded (the captions in the streamed encoder's W_ih gradient,
x[t] in the composed decoder's W_ih0 gradient), dw16 / dout_combine_kernel's bf16 dOut of the composed BPTT, and the
three-exchange BPTT behind a composed forward (knob coco_no_comb_bwd), which reads W_ih0^T and bf16(x[t]) where the composed
BPTT reads W_comb^T; its cases are gated with the composed emulation, whose forward pass is theirs.

Gates come from this side alone: GATE_FACTOR = 4 times what the emulation of the case's own form differs from the unrounded
oracle on the same inputs -- 2 for the bf16-stored backward operands the emulation leaves out, 2 the project's margin (the
factor and the reasoning of tests/text_ref.py).  Outputs are compared element-wise (absolute), dz and every parameter gradient
tensor by relative L2; a tensor whose reference gradient is exactly zero (the hidden weights of the encoder's one-step reverse
direction; at T = 1 those of the forward direction too) must be exactly zero.
Floor.  Where bf16 rounds (next to) nothing -- the streamed encoder's output at T = 1 exactly, its first steps nearly -- what is
left is an fp32 computation with __expf / __frcp_rn, and 4 x 0 is no bound for one.  There the gate is what the project already
asks of the fp32 kernels of these same modules (tests/test_gpu_coco.py: outputs 2e-5 absolute, gradient tensors 2e-4 relative
L2): FLOOR_ABS / FLOOR_REL, 50 times below the gates of any case in which bf16 takes part.

``fault`` turns the emulation into a stand-in engine with one defect:
  "last_column"  latent column D-1 is ignored (decoder)
  "row16"        row 16 of every per-row result is answered with row 0's
  "mask3"        the keep mask of step 3 is ignored (decoder)
  "units192"     hidden units 192..199 of the decoder's layer 1 / of the encoder state are not updated from step 1 on: the
                 half-filled thirteenth 16-unit block, which one rank of a cluster owns
  "last_step"    the encoder's forward direction never sees text[:, T-1]

Bit-for-bit helpers (permutation_violations, sub_batch_violations) and the sizes at which they hold:
  Every row of sentence / dz / encoder output is produced by MFMA tiles and fp32 `lin` products whose summation order over k
  does not depend on the row's position, so a row permutation at the SAME batch size must reproduce each row exactly.
  Across batch sizes the summation order can change only where a launcher picks a kernel by the row count:
    * `lin` / `lin_dx` (gemm_f32, csrc/gemm_f32.hip) split k over KS waves by tiles = ceil(M/32) ceil(N/32) and
      per = ceil(K/16): 8 if tiles <= 128 and per >= 16, else 4 if tiles <= 256 and per >= 8, else 2 if tiles <= 512 and
      per >= 4, else 1 (f32_gemm_ks).  Decoder: M = B, N in (600, 300, 200), K = D forward and N = D, K in (200, 600, 300)
      for dz: at B <= 32 every one of them has M/32 = 1, so any two batches up to 32 rows agree (dec_dispatch).
    * the decoder's ranks per block depend on the knob and on ceil(ceil(B/16)/8): equal for all B <= 128.
    * the streamed encoder's input projection is lin with M = T B, N = 600, K = 300 (per = 19): KS = 8 up to T B = 192, 4 up to
      416, 2 up to 832, 1 above.
    * the resident encoder's input projection (launch_gemm_gather, 600 rows, K = 320, N = T B columns; gemm_of never splits K
      at K = 320) goes to gemm_small with 2 k-slices up to T B = 832, with 1 up to 2560, and to the 128-row tile kernel above.
    * the encoder's form itself: resident at B % 4 == 0 unless coco_enc_streamed is set.
  enc_dispatch / dec_dispatch restate these rules; sub-batches are valid where they return equal tuples."""
import torch
import torch.nn.functional as F

from oracle import mmvae_ref as R

H, E = R.COCO_HID, R.COCO_EMB
GATE_FACTOR = 4.0
FLOOR_ABS, FLOOR_REL = 2e-5, 2e-4          # the fp32 bounds of tests/test_gpu_coco.py (module docstring: Floor)
ENC, DEC = "text_encoder.", "text_decoder."
DEC_FORMS = ("three", "composed")
ENC_FORMS = ("resident", "streamed")
DEC_FAULTS = ("last_column", "row16", "mask3", "units192")
ENC_FAULTS = ("row16", "units192", "last_step")


class _RoundBf16(torch.autograd.Function):
    """value rounded to bf16, gradient passed through: the engine's backward GEMMs read the same rounded operand"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundGrad(torch.autograd.Function):
    """identity forward, gradient rounded to bf16: placed where a backward kernel stores a bf16 gradient operand"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def _ident(x):
    return x


def _gates(gi, gh, h):
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return (1 - z) * n + z * h


def _cell(x, h, w_ih, w_hh, b_ih, b_hh, qx, qh, qg=_ident):
    """oracle.mmvae_ref.gru_cell with the input-side operands through qx, the hidden-side operands through qh and the
    gradients of the two pre-activations (dgi, dgh) through qg"""
    return _gates(qg(qx(x) @ qx(w_ih).t() + b_ih), qg(qh(h) @ qh(w_hh).t() + b_hh), h)


def _stale(new, old, t, fault):
    """units192: units 192..199 keep their previous value from step 1 on"""
    if fault == "units192" and t >= 1:
        return torch.cat((new[:, :192], old[:, 192:]), 1)
    return new


def text_encoder(p, text, rounded=False, form="resident", fault=None):
    """coco/model.py:219-245 -> (B, 2D)"""
    assert form in ENC_FORMS
    q = _RoundBf16.apply if rounded else _ident
    qx = q if form == "resident" else _ident
    qg = _RoundGrad.apply if rounded else _ident
    g = ENC + "gru."
    B, T, _ = text.shape
    h = text.new_zeros(B, H)
    for t in range(T):
        if fault == "last_step" and t == T - 1:
            break
        hn = _cell(text[:, t], h, p[g + "weight_ih_l0"], p[g + "weight_hh_l0"], p[g + "bias_ih_l0"], p[g + "bias_hh_l0"], qx, q, qg)
        h = _stale(hn, h, t, fault)
    hb = _cell(text[:, T - 1], text.new_zeros(B, H), p[g + "weight_ih_l0_reverse"], p[g + "weight_hh_l0_reverse"],
               p[g + "bias_ih_l0_reverse"], p[g + "bias_hh_l0_reverse"], _ident, _ident)
    return F.linear(h + hb, p[ENC + "h2p.weight"], p[ENC + "h2p.bias"])


def text_decoder(p, z, sos, steps, keep=None, rounded=False, form="three", fault=None):
    """coco/model.py:256-312 in train mode with the keep masks keep[t] (None: no dropout) -> sentence (B, steps, 300)"""
    assert form in DEC_FORMS
    q = _RoundBf16.apply if rounded else _ident
    qg = _RoundGrad.apply if rounded else _ident
    g = DEC + "gru."
    if fault == "last_column":
        col = torch.ones(z.shape[1], dtype=z.dtype)
        col[-1] = 0
        z = z * col
    B = z.shape[0]
    w_ih0, w_ho, b_ih0, b_ho = p[g + "weight_ih_l0"], p[DEC + "h2o.weight"], p[g + "bias_ih_l0"], p[DEC + "h2o.bias"]
    exact = not rounded and form == "three"            # the oracle's own operations, concatenations included
    w_in = sos.to(z.dtype).reshape(1, E).expand(B, E)
    hinit = F.linear(z, p[DEC + "z2h.weight"], p[DEC + "z2h.bias"])
    h = [hinit, hinit]
    if not exact:
        wx, wo = w_ih0[:, :E], w_ho[:, :H]
        zi0 = z @ w_ih0[:, E:].t() + b_ih0
        zo = z @ w_ho[:, H:].t() + b_ho
        if form == "composed":
            w_comb = wx @ wo
            zi0p = z @ (w_ih0[:, E:] + wx @ w_ho[:, H:]).t() + (b_ih0 + wx @ b_ho)
            sosv = wx @ sos.to(z.dtype).reshape(E)
    out = []
    for t in range(steps):
        if exact:
            gi = torch.cat((w_in, z), dim=1) @ w_ih0.t() + b_ih0
        elif form == "three":
            gi = q(w_in) @ q(wx).t() + zi0
        elif t == 0:
            gi = zi0 + sosv
        else:
            gi = q(h[1]) @ q(w_comb).t() + zi0p
        h[0] = _gates(qg(gi), qg(q(h[0]) @ q(p[g + "weight_hh_l0"]).t() + p[g + "bias_hh_l0"]), h[0])
        mid = h[0]
        if keep is not None and not (fault == "mask3" and t == 3):
            mid = R.dropout(mid, True, keep[t])
        h1 = _cell(mid, h[1], p[g + "weight_ih_l1"], p[g + "weight_hh_l1"], p[g + "bias_ih_l1"], p[g + "bias_hh_l1"], q, q, qg)
        h[1] = _stale(h1, h[1], t, fault)
        if exact:
            w_out = F.linear(torch.cat((h[1], z), dim=1), w_ho, b_ho)
        else:
            w_out = qg(q(h[1]) @ q(wo).t()) + zo            # (dout is stored as bf16; the z-term sees the fp32 time sum)
        out.append(w_out)
        w_in = w_out
    return torch.stack(out, dim=1)


# ------------------------------------------------------------------------------------------------ parameters and inputs
def text_params(D):
    """the text_encoder.* / text_decoder.* tensors of the formula initialisation, float32 (what the engine is loaded with)"""
    P = R.formula_params("coco", D)
    return {k: v.detach().clone() for k, v in P.items() if k.startswith((ENC, DEC))}


def f64(P, requires_grad=False):
    return {k: v.detach().double().clone().requires_grad_(requires_grad) for k, v in P.items()}


def single_column_params(P, D, col):
    """Every path from z into the decoder is cut except latent column `col`, and that one is scaled by 4: a kernel that drops the
    last k-step or the last column of its z operand returns the z-independent answer, O(1) away."""
    Q = {k: v.clone() for k, v in P.items()}
    for name, lo in ((DEC + "z2h.weight", 0), (DEC + "gru.weight_ih_l0", E), (DEC + "h2o.weight", H)):
        w = Q[name]
        kept = w[:, lo + col].clone() * 4
        w[:, lo:] = 0
        w[:, lo + col] = kept
    return Q


def make_inputs(D, B, T, seed=0):
    """float32 / integer inputs of one comparison: z, the captions (GloVe-like scale), keep masks and upstream gradients on the
    sentence and on the encoder output"""
    g = torch.Generator().manual_seed(7000 + 131 * D + 17 * B + 1009 * T + seed)
    return dict(
        z=torch.randn(B, D, generator=g),
        text=0.4 * torch.randn(B, T, E, generator=g),
        keep=(torch.rand(T, B, H, generator=g) >= R.DROP_P).to(torch.uint8),
        gs=torch.randn(B, T, E, generator=g),
        ge=torch.randn(B, 2 * D, generator=g))


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


def _names(P, prefix):
    return [k for k in P if k.startswith(prefix)]


def run_decoder(P32, inp, keep=True, rounded=False, form="three", fault=None, oracle=False):
    """forward and backward of the decoder in float64 -> dict(sentence, dz, grads {name: gradient}); oracle=True runs
    oracle.mmvae_ref.coco_text_decoder itself"""
    P = f64(P32, requires_grad=True)
    z = inp["z"].double().requires_grad_(True)
    T = inp["gs"].shape[1]
    km = [inp["keep"][t].double() for t in range(T)] if keep else None
    sos = R.formula_sos().double()
    if oracle:
        sent = R.coco_text_decoder(P, z, True, sos, T, km, drop_p=R.DROP_P if keep else 0.0)
    else:
        sent = text_decoder(P, z, sos, T, km, rounded, form, fault)
    (sent * inp["gs"].double()).sum().backward()
    return dict(sentence=_row16(sent.detach(), fault), dz=_row16(z.grad, fault), grads={k: P[k].grad for k in _names(P, DEC)})


def run_encoder(P32, inp, rounded=False, form="resident", fault=None, oracle=False):
    """forward and backward of the encoder in float64 -> dict(encout, grads)"""
    P = f64(P32, requires_grad=True)
    text = inp["text"].double()
    out = R.coco_text_encoder(P, text) if oracle else text_encoder(P, text, rounded, form, fault)
    (out * inp["ge"].double()).sum().backward()
    zero = torch.zeros(())
    return dict(encout=_row16(out.detach(), fault),
                grads={k: (P[k].grad if P[k].grad is not None else zero.expand_as(P[k]).double()) for k in _names(P, ENC)})


# ------------------------------------------------------------------------------------------------ comparisons
ABS = ("sentence", "encout")       # element-wise, absolute
REL = ("dz",)                      # relative L2


def rel_l2(a, b):
    """relative L2 distance; against an exactly zero reference: 0 when `a` is exactly zero too, inf otherwise"""
    a, b = a.double(), b.double()
    nb = float(b.norm())
    if nb == 0.0:
        return 0.0 if bool((a == 0).all()) else float("inf")
    return float((a - b).norm()) / nb


def errors(got, ref):
    """what the comparisons measure: sentence / encoder output element-wise (max abs), dz and every parameter gradient by
    relative L2 (`grads`: the worst tensor; `grads_by_name`: each)"""
    by = {k: rel_l2(got["grads"][k].cpu(), ref["grads"][k]) for k in ref["grads"]}
    worst = max(by, key=by.get)
    e = dict(grads=by[worst], grads_worst=worst, grads_by_name=by)
    for k in ABS:
        if k in ref:
            e[k] = float((got[k].double().cpu() - ref[k]).abs().max())
    for k in REL:
        if k in ref:
            e[k] = rel_l2(got[k].cpu(), ref[k])
    return e


def quantities(ref):
    return [k for k in ABS + REL if k in ref] + ["grads"]


def gates(emu, ref):
    """GATE_FACTOR times the emulation's own distance from the unrounded oracle on the same inputs -> (gates, yardsticks)"""
    e = errors(emu, ref)
    return {k: max(GATE_FACTOR * e[k], FLOOR_ABS if k in ABS else FLOOR_REL) for k in quantities(ref)}, e


def violations(got, ref, gate, what=""):
    """list of the comparisons `got` misses (empty: it passes), and the measured errors"""
    e = errors(got, ref)
    bad = ["%s %s: %.3e > gate %.3e" % (what, k, e[k], gate[k]) for k in quantities(ref) if k != "grads" and not e[k] <= gate[k]]
    for n, v in e["grads_by_name"].items():
        if float(ref["grads"][n].double().norm()) == 0.0:
            if v != 0.0:
                bad.append("%s grad %s: not exactly zero where the reference is" % (what, n))
        elif not v <= gate["grads"]:
            bad.append("%s grad %s: %.3e > gate %.3e" % (what, n, v, gate["grads"]))
    for k in quantities(ref):
        if k != "grads" and not bool(torch.isfinite(got[k].double()).all()):
            bad.append("%s %s: not finite" % (what, k))
    return bad, e


def worst_ratio(e, gate, ref):
    """error / gate per quantity (gradient tensors with an exactly zero reference left out)"""
    out = {k: e[k] / gate[k] for k in quantities(ref) if k != "grads"}
    live = [v for n, v in e["grads_by_name"].items() if float(ref["grads"][n].double().norm()) != 0.0]
    out["grads"] = max(live) / gate["grads"]
    return out


def _row_diffs(part, full, rows, name, keys):
    bad = []
    idx = torch.as_tensor(rows)
    for k in keys:
        a, b = part[k].cpu(), full[k].cpu()[idx]
        if not torch.equal(a, b):
            diff = (a != b).reshape(len(rows), -1).any(1)
            bad.append("%s: %s differs in rows %s of the part" % (name, k, torch.nonzero(diff).reshape(-1).tolist()[:8]))
    return bad


def permutation_violations(run, inp, keys, full=None):
    """run(inputs) -> dict of per-row results.  Reversed rows and rows rotated by 7, at the same batch size: the dispatch and
    every summation order are the same, so each row's result must be identical."""
    n = inp["z"].shape[0]
    full = run(inp) if full is None else full
    bad = []
    if n < 2:
        return bad
    rot = [(i + 7) % n for i in range(n)]
    for name, rows in (("reversed rows", list(range(n - 1, -1, -1))), ("rows rotated by 7", rot)):
        bad += _row_diffs(run(take_rows(inp, rows)), full, rows, name, keys)
    return bad


def sub_batch_violations(run, inp, row_sets, keys, full=None):
    """each row set alone (moved to the front) against the same rows of the full batch.  Only for row sets at which the
    dispatch (enc_dispatch / dec_dispatch) is the full batch's: the caller asserts that."""
    full = run(inp) if full is None else full
    bad = []
    for rows in row_sets:
        bad += _row_diffs(run(take_rows(inp, rows)), full, rows, "rows %d..%d alone" % (rows[0], rows[-1]), keys)
    return bad


def single_column_violations(run, P32, D, col, inp, keep, form, cache=None):
    """run(P, inputs) -> the decoder's result on the parameters of single_column_params: `sentence` and dz[:, col] inside the
    gate of these parameters and inputs, every other column of dz exactly 0.  cache: a dict that keeps the reference and the
    emulation of (these formula parameters and inputs, col, form) for the next caller"""
    Q = single_column_params(P32, D, col)
    cache = {} if cache is None else cache
    key = (D, col, tuple(inp["gs"].shape), keep)
    if key not in cache:
        cache[key] = run_decoder(Q, inp, keep)
    if key + (form,) not in cache:
        cache[key + (form,)] = run_decoder(Q, inp, keep, rounded=True, form=form)
    ref, emu = cache[key], cache[key + (form,)]
    g_s = max(GATE_FACTOR * float((emu["sentence"] - ref["sentence"]).abs().max()), FLOOR_ABS)
    g_dz = max(GATE_FACTOR * rel_l2(emu["dz"][:, col], ref["dz"][:, col]), FLOOR_REL)
    got = run(Q, inp)
    dz = got["dz"].double().cpu()
    e_s = float((got["sentence"].double().cpu() - ref["sentence"]).abs().max())
    e_dz = rel_l2(dz[:, col], ref["dz"][:, col])
    bad = []
    if not e_s <= g_s:
        bad.append("column %d kept: sentence %.3e > gate %.3e" % (col, e_s, g_s))
    if not e_dz <= g_dz:
        bad.append("column %d kept: dz[:, %d] %.3e > gate %.3e" % (col, col, e_dz, g_dz))
    others = torch.cat((dz[:, :col], dz[:, col + 1:]), 1)
    if others.numel() and not bool((others == 0).all()):
        bad.append("column %d kept: dz is nonzero in %d elements of the cut columns" % (col, int((others != 0).sum())))
    return bad, dict(sentence=e_s, dz=e_dz, gate_sentence=g_s, gate_dz=g_dz)


# ------------------------------------------------------------------------------------------------ the cases of the GPU table
# decoder form -> (knobs away from their defaults, emulation form at H + D <= 320, emulation form above)
DEC_FORM_KNOBS = {
    "wg1": (dict(coco_cluster=0), "three", "three"),              # one workgroup per 16-row block
    "cl4": (dict(coco_cluster=4), "three", "three"),              # cluster of 4
    "cl8x3": (dict(coco_no_comb=1), "three", "three"),            # cluster of 8, three exchanges
    "comb_fwd": (dict(coco_no_comb_bwd=1), "composed", "three"),  # composed forward, three-exchange BPTT
    "comb": (dict(), "composed", "three"),                        # the default: composed both ways (D <= 120)
}


def dec_emulation_form(form, D):
    return DEC_FORM_KNOBS[form][1 if H + D <= 320 else 2]


def _dec_cases():
    c = []
    for f in DEC_FORM_KNOBS:                                      # one full row block and a ragged one of 7
        c += [(f, 100, 23, 7, True), (f, 100, 23, 102, False), (f, 100, 23, 1, True), (f, 100, 23, 2, True)]
    c += [("comb", 100, b, 3, True) for b in (1, 16, 17)]
    c += [(f, 100, 133, 3, True) for f in ("wg1", "cl4", "comb")]  # nine row blocks: a second octet with idle padding workgroups
    c += [("comb", d, 23, 7, True) for d in (4, 20, 120, 124)]     # 120: the last composed size; 124: three exchanges
    return c


DEC_CASES = _dec_cases()                                          # (form, D, B, T, keep masks)
# (D, B, T, coco_enc_streamed): resident at B = 4, 20, 36; streamed at B = 1, 23 and at B = 20 with the knob
ENC_CASES = [(d, b, t, k) for d in (4, 100) for t in (1, 2, 7, 102) for b, k in ((4, 0), (20, 0), (36, 0), (1, 0), (23, 0), (20, 1))]


def dec_id(c):
    return "%s-D%d-B%d-T%d-%s" % (c[0], c[1], c[2], c[3], "keep" if c[4] else "nokeep")


def enc_id(c):
    return "D%d-B%d-T%d-%s" % (c[0], c[1], c[2], enc_form(c[1], c[3]))


def enc_form(B, streamed_knob):
    return "resident" if B % 4 == 0 and not streamed_knob else "streamed"


def dec_fault_applies(fault, D, B, T, keep):
    """is the fault a defect at this case at all?"""
    return {"last_column": True, "row16": B > 16, "mask3": keep and T > 3, "units192": T > 1}[fault]


def enc_fault_applies(fault, B, T):
    return {"row16": B > 16, "units192": T > 1, "last_step": True}[fault]


# ------------------------------------------------------------------------------------------------ the launchers' choices, restated
def _cdiv(a, b):
    return (a + b - 1) // b


def f32_gemm_ks(M, N, K):
    """waves a workgroup of gemm_f32 splits k over (csrc/gemm_f32.hip gemm_f32, no grid-level split)"""
    tiles, per = _cdiv(M, 32) * _cdiv(N, 32), _cdiv(K, 16)
    if tiles <= 128 and per >= 16:
        return 8
    if tiles <= 256 and per >= 8:
        return 4
    if tiles <= 512 and per >= 4:
        return 2
    return 1


def dec_dispatch(B, D, cluster=8):
    """everything in the decoder's launches that depends on the row count and can change a row's summation order"""
    fwd = tuple(f32_gemm_ks(B, n, D) for n in (600, 300, 200))
    bwd = tuple(f32_gemm_ks(B, D, k) for k in (200, 600, 300))
    nblk_pad = _cdiv(_cdiv(B, 16), 8) * 8
    ranks = cluster
    while ranks > 1 and nblk_pad * ranks > 256 * 7 // 8:         # (coco_dec_cluster on the MI355X's 256 compute units)
        ranks //= 2
    return fwd + bwd + (ranks if ranks in (4, 8) else 0,)


def enc_dispatch(B, T, D, streamed_knob=False):
    """(form, what the input projection's launcher picks at T*B, KS of the B-row lin launches: reverse direction and h2p)"""
    n = T * B
    small = (f32_gemm_ks(B, 600, 300), f32_gemm_ks(B, 600, 200), f32_gemm_ks(B, 2 * D, 200))
    if B % 4 == 0 and not streamed_knob:
        return ("resident", "small2" if n <= 832 else "small1" if n <= 2560 else "tile128") + small
    return ("streamed", f32_gemm_ks(n, 600, 300)) + small
