"""Host side of the COCO evaluation: the loglik_coco command line, its host-side refusals, the declarations of the scoring call and
its two test hooks in the public header, the family record of the evaluation and the constant of the Gaussian caption likelihood."""
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_loglik_coco_parser():
    from multimodal_vae_amd.evaluate import _parser
    a = _parser().parse_args(["loglik_coco", "model.pth.tar"])
    assert a.cmd == "loglik_coco" and a.model_path == "model.pth.tar"
    assert (a.image_only, a.text_only, a.all, a.n_samples, a.batch_size) == (False, False, False, 100, 64)
    assert (a.sos, a.words, a.data, a.synthetic, a.seed, a.json, a.text_sigma) == (None, None, None, 0, 0, None, 1.0)
    a = _parser().parse_args(["loglik_coco", "m", "--all", "--synthetic", "8", "--n_samples", "4", "--json", "o", "--seed", "3",
                              "--batch_size", "16", "--text_sigma", "0.5", "--sos", "s.pt"])
    assert (a.all, a.synthetic, a.n_samples, a.json, a.seed, a.batch_size, a.text_sigma, a.sos) == (True, 8, 4, "o", 3, 16, 0.5, "s.pt")
    assert _parser().parse_args(["loglik_coco", "m", "--text_only", "--words", "t.pt"]).words == "t.pt"
    assert _parser().parse_args(["loglik_coco", "m", "--image_only", "--data", "d"]).data == "d"
    for bad in (["--image_only", "--text_only"], ["--all", "--image_only"], ["--all", "--text_only"], ["--data", "d", "--synthetic", "3"],
                ["--sos", "s.pt", "--words", "t.pt"], ["--attrs_only"], ["--dataset", "coco"], ["--text_sigma", "x"]):
        with pytest.raises(SystemExit):
            _parser().parse_args(["loglik_coco", "m"] + bad)
    with pytest.raises(SystemExit):
        _parser().parse_args(["loglik_coco"])


def test_loglik_still_rejects_coco():
    from multimodal_vae_amd.evaluate import _parser
    with pytest.raises(SystemExit):
        _parser().parse_args(["loglik", "m", "--dataset", "coco"])
    with pytest.raises(SystemExit):
        _parser().parse_args(["loglik", "m", "--text_sigma", "1.0"])
    with pytest.raises(SystemExit):
        _parser().parse_args(["loglik_celeba", "m", "--text_sigma", "1.0"])


def test_mis_shaped_files_and_sigma_are_refused_on_the_host(tmp_path):
    from multimodal_vae_amd.evaluate import _loglik_coco_main, _parser, check_coco_eval_data
    from multimodal_vae_amd.train_coco import synthetic_coco
    x, t, sos = synthetic_coco(3, seed=1)
    x2, t2 = check_coco_eval_data(x, t.double(), 0.5)
    assert torch.equal(x2, x) and t2.dtype == torch.float32 and torch.equal(t2, t)
    for bad_x in (x.float(), x[:, :, :31], x[:, :1], x.view(3, -1), x[:0]):
        with pytest.raises(ValueError):
            check_coco_eval_data(bad_x, t[:bad_x.shape[0]])
    for bad_t in (t[:, :101], t[:, :, :299], t[:2], t.long(), t.view(3, -1)):
        with pytest.raises(ValueError):
            check_coco_eval_data(x, bad_t)
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            check_coco_eval_data(x, t, sigma)
    # the command refuses before the checkpoint is opened (the path does not exist) and without a GPU
    for name, xs, ts in (("img", x[:, :, :16], t), ("cap", x, t[:, :50])):
        d = tmp_path / name
        d.mkdir()
        torch.save(xs, str(d / "images_u8.pt")); torch.save(ts, str(d / "captions.pt")); torch.save(sos, str(d / "sos.pt"))
        with pytest.raises(ValueError):
            _loglik_coco_main(_parser().parse_args(["loglik_coco", str(tmp_path / "none.pth.tar"), "--data", str(d)]))
    with pytest.raises(ValueError):
        _loglik_coco_main(_parser().parse_args(["loglik_coco", str(tmp_path / "none.pth.tar"), "--synthetic", "2", "--text_sigma", "0"]))
    with pytest.raises(SystemExit):
        _loglik_coco_main(_parser().parse_args(["loglik_coco", str(tmp_path / "none.pth.tar")]))


def _declared_args(text, name, ret="int"):
    m = re.search(r"%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), text)
    assert m, "%s is not declared in include/mmvae_hip.h" % name
    return [a.strip() for a in re.sub(r"/\*.*?\*/", " ", m.group(1).replace("\n", " ")).split(",")]


def test_header_declares_the_coco_scorer_and_its_hooks():
    from multimodal_vae_amd._lib import SIGNATURES
    text = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    score = _declared_args(text, "mmvae_coco_iw_score")
    assert len(score) == 12 and score[0].startswith("mmvae_coco_t*") and score[-1].startswith("void*")
    assert "text" in score[5] and "sos" in score[6] and "sse_y" in score[10]
    assert len(SIGNATURES["mmvae_coco_iw_score"][1]) == 12
    tail = _declared_args(text, "mmvae_coco_iw_tail")
    assert len(tail) == 10 and tail[0].startswith("const void*") and tail[-1].startswith("void*")
    assert len(SIGNATURES["mmvae_coco_iw_tail"][1]) == 10
    sse = _declared_args(text, "mmvae_coco_iw_text_sse")
    assert len(sse) == 7 and sse[0].startswith("const float*") and "steps" in sse[4] and sse[-1].startswith("void*")
    assert len(SIGNATURES["mmvae_coco_iw_text_sse"][1]) == 7
    ws = _declared_args(text, "mmvae_coco_iw_workspace_bytes", ret="size_t")
    assert len(ws) == 1 and len(SIGNATURES["mmvae_coco_iw_workspace_bytes"][1]) == 1
    inner = open(os.path.join(ROOT, "multimodal-vae_amd", "csrc", "coco.h")).read()
    for name in ("coco_iw_score", "coco_iw_workspace_bytes", "launch_coco_iw_tail", "launch_coco_iw_text_sse"):
        assert re.search(r"\b%s\s*\(" % name, inner), name


def test_coco_is_a_family_of_the_evaluation():
    from multimodal_vae_amd import evaluate as E
    from multimodal_vae_amd.coco import MultimodalVAE
    fam = E._FAMILIES["coco"]
    assert (fam.name, fam.T, fam.V, fam.image_shape, fam.rows, fam.float_text) == ("coco", 1, 1, (3, 32, 32), E.IW_ROWS_COCO, True)
    assert E.IW_ROWS_COCO % 4 == 0 and 4 <= E.IW_ROWS_COCO <= 512
    assert E._family(MultimodalVAE(8, sos=torch.zeros(300))) is fam
    assert E._family(MultimodalVAE(8, sos=torch.zeros(300), steps=3)) is fam
    # the other records are what they were
    assert [(f.name, f.T, f.V, f.float_text) for f in (E._FAMILIES[k] for k in ("multimnist", "mnist", "celeba"))] == \
        [("multimnist", 4, 12, False), ("mnist", 1, 10, False), ("celeba", 18, 2, False)]
    chunks = E.iw_chunks(64, 1000, fam.rows)
    assert sum(nr * nk for _, nr, _, nk in chunks) == 64000 and max(nr * nk for _, nr, _, nk in chunks) <= fam.rows
    assert all((nr * nk) % 4 == 0 for _, nr, _, nk in chunks)          # a 64-example batch stays on the 4-row caption form


def test_workspace_of_an_iw_rows_plan_stays_below_one_gib():
    """The plan is sized on the host; the figure next to IW_ROWS_COCO is this one."""
    from multimodal_vae_amd import evaluate as E
    from multimodal_vae_amd._lib import call
    h = call("mmvae_coco_create_t", 100, E.IW_ROWS_COCO, 102)
    assert h
    try:
        wsb = call("mmvae_coco_iw_workspace_bytes", h)
    finally:
        call("mmvae_coco_destroy", h)
    print("mmvae_coco_iw_workspace_bytes(%d rows, 102 steps) = %d" % (E.IW_ROWS_COCO, wsb))
    assert 0 < wsb < 1 << 30
    src = open(os.path.join(ROOT, "multimodal-vae_amd", "evaluate.py")).read()
    line = [l for l in src.splitlines() if l.startswith("IW_ROWS_COCO")][0]
    assert str(wsb) in line.replace(",", ""), line


@pytest.mark.parametrize("steps,sigma", [(102, 1.0), (3, 0.5), (5, 2.0)])
def test_gaussian_constant_and_the_post_finalize_shift(steps, sigma):
    from multimodal_vae_amd.evaluate import _shift_text_terms, coco_text_constant
    c = coco_text_constant(steps, sigma)
    want = -0.5 * steps * 300 * (math.log(2 * math.pi) + 2 * math.log(sigma))
    assert abs(c - want) <= 1e-12 * abs(want)
    if steps == 102 and sigma == 1.0:
        assert abs(c + 28119.0) < 1.0                                 # "about -28,119"
    g = torch.Generator().manual_seed(steps)
    out = torch.randn(4, 8, generator=g) * 10
    lw = torch.randn(4, 6, 3, generator=g) * 10
    out0, lw0 = out.clone(), lw.clone()
    _shift_text_terms(out, lw, c)
    ulp = 2.0 ** -23 * (abs(c) + 100.0)                              # one fp32 rounding of a sum of this size
    # log p^(x), the ESS columns and the image NLL are untouched; log p^(y), log p^(x,y) move by c, the caption NLL by -c
    assert torch.equal(out[:, 0], out0[:, 0]) and torch.equal(out[:, 3:7], out0[:, 3:7])
    assert float((out[:, 1:3].double() - (out0[:, 1:3].double() + c)).abs().max()) <= ulp
    assert float((out[:, 7].double() - (out0[:, 7].double() - c)).abs().max()) <= ulp
    assert torch.equal(lw[..., 0], lw0[..., 0])
    assert float((lw[..., 1:].double() - (lw0[..., 1:].double() + c)).abs().max()) <= ulp
    out1 = out0.clone()
    _shift_text_terms(out1, None, c)
    assert torch.equal(out1, out)
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError):
            coco_text_constant(steps, bad)
