"""Host side of the CelebA evaluation: the loglik_celeba command line, the synthetic CelebA stand-in, the checkpoint loader, the
host-side check of the evaluation file and the declarations of the scoring call and its two test hooks in the public header."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_loglik_celeba_parser():
    from multimodal_vae_amd.evaluate import _parser
    a = _parser().parse_args(["loglik_celeba", "model.pth.tar"])
    assert a.cmd == "loglik_celeba" and a.model_path == "model.pth.tar"
    assert (a.image_only, a.attrs_only, a.all, a.n_samples, a.cuda) == (False, False, False, 100, False)
    assert (a.batch_size, a.data, a.synthetic, a.seed, a.json) == (64, None, 0, 0, None)
    a = _parser().parse_args(["loglik_celeba", "m", "--all", "--synthetic", "32", "--n_samples", "4", "--json", "o", "--seed", "3",
                              "--batch_size", "16", "--cuda"])
    assert (a.all, a.synthetic, a.n_samples, a.json, a.seed, a.batch_size, a.cuda) == (True, 32, 4, "o", 3, 16, True)
    assert _parser().parse_args(["loglik_celeba", "m", "--attrs_only"]).attrs_only
    assert _parser().parse_args(["loglik_celeba", "m", "--image_only", "--data", "f.pt"]).data == "f.pt"
    for bad in (["--image_only", "--attrs_only"], ["--all", "--image_only"], ["--all", "--attrs_only"],
                ["--data", "f.pt", "--synthetic", "3"], ["--text_only"], ["--dataset", "celeba"]):
        with pytest.raises(SystemExit):
            _parser().parse_args(["loglik_celeba", "m"] + bad)
    with pytest.raises(SystemExit):
        _parser().parse_args(["loglik_celeba"])


def test_loglik_still_rejects_celeba_and_keeps_its_flags():
    from multimodal_vae_amd.evaluate import _parser
    with pytest.raises(SystemExit):
        _parser().parse_args(["loglik", "m", "--dataset", "celeba"])
    with pytest.raises(SystemExit):
        _parser().parse_args(["loglik", "m", "--attrs_only"])
    a = _parser().parse_args(["loglik", "m"])
    assert (a.dataset, a.data, a.text_only) == ("multimnist", "./data", False)
    assert _parser().parse_args(["sample", "m"]).n_samples == 64


def test_synthetic_celeba():
    from multimodal_vae_amd.data import synthetic_celeba
    x, a = synthetic_celeba(37, seed=2)
    assert x.shape == (37, 3, 64, 64) and x.dtype == torch.uint8
    assert a.shape == (37, 18) and a.dtype == torch.float32
    assert bool(((a == 0) | (a == 1)).all()) and 0 < float(a.mean()) < 1
    assert all(int(x[i].max()) > 0 for i in range(37))               # no empty image
    x2, a2 = synthetic_celeba(37, seed=2)
    assert torch.equal(x, x2) and torch.equal(a, a2)
    x3, a3 = synthetic_celeba(37, seed=3)
    assert not torch.equal(x, x3) and not torch.equal(a, a3)


def test_celeba_load_checkpoint_round_trip(tmp_path):
    from multimodal_vae_amd import celeba as M
    from multimodal_vae_amd.train import save_checkpoint
    from oracle import mmvae_ref as R
    D = 12
    P = R.formula_params("celeba", D)
    P["image_decoder.hallucinate.7.running_mean"] = torch.linspace(-1, 1, 32)
    P["image_decoder.hallucinate.7.running_var"] = torch.linspace(0.5, 2, 32)
    P["attrs_decoder.net.1.running_var"] = torch.linspace(0.25, 3, 64)
    P["attrs_decoder.net.1.num_batches_tracked"] = torch.tensor(7)
    save_checkpoint({"state_dict": {k: v.clone() for k, v in P.items()}, "n_latents": D}, False, folder=str(tmp_path))
    vae = M.load_checkpoint(str(tmp_path / "checkpoint.pth.tar"), use_cuda=False)
    assert isinstance(vae, M.MultimodalVAE) and vae.n_latents == D
    sd = vae.state_dict()
    assert set(sd) == set(P)
    for k, v in P.items():
        assert torch.equal(sd[k], v), k
    # the reference's default when the dict has no n_latents (celeba/train.py: --n_latents 100)
    P100 = R.formula_params("celeba", 100)
    save_checkpoint({"state_dict": P100}, False, folder=str(tmp_path), filename="old.pth.tar")
    assert M.load_checkpoint(str(tmp_path / "old.pth.tar")).n_latents == 100


def test_evaluation_file_is_checked_on_the_host(tmp_path):
    from multimodal_vae_amd.data import synthetic_celeba
    from multimodal_vae_amd.evaluate import load_celeba_eval_file
    x, a = synthetic_celeba(5, seed=1)
    torch.save((x, a.to(torch.int64)), str(tmp_path / "ok.pt"))       # 0 / 1 of any dtype
    x2, a2 = load_celeba_eval_file(str(tmp_path / "ok.pt"))
    assert torch.equal(x2, x) and a2.dtype == torch.float32 and torch.equal(a2, a)
    for name, bad in (("half", a * 0.5 + 0.25), ("minus", a * 2 - 1), ("nan", torch.full_like(a, float("nan")))):
        torch.save((x, bad), str(tmp_path / (name + ".pt")))
        with pytest.raises(ValueError):
            load_celeba_eval_file(str(tmp_path / (name + ".pt")))
    torch.save((x, a[:, :17]), str(tmp_path / "short.pt"))
    with pytest.raises(ValueError):
        load_celeba_eval_file(str(tmp_path / "short.pt"))
    torch.save((x.float(), a), str(tmp_path / "float.pt"))
    with pytest.raises(ValueError):
        load_celeba_eval_file(str(tmp_path / "float.pt"))


def _declared_args(text, name, ret="int"):
    m = re.search(r"%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), text)
    assert m, "%s is not declared in include/mmvae_hip.h" % name
    return [a.strip() for a in re.sub(r"/\*.*?\*/", " ", m.group(1).replace("\n", " ")).split(",")]


def test_header_declares_the_celeba_scorer_and_its_hooks():
    from multimodal_vae_amd._lib import SIGNATURES
    text = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    score = _declared_args(text, "mmvae_celeba_iw_score")
    assert len(score) == 10 and score[0].startswith("mmvae_celeba_t*") and score[-1].startswith("void*")
    assert len(SIGNATURES["mmvae_celeba_iw_score"][1]) == 10
    tail = _declared_args(text, "mmvae_celeba_iw_tail")
    assert len(tail) == 10 and tail[0].startswith("const void*") and tail[-1].startswith("void*")
    assert len(SIGNATURES["mmvae_celeba_iw_tail"][1]) == 10
    attrs = _declared_args(text, "mmvae_celeba_iw_attrs")
    assert len(attrs) == 5 and attrs[0].startswith("mmvae_celeba_t*") and "long long" in attrs[2]
    assert len(SIGNATURES["mmvae_celeba_iw_attrs"][1]) == 5
    ws = _declared_args(text, "mmvae_celeba_iw_workspace_bytes", ret="size_t")
    assert len(ws) == 1 and len(SIGNATURES["mmvae_celeba_iw_workspace_bytes"][1]) == 1


def test_celeba_is_a_family_of_the_evaluation():
    from multimodal_vae_amd import evaluate as E
    from multimodal_vae_amd.celeba import MultimodalVAE
    fam = E._FAMILIES["celeba"]
    assert (fam.name, fam.T, fam.V, fam.image_shape, fam.rows) == ("celeba", 18, 2, (3, 64, 64), E.IW_ROWS_CELEBA)
    assert E._family(MultimodalVAE(8)) is fam
    assert E._posterior("attrs") == "text" and E._posterior("joint") == "joint"
    # the row count of one scoring call splits a batch x particles grid like the other families'
    chunks = E.iw_chunks(64, 100, fam.rows)
    assert sum(nr * nk for _, nr, _, nk in chunks) == 6400 and max(nr * nk for _, nr, _, nk in chunks) <= fam.rows
