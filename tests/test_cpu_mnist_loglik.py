"""Host side of the MNIST evaluation: the loglik command line's --dataset switch, the synthetic MNIST stand-in, the checkpoint
loader and the declaration of the fused scorer in the public header."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_loglik_parser_has_the_dataset_switch():
    from multimodal_vae_amd.evaluate import _parser
    a = _parser().parse_args(["loglik", "model.pth.tar"])
    assert a.dataset == "multimnist"
    # every flag the command line had keeps its default
    assert (a.image_only, a.text_only, a.all, a.n_samples, a.cuda) == (False, False, False, 100, False)
    assert (a.batch_size, a.data, a.synthetic, a.seed, a.json) == (64, "./data", 0, 0, None)
    a = _parser().parse_args(["loglik", "m", "--dataset", "mnist", "--all", "--synthetic", "64", "--n_samples", "8", "--json", "o"])
    assert (a.dataset, a.all, a.synthetic, a.n_samples, a.json) == ("mnist", True, 64, 8, "o")
    assert _parser().parse_args(["loglik", "m", "--dataset", "multimnist"]).dataset == "multimnist"
    assert _parser().parse_args(["loglik", "m", "--dataset", "mnist", "--data", "test.pt"]).data == "test.pt"
    for bad in (["--dataset", "celeba"], ["--dataset"], ["--dataset", "mnist", "--data", "d", "--synthetic", "3"]):
        with pytest.raises(SystemExit):
            _parser().parse_args(["loglik", "m"] + bad)


def test_synthetic_mnist():
    from multimodal_vae_amd.data import synthetic_mnist
    x, y = synthetic_mnist(37, seed=2)
    assert x.shape == (37, 28, 28) and x.dtype == torch.uint8
    assert y.shape == (37,) and y.dtype == torch.int64 and int(y.min()) >= 0 and int(y.max()) <= 9
    assert len(set(y.tolist())) > 1 and int(x.max()) > 0
    assert all(int(x[i].max()) > 0 for i in range(37))               # no empty canvas
    x2, y2 = synthetic_mnist(37, seed=2)
    assert torch.equal(x, x2) and torch.equal(y, y2)
    x3, y3 = synthetic_mnist(37, seed=3)
    assert not torch.equal(x, x3)


def test_mnist_load_checkpoint_round_trip(tmp_path):
    from multimodal_vae_amd import mnist as M
    from multimodal_vae_amd.train import save_checkpoint
    from oracle import mmvae_ref as R
    D = 12
    P = R.formula_params("mnist", D)
    P["image_decoder.net.1.running_mean"] = torch.linspace(-1, 1, 200)
    P["text_decoder.net.1.num_batches_tracked"] = torch.tensor(7)
    save_checkpoint({"state_dict": {k: v.clone() for k, v in P.items()}, "n_latents": D}, False, folder=str(tmp_path))
    vae = M.load_checkpoint(str(tmp_path / "checkpoint.pth.tar"), use_cuda=False)
    assert isinstance(vae, M.MultimodalVAE) and vae.n_latents == D
    sd = vae.state_dict()
    assert set(sd) == set(P)
    for k, v in P.items():
        assert torch.equal(sd[k], v), k
    # the reference's default when the dict has no n_latents (mnist/train.py load_checkpoint)
    P20 = R.formula_params("mnist", 20)
    save_checkpoint({"state_dict": P20}, False, folder=str(tmp_path), filename="old.pth.tar")
    assert M.load_checkpoint(str(tmp_path / "old.pth.tar")).n_latents == 20


def test_header_declares_the_mnist_scorer():
    text = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    m = re.search(r"int\s+mmvae_mnist_iw_score\s*\(([^;]*)\)\s*;", text)
    assert m, "mmvae_mnist_iw_score is not declared in include/mmvae_hip.h"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 8 and args[0].startswith("mmvae_mnist_t*") and args[-1].startswith("void*")
    from multimodal_vae_amd._lib import SIGNATURES
    assert len(SIGNATURES["mmvae_mnist_iw_score"][1]) == 8
