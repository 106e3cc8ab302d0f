"""Records tests/golden/mnist_vae_keys.json from the reference's own ``VAE`` (``mnist/model.py:188-232``)::

    python tools/record_mnist_vae_keys.py /path/to/reference/checkout

Stored: the names and shapes of ``VAE(20).state_dict()`` in its order, and the defaults of the argument parser of
``mnist/imageonly/train_imageonly.py:76-89`` as that file states them.  Data only; run once by hand, no test runs it.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(checkout):
    sys.path.insert(0, os.path.join(checkout, "mnist"))
    from model import VAE                             # the reference's
    sd = VAE(n_latents=20).state_dict()
    record = {
        "n_latents": 20,
        "state_dict": [[k, list(v.shape)] for k, v in sd.items()],
        # mnist/imageonly/train_imageonly.py:77-88
        "train_defaults": {"n_latents": 20, "batch_size": 128, "epochs": 20, "lr": 1e-3, "log_interval": 10, "cuda": False},
    }
    out = os.path.join(ROOT, "tests", "golden", "mnist_vae_keys.json")
    with open(out, "w") as fp:
        json.dump(record, fp, indent=1)
    print(out, len(record["state_dict"]), "entries")


if __name__ == "__main__":
    main(sys.argv[1])
