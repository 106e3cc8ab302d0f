"""Records tests/golden/mnist_infovae_reference.npz from the reference's own ``InfoVAE`` (``mnist/model.py``), executed as it stands
in float64::

    python tools/record_infovae_mnist_reference.py /path/to/reference/checkout

The weights (51 MB) do not fit a fixture, so they and the inputs come from the formulas of tests/conv4s2_ref.py (``formula_state_dict``,
``formula_input``, ``formula_latent_grid``) that the tests rebuild.  Stored: the ``state_dict`` key names and shapes, recon (4,1,28,28)
and z (4,20) of the whole model in ``eval()``, the output of ``encoder_conv`` alone on the first two inputs and the output of
``decoder_conv`` on the formula input (4,128,7,7).  Run once by hand; no test runs it.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conv4s2_ref as C  # noqa: E402


def main(checkout):
    sys.path.insert(0, os.path.join(checkout, "mnist"))
    from model import InfoVAE                         # the reference's
    vae = InfoVAE(n_latents=20).double().eval()
    names = list(vae.state_dict())
    shapes = [tuple(v.shape) for v in vae.state_dict().values()]
    vae.load_state_dict(C.formula_state_dict(names, shapes))
    x, grid = C.formula_input(4), C.formula_latent_grid(4)
    with torch.no_grad():
        recon, z = vae(x)
        enc = vae.encoder_conv(x[:2].clone())
        dec = vae.decoder_conv(grid.clone())
    out = os.path.join(ROOT, "tests", "golden", "mnist_infovae_reference.npz")
    np.savez(out, names=np.array(names), shapes=np.array([list(s) + [0] * (4 - len(s)) for s in shapes], dtype=np.int64),
             recon=recon.numpy(), z=z.numpy(), encoder_conv=enc.numpy(), decoder_conv=dec.numpy())
    print(out, os.path.getsize(out), "bytes; recon %.3f..%.3f, z std %.3f" % (float(recon.min()), float(recon.max()), float(z.std())))


if __name__ == "__main__":
    main(sys.argv[1])
