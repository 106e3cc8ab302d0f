"""Index arithmetic of the weight pack (multimodal-vae_amd/csrc/pack_geo.h: plain C++17, called by pack_block in elementwise.hip)
checked on the host: tests/host/pack_geo_check.cpp walks every block, wave and lane of a hand-written list of descriptors with the
real layers' sizes (Conv2d forward form, the stride-parity classes of a data gradient, ConvTranspose2d 64->32 k5, conv1 with one
channel, a Linear with a folded bias column and Kpad > K, transposed Linears with Npad > N, fragment-major destinations, an fp32
vector) and asserts that every destination vector has exactly one writer, holds the element the original formula names or a zero
pad, that every read stays inside the descriptor's parameter tensor, and that every load instruction of a wave reads runs of at
least 64 bytes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pack_geometry_owners_sources_and_run_lengths(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "pack_geo_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "multimodal-vae_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "pack_geo_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:]
    assert "descriptors 17" in r.stdout
    for kind in ("conv2d 32->64 k4 forward", "dgrad class 3", "convT 64->32 k5", "conv1 1->32", "bias column", "Npad > N",
                 "fragment-major", "fp32 vector"):
        assert kind in r.stdout, kind
