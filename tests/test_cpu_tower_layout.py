"""CPU-only: the CelebA and COCO plans keep the sizes and the workspace layout recorded in tests/golden/tower_layout.json
(tools/record_tower_layout.py).  Both families build their image half from csrc/img_tower.h and carve their workspace in an order
of their own; a restructuring of either must leave every byte offset where it was."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "tower_layout.json")) as _f:
    GOLDEN = json.load(_f)


def _recorder():
    spec = importlib.util.spec_from_file_location("record_tower_layout", os.path.join(ROOT, "tools", "record_tower_layout.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_golden_covers_both_families_and_every_name():
    rec = _recorder()
    assert sorted(GOLDEN) == sorted("%s_D%d_B%d" % (fam, D, B) for fam in rec.NAMES for D, B in rec.CASES)
    for fam, names in rec.NAMES.items():
        assert len(names) == len(set(names)) == {"celeba": 64, "coco": 68}[fam]
        for D, B in rec.CASES:
            assert sorted(GOLDEN["%s_D%d_B%d" % (fam, D, B)]["debug_offset"]) == sorted(names)


@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_sizes_and_offsets_equal_the_recorded_ones(case):
    import multimodal_vae_amd  # noqa: F401
    from multimodal_vae_amd._lib import call, load
    load()
    fam, D, B = case.split("_")
    want = GOLDEN[case]
    h = call("mmvae_%s_create" % fam, int(D[1:]), int(B[1:]))
    assert h
    for q in ("workspace_bytes", "iw_workspace_bytes", "packed_elems", "param_count"):
        assert int(call("mmvae_%s_%s" % (fam, q), h)) == want[q], q
    got = {n: int(call("mmvae_%s_debug_offset" % fam, h, n.encode())) for n in want["debug_offset"]}
    assert got == want["debug_offset"]
    for unknown in (b"", b"no_such_buffer", b"r5", b"st_e3", b"dz_att" if fam == "coco" else b"y2"):
        assert call("mmvae_%s_debug_offset" % fam, h, unknown) == -1
    call("mmvae_%s_destroy" % fam, h)
