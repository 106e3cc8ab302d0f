"""Records tests/golden/tower_layout.json: the host-side sizes and the workspace layout of the CelebA and COCO plans::

    python tools/record_tower_layout.py

For each family at (n_latents, batch) = (20, 4) and (100, 8): workspace_bytes, iw_workspace_bytes, packed_elems, param_count and
the debug_offset of every named workspace buffer.  Plans are created and carved on the host, so no GPU is needed.
tests/test_cpu_tower_layout.py asserts equality with the file: record it from the commit whose layout is to be kept, by hand.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(20, 4), (100, 8)]
_TABLES = ["%s_%s%d" % (t, h, i) for t in ("st", "red", "aff", "mr") for h in "ed" for i in range(3)]
_COMMON = ("patches1 r1 r2 r3 r4 a1 a2 a3 a4 y1 ay1 encout m1 z_bf z_f32 u au q1 q2 q3 aq1 aq2 aq3 dlogit patches4 d3 d2 d1 du dz_img "
           "d_encout dy1 db4 dr4 d3e d2e d1e tmp_f32 slab").split() + _TABLES
NAMES = {"celeba": _COMMON + ["dz_att"], "coco": _COMMON + ["y2", "ay2", "m2", "dy2", "sums"]}


def record():
    import multimodal_vae_amd  # noqa: F401
    from multimodal_vae_amd._lib import call, load
    load()
    out = {}
    for fam, names in sorted(NAMES.items()):
        for D, B in CASES:
            h = call("mmvae_%s_create" % fam, D, B)
            rec = {q: int(call("mmvae_%s_%s" % (fam, q), h)) for q in ("workspace_bytes", "iw_workspace_bytes", "packed_elems", "param_count")}
            rec["debug_offset"] = {n: int(call("mmvae_%s_debug_offset" % fam, h, n.encode())) for n in sorted(names)}
            assert min(rec["debug_offset"].values()) >= 0, rec["debug_offset"]
            call("mmvae_%s_destroy" % fam, h)
            out["%s_D%d_B%d" % (fam, D, B)] = rec
    return out


if __name__ == "__main__":
    path = os.path.join(ROOT, "tests", "golden", "tower_layout.json")
    with open(path, "w") as f:
        json.dump(record(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")
