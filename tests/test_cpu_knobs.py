"""The library's knob table (csrc/knobs.h) through the C boundary -- mmvae_debug_set / _get / _reset / _knob_name -- and the
Python helper ``_lib.knobs``.  No device is needed: the table is host state."""
import ctypes as C
import glob
import os
import re

import pytest

from multimodal_vae_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multimodal-vae_amd", "csrc")
EINVAL = -1
# (name, default, kind) of every KNOB(...) line of the table
TABLE = [(n, int(d), k) for n, d, k in re.findall(r'^\s*KNOB\((\w+), (-?\d+), (AB|TUNE|MEASURE|ADDR), "', open(os.path.join(CSRC, "knobs.h")).read(), re.M)]
MEASURE = {"dbg_skip_wgrad", "dbg_skip_text", "dbg_skip_edges", "dbg_begin_skip", "dbg_begin_skip_zero", "dbg_text_rows_div", "wr_dbg",
           "convres_dbg", "dec_last_ca_dbg"}


@pytest.fixture()
def lib():
    lib = _lib.load()
    assert lib.mmvae_debug_reset(None) == 0
    yield lib
    assert lib.mmvae_debug_reset(None) == 0


def _get(lib, name):
    v, d = C.c_int(-12345), C.c_int(-12345)
    assert lib.mmvae_debug_get(name.encode(), C.byref(v), C.byref(d)) == 0
    return v.value, d.value


def _names(lib):
    out = []
    while lib.mmvae_debug_knob_name(len(out)) is not None:
        out.append(lib.mmvae_debug_knob_name(len(out)).decode())
    return out


def _state(lib):
    return {n: _get(lib, n)[0] for n, _, _ in TABLE}


def test_every_entry_reads_back_its_default(lib):
    assert len(TABLE) >= 63 and len({n for n, _, _ in TABLE}) == len(TABLE)
    assert _names(lib) == [n for n, _, _ in TABLE]
    assert lib.mmvae_debug_knob_name(len(TABLE)) is None and lib.mmvae_debug_knob_name(-1) is None       # K_COUNT and past either end
    for n, d, _ in TABLE:
        assert _get(lib, n) == (d, d), n
    assert {n for n, _, k in TABLE if k == "MEASURE"} == MEASURE
    assert {n for n, _, k in TABLE if k == "ADDR"} == {p + h for p in ("convres_ts", "wr_ts", "txt_ts") for h in ("_lo", "_hi")}


@pytest.mark.parametrize("name", ["pack_runs", "wr_atomic_kb", "dbg_skip_wgrad", "wr_ts_hi"])      # AB, TUNE, MEASURE, ADDR
def test_set_get_reset_round_trip(lib, name):
    kind = {n: k for n, _, k in TABLE}
    assert [kind[n] for n in ("pack_runs", "wr_atomic_kb", "dbg_skip_wgrad", "wr_ts_hi")] == ["AB", "TUNE", "MEASURE", "ADDR"]
    dflt = _get(lib, name)[1]
    before = _state(lib)
    for value in (dflt + 7, -2 ** 31, 2 ** 31 - 1):
        assert lib.mmvae_debug_set(name.encode(), value) == 0
        assert _get(lib, name) == (value, dflt)
        assert lib.mmvae_debug_get(name.encode(), None, None) == 0                  # either out pointer may be NULL
        v = C.c_int()
        assert lib.mmvae_debug_get(name.encode(), C.byref(v), None) == 0 and v.value == value
        assert {k: x for k, x in _state(lib).items() if k != name} == {k: x for k, x in before.items() if k != name}
    assert lib.mmvae_debug_reset(name.encode()) == 0
    assert _state(lib) == before


def test_reset_null_restores_everything(lib):
    before = _state(lib)
    for i, (n, d, _) in enumerate(TABLE[::5]):
        assert lib.mmvae_debug_set(n.encode(), d + 1 + i) == 0
    assert sum(a != b for a, b in zip(_state(lib).values(), before.values())) == len(TABLE[::5])
    assert lib.mmvae_debug_reset(None) == 0
    assert _state(lib) == before == {n: d for n, d, _ in TABLE}


def test_unknown_name_is_refused_and_changes_nothing(lib):
    before = _state(lib)
    v, d = C.c_int(77), C.c_int(78)
    for rc in (lib.mmvae_debug_set(b"wgrad_rnig", 0), lib.mmvae_debug_get(b"wgrad_rnig", C.byref(v), C.byref(d)), lib.mmvae_debug_reset(b"wgrad_rnig")):
        assert rc == EINVAL
        assert "wgrad_rnig" in lib.mmvae_last_error().decode()
    assert (v.value, d.value) == (77, 78)
    assert lib.mmvae_debug_set(None, 1) == EINVAL and lib.mmvae_debug_get(None, C.byref(v), C.byref(d)) == EINVAL
    assert lib.mmvae_debug_set(b"", 1) == EINVAL and lib.mmvae_debug_set(b"wgrad_ring ", 0) == EINVAL and lib.mmvae_debug_set(b"K_wgrad_ring", 0) == EINVAL
    with pytest.raises(_lib.MMVAEError, match="wgrad_rnig"):
        _lib.call("mmvae_debug_set", b"wgrad_rnig", 0)
    assert _state(lib) == before


def test_knobs_helper_restores_on_exit_and_on_exception(lib):
    before = _state(lib)
    with _lib.knobs(wgrad_ring=0, coco_cluster=4):
        assert _get(lib, "wgrad_ring")[0] == 0 and _get(lib, "coco_cluster")[0] == 4
        with _lib.knobs(coco_cluster=0):
            assert _get(lib, "coco_cluster")[0] == 0
        assert _get(lib, "coco_cluster")[0] == 8                    # the inner block's names are back at the DEFAULT
    assert _state(lib) == before
    with pytest.raises(ZeroDivisionError):
        with _lib.knobs(adam_blocks=3, wr_pair=1):
            assert _get(lib, "adam_blocks")[0] == 3
            1 / 0
    assert _state(lib) == before
    assert lib.mmvae_debug_set(b"side_lanes", 1) == 0               # exactly the named ones: another knob keeps what it was set to
    with _lib.knobs(ev_flags=0):
        pass
    assert _get(lib, "side_lanes")[0] == 1 and _get(lib, "ev_flags")[0] == 2
    assert lib.mmvae_debug_reset(b"side_lanes") == 0
    with pytest.raises(_lib.MMVAEError, match="no_such_knob"):      # a bad name raises, and what was set in front of it is put back
        with _lib.knobs(pack_runs=0, no_such_knob=1):
            pytest.fail("the block must not run")
    assert _state(lib) == before
    assert _lib.knob_default("coco_cluster") == 8


def test_knob_ptr_halves():
    class T:
        def data_ptr(self):
            return 0x7F12_8000_FFFF_0010

    kw = _lib.knob_ptr("wr_ts", T())
    assert set(kw) == {"wr_ts_lo", "wr_ts_hi"}
    assert ((kw["wr_ts_hi"] & 0xFFFFFFFF) << 32) | (kw["wr_ts_lo"] & 0xFFFFFFFF) == 0x7F12_8000_FFFF_0010
    assert all(-2 ** 31 <= v < 2 ** 31 for v in kw.values())
    assert _lib.knob_ptr("txt_ts", None) == {"txt_ts_lo": 0, "txt_ts_hi": 0}


def test_table_and_sources_agree():
    """every entry is read somewhere (no dead entries), and the string form of the call is gone"""
    text = ""
    for p in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")):
        if os.path.basename(p) != "knobs.h":
            text += open(p).read()
    for n, _, _ in TABLE:
        assert re.search(r"\bK_%s\b" % n, text), "knob %s is in the table and nothing reads it" % n
    for p in glob.glob(os.path.join(CSRC, "*")):
        assert 'mmvae_knob("' not in open(p, errors="replace").read(), p


def test_mnist_strip_route_follows_the_knob(lib):
    assert lib.mmvae_mnist_strip_route(2) == 1                      # -1, the default: on
    with _lib.knobs(mnist_strip=0):
        assert lib.mmvae_mnist_strip_route(2) == 0
    assert lib.mmvae_mnist_strip_route(2) == 1
    with _lib.knobs(mnist_strip=1):
        assert lib.mmvae_mnist_strip_route(2) == 1
