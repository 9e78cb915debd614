"""The names the three tile families answer with, pinned under every selection knob their host code reads.

``tests/golden/kernel_names.json`` pins the name queries at default knobs.  The tile families -- csrc/conv_mfma.hip,
csrc/resblock_mfma.hip, csrc/conv_direct.hip: the fallback of every layer a ring kernel refuses -- also read ``conv_cc``,
``conv_shape``, ``conv_short``, ``rb_cc`` and ``patch_tie`` when they choose a variant.  ``tests/golden/tile_kernel_names.json``
holds the answer (the name, or the negative return code) of the four host-only name queries for every descriptor of
``tests/test_kernel_names_cpu.py`` (plus the DIRECT and BF16X3 forms of each 1-D one), with ``conv_impl = rb_impl = 0`` so that
the tile families answer, under each setting of ``SETTINGS``.  It was recorded on the commit named inside it, BEFORE each family
got one variant table that name query, fit test and launcher share; a row of a table that moves, or a rule of a selector that
changes, changes some entry.  No kernel is launched.

Regenerate (on the recording commit only): ``python -m tests.test_tile_variants_cpu <commit hash>``.
"""
import ctypes
import json
import os
import sys

from audio_generation_amd import _lib
from tests import test_kernel_names_cpu as names

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_kernel_names.json")
SETTINGS = [{}, {"conv_cc": 8}, {"conv_cc": 16}, {"conv_cc": 32}, {"conv_shape": 1}, {"conv_short": 0},
            {"conv_shape": 1, "conv_short": 0}, {"rb_cc": 32}, {"patch_tie": 0}]
KNOBS = ("conv_impl", "rb_impl", "conv_cc", "conv_shape", "conv_short", "rb_cc", "patch_tie")
DEFAULTS = {"conv_impl": 1, "rb_impl": 1, "conv_cc": 0, "conv_shape": 0, "conv_short": 1, "rb_cc": 16, "patch_tie": 1}


# rows of the direct tables the names test's list does not reach: 2..4 and 5..8 rows off the streaming shape
EXTRA = [("conv", names._conv(names.CAUSAL, 2, 16, 3, 100, 3) + (names.AUTO,)),
         ("conv", names._conv(names.CAUSAL, 2, 16, 7, 100, 5, 2) + (names.AUTO,))]


def grid():
    """[(op, descriptor fields incl. impl)]: each descriptor of the names test once, 1-D ones also as DIRECT and BF16X3."""
    out = {}
    for op, f in [c[:2] for c in names.cases()] + EXTRA:
        out.setdefault((op, f))
        if op in ("conv", "resblock"):
            for impl in (names.DIRECT, names.BF16X3):
                out.setdefault((op, f[:-1] + (impl,)))
    return list(out)


def setting_key(setting):
    return ",".join(f"{k}={v}" for k, v in setting.items()) or "default"


def knobs(lib):
    return {k: lib.agx_get_tuning(k.encode()) for k in KNOBS}


def answers(lib, setting, cases):
    """The name, or the (negative) return code, of every case under `setting` on the tile families."""
    out, buf = [], ctypes.create_string_buffer(96)
    try:
        for k, v in {"conv_impl": 0, "rb_impl": 0, **setting}.items():
            assert lib.agx_set_tuning(k.encode(), v) == 0, k
        for op, f in cases:
            if op in ("conv", "resblock"):
                d = _lib.ConvDesc(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], 0.1, f[11], f[9], f[10])
            else:
                d = _lib.Conv2dDesc(*f[:12], 0.2, f[12])
            rc = getattr(lib, names.QUERY[op])(ctypes.byref(d), buf, len(buf))
            out.append(buf.value.decode() if rc == 0 else int(rc))
    finally:
        for k, v in DEFAULTS.items():
            lib.agx_set_tuning(k.encode(), v)
    return out


def _grid_hash(cases):
    return names._grid_hash([(op, f, 0, 0) for op, f in cases])


def test_tile_kernel_names_match_the_recording_under_every_selection_knob():
    lib = _lib.load()
    fixture = json.load(open(FIXTURE))
    table, cases = fixture["names"], grid()
    assert knobs(lib) == DEFAULTS
    assert len(cases) > 2000 and _grid_hash(cases) == fixture["grid_sha256"], "grid() is no longer the grid of the recording"
    assert list(fixture["values"]) == [setting_key(s) for s in SETTINGS]
    wrong, seen = [], set()
    for setting in SETTINGS:
        want = [v if v < 0 else table[v] for v in fixture["values"][setting_key(setting)]]
        got = answers(lib, setting, cases)
        assert knobs(lib) == DEFAULTS, setting
        assert len(got) == len(want)
        wrong += [(setting_key(setting), names.key(c + (0, 0)), w, g) for c, w, g in zip(cases, want, got) if w != g]
        seen.update(g for g in got if not isinstance(g, int))
    assert not wrong, f"{len(wrong)} tile kernel names differ from the recording, e.g. {wrong[:5]}"
    # with the ring kernels off every answer is a tile family's (or a Conv2d form that has no ring / tile choice), and the
    # settings reach the forced chunks, the alternative 128-row shapes and the 32-channel residual block
    assert not any(n.startswith(("conv_p<", "conv_b3<", "resblock_p<", "resblock_b3<")) for n in seen)
    for n in ("conv_mfma<2,2,2,2,16>", "conv_mfma<2,2,2,2,8>", "conv_mfma<2,2,2,2,32>", "conv_mfma<1,2,4,1,16>", "conv_mfma<1,4,4,1,16>",
              "conv_mfma<2,1,1,4,16>", "conv_mfma<1,1,1,4,16>", "conv_mfma<1,4,1,4,32>", "resblock_mfma<1,4,32>", "resblock_mfma<8,1,16>",
              "resblock_mfma<2,2,16>:bf16x3", "conv_narrow<16>", "conv_narrow<1>", "conv_fewrows<16>", "conv_fewrows<8>", "conv_fewrows<4>", "conv_fewrows<1>",
              "conv_direct<32>", "conv_direct<16>", "conv_direct<4>", "conv_direct<1>", "2x:conv_direct<32>"):
        assert n in seen, n


def record(commit):
    lib = _lib.load()
    cases, table, values = grid(), [], {}
    for setting in SETTINGS:
        row = []
        for got in answers(lib, setting, cases):
            if not isinstance(got, int):
                if got not in table:
                    table.append(got)
                got = table.index(got)
            row.append(got)
        values[setting_key(setting)] = row
    blob = {"recorded_on": commit,
            "format": "values[setting][i] answers grid()[i] of tests/test_tile_variants_cpu.py with conv_impl = rb_impl = 0 and the "
                      "knobs of `setting`: an index into names, or the negative return code",
            "grid_sha256": _grid_hash(cases), "names": table, "values": values}
    with open(FIXTURE, "w") as fh:
        json.dump(blob, fh, separators=(",", ":"))
    print(len(cases), "descriptors x", len(SETTINGS), "settings,", len(table), "names,", os.path.getsize(FIXTURE), "bytes")
    print("\n".join(sorted(table)))


if __name__ == "__main__":
    record(sys.argv[1])
