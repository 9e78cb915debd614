"""What the ring-kernel geometry tables decide besides the kernel name, pinned against a recording (no kernel is launched).

``tests/test_kernel_names_cpu.py`` pins the four name queries.  The tables of csrc/conv_p.hip, conv_b3.hip, resblock_p.hip and
resblock_b3.hip answer three more questions that it does not see; ``tests/golden/ring_geometry.json`` holds them, recorded on
the commit named inside it BEFORE the tables replaced the hand-written dispatch:

* the packed-image sizes -- "does a ring geometry exist" decides whether the packed buffer carries the tile image the ring
  kernels DMA from: ``agx_conv_packed_floats`` / ``agx_conv_bwd_packed_floats`` for every 1-D case of ``cases()``,
  ``agx_conv2d_packed_floats`` / ``agx_conv2d_bwd_packed_floats`` for every Conv2d case;
* ``agx_conv_planes_supported`` for every 1-D case;
* name and sizes of the layers ``cases()`` (strides 2, 4, 5, 8) never reaches: a generator with the class-default strides
  (2, 3, 4, 4, 5) (vae.py: CausalVQAE) for the stride-3 geometries ``conv_p<down3>`` / ``conv_p<up3>``, a WaveletLayer in the
  stride-5 block for ``conv_p<same11>`` / ``conv_p<same3>``, strided Conv2d layers with 32 / 64 GEMM rows.

Every row of every table is the answer of some recorded case (``test_every_table_row_is_reached``), except the rows listed in
``UNREACHED`` with the reason.

Regenerate (on the recording commit only): ``python -m tests.test_ring_geometry_cpu <commit hash>``.
"""
import ctypes
import hashlib
import json
import os
import sys

from audio_generation_amd import _lib
from tests.test_kernel_names_cpu import (AUTO, BF16X3, CAUSAL, FIXTURE as NAMES_FIXTURE, IMPLS, LEAKY_PRE, SAME, TRANSPOSED, UPSAMPLE,
                                         _c2d, _conv, _out_len, cases, key, query)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ring_geometry.json")
DEFAULT_STRIDES = (2, 3, 4, 4, 5)


def default_stride_layers(lib, b, clip):
    """generator_layers() of tests/test_kernel_names_cpu.py for the class-default strides: six channel counts 32 .. 1024."""
    ch = [32 << i for i in range(6)]
    out, length = [("conv", _conv(CAUSAL, b, 1, 32, clip, 7))], clip
    for i, s in enumerate(DEFAULT_STRIDES):
        out += [("resblock", _conv(CAUSAL, b, ch[i], ch[i], length, 7, 1, 3 ** j)) for j in range(3)]
        down = _conv(CAUSAL, b, ch[i], ch[i + 1], length, 2 * s + 1, s, 1, LEAKY_PRE)
        out.append(("conv", down))
        length = _out_len(lib, down)
    out.append(("conv", _conv(CAUSAL, b, 1024, 1024, length, 3)))
    out.append(("conv", _conv(TRANSPOSED, b, 1024, 1024, length, 7, 1)))
    for i in range(4, -1, -1):
        s = DEFAULT_STRIDES[i]
        out.append(("conv", _conv(UPSAMPLE, b, ch[i + 1], ch[i], length, 2 * s + 1, s, 1, LEAKY_PRE)))
        length *= s
        out += [("resblock", _conv(CAUSAL, b, ch[i], ch[i], length, 7, 1, 3 ** j)) for j in range(3)]
    out.append(("conv", _conv(CAUSAL, b, 32, 1, length, 7)))
    return out


# WaveletLayer in the stride-5 decoder block (wavelets.py: Conv1d(K = 11, "same") 256 -> 4 x 128, Conv1d(K = 3, "same") 512 -> 128):
# cases() puts the WaveletLayer into the stride-4 block, whose K = 9 has no ring geometry
WAVELET5 = [_conv(SAME, 32, 256, 512, 1125, 11), _conv(SAME, 32, 512, 128, 5625, 3, 1, 1, LEAKY_PRE)]
# Conv2d layers whose forward / backward-data GEMM has M = 32 or 64 rows on the strided bf16x3 forms (batch 2, 22 x 64 maps)
C2D_FEW_ROWS = [_c2d(2, 64, 32, 22, 64, 4, 4, 2, 2, 1, 1), _c2d(2, 64, 64, 22, 64, 4, 4, 2, 2, 1, 1), _c2d(2, 32, 32, 21, 64, 3, 4, 1, 2, 1, 1),
                _c2d(2, 16, 32, 21, 64, 3, 4, 1, 2, 1, 1), _c2d(2, 8, 32, 22, 64, 4, 4, 2, 2, 1, 1), _c2d(2, 16, 32, 22, 64, 4, 4, 2, 2, 1, 1)]


def extra_cases():
    """Cases in the form of cases(): the default-stride generator at batch 32 / 1, the full clip and a ragged one; WAVELET5;
    C2D_FEW_ROWS."""
    lib = _lib.load()
    out, seen = [], set()
    for f in WAVELET5:
        out += [("conv", f + (impl,), 1, 1) for impl in (AUTO, BF16X3)]
    for f in C2D_FEW_ROWS:
        out += [(op, f + (impl,), 1, 1) for impl in (AUTO, BF16X3) for op in ("conv2d", "conv2d_bwd")]
    for b in (32, 1):
        for clip in (72000, 71999):
            for op, f in default_stride_layers(lib, b, clip):
                for impl in (IMPLS if clip == 72000 else (AUTO, BF16X3)):
                    for ci in (1, 0):
                        for rb in ((1, 0) if op == "resblock" else (1,)):
                            case = (op, f + (impl,), ci, rb)
                            if case not in seen:
                                seen.add(case)
                                out.append(case)
    return out


def sizes(lib, case):
    """1-D: [packed floats, backward packed floats, agx_conv_planes_supported]; Conv2d: [packed floats of the case's direction]."""
    op, f, ci, rb = case
    lib.agx_set_tuning(b"conv_impl", ci)
    lib.agx_set_tuning(b"rb_impl", rb)
    try:
        if op in ("conv", "resblock"):
            d = _lib.ConvDesc(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], 0.1, f[11], f[9], f[10])
            return [int(lib.agx_conv_packed_floats(ctypes.byref(d))), int(lib.agx_conv_bwd_packed_floats(ctypes.byref(d))),
                    int(lib.agx_conv_planes_supported(ctypes.byref(d)))]
        d = _lib.Conv2dDesc(*f[:12], 0.2, f[12])
        fn = lib.agx_conv2d_packed_floats if op == "conv2d" else lib.agx_conv2d_bwd_packed_floats
        return [int(fn(ctypes.byref(d)))]
    finally:
        lib.agx_set_tuning(b"conv_impl", 1)
        lib.agx_set_tuning(b"rb_impl", 1)


def _grid_hash(grid, extra):
    return hashlib.sha256("\n".join(key(c) for c in grid + extra).encode()).hexdigest()[:16]


# every row of the geometry tables, by its pinned name
ROWS = (
    [f"conv_p<{n}>" for n in ("down2,64x256", "down3,128x128", "down4,128x128", "down5,128x128", "down8,128x64", "k3,128x64", "k7,128x64",
                              "up8,128x64", "up5,128x128", "up4,128x128", "up3,64x256", "up2,64x256", "k1,128x128", "same11,128x128",
                              "same3,128x64")] +
    [f"conv_p2d<{n}>" for n in ("k3,128x128", "k3,64x256", "k3,32x512", "k4s2,128x128", "k4s2,64x256", "bwd s(1,2),128x128",
                                "bwd s(1,2),64x256", "bwd s(2,2),128x128")] +
    [f"conv_b3<{n}>" for n in ("up2,64x256", "up4,128x128", "up5,128x128", "up8,128x128", "k7,128x128", "k3,128x128", "down2,64x128",
                               "down4,128x64", "down5,128x64", "down8,128x32")] +
    [f"conv2d_b3<{t},{m}>" for t in ("3x3", "2x2 phases 2x2", "3x2 phases 1x2", "4x4 s2 as 2x2 s2d", "3x4 s(1,2) as 3x2 s2d")
     for m in ("128x128", "64x256", "32x256")] +
    [f"resblock_p<{n}>" for n in ("1,4,8", "2,2,8", "4,1,4", "8,1,4")] +
    [f"resblock_b3<{n}>" for n in ("1,4,x2", "2,2,x2", "4,1,x2", "8,1")])
# rows no recorded descriptor reaches: the strided bf16x3 Conv2d forms on the 64- / 32-row tiles.  The Conv2d selectors (conv2d.hip)
# send the M = 32 / 64 layers of C2D_FEW_ROWS to conv_mfma or conv_p2d first; the instantiations stay
UNREACHED = {"conv2d_b3<2x2 phases 2x2,32x256>", "conv2d_b3<2x2 phases 2x2,64x256>", "conv2d_b3<3x2 phases 1x2,32x256>",
             "conv2d_b3<4x4 s2 as 2x2 s2d,32x256>", "conv2d_b3<4x4 s2 as 2x2 s2d,64x256>"}


def _reached(fixture):
    names = json.load(open(NAMES_FIXTURE))["names"] + fixture["names"]
    return {r for r in ROWS if any(r in n for n in names)}


def test_sizes_and_plane_support_match_the_recording():
    lib = _lib.load()
    fixture = json.load(open(FIXTURE))
    grid, extra = cases(), extra_cases()
    assert len(grid) == len(fixture["values"]) and len(extra) == len(fixture["extra_values"]) == len(fixture["extra_names"])
    assert _grid_hash(grid, extra) == fixture["grid_sha256"], "cases() / extra_cases() are no longer the grid the recording was made on"
    rows, names = fixture["rows"], fixture["names"]
    wrong = []
    for case, want in zip(grid + extra, fixture["values"] + fixture["extra_values"]):
        got = sizes(lib, case)
        if got != rows[want]:
            wrong.append((key(case), rows[want], got))
    assert not wrong, f"{len(wrong)} packed sizes / plane answers differ from the recording, e.g. {wrong[:5]}"
    for case, want in zip(extra, fixture["extra_names"]):
        got = query(lib, case)
        if got != (want if want < 0 else names[want]):
            wrong.append((key(case), want if want < 0 else names[want], got))
    assert not wrong, f"{len(wrong)} kernel names of the default-stride generator differ from the recording, e.g. {wrong[:5]}"
    # both answers of the plane query, and both of "has a tile image", occur
    assert {r[2] for r in rows if len(r) == 3} == {0, 1, 2}


def test_every_table_row_is_reached():
    reached = _reached(json.load(open(FIXTURE)))
    assert set(ROWS) - reached == set(UNREACHED), sorted(set(ROWS) - reached)


def record(commit):
    lib = _lib.load()
    grid, extra = cases(), extra_cases()
    rows, names = [], []

    def index(table, v):
        if v not in table:
            table.append(v)
        return table.index(v)

    values = [index(rows, sizes(lib, c)) for c in grid]
    extra_values = [index(rows, sizes(lib, c)) for c in extra]
    extra_names = []
    for c in extra:
        got = query(lib, c)
        extra_names.append(got if isinstance(got, int) else index(names, got))
    blob = {"recorded_on": commit,
            "format": "values[i] answers cases()[i] of tests/test_kernel_names_cpu.py, extra_values[i] / extra_names[i] answer "
                      "extra_cases()[i] of tests/test_ring_geometry_cpu.py.  A value is an index into rows: [agx_conv_packed_floats, "
                      "agx_conv_bwd_packed_floats, agx_conv_planes_supported] of a 1-D case, [agx_conv2d_packed_floats] of a conv2d "
                      "case, [agx_conv2d_bwd_packed_floats] of a conv2d_bwd case.  A name is an index into names, or the negative "
                      "return code",
            "grid_sha256": _grid_hash(grid, extra), "names": names, "rows": rows, "values": values, "extra_names": extra_names,
            "extra_values": extra_values}
    with open(FIXTURE, "w") as fh:
        json.dump(blob, fh, separators=(",", ":"))
    print(len(values), "+", len(extra_values), "entries,", len(rows), "rows,", len(names), "names,", os.path.getsize(FIXTURE), "bytes")
    print("rows of the tables no recorded case reaches:", sorted(set(ROWS) - _reached(blob)))


if __name__ == "__main__":
    record(sys.argv[1])
