"""The three weight-gradient name queries and their workspace sizes, pinned entry for entry against a recording (host only:
no kernel is launched).

``agx_conv_bwd_weight_kernel_name`` / ``agx_conv2d_bwd_weight_kernel_name`` / ``agx_conv_grouped_bwd_weight_kernel_name``
print what their launcher runs: instantiation, ``cfg``, operand copy, contraction slices and items; the matching
``*_workspace_bytes`` is what the launcher carves its partial tiles and operand copies out of.  Both follow from the geometry
functions of csrc/conv_bwd_weight.hip (and csrc/conv_grouped_bwd.hip), so the order of their
branches, the tile ladder, the slice clamp and the workspace layout all show up here.
``tests/golden/wgrad_kernel_names.json`` holds, for every case of ``cases()``, the full string (or the negative return code;
stored as its part up to ``op=``, the slices and the items: ``load_recording``) and the byte count, recorded on the commit named inside it BEFORE the host side was rewritten around one variant table.

The grid (``cases()``):

* every conv / residual-block conv / Conv2d layer tests/test_kernel_names_cpu.py enumerates (generator, wavelet variant,
  attention projections, waveform discriminator -- its grouped layers on the grouped op as well --, the five STFT
  discriminators), batch 32 and 1, full clip / sub-tile clip / two ragged clips; ``impl`` AUTO and BF16X3;
* each selection knob at every value it distinguishes, one knob off its default at a time: ``dw_direct`` 0..3, ``dw1_wgs``
  1 / 768 / 1024 (1-D op); ``dw2_direct`` 0..2, ``dw2_shared`` 0..2, ``dw2_prepad`` 0 / 1, ``dw2_bf`` 0 / 1, ``dw_wgs``
  1 / 1536 / 2048 (2-D op).  The grouped op reads no knob;
* the Conv2d shapes of tests/test_gpu_conv2d_b3.py (its narrow maps included); dense 1-D layers that stay on the staged
  kernel at the default knobs (stride or phase count above 16, stride and phases together); layers with too few rows or
  columns for any tile; descriptors the ops refuse.

Reachability (checked by ``test_the_grid_reaches_every_instantiation``): all 16 instantiations of the 1-D op, all 17 of the
2-D op and every ``op=`` value occur in the recording.  ``conv2d_bwd_weight_shared<1,2,1,4>`` (cfg 16) and the three
staged 1-D ``...,1>`` (bf16x3) kernels are reached at the default knobs; none is unreachable.

Regenerate (on the recording commit only): ``python -m tests.test_wgrad_kernel_names_cpu <commit hash>``.
"""
import ctypes
import hashlib
import json
import os
import sys

from audio_generation_amd import _lib
from tests.test_kernel_names_cpu import (AUTO, BF16X3, C2B3, CAUSAL, PADDED, SAME, TRANSPOSED, UPSAMPLE, _c2d, _conv,
                                         attention_layers, generator_layers, stft_disc_layers, waveform_disc_layers)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_kernel_names.json")
QUERY = {"w1": ("agx_conv_bwd_weight_kernel_name", "agx_conv_bwd_weight_workspace_bytes"),
         "w2": ("agx_conv2d_bwd_weight_kernel_name", "agx_conv2d_bwd_weight_workspace_bytes"),
         "wg": ("agx_conv_grouped_bwd_weight_kernel_name", "agx_conv_grouped_bwd_weight_workspace_bytes")}
# knob -> (default, the other values it distinguishes)
KNOBS = {"w1": {"dw_direct": (3, (0, 1, 2)), "dw1_wgs": (768, (1, 1024))},
         "w2": {"dw2_direct": (2, (0, 1)), "dw2_shared": (2, (0, 1)), "dw2_prepad": (1, (0,)), "dw2_bf": (1, (0,)),
                "dw_wgs": (1536, (1, 2048))},
         "wg": {}}
BW1 = ["conv_bwd_weight_direct<2,2,2,2>", "conv_bwd_weight_direct<2,2,1,2>", "conv_bwd_weight_direct<2,2,1,1>",
       "conv_bwd_weight_direct<1,2,1,4>", "conv_bwd_weight_direct<1,1,1,1>",
       "conv_bwd_weight_direct<2,2,2,2,true>", "conv_bwd_weight_direct<2,2,1,2,true>", "conv_bwd_weight_direct<2,2,1,1,true>",
       "conv_bwd_weight_direct<1,2,1,4,true>", "conv_bwd_weight_direct<1,1,1,1,true>",
       "conv_bwd_weight<2,2,2,2>", "conv_bwd_weight<1,2,2,2>", "conv_bwd_weight<1,1,1,4>",
       "conv_bwd_weight<2,2,2,2,1>", "conv_bwd_weight<1,2,2,2,1>", "conv_bwd_weight<1,1,1,4,1>"]
BW2 = ["conv2d_bwd_weight_shared<2,2,2,2>", "conv2d_bwd_weight_shared<2,2,2,2,1>", "conv2d_bwd_weight_shared<2,1,1,4>",
       "conv2d_bwd_weight_shared<2,1,1,4,1>", "conv2d_bwd_weight_shared<1,2,1,4>",
       "conv2d_bwd_weight_direct<2,2,2,2>", "conv2d_bwd_weight_direct<2,2,1,2>", "conv2d_bwd_weight_direct<2,2,1,1>",
       "conv2d_bwd_weight_direct<1,2,1,4>", "conv2d_bwd_weight_direct<1,3,1,1>", "conv2d_bwd_weight_direct<1,1,1,1>",
       "conv2d_bwd_weight<2,2,2,2>", "conv2d_bwd_weight<1,2,2,2>", "conv2d_bwd_weight<1,1,1,4>",
       "conv2d_bwd_weight<2,2,2,2,1>", "conv2d_bwd_weight<1,2,2,2,1>", "conv2d_bwd_weight<1,1,1,4,1>"]
OPS = ("none", "phase_x", "phase_dy", "prepad", "deinterleave")

# dense 1-D layers off the production path: stride / phase count above 16 and stride together with phases (staged kernel
# at the default knobs, every row-tile height), few rows and few columns (the small direct tiles, plain and phase-split),
# one position, an LDS patch the staged kernel has no room for
C1D_EXTRA = [_conv(CAUSAL, 2, 64, 128, 4000, 35, 17), _conv(CAUSAL, 2, 64, 64, 4000, 41, 20), _conv(CAUSAL, 2, 16, 32, 4000, 35, 17),
             _conv(UPSAMPLE, 2, 64, 4, 200, 35, 17), _conv(TRANSPOSED, 2, 64, 2, 200, 40, 20), _conv(TRANSPOSED, 2, 256, 8, 200, 40, 20),
             _conv(CAUSAL, 2, 4, 64, 500, 3), _conv(CAUSAL, 2, 4, 32, 500, 3), _conv(CAUSAL, 2, 4, 16, 500, 7), _conv(CAUSAL, 2, 8, 40, 500, 7),
             _conv(CAUSAL, 2, 4, 64, 500, 5, 2), _conv(CAUSAL, 2, 4, 32, 500, 5, 2), _conv(CAUSAL, 2, 4, 16, 500, 9, 4), _conv(CAUSAL, 2, 8, 40, 500, 9, 4),
             _conv(CAUSAL, 2, 64, 200, 500, 5, 2), _conv(UPSAMPLE, 2, 64, 8, 77, 5, 2), _conv(UPSAMPLE, 2, 4, 4, 77, 5, 2), _conv(TRANSPOSED, 2, 128, 64, 77, 8, 4),
             _conv(CAUSAL, 1, 64, 64, 1, 7), _conv(SAME, 2, 64, 64, 501, 11), _conv(SAME, 2, 64, 64, 501, 5, 1, 2), _conv(CAUSAL, 2, 48, 24, 333, 7, 1, 3),
             _conv(CAUSAL, 1, 32, 32, 4000, 1001, 17), _conv(CAUSAL, 1, 32, 32, 1 << 24, 7), _conv(CAUSAL, 70000, 32, 32, 64, 7)]
# refused: unknown kind, no input channels, no length, a kernel the grouped op does not take (groups = 1 is accepted there)
C1D_REFUSED = [_conv(7, 2, 64, 64, 100, 3), _conv(CAUSAL, 2, 0, 64, 100, 3), _conv(CAUSAL, 2, 64, 64, 0, 3), _conv(PADDED, 2, 64, 96, 100, 3, 1, 1, 0, 5, 1)]
CG_EXTRA = [_conv(PADDED, 2, 64, 64, 501, 3, 1, 1, 0, 64, 1), _conv(PADDED, 2, 64, 96, 501, 9, 2, 1, 0, 4, 4), _conv(PADDED, 2, 64, 64, 501, 3, 1, 1, 0, 1, 1),
             _conv(CAUSAL, 1, 4, 4, 64, 3), _conv(PADDED, 2, 64, 64, 501, 3, 1, 2, 0, 4, 1), _conv(PADDED, 1, 16, 16, 30, 3, 1, 1, 0, 4, 1)]
# Conv2d layers off the production path: few rows / columns (every small direct tile), the 96-column rung, row-strided and
# unpadded layers, kernels too large for the direct / narrow-map forms, an LDS patch without room, refused descriptors
C2D_EXTRA = [_c2d(2, 3, 5, 20, 33, 3, 3, 1, 1, 1, 1), _c2d(2, 24, 40, 20, 33, 3, 3, 1, 1, 1, 1), _c2d(2, 2, 64, 20, 64, 3, 3, 1, 1, 1, 1),
             _c2d(2, 2, 32, 20, 64, 3, 3, 1, 1, 1, 1), _c2d(2, 2, 128, 20, 64, 3, 3, 1, 1, 1, 1), _c2d(2, 32, 16, 20, 64, 3, 3, 1, 1, 1, 1),
             _c2d(2, 32, 32, 20, 64, 5, 5, 1, 1, 2, 2), _c2d(2, 8, 32, 20, 64, 5, 5, 1, 1, 2, 2),
             _c2d(2, 20, 16, 20, 64, 5, 5, 1, 1, 2, 2), _c2d(2, 64, 32, 20, 64, 3, 3, 1, 1, 1, 1), _c2d(2, 8, 32, 20, 64, 3, 3, 1, 1, 1, 1),
             _c2d(2, 8, 64, 20, 64, 3, 4, 1, 2, 1, 1), _c2d(2, 32, 32, 20, 64, 3, 4, 1, 2, 1, 1), _c2d(2, 64, 64, 20, 96, 3, 5, 1, 3, 1, 1),
             _c2d(2, 64, 64, 20, 64, 5, 3, 2, 1, 2, 1), _c2d(1, 16, 32, 64, 64, 3, 3, 1, 1, 0, 0), _c2d(1, 32, 32, 12, 40, 5, 5, 1, 1, 1, 1),
             _c2d(1, 64, 64, 40, 64, 11, 11, 1, 1, 5, 5), _c2d(1, 64, 64, 40, 16, 9, 9, 1, 1, 4, 4), _c2d(1, 64, 64, 40, 3, 3, 3, 1, 1, 1, 1),
             _c2d(1, 32, 64, 40, 16, 3, 3, 1, 1, 1, 1), _c2d(1, 64, 32, 40, 16, 3, 3, 1, 1, 1, 1), _c2d(2, 48, 1, 20, 33, 1, 5, 1, 1, 0, 2),
             _c2d(1, 16, 64, 40, 4000, 9, 41, 1, 8, 4, 20), _c2d(1, 32, 32, 30, 3000, 31, 31, 1, 1, 15, 15), _c2d(1, 16, 16, 40, 600, 15, 15, 1, 1, 7, 7),
             _c2d(1, 8, 8, 300, 300, 127, 127, 1, 1, 63, 63), _c2d(70000, 32, 32, 4, 32, 3, 3, 1, 1, 1, 1)]
C2D_REFUSED = [_c2d(0, 32, 32, 20, 33, 3, 3, 1, 1, 1, 1), _c2d(1, 32, 32, 2, 2, 5, 5, 1, 1, 0, 0), _c2d(1, 32, 32, 20, 33, 3, 3, 0, 1, 1, 1)]


def cases():
    """[(op, descriptor fields incl. impl, knob, value)] -- a fixed order, each case once; knob "" = all defaults."""
    lib = _lib.load()
    layers = {"w1": [], "w2": [], "wg": []}

    def add1(fields):
        for op, f in fields:
            f = f[:8] + (0,) + f[9:]                                 # the epilogue is no business of the weight gradient
            layers["w1"].append(f)
            if op == "resblock":                                     # ... and the block's second conv, k = 1
                layers["w1"].append(_conv(CAUSAL, f[1], f[2], f[3], f[4], 1))
            if f[9] > 1:
                layers["wg"].append(f)

    for b in (32, 1):
        for clip in (72000, 3200, 72001, 71999):          # full size / 10 frames: under one tile / ragged
            add1(generator_layers(lib, b, 1, clip, (False,) * 4))
        for clip in (144000, 4800, 143999):
            add1(generator_layers(lib, b, 2, clip, (False, True, False, False)))
        for frames in (225, 10, 226):
            add1(attention_layers(b, frames))
        for clip in (72000, 3200, 72001, 71999):
            add1(waveform_disc_layers(lib, b, clip))
        for clip in (72000, 3200, 72001, 71999):
            for win in (2048, 1024, 512, 256, 128):
                layers["w2"] += [f[:11] + (0,) for f in stft_disc_layers(lib, b, clip, win)]
    add1([("conv", f) for f in C1D_EXTRA + C1D_REFUSED])
    layers["wg"] += CG_EXTRA + C1D_REFUSED
    for b, cin, cout, h, w, kh, kw, sh, sw in C2B3:
        layers["w2"].append(_c2d(b, cin, cout, h, w, kh, kw, sh, sw, (kh - 1) // 2, (kw - 1) // 2))
    layers["w2"] += C2D_EXTRA + C2D_REFUSED

    out = []
    for op in ("w1", "wg", "w2"):
        for f in dict.fromkeys(layers[op]):
            for impl in (AUTO, BF16X3):
                out.append((op, f + (impl,), "", 0))
                for knob, (_, values) in KNOBS[op].items():
                    out += [(op, f + (impl,), knob, v) for v in values]
    return out


def key(case):
    op, f, knob, value = case
    return f"{op} {','.join(map(str, f))} {knob}={value}"


def query(lib, case):
    """[the string or the (negative) return code, workspace bytes]."""
    op, f, knob, value = case
    if op == "w2":
        d = _lib.Conv2dDesc(*f[:12], 0.2, f[12])
    else:
        d = _lib.ConvDesc(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], 0.1, f[11], f[9], f[10])
    buf = ctypes.create_string_buffer(128)
    name_fn, bytes_fn = QUERY[op]
    if knob:
        lib.agx_set_tuning(knob.encode(), value)
    try:
        rc = getattr(lib, name_fn)(ctypes.byref(d), buf, len(buf))
        nbytes = int(getattr(lib, bytes_fn)(ctypes.byref(d)))
    finally:
        if knob:
            lib.agx_set_tuning(knob.encode(), KNOBS[op][knob][0])
    return [buf.value.decode() if rc == 0 else int(rc), nbytes]


def _grid_hash(grid):
    return hashlib.sha256("\n".join(key(c) for c in grid).encode()).hexdigest()[:16]


def test_knob_defaults_are_the_ones_the_grid_restores():
    lib = _lib.load()
    for op in KNOBS:
        for knob, (default, _) in KNOBS[op].items():
            assert lib.agx_get_tuning(knob.encode()) == default, knob


def load_recording():
    """(fixture, [[string or negative return code, workspace bytes]] in the order of cases())."""
    fx = json.load(open(FIXTURE))
    heads, ans = fx["heads"], fx["answers"]
    full = [[h if h < 0 else f"{heads[h]} slices={s} items={i}", b]
            for h, s, i, b in zip(ans["head"], ans["slices"], ans["items"], ans["bytes"])]
    return fx, [full[v] for v in fx["values"]]


def test_wgrad_kernel_names_and_workspace_bytes_match_the_recording():
    lib = _lib.load()
    fixture, values = load_recording()
    grid = cases()
    assert len(grid) == len(values) and len(grid) > 5000, (len(grid), len(values))
    assert _grid_hash(grid) == fixture["grid_sha256"], "cases() is no longer the grid the recording was made on"
    wrong = []
    for case, want in zip(grid, values):
        got = query(lib, case)
        if got != want:
            wrong.append((key(case), want, got))
    assert not wrong, f"{len(wrong)} of {len(grid)} entries differ from the recording, e.g. {wrong[:5]}"


def test_the_grid_reaches_every_instantiation():
    values = load_recording()[1]
    names = {v for v, _ in values if not isinstance(v, int)}
    seen = {n.split(" ")[0] for n in names}
    assert [n for n in BW1 + BW2 if n not in seen] == []
    assert any(n.startswith("grouped_bwd_weight ") for n in names) and any(n.startswith("grouped_bwd_weight_tiled<") for n in names)
    for op in OPS:
        assert any(f" op={op} " in n for n in names), op
    assert {-1, -5} <= {v for v, _ in values if isinstance(v, int)}, "bad-argument and unsupported refusals"


def record(commit):
    import collections
    import re
    lib = _lib.load()
    grid = cases()
    got = [tuple(query(lib, case)) for case in grid]
    order = [a for a, _ in collections.Counter(got).most_common()]          # frequent answers get the short indices
    heads, ans = [], {"head": [], "slices": [], "items": [], "bytes": []}
    for name, nbytes in order:
        h, s, i = name, 0, 0
        if not isinstance(name, int):
            head, s, i = re.fullmatch(r"(.*) slices=(\d+) items=(\d+)", name).groups()
            if head not in heads:
                heads.append(head)
            h, s, i = heads.index(head), int(s), int(i)
        for k, v in zip(("head", "slices", "items", "bytes"), (h, s, i, nbytes)):
            ans[k].append(v)
    blob = {"recorded_on": commit,
            "format": "values[i] answers cases()[i] of tests/test_wgrad_kernel_names_cpu.py with answer k = values[i]: the name query "
                      "returned the negative code answers.head[k], or printed '<heads[answers.head[k]]> slices=<answers.slices[k]> "
                      "items=<answers.items[k]>'; the matching *_workspace_bytes returned answers.bytes[k]",
            "grid_sha256": _grid_hash(grid), "heads": heads, "answers": ans, "values": [order.index(g) for g in got]}
    with open(FIXTURE, "w") as fh:
        json.dump(blob, fh, separators=(",", ":"))
    assert [list(g) for g in got] == load_recording()[1]
    print(len(got), "entries,", len(order), "answers,", os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    record(sys.argv[1])
