"""The four host-only kernel-name queries, pinned entry for entry against a recording (no kernel is launched).

``agx_conv_kernel_name`` / ``agx_resblock_kernel_name`` / ``agx_conv2d_kernel_name`` / ``agx_conv2d_bwd_data_kernel_name``
print from the selection function their launcher switches on (csrc/conv_api.hip: conv_kernel / resblock_kernel,
csrc/conv2d.hip: conv2d_kernel / conv2d_bwd_kernel), so "which kernel does this descriptor run on" is decided by the order
of the branches in those four functions.  ``tests/golden/kernel_names.json`` holds the answer (the name, or the negative
return code) for every case of ``cases()``, recorded on the commit named inside it BEFORE the selection was pulled into one
place; reordering or dropping a branch of a selector changes some entry.

The grid (``cases()``):

* every conv / residual-block / Conv2d layer of BASELINE configs S, 3, 4 and 5 -- the generator (mono 24 kHz), its wavelet
  variant (stereo 48 kHz, WaveletLayer in decoder block 2), the attention-bottleneck projections (k = 1), the waveform
  discriminator and the five STFT discriminators -- at batch 32 and batch 1, at the full clip, a clip shorter than one tile
  and two ragged clips (lengths the reference's ``_calc_extra_pad`` pads), with the epilogue the model runs them with;
* ``impl`` AUTO / DIRECT / MFMA / BF16X3; ``conv_impl`` 0 / 1 (and ``rb_impl`` 0 / 1 for the residual block);
* every epilogue bit on every distinct generator layer; the narrow-map Conv2d shapes of tests/test_gpu_conv_p2d.py and
  tests/test_gpu_conv2d_b3.py; channel counts that fit no MFMA tile; descriptors the launchers refuse.

Regenerate (on the recording commit only): ``python -m tests.test_kernel_names_cpu <commit hash>``.
"""
import ctypes
import hashlib
import json
import os
import sys

from audio_generation_amd import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_names.json")
AUTO, DIRECT, MFMA, BF16X3 = _lib.IMPL_AUTO, _lib.IMPL_DIRECT, _lib.IMPL_MFMA, _lib.IMPL_MFMA_BF16X3
IMPLS = (AUTO, DIRECT, MFMA, BF16X3)
CAUSAL, TRANSPOSED, UPSAMPLE, SAME, PADDED = 0, 1, 2, 3, 4
LEAKY_PRE, RESIDUAL, LEAKY_POST, GELU_PRE, MASK = 1, 2, 4, 8, 16
STRIDES = (2, 4, 5, 8)
QUERY = {"conv": "agx_conv_kernel_name", "resblock": "agx_resblock_kernel_name", "conv2d": "agx_conv2d_kernel_name",
         "conv2d_bwd": "agx_conv2d_bwd_data_kernel_name"}


def _conv(kind, b, cin, cout, length, k, s=1, d=1, epi=0, groups=1, pad=0):
    return (kind, b, cin, cout, length, k, s, d, epi, groups, pad)


def _out_len(lib, f):
    d = _lib.ConvDesc(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], 0.1, AUTO, f[9], f[10])
    return int(lib.agx_conv_out_len(ctypes.byref(d)))


def generator_layers(lib, b, in_ch, clip, wavelet):
    """("conv" | "resblock", fields) of one CausalVQAE forward (vae.py: first_block_channels 32, strides (2, 4, 5, 8),
    three residual blocks per block, codebook_dim 512); ``wavelet[i]``: decoder block of stride STRIDES[i] is a WaveletLayer."""
    ch = [32 << i for i in range(5)]
    out, length = [("conv", _conv(CAUSAL, b, in_ch, 32, clip, 7))], clip
    for i, s in enumerate(STRIDES):
        out += [("resblock", _conv(CAUSAL, b, ch[i], ch[i], length, 7, 1, 3 ** j)) for j in range(3)]
        down = _conv(CAUSAL, b, ch[i], ch[i + 1], length, 2 * s + 1, s, 1, LEAKY_PRE)
        out.append(("conv", down))
        length = _out_len(lib, down)
    out.append(("conv", _conv(CAUSAL, b, 512, 512, length, 3)))
    out.append(("conv", _conv(TRANSPOSED, b, 512, 512, length, 7, 1)))
    for i in range(3, -1, -1):
        s = STRIDES[i]
        if wavelet[i]:
            out.append(("conv", _conv(SAME, b, ch[i + 1], 4 * ch[i], length, 2 * s + 1)))
            out.append(("conv", _conv(SAME, b, 4 * ch[i], ch[i], length * s, 3, 1, 1, LEAKY_PRE)))
        else:
            out.append(("conv", _conv(UPSAMPLE, b, ch[i + 1], ch[i], length, 2 * s + 1, s, 1, LEAKY_PRE)))
        length *= s
        out += [("resblock", _conv(CAUSAL, b, ch[i], ch[i], length, 7, 1, 3 ** j)) for j in range(3)]
    out.append(("conv", _conv(CAUSAL, b, 32, in_ch, length, 7)))
    return out


def attention_layers(b, frames):
    """k = 1 projections of Transformer(512, heads 8 x 64, FFN x 4) on (B, 512, frames): qkv, out + residual, FFN."""
    return [("conv", _conv(CAUSAL, b, 512, 1536, frames, 1)), ("conv", _conv(CAUSAL, b, 512, 512, frames, 1, 1, 1, RESIDUAL)),
            ("conv", _conv(CAUSAL, b, 512, 2048, frames, 1, 1, 1, GELU_PRE)),
            ("conv", _conv(CAUSAL, b, 2048, 512, frames, 1, 1, 1, RESIDUAL))]


def waveform_disc_layers(lib, b, clip):
    """WaveFormDiscriminator(1): three blocks behind AvgPool1d(2 s, s, s), s = 1, 2, 4 (discriminator.py)."""
    spec = [(1, 16, 15, 1, 1), (16, 64, 41, 4, 4), (64, 256, 41, 4, 16), (256, 512, 41, 4, 64), (512, 1024, 41, 4, 256),
            (1024, 1024, 5, 1, 1), (1024, 1, 3, 1, 1)]
    out = []
    for scale in (1, 2, 4):
        length = clip // scale + 1
        for n, (cin, cout, k, s, g) in enumerate(spec):
            f = _conv(PADDED, b, cin, cout, length, k, s, 1, LEAKY_PRE if n < 6 else 0, g, 0)
            out.append(("conv", f))
            length = _out_len(lib, f)
            if length <= 0:
                break
    return out


def _c2d(b, cin, cout, h, w, kh, kw, sh=1, sw=1, ph=0, pw=0, epi=0):
    return (b, cin, cout, h, w, kh, kw, sh, sw, ph, pw, epi)


def stft_disc_layers(lib, b, clip, win):
    """STFTDiscriminator(win_length = win): (B, 2, clip / hop + 1, win) through the 7 x 7 conv, six blocks, the (1, fk) conv."""
    h, w, ch, out = clip // (win // 4) + 1, win, 32, []

    def push(f):
        nonlocal h, w
        out.append(f)
        d = _lib.Conv2dDesc(*f, 0.2, AUTO)
        ho, wo = ctypes.c_int32(0), ctypes.c_int32(0)
        if lib.agx_conv2d_out_shape(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)) == 0:
            h, w = ho.value, wo.value

    push(_c2d(b, 2, 32, h, w, 7, 7, 1, 1, 3, 3))
    for mult, (sh, sw) in zip((2, 2, 1, 2, 1, 2), ((1, 2), (2, 2)) * 3):
        push(_c2d(b, ch, ch, h, w, 3, 3, 1, 1, 1, 1, LEAKY_PRE))
        push(_c2d(b, ch, ch * mult, h, w, sh + 2, sw + 2, sh, sw, (sh + 1) // 2, (sw + 1) // 2))
        ch *= mult
    fk = win // 128
    push(_c2d(b, ch, 1, h, w, 1, fk, 1, 1, 0, (fk - 1) // 2))
    return out


# cin, cout, kh, kw, sh, sw, h, w  (tests/test_gpu_conv_p2d.py: FWD and the backward table; batch 3 / 2 there)
P2D = [(64, 64, 3, 3, 1, 1, 7, 250), (64, 64, 3, 3, 1, 1, 3, 512), (128, 128, 3, 3, 1, 1, 6, 250), (128, 128, 3, 3, 1, 1, 5, 253),
       (256, 256, 3, 3, 1, 1, 5, 120), (32, 128, 3, 3, 1, 1, 1, 128), (32, 64, 3, 4, 1, 2, 6, 500), (64, 128, 4, 4, 2, 2, 10, 256),
       (64, 128, 4, 4, 2, 2, 11, 250), (128, 128, 3, 4, 1, 2, 5, 480), (256, 512, 4, 4, 2, 2, 6, 241), (64, 128, 5, 3, 2, 1, 9, 125),
       (128, 128, 3, 3, 1, 1, 9, 64), (256, 256, 3, 3, 1, 1, 7, 32), (128, 128, 3, 3, 1, 1, 6, 50), (64, 64, 3, 3, 1, 1, 9, 128),
       (64, 64, 3, 3, 1, 1, 5, 64), (32, 32, 3, 3, 1, 1, 9, 128), (128, 256, 4, 4, 2, 2, 10, 128), (256, 256, 3, 4, 1, 2, 7, 64),
       (32, 64, 3, 4, 1, 2, 11, 128), (128, 64, 3, 3, 1, 1, 4, 500), (128, 64, 5, 3, 1, 1, 9, 125), (64, 32, 4, 4, 2, 2, 3, 256),
       (64, 128, 4, 4, 2, 2, 9, 60), (128, 128, 3, 3, 1, 1, 9, 8)]
# batch, cin, cout, h, w, kh, kw, sh, sw  (tests/test_gpu_conv2d_b3.py: SHAPES, STRIDED, STRIDED_FWD, NARROW)
C2B3 = [(2, 32, 32, 37, 128, 3, 3, 1, 1), (2, 32, 64, 21, 96, 3, 3, 1, 1), (2, 64, 64, 33, 62, 3, 3, 1, 1), (1, 64, 128, 19, 30, 3, 3, 1, 1),
        (2, 128, 128, 9, 257, 3, 3, 1, 1), (1, 128, 256, 15, 16, 3, 3, 1, 1), (1, 256, 256, 35, 31, 3, 3, 1, 1),
        (3, 64, 64, 150, 131, 3, 3, 1, 1), (1, 256, 256, 32, 8, 3, 3, 1, 1),
        (2, 32, 64, 21, 62, 3, 4, 1, 2), (2, 64, 128, 22, 62, 4, 4, 2, 2), (1, 128, 128, 17, 126, 3, 4, 1, 2), (1, 128, 256, 30, 30, 4, 4, 2, 2),
        (2, 256, 512, 10, 30, 4, 4, 2, 2), (1, 256, 256, 33, 30, 3, 4, 1, 2), (2, 64, 128, 61, 250, 4, 4, 2, 2),
        (1, 64, 128, 282, 512, 4, 4, 2, 2), (1, 32, 64, 9, 512, 3, 4, 1, 2), (1, 128, 128, 5, 384, 4, 4, 2, 2), (1, 64, 64, 7, 1000, 3, 4, 1, 2),
        (2, 32, 64, 21, 64, 3, 4, 1, 2), (2, 64, 128, 22, 64, 4, 4, 2, 2), (1, 128, 128, 17, 128, 3, 4, 1, 2), (1, 128, 256, 30, 64, 4, 4, 2, 2),
        (2, 256, 512, 12, 64, 4, 4, 2, 2), (1, 256, 256, 33, 32, 3, 4, 1, 2), (1, 32, 64, 9, 1024, 3, 4, 1, 2),
        (2, 128, 128, 40, 16, 3, 3, 1, 1), (2, 128, 256, 40, 16, 4, 4, 2, 2), (1, 256, 256, 50, 8, 3, 3, 1, 1), (1, 256, 256, 50, 8, 3, 4, 1, 2),
        (2, 64, 64, 33, 12, 3, 3, 1, 1), (1, 128, 128, 281, 4, 3, 3, 1, 1), (3, 64, 128, 37, 24, 4, 4, 2, 2)]
# Conv2d layers off the beaten track: channel counts without an MFMA tile (row-folded / gather forms), a patch-mode
# plan whose input patch fits no tile's LDS (the forward launcher refuses it), kernels larger than the padding allows
# the tight backward form, an epilogue Conv2d does not take, an impl value that does not exist
C2D_ODD = [_c2d(2, 3, 5, 20, 33, 3, 3, 1, 1, 1, 1), _c2d(2, 24, 40, 20, 33, 3, 3, 1, 1, 1, 1), _c2d(2, 16, 4, 20, 33, 3, 3, 1, 1, 1, 1),
           _c2d(2, 16, 8, 20, 33, 3, 3, 2, 2, 1, 1), _c2d(2, 48, 1, 20, 33, 1, 5, 1, 1, 0, 2), _c2d(2, 48, 3, 20, 33, 3, 5, 1, 2, 1, 2),
           _c2d(2, 7, 9, 20, 33, 4, 4, 2, 2, 1, 1), _c2d(1, 16, 32, 64, 64, 3, 3, 1, 1, 0, 0), _c2d(1, 32, 32, 12, 40, 5, 5, 1, 1, 1, 1),
           _c2d(1, 16, 16, 40, 600, 15, 15, 1, 1, 7, 7), _c2d(1, 16, 64, 40, 4000, 9, 41, 1, 8, 4, 20), _c2d(1, 32, 32, 30, 3000, 31, 31, 1, 1, 15, 15),
           _c2d(1, 32, 32, 20, 33, 3, 3, 1, 1, 1, 1, RESIDUAL), _c2d(1, 32, 32, 20, 33, 3, 3, 1, 1, 1, 1, LEAKY_PRE)]
# 1-D layers without an MFMA tile / ring geometry, odd kernels, grouped layers, refused descriptors
C1D_ODD = [_conv(CAUSAL, 2, 3, 5, 100, 3), _conv(CAUSAL, 2, 24, 40, 100, 5, 2), _conv(CAUSAL, 2, 16, 16, 100, 7), _conv(CAUSAL, 2, 48, 24, 333, 7, 1, 3),
           _conv(CAUSAL, 2, 64, 64, 3, 7), _conv(CAUSAL, 2, 64, 128, 1000, 6, 2), _conv(UPSAMPLE, 2, 128, 64, 77, 7, 3), _conv(UPSAMPLE, 2, 20, 10, 77, 5, 2),
           _conv(TRANSPOSED, 2, 128, 64, 77, 8, 4), _conv(TRANSPOSED, 2, 128, 64, 77, 3, 4), _conv(SAME, 2, 64, 64, 501, 11), _conv(SAME, 2, 64, 64, 501, 5, 1, 2),
           _conv(PADDED, 2, 64, 64, 501, 3, 1, 1, 0, 1, 1), _conv(PADDED, 2, 64, 64, 501, 3, 1, 1, 0, 64, 1), _conv(PADDED, 2, 64, 96, 501, 9, 2, 1, LEAKY_PRE, 4, 4),
           _conv(CAUSAL, 1, 512, 512, 1 << 22, 3), _conv(CAUSAL, 1, 32, 32, 1 << 24, 7), _conv(7, 2, 64, 64, 100, 3), _conv(CAUSAL, 2, 0, 64, 100, 3)]
RES_ODD = [_conv(CAUSAL, 2, 48, 48, 500, 7, 1, 3), _conv(CAUSAL, 2, 16, 16, 500, 7), _conv(CAUSAL, 2, 64, 64, 500, 5, 1, 3), _conv(CAUSAL, 2, 64, 64, 500, 7, 1, 27),
           _conv(CAUSAL, 2, 1024, 1024, 500, 7), _conv(CAUSAL, 2, 128, 128, 5, 7, 1, 9), _conv(CAUSAL, 1, 64, 64, 1 << 24, 7), _conv(CAUSAL, 2, 64, 32, 500, 7),
           _conv(CAUSAL, 2, 64, 64, 500, 7, 2), _conv(SAME, 2, 64, 64, 500, 7)]


def cases():
    """[(op, descriptor fields incl. impl, conv_impl, rb_impl)] -- a fixed order, each case once."""
    lib = _lib.load()
    conv, res, c2d = [], [], []   # (fields, impls) in first-seen order

    def add(layers, impls=IMPLS):
        for op, f in layers:
            (conv if op == "conv" else res).append((f, impls))

    for b in (32, 1):
        for clip in (72000, 3200, 72001, 71999):          # full size / 10 frames: under one tile / ragged
            add(generator_layers(lib, b, 1, clip, (False,) * 4), IMPLS if clip == 72000 else (AUTO, BF16X3))
        for clip in (144000, 4800, 143999):
            add(generator_layers(lib, b, 2, clip, (False, True, False, False)), IMPLS if clip == 144000 else (AUTO, BF16X3))
        for frames in (225, 10, 226):
            add(attention_layers(b, frames))
        for clip in (72000, 71999):
            add(waveform_disc_layers(lib, b, clip), (AUTO, DIRECT) if clip == 72000 else (AUTO,))
        for win in (2048, 1024, 512, 256, 128):
            c2d += [(f, IMPLS) for f in stft_disc_layers(lib, b, 72000, win)]
            c2d += [(f, (AUTO, BF16X3)) for f in stft_disc_layers(lib, b, 71999, win)]
    # every epilogue bit (and the combinations the models use) on every distinct full-size generator layer
    distinct = list(dict.fromkeys(f for op, f in generator_layers(lib, 32, 1, 72000, (False,) * 4) +
                                  generator_layers(lib, 32, 2, 144000, (False, True, False, False)) if op == "conv"))
    for f in distinct + [l[1] for l in attention_layers(32, 225)]:
        for epi in (0, LEAKY_PRE, RESIDUAL, LEAKY_POST, GELU_PRE, MASK, RESIDUAL | LEAKY_POST, LEAKY_PRE | RESIDUAL, 31):
            conv.append((f[:8] + (epi,) + f[9:], (AUTO, BF16X3)))
    conv += [(f, IMPLS + (9,)) for f in C1D_ODD]
    res += [(f, IMPLS + (9,)) for f in RES_ODD]
    for cin, cout, kh, kw, sh, sw, h, w in P2D:
        for b in (3, 2):
            for epi in (0, LEAKY_PRE):
                c2d.append((_c2d(b, cin, cout, h, w, kh, kw, sh, sw, (kh - 1) // 2, 1, epi), (AUTO, MFMA, BF16X3)))
    for b, cin, cout, h, w, kh, kw, sh, sw in C2B3:
        for epi in (0, LEAKY_PRE):
            c2d.append((_c2d(b, cin, cout, h, w, kh, kw, sh, sw, (kh - 1) // 2, (kw - 1) // 2, epi), (AUTO, MFMA, BF16X3)))
    c2d += [(f, IMPLS + (9,)) for f in C2D_ODD]

    out, seen = [], set()

    def emit(op, f, impl, ci, rb):
        case = (op, f + (impl,), ci, rb)
        if case not in seen:
            seen.add(case)
            out.append(case)

    for f, impls in conv:
        for impl in impls:
            for ci in (1, 0):
                emit("conv", f, impl, ci, 1)
    for f, impls in res:
        for impl in impls:
            for ci in (1, 0):
                for rb in (1, 0):
                    emit("resblock", f, impl, ci, rb)
    for f, impls in c2d:
        for impl in impls:
            for ci in (1, 0):
                emit("conv2d", f, impl, ci, 1)
                emit("conv2d_bwd", f, impl, ci, 1)
    return out


def key(case):
    op, f, ci, rb = case
    return f"{op} {','.join(map(str, f))} conv_impl={ci} rb_impl={rb}"


def query(lib, case):
    """The name, or the (negative) return code."""
    op, f, ci, rb = case
    lib.agx_set_tuning(b"conv_impl", ci)
    lib.agx_set_tuning(b"rb_impl", rb)
    if op in ("conv", "resblock"):
        d = _lib.ConvDesc(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], 0.1, f[11], f[9], f[10])
    else:
        d = _lib.Conv2dDesc(*f[:12], 0.2, f[12])
    buf = ctypes.create_string_buffer(96)
    try:
        rc = getattr(lib, QUERY[op])(ctypes.byref(d), buf, len(buf))
    finally:
        lib.agx_set_tuning(b"conv_impl", 1)
        lib.agx_set_tuning(b"rb_impl", 1)
    return buf.value.decode() if rc == 0 else int(rc)


def _grid_hash(grid):
    return hashlib.sha256("\n".join(key(c) for c in grid).encode()).hexdigest()[:16]


def test_kernel_names_match_the_recording():
    lib = _lib.load()
    fixture = json.load(open(FIXTURE))
    names, values, refused = fixture["names"], fixture["values"], fixture["refused_since"]
    grid = cases()
    assert len(grid) == len(values) and len(grid) > 5000, (len(grid), len(values))
    assert _grid_hash(grid) == fixture["grid_sha256"], "cases() is no longer the grid the recording was made on"
    wrong = []
    for case, want in zip(grid, values):
        want = want if want < 0 else names[want]
        if key(case) in refused:        # the launcher refused it on the recording commit; the query now says so
            assert refused[key(case)][0] == want
            want = refused[key(case)][1]
        got = query(lib, case)
        if got != want:
            wrong.append((key(case), want, got))
    assert not wrong, f"{len(wrong)} of {len(grid)} kernel names differ from the recording, e.g. {wrong[:5]}"
    # the grid reaches every family the selectors can name
    for family in ("conv_p<", "conv_b3<", "conv_mfma<", "conv_direct<", "conv_narrow<", "conv_fewrows<", "conv_p2d<", "conv2d_b3<",
                   "conv2d_fewout<", "conv2d_bwd_data_gather", "resblock_p<", "resblock_b3<", "resblock_mfma<", "2x:conv_mfma<", "2x:conv_direct<",
                   ":bf16x3"):
        assert any(family in n for n in names), family


def test_a_refused_descriptor_reports_the_launchers_error():
    """A patch-mode Conv2d plan no MFMA tile fits, and an impl value that does not exist: agx_conv2d_forward /
    agx_conv_forward refuse them (before any pointer is touched beyond the NULL check), and the name query says the same."""
    lib = _lib.load()
    refused = [k for k, v in json.load(open(FIXTURE))["refused_since"].items()]
    assert refused
    d = _lib.Conv2dDesc(1, 16, 64, 40, 4000, 9, 41, 1, 8, 4, 20, 0, 0.2, AUTO)
    buf = ctypes.create_string_buffer(96)
    assert lib.agx_conv2d_kernel_name(ctypes.byref(d), buf, len(buf)) == -5
    assert b"no MFMA tile fits" in lib.agx_last_error()
    d1 = _lib.ConvDesc(CAUSAL, 2, 64, 64, 100, 3, 1, 1, 0, 0.1, 9, 1, 0)
    assert lib.agx_conv_kernel_name(ctypes.byref(d1), buf, len(buf)) == -1
    assert b"unknown impl 9" in lib.agx_last_error()


def record(commit):
    lib = _lib.load()
    grid, names, values = cases(), [], []
    for case in grid:
        got = query(lib, case)
        if not isinstance(got, int):
            if got not in names:
                names.append(got)
            got = names.index(got)
        values.append(got)
    blob = {"recorded_on": commit,
            "format": "values[i] answers cases()[i] of tests/test_kernel_names_cpu.py: an index into names, or the negative return "
                      "code.  refused_since[key] = [answer on the recording commit, answer now]: descriptors whose launcher "
                      "refused them on that commit while the name query printed a name",
            "grid_sha256": _grid_hash(grid), "names": names, "refused_since": {}, "values": values}
    with open(FIXTURE, "w") as fh:
        json.dump(blob, fh, separators=(",", ":"))
    print(len(values), "entries,", len(names), "names,", os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    record(sys.argv[1])
