"""Wavelet decoder blocks in a codec stream, without a GPU: the float64 restatement (tests/wavelet_stream_ref.py)
against the oracle's plain calls, what its mask, tail rule and selects are needed for, the plan of the reference default
architecture, and every refusal of the new entry points."""
import ctypes
import math
import os

import pytest
import torch

from audio_generation_amd import _lib, ops, streaming
from audio_generation_amd._lib import AgxError
from audio_generation_amd.vae import CausalVQAE
from oracle import codec, wavelets
from tests import wavelet_stream_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEDULES = {9: ([9], [1] * 9, [2, 1, 3, 1, 2], [4, 5]), 1: ([1],)}
SPECS = (((2, 3), (True, False)), ((2, 3), (False, True)), ((2, 4, 5), (False, True, False)))
REL = 1e-10


def _spec(strides, wav):
    return codec.CodecSpec(in_channels=1, n_blocks=len(strides), strides=strides, first_block_channels=4, codebook_dim=8,
                           wavelet_decoders=list(wav), input_format="n c l")


_CASES = {}


def _case(strides, wav, t):
    """Shared per (spec, T): float64 state dict, latents and the oracle's plain decode (computed once, never modified)."""
    key = (strides, wav, t)
    if key not in _CASES:
        spec = _spec(strides, wav)
        sd = {k: v.double() for k, v in codec.init_state_dict(spec, seed=5).items()}
        for k in sd:                                     # per-channel wavelet scales that differ, so that a channel mix-up shows
            if k.endswith("wavelet_scale"):
                sd[k] = sd[k] * torch.linspace(0.5, 1.5, sd[k].numel(), dtype=torch.float64).reshape(sd[k].shape)
        zq = torch.randn(2, spec.codebook_dim, t, generator=torch.Generator().manual_seed(17), dtype=torch.float64)
        y_plain = codec.decode_latents(zq.transpose(1, 2).contiguous(), sd, spec)
        _CASES[key] = spec, sd, zq, y_plain
    return _CASES[key]


def _stream_decode(spec, sd, zq, schedule, **switches):
    s = ref.StackStream(ref.stack_units(sd, spec), 1, zq.shape[0], max(schedule), **switches)
    at, out = 0, []
    for n in schedule:
        out.append(s.run(zq[:, :, at:at + n]))
        at += n
    s.finish()
    left = math.ceil(s.delay_out / spec.scale_factor)
    while left > 0:
        n = min(left, max(schedule))
        out.append(s.run(torch.zeros(zq.shape[0], zq.shape[1], n, dtype=torch.float64)))
        left -= n
    return torch.cat(out, dim=2), s.delay_out


@pytest.mark.parametrize("t", (9, 1))
@pytest.mark.parametrize("strides,wav", SPECS)
def test_restatement_equals_the_oracle_plain_decode(strides, wav, t):
    spec, sd, zq, y_plain = _case(strides, wav, t)
    n_out = t * spec.scale_factor
    for schedule in SCHEDULES[t]:
        y, delay = _stream_decode(spec, sd, zq, schedule)
        err = float((y[:, :, delay:delay + n_out] - y_plain).abs().max()) / float(y_plain.abs().max())
        print(f"strides {strides} wavelet {wav} T {t} schedule {schedule}: relative {err:.3e}, delay {delay}")
        assert err < REL
        assert float(y[:, :, :delay].abs().max()) == 0.0
        assert float(y[:, :, delay + n_out:].abs().max()) == 0.0


# --------------------------------------------------------------------------------------------- a stand-alone unit
UNITS = ((3, 7, 3, 4, 1, 0), (4, 9, 3, 4, 5, 5), (5, 11, 3, 2, 2, 2), (2, 5, 5, 4, 3, 3))      # (s, k_in, k_out, ratio, r, D)
C_IN, HIDDEN, C_OUT = 3, 5, 2


def _unit_params(s, k_in, k_out, ratio, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    sd = {"conv_in.weight": torch.randn(HIDDEN, C_IN, k_in, generator=g, dtype=torch.float64) / (C_IN * k_in) ** 0.5,
          "conv_in.bias": torch.randn(HIDDEN, generator=g, dtype=torch.float64),
          "conv_out.weight": torch.randn(C_OUT, HIDDEN, k_out, generator=g, dtype=torch.float64) / (HIDDEN * k_out) ** 0.5,
          "conv_out.bias": torch.randn(C_OUT, generator=g, dtype=torch.float64),
          "space": torch.linspace(-10, 10, ratio * s, dtype=torch.float64).reshape(1, 1, 1, -1),
          "wavelet_scale": (20.0 + 10.0 * torch.arange(HIDDEN, dtype=torch.float64)).reshape(1, HIDDEN, 1, 1)}
    table = ref.fold_table64(sd["space"], sd["wavelet_scale"], HIDDEN, s)
    unit = ref.WaveletUnit(sd["conv_in.weight"], sd["conv_in.bias"], sd["conv_out.weight"], sd["conv_out.bias"], table, s)
    return sd, unit


def _run_unit(unit, x, r, d, schedule, plant=False, extra=0, **switches):
    """A wavelet unit alone: ``x`` (B, c_in, L) is the signal at the unit's input, L = T r, fed in frames at delay ``d`` (the chunk of
    a step holds the columns [pos r - d, (pos + n) r - d), exact 0 outside [0, L)), then finish and flush.  ``plant``: NaN into the
    column L of the ring of h -- the one l0 + 1 behind ph == 0 that nothing else reads -- before every out-step that holds it.
    Returns (raw output from column -D_out, D_out)."""
    b, _, length = x.shape
    t = length // r
    mc = max(schedule)
    tail = switches.pop("tail", True)
    ring = torch.zeros(b, unit.c_in, unit.reach + mc * r + extra, dtype=torch.float64)
    hring = torch.zeros(b, unit.hidden, unit.reach_h + mc * r + extra, dtype=torch.float64)
    d_h, (rate_out, d_out) = unit.delay_h(d), unit.rates(r, d)
    pos, end, out = [0] * b, [ref.LIVE] * b, []
    steps = list(schedule) + [None]
    left = math.ceil(d_out / rate_out) + 1
    while left > 0:
        steps.append(min(left, mc))
        left -= steps[-1]
    planted = 0
    for n in steps:
        if n is None:
            end = list(pos)
            continue
        j = torch.arange(pos[0] * r - d, (pos[0] + n) * r - d, dtype=torch.int64)
        ok = (j >= 0) & (j < length)
        chunk = torch.where(ok, x[:, :, j.clamp(0, length - 1)], torch.zeros((), dtype=torch.float64))
        ring[:, :, torch.remainder(j, ring.shape[2])] = chunk
        ref.in_step(unit, ring, hring, pos, end, n, r, d, **switches)
        nxt = (pos[0] + n) * r - d_h                                  # the first column of h not produced yet
        if plant and end[0] != ref.LIVE and nxt - hring.shape[2] <= length < nxt:
            hring[:, :, length % hring.shape[2]] = float("nan")
            planted += 1
        dst = torch.zeros(b, unit.c_out, n * rate_out, dtype=torch.float64)
        blk, _ = ref.out_step(unit, hring, dst, pos, end, n, r, d_h, dst_ring=False, tail=tail, **switches)
        out.append(blk)
        pos = [p + n for p in pos]
    assert sum(schedule) == t and (not plant or planted > 0)
    return torch.cat(out, dim=2), d_out


@pytest.mark.parametrize("s,k_in,k_out,ratio,r,d", UNITS)
def test_a_unit_alone_equals_the_oracle_wavelet_layer(s, k_in, k_out, ratio, r, d):
    sd, unit = _unit_params(s, k_in, k_out, ratio)
    assert unit.rates(r, d) == (r * s, (d + (k_in - 1) // 2) * s + s + (k_out - 1) // 2)
    for t in (1, 2, 5):
        x = torch.randn(2, C_IN, t * r, generator=torch.Generator().manual_seed(t), dtype=torch.float64)
        want = wavelets.wavelet_layer(x, sd, "", s)
        assert want.shape[2] == t * r * s
        for schedule in ([t], [1] * t, [2, 1, 2][:3] if t == 5 else [t]):
            y, d_out = _run_unit(unit, x, r, d, schedule)
            err = float((y[:, :, d_out:d_out + t * r * s] - want).abs().max()) / float(want.abs().max())
            print(f"unit {(s, k_in, k_out, ratio, r, d)} L {t * r} schedule {schedule}: relative {err:.3e}")
            assert err < REL
            assert float(y[:, :, :d_out].abs().max()) == 0.0 and float(y[:, :, d_out + t * r * s:].abs().max()) == 0.0


# --------------------------------------------------------------------------------------------- mask, tail and select
@pytest.mark.parametrize("off", ["tail", "mask_end", "mask_start"])
def test_restatement_without_the_tail_rule_or_a_mask_differs(off):
    spec, sd, zq, y_plain = _case((2, 3), (False, True), 9)
    y, delay = _stream_decode(spec, sd, zq, [2, 1, 3, 1, 2], **{off: False})
    err = float((y[:, :, delay:delay + 9 * spec.scale_factor] - y_plain).abs().max()) / float(y_plain.abs().max())
    print(f"without {off}: relative {err:.3e}")
    assert err > 1e-6
    s, k_in, k_out, ratio, r, d = UNITS[1]
    sdu, unit = _unit_params(s, k_in, k_out, ratio)
    x = torch.randn(2, C_IN, 2 * r, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    want = wavelets.wavelet_layer(x, sdu, "", s)
    y, d_out = _run_unit(unit, x, r, d, [1, 1], **{off: False})
    whole = torch.zeros_like(y)
    whole[:, :, d_out:d_out + want.shape[2]] = want
    assert float((y - whole).abs().max()) > 1e-6 * float(want.abs().max())


@pytest.mark.parametrize("s,k_in,k_out,ratio,r,d", UNITS)
def test_nan_behind_phase_zero_changes_nothing(s, k_in, k_out, ratio, r, d):
    """Column L of h is l0 + 1 of the window v = (L - 1) s, whose phase is 0, and of no other: a select never reads it."""
    sd, unit = _unit_params(s, k_in, k_out, ratio)
    x = torch.randn(2, C_IN, 2 * r, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    clean, _ = _run_unit(unit, x, r, d, [1, 1])
    dirty, _ = _run_unit(unit, x, r, d, [1, 1], plant=True)
    assert torch.equal(clean, dirty)


# --------------------------------------------------------------------------------------------- the plan
def test_plan_of_the_reference_default_architecture():
    with torch.device("meta"):
        model = CausalVQAE().eval()
    with pytest.raises(NotImplementedError, match="wavelet"):
        streaming.plan(model, 4)
    p = streaming.plan(model, 4, wavelet_blocks=True)
    heads = [u for u in p.decoders if u.kind in ("up", "wavelet")]
    assert [u.kind for u in heads] == ["up", "wavelet", "up", "up", "up"]
    assert [(u.rate_in, u.delay_in) for u in heads] == [(1, 0), (5, 5), (20, 41), (80, 168), (240, 507)]
    assert [(u.rate_out, u.delay_out) for u in heads] == [(5, 5), (20, 41), (80, 168), (240, 507), (480, 1016)]
    assert p.decoder_delay == 1016 and p.flush_frames == 3 and p.scale_factor == 480
    w = heads[1]
    assert (w.k, w.s, w.k_out, w.delay_h, w.reach, w.cap, w.reach_h, w.cap_h) == (9, 4, 3, 9, 8, 8 + 4 * 5, 2, 2 + 4 * 5)
    assert all(u.hidden == 0 and u.cap_h == 0 for u in p.decoders if u.kind != "wavelet")
    s = model.new_stream(2, max_chunk=4, device="meta", wavelet_blocks=True)
    assert len(s.dec_rings) == len(p.decoders) == len(s.dec_hidden)
    assert [h is not None for h in s.dec_hidden] == [u.kind == "wavelet" for u in p.decoders]
    assert tuple(s.dec_hidden[p.decoders.index(w)].shape) == (2, w.hidden, w.cap_h) and s.decoder_delay == 1016


def _model(wav, strides=(2, 3)):
    return CausalVQAE(in_channels=1, n_blocks=len(strides), strides=strides, first_block_channels=4, codebook_dim=8, num_quantizers=2,
                      codebook_size=16, wavelet_decoders=wav, input_format="n c l").eval()


@pytest.mark.parametrize("strides,wav", SPECS)
def test_package_plan_equals_the_restatements(strides, wav):
    model = _model(wav, strides)
    spec = _spec(strides, wav)
    sd = {k: v.double() for k, v in codec.init_state_dict(spec, seed=5).items()}
    p = streaming.plan(model, 3, wavelet_blocks=True)
    s = ref.StackStream(ref.stack_units(sd, spec), 1, 1, 3)
    assert [(u.rate_in, u.delay_in, u.reach, u.cap) for u in p.decoders] == s.plan
    assert (p.decoders[-1].rate_out, p.decoders[-1].delay_out) == (s.rate_out, s.delay_out)
    assert [u.cap_h if u.kind == "wavelet" else None for u in p.decoders] == [None if h is None else h.shape[2] for h in s.hidden]


# --------------------------------------------------------------------------------------------- the surface
def test_without_the_keyword_nothing_changes():
    model = _model((True, False))
    with pytest.raises(NotImplementedError, match="wavelet"):
        model.new_stream(1)
    with pytest.raises(NotImplementedError, match="wavelet"):
        model.new_stream(1, wavelet_blocks=False)
    plain = _model(False)
    assert streaming.plan(plain, 3) == streaming.plan(plain, 3, wavelet_blocks=True)
    s = plain.new_stream(1)
    assert s.dec_hidden == [None] * len(s.dec_rings)
    s = model.new_stream(2, max_chunk=3, wavelet_blocks=True)
    hid = [h for h in s.dec_hidden if h is not None]
    assert len(hid) == 1 and float(hid[0].abs().max()) == 0.0
    hid[0].fill_(1.0)
    s.reset(rows=[1])
    assert float(hid[0][1].abs().max()) == 0.0 and float(hid[0][0].min()) == 1.0
    with torch.no_grad(), pytest.raises(AgxError, match="MI355X only"):       # a valid call: no CPU fallback
        model.decode_stream(torch.zeros(2, 8, 2), s)


def test_other_unit_kinds_stay_refused_with_the_keyword():
    args = dict(in_channels=1, n_blocks=2, strides=(2, 3), first_block_channels=4, codebook_dim=8, num_quantizers=2, codebook_size=16,
                input_format="n c l")
    with pytest.raises(NotImplementedError, match="multires"):
        CausalVQAE(wavelet_decoders=(True, False), multires_decoders=True, **args).eval().new_stream(1, wavelet_blocks=True)
    with pytest.raises(NotImplementedError, match="depthwise"):
        CausalVQAE(wavelet_decoders=(True, False), depthwise=True, **args).eval().new_stream(1, wavelet_blocks=True)


def test_wrapper_refusals_precede_every_launch():
    """On the CPU nothing can be launched: a call that got past the shape checks raises the 'MI355X only' error instead."""
    f = torch.zeros
    pos, end = f(2, dtype=torch.int64), torch.full((2,), ops.STREAM_LIVE, dtype=torch.int64)
    img_in, img_out, table = f(16 * 7 * 24), f(32 * 3 * 16), f(24, 8)
    src, h, dst = f(2, 6, 6 + 4), f(2, 24, 2 + 4), f(2, 3, 12)
    ok_in = dict(c_in=6, hidden=24, kernel=7, packed=img_in, bias=None, src=src, dst=h, pos=pos, end=end, n=4, rate_in=1, delay_in=0)
    for change, match in ((dict(kernel=6), "odd kernel"), (dict(n=0), "n >= 1"), (dict(src=f(2, 6, 9)), "alias its history"),
                          (dict(src=f(2, 5, 10)), "6 channels"), (dict(dst=f(2, 24, 3)), "new columns of a ring"),
                          (dict(dst=f(2, 23, 6)), "c_out=24"), (dict(end=None), "end is needed"), (dict(rate_in=0), "rate_in"),
                          (dict(src=src.double()), "contiguous float32"), (dict(delay_in=-1), "delay_in"), ({}, "MI355X only")):
        with pytest.raises(AgxError, match=match):
            ops.wavelet_stream_in_step(**{**ok_in, **change})
    ok_out = dict(hidden=24, c_out=3, kernel=3, scale=3, packed=img_out, bias=None, table=table, h=h, dst=dst, pos=pos, end=end, n=4,
                  rate_h=1, delay_h=3, dst_ring=False)
    for change, match in ((dict(kernel=4), "odd kernel"), (dict(scale=1), "scale = 1 < 2"), (dict(table=f(24, 9)), "table"),
                          (dict(table=f(23, 8)), "table"), (dict(h=f(2, 24, 5)), "alias its history"), (dict(dst=f(2, 3, 11)), "plain columns"),
                          (dict(dst=f(2, 3, 11), dst_ring=True), "new columns of a ring"), (dict(epilogue=_lib.EPI_RESIDUAL), "epilogue"),
                          (dict(end=None), "end is needed"), (dict(n=0), "n >= 1"), (dict(rate_h=0), "rate_h"), ({}, "MI355X only")):
        with pytest.raises(AgxError, match=match):
            ops.wavelet_stream_out_step(**{**ok_out, **change})
    space, sigma = torch.linspace(-10, 10, 24), torch.full((24,), 40.0)
    for args, match in (((space, sigma, 24, 5), "divide"), ((space, sigma, 24, 1), ">= 2"), ((space, sigma[:7], 24, 3), "entries"),
                        ((space, sigma, 24, 3), "MI355X only"), ((space, sigma[:1], 24, 3), "MI355X only")):
        with pytest.raises(AgxError, match=match):
            ops.wavelet_fold_table(*args)


@pytest.fixture(scope="module")
def lib():
    from audio_generation_amd import build
    build.build()
    return _lib.load()


SYMBOLS = ("agx_wavelet_fold_table", "agx_wavelet_stream_in_step", "agx_wavelet_stream_in_step_counted", "agx_wavelet_stream_out_step",
           "agx_wavelet_stream_out_step_counted", "agx_wavelet_stream_in_kernel_name", "agx_wavelet_stream_out_kernel_name")
BAD_SHAPE, NULL_POINTER, UNSUPPORTED = -1, -2, -5


def test_new_symbols_are_declared_bound_and_exported(lib):
    assert lib.agx_version() == 122
    header = open(os.path.join(ROOT, "include", "agx.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    for name in ("agx_wavelet_stream_in_step", "agx_wavelet_stream_out_step"):
        assert len(_lib.SIGNATURES[name + "_counted"][1]) == len(_lib.SIGNATURES[name][1]) + 1


def test_kernel_names_keep_the_split_whatever_the_step(lib):
    for c_in, hidden, k, rate in ((512, 1024, 9, 5), (16, 32, 7, 1), (6, 24, 9, 5), (40, 80, 5, 3)):
        names = [ops.wavelet_stream_in_kernel_name(c_in, hidden, k, n, rate) for n in (1, 2, 4, 16)]
        assert all(nm.startswith("conv_stream<") for nm in names) and len({nm.split(",")[0] for nm in names}) == 1, names
    for hidden, c_out, k, s, rate in ((1024, 256, 3, 4, 5), (32, 8, 3, 3, 1), (80, 20, 3, 2, 3), (20, 10, 5, 5, 2)):
        names = [ops.wavelet_stream_out_kernel_name(hidden, c_out, k, s, n, rate) for n in (1, 2, 4, 16)]
        assert all(nm.startswith("wavelet_stream_out<") for nm in names) and len({nm.split(",")[0] for nm in names}) == 1, names
    assert ops.wavelet_stream_in_kernel_name(8, 8, 3, 0, 1) == "none" and ops.wavelet_stream_out_kernel_name(8, 8, 3, 2, 0, 1) == "none"
    for bad in ((8, 8, 4, 1, 1),):
        with pytest.raises(AgxError, match="odd kernel"):
            ops.wavelet_stream_in_kernel_name(*bad)
    for bad in ((8, 8, 4, 2, 1, 1), (8, 8, 3, 1, 1, 1)):
        with pytest.raises(AgxError):
            ops.wavelet_stream_out_kernel_name(*bad)
    # the public conv entry points keep refusing the kind
    with pytest.raises(AgxError):
        ops.conv_stream_kernel_name(_lib.CONV_SAME, 8, 8, 3, 1, 1, 1, 1)


def test_library_refusals_precede_every_use_of_a_pointer(lib):
    one = ctypes.c_void_p(64)                                       # never dereferenced
    tbl = ctypes.c_void_p(128)
    dst = ctypes.c_void_p(256)
    assert lib.agx_wavelet_fold_table(one, one, 1, dst, 8, 24, 1, None) == BAD_SHAPE          # s < 2
    assert lib.agx_wavelet_fold_table(one, one, 1, dst, 8, 25, 3, None) == BAD_SHAPE          # s does not divide P
    assert lib.agx_wavelet_fold_table(one, one, 3, dst, 8, 24, 3, None) == BAD_SHAPE          # sigma_len
    assert lib.agx_wavelet_fold_table(one, None, 1, dst, 8, 24, 3, None) == NULL_POINTER
    assert lib.agx_wavelet_fold_table(one, one, 1, None, 8, 24, 3, None) == NULL_POINTER

    def in_step(kernel=7, src=one, src_cap=10, dst_=dst, dst_cap=6, pos=one, end=one, packed=one, n=4, batch=2):
        return lib.agx_wavelet_stream_in_step(6, 24, kernel, packed, None, src, src_cap, dst_, dst_cap, pos, end, batch, n, 1, 0, None)

    assert in_step(kernel=6) == UNSUPPORTED and "odd kernel" in lib.agx_last_error().decode()
    assert in_step(src_cap=9) == BAD_SHAPE and in_step(dst_cap=3) == BAD_SHAPE and in_step(dst_cap=0) == BAD_SHAPE
    assert in_step(end=None) == NULL_POINTER and in_step(pos=None) == NULL_POINTER and in_step(packed=None) == NULL_POINTER
    assert in_step(src=dst) == BAD_SHAPE and "one of the sources" in lib.agx_last_error().decode()
    assert in_step(n=0) == 0 and in_step(batch=0) == 0
    assert lib.agx_wavelet_stream_in_step_counted(6, 24, 7, one, None, one, 10, dst, 6, one, one, None, 2, 4, 1, 0, None) == NULL_POINTER
    assert "NULL counts" in lib.agx_last_error().decode()

    def out_step(kernel=3, scale=3, h=one, h_cap=6, table=tbl, dst_=dst, dst_cap=0, end=one, n=4, epi=0, counted=False):
        if counted:
            return lib.agx_wavelet_stream_out_step_counted(24, 3, kernel, scale, epi, 0.1, one, None, table, h, h_cap, dst_, dst_cap, one,
                                                           end, None, 2, n, 1, 3, None)
        return lib.agx_wavelet_stream_out_step(24, 3, kernel, scale, epi, 0.1, one, None, table, h, h_cap, dst_, dst_cap, one, end, 2, n, 1,
                                               3, None)

    assert out_step(scale=1) == BAD_SHAPE and out_step(kernel=4) == UNSUPPORTED
    assert out_step(h_cap=5) == BAD_SHAPE and "alias its history" in lib.agx_last_error().decode()
    assert out_step(dst_cap=11) == BAD_SHAPE and out_step(epi=_lib.EPI_RESIDUAL) == UNSUPPORTED
    assert out_step(end=None) == NULL_POINTER and out_step(table=None) == NULL_POINTER and out_step(h=None) == NULL_POINTER
    assert out_step(dst_=one) == BAD_SHAPE and out_step(dst_=tbl) == BAD_SHAPE
    assert out_step(n=0) == 0
    assert out_step(counted=True) == NULL_POINTER and "NULL counts" in lib.agx_last_error().decode()
