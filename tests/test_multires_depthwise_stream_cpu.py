"""Multires layers and depthwise residual blocks in a codec stream, without a GPU: the float64 restatement
(tests/multires_stream_ref.py) against the oracle's plain calls, what the depthwise operand's select is needed for, the plans of
the three architectures of the issue, and the surface: keywords, symbols, refusals."""
import ctypes
import os

import pytest
import torch

from audio_generation_amd import _lib, longform, ops, streaming
from audio_generation_amd._lib import CONV_CAUSAL, CONV_TRANSPOSED, EPI_LEAKY_PRE, AgxError
from audio_generation_amd.vae import CausalVQAE
from oracle import codec, wavelets
from tests import codec_stream_ref as cref
from tests import multires_stream_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEDULES = ([6], [1] * 6, [2, 1, 3])
REL = 1e-12
F64 = torch.float64


def _multires_params(c, k, depth, seed=0):
    g = torch.Generator().manual_seed(40 + seed)
    return (torch.randn(c, 1, k, generator=g, dtype=F64) / k, torch.randn(c, 1, k, generator=g, dtype=F64) / k,
            torch.randn(c, depth + 2, generator=g, dtype=F64))


# --------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("c,k,depth,rate,delay", [(6, 2, 3, 1, 0), (5, 3, 4, 6, 6), (3, 4, 1, 4, 0), (2, 1, 2, 2, 2), (2, 3, 0, 1, 0)])
def test_multires_restatement_equals_the_oracle_on_the_whole_clip(c, k, depth, rate, delay):
    h0, h1, w = _multires_params(c, k, depth)
    x = torch.randn(2, c, 6 * rate, generator=torch.Generator().manual_seed(1), dtype=F64)
    want = wavelets.multires_conv(x, h0, h1, w, depth)
    hh = ref.reach(k, depth)
    for schedule in SCHEDULES:
        sched = list(schedule) + [1] * (-(-delay // rate) + 1 if delay else 0)      # bring a delayed tail out, and one frame past the end
        y = ref.stream_clip(lambda ring, dst, pos, n: ref.multires_step(h0, h1, w, depth, ring, dst, pos, [6] * 2, n, rate, delay,
                                                                        dst_ring=False),
                            x, c, hh, sched, rate, delay)
        err = float((y[:, :, delay:delay + 6 * rate] - want).abs().max()) / float(want.abs().max())
        print(f"multires C={c} K={k} depth={depth} rate={rate} delay={delay} schedule {schedule}: relative {err:.3e}")
        assert err < REL
        if delay:                                   # exact 0 before the start and after the end
            assert float(y[:, :, :delay].abs().max()) == 0.0 and float(y[:, :, delay + 6 * rate:].abs().max()) == 0.0


def _resdw_sd(c, k, seed=0):
    """A depthwise residual block in the oracle's state-dict layout, float64; the per-channel conv's bias of magnitude 0.5 .. 1."""
    g = torch.Generator().manual_seed(60 + seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)      # noqa: E731
    sign = torch.where(r(c) > 0, 1.0, -1.0).double()
    return {"conv1.0.conv.weight": 1.0 + 0.5 * r(c, 1, 1), "conv1.0.conv.bias": sign * (0.5 + 0.5 * torch.rand(c, generator=g, dtype=F64)),
            "conv1.1.conv.weight": r(c, c, k) / (c * k) ** 0.5, "conv1.1.conv.bias": r(c),
            "conv2.conv.weight": r(c, c, 1) / c ** 0.5, "conv2.conv.bias": r(c)}


def _resdw_ops(sd, d):
    op1 = cref.Op("causal", sd["conv1.1.conv.weight"], sd["conv1.1.conv.bias"], d=d, pre=cref.SLOPE)
    op2 = cref.Op("causal", sd["conv2.conv.weight"], sd["conv2.conv.bias"], residual=True)
    return op1, op2, sd["conv1.0.conv.weight"].reshape(-1), sd["conv1.0.conv.bias"]


def _stream_resdw(sd, x, d, schedule, rate, delay, select=True, frames=6):
    op1, op2, scale, shift = _resdw_ops(sd, d)
    sched = list(schedule) + [1] * -(-delay // rate)
    return ref.stream_clip(lambda ring, dst, pos, n: ref.resdw_unit_step(op1, op2, scale, shift, ring, dst, pos, [frames] * x.shape[0], n,
                                                                         rate, delay, dst_ring=False, select=select)[0],
                           x, op2.c_out, op1.d * (op1.k - 1), sched, rate, delay)


@pytest.mark.parametrize("c,k,d,rate,delay", [(5, 7, 1, 2, 0), (4, 7, 9, 1, 0), (3, 3, 3, 3, 3)])
def test_depthwise_restatement_equals_the_oracle_block_and_needs_its_select(c, k, d, rate, delay):
    sd = _resdw_sd(c, k)
    assert float(sd["conv1.0.conv.bias"].abs().min()) >= 0.5
    x = torch.randn(2, c, 6 * rate, generator=torch.Generator().manual_seed(2), dtype=F64)
    want = codec.residual_block(x, sd, "", d)
    for schedule in SCHEDULES:
        y = _stream_resdw(sd, x, d, schedule, rate, delay)
        err = float((y[:, :, delay:delay + 6 * rate] - want).abs().max()) / float(want.abs().max())
        print(f"resdw C={c} k={k} d={d} rate={rate} delay={delay} schedule {schedule}: relative {err:.3e}")
        assert err < REL
        assert delay == 0 or float(y[:, :, :delay].abs().max()) == 0.0
    # without the select the conv sees shift, not 0, before the start of the stream: wrong within the reach, right behind it
    y = _stream_resdw(sd, x, d, [2, 1, 3], rate, delay, select=False)[:, :, delay:delay + 6 * rate]
    hh = d * (k - 1)
    head = float((y[:, :, :hh] - want[:, :, :hh]).abs().max())
    print(f"resdw without the select: {head:.3e} at the start of the clip")
    assert head > 1e-2
    if hh < 6 * rate:
        assert float((y[:, :, hh:] - want[:, :, hh:]).abs().max()) < REL * float(want.abs().max())


def test_counted_restatement_takes_the_first_frames_and_reads_nothing_behind_them():
    h0, h1, w = _multires_params(4, 3, 2)
    ring = torch.randn(3, 4, 6 + 4 * 2, generator=torch.Generator().manual_seed(3), dtype=F64)
    pos, counts = [5, 2, 9], [0, 4, 1]
    full = ref.multires_step(h0, h1, w, 2, ring, torch.zeros(3, 4, 8, dtype=F64), pos, None, 4, 2, 0, dst_ring=False)
    dirty = ring.clone()
    for r, (p, cnt) in enumerate(zip(pos, counts)):                 # NaN in every column behind a row's count
        j = torch.arange((p + cnt) * 2, (p + 4) * 2)
        dirty[r][:, torch.remainder(j, ring.shape[2])] = float("nan")
    dst = torch.full((3, 4, 8), 7.0, dtype=F64)
    got = ref.multires_step(h0, h1, w, 2, dirty, dst, pos, None, 4, 2, 0, dst_ring=False, counts=counts)
    assert float(got[0].abs().max()) == 0.0 and torch.equal(got[1], full[1]) and torch.equal(got[2, :, :2], full[2, :, :2])
    assert float(got[2, :, 2:].abs().max()) == 0.0 and torch.equal(dst, got)
    ring_dst = torch.full((3, 4, 11), 7.0, dtype=F64)
    ref.multires_step(h0, h1, w, 2, dirty, ring_dst, pos, None, 4, 2, 0, counts=counts)
    assert float((ring_dst[0] - 7.0).abs().max()) == 0.0 and int((ring_dst[2] != 7.0).sum()) == 4 * 2
    sd = _resdw_sd(4, 3)
    op1, op2, scale, shift = _resdw_ops(sd, 3)
    full, _ = ref.resdw_unit_step(op1, op2, scale, shift, ring, torch.zeros(3, 4, 8, dtype=F64), pos, None, 4, 2, 0, dst_ring=False)
    got, bound = ref.resdw_unit_step(op1, op2, scale, shift, dirty, torch.zeros(3, 4, 8, dtype=F64), pos, None, 4, 2, 0, dst_ring=False,
                                     counts=counts)
    assert float(got[0].abs().max()) == 0.0 and torch.equal(got[1], full[1]) and torch.equal(got[2, :, :2], full[2, :, :2])
    assert float(got[2, :, 2:].abs().max()) == 0.0 and float(bound[2, :, 2:].abs().max()) == 0.0 and float(bound[1].min()) > 0.0


# --------------------------------------------------------------------------------------------- the plans
CONFIG4 = dict(in_channels=2, n_blocks=4, strides=(2, 4, 5, 8), num_quantizers=2, codebook_size=64, codebook_dim=512, input_format="n c l",
               wavelet_decoders=[False, True, False, False], multires_encoders=[True, False, True, False],
               multires_decoders=[False, False, True, True], multires_kernel_size=3, multires_depth=4)
KEYS = ("multires_encoders", "multires_decoders", "multires_kernel_size", "multires_depth", "depthwise")


def _meta(**kw):
    with torch.device("meta"):
        return CausalVQAE(**kw).eval()


def _strip(units):
    """A stack's plan without its multires units, the depthwise blocks as plain ones: what the same model without them plans."""
    return [(("res" if u.kind == "resdw" else u.kind), u.c_in, u.c_out, u.k, u.s, u.d, u.rate_in, u.delay_in, u.rate_out, u.delay_out,
             u.reach, u.cap) for u in units if u.kind != "multires"]


def _check_plan(kw, max_chunk, k, depth, enc_rates, dec_rates):
    model, bare = _meta(**kw), _meta(**{a: b for a, b in kw.items() if a not in KEYS})
    p = streaming.plan(model, max_chunk, wavelet_blocks=True, multires_layers=True, depthwise_blocks=True)
    p0 = streaming.plan(bare, max_chunk, wavelet_blocks=True)
    reach = (k - 1) * ((1 << depth) - 1)
    for units, rates in ((p.encoders, enc_rates), (p.decoders, dec_rates)):
        mr = [u for u in units if u.kind == "multires"]
        assert [u.rate_in for u in mr] == rates
        for u in mr:
            prev = units[units.index(u) - 1]
            assert (u.k, u.s, u.depth, u.reach, u.cap) == (k, 1, depth, reach, reach + max_chunk * u.rate_in)
            assert (u.rate_out, u.delay_out) == (u.rate_in, u.delay_in) == (prev.rate_out, prev.delay_out) and u.c_in == u.c_out == prev.c_out
    assert _strip(p.encoders) == _strip(p0.encoders) and _strip(p.decoders) == _strip(p0.decoders)
    want_dw = bool(kw.get("depthwise"))
    for units in (p.encoders, p.decoders):
        blocks = [u for u in units if u.kind in ("res", "resdw")]
        assert blocks and all((u.kind == "resdw") == want_dw for u in blocks)
        assert all(u.reach == u.d * (u.k - 1) and u.cap == u.reach + max_chunk * u.rate_in and u.rate_out == u.rate_in
                   and u.delay_out == u.delay_in for u in blocks)
    assert p.decoder_delay == p0.decoder_delay and p.flush_frames == p0.flush_frames
    assert p.enc_left == longform.receptive_field(model).enc_left
    assert p.enc_left == p0.enc_left + sum(reach * (p.scale_factor // r) for r in enc_rates)
    s = model.new_stream(2, max_chunk=max_chunk, device="meta", wavelet_blocks=True, multires_layers=True, depthwise_blocks=True)
    assert [tuple(r.shape) for r in s.dec_rings] == [(2, u.c_in, u.cap) for u in p.decoders]
    assert [tuple(r.shape) for r in s.enc_rings] == [(2, u.c_in, u.cap) for u in p.encoders]      # no new rings
    assert [h is not None for h in s.dec_hidden] == [u.kind == "wavelet" for u in p.decoders]
    return p


def test_plan_of_the_default_architecture_with_multires_layers():
    p = _check_plan(dict(multires_encoders=True, multires_decoders=True), 4, 2, 3, [240, 80, 20, 5, 1], [5, 20, 80, 240, 480])
    assert p.decoder_delay == 1016 and p.scale_factor == 480
    assert [u.delay_in for u in p.decoders if u.kind == "multires"] == [5, 41, 168, 507, 1016]


def test_plan_of_the_default_architecture_with_depthwise_blocks():
    p = _check_plan(dict(depthwise=True), 4, 2, 3, [], [])
    assert p.decoder_delay == 1016 and sum(u.kind == "resdw" for u in p.decoders) == 15 == sum(u.kind == "resdw" for u in p.encoders)
    assert sorted({u.d for u in p.encoders if u.kind == "resdw"}) == [1, 3, 9] and {u.k for u in p.encoders if u.kind == "resdw"} == {7}


def test_plan_of_config_4():
    p = _check_plan(CONFIG4, 4, 3, 4, [160, 8], [160, 320])
    assert [u.reach for u in (*p.encoders, *p.decoders) if u.kind == "multires"] == [30] * 4


def test_a_reach_the_step_kernel_cannot_hold_is_refused_at_plan_time():
    model = _meta(in_channels=1, n_blocks=2, strides=(2, 3), first_block_channels=4, codebook_dim=8, num_quantizers=2, codebook_size=16,
                  wavelet_decoders=False, multires_encoders=True, multires_kernel_size=3, multires_depth=13)
    with pytest.raises(NotImplementedError, match="reach 16382"):
        streaming.plan(model, 2, multires_layers=True)
    assert not ops.multires_stream_fits(3, 13, 1) and ops.multires_stream_fits(3, 11, 1024) and not ops.multires_stream_fits(2, 21, 1)


# --------------------------------------------------------------------------------------------- the surface
ARGS = dict(in_channels=1, n_blocks=2, strides=(2, 3), first_block_channels=4, codebook_dim=8, num_quantizers=2, codebook_size=16,
            input_format="n c l")


def test_without_the_keywords_nothing_changes():
    mr = CausalVQAE(wavelet_decoders=False, multires_decoders=True, **ARGS).eval()
    dw = CausalVQAE(wavelet_decoders=False, depthwise=True, **ARGS).eval()
    for kw in ({}, dict(wavelet_blocks=True), dict(depthwise_blocks=True), dict(multires_layers=False)):
        with pytest.raises(NotImplementedError, match="a multiresolution layer has no streaming step"):
            mr.new_stream(1, **kw)
    for kw in ({}, dict(wavelet_blocks=True), dict(multires_layers=True), dict(depthwise_blocks=False)):
        with pytest.raises(NotImplementedError, match=r"a depthwise residual block \(depthwise=True\) has no streaming step"):
            dw.new_stream(1, **kw)
    for wav in (False, (True, False)):
        plain = CausalVQAE(wavelet_decoders=wav, **ARGS).eval()
        assert streaming.plan(plain, 3, wavelet_blocks=True) == streaming.plan(plain, 3, wavelet_blocks=True, multires_layers=True,
                                                                                depthwise_blocks=True)
    both = CausalVQAE(wavelet_decoders=(True, False), multires_encoders=True, multires_decoders=True, depthwise=True, **ARGS).eval()
    s = both.new_stream(2, max_chunk=3, wavelet_blocks=True, multires_layers=True, depthwise_blocks=True)
    assert {u.kind for u in s.plan.decoders} == {"convt", "wavelet", "up", "multires", "resdw", "causal"}
    with torch.no_grad(), pytest.raises(AgxError, match="MI355X only"):       # a valid call: no CPU fallback
        both.decode_stream(torch.zeros(2, 8, 2), s)
    with torch.no_grad(), pytest.raises(AgxError, match="MI355X only"):
        both.encode_stream(torch.zeros(2, 1, 12), s)


def test_wrapper_refusals_precede_every_launch():
    """On the CPU nothing can be launched: a call that got past the shape checks raises the 'MI355X only' error instead."""
    f = torch.zeros
    pos = f(2, dtype=torch.int64)
    ok = dict(h0=f(6, 1, 3), h1=f(6, 1, 3), w=f(6, 4), depth=2, src=f(2, 6, 6 + 8), dst=f(2, 6, 8), pos=pos, n=4, rate=2, delay=0,
              dst_ring=False)
    for change, match in ((dict(n=0), "n >= 1"), (dict(rate=0), "rate = 0"), (dict(delay=-1), "delay = -1"),
                          (dict(src=f(2, 6, 13)), "alias its history"), (dict(src=f(2, 5, 14)), "parameter shapes"),
                          (dict(w=f(6, 5)), "parameter shapes"), (dict(h1=f(6, 1, 2)), "parameter shapes"),
                          (dict(dst=f(2, 6, 7)), "plain columns"), (dict(dst=f(2, 6, 7), dst_ring=True), "new columns of a ring"),
                          (dict(dst=f(1, 6, 8)), "batch 2"), (dict(src=f(2, 6, 14).double()), "contiguous float32"),
                          (dict(depth=13, w=f(6, 15), src=f(2, 6, 2 * 8191 + 8)), "does not fit"), ({}, "MI355X only")):
        with pytest.raises(AgxError, match=match):
            ops.multires_stream_step(**{**ok, **change})
    img = f(16 * 7 * 5)
    okc = dict(c_in=5, c_out=5, kernel=7, dilation=3, packed=img, bias=None, scale=f(5), shift=f(5), src=f(2, 5, 18 + 4), dst=f(2, 5, 4),
               pos=pos, n=4, rate_in=1, delay_in=0, dst_ring=False, epilogue=EPI_LEAKY_PRE)
    for change, match in ((dict(kind=CONV_TRANSPOSED), "stride-1 causal conv reading a ring"), (dict(stride=2), "stride-1 causal conv"),
                          (dict(src_ring=False), "reading a ring"), (dict(shift=f(4)), r"two contiguous float32 \(5,\)"),
                          (dict(scale=f(5).double()), "two contiguous"), (dict(scale=f(10)[::2]), "two contiguous"),
                          ({}, "MI355X only")):
        with pytest.raises(AgxError, match=match):
            ops.conv_stream_step_affine(**{**okc, **change})


@pytest.fixture(scope="module")
def lib():
    from audio_generation_amd import build
    build.build()
    return _lib.load()


SYMBOLS = ("agx_multires_stream_step", "agx_conv_stream_step_affine")
BAD_SHAPE, NULL_POINTER, UNSUPPORTED = -1, -2, -5


def test_new_symbols_are_declared_bound_and_exported(lib):
    assert lib.agx_version() == 122
    header = open(os.path.join(ROOT, "include", "agx.h")).read()
    for name in SYMBOLS:
        for sym in (name, name + "_counted"):
            assert sym + "(" in header and sym in _lib.SIGNATURES and hasattr(lib, sym), sym
        plain, counted = _lib.SIGNATURES[name][1], _lib.SIGNATURES[name + "_counted"][1]
        assert len(counted) == len(plain) + 1
        at = [i for i in range(len(plain)) if counted[:i] == plain[:i] and counted[i + 1:] == plain[i:]]
        assert at and any(counted[i] is ctypes.c_void_p for i in at), name      # the plain signature plus one pointer: counts
    assert _lib.SIGNATURES["agx_conv_stream_step_affine"][1][:10] == _lib.SIGNATURES["agx_conv_stream_step"][1][:10]
    assert len(_lib.SIGNATURES["agx_conv_stream_step_affine"][1]) == len(_lib.SIGNATURES["agx_conv_stream_step"][1]) + 2
    assert ops.MULTIRES_STREAM_TILE == 1024 and "#define AGX_MULTIRES_STREAM_TILE 1024" in header
    assert f"#define AGX_MULTIRES_STREAM_LDS_BYTES {ops.MULTIRES_STREAM_LDS_BYTES}" in header


def test_library_refusals_precede_every_use_of_a_pointer(lib):
    one, two = ctypes.c_void_p(64), ctypes.c_void_p(4096)              # never dereferenced

    def mr(h0=one, src=one, src_cap=14, dst=two, dst_cap=0, pos=one, batch=2, c=6, n=4, k=3, depth=2, rate=2, delay=0, counted=None):
        if counted is not None:
            return lib.agx_multires_stream_step_counted(h0, one, one, src, src_cap, dst, dst_cap, pos, None, counted[0], batch, c, n, k,
                                                        depth, rate, delay, None)
        return lib.agx_multires_stream_step(h0, one, one, src, src_cap, dst, dst_cap, pos, None, batch, c, n, k, depth, rate, delay, None)

    assert mr(src_cap=13) == BAD_SHAPE and "alias its history" in lib.agx_last_error().decode()
    assert mr(dst_cap=7) == BAD_SHAPE and "written twice" in lib.agx_last_error().decode()
    assert mr(dst=one) == BAD_SHAPE and "the destination is the source" in lib.agx_last_error().decode()
    assert mr(h0=None) == NULL_POINTER and mr(src=None) == NULL_POINTER and mr(dst=None) == NULL_POINTER and mr(pos=None) == NULL_POINTER
    assert mr(k=0) == BAD_SHAPE and mr(depth=21) == BAD_SHAPE and mr(depth=-1) == BAD_SHAPE and mr(rate=0) == BAD_SHAPE
    assert mr(c=0) == BAD_SHAPE and mr(delay=-1) == BAD_SHAPE and mr(batch=65536) == BAD_SHAPE
    assert mr(depth=13, src_cap=1 << 20) == UNSUPPORTED and "LDS" in lib.agx_last_error().decode()
    assert mr(n=1 << 24, src_cap=1 << 30) == BAD_SHAPE and "beyond the grid" in lib.agx_last_error().decode()
    assert mr(n=0) == 0 and mr(batch=0) == 0 and mr(n=0, src=None) == 0
    assert mr(counted=(None,)) == NULL_POINTER and "NULL counts" in lib.agx_last_error().decode()

    def aff(kind=CONV_CAUSAL, stride=1, src_cap=22, scale=one, shift=one, dst=two, n=4, counted=None):
        head = (kind, 5, 5, 7, stride, 3, EPI_LEAKY_PRE, 0.1, one, None, scale, shift, one, src_cap, None, 0, dst, 0, one, None)
        if counted is not None:
            return lib.agx_conv_stream_step_affine_counted(*head, counted[0], 2, n, 1, 0, None)
        return lib.agx_conv_stream_step_affine(*head, 2, n, 1, 0, None)

    assert aff(kind=CONV_TRANSPOSED) == UNSUPPORTED and "stride-1 causal conv reading a ring" in lib.agx_last_error().decode()
    assert aff(src_cap=0) in (UNSUPPORTED, BAD_SHAPE) and aff(src_cap=21) == BAD_SHAPE
    assert aff(scale=None) == NULL_POINTER and aff(shift=None) == NULL_POINTER and "scale or shift" in lib.agx_last_error().decode()
    assert aff(dst=one) == BAD_SHAPE and aff(n=0) == 0
    assert aff(counted=(None,)) == NULL_POINTER and "NULL counts" in lib.agx_last_error().decode()
    # a strided causal conv: the stride has to divide the rate first; with rate 2 it is the affine's own refusal
    head = (CONV_CAUSAL, 5, 5, 7, 2, 3, 0, 0.1, one, None, one, one, one, 64, None, 0, two, 0, one, None)
    assert lib.agx_conv_stream_step_affine(*head, 2, 4, 2, 0, None) == UNSUPPORTED
