"""Per-row stage counts of the RVQ streaming step without a GPU: the three new entry points in header, binding and
library beside the untouched old ones, the CPU statement of the staged packets (tests/rvq_stages_ref.py), ``stages_for_bitrate``,
and the refusals of ops and model, which precede every launch."""
import os

import numpy as np
import pytest
import torch

from audio_generation_amd import _lib, ops
from audio_generation_amd._lib import AgxError
from oracle import bitstream
from tests import rvq_stages_ref as sref
from tests import rvq_step_ref as ref
from tests.test_codec_stream_cpu import _model

SYMBOLS = ("agx_rvq_step_encode_staged", "agx_rvq_step_decode_staged", "agx_rvq_packets_restage")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "agx.h")


def test_entry_points_in_header_binding_and_library():
    lib = _lib.load()
    header = open(HEADER).read()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "Per-row stage counts" in header
    assert lib.agx_version() == 122 and "#define AGX_VERSION 122" in header                  # new symbols, the same version
    sig = _lib.SIGNATURES
    assert len(sig["agx_rvq_step_encode"][1]) == 23 and len(sig["agx_rvq_step_decode"][1]) == 17       # the old ones as they were
    assert len(sig["agx_rvq_step_encode_staged"][1]) == 24 and len(sig["agx_rvq_step_decode_staged"][1]) == 18
    assert len(sig["agx_rvq_packets_restage"][1]) == 11


def test_taken_stages_clamps_at_both_ends():
    assert sref.taken_stages([4, 1, 2, 0, 2, -7], 6, 3) == [3, 1, 2, 0, 2, 0]
    assert sref.taken_stages(None, 4, 8) == [8] * 4


@pytest.mark.parametrize("bits,q_used,k", [(5, 3, 24), (10, 8, 1024), (1, 3, 2), (16, 2, 65536), (11, 3, 2048)])
def test_staged_packet_layout_reference(bits, q_used, k):
    """tests/rvq_stages_ref.packets: uniform stages are the plain packets of the index prefix, rows never share a byte, the zero
    tail, and the round trip through oracle.bitstream.unpack."""
    rng = np.random.default_rng(bits * 100 + q_used)
    n, counts = 4, [0, 1, 4, 9, -3, 3]
    b = len(counts)
    index = rng.integers(0, k, size=(b, n, q_used), dtype=np.int64)
    index[2, -1, :] = k - 1                                    # the top bits of the last live code are set, at every stage count
    p = ref.packet_bytes(n, q_used, bits)
    for q in range(q_used + 1):                                # every row at q: the packets of index[..., :q], in the width of q_used
        got = sref.packets(index, counts, [q] * b, bits, q_used)
        plain = ref.packets(index[..., :q], counts, bits)
        assert got.shape == (b, p) and got.dtype == np.uint8
        assert np.array_equal(got[:, :plain.shape[1]], plain) and not got[:, plain.shape[1]:].any(), q
    assert np.array_equal(sref.packets(index, counts, None, bits, q_used), ref.packets(index, counts, bits))
    stages = [q_used + 5, 1, 2, 0, 2, q_used - 1]
    taken_q = sref.taken_stages(stages, b, q_used)
    got = sref.packets(index, counts, stages, bits, q_used)
    for r, (c, q) in enumerate(zip(ref.taken(counts, b, n), taken_q)):
        live = sref.live_bytes(c, q, bits)
        assert not got[r, live:].any(), r                                                    # every byte behind the packet
        if c * q:
            assert np.array_equal(got[r, :live], bitstream.pack(index[r, :c, :q].reshape(-1), bits))
            unused = live * 8 - c * q * bits                                                 # high bits of the last byte
            assert 0 <= unused < 8 and int(got[r, live - 1]) >> (8 - unused) == 0
            assert np.array_equal(ref.unpack_row(got[r], c, q, bits), index[r, :c, :q])      # the round trip, zero tail included
    back = sref.unpacked(got, counts, stages, bits, q_used, n)
    for r, (c, q) in enumerate(zip(ref.taken(counts, b, n), taken_q)):
        assert np.array_equal(back[r, :c, :q], index[r, :c, :q]) and (back[r, c:] == -1).all() and (back[r, :, q:] == -1).all()
    other = index.copy()
    other[2] = rng.integers(0, k, size=(n, q_used))            # rows never share a byte: only row 2's packet changes
    again = sref.packets(other, counts, stages, bits, q_used)
    keep = [r for r in range(b) if r != 2]
    assert np.array_equal(again[keep], got[keep]) and not np.array_equal(again[2], got[2])


@pytest.mark.parametrize("bits,q_used,k", [(5, 3, 24), (10, 8, 1024), (3, 4, 8)])
def test_restaged_reference(bits, q_used, k):
    rng = np.random.default_rng(7 * bits + q_used)
    n, counts = 4, [4, 2, -1, 3, 9]
    b = len(counts)
    index = rng.integers(0, k, size=(b, n, q_used), dtype=np.int64)
    stages_in = [q_used, 1, 2, q_used - 1, 99]
    pk = sref.packets(index, counts, stages_in, bits, q_used)
    same, q_same = sref.restaged(pk, counts, stages_in, stages_in, bits, q_used, n=n)           # to q_in: the identity
    assert np.array_equal(same, pk) and q_same == sref.taken_stages(stages_in, b, q_used)
    up, q_up = sref.restaged(pk, counts, stages_in, [99] * b, bits, q_used, n=n)                # never upward
    assert np.array_equal(up, pk) and q_up == q_same
    none, q_none = sref.restaged(pk, counts, stages_in, [0] * b, bits, q_used, n=n)             # to 0: all zeros
    assert not none.any() and q_none == [0] * b
    to = [2, 0, 1, 2, 1]
    got, q_out = sref.restaged(pk, counts, stages_in, to, bits, q_used, n=n)
    assert q_out == [min(a, t) for a, t in zip(q_same, to)]
    assert np.array_equal(got, sref.packets(index, counts, q_out, bits, q_used))                 # = the encode at the minimum
    full = sref.packets(index, counts, None, bits, q_used)
    assert np.array_equal(sref.restaged(full, counts, None, to, bits, q_used, n=n)[0], sref.packets(index, counts, to, bits, q_used))
    if q_used * bits >= 8:                                                                       # then P fixes n
        assert np.array_equal(sref.restaged(pk, counts, stages_in, to, bits, q_used)[0], got)


def test_reference_rows_are_prefix_runs():
    gen = torch.Generator().manual_seed(3)
    b, n, d, k, q = 4, 3, 8, 16, 3
    z, cbs = torch.randn(b, d, n, generator=gen), torch.randn(q, k, d, generator=gen)
    full_q, full_i = ref.exact_reference(z, cbs)
    counts, stages = [3, 2, 0, 3], [3, 1, 2, 0]
    zq, index = sref.reference(z, cbs, None, counts, stages)
    assert torch.equal(zq[0], full_q[0]) and torch.equal(index[0], full_i[0])
    assert torch.equal(index[1, :2, :1], full_i[1, :2, :1]) and bool((index[1, 2:] == -1).all()) and bool((index[1, :, 1:] == -1).all())
    assert torch.equal(zq[1, :, :2], cbs[0][full_i[1, :2, 0]].t()) and not zq[1, :, 2:].any()
    assert not zq[2].any() and not zq[3].any() and bool((index[2:] == -1).all())


def test_stages_for_bitrate_on_a_grid():
    model = _model()                                          # Q = 2, 4-bit codes, scale factor 6
    bits, sf, q_max = model._code_bits, model.scale_factor, model.num_quantizers
    assert (bits, sf, q_max) == (4, 6, 2)
    for sample_rate in (6000, 16000, 24000, 44100):
        per_stage = bits * sample_rate / sf
        for bitrate in (0, 1, per_stage - 1, per_stage, per_stage + 1, 2 * per_stage - 0.5, 2 * per_stage, 3 * per_stage, 1e9):
            want = max(q for q in range(q_max + 1) if q * bits * sample_rate / sf <= bitrate)
            got = model.stages_for_bitrate(bitrate, sample_rate)
            assert got == want and isinstance(got, int), (sample_rate, bitrate, got, want)
    assert model.stages_for_bitrate(0, 24000) == 0 and model.stages_for_bitrate(15999, 24000) == 0      # not even one stage
    assert model.stages_for_bitrate(16000, 24000) == 1 and model.stages_for_bitrate(32000, 24000) == 2
    assert model.stages_for_bitrate(1e12, 24000) == 2                                                     # the cap


def _bad_stages(batch):
    """(stages, why) that every entry must refuse: int32, the wrong length, a non-contiguous view."""
    return [(torch.zeros(batch, dtype=torch.int32), "int32"), (torch.zeros(batch + 1, dtype=torch.int64), "length"),
            (torch.zeros(2 * batch, dtype=torch.int64)[::2], "stride"), ([1] * batch, "a list")]


def test_op_refusals_precede_the_launch():
    n, q, bits = 3, 2, 4
    packets = torch.zeros(2, ref.packet_bytes(n, q, bits), dtype=torch.uint8)
    good = torch.ones(2, dtype=torch.int64)
    for bad, why in _bad_stages(2):
        with pytest.raises(AgxError, match="stages_to"):
            ops.rvq_packets_restage(packets, n, q, bits, bad)
        with pytest.raises(AgxError, match="stages_from"):
            ops.rvq_packets_restage(packets, n, q, bits, good, stages_from=bad)
    with pytest.raises(AgxError, match="stages_to is on 'meta'"):
        ops.rvq_packets_restage(packets, n, q, bits, good.to("meta"))
    with pytest.raises(AgxError, match="counts"):
        ops.rvq_packets_restage(packets, n, q, bits, good, counts=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(AgxError, match=r"uint8 \(B, 3\)"):
        ops.rvq_packets_restage(torch.zeros(2, 4, dtype=torch.uint8), n, q, bits, good)          # the wrong width
    with pytest.raises(AgxError, match="MI355X only"):                                           # past every check: the launch is next
        ops.rvq_packets_restage(packets, n, q, bits, good, stages_from=good, counts=good)
    z, cbs = torch.zeros(2, 8, 3), torch.zeros(2, 16, 8)
    with pytest.raises(AgxError, match="MI355X only"):
        ops.rvq_step_encode(z, cbs, 2, stages=good)
    with pytest.raises(AgxError, match="MI355X only"):
        ops.rvq_step_decode(packets, n, cbs, q, bits, stages=good)
    with pytest.raises(TypeError):
        ops.rvq_step_encode(z, cbs, 2, None, None, None, True, good)                             # stages is keyword-only
    with pytest.raises(TypeError):
        ops.rvq_step_decode(packets, n, cbs, q, bits, None, None, False, good)


def test_model_refusals_precede_every_launch():
    """On the CPU nothing can be launched: a call that got past the checks raises the 'MI355X only' error instead."""
    model = _model()                                          # Q = 2, K = 16: 4-bit codes, sf = 6, D = 8
    s = model.new_stream(2, max_chunk=3)
    x, packets = torch.zeros(2, 1, 12), torch.zeros(2, 2, dtype=torch.uint8)
    good = torch.ones(2, dtype=torch.int64)
    with torch.no_grad():
        for bad, why in _bad_stages(2):
            with pytest.raises(AgxError, match="stages"):
                model.compress_stream(x, s, stages=bad)
            with pytest.raises(AgxError, match="stages"):
                model.decompress_stream(packets, s, 2, stages=bad)
            with pytest.raises(AgxError, match="stages"):
                model.restage_packets(packets, 2, bad)
            with pytest.raises(AgxError, match="stages_from"):
                model.restage_packets(packets, 2, good, stages_from=bad)
        meta = model.new_stream(2, max_chunk=3, device="meta")
        with pytest.raises(AgxError, match="stages is on 'cpu'"):                            # a CPU tensor for a stream elsewhere
            model.compress_stream(x.to("meta"), meta, stages=good)
        with pytest.raises(AgxError, match="stages is on 'cpu'"):
            model.decompress_stream(packets.to("meta"), meta, 2, stages=good)
        with pytest.raises(AgxError, match="stages_to is on 'cpu'"):
            model.restage_packets(packets.to("meta"), 2, good)
        with pytest.raises(AgxError, match=r"uint8 \(B, 2\)"):
            model.restage_packets(torch.zeros(2, 3, dtype=torch.uint8), 2, good)                 # the wrong width
        with pytest.raises(AgxError, match=r"uint8 \(B, 1\)"):
            model.restage_packets(packets, 2, good, codebook_n=1)
        with pytest.raises(AgxError, match="frames"):
            model.restage_packets(packets, 0, good)
        with pytest.raises(AgxError, match="MI355X only"):                                       # past every check: the launch is next
            model.decompress_stream(packets, s, 2, stages=good)
        with pytest.raises(AgxError, match="MI355X only"):
            model.restage_packets(packets, 2, good, stages_from=good, counts=good)
        with pytest.raises(AgxError, match="MI355X only"):
            model.compress_stream(x, s, stages=good)
