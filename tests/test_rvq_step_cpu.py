"""The RVQ streaming step without a GPU: its four entry points in header, binding and library, the packet size, the
packet layout's CPU statement (tests/rvq_step_ref.py) and the model-level refusals, which precede every launch."""
import os

import numpy as np
import pytest
import torch

from audio_generation_amd import _lib, ops
from audio_generation_amd._lib import AgxError
from oracle import bitstream
from tests import rvq_step_ref as ref
from tests.test_codec_stream_cpu import _model

SYMBOLS = ("agx_rvq_step_packet_bytes", "agx_rvq_step_workspace_bytes", "agx_rvq_step_encode", "agx_rvq_step_decode")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "agx.h")


def test_entry_points_in_header_binding_and_library():
    lib = _lib.load()
    header = open(HEADER).read()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.agx_version() == 122 and "#define AGX_VERSION 122" in header
    assert f"#define AGX_RVQ_STEP_MAX_N {ops.RVQ_STEP_MAX_N}\n" in header and ops.RVQ_STEP_MAX_N >= 8
    assert len(_lib.SIGNATURES["agx_rvq_step_encode"][1]) == 23 and len(_lib.SIGNATURES["agx_rvq_step_decode"][1]) == 17


def test_packet_bytes_on_a_grid_and_its_refusals():
    lib = _lib.load()
    for n in (1, 2, 3, 4, 8, ops.RVQ_STEP_MAX_N):
        for q in (0, 1, 2, 3, 8, 64):
            for bits in (1, 5, 8, 10, 11, 16):
                want = -((-n * q * bits) // 8)
                assert lib.agx_rvq_step_packet_bytes(n, q, bits) == want == ref.packet_bytes(n, q, bits), (n, q, bits)
                assert ops.rvq_step_packet_bytes(n, q, bits) == want
    assert lib.agx_rvq_step_packet_bytes(1, 2, 5) == 2 and lib.agx_rvq_step_packet_bytes(3, 2, 5) == 4   # 10-bit frames end mid-byte
    for bad in ((0, 2, 10), (-1, 2, 10), (ops.RVQ_STEP_MAX_N + 1, 2, 10), (4, -1, 10), (4, 65, 10), (4, 2, 0), (4, 2, 17)):
        assert lib.agx_rvq_step_packet_bytes(*bad) < 0, bad
        with pytest.raises(AgxError, match="rvq_step_packet_bytes"):
            ops.rvq_step_packet_bytes(*bad)


def test_workspace_bytes_cover_the_partials():
    lib = _lib.load()
    assert lib.agx_rvq_step_workspace_bytes(8, 4, 512, 1024, 0) == 0 and lib.agx_rvq_step_workspace_bytes(0, 4, 512, 1024, 8) == 0
    f, d, k, q = 8 * 4, 512, 1024, 8
    nb = k // 64
    floor = 2 * f * nb * 12 + 2 * f * d * 4 + f * q * 4        # two slots of (binary64, int32) partials and of residuals, the codes
    got = lib.agx_rvq_step_workspace_bytes(8, 4, d, k, q)
    assert floor <= got <= floor + 64 and got % 8 == 0
    assert lib.agx_rvq_step_workspace_bytes(1, 1, 20, 24, 2) >= 2 * 12 + 2 * 20 * 4 + 2 * 4


@pytest.mark.parametrize("bits,q,k", [(5, 2, 24), (10, 8, 1024), (1, 3, 2), (16, 1, 65536), (11, 3, 2048)])
def test_packet_layout_reference(bits, q, k):
    """tests/rvq_step_ref.packets: the zero tail, row independence, and the round trip through oracle.bitstream.unpack."""
    rng = np.random.default_rng(bits * 100 + q)
    n, counts = 4, [0, 1, 4, 9, -3, 3]
    b = len(counts)
    index = rng.integers(0, k, size=(b, n, q), dtype=np.int64)
    index[2, -1, -1] = k - 1                                   # the top bits of the last live code are set
    got = ref.packets(index, counts, bits)
    assert got.dtype == np.uint8 and got.shape == (b, ref.packet_bytes(n, q, bits))
    for r, c in enumerate(ref.taken(counts, b, n)):
        live = ref.packet_bytes(c, q, bits) if c else 0
        assert not got[r, live:].any(), r                                                    # every byte behind the packet
        if c:
            assert np.array_equal(got[r, :live], bitstream.pack(index[r, :c].reshape(-1), bits))
            unused = live * 8 - c * q * bits                                                 # high bits of the last byte
            assert 0 <= unused < 8 and int(got[r, live - 1]) >> (8 - unused) == 0
            assert np.array_equal(ref.unpack_row(got[r], c, q, bits), index[r, :c])        # the round trip, zero tail included
            assert np.array_equal(ref.unpack_row(got[r, :live], c, q, bits), index[r, :c])
    assert ref.taken(counts, b, n) == [0, 1, 4, 4, 0, 3] and not got[0].any() and not got[4].any()
    other = index.copy()
    other[3] = rng.integers(0, k, size=(n, q))                 # rows never share a byte: only row 3's packet changes
    again = ref.packets(other, counts, bits)
    keep = [r for r in range(b) if r != 3]
    assert np.array_equal(again[keep], got[keep])
    assert np.array_equal(ref.packets(index, None, bits), ref.packets(index, [n] * b, bits))
    whole = ref.packets(index, None, bits)
    for r in range(b):                                                                       # a full row is the plain packing
        assert np.array_equal(whole[r], bitstream.pack(index[r].reshape(-1), bits))


def test_model_refusals_precede_every_launch():
    """On the CPU nothing can be launched: a call that got past the checks would raise the 'MI355X only' error instead."""
    model, other = _model(), _model()                         # Q = 2, K = 16: 4-bit codes, sf = 6, D = 8
    s = model.new_stream(2, max_chunk=3)
    assert model._code_bits == 4
    x, packets = torch.zeros(2, 1, 12), torch.zeros(2, 2, dtype=torch.uint8)
    with torch.no_grad():
        with pytest.raises(AgxError, match="another model"):
            other.compress_stream(x, s)
        with pytest.raises(AgxError, match="another model"):
            other.decompress_stream(packets, s, 2)
        with pytest.raises(AgxError, match="max_chunk"):
            model.compress_stream(torch.zeros(2, 1, 24), s)
        for frames in (0, 4):
            with pytest.raises(AgxError, match="max_chunk"):
                model.decompress_stream(packets, s, frames)
        with pytest.raises(AgxError, match=r"uint8 \(B, 2\)"):
            model.decompress_stream(torch.zeros(2, 3, dtype=torch.uint8), s, 2)          # the wrong width
        with pytest.raises(AgxError, match=r"uint8 \(B, 1\)"):
            model.decompress_stream(packets, s, 2, codebook_n=1)
        with pytest.raises(AgxError, match="uint8"):
            model.decompress_stream(torch.zeros(2, 2, dtype=torch.int64), s, 2)
        with pytest.raises(AgxError, match="uint8"):
            model.decompress_stream(torch.zeros(4, dtype=torch.uint8), s, 2)
        with pytest.raises(AgxError, match="batch"):
            model.decompress_stream(torch.zeros(3, 2, dtype=torch.uint8), s, 2)
        with pytest.raises(AgxError, match="counts"):
            model.decompress_stream(packets, s, 2, counts=torch.zeros(2, dtype=torch.int32))
        with pytest.raises(AgxError, match="counts"):
            model.compress_stream(x, s, counts=torch.zeros(3, dtype=torch.int64))
        with pytest.raises(AgxError, match="on 'cpu'"):
            model.decompress_stream(packets, model.new_stream(2, max_chunk=3, device="meta"), 2)
        with pytest.raises(AgxError, match="MI355X only"):                                # past every check: the launch is next
            model.decompress_stream(packets, s, 2)
    model.train()
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="inference only"):
            model.compress_stream(x, s)
        with pytest.raises(NotImplementedError, match="inference only"):
            model.decompress_stream(packets, s, 2)
    model.eval()
    from torch import nn
    model.replace_quantizer(nn.Identity())
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="ResidualQuantizer"):
            model.compress_stream(x, s)
        with pytest.raises(NotImplementedError, match="ResidualQuantizer"):
            model.decompress_stream(packets, s, 2)


def test_op_refusals_on_the_cpu():
    z, cbs = torch.zeros(2, 8, 3), torch.zeros(2, 16, 8)
    with pytest.raises(AgxError, match="MI355X only"):
        ops.rvq_step_encode(z, cbs, 2)
    with pytest.raises(AgxError, match="MI355X only"):
        ops.rvq_step_decode(torch.zeros(2, 3, dtype=torch.uint8), 3, cbs, 2, 4)
