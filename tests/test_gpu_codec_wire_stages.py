"""A sender, a relay and a receiver over packets with one bitrate per stream (``compress_stream(stages=)``, ``restage_packets``,
``decompress_stream(stages=)``).

A codec of the size of tests/test_gpu_codec_stream_counts.py's, with four quantiser stages: batch 3, ``max_chunk = 4``, six hops in
which both the frame count and the stage count of every row change -- a row sends no stage in one hop and is paused in another.
Every comparison is ``torch.equal`` against the CPU statement (tests/rvq_stages_ref.py) or against a twin stream of the SAME batch
on the same kernels, so nothing here leans on batch-size invariance.
"""
import numpy as np
import pytest
import torch

from audio_generation_amd import streaming
from audio_generation_amd.graph import GraphedForward
from audio_generation_amd.vae import CausalVQAE
from tests import rvq_stages_ref as sref
from tests import rvq_step_ref as ref
from tests.test_gpu_codec_stream import DEV
from tests.test_gpu_codec_stream_counts import _counted_chunk
from tests.test_gpu_longform import _data_codebooks

pytestmark = pytest.mark.gpu
B, T, N, Q = 3, 12, 4, 4
COUNTS = ([4, 4, 4, 0, 0, 0], [1, 0, 3, 2, 4, 2], [0, 0, 4, 4, 0, 4])          # per row: its 12 frames in six hops, with pauses
STAGES = ([4, 2, 0, 3, 1, 4], [3, 4, 1, 0, 9, 2], [0, 1, 2, 4, 3, -1])         # per row and hop; 9 and -1 clamp to 4 and 0
HOPS = list(zip(zip(*COUNTS), zip(*STAGES)))


def _i64(values):
    return torch.tensor(values, dtype=torch.int64, device=DEV)


@pytest.fixture(scope="module")
def case():
    """The model, the clip, and per hop the CPU reference of the sender on the latents of a twin stream:
    (counts, stages, zq, index, packets)."""
    torch.manual_seed(0)
    model = CausalVQAE(in_channels=1, n_blocks=2, strides=(2, 3), codebook_dim=16, num_quantizers=Q, codebook_size=32,
                       wavelet_decoders=False, input_format="n c l").eval().to(DEV)
    gen = torch.Generator().manual_seed(4321)
    x = (0.1 * torch.randn(B, 1, T * model.scale_factor, generator=gen)).clamp(-1, 1).to(DEV)
    cbs = _data_codebooks(model, x)
    assert model._code_bits == 5 and cbs.shape == (Q, 32, 16)
    assert any(c > 0 and min(max(s, 0), Q) == 0 for cs, ss in HOPS for c, s in zip(cs, ss))      # live frames, no stage
    assert any(c == 0 and s > 0 for cs, ss in HOPS for c, s in zip(cs, ss))                      # paused
    twin, at, hops = model.new_stream(B, max_chunk=N), [0] * B, []
    with torch.no_grad():
        for counts, stages in HOPS:
            z = streaming.encode_latents_stream(model, _counted_chunk(x, at, counts, model.scale_factor), twin, _i64(counts)).cpu()
            zq, index = sref.reference(z, cbs, None, counts, stages)
            hops.append((counts, stages, zq, index, sref.packets(index.numpy(), counts, stages, 5, Q)))
            at = [a + c for a, c in zip(at, counts)]
    assert at == [T] * B
    return model, x, hops


def _receiver_reference(model, hops):
    """``decode_stream`` on a twin stream of the same batch, fed the reference zq with the same counts."""
    twin = model.new_stream(B, max_chunk=N)
    with torch.no_grad():
        return [model.decode_stream(zq.to(DEV), twin, counts=_i64(counts)) for counts, _, zq, _, _ in hops], twin


def test_sender_packets_equal_the_reference(case):
    model, x, hops = case
    sf, bits = model.scale_factor, model._code_bits
    sender, at = model.new_stream(B, max_chunk=N), [0] * B
    with torch.no_grad():
        for counts, stages, want_q, want_i, want_p in hops:
            chunk = _counted_chunk(x, at, counts, sf)
            zq, index, packets = streaming.encode_codes_stream(model, chunk, sender, None, _i64(counts), _i64(stages))
            assert packets.shape == (B, ref.packet_bytes(N, Q, bits)) and packets.dtype == torch.uint8
            assert np.array_equal(packets.cpu().numpy(), want_p) and torch.equal(index.cpu(), want_i) and torch.equal(zq.cpu(), want_q)
            at = [a + c for a, c in zip(at, counts)]
            assert sender.positions()["enc_pos"] == at                      # the rings advance by c_b whatever q_b is
    with torch.no_grad():                                                    # the model's entry point is the same call
        again, at = model.new_stream(B, max_chunk=N), [0] * B
        for counts, stages, _, want_i, want_p in hops[:2]:
            packets, index = model.compress_stream(_counted_chunk(x, at, counts, sf), again, counts=_i64(counts), stages=_i64(stages))
            assert np.array_equal(packets.cpu().numpy(), want_p) and torch.equal(index.cpu(), want_i)
            at = [a + c for a, c in zip(at, counts)]


def test_receiver_equals_decode_stream_of_the_reference_zq(case):
    model, _, hops = case
    want_y, twin = _receiver_reference(model, hops)
    receiver, at = model.new_stream(B, max_chunk=N), [0] * B
    with torch.no_grad():
        for (counts, stages, _, want_i, want_p), want in zip(hops, want_y):
            y, index = model.decompress_stream(torch.from_numpy(want_p).to(DEV), receiver, N, counts=_i64(counts), stages=_i64(stages))
            assert torch.equal(y, want) and torch.equal(index.cpu(), want_i)
            at = [a + c for a, c in zip(at, counts)]
            assert receiver.positions()["dec_pos"] == at                    # a row with frames and no stage advances too
    assert receiver.positions() == twin.positions()
    assert max(float(w.abs().max()) for w in want_y) > 1e-3


def test_relay_restages_full_packets_to_the_schedule(case):
    model, x, hops = case
    want_y, _ = _receiver_reference(model, hops)
    sender, receiver, at = model.new_stream(B, max_chunk=N), model.new_stream(B, max_chunk=N), [0] * B
    with torch.no_grad():
        for (counts, stages, _, want_i, want_p), want in zip(hops, want_y):
            cd = _i64(counts)
            full, _ = model.compress_stream(_counted_chunk(x, at, counts, model.scale_factor), sender, counts=cd)
            packets, stages_out = model.restage_packets(full, N, _i64(stages), counts=cd)
            assert np.array_equal(packets.cpu().numpy(), want_p)
            assert stages_out.is_cuda and stages_out.tolist() == sref.taken_stages(stages, B, Q)
            y, index = model.decompress_stream(packets, receiver, N, counts=cd, stages=stages_out)
            assert torch.equal(y, want) and torch.equal(index.cpu(), want_i)
            at = [a + c for a, c in zip(at, counts)]


def test_graphed_sender_and_receiver_replay_with_changing_counts_and_stages(case):
    """One sender step and one receiver step, each captured once; between replays only ``copy_`` into the counts, the stages and
    the input buffers."""
    model, x, hops = case
    sf = model.scale_factor
    width = ref.packet_bytes(N, Q, model._code_bits)

    def run(send, receive, counts_t, stages_t):
        at, outs = [0] * B, []
        for counts, stages, _, _, _ in hops:
            counts_t.copy_(torch.tensor(counts, dtype=torch.int64))
            stages_t.copy_(torch.tensor(stages, dtype=torch.int64))
            packets, index = send(_counted_chunk(x, at, counts, sf))
            packets, index = packets.clone(), index.clone()
            y, index_r = receive(packets)
            outs.append((packets, index, y.clone(), index_r.clone()))
            at = [a + c for a, c in zip(at, counts)]
        return outs

    e_send, e_recv = model.new_stream(B, max_chunk=N), model.new_stream(B, max_chunk=N)
    e_counts, e_stages = _i64([0] * B), _i64([0] * B)
    with torch.no_grad():
        eager = run(lambda c: model.compress_stream(c, e_send, counts=e_counts, stages=e_stages),
                    lambda p: model.decompress_stream(p, e_recv, N, counts=e_counts, stages=e_stages), e_counts, e_stages)
    g_send, g_recv = model.new_stream(B, max_chunk=N), model.new_stream(B, max_chunk=N)
    g_counts, g_stages = _i64([0] * B), _i64([0] * B)
    send = GraphedForward(lambda c: model.compress_stream(c, g_send, counts=g_counts, stages=g_stages), torch.zeros(B, 1, N * sf, device=DEV))
    receive = GraphedForward(lambda p: model.decompress_stream(p, g_recv, N, counts=g_counts, stages=g_stages),
                             torch.zeros(B, width, dtype=torch.uint8, device=DEV))
    g_send.reset(), g_recv.reset()
    graphed = run(send, receive, g_counts, g_stages)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(graphed, eager)):
        assert all(torch.equal(u, v) for u, v in zip(a, b)), i
        assert np.array_equal(a[0].cpu().numpy(), hops[i][4]) and torch.equal(a[1].cpu(), hops[i][3]), i
    assert g_send.positions() == e_send.positions() and g_recv.positions() == e_recv.positions()
    assert g_send.positions()["enc_pos"] == [T] * B and g_recv.positions()["dec_pos"] == [T] * B
