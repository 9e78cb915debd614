"""``CausalVQAE`` streaming with per-row frame counts (``counts=``) against the uncounted stream of the same batch.

Model A of tests/test_gpu_codec_stream.py, batch 3, 12 frames per row, ``max_chunk = 4``: six steps of n = 4 in which every row
takes its own number of frames.  Each row's concatenated valid latents, indices and waveform are ``torch.equal`` to the uncounted
stream on [4, 4, 4] + finish + flush; the indices also equal ``oracle.rvq.residual_quantize`` on the stream's own latents.  The
chunk holds NaN behind every row's count.  Then a lifecycle on row 0 (finish, flush and reset of that row alone, a second clip)
and one captured ``forward_stream`` step replayed with changing counts.
"""
import pytest
import torch

from audio_generation_amd import ops, streaming
from audio_generation_amd.graph import GraphedForward
from oracle import rvq
from tests.test_gpu_codec_stream import DEV, _chunks, _model_a
from tests.test_gpu_longform import _data_codebooks, _frames

pytestmark = pytest.mark.gpu
B, T, N = 3, 12, 4
SCHEDULES = ([4, 4, 4, 0, 0, 0], [1, 0, 3, 2, 4, 2], [0, 0, 4, 4, 0, 4])       # per row; every row takes its 12 frames in six steps


def _model():
    model, _ = _model_a()
    gen = torch.Generator().manual_seed(4321)
    x = (0.1 * torch.randn(B, 1, T * model.scale_factor, generator=gen)).clamp(-1, 1).to(DEV)
    cbs = _data_codebooks(model, x)
    return model, x, cbs


def _uncounted(model, x, stream=None):
    """The reference: the uncounted stream of the whole batch on [4, 4, 4], then finish and flush -> (z, index, y)."""
    s = model.new_stream(x.shape[0], max_chunk=N) if stream is None else stream
    z, idx, y = [], [], []
    with torch.no_grad():
        for chunk in _chunks(x, [N] * (T // N), model.scale_factor):
            z.append(streaming.encode_latents_stream(model, chunk, s))
            zq, index, _ = model.quantizer.quantize_bcl(z[-1], None, update_codebook=False, prioritize_early=False)
            idx.append(index)
            y.append(model.decode_stream(zq, s))
        s.finish()
        y.append(model.decode_flush(s))
    return torch.cat(z, dim=2), torch.cat(idx, dim=1), torch.cat(y, dim=2)


def _counted_chunk(x, at, step, sf):
    """(B, 1, N sf): row r holds its next step[r] frames, then NaN."""
    chunk = torch.full((x.shape[0], 1, N * sf), float("nan"), device=DEV)
    for r, c in enumerate(step):
        chunk[r, :, :c * sf] = x[r, :, at[r] * sf:(at[r] + c) * sf]
    return chunk


@pytest.fixture(scope="module")
def case():
    model, x, cbs = _model()
    return model, x, cbs, _uncounted(model, x)


def test_counted_schedules_equal_the_uncounted_stream(case):
    model, x, cbs, (z_ref, idx_ref, y_ref) = case
    sf = model.scale_factor
    s = model.new_stream(B, max_chunk=N)
    at = [0] * B
    z, idx, y = [[] for _ in range(B)], [[] for _ in range(B)], [[] for _ in range(B)]
    with torch.no_grad():
        for step in zip(*SCHEDULES):
            counts = torch.tensor(step, dtype=torch.int64, device=DEV)
            zc = streaming.encode_latents_stream(model, _counted_chunk(x, at, step, sf), s, counts)
            zq, index, _ = model.quantizer.quantize_bcl(zc, None, update_codebook=False, prioritize_early=False)
            zq = ops.mask_tail(zq, None, counts=counts)
            yc = model.decode_stream(zq, s, counts=counts)
            assert not torch.isnan(zc).any() and not torch.isnan(yc).any()
            for r, c in enumerate(step):
                assert float(zc[r, :, c:].abs().max() if c < N else 0.0) == 0.0          # behind the count: exact zeros
                assert float(zq[r, :, c:].abs().max() if c < N else 0.0) == 0.0
                assert float(yc[r, :, c * sf:].abs().max() if c < N else 0.0) == 0.0
                z[r].append(zc[r, :, :c]), idx[r].append(index[r, :c]), y[r].append(yc[r, :, :c * sf])
                at[r] += c
            assert s.positions() == {"enc_pos": at, "dec_pos": at, "end": [ops.STREAM_LIVE] * B}
        s.finish()
        tail = model.decode_flush(s)
    for r in range(B):
        zr, ir, yr = torch.cat(z[r], dim=1), torch.cat(idx[r], dim=0), torch.cat(y[r] + [tail[r]], dim=1)
        assert torch.equal(zr, z_ref[r]) and torch.equal(ir, idx_ref[r]) and torch.equal(yr, y_ref[r]), r
        assert torch.equal(ir.cpu(), rvq.residual_quantize(_frames(zr[None]), cbs)[1][0])  # the search, on the stream's own latents
    assert float(y_ref.abs().max()) > 1e-3


def test_forward_stream_with_counts_is_its_pieces(case):
    model, x, _, _ = case
    sf = model.scale_factor
    a, b = model.new_stream(B, max_chunk=N), model.new_stream(B, max_chunk=N)
    at = [0] * B
    with torch.no_grad():
        for step in list(zip(*SCHEDULES))[:3]:
            counts = torch.tensor(step, dtype=torch.int64, device=DEV)
            chunk = _counted_chunk(x, at, step, sf)
            y, _, index = model.forward_stream(chunk, a, counts=counts)
            zq, _, index_b = model.encode_stream(chunk, b, counts=counts)
            assert torch.equal(y, model.decode_stream(zq, b, counts=counts)) and torch.equal(index, index_b)
            for r, c in enumerate(step):
                assert float(zq[r, :, c:].abs().max() if c < N else 0.0) == 0.0
                at[r] += c
    assert a.positions() == b.positions()


def test_a_row_ends_flushes_and_restarts_alone(case):
    """Row 0 ends after its twelfth frame, is flushed and reset while rows 1 and 2 sit between steps, and runs a second clip; every
    clip equals its uncounted run, and rows 1 and 2 theirs."""
    model, x, _, (_, idx_ref, y_ref) = case
    sf = model.scale_factor
    x2 = (0.1 * torch.randn(1, 1, T * sf, generator=torch.Generator().manual_seed(77))).clamp(-1, 1).to(DEV)
    _, idx2_ref, y2_ref = _uncounted(model, x2)
    flush = model.new_stream(1, max_chunk=N).plan.flush_frames
    s = model.new_stream(B, max_chunk=N)
    clips = [x, torch.cat([x2, x[1:]], dim=0)]               # row 0 reads its second clip after the reset
    # (clip that row 0 reads, counts of the step); rows 1 and 2 take 12 frames over the whole run
    steps = [(0, [4, 2, 0]), (0, [4, 0, 4]), (0, [4, 3, 0]), "end row 0", (1, [4, 4, 4]), (1, [4, 3, 0]), (1, [4, 0, 4])]
    at = [0] * B
    idx, y = [[] for _ in range(B)], [[] for _ in range(B)]
    first = None
    with torch.no_grad():
        for item in steps:
            if item == "end row 0":
                assert at[0] == T
                s.finish(rows=[0])
                tail = model.decode_flush(s, rows=[0])
                assert float(tail[1:].abs().max()) == 0.0                                  # the other rows received nothing
                assert s.positions() == {"enc_pos": at, "dec_pos": [T + flush, at[1], at[2]],
                                         "end": [T, ops.STREAM_LIVE, ops.STREAM_LIVE]}
                first = (torch.cat(idx[0], dim=0), torch.cat(y[0] + [tail[0]], dim=1))
                s.reset(rows=[0])
                at[0], idx[0], y[0] = 0, [], []
                assert s.positions() == {"enc_pos": at, "dec_pos": at, "end": [ops.STREAM_LIVE] * B}
                continue
            clip, step = item
            counts = torch.tensor(step, dtype=torch.int64, device=DEV)
            yc, _, index = model.forward_stream(_counted_chunk(clips[clip], at, step, sf), s, counts=counts)
            for r, c in enumerate(step):
                idx[r].append(index[r, :c]), y[r].append(yc[r, :, :c * sf])
                at[r] += c
        assert at == [T, T, T]
        s.finish()
        tail = model.decode_flush(s)
    assert torch.equal(first[0], idx_ref[0]) and torch.equal(first[1], y_ref[0])
    assert torch.equal(torch.cat(idx[0], dim=0), idx2_ref[0]) and torch.equal(torch.cat(y[0] + [tail[0]], dim=1), y2_ref[0])
    for r in (1, 2):
        assert torch.equal(torch.cat(idx[r], dim=0), idx_ref[r]) and torch.equal(torch.cat(y[r] + [tail[r]], dim=1), y_ref[r]), r
    assert s.positions() == {"enc_pos": [T] * B, "dec_pos": [T + flush] * B, "end": [T] * B}


def test_a_graphed_counted_step_replays_with_changing_counts(case):
    """One captured ``forward_stream`` step with a counts tensor; ``counts.copy_`` between replays.  The kernels read the tensor, so
    the graph replays with whatever it holds."""
    model, x, _, _ = case
    sf = model.scale_factor
    steps = list(zip(*SCHEDULES))

    def run(step_fn, counts):
        at, outs = [0] * B, []
        for step in steps:
            counts.copy_(torch.tensor(step, dtype=torch.int64))
            y, commit, index = step_fn(_counted_chunk(x, at, step, sf))
            outs.append((y.clone(), commit.clone(), index.clone()))
            at = [a + c for a, c in zip(at, step)]
        return outs

    eager_stream, eager_counts = model.new_stream(B, max_chunk=N), torch.zeros(B, dtype=torch.int64, device=DEV)
    with torch.no_grad():
        eager = run(lambda c: model.forward_stream(c, eager_stream, counts=eager_counts), eager_counts)
    graph_stream, graph_counts = model.new_stream(B, max_chunk=N), torch.zeros(B, dtype=torch.int64, device=DEV)
    g = GraphedForward(lambda c: model.forward_stream(c, graph_stream, counts=graph_counts), torch.zeros(B, 1, N * sf, device=DEV))
    graph_stream.reset()
    graphed = run(g, graph_counts)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(graphed, eager)):
        assert all(torch.equal(u, v) for u, v in zip(a, b)), i
    assert graph_stream.positions() == eager_stream.positions()
    assert graph_stream.positions()["enc_pos"] == [T] * B
