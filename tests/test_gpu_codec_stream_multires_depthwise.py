"""``CausalVQAE`` streaming with multires layers and depthwise residual blocks (``new_stream(..., multires_layers=True,
depthwise_blocks=True)``) on the GPU against the plain calls, with the yardsticks of tests/test_gpu_codec_stream.py
(``_check_streamed_against_plain``: latents within LATENT_REL_TOL, indices equal or proved near ties and bit-exact against the
oracle's search on the stream's own latents, the waveform on the plain call's zq under WAVE_RMS_TOL per clip, exact zeros before
the delay and after the end, the schedules bit for bit).

Model A of that file -- 2 blocks, strides (2, 3), codebook_dim 16, 2 x 32 codes, 2 clips x 12 frames -- in three variants:
multires layers in every encoder and decoder block; depthwise residual blocks; both, with a wavelet block in the decoder.  The
per-channel k = 1 convs' biases are set to magnitude 0.5 .. 1, so that a padding column that saw the bias instead of 0 is far
outside every yardstick.  On the third variant: a captured step, a counted run against each row streamed alone, one wire round
and the reset of one row.
"""
import pytest
import torch

from audio_generation_amd import ops
from audio_generation_amd.graph import GraphedForward
from audio_generation_amd.vae import CausalResidualBlock1d, CausalVQAE
from tests.test_gpu_codec_stream import _check_streamed_against_plain, _chunks
from tests.test_gpu_longform import _data_codebooks

pytestmark = pytest.mark.gpu
DEV = "cuda"
FRAMES, MAX_CHUNK = 12, 5
SCHEDULES = ([5, 5, 2], [1] * 12, [2, 1, 3, 1, 5])
VARIANTS = {
    "multires": (dict(wavelet_decoders=False, multires_encoders=True, multires_decoders=True), dict(multires_layers=True)),
    "depthwise": (dict(wavelet_decoders=False, depthwise=True), dict(depthwise_blocks=True)),
    "all": (dict(wavelet_decoders=(True, False), multires_encoders=True, multires_decoders=True, depthwise=True),
            dict(wavelet_blocks=True, multires_layers=True, depthwise_blocks=True)),
}


class _Keyed(CausalVQAE):
    """The model with its streams made with the variant's keywords, so that the helpers of tests/test_gpu_codec_stream.py, which
    call ``model.new_stream(batch, max_chunk=)``, stream it."""
    stream_keywords = {}

    def new_stream(self, batch, max_chunk=4, device=None, **kw):
        return super().new_stream(batch, max_chunk, device, **{**self.stream_keywords, **kw})


def _model(which):
    torch.manual_seed(0)
    build, keywords = VARIANTS[which]
    model = _Keyed(in_channels=1, n_blocks=2, strides=(2, 3), codebook_dim=16, num_quantizers=2, codebook_size=32, input_format="n c l",
                   **build)
    model.stream_keywords = keywords
    gen = torch.Generator().manual_seed(99)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, CausalResidualBlock1d) and m.depthwise:
                b = m.conv1[0].conv.bias
                sign = torch.where(torch.randn(b.shape, generator=gen) > 0, 1.0, -1.0)
                b.copy_(sign * (0.5 + 0.5 * torch.rand(b.shape, generator=gen)))
    model = model.eval().to(DEV)
    x = (0.1 * torch.randn(2, 1, FRAMES * model.scale_factor, generator=torch.Generator().manual_seed(1234))).clamp(-1, 1)
    return model, x.to(DEV)


_CASES = {}


def _case(which):
    """(model, x, codebooks) per variant, built once; the tests make their own streams and change nothing of the model."""
    if which not in _CASES:
        model, x = _model(which)
        _CASES[which] = model, x, _data_codebooks(model, x)
    return _CASES[which]


@pytest.mark.parametrize("which", list(VARIANTS))
def test_streamed_against_plain(which):
    model, x, cbs = _case(which)
    with pytest.raises(NotImplementedError, match="multires|depthwise"):
        CausalVQAE.new_stream(model, 2)
    s = _check_streamed_against_plain(model, x, SCHEDULES, MAX_CHUNK, cbs, f"model A, {which}, 2 x 12 frames")
    kinds = {u.kind for u in (*s.plan.encoders, *s.plan.decoders)}
    assert {"multires": {"multires"}, "depthwise": {"resdw"}, "all": {"multires", "resdw", "wavelet"}}[which] <= kinds
    assert "res" not in kinds or which == "multires"


def test_a_graphed_step_replays_the_eager_steps():
    """One captured ``forward_stream`` step, replayed for every chunk, with ``reset(rows=[1])`` between two replays."""
    model, x, _ = _case("all")
    n = 2
    chunks = list(_chunks(x, [n] * (FRAMES // n), model.scale_factor))

    def run(step, stream):
        outs = []
        for i, c in enumerate(chunks):
            if i == 2:
                stream.reset(rows=[1])
            y, commit, index = step(c)
            outs.append((y.clone(), commit.clone(), index.clone()))
        return outs

    eager_stream = model.new_stream(2, max_chunk=n)
    with torch.no_grad():
        eager = run(lambda c: model.forward_stream(c, eager_stream), eager_stream)
    graph_stream = model.new_stream(2, max_chunk=n)
    g = GraphedForward(lambda c: model.forward_stream(c, graph_stream), chunks[0])
    graph_stream.reset()                                                     # the warm-up calls advanced it
    graphed = run(g, graph_stream)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(graphed, eager)):
        assert all(torch.equal(u, v) for u, v in zip(a, b)), i
    assert graph_stream.positions() == eager_stream.positions()
    assert float(eager[-1][0].abs().max()) > 0


def _alone(model, x_row, schedule, n):
    """One row streamed alone, uncounted: (index, y with the flushed tail)."""
    s = model.new_stream(1, max_chunk=n)
    idx, y = [], []
    with torch.no_grad():
        for chunk in _chunks(x_row, schedule, model.scale_factor):
            yc, _, index = model.forward_stream(chunk, s)
            idx.append(index), y.append(yc)
        s.finish()
        y.append(model.decode_flush(s))
    return torch.cat(idx, dim=1)[0], torch.cat(y, dim=2)[0]


def test_a_counted_run_equals_each_row_streamed_alone():
    """Row 0's clip has 10 frames: it takes 4, 4, 2, ends and is flushed alone.  Row 1 takes 4, pauses for two hops, and goes on.
    The chunk holds NaN behind every row's count."""
    model, x, _ = _case("all")
    sf, n = model.scale_factor, 4
    frames = [10, 12]
    want = [_alone(model, x[0:1, :, :10 * sf].contiguous(), [4, 4, 2], n), _alone(model, x[1:2], [4, 4, 4], n)]
    s = model.new_stream(2, max_chunk=n)
    flush = s.plan.flush_frames
    at, idx, y = [0, 0], [[], []], [[], []]
    with torch.no_grad():
        for step in ([4, 4], [4, 0], [2, 0], "end row 0", [0, 4], [0, 4]):
            if step == "end row 0":
                s.finish(rows=[0])
                state = [r.clone() for r in (*s.enc_rings, *s.dec_rings, *s.dec_hidden) if r is not None]
                tail = model.decode_flush(s, rows=[0])
                y[0].append(tail[0])
                assert float(tail[1].abs().max()) == 0.0
                after = [r for r in (*s.enc_rings, *s.dec_rings, *s.dec_hidden) if r is not None]
                assert all(torch.equal(a[1], b[1]) for a, b in zip(after, state))            # row 1: not one ring column changed
                assert s.positions() == {"enc_pos": at, "dec_pos": [10 + flush, at[1]], "end": [10, ops.STREAM_LIVE]}
                continue
            counts = torch.tensor(step, dtype=torch.int64, device=DEV)
            chunk = torch.full((2, 1, n * sf), float("nan"), device=DEV)
            for r, c in enumerate(step):
                chunk[r, :, :c * sf] = x[r, :, at[r] * sf:(at[r] + c) * sf]
            yc, _, index = model.forward_stream(chunk, s, counts=counts)
            assert not torch.isnan(yc).any()
            for r, c in enumerate(step):
                assert c == n or float(yc[r, :, c * sf:].abs().max()) == 0.0
                idx[r].append(index[r, :c]), y[r].append(yc[r, :, :c * sf])
                at[r] += c
        assert at == frames
        s.finish(rows=[1])
        y[1].append(model.decode_flush(s, rows=[1])[1])
    for r in range(2):
        assert torch.equal(torch.cat(idx[r], dim=0), want[r][0]) and torch.equal(torch.cat(y[r], dim=1), want[r][1]), r
    assert float(want[0][1].abs().max()) > 1e-3


def test_the_wire_reproduces_forward_stream():
    """``compress_stream`` -> ``decompress_stream`` on two streams against ``forward_stream`` on a third, then finish and flush."""
    model, x, _ = _case("all")
    schedule = [1, 3, 4, 2, 2]
    sender, receiver, direct = (model.new_stream(2, max_chunk=4) for _ in range(3))
    idx, y, idx_ref, y_ref = [], [], [], []
    with torch.no_grad():
        for chunk in _chunks(x, schedule, model.scale_factor):
            n = chunk.shape[2] // model.scale_factor
            packets, index = model.compress_stream(chunk, sender)
            yc, index_r = model.decompress_stream(packets, receiver, n)
            yd, _, index_d = model.forward_stream(chunk, direct)
            assert torch.equal(index, index_r)
            idx.append(index_r), y.append(yc), idx_ref.append(index_d), y_ref.append(yd)
        receiver.finish(), direct.finish()
        y.append(model.decode_flush(receiver)), y_ref.append(model.decode_flush(direct))
    assert torch.equal(torch.cat(idx, dim=1), torch.cat(idx_ref, dim=1))
    assert torch.equal(torch.cat(y, dim=2), torch.cat(y_ref, dim=2))
    assert float(torch.cat(y_ref, dim=2).abs().max()) > 1e-3


@pytest.mark.parametrize("which", list(VARIANTS))
def test_reset_of_one_row_restarts_it_while_the_other_continues(which):
    model, x, _ = _case(which)
    sf = model.scale_factor
    chunks = list(_chunks(x, [2] * 6, sf))
    with torch.no_grad():
        s = model.new_stream(2, max_chunk=2)
        straight = [model.forward_stream(c, s) for c in chunks]
        s = model.new_stream(2, max_chunk=2)
        first = [model.forward_stream(c, s) for c in chunks[:3]]
        s.reset(rows=[0])
        mixed = [torch.cat([chunks[i][0:1], chunks[3 + i][1:2]]) for i in range(3)]          # row 0 starts over, row 1 goes on
        second = [model.forward_stream(c, s) for c in mixed]
    assert s.positions()["enc_pos"] == [6, 12] and s.positions()["dec_pos"] == [6, 12]
    for i in range(3):
        for part in (0, 2):                                           # y and index
            assert torch.equal(first[i][part], straight[i][part])
            assert torch.equal(second[i][part][0], straight[i][part][0]), (i, part)
            assert torch.equal(second[i][part][1], straight[3 + i][part][1]), (i, part)
