"""``CausalVQAE`` streaming (``new_stream`` / ``encode_stream`` / ``decode_stream`` / ``forward_stream`` / ``decode_flush``) on the
GPU against the plain calls, with the yardsticks of tests/test_gpu_longform.py:

  latents   per-frame relative difference streamed vs plain < LATENT_REL_TOL;
  indices   equal, or every first disagreement proved a near tie (oracle/neartie.py); and bit-exact against
            oracle.rvq.residual_quantize on the stream's own latents;
  waveform  ``decode_stream`` + ``decode_flush`` on the PLAIN call's zq, delay removed, vs ``model.decode(zq)``: RMS under
            WAVE_RMS_TOL on every clip (independent of the indices, so never vacuous);
  schedules bit-identical to one another; a ``GraphedForward`` step replays bit-identically to eager steps.
"""
import pytest
import torch

from audio_generation_amd import streaming
from audio_generation_amd.graph import GraphedForward
from audio_generation_amd.vae import CausalVQAE
from oracle import neartie, rvq
from tests.helpers import rms
from tests.test_gpu_longform import LATENT_REL_TOL, WAVE_RMS_TOL, _config_s, _data_codebooks, _frames

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _model_a():
    torch.manual_seed(0)
    model = CausalVQAE(in_channels=1, n_blocks=2, strides=(2, 3), codebook_dim=16, num_quantizers=2, codebook_size=32,
                       wavelet_decoders=False, input_format="n c l").eval().to(DEV)
    gen = torch.Generator().manual_seed(1234)
    x = (0.1 * torch.randn(2, 1, 12 * model.scale_factor, generator=gen)).clamp(-1, 1)
    return model, x


def _chunks(x_dev, schedule, per_frame):
    at = 0
    for n in schedule:
        yield x_dev[:, :, at * per_frame:(at + n) * per_frame].contiguous()
        at += n
    assert at * per_frame == x_dev.shape[2]


def _stream_forward(model, x_dev, schedule, max_chunk):
    """The pieces of ``forward_stream`` chunk by chunk (so that the latents are seen), then finish and flush."""
    s = model.new_stream(x_dev.shape[0], max_chunk=max_chunk)
    z, idx, y = [], [], []
    with torch.no_grad():
        for chunk in _chunks(x_dev, schedule, model.scale_factor):
            z.append(streaming.encode_latents_stream(model, chunk, s))
            zq, index, _ = model.quantizer.quantize_bcl(z[-1], None, update_codebook=False, prioritize_early=False)
            idx.append(index)
            y.append(model.decode_stream(zq, s))
        s.finish()
        y.append(model.decode_flush(s))
    return torch.cat(z, dim=2), torch.cat(idx, dim=1), torch.cat(y, dim=2), s


def _stream_decode(model, zq, schedule, max_chunk):
    s = model.new_stream(zq.shape[0], max_chunk=max_chunk)
    with torch.no_grad():
        y = [model.decode_stream(c, s) for c in _chunks(zq, schedule, 1)]
        s.finish()
        y.append(model.decode_flush(s))
    return torch.cat(y, dim=2), s.decoder_delay


def _check_streamed_against_plain(model, x_dev, schedules, max_chunk, cbs, what):
    sf = model.scale_factor
    b, t = x_dev.shape[0], x_dev.shape[2] // sf
    with torch.no_grad():
        z_p = model._run_encoders(model.rearrange_in(x_dev))
        zq_p, _, idx_p = model.encode(x_dev)
        y_p = model.decode(zq_p)
    runs = [_stream_forward(model, x_dev, sched, max_chunk) for sched in schedules]
    z_s, idx_s, y_s, s = runs[0]
    delay, flush = s.decoder_delay, s.plan.flush_frames
    assert z_s.shape == z_p.shape and idx_s.shape == idx_p.shape and y_s.shape == (b, 1, (t + flush) * sf)
    assert s.positions() == {"enc_pos": [t] * b, "dec_pos": [t + flush] * b, "end": [t] * b}
    for sched, (z, idx, y, _) in zip(schedules[1:], runs[1:]):                       # schedules: bit for bit
        assert torch.equal(z, z_s) and torch.equal(idx, idx_s) and torch.equal(y, y_s), sched
    fz_s, fz_p = _frames(z_s), _frames(z_p)
    rep = neartie.explain_disagreements(fz_s.reshape(b * t, -1).numpy(), fz_p.reshape(b * t, -1).numpy(),
                                        idx_s.cpu().reshape(b * t, -1).numpy(), idx_p.cpu().reshape(b * t, -1).numpy(), cbs.numpy())
    yd, _ = _stream_decode(model, zq_p, schedules[0], max_chunk)
    wave = [rms(yd[i, :, delay:delay + t * sf].cpu(), y_p[i].cpu()) for i in range(b)]
    print(f"{what}: bit-identical latents {torch.equal(z_s, z_p)}, indices {torch.equal(idx_s, idx_p)}; latent rel "
          f"{rep['max_latent_error_relative']:.3e}, frames with a disagreement {rep['frames_with_a_disagreement']}, "
          f"decode on the plain zq: RMS per clip {['%.3e' % w for w in wave]}, bit-identical "
          f"{torch.equal(yd[:, :, delay:delay + t * sf], y_p)}")
    assert rep["max_latent_error_relative"] < LATENT_REL_TOL, rep
    assert rep["proved"], rep
    assert torch.equal(idx_s.cpu(), rvq.residual_quantize(fz_s, cbs)[1])                # the search, on the stream's own latents
    assert all(w < WAVE_RMS_TOL for w in wave), wave
    assert float(yd[:, :, :delay].abs().max()) == 0.0                                   # before the start: the mask's exact zeros
    assert float(yd[:, :, delay + t * sf:].abs().max()) == 0.0                          # after the end
    assert float(y_p.abs().max()) > 1e-3                                                # the comparison is about a signal
    return s


def test_model_a_streamed_against_plain():
    model, x = _model_a()
    x_dev = x.to(DEV)
    cbs = _data_codebooks(model, x_dev)
    _check_streamed_against_plain(model, x_dev, ([5, 5, 2], [1] * 12, [2, 1, 3, 1, 5]), 5, cbs, "model A 2 x 12 frames")


def test_config_s_streamed_against_plain():
    model, spec, x = _config_s(2, 40 * 320)
    x_dev = x.to(DEV)
    cbs = _data_codebooks(model, x_dev)
    s = _check_streamed_against_plain(model, x_dev, ([4] * 10, [3] * 13 + [1]), 4, cbs, "config S 2 x 40 frames")
    assert s.decoder_delay == 370


def test_forward_stream_is_its_pieces():
    model, x = _model_a()
    x_dev = x.to(DEV)
    _data_codebooks(model, x_dev)
    _, idx_s, y_s, _ = _stream_forward(model, x_dev, [5, 5, 2], 5)
    s = model.new_stream(2, max_chunk=5)
    with torch.no_grad():
        outs = [model.forward_stream(c, s) for c in _chunks(x_dev, [5, 5, 2], model.scale_factor)]
        s.finish(rows=[0, 1])
        tail = model.decode_flush(s)
    assert torch.equal(torch.cat([o[0] for o in outs] + [tail], dim=2), y_s)
    assert torch.equal(torch.cat([o[2] for o in outs], dim=1), idx_s)
    assert all(o[1].shape == outs[0][1].shape for o in outs)


@pytest.mark.parametrize("which", ["A", "S"])
def test_a_graphed_step_replays_the_eager_steps(which):
    """One captured ``forward_stream`` step, replayed for every chunk, with ``reset(rows=[1])`` between two replays: the positions
    are device memory, so the graph neither knows nor cares where a row stands."""
    if which == "A":
        model, x = _model_a()
        n = 2
    else:
        model, _, x = _config_s(2, 12 * 320)
        n = 4
    x_dev = x.to(DEV)
    _data_codebooks(model, x_dev)
    chunks = list(_chunks(x_dev, [n] * (12 // n), model.scale_factor))

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
    assert graph_stream.positions()["enc_pos"] == [12, 12 - 2 * n]
