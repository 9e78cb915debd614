"""Time-folded long-clip inference on the GPU: the two copy kernels against torch indexing, and ``encode_long`` /
``decode_long`` / ``forward_long`` against the plain calls and the CPU oracle.

Bit-identity of folded vs plain is REPORTED (printed), not required: the conv selector chooses by shape and a folded
launch has a different (B, L).  Required, with the yardsticks of tests/test_gpu_fullclip_oracle.py:
  latents   per-frame relative difference folded vs plain < LATENT_REL_TOL;
  indices   equal, or every first disagreement proved a near tie from the two measured latents (oracle/neartie.py); and
            bit-exact against oracle.rvq.residual_quantize on the folded path's own latents;
  waveform  RMS folded vs plain < WAVE_RMS_TOL on every clip whose indices agree -- at least one such clip per case;
            ``decode_long`` alone on identical ``zq``: every clip.
"""
import pytest
import torch

from audio_generation_amd import longform, ops
from audio_generation_amd._lib import AgxError
from audio_generation_amd.graph import GraphedForward
from audio_generation_amd.vae import CausalVQAE
from oracle import codec, neartie, rvq
from tests.helpers import rms

pytestmark = pytest.mark.gpu
DEV = "cuda"
LATENT_REL_TOL = 2e-5           # tests/test_gpu_fullclip_oracle.py: two fp32 evaluations of a 30-conv stack
WAVE_RMS_TOL = 1e-4             # north_star: reconstructed waveform within 1e-4 RMS


# ------------------------------------------------------------------------------------------------ kernels
def _fold_ref(x, windows, hop, width, off):
    return torch.stack([x[:, :, off + s * hop: off + s * hop + width] for s in range(windows)], dim=1).reshape(
        x.shape[0] * windows, x.shape[1], width)


@pytest.mark.parametrize("c", [1, 2, 512])
def test_time_fold_and_unfold_equal_torch_indexing(c):
    gen = torch.Generator().manual_seed(c)
    long_rows = c <= 2
    cases = [  # (B, L, S, hop, W, src_off)
        (1, 40013, 5, 7001, 9007, 0), (3, 40013, 4, 6400, 12800, 3), (2, 5001, 1, 0, 4097, 901), (2, 5001, 3, 1, 4999, 0),
    ] if long_rows else [
        (1, 225, 6, 32, 54, 0), (2, 101, 4, 17, 33, 5), (3, 67, 1, 0, 29, 38), (2, 64, 3, 8, 48, 0),
    ]
    for b, length, s, hop, w, off in cases:
        x = torch.randn(b, c, length, generator=gen).to(DEV)
        got = ops.time_fold(x, s, hop, w, off)
        assert got.shape == (b * s, c, w) and torch.equal(got, _fold_ref(x, s, hop, w, off)), (b, length, s, hop, w, off)
        # unfold: all windows at an odd crop, then window 0 alone, then a tail with S = 1 -- into one poisoned tensor
        keep = hop if hop else w - 2
        src_off, dst_off = min((w - keep) // 2 + 1, w - keep), 3
        out_len = dst_off + s * keep + 11
        out = torch.full((b, c, out_len), float("nan"), device=DEV)
        want = out.clone()
        ops.time_unfold(got, out, s, keep, src_off, dst_off)
        g4 = got.reshape(b, s, c, w)
        for i in range(s):
            want[:, :, dst_off + i * keep: dst_off + (i + 1) * keep] = g4[:, i, :, src_off:src_off + keep]
        ops.time_unfold(got, out, s, 3, 0, 0, n_win=1)                         # window 0's own start
        want[:, :, :3] = g4[:, 0, :, :3]
        tail = torch.randn(b, c, 23, generator=gen).to(DEV)
        ops.time_unfold(tail, out, 1, 11, 12, out_len - 11)                    # the separately run tail
        want[:, :, out_len - 11:] = tail[:, :, 12:]
        assert not torch.isnan(out).any(), (b, length, s, hop, w, off)
        assert torch.equal(out, want), (b, length, s, hop, w, off)


def test_time_fold_wrappers_refuse_what_leaves_the_tensors():
    x = torch.zeros(2, 2, 100, device=DEV)
    ops.time_fold(x, 3, 30, 40)                                                  # last window ends at 100: fine
    for args in ((3, 30, 41), (3, 31, 40), (1, 0, 100, 1), (0, 1, 1), (1, 0, 0)):
        with pytest.raises(AgxError):
            ops.time_fold(x, *args)
    with pytest.raises(AgxError):
        ops.time_fold(x.cpu(), 1, 0, 10)
    with pytest.raises(AgxError):
        ops.time_fold(x.double(), 1, 0, 10)
    with pytest.raises(AgxError):
        ops.time_fold(x.transpose(1, 2), 1, 0, 2)
    w = torch.zeros(6, 2, 40, device=DEV)
    out = torch.zeros(2, 2, 100, device=DEV)
    ops.time_unfold(w, out, 3, 30, 10, 10)
    for kw in (dict(keep=31, src_off=10, dst_off=0), dict(keep=30, src_off=0, dst_off=11), dict(keep=30, n_win=4),
               dict(keep=0), dict(keep=10, src_off=-1)):
        with pytest.raises(AgxError):
            ops.time_unfold(w, out, 3, **kw)
    with pytest.raises(AgxError):
        ops.time_unfold(w, out, 2, 10)                                            # 6 rows are not 2 windows x 2 clips


# ------------------------------------------------------------------------------------------------ model
def _config_s(n_clips, length, seed=1234):
    torch.manual_seed(0)
    model = CausalVQAE(in_channels=1, n_blocks=4, strides=(2, 4, 5, 8), num_quantizers=8, codebook_size=1024,
                       codebook_dim=512, input_format="n c l", wavelet_decoders=False).eval().to(DEV)
    spec = codec.CodecSpec(in_channels=1, n_blocks=4, strides=(2, 4, 5, 8), codebook_dim=512,
                           wavelet_decoders=False, input_format="n c l")
    gen = torch.Generator().manual_seed(seed)
    x = (0.1 * torch.randn(n_clips, 1, length, generator=gen)).clamp(-1, 1)      # SURVEY 8(d) inputs, seeded as the full-clip test
    return model, spec, x


def _data_codebooks(model, x_dev):
    with torch.no_grad():
        model.quantizer.init_from_latents(model._run_encoders(model.rearrange_in(x_dev))[:2])
    return model.quantizer.codebooks.detach().cpu().clone()


def _frames(z):
    """(B, D, T) device latents -> (B, T, D) host frames."""
    return z.cpu().transpose(1, 2).contiguous()


def _check_folded_against_plain(model, x_dev, seg, cbs, what):
    """The three exactness statements of the module docstring + shapes, dtypes and run-to-run identity."""
    with torch.no_grad():
        y_p, commit_p, idx_p = model(x_dev)
        z_p = model._run_encoders(model.rearrange_in(x_dev))
        zq_p = model.encode(x_dev)[0]
        y_f, commit_f, idx_f = model.forward_long(x_dev, segment_frames=seg)
        y_f2, commit_f2, idx_f2 = model.forward_long(x_dev, segment_frames=seg)
        z_f = longform.encode_latents_long(model, model.rearrange_in(x_dev), seg)
        yd_f, yd_p = model.decode_long(zq_p, segment_frames=seg), model.decode(zq_p)
    assert z_f is not None, "this segment length leaves a single window: nothing is folded"
    for a, b in ((y_f, y_p), (idx_f, idx_p), (commit_f, commit_p), (z_f, z_p), (yd_f, yd_p)):
        assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device
    assert torch.equal(y_f, y_f2) and torch.equal(idx_f, idx_f2) and torch.equal(commit_f, commit_f2)   # run to run
    b, t = idx_f.shape[:2]
    fz_f, fz_p = _frames(z_f), _frames(z_p)
    rep = neartie.explain_disagreements(fz_f.reshape(b * t, -1).numpy(), fz_p.reshape(b * t, -1).numpy(),
                                        idx_f.cpu().reshape(b * t, -1).numpy(), idx_p.cpu().reshape(b * t, -1).numpy(), cbs.numpy())
    clean = [i for i in range(b) if torch.equal(idx_f[i], idx_p[i])]
    wave = rms(y_f[clean].cpu(), y_p[clean].cpu()) if clean else float("nan")
    wave_dec = max(rms(yd_f[i].cpu(), yd_p[i].cpu()) for i in range(b))
    print(f"{what} segment_frames={seg}: bit-identical latents {torch.equal(z_f, z_p)}, indices {torch.equal(idx_f, idx_p)}, "
          f"waveform {torch.equal(y_f, y_p)}, decode_long on identical zq {torch.equal(yd_f, yd_p)}; "
          f"latent rel {rep['max_latent_error_relative']:.3e}, frames with a disagreement {rep['frames_with_a_disagreement']}, "
          f"clean clips {len(clean)}/{b}, waveform RMS {wave:.3e}, decode_long RMS {wave_dec:.3e}")
    assert rep["max_latent_error_relative"] < LATENT_REL_TOL, rep
    assert rep["proved"], rep
    idx_same = rvq.residual_quantize(fz_f, cbs)[1]
    assert torch.equal(idx_f.cpu(), idx_same)                     # the search itself, on the folded path's own latents
    assert clean, "no clip with fully equal indices: the waveform statement would be vacuous"
    assert wave < WAVE_RMS_TOL
    assert wave_dec < WAVE_RMS_TOL
    return rep


@pytest.mark.parametrize("n_clips,length,segments", [(1, 360000, (64, 100, 256)), (2, 72000, (32, 50, 100))])
def test_config_s_folded_against_plain(n_clips, length, segments):
    """training.py:488-500 pushes one clip of 360 000 samples, utils.py:238-259 one of 72 000.  256 / 100 leave a short tail."""
    model, spec, x = _config_s(n_clips, length)
    x_dev = x.to(DEV)
    cbs = _data_codebooks(model, x_dev)
    for seg in segments:
        _check_folded_against_plain(model, x_dev, seg, cbs, f"config S {n_clips} x {length}")


def test_config_s_folded_clip_against_the_whole_oracle_forward():
    """The obligations tests/test_gpu_fullclip_oracle.py::_check_against_oracle puts on the plain forward, on the folded one."""
    model, spec, x = _config_s(1, 72000)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    z_cpu = codec.encode_latents(x, sd, spec)
    model.quantizer.init_from_latents(z_cpu.transpose(1, 2).to(DEV))
    cbs = model.quantizer.codebooks.detach().cpu().clone()
    seg = 40
    with torch.no_grad():
        y, commit, index = model.forward_long(x.to(DEV), segment_frames=seg)
        z_gpu = longform.encode_latents_long(model, x.to(DEV), seg)
    assert z_gpu is not None
    b, t = index.shape[:2]
    assert index[..., 0].unique().numel() >= 64
    zq_cpu, idx_cpu, commit_cpu = rvq.residual_quantize(z_cpu, cbs)
    y_cpu = codec.decode_latents(zq_cpu, sd, spec)
    frames_gpu = _frames(z_gpu)
    zq_same, idx_same, commit_same = rvq.residual_quantize(frames_gpu, cbs)
    assert torch.equal(index.cpu(), idx_same)
    assert abs(float(commit) - float(commit_same)) < 1e-5 * max(1.0, float(commit_same))
    assert rms(y.cpu(), codec.decode_latents(zq_same, sd, spec)) < WAVE_RMS_TOL
    rep = neartie.explain_disagreements(frames_gpu.reshape(b * t, -1).numpy(), z_cpu.reshape(b * t, -1).numpy(),
                                        index.cpu().reshape(b * t, -1).numpy(), idx_cpu.reshape(b * t, -1).numpy(), cbs.numpy())
    print("folded clip vs oracle:", {k: rep[k] for k in ("agreement", "frames_with_a_disagreement", "max_margin_over_bound",
                                                         "max_latent_error_relative")})
    assert rep["max_latent_error_relative"] < LATENT_REL_TOL, rep
    assert rep["proved"], rep
    if rep["frames_with_a_disagreement"] == 0:
        assert rms(y.cpu(), y_cpu) < WAVE_RMS_TOL
        assert abs(float(commit) - float(commit_cpu)) < 1e-5 * max(1.0, float(commit_cpu))


def test_reference_default_wiring_with_wavelet_decoder_stereo_ragged_length():
    """vae.py:205-223 as it stands: strides 2,3,4,4,5 (480 samples per frame), the wavelet layer in the second decoder
    block, "b l c" input; stereo, and a clip length that is not a multiple of 480."""
    torch.manual_seed(0)
    model = CausalVQAE(in_channels=2).eval().to(DEV)
    length = 480 * 120 + 137
    gen = torch.Generator().manual_seed(1234)
    x_dev = (0.1 * torch.randn(2, length, 2, generator=gen)).clamp(-1, 1).to(DEV)
    cbs = _data_codebooks(model, x_dev)
    for seg in (24, 50):
        _check_folded_against_plain(model, x_dev, seg, cbs, f"reference default 2 x {length} x 2")


def test_a_segment_that_leaves_one_window_is_the_plain_call():
    model, spec, x = _config_s(2, 72000)
    x_dev = x.to(DEV)
    _data_codebooks(model, x_dev)
    with torch.no_grad():
        y_p, commit_p, idx_p = model(x_dev)
        zq_p = model.encode(x_dev)[0]
        for seg in (225, 210, 10 ** 6):
            y, commit, idx = model.forward_long(x_dev, segment_frames=seg)
            assert torch.equal(y, y_p) and torch.equal(idx, idx_p) and torch.equal(commit, commit_p), seg
            zq, _, idx_e = model.encode_long(x_dev, segment_frames=seg)
            assert torch.equal(zq, zq_p) and torch.equal(idx_e, idx_p), seg
            assert torch.equal(model.decode_long(zq_p, segment_frames=seg), model.decode(zq_p)), seg


def test_forward_long_replays_from_a_captured_graph():
    model, spec, x = _config_s(1, 72000)
    x_dev = x.to(DEV)
    _data_codebooks(model, x_dev)
    seg = 40
    with torch.no_grad():
        y, commit, idx = model.forward_long(x_dev, segment_frames=seg)
    g = GraphedForward(lambda t: model.forward_long(t, segment_frames=seg), x_dev)
    y_g, commit_g, idx_g = g(x_dev)
    torch.cuda.synchronize()
    assert torch.equal(y_g, y) and torch.equal(idx_g, idx) and torch.equal(commit_g, commit)
