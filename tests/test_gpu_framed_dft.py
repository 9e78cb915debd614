"""The discriminator STFT runs the framed DFT's kernels at one row of its geometry (spectral.hip: fdft_geom with
win_length = n_fft, hop = n_fft / 4, two-sided, rectangular window), so ``agx_stft_*`` and ``agx_fdft_*`` write the
same bytes: the weight images, the forward up to the STFT's (B, 2N, T) -> (B, 2, T, N) transpose, and the adjoint.

(64, 500): hop 16, so the adjoint conv has 16 rows -- the direct kernel, the one place the MFMA-or-direct choice goes the
other way.  (256, 1030): 17 frames, not a multiple of the 64-wide transpose tile, and a length the hop does not divide."""
import pytest
import torch

from audio_generation_amd import _lib, ops
from audio_generation_amd.ops import _ptr, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
BATCH = 2
CASES = [(64, 500), (256, 1030)]


def fdft_image(lib, n_fft, normalized, backward):
    hop = n_fft // 4
    n = lib.agx_fdft_packed_floats(n_fft, n_fft, hop, 0, backward)
    assert n > 0
    img = torch.empty(int(n), dtype=torch.float32, device=DEV)
    _lib.check(lib.agx_fdft_pack(n_fft, n_fft, hop, 0, 0, 1 if normalized else 0, backward, _ptr(img), _stream()),
               "agx_fdft_pack")
    return img


def fdft_workspace(lib, length, n_fft):
    n = lib.agx_fdft_workspace_bytes(BATCH, length, n_fft, n_fft // 4)
    assert n > 0
    return torch.empty(int(n) // 4, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("n_fft", [n for n, _ in CASES])
def test_stft_images_are_the_framed_dft_images(n_fft, normalized):
    lib = _lib.load()
    for backward, pack, name in ((0, lib.agx_stft_pack, "agx_stft_pack"), (1, lib.agx_stft_pack_bwd, "agx_stft_pack_bwd")):
        got = torch.empty(int(lib.agx_stft_packed_floats(n_fft)), dtype=torch.float32, device=DEV)
        _lib.check(pack(n_fft, int(normalized), _ptr(got), _stream()), name)
        want = fdft_image(lib, n_fft, normalized, backward)
        assert float(got.abs().max()) > 0
        assert got.shape == want.shape and torch.equal(got, want), (name, n_fft, normalized)


@pytest.mark.parametrize("n_fft,length", CASES)
def test_stft_forward_is_the_framed_dft_transposed(n_fft, length):
    lib = _lib.load()
    torch.manual_seed(n_fft)
    x = (0.3 * torch.randn(BATCH, length)).to(DEV)
    frames = int(lib.agx_fdft_frames(length, n_fft, n_fft // 4))
    cv = torch.empty(BATCH, 2 * n_fft, frames, dtype=torch.float32, device=DEV)
    img, ws = fdft_image(lib, n_fft, True, 0), fdft_workspace(lib, length, n_fft)    # (_ptr keeps no tensor alive)
    _lib.check(lib.agx_fdft_forward(_ptr(x), _ptr(img), _ptr(cv), _ptr(ws), BATCH, length, n_fft, n_fft, n_fft // 4, 0,
                                    _stream()), "agx_fdft_forward")
    got = ops.stft(x, n_fft, True)
    assert got.shape == (BATCH, 2, frames, n_fft)
    assert float(got.abs().max()) > 0
    assert torch.equal(got, cv.view(BATCH, 2, n_fft, frames).permute(0, 1, 3, 2))


@pytest.mark.parametrize("n_fft,length", CASES)
def test_stft_backward_is_the_framed_dft_adjoint_of_the_untransposed_gradient(n_fft, length):
    lib = _lib.load()
    torch.manual_seed(n_fft + 1)
    frames = int(lib.agx_fdft_frames(length, n_fft, n_fft // 4))
    dy = torch.randn(BATCH, 2, frames, n_fft).to(DEV)
    dcv = dy.permute(0, 1, 3, 2).reshape(BATCH, 2 * n_fft, frames).contiguous()
    want = torch.empty(BATCH, length, dtype=torch.float32, device=DEV)
    img, ws = fdft_image(lib, n_fft, True, 1), fdft_workspace(lib, length, n_fft)    # (_ptr keeps no tensor alive)
    _lib.check(lib.agx_fdft_backward(_ptr(dcv), _ptr(img), _ptr(want), _ptr(ws), BATCH, length, n_fft, n_fft, n_fft // 4, 0,
                                     _stream()), "agx_fdft_backward")
    got = ops.stft_backward(dy, length, n_fft, True)
    assert float(got.abs().max()) > 0
    assert got.shape == want.shape and torch.equal(got, want)
