"""The discriminator STFT is one row of the framed DFT's geometry (spectral.hip: fdft_geom with win_length = n_fft,
hop = n_fft / 4, two-sided): every size the ``agx_stft_*`` queries answer is the ``agx_fdft_*`` answer at that row, plus
the STFT's own transpose buffer, and the STFT keeps its own, stricter refusals.  Host only: no kernel is launched."""
import pytest

from audio_generation_amd import _lib

N_FFTS = (64, 128, 256, 512, 1024, 2048)
BAD_SHAPE, UNSUPPORTED = -1, -5
NOT_A_POWER = b"stft: n_fft must be a power of two >= 64"
TOO_SHORT = b"stft: reflect padding needs length > n_fft / 2"


@pytest.fixture(scope="module")
def lib():
    from audio_generation_amd import build
    build.build()
    return _lib.load()


def lengths(n_fft):
    return [length for length in (n_fft // 2 + 1, 500, 4096, 72000) if length > n_fft // 2]


@pytest.mark.parametrize("n_fft", N_FFTS)
def test_stft_sizes_are_the_framed_dft_sizes(lib, n_fft):
    hop = n_fft // 4
    packed = lib.agx_stft_packed_floats(n_fft)
    assert packed > 0
    assert packed == lib.agx_fdft_packed_floats(n_fft, n_fft, hop, 0, 0) == lib.agx_fdft_packed_floats(n_fft, n_fft, hop, 0, 1)
    for length in lengths(n_fft):
        frames = lib.agx_stft_frames(length, n_fft)
        assert frames == lib.agx_fdft_frames(length, n_fft, hop) == 1 + length // hop, (n_fft, length)
        for batch in (1, 32):
            transposed = 4 * batch * 2 * n_fft * frames       # the (B, 2N, T) conv output, before the transpose
            assert lib.agx_stft_workspace_bytes(batch, length, n_fft) == \
                   lib.agx_fdft_workspace_bytes(batch, length, n_fft, hop) + transposed, (n_fft, length, batch)


@pytest.mark.parametrize("n_fft", [96, 32])
def test_stft_refuses_what_is_not_a_power_of_two_from_64(lib, n_fft):
    for query in (lambda: lib.agx_stft_frames(4096, n_fft), lambda: lib.agx_stft_packed_floats(n_fft),
                  lambda: lib.agx_stft_workspace_bytes(2, 4096, n_fft)):
        assert query() == UNSUPPORTED
        assert lib.agx_last_error() == NOT_A_POWER


@pytest.mark.parametrize("n_fft", N_FFTS)
def test_stft_refuses_a_signal_that_reflect_padding_cannot_extend(lib, n_fft):
    assert lib.agx_stft_frames(n_fft // 2, n_fft) == BAD_SHAPE
    assert lib.agx_last_error() == TOO_SHORT


def test_stft_workspace_refuses_an_empty_batch(lib):
    assert lib.agx_stft_workspace_bytes(0, 4096, 256) == BAD_SHAPE
    assert lib.agx_last_error() == b"stft: batch <= 0"


def test_fdft_size_queries_answer_from_the_shape_alone(lib):
    """agx_fdft_rows and agx_fdft_workspace_bytes are queries: they answer (bins rounded up to 8; hop rounded up to 16 channels,
    n_fft // hop taps) also where agx_fdft_pack / _forward would refuse the geometry."""
    assert [lib.agx_fdft_rows(n, one) for n, one in ((512, 1), (512, 0), (400, 1), (8, 1))] == [264, 512, 208, 8]
    assert lib.agx_fdft_workspace_bytes(32, 72000, 512, 8) == 4 * 32 * 16 * (9001 + 63)
    assert lib.agx_fdft_workspace_bytes(2, 3000, 400, 30) == 4 * 2 * 32 * (101 + 12)
    assert lib.agx_fdft_packed_floats(400, 400, 30, 1, 0) == -1
