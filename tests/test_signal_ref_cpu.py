"""``tests/signal_ref.py`` pinned on the CPU at ordinary shapes, against ``oracle/signal.py`` and scipy: the GPU edge tests
(``tests/test_gpu_signal_edges.py``) rest on these references, so they are checked here first."""
import math

import numpy as np
import pytest
import torch

from oracle import signal as osg
from tests import signal_ref as ref

FILTERS = [(24000, 11900.0, 0.707), (24000, 50.0, 0.707), (24000, 20.0, 0.707), (48000, 20.0, 5.0), (24000, 200.0, 10.0),
           (24000, 800.0, 0.707), (24000, 5000.0, 0.707), (24000, 11000.0, 0.707), (24000, 11500.0, 0.707)]


def _oracle_coeffs32(sr, cutoff, q):
    w0 = 2 * math.pi * cutoff / sr
    alpha = math.sin(w0) / 2 / q
    b0 = (1 - math.cos(w0)) / 2
    a0 = 1 + alpha
    return np.array([b0 / a0, 2 * b0 / a0, b0 / a0, -2 * math.cos(w0) / a0, (1 - alpha) / a0]).astype(np.float32)


@pytest.mark.parametrize("sr,cutoff,q", FILTERS)
def test_coefficients_are_the_oracles(sr, cutoff, q):
    """Q reaches the kernel as a float, and 0.707 is not one: at 800 and 5000 Hz that moves a2 by one float32 ulp against the
    oracle's, which keeps the double.  So: bit-equal for a Q that is a float32, within one ulp for the Q as written."""
    q32 = float(np.float32(q))
    assert np.array_equal(ref.biquad_coeffs32(sr, cutoff, q), ref.biquad_coeffs32(sr, cutoff, q32))
    assert np.array_equal(ref.biquad_coeffs32(sr, cutoff, q), _oracle_coeffs32(sr, cutoff, q32))
    c, o = ref.biquad_coeffs32(sr, cutoff, q), _oracle_coeffs32(sr, cutoff, q)
    assert np.all(np.abs(c.astype(np.float64) - o) <= np.spacing(np.abs(o)))


@pytest.mark.parametrize("sr,cutoff,q", [(24000, 5000.0, 0.707), (24000, 200.0, 10.0)])
def test_float32_sequential_is_the_oracles_recurrence(sr, cutoff, q):
    torch.manual_seed(0)
    x = 0.3 * torch.randn(3, 1500)
    x[2] *= 10.0                                                            # one row that clamps
    got = ref.biquad_f32_sequential(x.numpy(), ref.biquad_coeffs32(sr, cutoff, q))
    want = osg.lowpass_biquad(x, sr, cutoff, float(np.float32(q))).numpy()   # (the Q the kernel receives)
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_biquad_f64_is_lfilter_and_the_oracle_in_double():
    from scipy.signal import lfilter
    torch.manual_seed(1)
    x = (0.3 * torch.randn(2, 2000)).double()
    c = ref.biquad_coeffs32(24000, 800.0, 0.707).astype(np.float64)
    want = np.clip(lfilter(c[:3], [1.0, c[3], c[4]], x.numpy(), axis=-1), -1, 1)
    assert np.array_equal(ref.biquad_f64(x.numpy(), c), want)
    # the oracle run in float64 keeps the unrounded coefficients: equal to coefficient rounding, far below float32's own error
    orc = osg.lowpass_biquad(x, 24000, 800.0).numpy()
    assert np.abs(orc - want).max() < 1e-6
    # the float32 recurrence sits within float32 rounding of it
    seq = ref.biquad_f32_sequential(x.numpy(), c)
    assert np.abs(seq - want).max() < 2e-5 * np.abs(want).max()


def test_biquad_f64_clamps_the_output_only():
    c = ref.biquad_coeffs32(24000, 11000.0, 0.707)
    x = np.zeros((1, 50))
    x[0, 3], x[0, 4] = 4.0, -4.0
    y, raw = ref.biquad_f64(x, c), ref.biquad_f64(x, c, clamp=False)
    assert np.abs(raw).max() > 1.0 and np.abs(y).max() == 1.0
    inside = np.abs(raw) <= 1.0
    assert np.array_equal(y[inside], raw[inside])                           # the state behind a clamped sample is not clamped


@pytest.mark.parametrize("F,n_mels,T", [(257, 64, 50), (129, 40, 7)])
def test_melpower_is_the_oracles_matmul_and_its_autograd(F, n_mels, T):
    Fp = -(-F // 8) * 8
    torch.manual_seed(F)
    cv = torch.randn(2, 2 * Fp, T, dtype=torch.float64)
    fb = osg.mel_fbanks(F, 24000, n_mels).double()
    dmel = torch.randn(2, n_mels, T, dtype=torch.float64)
    cvg = cv.clone().requires_grad_(True)
    power = cvg[:, :F] ** 2 + cvg[:, Fp:Fp + F] ** 2
    want = torch.matmul(power.transpose(1, 2), fb).transpose(1, 2)          # oracle.signal.mel_spectrogram's last line
    want.backward(dmel)
    got, absum = ref.melpower_f64(cv.numpy(), fb.numpy(), F, Fp, return_abs=True)
    assert np.abs(got - want.detach().numpy()).max() <= 1e-12 * np.abs(got).max()
    assert np.all(absum >= np.abs(got) - 1e-12)
    dgot, dabs = ref.melpower_bwd_f64(cv.numpy(), fb.numpy(), dmel.numpy(), F, Fp, return_abs=True)
    assert np.abs(dgot - cvg.grad.numpy()).max() <= 1e-12 * np.abs(dgot).max()
    assert np.all(dgot[:, F:Fp] == 0) and np.all(dgot[:, Fp + F:] == 0) and np.all(dabs >= np.abs(dgot) - 1e-12)


@pytest.mark.parametrize("window", [32, 256])
def test_stft_f64_feeds_the_oracles_mel_spectrogram(window):
    torch.manual_seed(window)
    x = torch.randn(2, 3000, dtype=torch.float64)
    n_fft, hop = max(window, 512), window // 4
    st, w = ref.stft_f64(x, n_fft, hop, window, hann=True, onesided=True)
    cv = torch.cat([st.real, st.imag], dim=1).numpy() / math.sqrt(float((w * w).sum()))
    F = n_fft // 2 + 1
    got = ref.melpower_f64(cv, osg.mel_fbanks(F, 24000, 64).numpy(), F, F)
    want = osg.mel_spectrogram(x, 24000, window).numpy()
    assert got.shape == want.shape == (2, 64, 1 + 3000 // hop)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


def test_stft_f64_two_sided_rectangular_is_the_dft_of_the_reflected_frames():
    x = torch.arange(100, dtype=torch.float64).reshape(1, 100) / 100
    st, _ = ref.stft_f64(x, 64, 16, hann=False, onesided=False)
    xp = torch.nn.functional.pad(x[:, None], (32, 32), mode="reflect")[:, 0]
    want = torch.fft.fft(xp.unfold(-1, 64, 16), dim=-1).transpose(1, 2)
    assert st.shape == (1, 64, 7) and float((st - want).abs().max()) < 1e-10


@pytest.mark.parametrize("orig,new,length", [(48000, 24000, 500), (44100, 24000, 700), (16000, 24000, 333), (24000, 16000, 100),
                                              (8000, 24000, 7), (44100, 48000, 5)])
def test_resample_f64_is_the_oracles_conv(orig, new, length):
    torch.manual_seed(length)
    x = torch.randn(2, length)
    table, width, of, nf = osg.resample_kernel(orig, new)
    got, absum = ref.resample_f64(x.numpy(), table.numpy(), of, nf, width, return_abs=True)
    want = osg.resample(x, orig, new).numpy()
    assert got.shape == want.shape == (2, math.ceil(nf * length / of))
    assert np.all(np.abs(got - want) <= ref.dot_bound(table.shape[1], absum) + 1e-30)
    imp = np.zeros((1, length))
    imp[0, -1] = 1.0                                                        # an impulse reads the table back
    y = ref.resample_f64(imp, table.numpy(), of, nf, width)
    n, p = divmod(y.shape[1] - 1, nf)
    assert y[0, -1] == float(table[p, length - 1 - (n * of - width)])


def test_preemphasis_f64_is_the_oracle_and_its_transpose():
    torch.manual_seed(5)
    x = torch.randn(3, 300, dtype=torch.float64, requires_grad=True)
    c = float(np.float32(0.97))
    y = osg.preemphasis(x, c)
    dy = torch.randn_like(y)
    y.backward(dy)
    got, bound = ref.preemphasis_f64(x.detach().numpy(), 0.97, return_bound=True)
    assert np.abs(got - y.detach().numpy()).max() < 1e-15 and np.all(bound >= 2.0 ** -23 * np.abs(x.detach().numpy()))
    assert np.abs(ref.preemphasis_f64(dy.numpy(), 0.97, adjoint=True) - x.grad.numpy()).max() < 1e-15
