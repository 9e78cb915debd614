"""Float64 references for the training-loop signal ops (``csrc/spectral.hip``) -- CPU only, numpy / scipy / torch.

Plain restatements of each operation in double precision; nothing here imports the package under test.
``tests/test_signal_ref_cpu.py`` pins them against ``oracle/signal.py`` and scipy, ``tests/test_gpu_signal_edges.py``
measures the kernels against them.

Error bounds the GPU tests take from here are derived from the reference's own sums, not tuned:

* a float32 dot product of n terms, accumulated in any order with or without FMA, is within ``n * u * sum|terms|`` of the
  exact sum (u = 2^-24, first order); ``dot_bound`` allows 4 x that, which also covers the one or two roundings that
  form each term (the power re^2 + im^2, the factor 2 cv of the mel backward);
* pre-emphasis is one product and one subtraction: ``2^-23 (|x[n]| + |c x[n +- 1]|)`` covers both the separately rounded
  and the FMA-contracted form.
"""
from __future__ import annotations

import math

import numpy as np
import torch

U32 = 2.0 ** -24          # unit roundoff of float32


def dot_bound(n_terms: int, abs_sum):
    """|float32 dot product - exact| <= 4 n u sum|terms| (see the module docstring)."""
    return 4.0 * n_terms * U32 * abs_sum


# ------------------------------------------------------------------ low-pass biquad
def biquad_coeffs32(sample_rate, cutoff, q=0.707) -> np.ndarray:
    """RBJ low-pass coefficients (b0, b1, b2, a1, a2) / a0, computed in double and rounded to float32 -- what the kernel's
    host code and ``oracle.signal.lowpass_biquad`` both run with.  The C ABI takes sample rate, cut-off and Q as floats, so
    they pass through float32 first (0.707 is not a float32; the oracle keeps the double -- the two agree to the last bit
    on every filter the tests use, ``test_signal_ref_cpu.py`` checks that)."""
    sample_rate, cutoff, q = (float(np.float32(v)) for v in (sample_rate, cutoff, q))
    w0 = 2.0 * math.pi * cutoff / sample_rate
    alpha = math.sin(w0) / 2.0 / q
    b0, b1, b2 = (1 - math.cos(w0)) / 2, 1 - math.cos(w0), (1 - math.cos(w0)) / 2
    a0, a1, a2 = 1 + alpha, -2 * math.cos(w0), 1 - alpha
    return np.array([b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0]).astype(np.float32)


def biquad_f64(x, coeffs32, clamp: bool = True) -> np.ndarray:
    """``scipy.signal.lfilter`` in float64 along the last axis with the float32-rounded coefficients, clamped to +-1
    (``lfilter(clamp=True)``: the clamp is on the output, never on the feedback state)."""
    from scipy.signal import lfilter
    c = np.asarray(coeffs32, dtype=np.float32).astype(np.float64)
    y = lfilter(c[:3], np.array([1.0, c[3], c[4]]), np.asarray(x, dtype=np.float64), axis=-1)
    return np.clip(y, -1.0, 1.0) if clamp else y


def biquad_f32_sequential(x, coeffs32) -> np.ndarray:
    """The recurrence of ``oracle.signal.lowpass_biquad`` -- direct form I, every product and sum rounded to float32, left to
    right, one sample after the other: the definition in float32 that the kernel's error is measured against."""
    b0, b1, b2, a1, a2 = (np.float32(v) for v in np.asarray(coeffs32, dtype=np.float32))
    xs = np.asarray(x, dtype=np.float32)
    rows = xs.reshape(-1, xs.shape[-1])
    y = np.zeros_like(rows)
    x1 = x2 = y1 = y2 = np.zeros(rows.shape[0], dtype=np.float32)
    for n in range(rows.shape[1]):
        xn = rows[:, n]
        yn = b0 * xn + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        y[:, n] = yn
        x2, x1, y2, y1 = x1, xn, y1, yn
    return np.clip(y, np.float32(-1.0), np.float32(1.0)).reshape(xs.shape)


# ------------------------------------------------------------------ mel / power on the channel-major spectrum
def _halves(cv, F, Fp):
    cv = np.asarray(cv, dtype=np.float64)
    assert cv.shape[1] == 2 * Fp
    return cv[:, :F], cv[:, Fp:Fp + F]


def melpower_f64(cv, fb, F, Fp, return_abs: bool = False):
    """mel[b, m, t] = sum_f fb[f, m] (re[b, f, t]^2 + im[b, f, t]^2) on cv (B, 2 Fp, T): rows [0, F) real, [Fp, Fp + F)
    imaginary, the rows F <= f < Fp of each half are padding and take no part.  With ``return_abs`` also sum_f |fb| pw."""
    re, im = _halves(cv, F, Fp)
    fb = np.asarray(fb, dtype=np.float64)
    pw = re * re + im * im
    mel = np.einsum("bft,fm->bmt", pw, fb)
    return (mel, np.einsum("bft,fm->bmt", pw, np.abs(fb))) if return_abs else mel


def melpower_bwd_f64(cv, fb, dmel, F, Fp, return_abs: bool = False):
    """dcv[b, c, f, t] = 2 cv[b, c, f, t] sum_m fb[f, m] dmel[b, m, t] for both halves c, zeros in the padding rows.
    With ``return_abs`` also 2 |cv| sum_m |fb dmel|."""
    cv = np.asarray(cv, dtype=np.float64)
    fb, dmel = np.asarray(fb, dtype=np.float64), np.asarray(dmel, dtype=np.float64)
    g = np.einsum("fm,bmt->bft", fb, dmel)
    ga = np.einsum("fm,bmt->bft", np.abs(fb), np.abs(dmel))
    dcv, absum = np.zeros_like(cv), np.zeros_like(cv)
    for h in (0, Fp):
        dcv[:, h:h + F] = 2.0 * cv[:, h:h + F] * g
        absum[:, h:h + F] = 2.0 * np.abs(cv[:, h:h + F]) * ga
    return (dcv, absum) if return_abs else dcv


# ------------------------------------------------------------------ framed DFT
def stft_f64(x, n_fft, hop, win_length=None, hann: bool = True, onesided: bool = True):
    """``torch.stft`` in float64, centred and reflect-padded, unnormalised: (B, L) -> complex (B, F, T).  Differentiable
    (the gradient references are autograd through it).  Returns (spectrum, window)."""
    win_length = n_fft if win_length is None else win_length
    w = (torch.hann_window(win_length, periodic=True, dtype=torch.float64) if hann
         else torch.ones(win_length, dtype=torch.float64))
    st = torch.stft(x.double(), n_fft, hop, win_length, window=w, center=True, pad_mode="reflect", normalized=False,
                    onesided=onesided, return_complex=True)
    return st, w


# ------------------------------------------------------------------ resampler
def resample_out_len(length, of, nf):
    return -(-nf * length // of)


def resample_f64(x, table32, of, nf, width, return_abs: bool = False):
    """The direct double sum y[n nf + p] = sum_k table[p][k] xpad[n of + k], xpad = x with ``width`` zeros in front (and zeros
    behind), cropped to ceil(nf L / of) samples; x (rows, L), table (nf, K = 2 width + of) as the module holds it (float32).
    With ``return_abs`` also sum_k |table xpad|."""
    x = np.asarray(x, dtype=np.float64)
    tab = np.asarray(table32, dtype=np.float32).astype(np.float64)
    rows, length = x.shape
    K = tab.shape[1]
    assert tab.shape == (nf, 2 * width + of)
    out_len = resample_out_len(length, of, nf)
    frames = -(-out_len // nf)
    xpad = np.zeros((rows, (frames - 1) * of + K))
    stop = min(xpad.shape[1], width + length)
    xpad[:, width:stop] = x[:, :stop - width]
    y, ya = np.zeros((rows, frames * nf)), np.zeros((rows, frames * nf))
    for n in range(frames):
        seg = xpad[:, n * of:n * of + K]                                  # (rows, K)
        y[:, n * nf:(n + 1) * nf] = seg @ tab.T
        ya[:, n * nf:(n + 1) * nf] = np.abs(seg) @ np.abs(tab).T
    return (y[:, :out_len], ya[:, :out_len]) if return_abs else y[:, :out_len]


# ------------------------------------------------------------------ pre-emphasis
def preemphasis_f64(x, coeff, adjoint: bool = False, return_bound: bool = False):
    """y[n] = x[n] - c x[n - 1] (adjoint: x[n] - c x[n + 1]) with c rounded to float32 as the kernel receives it.
    With ``return_bound`` also 2^-23 (|x[n]| + |c x[n +- 1]|)."""
    x = np.asarray(x, dtype=np.float64)
    c = float(np.float32(coeff))
    nb = np.zeros_like(x)
    if adjoint:
        nb[..., :-1] = x[..., 1:]
    else:
        nb[..., 1:] = x[..., :-1]
    y = x - c * nb
    return (y, 2.0 ** -23 * (np.abs(x) + np.abs(c * nb))) if return_bound else y
