"""The signal kernels of ``csrc/spectral.hip`` at their chunk, band, reflection and tap edges, against the float64 references
of ``tests/signal_ref.py`` (pinned on the CPU by ``tests/test_signal_ref_cpu.py``).

Inputs are structured -- impulses at named positions, a 0.5 step, a ramp, a sinusoid at the cut-off, one seeded noise row -- and
every call has at least two rows of different content, so a row-stride error shows.  Bounds are derived from the
reference's own sums (``signal_ref.dot_bound``, ``signal_ref.preemphasis_f64``) or are the project's existing figure for the
path (5e-5 of the reference's maximum for the framed DFT); none is tuned to what the kernels give.

Low-pass biquad.  ``biquad_kernel`` cuts a row into 64 chunks of Lc = ceil(L / 64) samples and carries each chunk's entry state
over the lanes.  Per row, with ``ref`` = ``biquad_f64`` (float64 ``lfilter`` on the SAME float32-rounded coefficients) and
``scale`` = max |ref|:

    err(kernel) <= FACTOR * err(float32 sequential) + 1e-6 * scale,        FACTOR = 4

The figure printed per row and tabulated below is ``err(kernel) / (err(float32 sequential) + 0.25e-6 * scale)`` -- the bound
is that figure <= FACTOR.

Measured on the MI355X, worst row of each case (rows: the impulses at the chunk edges, step, ramp, sinusoid at the cut-off,
noise), columns = row length L.  Parent commit (pass 1 and the 64-step carry in float32) -- 31 of the 77 cases over 4:

    rate  cut-off  Q            1      2      3     63     64     65    127    128    129   4033   4096
    24000   11900  0.707     0.07   0.37   0.60   2.62   2.62   8.19   8.40   8.40  29.97 220.91 220.91
    24000      50  0.707     0.09   0.17   0.19   2.35   2.18   4.47   7.46   4.73   4.88  48.17  48.17
    24000      20  0.707     0.10   0.12   0.11   1.28   7.55   4.90  11.41  11.48  26.36  17.90  33.58
    48000      20  5         0.07   0.22   0.30   4.57   2.72   9.82  34.39  15.66  12.57 306.21 306.20
    24000     200  10        0.15   0.27   0.27   3.63   3.55   3.98   5.05   5.05   5.83  24.16  28.37
    24000     800  0.707     0.17   0.16   0.16   1.21   1.21   2.54   3.38   2.53   2.26   0.93   0.87
    24000    5000  0.707     0.12   0.16   0.24   0.40   0.40   0.31   0.32   0.31   0.37   0.42   0.35

This commit (pass 1 and the carry in float64, the entry state rounded to float32 for the unchanged pass 2):

    rate  cut-off  Q            1      2      3     63     64     65    127    128    129   4033   4096
    24000   11900  0.707     0.07   0.37   0.28   0.14   0.14   0.24   0.23   0.23   0.34   1.17   1.17
    24000      50  0.707     0.09   0.17   0.19   0.13   0.12   0.30   0.22   0.27   0.19   1.02   1.02
    24000      20  0.707     0.10   0.12   0.11   0.11   0.23   0.29   0.38   0.11   0.32   0.32   0.94
    48000      20  5         0.07   0.22   0.27   0.10   0.08   0.09   0.11   0.19   0.19   0.16   0.97
    24000     200  10        0.15   0.27   0.27   0.27   0.27   0.27   0.27   0.34   0.34   1.18   0.98
    24000     800  0.707     0.17   0.16   0.16   0.26   0.22   0.62   0.53   0.40   0.55   0.95   0.84
    24000    5000  0.707     0.12   0.16   0.24   0.27   0.27   0.31   0.31   0.31   0.32   0.42   0.35

The slow filters at the lengths and inputs the carry error was predicted for (``test_biquad_slow_filters_on_short_rows``):
relative max error of the named row against float64, then the figure of that row and of the case's worst row.

    rate  cut-off  Q          L  row     float32 seq.   parent              this commit        worst row, parent -> this
    24000   11900  0.707   4033  step    1.0e-05        6.9e-04 ( 67.06)    1.2e-05 (1.17)     220.91 -> 1.17
    24000      50  0.707   4097  noise   4.2e-05        3.4e-04 (  7.99)    2.1e-05 (0.50)      36.89 -> 0.91
    24000      20  0.707   8000  noise   1.5e-04        9.0e-03 ( 58.26)    5.3e-05 (0.34)      58.26 -> 0.95
    48000      20  5       8000  noise   9.8e-04        1.0e-01 (103.38)    1.1e-04 (0.11)     121.82 -> 0.98
    24000     200  10      4096  noise   2.0e-05        5.9e-04 ( 28.37)    1.2e-05 (0.58)      28.37 -> 0.98
    24000   11000  0.707    777  3-sigma noise, clamped (two rows)          parent 0.98, 0.72   this 0.74, 0.57

The largest figure of the corrected kernel is 1.18, below 3, so FACTOR stays at the 4 the bound was set with (a CPU emulation
without FMA contraction had predicted <= 1.2 for a correct carry and >= 11 for the float32 one; the device gives 1.18 and up to
306).  Above the figure 1 the second pass's own float32 rounding is what remains.
"""
import math

import numpy as np
import pytest
import torch

from audio_generation_amd import _lib, ops, signal_ops as sg
from audio_generation_amd.ops import _ptr, _stream
from tests import signal_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR = 4.0


def _dev(a) -> torch.Tensor:
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV)


def _host(t) -> np.ndarray:
    return t.detach().cpu().numpy().astype(np.float64)


def _noise(shape, seed, sigma=0.3):
    return (sigma * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


# ------------------------------------------------------------------ low-pass biquad
HARD_FILTERS = [(24000, 11900.0, 0.707), (24000, 50.0, 0.707), (24000, 20.0, 0.707), (48000, 20.0, 5.0), (24000, 200.0, 10.0)]
EASY_FILTERS = [(24000, 800.0, 0.707), (24000, 5000.0, 0.707)]
BIQUAD_LENGTHS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 4033, 4096]
# the rows of the issue's table: the regime where the float32 carry lost 10 .. 100 x against the float32 recurrence
TABLE_CASES = [(24000, 11900.0, 0.707, 4033, "step"), (24000, 50.0, 0.707, 4097, "noise"), (24000, 20.0, 0.707, 8000, "noise"),
               (48000, 20.0, 5.0, 8000, "noise"), (24000, 200.0, 10.0, 4096, "noise")]


def chunk_edges(L):
    """Impulse positions: 0, L - 1 and both sides of a chunk boundary (k Lc - 1, k Lc) for k = 1 and the last non-empty lane."""
    Lc = (L + 63) // 64
    last = (L + Lc - 1) // Lc - 1
    pos = {0, L - 1}
    for k in (1, last):
        pos.update((k * Lc - 1, k * Lc))
    return sorted(p for p in pos if 0 <= p < L)


def biquad_rows(sr, cutoff, q, L, kinds=("impulses", "step", "ramp", "sine", "noise")):
    names, rows = [], []
    n = np.arange(L, dtype=np.float64)
    for kind in kinds:
        if kind == "impulses":
            for p in chunk_edges(L):
                r = np.zeros(L)
                r[p] = 0.9
                names.append(f"impulse@{p}")
                rows.append(r)
            continue
        r = {"step": lambda: np.full(L, 0.5),
             "ramp": lambda: np.linspace(-0.5, 0.5, L),
             "sine": lambda: 0.6 / max(q, 1.0) * np.cos(2 * math.pi * cutoff / sr * n),
             "noise": lambda: np.clip(_noise(L, seed=L + int(cutoff)), -1, 1)}[kind]()
        names.append(kind)
        rows.append(r)
    return names, np.stack(rows).astype(np.float32)


def check_biquad(sr, cutoff, q, x, names):
    c = ref.biquad_coeffs32(sr, cutoff, q)
    want = ref.biquad_f64(x, c)
    seq = ref.biquad_f32_sequential(x, c).astype(np.float64)
    got = _host(sg.lowpass_biquad(_dev(x), sr, cutoff, q))
    assert got.shape == want.shape
    bad = []
    for r, name in enumerate(names):
        scale = np.abs(want[r]).max()
        ek, es = np.abs(got[r] - want[r]).max(), np.abs(seq[r] - want[r]).max()
        ratio = ek / (es + 0.25e-6 * scale)
        print(f"BIQUAD {sr} {cutoff:g} {q:g} L={x.shape[1]} {name}: kernel {ek / scale:.2e} sequential {es / scale:.2e} "
              f"ratio {ratio:.2f}")
        if not ek <= FACTOR * es + 1e-6 * scale:
            bad.append((name, ek / scale, es / scale, ratio))
    assert not bad, bad
    return got, want


@pytest.mark.parametrize("L", BIQUAD_LENGTHS)
@pytest.mark.parametrize("sr,cutoff,q", HARD_FILTERS + EASY_FILTERS)
def test_biquad_chunk_edges(sr, cutoff, q, L):
    names, x = biquad_rows(sr, cutoff, q, L)
    check_biquad(sr, cutoff, q, x, names)


@pytest.mark.parametrize("sr,cutoff,q,L,kind", TABLE_CASES)
def test_biquad_slow_filters_on_short_rows(sr, cutoff, q, L, kind):
    """The filters whose impulse response is long against Lc, at the lengths and inputs the carry error was predicted for."""
    names, x = biquad_rows(sr, cutoff, q, L, kinds=(kind, "impulses"))
    check_biquad(sr, cutoff, q, x, names)


def test_biquad_clamps_the_output_not_the_state():
    L = 777
    x = np.stack([_noise(L, 1, sigma=3.0), _noise(L, 2, sigma=3.0)])
    c = ref.biquad_coeffs32(24000, 11000.0, 0.707)
    raw = ref.biquad_f64(x, c, clamp=False)
    assert np.all(np.abs(raw).max(axis=1) > 1.0)
    got, want = check_biquad(24000, 11000.0, 0.707, x, ["3-sigma noise a", "3-sigma noise b"])
    assert np.abs(got).max() <= 1.0
    over = np.abs(raw) > 1.0
    after = np.zeros_like(over)
    after[:, 1:] = over[:, :-1] & ~over[:, 1:]            # first unclamped sample behind a clamped stretch
    assert after.sum() > 20
    seq = ref.biquad_f32_sequential(x, c)
    tol = FACTOR * np.abs(seq - want).max(axis=1, keepdims=True) + 1e-6 * np.abs(want).max(axis=1, keepdims=True)
    assert np.all((np.abs(got - want) <= tol)[after])
    assert np.all(np.abs(got[over]) == 1.0)


# ------------------------------------------------------------------ mel / power, forward and backward
def _htk_bank(F, n_mels):
    return sg.melscale_fbanks(F, 24000, n_mels).numpy()


def _hand_bank():
    fb = np.zeros((17, 9), dtype=np.float32)
    fb[2:7, 0] = [0.5, -1.0, 0.75, -0.25, 1.0]             # negative entries
    fb[4:11, 1] = [0.25, 0.5, 0.75, 0.0, 0.75, 0.5, 0.25]  # a zero strictly inside the band (f = 7)
    fb[0, 2], fb[16, 2] = 0.5, -0.75                      # non-zero only at f = 0 and f = F - 1
    fb[8, 3] = 1.0
    fb[:, 4] = np.cos(np.arange(17) * 0.7) + 0.1           # dense and signed
    fb[16, 6] = 1.0                                       # (filter 5 is all zero)
    fb[0, 7] = 2.0
    return fb                                             # filter 8 = the whole second workgroup: all zero, band stays [F, 0)


MEL_BANKS = {"htk129x80": lambda: _htk_bank(129, 80), "htk33x37": lambda: _htk_bank(33, 37), "htk257x13": lambda: _htk_bank(257, 13),
             "htk257x20": lambda: _htk_bank(257, 20), "hand17x9": _hand_bank}
ZERO_FILTERS = {"htk129x80": [0, 1, 4, 7, 12], "htk33x37": [0, 1, 2, 3, 6, 7, 10, 13], "hand17x9": [5, 8]}


def _structured(shape, salt):
    """Distinct, signed values: sign by index parity, magnitude 0.5 + frac(i phi) (no two equal within a tensor)."""
    i = np.arange(int(np.prod(shape)), dtype=np.float64) + salt
    sign = np.where((i.astype(np.int64) // 3 + i.astype(np.int64)) % 2 == 0, 1.0, -1.0)
    return (sign * (0.5 + np.modf(i * 0.6180339887498949)[0])).reshape(shape).astype(np.float32)


def _mel_case(bank, T):
    fb = MEL_BANKS[bank]()
    F, n_mels = fb.shape
    Fp = -(-F // 8) * 8
    cv = _structured((2, 2, Fp, T), salt=F)
    cv[:, :, F:] = 1e3 * (1.0 + np.abs(cv[:, :, F:]))     # the padding rows: finite, non-zero, large enough to show if read
    return fb, F, Fp, n_mels, cv.reshape(2, 2 * Fp, T)


@pytest.mark.parametrize("T", [1, 255, 256, 257])
@pytest.mark.parametrize("bank", list(MEL_BANKS))
def test_melpower_bands(bank, T):
    fb, F, Fp, n_mels, cv = _mel_case(bank, T)
    assert sorted(np.flatnonzero(~fb.any(axis=0))) == ZERO_FILTERS.get(bank, [])
    want, absum = ref.melpower_f64(cv, fb, F, Fp, return_abs=True)
    cvd, fbd = _dev(cv), _dev(fb)
    mel = torch.full((2, n_mels, T), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().agx_melpower(_ptr(cvd), _ptr(fbd), _ptr(mel), 2, F, T, n_mels, _stream()), "agx_melpower")
    got = _host(mel)
    excess = np.abs(got - want) - ref.dot_bound(F, absum)
    assert np.all(excess <= 0), (float(excess.max()), np.argwhere(excess > 0)[:4].tolist())
    for m in ZERO_FILTERS.get(bank, []):
        assert np.all(got[:, m] == 0.0), m


@pytest.mark.parametrize("T", [1, 255, 256, 257])
@pytest.mark.parametrize("bank", list(MEL_BANKS))
def test_melpower_backward_bands(bank, T):
    fb, F, Fp, n_mels, cv = _mel_case(bank, T)
    dmel = _structured((2, n_mels, T), salt=7 * n_mels)
    want, absum = ref.melpower_bwd_f64(cv, fb, dmel, F, Fp, return_abs=True)
    cvd, fbd, dmd = _dev(cv), _dev(fb), _dev(dmel)
    dcv = torch.full((2, 2 * Fp, T), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().agx_melpower_backward(_ptr(cvd), _ptr(fbd), _ptr(dmd), _ptr(dcv), 2, F, T, n_mels, _stream()),
               "agx_melpower_backward")
    got = _host(dcv)
    excess = np.abs(got - want) - ref.dot_bound(n_mels, absum)
    assert np.all(excess <= 0), (float(excess.max()), np.argwhere(excess > 0)[:4].tolist())
    pad = got.reshape(2, 2, Fp, T)[:, :, F:]
    assert np.all(pad == 0.0)                               # exact zeros in the padding rows, whatever cv holds there


# ------------------------------------------------------------------ framed DFT: shortest rows, reflections that meet
def _dft_lengths(n_fft, hop):
    return [n_fft // 2 + 1, n_fft // 2 + 2, n_fft - 1, n_fft + hop - 1]


def _special_samples(L, n_fft):
    """The samples stft_unprep_kernel treats specially: both ends, their neighbours, and the last sample the left reflection reads."""
    return sorted({0, 1, n_fft // 2, L - 2, L - 1} & set(range(L)))


def _dft_rows(L, n_fft):
    rows = [np.linspace(-0.5, 0.5, L)]
    for k, p in enumerate(_special_samples(L, n_fft)):
        r = np.zeros(L)
        r[p] = 0.9 if k % 2 == 0 else -0.7
        rows.append(r)
    return np.stack(rows).astype(np.float32)


def _rows_close(got, want, tol, what, samples=()):
    """Per row: max error <= tol * that row's reference maximum; and the same at each named sample of the last axis, separately."""
    got, want = _host(got), _host(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    for r in range(want.shape[0]):
        scale = np.abs(want[r]).max()
        assert scale > 0, (what, r)
        err = np.abs(got[r] - want[r])
        assert err.max() <= tol * scale, (what, "row", r, float(err.max() / scale))
        for n in samples:
            assert err[..., n].max() <= tol * scale, (what, "row", r, "sample", n, float(err[..., n].max() / scale))


def _adjoint_identity(y, g, x, dx, what):
    """<fwd(x), g> = <x, bwd(g)> per row, inner products in float64, to 1e-5 relative."""
    y, g, x, dx = (_host(t) for t in (y, g, x, dx))
    for r in range(x.shape[0]):
        lhs, rhs = float(np.sum(y[r] * g[r])), float(np.sum(x[r] * dx[r]))
        assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (what, "row", r, lhs, rhs)


@pytest.mark.parametrize("n_fft", [64, 128])
@pytest.mark.parametrize("which", range(4))
def test_stft_shortest_rows(n_fft, which):
    """The discriminator STFT (two-sided, rectangular, hop n_fft / 4): forward, gradient, adjoint identity."""
    L = _dft_lengths(n_fft, n_fft // 4)[which]
    x = _dft_rows(L, n_fft)
    xr = torch.from_numpy(x).double().requires_grad_(True)
    st, _ = ref.stft_f64(xr, n_fft, n_fft // 4, hann=False, onesided=False)
    want = torch.stack([st.real, st.imag], dim=1).transpose(2, 3) / math.sqrt(n_fft)       # (B, 2, T, N)
    g = torch.from_numpy(_structured(tuple(want.shape), salt=L).astype(np.float64))
    (want * g).sum().backward()
    xd = _dev(x)
    got = ops.stft(xd, n_fft, normalized=True)
    assert got.shape == want.shape == (x.shape[0], 2, 1 + L // (n_fft // 4), n_fft)
    _rows_close(got, want, 5e-5, "stft forward")
    dx = ops.stft_backward(_dev(g.numpy()), L, n_fft, normalized=True)
    _rows_close(dx, xr.grad, 5e-5, "stft gradient", _special_samples(L, n_fft))
    # g that does not cancel against fwd(x): the spectrum itself plus the structured values
    g2 = (got + 0.25 * got.abs().amax(dim=(1, 2, 3), keepdim=True) * _dev(g.numpy())).contiguous()
    _adjoint_identity(got, g2, xd, ops.stft_backward(g2, L, n_fft, normalized=True), "stft adjoint")


MEL_FRONT_ENDS = [(512, 32, 8), (512, 96, 32), (400, 100, 25), (256, 256, 64)]     # hops 8 and 25: padded phase channels (Hc != H)


@pytest.mark.parametrize("n_fft,win,hop", MEL_FRONT_ENDS)
@pytest.mark.parametrize("which", range(4))
def test_mel_front_end_shortest_rows(n_fft, win, hop, which):
    """MelSpectrogram (one-sided, Hann, window energy normalisation): forward and gradient against torch.stft in float64 and
    autograd through it; the adjoint identity on its linear part, the framed DFT."""
    L = _dft_lengths(n_fft, hop)[which]
    n_mels = 20
    x = _dft_rows(L, n_fft)
    spec = sg.MelSpectrogram(24000, n_fft, win, hop, n_mels, True).to(DEV)
    xr = torch.from_numpy(x).double().requires_grad_(True)
    st, w = ref.stft_f64(xr, n_fft, hop, win, hann=True, onesided=True)
    want = torch.einsum("bft,fm->bmt", (st.real ** 2 + st.imag ** 2) / float((w * w).sum()), spec.fb.cpu().double())
    g = torch.from_numpy(_structured(tuple(want.shape), salt=L).astype(np.float64))
    (want * g).sum().backward()
    xd = _dev(x).requires_grad_(True)
    got = spec(xd)
    assert got.shape == want.shape == (x.shape[0], n_mels, 1 + L // hop)
    _rows_close(got, want, 5e-5, "mel forward")
    got.backward(_dev(g.numpy()))
    _rows_close(xd.grad, xr.grad, 5e-5, "mel gradient", _special_samples(L, n_fft))

    lib = _lib.load()
    B, T, rows = x.shape[0], 1 + L // hop, int(lib.agx_fdft_rows(n_fft, 1))
    xd = xd.detach()
    cv = torch.full((B, 2 * rows, T), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(lib.agx_fdft_forward(_ptr(xd), _ptr(spec._image(0, xd.device)), _ptr(cv), _ptr(spec._ws(B, L, xd.device)), B, L, n_fft,
                                    win, hop, 1, _stream()), "agx_fdft_forward")
    cvw = torch.cat([st.real, st.imag], dim=1).detach() / math.sqrt(float((w * w).sum()))
    F = n_fft // 2 + 1
    _rows_close(torch.cat([cv[:, :F], cv[:, rows:rows + F]], dim=1), cvw, 5e-5, "framed DFT forward")
    assert bool((cv[:, F:rows] == 0).all()) and bool((cv[:, rows + F:] == 0).all())
    g2 = (cv + 0.25 * cv.abs().amax(dim=(1, 2), keepdim=True) * _dev(_structured(tuple(cv.shape), salt=3))).contiguous()
    dx = torch.full((B, L), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(lib.agx_fdft_backward(_ptr(g2), _ptr(spec._image(1, xd.device)), _ptr(dx), _ptr(spec._ws(B, L, xd.device)), B, L,
                                     n_fft, win, hop, 1, _stream()), "agx_fdft_backward")
    _adjoint_identity(cv, g2, xd, dx, "framed DFT adjoint")


# ------------------------------------------------------------------ resampler: taps clipped at both ends
RATIOS = [(48000, 44100), (44100, 48000), (24000, 16000), (8000, 24000), (44100, 24000)]


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("orig,new", RATIOS)
def test_resample_clipped_taps(orig, new, which):
    mod = sg.Resample(orig, new).to(DEV)
    of, nf, width = mod.of, mod.nf, mod.width
    L = [1, 2, width - 1, width, width + of, 701][which]                           # 701: no multiple of any of > 1 here
    assert of == 1 or 701 % of
    table = mod.kernel.cpu().numpy()
    K = table.shape[1]
    assert table.shape == (nf, 2 * width + of)
    assert (4 * nf * K > 64 * 1024) == ((orig, new) in RATIOS[:2])                 # the two ratios whose table stays in global memory
    first, last = np.zeros(L), np.zeros(L)
    first[0], last[L - 1] = 1.0, 1.0
    x = np.stack([first, last, np.linspace(-1.0, 1.0, L) if L > 1 else np.array([0.75]), _noise(L, seed=L + of, sigma=1.0)])
    x = x.astype(np.float32)
    want, absum = ref.resample_f64(x, table, of, nf, width, return_abs=True)
    got = _host(mod(_dev(x)))
    assert got.shape == want.shape == (4, math.ceil(nf * L / of))
    excess = np.abs(got - want) - ref.dot_bound(K, absum)
    assert np.all(excess <= 0), (float(excess.max()), np.argwhere(excess > 0)[:4].tolist())
    # a unit impulse leaves one non-zero product per output sample: the table's own entries, exactly
    assert np.array_equal(got[:2], want[:2])
    assert np.abs(want[0]).max() > 0 and np.abs(want[1]).max() > 0


# ------------------------------------------------------------------ pre-emphasis and its adjoint
@pytest.mark.parametrize("adjoint", [0, 1])
@pytest.mark.parametrize("L", [1, 2, 255, 256, 257, 513])
def test_preemphasis_block_edges(L, adjoint):
    n = np.arange(L)
    x = np.stack([np.linspace(-1.0, 1.0, L) if L > 1 else np.array([0.625]), _noise(L, seed=L, sigma=1.0),
                  np.where(n % 256 >= 255, 0.9, -0.3) + 0.001 * n]).astype(np.float32)
    want, bound = ref.preemphasis_f64(x, 0.97, adjoint=bool(adjoint), return_bound=True)
    got = _host(sg._preemph_raw(_dev(x), 0.97, adjoint))
    assert got.shape == want.shape == (3, L)
    assert np.all(np.abs(got - want) <= bound), float((np.abs(got - want) - bound).max())
    edge = L - 1 if adjoint else 0
    assert np.array_equal(got[:, edge], x[:, edge].astype(np.float64))              # dx[L-1] = dy[L-1], y[0] = x[0]: exactly
