"""LayerNorm over the channels of (B, C, T): every kernel ``agx_layernorm_ct`` can pick, on both sides of every threshold, on
inputs that separate a centred variance from an uncentred one -- and ``agx_layernorm_ct_backward`` at the same widths.

The dispatch has no name query.  As read from ``agx_layernorm_ct`` (audio_generation_amd/csrc/attention.hip:571-591):

    C <=   64   layernorm_ct_regs_kernel< 4,16>      C <=  512   layernorm_ct_regs_kernel<16,32>
    C <=  128   layernorm_ct_regs_kernel< 8,16>      C <= 1024   layernorm_ct_regs_kernel<32,32>
    C <=  256   layernorm_ct_regs_kernel< 8,32>      C <= 2048   layernorm_ct_regs_kernel<64,32>
    C >  2048   layernorm_ct_kernel (three passes over memory)

(``<CPT,NG>``: a thread holds CPT channels c = g + NG k; its ``c < C`` masks are live when C < CPT * NG; one workgroup takes 16
columns, the three-pass kernel and the backward (attention.hip:259-314, one kernel for every C) take 64.)  A change to that
dispatch needs a change to ``KERNEL_OF`` and to ``attention_cases.LN_CHANNELS``: C = 63, 65, 129, 256, 257, 500, 513, 1000, 1024,
1025, 2048, 2049, 2100 puts a width on both sides of every threshold and a masked one into every instantiation; T = 1, 17, 65
are no multiples of either column block.

Inputs (``attention_cases.ln_input``): ``gauss``; ``offset`` = 1e3 + randn (E[x^2] - mean^2 would lose the variance to
cancellation); ``constant`` = every third column exactly constant (var == 0: y == bias exactly, the backward's rstd is
eps^-1/2); ``outlier`` = one channel at 1e4.  Each with weight and bias, and with neither.

Criterion: that of tests/test_gpu_attention_conditioned.py -- ``max|gpu - fp64| <= M * err32 + floor`` and the same for the RMS,
``err32`` from ``F.layer_norm`` in fp32 on the CPU, for y, dx, dweight and dbias.

FIXED BY THESE TESTS.  On ``offset`` the forward needed more than 8 at C = 257 (regs<16,32>: 8.7 max / 15.6 rms) and beyond 2048
(three-pass: 21), and 2 to 4.4 elsewhere.  The column sum is a plain sequential fp32 sum of values near 1e3 (per thread, then over
the NG group partials; the three-pass kernel adds 525 values per wave in a row): its rounding landed in the mean as 2 (C = 257) to
18 (C = 2100) ulp of 1e3, and ``(x - mean) * rstd`` carried it into every output of the column.  All three kernels now sum the
residuals ``x - mean`` next to their squares (same LDS exchange, no further pass) and take their mean off again -- the corrected
two-pass algorithm; ``offset`` is inside the floor everywhere (C = 2100: 1.8e-6 against 2.5e-4 for ATen's fp32).  The variance is
centred in every kernel: ``constant`` columns give the bias exactly.

MEASURED (MI355X; "M needed", max / rms, worst over T and the two parameter settings; 0 = inside the floor):
    forward, all seven kernels, all four families     0 (three-pass, outlier: 0.39)
    backward dx, dbias                                0
    backward dweight                                  0, but outlier: 4.96 at C = 1024, 2.91 at C = 2048 (max; rms 0)
    M = 8: the smallest of {2, 4, 8} above the one row that leaves the floor; it is not twice 4.96.  That row is the outlier
    channel's own dweight, sum_t dy xhat with xhat = 32: 130 terms of up to 100 whose xhat each carry the ~1.5 ulp of
    ``1 / sqrtf(var + eps)``.
"""
import functools

import pytest
import torch

from audio_generation_amd import ops
from tests import attention_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda"
M = 8
KERNEL_OF = [(64, "regs<4,16>"), (128, "regs<8,16>"), (256, "regs<8,32>"), (512, "regs<16,32>"), (1024, "regs<32,32>"),
             (2048, "regs<64,32>"), (1 << 30, "three-pass")]


def _kernel(c):
    return next(name for limit, name in KERNEL_OF if c <= limit)


def test_the_widths_cover_every_kernel_both_sides_of_every_threshold():
    assert {_kernel(c) for c in ac.LN_CHANNELS} == {name for _, name in KERNEL_OF}
    for limit, _ in KERNEL_OF[:-1]:
        assert any(c <= limit and _kernel(c) == _kernel(limit) for c in ac.LN_CHANNELS), limit      # at or below
        assert limit + 1 in ac.LN_CHANNELS, limit                                                   # just above


@functools.lru_cache(maxsize=None)
def _inputs(family, c, t):
    seed = 13 * c + t + 1000 * ac.LN_FAMILIES.index(family)
    g = torch.Generator().manual_seed(seed + 2)
    x = ac.ln_input(family, ac.LN_BATCH, c, t, seed)
    return x, ac.ln_params(c, seed), torch.randn(x.shape, generator=g), torch.randn(x.shape, generator=g)


@pytest.mark.parametrize("family", ac.LN_FAMILIES)
@pytest.mark.parametrize("c", ac.LN_CHANNELS)
def test_forward(family, c):
    for t in ac.LN_LENGTHS:
        x, (w, b), _, _ = _inputs(family, c, t)
        for affine in (True, False):
            weight, bias = (w, b) if affine else (None, None)
            ref = ac.ln_reference(x, weight, bias)
            y = ops.layernorm_ct(x.to(DEV), None if weight is None else weight.to(DEV), None if bias is None else bias.to(DEV),
                                 ac.LN_EPS)
            ac.check(f"layernorm {_kernel(c)} {family} c={c} t={t} affine={affine}", y, ref, "y", M)
            if family == "constant":      # v[k] - mean is exactly zero there
                cols = ac.ln_constant_columns(t)
                want = (b if affine else torch.zeros(c)).reshape(1, c, 1).expand(ac.LN_BATCH, c, int(cols.sum()))
                assert torch.equal(y.cpu()[:, :, cols], want)


@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("family", ac.LN_FAMILIES)
@pytest.mark.parametrize("c", ac.LN_CHANNELS)
def test_backward(family, c, add):
    for t in ac.LN_LENGTHS[1:]:
        x, (w, _), dy, extra = _inputs(family, c, t)
        for affine in (True, False):
            weight = w if affine else None
            ref = ac.ln_reference(x, weight, None, dy, extra if add else None)
            dx, dw, db = ops.layernorm_ct_backward(x.to(DEV), None if weight is None else weight.to(DEV), dy.to(DEV), ac.LN_EPS,
                                                   add=extra.to(DEV) if add else None)
            for name, got in (("dx", dx), ("dweight", dw), ("dbias", db)):
                ac.check(f"layernorm_bwd {family} c={c} t={t} affine={affine} add={add}", got, ref, name, M)
