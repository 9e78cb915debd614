"""Float64 restatement of the two streaming steps of DESIGN 4.24, in the terms of tests/codec_stream_ref.py: index gathers on
rings, the validity mask, per-row counts.

    multires(K, depth)   y[c, j] = gelu(w[c, depth + 1] x[c, j] + w[c, 0] low_depth[c, j] + sum_lvl w[c, lvl] high_lvl[c, j]);
                         level lvl = depth .. 1 has dilation 2^(depth - lvl) and reads j - (K - 1 - k) dil;
                         H = (K - 1)(2^depth - 1), r and D unchanged.  Input columns of index < 0 are 0 IN THE RING.
    resdw(d)             leaky(x + conv_1(leaky(conv_7,d(a) + b1)) + b2) with the operand a[c, i] = i >= 0 ? scale[c] x[c, i] + shift[c] : 0
                         -- the causal zero padding lies behind the per-channel affine; H = d (k - 1), r and D unchanged.

``counts``: row ``b`` takes its first ``clamp(counts[b], 0, n)`` frames; a plain destination holds 0 behind them, a ring is not
written there, and no source column behind the count is read.

Bound of the affine conv: codec_stream_ref's ``(c_in K + 2) U (sum |w| |a| + |bias|)`` on the operand a, plus the operand's own
rounding (one fused multiply-add) carried through the weights: ``+ U sum |w| (|scale x| + |shift|)``.
"""
import math

import torch

from tests import codec_stream_ref as ref
from tests.conformer_ref import U

LIVE = ref.LIVE


def reach(k, depth):
    return (k - 1) * ((1 << depth) - 1)


def _taken(counts, r, n):
    return n if counts is None else max(0, min(int(counts[r]), n))


def gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def multires_step(h0, h1, w, depth, src, dst, pos, end, n, rate, delay, dst_ring=True, counts=None, mask_start=True, mask_end=True):
    """One step of a multires layer for every row, float64, in place on ``dst``; returns the produced block (B, C, n rate), exact 0
    behind a row's count.  ``h0`` / ``h1`` (C, 1, K), ``w`` (C, depth + 2); ``src``: the ring (B, C, cap) of the layer's input."""
    b, c, cap = src.shape
    k = h0.shape[-1]
    hh = reach(k, depth)
    out = torch.zeros(b, c, n * rate, dtype=torch.float64)
    for r in range(b):
        cols = _taken(counts, r, n) * rate
        if not dst_ring:
            dst[r] = 0.0                                                               # a plain destination: exact 0 behind the count
        if cols == 0:
            continue
        j = torch.arange(pos[r] * rate - delay, pos[r] * rate - delay + cols, dtype=torch.int64)
        g = torch.arange(int(j[0]) - hh, int(j[-1]) + 1, dtype=torch.int64)            # the window: the reach, then the taken columns
        assert cap >= hh + n * rate, "the step's writes would alias its history"
        low = src[r][:, torch.remainder(g, cap)]                                       # index < 0: 0 in the ring itself
        x = low[:, hh:]
        y = torch.zeros(c, cols, dtype=torch.float64)
        dil = 1
        for lvl in range(depth, 0, -1):
            i = torch.arange(g.numel(), dtype=torch.int64).reshape(-1, 1) - (k - 1 - torch.arange(k, dtype=torch.int64)) * dil
            taps = torch.where(i >= 0, low[:, i.clamp(min=0)], torch.zeros((), dtype=torch.float64))     # (C, W, K)
            high = torch.einsum("ck,cwk->cw", h1[:, 0].double(), taps)
            low = torch.einsum("ck,cwk->cw", h0[:, 0].double(), taps)
            y = y + w[:, lvl:lvl + 1].double() * high[:, hh:]
            dil *= 2
        y = y + w[:, :1].double() * low[:, hh:]
        y = gelu(y + x * w[:, -1:].double())
        if end is not None:
            y = y * ref._valid(j, end[r], rate, mask_start, mask_end)
        out[r, :, :cols] = y
        if dst_ring:
            dst[r][:, torch.remainder(j, dst.shape[2])] = y
        else:
            dst[r] = out[r]
    return out


def affine_step(op, scale, shift, src, dst, pos, n, rate, delay, counts=None, select=True):
    """The dilated conv of a depthwise block (``op``: a stride-1 causal ``codec_stream_ref.Op`` with its ``pre`` slope) from the
    ring ``src`` into the plain ``dst`` (B, c_out, n rate), its operand formed from ``scale`` / ``shift`` (c_in,).  ``select=False``
    drops the ``i >= 0`` select, so that a test can show it is needed.  Returns (block, bound), both 0 behind a row's count."""
    assert op.kind == "causal" and op.s == 1 and not op.residual and op.post is None
    b, cap = src.shape[0], src.shape[2]
    out = torch.zeros(b, op.c_out, n * rate, dtype=torch.float64)
    bound = torch.zeros_like(out)
    sc, sh = scale.double()[:, None, None], shift.double()[:, None, None]
    wabs = op.w.abs()
    for r in range(b):
        cols = _taken(counts, r, n) * rate
        if cols == 0:
            continue
        j = torch.arange(pos[r] * rate - delay, pos[r] * rate - delay + cols, dtype=torch.int64)
        idx = op.reads(j)
        assert int(idx.min()) >= int(j[0]) + n * rate - cap, "a layer reads behind its ring"
        xg = src[r][:, torch.remainder(idx, cap)]                                      # (c_in, cols, k)
        a = sc * xg + sh
        round_a = (sc * xg).abs() + sh.abs()
        if select:
            keep = (idx >= 0)[None]
            a, round_a = a * keep, round_a * keep
        v = torch.einsum("oik,ijk->oj", op.w, a)
        mag = torch.einsum("oik,ijk->oj", wabs, a.abs())
        if op.bias is not None:
            v = v + op.bias[:, None]
            mag = mag + op.bias.abs()[:, None]
        bd = (op.c_in * op.k + 2) * U * mag + U * torch.einsum("oik,ijk->oj", wabs, round_a)
        if op.pre is not None:
            v = ref.leaky(v, op.pre)
        out[r, :, :cols], bound[r, :, :cols] = v, bd
    dst.copy_(out)
    return out, bound


def resdw_unit_step(op1, op2, scale, shift, ring, dst, pos, end, n, rate, delay, dst_ring=True, counts=None, select=True):
    """A depthwise residual unit as the two launches a stream runs: the affine conv into a plain hidden tensor, then the k = 1 conv
    with the residual from ``ring`` (``codec_stream_ref.step``, row by row when counted).  Returns (block, bound)."""
    b = ring.shape[0]
    h = torch.zeros(b, op1.c_out, n * rate, dtype=torch.float64)
    _, b1 = affine_step(op1, scale, shift, ring, h, pos, n, rate, delay, counts=counts, select=select)
    out = torch.zeros(b, op2.c_out, n * rate, dtype=torch.float64)
    bound = torch.zeros_like(out)
    for r in range(b):
        m = _taken(counts, r, n)
        if m == 0:
            continue
        cols = m * rate
        d_r = dst[r:r + 1] if dst_ring else torch.zeros(1, op2.c_out, cols, dtype=torch.float64)
        e_r = None if end is None else [end[r]]
        o, b2 = ref.step(op2, h[r:r + 1, :, :cols], d_r, [pos[r]], e_r, m, rate, delay, src_ring=False, dst_ring=dst_ring, res=ring[r:r + 1])
        carried = torch.einsum("oi,bij->boj", op2.w[:, :, 0].abs(), b1[r:r + 1, :, :cols] + U * h[r:r + 1, :, :cols].abs())
        if end is not None:
            j = torch.arange(pos[r] * rate - delay, pos[r] * rate - delay + cols, dtype=torch.int64)
            carried = carried * ref._valid(j, end[r], rate)
        out[r, :, :cols], bound[r, :, :cols] = o[0], (b2 + carried)[0]
    if not dst_ring:
        dst.copy_(out)
    return out, bound


def stream_clip(step_fn, x, c_out, hh, schedule, rate=1, delay=0):
    """Feed the clip ``x`` (B, C, T rate) through ``step_fn(ring, dst, pos, n)`` in the frames of ``schedule`` on a tight ring;
    the chunk of a step holds the columns [pos rate - delay, (pos + n) rate - delay), exact 0 outside the clip (what a producer
    stores).  Returns the concatenated plain outputs."""
    b, c, length = x.shape
    mc = max(schedule)
    ring = torch.zeros(b, c, hh + mc * rate, dtype=torch.float64)
    pos, outs = [0] * b, []
    for n in schedule:
        j = torch.arange(pos[0] * rate - delay, (pos[0] + n) * rate - delay, dtype=torch.int64)
        ok = (j >= 0) & (j < length)
        ring[:, :, torch.remainder(j, ring.shape[2])] = torch.where(ok, x[:, :, j.clamp(0, length - 1)].double(),
                                                                    torch.zeros((), dtype=torch.float64))
        dst = torch.zeros(b, c_out, n * rate, dtype=torch.float64)
        outs.append(step_fn(ring, dst, pos, n))
        pos = [p + n for p in pos]
    return torch.cat(outs, dim=2)
