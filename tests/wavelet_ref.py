"""Float64 restatement of the plain wavelet ops of ``csrc/wavelet.hip`` -- ``agx_multires_forward`` / ``_backward``,
``agx_group_sum``, ``agx_wavelet_fold`` / ``_backward`` -- written from the formulas, and the error bounds the tests hold the fp32
kernels to.  The conventions are those of tests/conformer_ref.py: u = 2^-24; a K-term fma chain costs ``(K + 2) u sum |term|`` in any
order; every right-hand side is evaluated in float64 from the operands an op is GIVEN; second-order terms are left to the factor 2
the checks allow.

    multires   low_0 = x;  level lvl = depth .. 1 has dilation dil = 2^(depth - lvl):
                   high_lvl[t] = sum_k h1[k] low[t - (K - 1 - k) dil],   low'[t] = sum_k h0[k] low[t - (K - 1 - k) dil]
               (a term whose index is negative is 0: a select, never a read), and
                   pre = sum_lvl w[lvl] high_lvl + w[0] low_depth + w[depth + 1] x,     y = gelu(pre) = pre Phi(pre)
    backward   dpre = dout gelu'(pre),  gelu'(v) = Phi(v) + v phi(v);   g_depth = w[0] dpre;  level j = depth - 1 .. 0 (dil = 2^j,
               wl = w[depth - j], in_j = the low-pass after j levels):
                   dh1[k] += sum_{b,t} wl dpre[t] in_j[t - (K - 1 - k) dil],    dh0[k] += sum_{b,t} g_{j+1}[t] in_j[t - (K - 1 - k) dil]
                   g_j[s] = sum_k h0[k] g_{j+1}[s + (K - 1 - k) dil] + h1[k] wl dpre[s + (K - 1 - k) dil]       (0 past the end)
               dx = g_0 + w[depth + 1] dpre;   dw[0] = sum dpre low_depth,  dw[lvl] = sum dpre high_lvl,  dw[depth + 1] = sum dpre x
    fold       tests/wavelet_stream_ref.py: ``kern64``, the table [S_hi | S_lo | tail] and ``fold_operand`` -- the plain fold and the
               streaming out-step form the same numbers in the same order (csrc/wavelet_fold.hpp).  Here the device forms the table
               too, so its error is carried:  kern = cos(t) exp(-t^2 / sigma) carries (5 + 2 t^2 / sigma) u |kern| (2 ulp of cosf, 1
               of expf, the product, and the two roundings of the exponent's argument, which exp turns into a relative error of
               that size); a sum of n of them, (n + 2) u sum |kern| more.  d kern / d sigma = kern t^2 / sigma^2: 4 more roundings.
               dh[l] is one fma chain of at most 3 s - 1 terms; dsigma's terms pass through a lane's chain over its frames
               (ceil(L / 256) (3 s) additions), the workgroup's tree (8) and the rows in turn (B C).
    group_sum  out[i] = sum_{j < group} g[i group + j], times gelu'(pre[i]) when given.

Bounds of the cascade.  The level errors are carried:
    d_low'  = sum_k |h0[k]| d_low[t - (K - 1 - k) dil] + (K + 2) u sum_k |h0[k] low[..]|,       d_high likewise with h1
    d_pre   = sum_lvl |w[lvl]| d_high_lvl + |w[0]| d_low + (depth + 4) u (sum_lvl |w[lvl] high_lvl| + |w[0] low| + |w[depth+1] x|)
    d_y     = 1.13 d_pre + G_GELU u (|pre| + |y|)                                                    |gelu'| <= 1.13
    d_dpre  = |dout| (G_GRAD u (1 + |gelu'(pre)|) + 0.8 d_pre) + u |dpre|                            |gelu''| <= 0.8
    d_g_j   = sum_k (|h0[k]| d_g_{j+1}[..] + |h1[k] wl| d_dpre[..]) + (2 K + 3) u sum_k (|h0 g| + |h1 wl dpre|);  d_g_depth = |w0| d_dpre + u |g|
    d_dx    = d_g_0 + |w_x| d_dpre + 2 u (|g_0| + |w_x dpre|)
    a parameter sum of terms a_n b_n:      sum (d_a |b| + |a| d_b) + (N + 3) u sum |a b|
        N is not the number of terms but the number of additions one term passes through, which is what the rounding of a sum
        grows with: a lane adds its 2 owned positions (1), the wave's butterfly (6), the 4 waves (2), the levels into one slot
        (depth; dh0 and dh1 only) and the (row, tile) partials in turn (B ceil(L / 512)).  At B L = 3075 terms this is several
        hundred times tighter than the term count, and a dropped tile or level no longer hides in it.

G_GELU and G_GRAD are the allowances for ``erff`` / ``expf`` inside the device's ``gelu_erf`` and ``gelu_grad``.  They are measured, on
the device, against float64 ``erf`` -- never against another run of the kernel: the depth-0 call with w = (0, 1) has pre = x exactly,
so its output IS gelu_erf(x) (and the backward's dx with dout = 1 IS gelu_grad(x)).  On a dense grid of 2^16 inputs in [-6, 6] plus
+-2^-e, e = 0 .. 20, ``tests/test_gpu_wavelet_ops.py::test_gelu_constants_against_float64_erf`` measured

    max |gelu_erf(x) - gelu(x)| / (u (|x| + |y|))      = 0.948        G_GELU = 2
    max |gelu_grad(x) - gelu'(x)| / (u (1 + |gelu'|))  = 1.096        G_GRAD = 3

on the MI355X, and the constants are twice that, rounded up to an integer.  Both are far below 16, the error OpenCL's full profile allows erf.
"""
import math
from types import SimpleNamespace

import torch

from tests.conformer_ref import U, f64
from tests.wavelet_stream_ref import fold_operand, fold_table64, kern64

__all__ = ["U", "G_GELU", "G_GRAD", "gelu", "gelu_grad", "reach", "contracting", "multires", "multires_backward", "fold",
           "fold_backward", "group_sum", "selector_offset", "shifted"]

G_GELU = 2.0            # measured 0.948, see above
G_GRAD = 3.0            # measured 1.096
GELU_LIP = 1.13         # max |gelu'|  (1.1290 at v = sqrt(2))
GRAD_LIP = 0.8          # max |gelu''| (2 phi(0) = 0.7979 at v = 0)
TILE_BWD = 512          # positions of a row one workgroup of the backward owns (csrc/wavelet.hip: MRB_TT)
ZERO = torch.zeros((), dtype=torch.float64)


def gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def gelu_grad(v):
    return 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def reach(k, depth):
    return (k - 1) * ((1 << depth) - 1)


def contracting(c, k, depth, gen):
    """The filters of tests/test_gpu_multires_stream.py: a cascade of them neither grows nor dies, so the bound stays near 2e-6 at
    every depth."""
    scalar = 2.0 ** 0.5 / (2 * k)
    h0 = (torch.rand(c, 1, k, generator=gen) * 2 - 1) * scalar
    h1 = (torch.rand(c, 1, k, generator=gen) * 2 - 1) * scalar
    w = (torch.rand(c, depth + 2, generator=gen) * 2 - 1) * (2.0 / (2 * depth + 4)) ** 0.5
    return h0, h1, w


def _back(v, k, dil):
    """(B, C, L) -> (B, C, L, K): v[t - (K - 1 - k) dil], 0 where that index is negative -- a select, a NaN there does not spread."""
    n = v.shape[-1]
    idx = torch.arange(n).reshape(-1, 1) - (k - 1 - torch.arange(k)) * dil
    return torch.where(idx >= 0, v[..., idx.clamp(min=0)], ZERO)


def _ahead(v, k, dil):
    """(B, C, L) -> (B, C, L, K): v[s + (K - 1 - k) dil], 0 past the end."""
    n = v.shape[-1]
    idx = torch.arange(n).reshape(-1, 1) + (k - 1 - torch.arange(k)) * dil
    return torch.where(idx < n, v[..., idx.clamp(max=n - 1)], ZERO)


def _levels(x, h0, h1, depth):
    """The cascade: ([low_0 .. low_depth], [d_low_j], [high_j], [d_high_j]) with high_j the high-pass of low_j (dilation 2^j)."""
    k = h0.shape[-1]
    a0, a1 = h0[:, 0].abs(), h1[:, 0].abs()
    low, d_low, high, d_high = [x], [torch.zeros_like(x)], [], []
    for j in range(depth):
        taps, d_taps = _back(low[j], k, 1 << j), _back(d_low[j], k, 1 << j)
        high.append(torch.einsum("ck,bclk->bcl", h1[:, 0], taps))
        d_high.append(torch.einsum("ck,bclk->bcl", a1, d_taps) + (k + 2) * U * torch.einsum("ck,bclk->bcl", a1, taps.abs()))
        low.append(torch.einsum("ck,bclk->bcl", h0[:, 0], taps))
        d_low.append(torch.einsum("ck,bclk->bcl", a0, d_taps) + (k + 2) * U * torch.einsum("ck,bclk->bcl", a0, taps.abs()))
    return low, d_low, high, d_high


def _pre(x, w, depth, low, d_low, high, d_high):
    wc = w[None, :, :, None]                                                   # (1, C, depth + 2, 1)
    pre = wc[:, :, 0] * low[depth] + wc[:, :, depth + 1] * x
    mag = (wc[:, :, 0] * low[depth]).abs() + (wc[:, :, depth + 1] * x).abs()
    carried = wc[:, :, 0].abs() * d_low[depth]
    for j in range(depth):
        term = wc[:, :, depth - j] * high[j]
        pre, mag, carried = pre + term, mag + term.abs(), carried + wc[:, :, depth - j].abs() * d_high[j]
    return pre, carried + (depth + 4) * U * mag


def multires(x, h0, h1, w, depth):
    """``x`` (B, C, L), ``h0`` / ``h1`` (C, 1, K), ``w`` (C, depth + 2) -> (y, pre, bound of y), float64."""
    x, h0, h1, w = f64(x, h0, h1, w)
    lv = _levels(x, h0, h1, depth)
    pre, d_pre = _pre(x, w, depth, *lv)
    y = gelu(pre)
    return y, pre, GELU_LIP * d_pre + G_GELU * U * (pre.abs() + y.abs())


def multires_backward(x, dout, h0, h1, w, depth):
    """-> ((dx, dh0, dh1, dw), their bounds), float64, in the shapes of the operands."""
    x, dout, h0, h1, w = f64(x, dout, h0, h1, w)
    b, c, n = x.shape
    k = h0.shape[-1]
    low, d_low, high, d_high = _levels(x, h0, h1, depth)
    pre, d_pre = _pre(x, w, depth, low, d_low, high, d_high)
    gg = gelu_grad(pre)
    dpre = dout * gg
    d_dpre = dout.abs() * (G_GRAD * U * (1.0 + gg.abs()) + GRAD_LIP * d_pre) + U * dpre.abs()
    wc = w[None, :, :, None]

    def psum(a, d_a, v, d_v, terms):
        """sum over (b, t) of a v, per channel [and tap]: a, v broadcastable to (B, C, L[, K])."""
        return (a * v).sum(dim=(0, 2)), (d_a * v.abs() + a.abs() * d_v).sum(dim=(0, 2)) + (terms + 3) * U * (a * v).abs().sum(dim=(0, 2))

    dw, d_dw = torch.zeros_like(w), torch.zeros_like(w)
    adds = 9 + b * -(-n // TILE_BWD)                                           # see the docstring
    dw[:, 0], d_dw[:, 0] = psum(dpre, d_dpre, low[depth], d_low[depth], adds)
    dw[:, depth + 1], d_dw[:, depth + 1] = psum(dpre, d_dpre, x, torch.zeros_like(x), adds)
    g = wc[:, :, 0] * dpre
    d_g = wc[:, :, 0].abs() * d_dpre + U * g.abs()
    dh0, dh1 = torch.zeros(c, k, dtype=torch.float64), torch.zeros(c, k, dtype=torch.float64)
    m0, m1, c0, c1 = torch.zeros_like(dh0), torch.zeros_like(dh0), torch.zeros_like(dh0), torch.zeros_like(dh0)
    a0, a1 = h0[:, 0].abs(), h1[:, 0].abs()
    for j in range(depth - 1, -1, -1):
        dil, wl = 1 << j, wc[:, :, depth - j]
        dw[:, depth - j], d_dw[:, depth - j] = psum(dpre, d_dpre, high[j], d_high[j], adds)
        taps, d_taps = _back(low[j], k, dil), _back(d_low[j], k, dil)                  # (B, C, L, K)
        q, d_q = wl * dpre, wl.abs() * d_dpre + U * (wl * dpre).abs()
        for acc, mag, car, a, d_a in ((dh0, m0, c0, g, d_g), (dh1, m1, c1, q, d_q)):
            term = a[..., None] * taps
            acc += term.sum(dim=(0, 2))
            mag += term.abs().sum(dim=(0, 2))
            car += (d_a[..., None] * taps.abs() + a.abs()[..., None] * d_taps).sum(dim=(0, 2))
        ga, qa = _ahead(g, k, dil), _ahead(q, k, dil)
        nxt = torch.einsum("ck,bclk->bcl", h0[:, 0], ga) + torch.einsum("ck,bclk->bcl", h1[:, 0], qa)
        d_nxt = (torch.einsum("ck,bclk->bcl", a0, _ahead(d_g, k, dil)) + torch.einsum("ck,bclk->bcl", a1, _ahead(d_q, k, dil))
                 + (2 * k + 3) * U * (torch.einsum("ck,bclk->bcl", a0, ga.abs()) + torch.einsum("ck,bclk->bcl", a1, qa.abs())))
        g, d_g = nxt, d_nxt
    wx = wc[:, :, depth + 1]
    dx = g + wx * dpre
    d_dx = d_g + wx.abs() * d_dpre + 2 * U * (g.abs() + (wx * dpre).abs())
    terms = adds + depth
    d_dh0, d_dh1 = c0 + (terms + 3) * U * m0, c1 + (terms + 3) * U * m1
    shape = (c, 1, k)
    return (dx, dh0.reshape(shape), dh1.reshape(shape), dw), (d_dx, d_dh0.reshape(shape), d_dh1.reshape(shape), d_dw)


# --------------------------------------------------------------------------- the fold
def _kern_bound(space, sigma, channels):
    """(kern, d_kern, dkern = d kern / d sigma, d_dkern), each (C, P)."""
    t = f64(space).reshape(1, -1)
    sg = f64(sigma).reshape(-1, 1).expand(channels, 1) if sigma.numel() == 1 else f64(sigma).reshape(channels, 1)
    kern = kern64(f64(space), f64(sigma), channels)
    rel = (5.0 + 2.0 * t * t / sg) * U
    dkern = kern * (t * t) / (sg * sg)
    return kern, rel * kern.abs(), dkern, (rel + 4 * U) * dkern.abs()


def _tables(space, sigma, channels, s):
    """(table, its bound, the table of d / d sigma, its bound): (C, 3 s - 1) each."""
    kern, d_kern, dkern, d_dkern = _kern_bound(space, sigma, channels)
    p = kern.shape[1]
    assert p % s == 0
    fold_ = p // s

    def sums(v):
        hi = torch.stack([v[:, ph * fold_:].sum(1) for ph in range(s)], 1)
        lo = torch.stack([v[:, :ph * fold_].sum(1) for ph in range(s)], 1)
        return torch.cat([hi, lo, v[:, p - (s - 1):]], 1)

    def bound(v, d_v):
        n = torch.cat([p - torch.arange(s) * fold_, torch.arange(s) * fold_, torch.zeros(s - 1, dtype=torch.int64)]).double()
        chain = torch.where(n > 0, (n + 2) * U, ZERO) * sums(v.abs())
        return sums(d_v) + chain

    table = sums(kern)                                         # s = 1 too: one window per frame, no tail
    assert s < 2 or torch.equal(table, fold_table64(f64(space), f64(sigma), channels, s))
    return table, bound(kern, d_kern), sums(dkern), bound(dkern, d_dkern)


def _operand(table, s, hrow, length):
    """``fold_operand`` on a whole row: y[c, u], its rounding bound and |dy / dh|, u < L s."""
    unit = SimpleNamespace(s=s, table=table)
    return fold_operand(unit, hrow, torch.arange(length * s, dtype=torch.int64), length, 0, length)


def fold(h, space, sigma, s):
    """``h`` (B, C, L) -> (y (B, C, L s), bound)."""
    h = f64(h)
    b, c, n = h.shape
    table, d_table, _, _ = _tables(space, sigma, c, s)
    y, bound = torch.zeros(b, c, n * s, dtype=torch.float64), torch.zeros(b, c, n * s, dtype=torch.float64)
    for r in range(b):
        y[r], ybd, _ = _operand(table, s, h[r], n)
        carried, _, _ = _operand(d_table, s, h[r].abs(), n)                            # |h0| d_S_hi + |h1| d_S_lo
        bound[r] = ybd + carried
    return y, bound


def _fold_terms(h, dout, table, s):
    """The terms of the fold's output as (B, C, L, 3 s - 1): term[b, c, l, e] = dout[u] h[l] table[e] for every output u that
    frame l feeds through table entry e -- so y's gradients are sums of them without h (dh) or with the sigma table (dsigma)."""
    b, c, n = h.shape
    d = dout.reshape(b, c, n, s)
    n_win = (n - 1) * s + 1
    u = torch.arange(n * s).reshape(n, s)
    hi = torch.where(u < n_win, d, ZERO)                                                # windows starting in frame l
    prev = torch.cat([torch.zeros(b, c, 1, s, dtype=torch.float64), d[:, :, :-1]], 2)   # windows of frame l - 1 spilling over
    lo = torch.where(torch.arange(s) > 0, prev, ZERO)
    tail = torch.zeros(b, c, n, s - 1, dtype=torch.float64)
    tail[:, :, n - 1] = dout[:, :, n_win:]
    return torch.cat([hi, lo, tail], 3)


def fold_backward(h, dout, space, sigma, s):
    """-> ((dh (B, C, L), dsigma in sigma's shape), their bounds)."""
    h, dout = f64(h), f64(dout)
    b, c, n = h.shape
    table, d_table, dtab, d_dtab = _tables(space, sigma, c, s)
    reads = _fold_terms(h, dout, table, s)                                              # (B, C, L, 3 s - 1): the dout behind each entry
    dh = (reads * table[None, :, None]).sum(3)
    d_dh = (reads.abs() * d_table[None, :, None]).sum(3) + (3 * s + 2) * U * (reads * table[None, :, None]).abs().sum(3)
    terms = reads * h[..., None] * dtab[None, :, None]
    per_c = terms.sum(dim=(0, 2, 3))
    count = -(-n // 256) * 3 * s + 8 + b * c + 3      # a lane's chain over its frames, the workgroup's tree, the rows in turn
    d_per_c = (reads * h[..., None]).abs().mul(d_dtab[None, :, None]).sum(dim=(0, 2, 3)) + count * U * terms.abs().sum(dim=(0, 2, 3))
    if sigma.numel() == 1:
        per_c, d_per_c = per_c.sum(), d_per_c.sum()
    return (dh, per_c.reshape(sigma.shape)), (d_dh, d_per_c.reshape(sigma.shape))


def group_sum(g, group, pre=None):
    """-> (out, bound): out[..., i] = sum_j g[..., i group + j] (times gelu'(pre[..., i]))."""
    g = f64(g)
    v = g.reshape(*g.shape[:-1], -1, group)
    s, bound = v.sum(-1), (group + 2) * U * v.abs().sum(-1)
    if pre is None:
        return s, bound
    gg = gelu_grad(f64(pre))
    out = s * gg
    return out, gg.abs() * bound + s.abs() * G_GRAD * U * (1.0 + gg.abs()) + U * out.abs()


# --------------------------------------------------------------------------- selector cases
def selector_offset(k, depth, i, a, b):
    """With h0 = e_a, h1 = e_b and w = e_i the pre-activation is x delayed by this many columns."""
    if i == 0:
        return (k - 1 - a) * ((1 << depth) - 1)
    j = depth - i
    return (k - 1 - a) * ((1 << j) - 1) + (k - 1 - b) * (1 << j)


def selector_params(c, k, depth, i, a, b):
    """(h0, h1, w) of a selector case, and (h, h, w) of its depth-0 anchor: w = (0, 1)."""
    h0, h1, w = torch.zeros(c, 1, k), torch.zeros(c, 1, k), torch.zeros(c, depth + 2)
    h0[:, 0, a], h1[:, 0, b], w[:, i] = 1.0, 1.0, 1.0
    return h0, h1, w


def anchor_params(c):
    return torch.zeros(c, 1, 1), torch.zeros(c, 1, 1), torch.tensor([[0.0, 1.0]]).repeat(c, 1)


def shifted(x, off):
    """x delayed by ``off`` columns, zero-filled; ``off`` < 0 advances it."""
    out = torch.zeros_like(x)
    n = x.shape[-1]
    if off >= 0 and off < n:
        out[..., off:] = x[..., :n - off]
    elif off < 0 and -off < n:
        out[..., :n + off] = x[..., -off:]
    return out


# --------------------------------------------------------------------------- the cases both test files run
# forward, selectors: (K, depth, L).  (3, 10): halo 2046 > the tile of 1024, the tile at 3072 draws on two earlier ones;
# (3, 13): halo 16382, 139 KB of LDS, just under the limit
FWD_SELECT = [(3, 3, 1025), (2, 5, 300), (3, 10, 3100), (3, 13, 1500)]
# backward, selectors.  (3, 9): halo 1022 > the tile of 512, 133 KB of LDS;  (29, 4): 2 K + depth + 2 = 64 exactly
BWD_SELECT = [(3, 9, 1300), (29, 4, 900)]
# forward, random values: (K, depth, B, C, L)
FWD_RANDOM = [(3, 3, 2, 3, n) for n in (1, 2, 1023, 1024, 1025, 2049)] + [
    (5, 4, 2, 3, 7),            # halo 60 longer than the signal
    (1, 20, 2, 2, 1100),        # the depth limit; K = 1: no halo at all
    (3, 0, 2, 3, 300),          # no level
    (2, 2, 70, 1000, 8),        # 70000 rows: more than a gridDim.y holds
]
FWD_WIDE = (257, 1, 1, 2, 600)  # K > the workgroup's 256 threads
BWD_RANDOM = [(3, 3, 3, 2, n) for n in (1, 511, 512, 513, 1025)] + [(3, 0, 3, 2, 300)]
# fold: (scale, P, L).  (5, 40, 4100): L scale = 20500 > 64 stripes of 256;  (256, 256, 3): fold = 1 at both limits
FOLD = [(5, 40, 4100), (8, 256, 33), (256, 256, 3), (1, 4, 19), (4, 8, 1)]
FOLD_BWD = [(5, 40, n) for n in (1, 255, 256, 257, 1000)] + [(256, 256, 3), (1, 4, 19)]
GROUP_SUM = [(group, n_out, pre) for group in (1, 5, 8) for n_out in (1, 257) for pre in (False, True)]


def ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def selectors(k, depth):
    """Every (i, a, b) of a selector sweep: all levels, both ends of both filters."""
    ends = sorted({0, k - 1})
    return [(i, a, b) for i in range(depth, -1, -1) for a in ends for b in ends]


def multires_inputs(case, backward=False):
    k, depth, b, c, n = case
    gen = torch.Generator().manual_seed(1000 * k + 100 * depth + 7 * b + c + 13 * n)
    x = torch.randn(b, c, n, generator=gen)
    h0, h1, w = contracting(c, k, depth, gen)
    if backward:
        return x, torch.randn(b, c, n, generator=gen), h0, h1, w
    return x, h0, h1, w


def fold_inputs(case, channelwise, b=2, c=3):
    s, p, n = case
    gen = torch.Generator().manual_seed(100 * s + p + 3 * n + int(channelwise))
    h = torch.randn(b, c, n, generator=gen)
    dout = torch.randn(b, c, n * s, generator=gen)
    space = torch.linspace(-10, 10, p)
    sigma = 20.0 + 30.0 * torch.rand((1, c, 1, 1) if channelwise else (1,), generator=gen)
    return h, dout, space, sigma
