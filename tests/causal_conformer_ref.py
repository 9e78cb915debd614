"""Float64 restatement of the causal Conformer conv module and its streaming cache (``csrc/conformer.hip``), on top
of ``tests/conformer_ref.py``: everything there holds with left = K - 1 in place of (K - 1) // 2, and with an optional history in
the halo before frame 0.  Channel-major (B, C, T); u is (B, 2 C, T), w (C, K), hist (B, C, K - 1), oldest frame first:

    g        = u[:, :C] s(u[:, C:])
    G[t]     = g[t] for 0 <= t < T;   G[t] = hist[.., (K - 1) + t] for -(K - 1) <= t < 0     (zeros without a history)
    z[.., t] = bias + sum_k w[:, k] G[.., t + k - (K - 1)]
    dg[.., t] = sum_k w[:, k] dz[.., t + (K - 1) - k]                  zeros at and beyond T
    dw[c, k] = sum_{b, t} dz[b, c, t] g[b, c, t + k - (K - 1)]         dbias = sum_{b, t} dz
    hist'    = the last K - 1 values of [hist | g]

The bound formulas are those of ``conformer_ref`` with the causal taps.  A history is an exact operand: it enters z as given --
its error term is that of the fma chain alone, no gate term.
"""
import torch
import torch.nn.functional as F

from tests.conformer_ref import (EPS, K_GATE, MAX_K, TILE, TINY, U, _ch, _sum_c, batch_stats, bn_parts, bn_silu, bound_y, d_gate, f64,  # noqa: F401
                                 feed_forward, glu, layer_norm_ct, linear_ct, sigmoid, silu)

MAX_STEP = 64           # AGX_CONFORMER_MAX_STEP


def shifted(v, k, hist=None):
    """(K, B, C, T): V[.., t + j - (K - 1)] for tap j, with V = [hist | v] (hist None: zeros)."""
    t = v.shape[-1]
    vp = F.pad(v, (k - 1, 0)) if hist is None else torch.cat([hist, v], dim=-1)
    return torch.stack([vp[..., j:j + t] for j in range(k)])


def dwconv(g, w, bias, hist=None):
    w = w.reshape(w.shape[0], -1)
    taps = shifted(g, w.shape[1], hist)                                     # (K, B, C, T)
    return bias.reshape(1, -1, 1) + (w.t().reshape(w.shape[1], 1, -1, 1) * taps).sum(0)


def glu_dwconv(u, w, bias, hist=None):
    return dwconv(glu(u), w, bias, hist)


def next_hist(u, k, hist=None):
    """The last K - 1 values of [hist | g(u)] (hist None: zeros)."""
    g = glu(u)
    if hist is None:
        hist = torch.zeros(g.shape[0], g.shape[1], k - 1, dtype=g.dtype)
    return torch.cat([hist, g], dim=-1)[..., g.shape[-1]:]


def correlate(dz, w):
    """dg[.., t] = sum_j w[:, j] dz[.., t + (K - 1) - j], zeros at and beyond T."""
    k = w.shape[1]
    t = dz.shape[-1]
    dzp = F.pad(dz, (0, k - 1))
    return sum(_ch(w[:, j]) * dzp[..., k - 1 - j:k - 1 - j + t] for j in range(k))


def glu_dwconv_backward(dz, u, w):
    """(du, dw (C, K), dbias) from the formulas."""
    w = w.reshape(w.shape[0], -1)
    c, k = w.shape
    dg = correlate(dz, w)
    ua, v = u[:, :c], u[:, c:]
    s = sigmoid(v)
    du = torch.cat([dg * s, dg * ua * s * (1.0 - s)], dim=1)
    taps = shifted(ua * s, k)
    dw = torch.stack([_sum_c(dz * taps[j]) for j in range(k)], dim=1)
    return du, dw, _sum_c(dz)


# ------------------------------------------------------------------ bounds (conformer_ref's formulas on the causal taps)
def bound_z(u, w, bias, hist=None):
    w = w.reshape(w.shape[0], -1)
    k = w.shape[1]
    g = glu(u)
    wa = w.abs()
    zero_hist = None if hist is None else torch.zeros_like(hist)            # exact: no gate error
    abs_hist = None if hist is None else hist.abs()
    return (dwconv(d_gate(u[:, :w.shape[0]], g), wa, torch.zeros_like(bias), zero_hist)
            + (k + 2) * U * dwconv(g.abs(), wa, bias.abs(), abs_hist))


def bound_conv_backward(dz, u, w):
    """(d_du, d_dw, d_dbias)."""
    w = w.reshape(w.shape[0], -1)
    c, k = w.shape
    n = dz.shape[0] * dz.shape[2]
    dg, d_dg = correlate(dz, w), (k + 2) * U * correlate(dz.abs(), w.abs())
    ua, v = u[:, :c], u[:, c:]
    s = sigmoid(v)
    q = 1.0 - s
    d_q = K_GATE * U * s + U * q
    du, _, _ = glu_dwconv_backward(dz, u, w)
    d_du = torch.cat([s * d_dg + (K_GATE + 1) * U * (dg * s).abs() + dg.abs().clamp_min(1.0) * TINY,
                      ua.abs() * s * q * d_dg + (dg * ua).abs() * (s * d_q + (K_GATE + 1) * U * s * q) + 3 * U * du[:, c:].abs()
                      + (dg * ua).abs().clamp_min(1.0) * TINY], 1)
    g = ua * s
    taps, d_taps = shifted(g, k), shifted(d_gate(ua, g), k)
    d_dw = torch.stack([_sum_c(dz.abs() * d_taps[j]) + (n + 2) * U * _sum_c((dz * taps[j]).abs()) for j in range(k)], dim=1)
    return d_du, d_dw, (n + 2) * U * _sum_c(dz.abs())


# ------------------------------------------------------------------ the modules (differentiable; autograd gives their gradients)
def conv_block(x, sd, prefix, training, stats=None, eps=EPS):
    """``ConformerConvBlock(causal=True)`` without a residual on (B, C, T)."""
    xn = layer_norm_ct(x, sd[prefix + "net.0.weight"], sd[prefix + "net.0.bias"])
    u = linear_ct(xn, sd[prefix + "net.1.weight"], sd[prefix + "net.1.bias"])
    z = glu_dwconv(u, sd[prefix + "net.3.weight"], sd[prefix + "net.3.bias"])
    if training:
        mean, var, m2 = batch_stats(z)
        if stats is not None:
            stats.update(mean=mean.detach(), var=var.detach(), m2=m2.detach(), n=z.shape[0] * z.shape[2])
    else:
        mean, var = sd[prefix + "net.4.running_mean"], sd[prefix + "net.4.running_var"]
    y = bn_silu(z, sd[prefix + "net.4.weight"], sd[prefix + "net.4.bias"], mean, var, eps)
    return linear_ct(y, sd[prefix + "net.6.weight"], sd[prefix + "net.6.bias"])


def attention(x, sd, prefix, heads, window=None):
    """The causal (windowed) ALiBi self-attention sub-block without its residual, through the definitions of
    ``tests/causal_attention_ref.py`` / ``tests/window_attention_ref.py`` (they take (B, T, dim))."""
    from tests.causal_attention_ref import causal_attention
    from tests.window_attention_ref import window_attention
    xt = x.transpose(1, 2)
    o = causal_attention(xt, sd, prefix, heads) if window is None else window_attention(xt, sd, prefix, heads, window)
    return o.transpose(1, 2)


def conformer_block(x, sd, heads, training, stats=None, window=None):
    """``ConformerBlock(causal=True, window=window)`` on (B, dim, T), no dropout."""
    x = x + 0.5 * feed_forward(x, sd, "first_ff.", silu)
    x = x + attention(x, sd, "attention.", heads, window)
    x = x + conv_block(x, sd, "conv_block.", training, stats)
    x = x + 0.5 * feed_forward(x, sd, "second_ff.", silu)
    return layer_norm_ct(x, sd["layer_norm.weight"], sd["layer_norm.bias"])
