"""Float64 restatement of the Conformer classes (networks/transformers.py:281-368) under the three build-defined decisions of
DESIGN 4.18 (depthwise conv, no ``activation`` for ``Attention``, LayerNorm over channels before the rearrangement), written
from the formulas, and the error bounds the tests hold the fp32 kernels of ``csrc/conformer.hip`` to.  Channel-major (B, C, T)
throughout; u is (B, 2 C, T), w (C, K), left = (K - 1) // 2:

    s(v)  = 1 / (1 + exp(-v))
    g     = u[:, :C] s(u[:, C:])                                      GLU(dim=-2)
    z     = bias + sum_k w[:, k] g[.., t + k - left]                  zeros outside [0, T): torch's padding="same"
    mean  = sum z / N,  M2 = sum (z - mean)^2,  var = M2 / N          N = B T; the running variance takes M2 / (N - 1)
    rstd  = 1 / sqrt(var + eps),  zhat = (z - mean) rstd,  a = zhat gamma + beta,  y = a s(a)
    da    = dy s(a) (1 + a (1 - s(a)))        dbeta = sum da        dgamma = sum da zhat
    dz    = gamma rstd (da - dbeta / N - zhat dgamma / N)             eval (frozen statistics): dz = gamma rstd da
    dg    = sum_k w[:, k] dz[.., t + left - k]
    du    = (dg s(v), dg u_a s(v) (1 - s(v)))                         u_a = u[:, :C], v = u[:, C:]
    dw[c, k] = sum_{b, t} dz[b, c, t] g[b, c, t + k - left]           dbias = sum_{b, t} dz

``tests/test_conformer_cpu.py`` pins these to the goldens of the reference and to a float64 composition of
``torch.nn.functional`` ops under autograd, gradients included.

Bounds (u = 2^-24; every right-hand side is evaluated in float64 from the operands an op is GIVEN -- an op's inputs are exact;
second-order terms are left to the factor 2 the checks allow, except where they are written out).  TINY = 2^-126 stands where
a result can be subnormal.

  sigmoid, gate, silu   K_GATE = 8: x s(v) is within 8 u |x s(v)| + max(1, |x|) TINY of exact: the relative constant is the one
                        ``tests/test_gpu_conditioning.py`` holds ``agx_sigmoid_gate`` to (16 u under its factor 2); s(v) itself is
                        the gate of x = 1.  expf(-v) overflows just below v = -88.7, where s(v) = 0.25 TINY: the device's sigmoid is
                        exactly 0 from there on, an absolute error below TINY that x multiplies.
  a K-term fma chain    (K + 2) u sum |term|, any order.
  z        sum_k |w_k| d_g + (K + 2) u (|bias| + sum_k |w_k g|),                   d_g = 8 u |g| + max(1, |u_a|) TINY
  mean     d_mean = (17 + 4 M) u Zmax.  A segment's sum goes through at most 16 additions per element (8 in a walker, 6 in the
           halving tree, 2 across the groups) and one division: 17 u Zmax with Zmax = max |z| of the channel; each of the at most
           M = min(P - 1, ceil(P / 64) + 6) merges a partial passes through (P = B ceil(T / 2048) partials) rounds a difference,
           a quotient and one fma of values no larger than Zmax: 4 u Zmax.
  var      through M2 = sum (z - mean)^2, never sum z^2:   d_var = ((20 + 6 M) u M2 + 2 d_mean sqrt(N M2) + N d_mean^2) / N.
           A segment's M2 about its own rounded mean m' is sum (z - m')^2 = M2_seg + n (m - m')^2, its terms are positive and
           each carries 3 roundings and at most 16 additions: 20 u; a merge adds positive terms with 6 more roundings; the error
           d_mean of a mean enters the between-segment term d^2 n_a n_b / n as 2 |d| d_mean, summed: 2 d_mean sqrt(N M2).
  running  r' = r + m (v - r) in one fma:  m d_v + 3 u (|r| + m |v - r|);  v = mean, or M2 / (N - 1) with d_var N / (N - 1) + 2 u v.
  a        rstd carries 4 u (eps rounded to fp32, add, sqrt, divide), zhat 6 u;  training: d_a = 6 u |zhat gamma| + u |a|;
           eval (scale = gamma rstd: 5 u; shift = beta - mean scale):  d_a = 5 u |z scale| + (5 u |mean scale| + u |shift|) + u |a|
  y        1.1 d_a + d_gate(a, y)                                                |silu'| <= 1.1
  silu'    q = 1 - s: d_q = 8 u s + u q;  r = 1 + a q: d_r = |a| d_q + u |r|;  p = s r: d_p = 9 u |p| + s d_r + 0.5 d_a   (|silu''| <= 0.5)
  da       |dy| d_p + u |da|
  dbeta    sum d_da + (N + 2) u sum |da|;     dgamma   sum (d_da |zhat| + 6 u |da zhat|) + (N + 2) u sum |da zhat|
  dz eval  |scale| d_da + 6 u |dz|
  dz train k1 = dbeta / N: d_k1 = d_dbeta / N + 2 u |k1|, k2 likewise;
           i = da - k1 - zhat k2:  d_i = d_da + d_k1 + u |da - k1| + |zhat| d_k2 + 6 u |zhat k2| + u |i|;   dz: |scale| d_i + 6 u |dz|
  dg       (K + 2) u sum_k |w_k dz|
  du       first half: s d_dg + 9 u |dg s|;   second: |u_a| s q d_dg + |dg u_a| (s d_q + 9 u s q) + 3 u |du|
  dw       sum |dz| d_g + (N + 2) u sum |dz g|;       dbias   (N + 2) u sum |dz|
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of fp32
TINY = 2.0 ** -126
K_GATE = 8.0            # see above
EPS = 1e-5
TILE = 1024             # positions of a row one workgroup of the conv kernels takes (csrc/conformer.hip: kTile)
SEGMENT = 2048          # floats of a row behind one partial of a reduction (csrc/conformer.hip: kRedSeg)
MAX_K = 64              # AGX_CONFORMER_MAX_K


def f64(*tensors):
    out = tuple(None if t is None else torch.as_tensor(t).detach().double() for t in tensors)
    return out[0] if len(out) == 1 else out


def sigmoid(v):
    return torch.sigmoid(v)


def silu(a):
    return a * sigmoid(a)


def silu_grad(a):
    s = sigmoid(a)
    return s * (1.0 + a * (1.0 - s))


def pads(k):
    left = (k - 1) // 2
    return left, k - 1 - left


def glu(u):
    c = u.shape[1] // 2
    return u[:, :c] * sigmoid(u[:, c:])


def shifted(v, k):
    """(K, B, C, T): v[.., t + j - left] for tap j, zeros outside [0, T)."""
    left, right = pads(k)
    t = v.shape[-1]
    vp = F.pad(v, (left, right))
    return torch.stack([vp[..., j:j + t] for j in range(k)])


def dwconv(g, w, bias):
    w = w.reshape(w.shape[0], -1)
    taps = shifted(g, w.shape[1])                                           # (K, B, C, T)
    return bias.reshape(1, -1, 1) + (w.t().reshape(w.shape[1], 1, -1, 1) * taps).sum(0)


def glu_dwconv(u, w, bias):
    return dwconv(glu(u), w, bias)


def _ch(v):
    return v.reshape(1, -1, 1)


def _sum_c(v):
    return v.sum((0, 2))


def correlate(dz, w):
    """dg[.., t] = sum_j w[:, j] dz[.., t + left - j], zeros outside [0, T)."""
    k = w.shape[1]
    left, right = pads(k)
    t = dz.shape[-1]
    dzp = F.pad(dz, (right, left))                     # dzp[i] = dz[i - right];  dz[t + left - j] = dzp[t + k - 1 - j]
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


def batch_stats(z):
    """(mean, biased var, M2) per channel over (B, T)."""
    n = z.shape[0] * z.shape[2]
    mean = _sum_c(z) / n
    m2 = _sum_c((z - _ch(mean)) ** 2)
    return mean, m2 / n, m2


def running_update(r_mean, r_var, mean, m2, n, momentum=0.1):
    return r_mean + momentum * (mean - r_mean), r_var + momentum * (m2 / (n - 1) - r_var)


def bn_parts(z, gamma, beta, mean, var, eps=EPS):
    rstd = 1.0 / torch.sqrt(var + eps)
    zhat = (z - _ch(mean)) * _ch(rstd)
    a = zhat * _ch(gamma) + _ch(beta)
    return dict(rstd=rstd, zhat=zhat, a=a, scale=gamma * rstd, shift=beta - mean * gamma * rstd)


def bn_silu(z, gamma, beta, mean, var, eps=EPS):
    return silu(bn_parts(z, gamma, beta, mean, var, eps)["a"])


def bn_silu_backward(dy, z, gamma, beta, mean, var, eps=EPS, training=True):
    """(dz, dgamma, dbeta) from the formulas."""
    p = bn_parts(z, gamma, beta, mean, var, eps)
    n = z.shape[0] * z.shape[2]
    da = dy * silu_grad(p["a"])
    dbeta, dgamma = _sum_c(da), _sum_c(da * p["zhat"])
    if training:
        dz = _ch(p["scale"]) * (da - _ch(dbeta) / n - p["zhat"] * _ch(dgamma) / n)
    else:
        dz = _ch(p["scale"]) * da
    return dz, dgamma, dbeta


# ------------------------------------------------------------------ bounds
def d_gate(x, g):
    """The bound of g = x s(v) given x."""
    return K_GATE * U * g.abs() + x.abs().clamp_min(1.0) * TINY


def bound_z(u, w, bias):
    w = w.reshape(w.shape[0], -1)
    k = w.shape[1]
    g = glu(u)
    wa = w.abs()
    return dwconv(d_gate(u[:, :w.shape[0]], g), wa, torch.zeros_like(bias)) + (k + 2) * U * dwconv(g.abs(), wa, bias.abs())


def _merges(b, t):
    p = b * math.ceil(t / SEGMENT)
    return min(p - 1, math.ceil(p / 64) + 6)


def bound_stats(z):
    """(d_mean, d_var) per channel."""
    b, _, t = z.shape
    n, m = b * t, _merges(b, t)
    _, _, m2 = batch_stats(z)
    zmax = z.abs().amax((0, 2))
    d_mean = (17 + 4 * m) * U * zmax
    d_var = ((20 + 6 * m) * U * m2 + 2 * d_mean * torch.sqrt(n * m2) + n * d_mean ** 2) / n
    return d_mean, d_var


def bound_running(z, r_mean, r_var, momentum=0.1):
    b, _, t = z.shape
    n = b * t
    mean, _, m2 = batch_stats(z)
    d_mean, d_var = bound_stats(z)
    unb = m2 / (n - 1)
    d_rm = momentum * d_mean + 3 * U * (r_mean.abs() + momentum * (mean - r_mean).abs())
    d_rv = momentum * (d_var * n / (n - 1) + 2 * U * unb) + 3 * U * (r_var.abs() + momentum * (unb - r_var).abs())
    return d_rm, d_rv


def bound_a(z, gamma, beta, mean, var, eps=EPS, training=True):
    p = bn_parts(z, gamma, beta, mean, var, eps)
    if training:
        return 6 * U * (p["zhat"] * _ch(gamma)).abs() + U * p["a"].abs()
    return 5 * U * (z * _ch(p["scale"])).abs() + _ch(5 * U * (mean * p["scale"]).abs() + U * p["shift"].abs()) + U * p["a"].abs()


def bound_silu(a, d_a=0.0):
    return 1.1 * d_a + d_gate(a, silu(a))


def bound_y(z, gamma, beta, mean, var, eps=EPS, training=True):
    return bound_silu(bn_parts(z, gamma, beta, mean, var, eps)["a"], bound_a(z, gamma, beta, mean, var, eps, training))


def bound_silu_grad(a, d_a=0.0):
    s = sigmoid(a)
    q = 1.0 - s
    d_q = K_GATE * U * s + U * q
    r = 1.0 + a * q
    d_r = a.abs() * d_q + U * r.abs()
    return (K_GATE + 1) * U * (s * r).abs() + s * d_r + 0.5 * d_a + (1.0 + a.abs()) * TINY


def bound_bn_backward(dy, z, gamma, beta, mean, var, eps=EPS, training=True):
    """(d_dz, d_dgamma, d_dbeta)."""
    p = bn_parts(z, gamma, beta, mean, var, eps)
    n = z.shape[0] * z.shape[2]
    zhat, scale = p["zhat"], _ch(p["scale"])
    da = dy * silu_grad(p["a"])
    d_da = dy.abs() * bound_silu_grad(p["a"], bound_a(z, gamma, beta, mean, var, eps, training)) + U * da.abs()
    d_dbeta = _sum_c(d_da) + (n + 2) * U * _sum_c(da.abs())
    d_dgamma = _sum_c(d_da * zhat.abs() + 6 * U * (da * zhat).abs()) + (n + 2) * U * _sum_c((da * zhat).abs())
    dz, dgamma, dbeta = bn_silu_backward(dy, z, gamma, beta, mean, var, eps, training)
    if not training:
        return scale.abs() * d_da + 6 * U * dz.abs(), d_dgamma, d_dbeta
    k1, k2 = _ch(dbeta) / n, _ch(dgamma) / n
    d_k1, d_k2 = _ch(d_dbeta) / n + 2 * U * k1.abs(), _ch(d_dgamma) / n + 2 * U * k2.abs()
    inner = da - k1 - zhat * k2
    d_i = d_da + d_k1 + U * (da - k1).abs() + zhat.abs() * d_k2 + 6 * U * (zhat * k2).abs() + U * inner.abs()
    return scale.abs() * d_i + 6 * U * dz.abs(), d_dgamma, d_dbeta


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
def layer_norm_ct(x, weight, bias, eps=1e-5):
    return F.layer_norm(x.transpose(1, 2), (x.shape[1],), weight, bias, eps).transpose(1, 2)


def linear_ct(x, weight, bias=None):
    weight = weight.reshape(weight.shape[0], -1)
    y = torch.einsum("oc,bct->bot", weight, x)
    return y if bias is None else y + _ch(bias)


def _factor(masks, site, like):
    """The dropout factor of ``site`` (None: 1), a tensor of ``like``'s shape."""
    return 1.0 if masks is None or masks.get(site) is None else masks[site].to(like.dtype)


def feed_forward(x, sd, prefix, act, masks=None, sites=("hid", "out")):
    """``FeedForward`` without its residual: LN -> Linear -> act -> dropout -> Linear -> dropout.  (B, dim, T)."""
    xn = layer_norm_ct(x, sd[prefix + "net.0.weight"], sd[prefix + "net.0.bias"])
    hid = act(linear_ct(xn, sd[prefix + "net.1.weight"], sd[prefix + "net.1.bias"]))
    hid = hid * _factor(masks, sites[0], hid)
    out = linear_ct(hid, sd[prefix + "net.4.weight"], sd[prefix + "net.4.bias"])
    return out * _factor(masks, sites[1], out)


def conv_block(x, sd, prefix, training, stats=None, mask=None, eps=EPS):
    """``ConformerConvBlock`` without a residual on (B, C, T).  ``stats``: a dict that receives mean, var, M2 of the batch (training
    mode)."""
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
    out = linear_ct(y, sd[prefix + "net.6.weight"], sd[prefix + "net.6.bias"])
    return out if mask is None else out * mask.to(out.dtype)


def attention(x, sd, prefix, heads, prob_factor=None, out_factor=None):
    """The ALiBi self-attention sub-block without its residual: LN -> q, k, v -> softmax(q k^T / sqrt(dh) - slope_h |i - j|) v -> W_o."""
    b, dim, t = x.shape
    xn = layer_norm_ct(x, sd[prefix + "norm.weight"], sd[prefix + "norm.bias"])
    q, k, v = (linear_ct(xn, sd[prefix + f"W_{n}.weight"]) for n in "qkv")
    dh = q.shape[1] // heads
    q, k, v = (m.reshape(b, heads, dh, t) for m in (q, k, v))
    slopes = 2.0 ** (-8.0 / torch.arange(heads, 0, -1, dtype=x.dtype))
    pos = torch.arange(t, dtype=x.dtype)
    bias = -(pos[:, None] - pos[None, :]).abs()[None] * slopes[:, None, None]
    pr = (torch.einsum("bhdi,bhdj->bhij", q, k) / dh ** 0.5 + bias).softmax(-1)
    if prob_factor is not None:
        pr = pr * prob_factor.to(x.dtype)
    o = torch.einsum("bhij,bhdj->bhdi", pr, v).reshape(b, heads * dh, t)
    o = linear_ct(o, sd[prefix + "W_o.weight"])
    return o if out_factor is None else o * out_factor.to(x.dtype)


def conformer_block(x, sd, heads, training, stats=None, masks=None):
    """``ConformerBlock`` on (B, dim, T).  ``masks``: the factors of the seven dropout sites by name -- ff1_hid, ff1_out, prob,
    attn_out, conv, ff2_hid, ff2_out -- or None."""
    m = masks or {}
    x = x + 0.5 * feed_forward(x, sd, "first_ff.", silu, m, ("ff1_hid", "ff1_out"))
    x = x + attention(x, sd, "attention.", heads, m.get("prob"), m.get("attn_out"))
    x = x + conv_block(x, sd, "conv_block.", training, stats, m.get("conv"))
    x = x + 0.5 * feed_forward(x, sd, "second_ff.", silu, m, ("ff2_hid", "ff2_out"))
    return layer_norm_ct(x, sd["layer_norm.weight"], sd["layer_norm.bias"])
