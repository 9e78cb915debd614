"""Float64 restatement of ``Snek`` / ``SnekReLU`` (networks/utils.py:44-105), written from the formulas, and the error bounds
the tests hold the fp32 kernels to.  x is (B, C, ...), alpha holds C elements or one; a = alpha[c], eps = 1e-6:

    inv = 1 / (a + eps)      theta = a x      sin2 = sin(2 theta)      sq = sin(theta)^2
    out       = (relu ? max(x, 0) : x) + inv sq
    dx        = dout ((relu ? [x >= 0] : 1) + a inv sin2)                 [x >= 0] is 1 at either zero: torch.clamp's gradient
    dalpha[c] = sum over batch and positions of  dout inv (x sin2 - inv sq)

``tests/test_snake_cpu.py`` pins these to the goldens of the reference, gradients included.

Bounds (u = 2^-24; every right-hand side is evaluated in float64 from the operands; second-order terms are left to the factor
2 the tests allow).  K_SIN is the absolute error, in units of u, of the device's sq and sin2 at the theta it was given.  The
kernels take (s, c) = sincosf(theta) from OCML, which is built to the OpenCL requirement of 4 ulp for sin and cos; an ulp of a
value in [-1, 1] is at most 2 u, so |ds|, |dc| <= 8 u, and
    sq   = fl(s s):        2 |s| 8 u + u               <= 17 u
    sin2 = 2 fl(s c):      2 ((|s| + |c|) 8 u + u / 2) <= (16 sqrt 2 + 1) u < 24 u          K_SIN = 24.
theta = fl(a x) is within u |a x| of a x; sq has Lipschitz constant 1 in theta and sin2 has 2.  inv = fl(1 / fl(a + eps)) with
eps rounded to fp32 is within 3 u |inv| of the exact one while |a + eps| >= eps, and fl(a inv) within 4 u |a inv|.

    out    |inv| (|a x| + K) u  +  4 u |inv sq|  +  u |out|
           (the sine; inv's rounding and one more for an evaluation that rounds the product; the final sum)
    g      |a inv| (2 |a x| + K) u  +  5 u |a inv sin2|  +  u |g|          g = dx / dout
    dx     |dout| d_g  +  u |dx|
    term   r = inv sq:  d_r = |inv| (|a x| + K) u + 4 u |r|
           w = x sin2 - r:  d_w = |x| (2 |a x| + K) u + d_r + u W
           t = inv w:  d_t = |inv| d_w + 4 u |inv| W
    dalpha sum |dout| d_t  +  (N + 2) u sum |dout| |inv| W          N = the number of summed terms
W is |w| for an evaluation that forms w per element before it sums (the kernels), and |x sin2| + |r| for one that sums the two
halves apart and subtracts the sums (autograd through the reference: ``split=True``).
"""
import math

import torch

U = 2.0 ** -24          # unit roundoff of fp32
K_SIN = 24.0            # see above
EPS = 1e-6
SEGMENT = 2048          # floats of a row behind one partial sum of the backward (csrc/snake.hip: kRedSeg)


def f64(*tensors):
    out = tuple(None if t is None else torch.as_tensor(t).detach().double() for t in tensors)
    return out[0] if len(out) == 1 else out


def _per_channel(alpha, x):
    """alpha as a tensor that broadcasts against x (B, C, ...)."""
    return alpha.reshape(-1).reshape((1, -1) + (1,) * (x.dim() - 2))


def _sum_to_alpha(v, channels):
    """Sum (B, C, ...) over everything but the channel (channels == C), or over everything (channels == 1)."""
    if channels == 1:
        return v.sum().reshape(1)
    return v.transpose(0, 1).reshape(channels, -1).sum(1)


def parts(x, alpha, relu, eps=EPS):
    """Every quantity of the formulas, in the dtype of the operands."""
    a = _per_channel(alpha, x)
    inv = 1.0 / (a + eps)
    theta = a * x
    sq, sin2 = torch.sin(theta) ** 2, torch.sin(2.0 * theta)
    base = torch.clamp(x, min=0.0) if relu else x
    mask = (x >= 0).to(x.dtype) if relu else torch.ones_like(x)
    r = inv * sq
    return dict(a=a + 0.0 * x, inv=inv + 0.0 * x, theta=theta, sq=sq, sin2=sin2, out=base + r, g=mask + a * inv * sin2, r=r,
                w=x * sin2 - r, xs=x * sin2)


def snake(x, alpha, relu, eps=EPS):
    return parts(x, alpha, relu, eps)["out"]


def snake_backward(x, alpha, dout, relu, eps=EPS):
    """(dx, dalpha) from the formulas; dalpha has alpha.numel() elements."""
    p = parts(x, alpha, relu, eps)
    return dout * p["g"], _sum_to_alpha(dout * p["inv"] * p["w"], alpha.numel())


def bounds(x, alpha, dout, relu, eps=EPS, split=False):
    """(d_out, d_dx, d_dalpha) of the module docstring for float64 operands."""
    p = parts(x, alpha, relu, eps)
    a, inv, th = p["a"].abs(), p["inv"].abs(), p["theta"].abs()
    d_out = inv * (th + K_SIN) * U + 4 * U * p["r"].abs() + U * p["out"].abs()
    d_g = a * inv * (2 * th + K_SIN) * U + 5 * U * (a * inv * p["sin2"]).abs() + U * p["g"].abs()
    d_dx = dout.abs() * d_g + U * (dout * p["g"]).abs()
    big_w = p["xs"].abs() + p["r"].abs() if split else p["w"].abs()
    d_r = inv * (th + K_SIN) * U + 4 * U * p["r"].abs()
    d_w = x.abs() * (2 * th + K_SIN) * U + d_r + U * big_w
    d_t = inv * d_w + 4 * U * inv * big_w
    channels = alpha.numel()
    n_terms = x.numel() // channels
    d_dalpha = _sum_to_alpha(dout.abs() * d_t, channels) + (n_terms + 2) * U * _sum_to_alpha(dout.abs() * inv * big_w, channels)
    return d_out, d_dx, d_dalpha


def partial_sums(x, alpha, dout, relu, eps=EPS):
    """What stage 1 of the backward leaves in its workspace: one sum per (row, segment of SEGMENT floats), rows = B * C."""
    p = parts(x, alpha, relu, eps)
    rows = x.shape[0] * x.shape[1]
    t = (dout * p["inv"] * p["w"]).reshape(rows, -1)
    segs = math.ceil(t.shape[1] / SEGMENT)
    pad = torch.zeros(rows, segs * SEGMENT - t.shape[1], dtype=t.dtype)
    return torch.cat([t, pad], dim=1).reshape(rows, segs, SEGMENT).sum(2).reshape(-1)
