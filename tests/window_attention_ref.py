"""CPU checker for sliding-window causal ALiBi self-attention (TEST INFRASTRUCTURE, beside the frozen ``oracle/``).

Build-defined, like the causal form of ``tests/causal_attention_ref.py`` that it narrows: the query at absolute position
``p = i + q_pos0`` sees the keys ``max(0, p - W + 1) <= j <= p`` at the bias ``-slope_h * (p - j)``.  Everything here is
``causal_attention_ref`` with the keys ``j < p - W + 1`` masked as well; ``tests/test_window_attention_cpu.py`` pins
``window_core`` to ``causal_core``: query ``i`` of the windowed definition is the last query of the causal definition on the
keys ``lo .. i``, ``lo = max(0, i - W + 1)``.
"""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn.functional as F

from oracle import attention as oattn

Tensor = torch.Tensor


def window_core(q: Tensor, kv: Tensor, slopes: Tensor, heads: int, head_dim: int, scale_div: float, window: int,
                q_pos0: int = 0) -> Tensor:
    """The definition on the kernels' layouts, in the dtype of ``q`` (float64 in the op tests; differentiable):
    q (B, H*Dh, Tq) at the absolute positions ``q_pos0 + i``, kv (B, 2*H*Dh, Tk) the keys 0 .. Tk - 1 -> (B, H*Dh, Tq)."""
    b, _, tq = q.shape
    tk = kv.shape[-1]
    qh = q.reshape(b, heads, head_dim, tq)
    kh, vh = (z.reshape(b, heads, head_dim, tk) for z in kv.chunk(2, dim=1))
    i = torch.arange(tq, dtype=q.dtype).reshape(-1, 1) + q_pos0
    j = torch.arange(tk, dtype=q.dtype).reshape(1, -1)
    bias = -(i - j).unsqueeze(0) * slopes.to(q.dtype).reshape(-1, 1, 1)
    s = torch.einsum("bhdi,bhdj->bhij", qh, kh) / scale_div + bias
    s = s.masked_fill(((j > i) | (j < i - window + 1)).unsqueeze(0).unsqueeze(0), float("-inf"))
    return torch.einsum("bhij,bhdj->bhdi", s.softmax(-1), vh).reshape(b, heads * head_dim, tq)


def window_attention(x: Tensor, sd: Dict[str, Tensor], prefix: str, n_heads: int, window: int) -> Tensor:
    """``Attention(causal=True, window=W).forward(x)``: ``causal_attention`` with the keys ``j < i - W + 1`` masked too.
    x (B, T, dim); T is not limited by a context here (the bias is evaluated, not looked up)."""
    b, t, dim = x.shape
    xn = F.layer_norm(x, (dim,), sd[prefix + "norm.weight"], sd[prefix + "norm.bias"])
    q = F.linear(xn, sd[prefix + "W_q.weight"], sd.get(prefix + "W_q.bias"))
    k = F.linear(xn, sd[prefix + "W_k.weight"], sd.get(prefix + "W_k.bias"))
    v = F.linear(xn, sd[prefix + "W_v.weight"], sd.get(prefix + "W_v.bias"))
    dh = q.shape[-1] // n_heads
    q, k, v = (z.reshape(b, t, n_heads, dh).transpose(1, 2) for z in (q, k, v))
    s = q @ k.transpose(-1, -2) / (dh ** 0.5) + oattn.alibi_bias(n_heads, t, t).to(x.dtype).unsqueeze(0)   # j <= i: |i - j| = i - j
    hidden = torch.ones(t, t, dtype=torch.bool).triu(1) | torch.ones(t, t, dtype=torch.bool).tril(-window)
    s = s.masked_fill(hidden, float("-inf"))
    o = (s.softmax(dim=-1) @ v).transpose(1, 2).reshape(b, t, n_heads * dh)
    return F.linear(o, sd[prefix + "W_o.weight"], sd.get(prefix + "W_o.bias"))


def window_transformer(x: Tensor, sd: Dict[str, Tensor], n_heads: int, window: int, depth: int = 1, prefix: str = "") -> Tensor:
    """``Transformer(causal=True, window=W).forward(x)``: every layer is windowed self-attention followed by the reference's FFN."""
    for layer in range(depth):
        p = f"{prefix}layers.{layer}."
        x = x + window_attention(x, sd, p + "0.", n_heads, window)
        x = x + oattn.feed_forward(x, sd, p + "1.")
    return x
