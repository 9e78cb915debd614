"""CPU checker for causal ALiBi self-attention (TEST INFRASTRUCTURE, beside the frozen ``oracle/``).

Build-defined: the reference's ``Alibi`` (networks/transformers.py:7-93) is symmetric and has no causal branch.  The causal
form is the standard one-sided ALiBi: the query at absolute position ``p = i + q_pos0`` sees the keys ``j <= p`` at the bias
``-slope_h * (p - j)`` -- the reference's ``-slope_h * |p - j|`` restricted to the keys it may see.  Built from
``oracle.attention`` plus the mask; pinned against ``tests/cross_attention_ref.cross_core`` (itself pinned against the g9
fixtures) by ``tests/test_causal_attention_cpu.py``: the last query of a prefix sees the whole prefix at distances ``i - j``.
"""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn.functional as F

from oracle import attention as oattn

Tensor = torch.Tensor


def causal_core(q: Tensor, kv: Tensor, slopes: Tensor, heads: int, head_dim: int, scale_div: float, q_pos0: int = 0) -> Tensor:
    """The definition on the kernels' layouts, in the dtype of ``q`` (float64 in the op tests; differentiable):
    q (B, H*Dh, Tq) at the absolute positions ``q_pos0 + i``, kv (B, 2*H*Dh, Tk) -> (B, H*Dh, Tq)."""
    b, _, tq = q.shape
    tk = kv.shape[-1]
    qh = q.reshape(b, heads, head_dim, tq)
    kh, vh = (z.reshape(b, heads, head_dim, tk) for z in kv.chunk(2, dim=1))
    i = torch.arange(tq, dtype=q.dtype).reshape(-1, 1) + q_pos0
    j = torch.arange(tk, dtype=q.dtype).reshape(1, -1)
    bias = -(i - j).unsqueeze(0) * slopes.to(q.dtype).reshape(-1, 1, 1)
    s = torch.einsum("bhdi,bhdj->bhij", qh, kh) / scale_div + bias
    s = s.masked_fill((j > i).unsqueeze(0).unsqueeze(0), float("-inf"))
    return torch.einsum("bhij,bhdj->bhdi", s.softmax(-1), vh).reshape(b, heads * head_dim, tq)


def causal_attention(x: Tensor, sd: Dict[str, Tensor], prefix: str, n_heads: int) -> Tensor:
    """``Attention(causal=True).forward(x)``: ``oracle.attention.attention`` with the keys ``j > i`` masked.  x (B, T, dim)."""
    b, t, dim = x.shape
    xn = F.layer_norm(x, (dim,), sd[prefix + "norm.weight"], sd[prefix + "norm.bias"])
    q = F.linear(xn, sd[prefix + "W_q.weight"], sd.get(prefix + "W_q.bias"))
    k = F.linear(xn, sd[prefix + "W_k.weight"], sd.get(prefix + "W_k.bias"))
    v = F.linear(xn, sd[prefix + "W_v.weight"], sd.get(prefix + "W_v.bias"))
    dh = q.shape[-1] // n_heads
    q, k, v = (z.reshape(b, t, n_heads, dh).transpose(1, 2) for z in (q, k, v))
    s = q @ k.transpose(-1, -2) / (dh ** 0.5) + oattn.alibi_bias(n_heads, t, t).to(x.dtype).unsqueeze(0)   # j <= i: |i - j| = i - j
    future = torch.ones(t, t, dtype=torch.bool).triu(1)
    s = s.masked_fill(future, float("-inf"))
    o = (s.softmax(dim=-1) @ v).transpose(1, 2).reshape(b, t, n_heads * dh)
    return F.linear(o, sd[prefix + "W_o.weight"], sd.get(prefix + "W_o.bias"))


def causal_transformer(x: Tensor, sd: Dict[str, Tensor], n_heads: int, depth: int = 1, prefix: str = "") -> Tensor:
    """``Transformer(causal=True).forward(x)``: every layer is causal self-attention followed by the reference's FFN."""
    for layer in range(depth):
        p = f"{prefix}layers.{layer}."
        x = x + causal_attention(x, sd, p + "0.", n_heads)
        x = x + oattn.feed_forward(x, sd, p + "1.")
    return x
