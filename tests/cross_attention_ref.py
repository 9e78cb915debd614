"""CPU checker for ALiBi cross-attention (TEST INFRASTRUCTURE, beside the frozen ``oracle/``).

networks/transformers.py:157-191 with ``cross_attention``: queries from ``LN(x)``, keys and values from the second sequence
``y`` as given (no LayerNorm, :170), the bias ``-slope_h * |i - j|`` on the absolute positions (``Alibi._create_M`` :45-77 --
the reference stores it transposed, which changes no value).  Built from ``oracle.attention``; pinned against the g9 fixtures
by ``tests/test_cross_attention_cpu.py``.
"""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn.functional as F

from oracle import attention as oattn

Tensor = torch.Tensor


def cross_core(q: Tensor, kv: Tensor, slopes: Tensor, heads: int, head_dim: int, scale_div: float) -> Tensor:
    """The definition on the kernels' layouts, in the dtype of ``q`` (float64 in the op tests; differentiable):
    q (B, H*Dh, Tq), kv (B, 2*H*Dh, Tk) -> (B, H*Dh, Tq)."""
    b, _, tq = q.shape
    tk = kv.shape[-1]
    qh = q.reshape(b, heads, head_dim, tq)
    kh, vh = (z.reshape(b, heads, head_dim, tk) for z in kv.chunk(2, dim=1))
    i = torch.arange(tq, dtype=q.dtype).reshape(-1, 1)
    j = torch.arange(tk, dtype=q.dtype).reshape(1, -1)
    bias = -(i - j).abs().unsqueeze(0) * slopes.to(q.dtype).reshape(-1, 1, 1)
    s = torch.einsum("bhdi,bhdj->bhij", qh, kh) / scale_div + bias
    return torch.einsum("bhij,bhdj->bhdi", s.softmax(-1), vh).reshape(b, heads * head_dim, tq)


def cross_attention(x: Tensor, y: Tensor, sd: Dict[str, Tensor], prefix: str, n_heads: int) -> Tensor:
    """``Attention.forward(x, y)`` of a cross-attention layer: x (B, Tx, dim), y (B, Ty, dim) -> (B, Tx, dim)."""
    b, tx, dim = x.shape
    ty = y.shape[1]
    xn = F.layer_norm(x, (dim,), sd[prefix + "norm.weight"], sd[prefix + "norm.bias"])
    q = F.linear(xn, sd[prefix + "W_q.weight"], sd.get(prefix + "W_q.bias"))
    k = F.linear(y, sd[prefix + "W_k.weight"], sd.get(prefix + "W_k.bias"))
    v = F.linear(y, sd[prefix + "W_v.weight"], sd.get(prefix + "W_v.bias"))
    dh = q.shape[-1] // n_heads
    q = q.reshape(b, tx, n_heads, dh).transpose(1, 2)
    k, v = (z.reshape(b, ty, n_heads, dh).transpose(1, 2) for z in (k, v))
    s = q @ k.transpose(-1, -2) / (dh ** 0.5) + oattn.alibi_bias(n_heads, tx, ty).to(x.dtype).unsqueeze(0)
    o = (s.softmax(dim=-1) @ v).transpose(1, 2).reshape(b, tx, n_heads * dh)
    return F.linear(o, sd[prefix + "W_o.weight"], sd.get(prefix + "W_o.bias"))


def cross_transformer(x: Tensor, y: Tensor, sd: Dict[str, Tensor], n_heads: int, depth: int = 1, prefix: str = "") -> Tensor:
    """``Transformer(context_y=...).forward(x, y)``: layer 0 cross-attends to ``y`` (transformers.py:272-273), later layers
    are ALiBi self-attention (the build-defined depth > 1)."""
    for layer in range(depth):
        p = f"{prefix}layers.{layer}."
        a = cross_attention(x, y, sd, p + "0.", n_heads) if layer == 0 else oattn.attention(x, sd, p + "0.", n_heads)
        x = x + a
        x = x + oattn.feed_forward(x, sd, p + "1.")
    return x
