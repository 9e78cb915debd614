"""CPU checker for the dropout paths of the transformer block (TEST INFRASTRUCTURE, beside the frozen ``oracle/``).

The masks come from ``tests/philox.py`` (the definition of ``include/agx.h``) and enter as constants; everything else is the
float64 definition of ``tests/cross_attention_ref.py`` / ``oracle.attention`` with the masks applied where
networks/transformers.py applies ``nn.Dropout``: to the softmax (:185), to the W_o output (:191), behind the GELU (:217) and
to the FFN output (:219).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle import attention as oattn
from tests import philox

Tensor = torch.Tensor


def attention_factor(seed: int, stream_id: int, p: float, b: int, heads: int, tq: int, tk: int, dtype=torch.float64) -> Tensor:
    """(b, heads, tq, tk): scale where the element is kept, 0 where it is dropped (scale = float32(1 / (1 - p)), exactly)."""
    keep = torch.from_numpy(philox.attention_keep(seed, stream_id, p, b, heads, tq, tk))
    return keep.to(dtype) * float(philox.thresh_scale(p)[1])


def elementwise_factor(seed: int, stream_id: int, p: float, shape, dtype=torch.float64) -> Tensor:
    """The factors of a contiguous tensor of ``shape``, indexed by the linear position."""
    n = 1
    for s in shape:
        n *= int(s)
    keep = torch.from_numpy(philox.elementwise_keep(seed, stream_id, p, n)).reshape(tuple(shape))
    return keep.to(dtype) * float(philox.thresh_scale(p)[1])


def drop_core(q: Tensor, kv: Tensor, slopes: Tensor, heads: int, head_dim: int, scale_div: float, factor: Tensor) -> Tensor:
    """``cross_core`` with the probabilities multiplied by ``factor`` (b, heads, tq, tk) behind the softmax:
    q (B, H*Dh, Tq), kv (B, 2*H*Dh, Tk) -> (B, H*Dh, Tq), in the dtype of ``q``; differentiable."""
    b, _, tq = q.shape
    tk = kv.shape[-1]
    qh = q.reshape(b, heads, head_dim, tq)
    kh, vh = (z.reshape(b, heads, head_dim, tk) for z in kv.chunk(2, dim=1))
    i = torch.arange(tq, dtype=q.dtype).reshape(-1, 1)
    j = torch.arange(tk, dtype=q.dtype).reshape(1, -1)
    bias = -(i - j).abs().unsqueeze(0) * slopes.to(q.dtype).reshape(-1, 1, 1)
    s = torch.einsum("bhdi,bhdj->bhij", qh, kh) / scale_div + bias
    return torch.einsum("bhij,bhdj->bhdi", s.softmax(-1) * factor.to(q.dtype), vh).reshape(b, heads * head_dim, tq)


def dropout_transformer(x: Tensor, y: Optional[Tensor], sd: Dict[str, Tensor], heads: int, depth: int, p: float, seed: int) -> Tensor:
    """``Transformer(dropout=p).train()`` on channel-major tensors: x (B, dim, Tx), y (B, dim, Ty) or None -> (B, dim, Tx).
    Layer ``l`` draws its four masks from ``seed`` with the stream ids 4 l + {0: probabilities, 1: attention output,
    2: FFN hidden, 3: FFN output}; the three elementwise masks are indexed by the linear position in the contiguous
    channel-major tensor.  Layer 0 cross-attends to ``y`` when it is given."""
    b, dim, tx = x.shape
    h = x.transpose(1, 2)                                     # (B, T, dim): the reference's layout
    for layer in range(depth):
        pa, pf = f"layers.{layer}.0.", f"layers.{layer}.1."
        src = y.transpose(1, 2) if (layer == 0 and y is not None) else None
        xn = F.layer_norm(h, (dim,), sd[pa + "norm.weight"], sd[pa + "norm.bias"])
        kin = xn if src is None else src                      # keys and values: LN(x), or y as given (transformers.py:170)
        tk = kin.shape[1]
        q, k, v = F.linear(xn, sd[pa + "W_q.weight"]), F.linear(kin, sd[pa + "W_k.weight"]), F.linear(kin, sd[pa + "W_v.weight"])
        dh = q.shape[-1] // heads
        q = q.reshape(b, tx, heads, dh).transpose(1, 2)
        k, v = (z.reshape(b, tk, heads, dh).transpose(1, 2) for z in (k, v))
        s = q @ k.transpose(-1, -2) / (dh ** 0.5) + oattn.alibi_bias(heads, tx, tk).to(x.dtype).unsqueeze(0)
        pr = s.softmax(dim=-1) * attention_factor(seed, 4 * layer + 0, p, b, heads, tx, tk, x.dtype)
        o = F.linear((pr @ v).transpose(1, 2).reshape(b, tx, heads * dh), sd[pa + "W_o.weight"])
        h = h + o * elementwise_factor(seed, 4 * layer + 1, p, (b, dim, tx), x.dtype).transpose(1, 2)
        xn = F.layer_norm(h, (dim,), sd[pf + "net.0.weight"], sd[pf + "net.0.bias"])
        hid = F.gelu(F.linear(xn, sd[pf + "net.1.weight"], sd[pf + "net.1.bias"]))
        hid = hid * elementwise_factor(seed, 4 * layer + 2, p, (b, hid.shape[-1], tx), x.dtype).transpose(1, 2)
        out = F.linear(hid, sd[pf + "net.4.weight"], sd[pf + "net.4.bias"])
        h = h + out * elementwise_factor(seed, 4 * layer + 3, p, (b, dim, tx), x.dtype).transpose(1, 2)
    return h.transpose(1, 2)
