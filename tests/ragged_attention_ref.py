"""CPU checker for ragged batches (TEST INFRASTRUCTURE, beside the frozen ``oracle/``): a valid length per batch row for the
queries and for the keys, padding on the right.

A ragged batch has no definition of its own: row ``b`` of the result IS the existing definition applied to row ``b`` cropped to
its lengths, with zeros behind it.  So both checkers crop, call the frozen checkers (``tests/cross_attention_ref.cross_core``,
``oracle.attention.transformer``, ``tests/cross_attention_ref.cross_transformer``) row by row, and pad.  What lies beyond a
length is never read: it may hold anything.  Pinned by ``tests/test_ragged_attention_cpu.py``.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch
import torch.nn.functional as F

from oracle import attention as oattn
from tests.cross_attention_ref import cross_core, cross_transformer

Tensor = torch.Tensor


def _lens(lengths: Optional[Sequence[int]], batch: int, t: int) -> list:
    if lengths is None:
        return [t] * batch
    lengths = [int(v) for v in lengths]
    assert len(lengths) == batch and all(0 <= v <= t for v in lengths), (lengths, batch, t)
    return lengths


def ragged_core(q: Tensor, kv: Tensor, slopes: Tensor, heads: int, head_dim: int, scale_div: float,
                q_len: Optional[Sequence[int]] = None, k_len: Optional[Sequence[int]] = None) -> Tensor:
    """q (B, H*Dh, Tq), kv (B, 2*H*Dh, Tk) -> (B, H*Dh, Tq) in the dtype of ``q`` (differentiable): row b is ``cross_core`` of
    ``q[b, :, :q_len[b]]`` and ``kv[b, :, :k_len[b]]``, zeros at ``i >= q_len[b]`` and everywhere when ``k_len[b] == 0``.
    Rows of equal lengths are cropped and passed to ``cross_core`` as one sub-batch (its rows are independent), so with all
    lengths full this IS one ``cross_core`` call on the given tensors, bit for bit."""
    b, c, tq = q.shape
    ql, kl = _lens(q_len, b, tq), _lens(k_len, b, kv.shape[-1])
    rows = [None] * b
    for lens in sorted(set(zip(ql, kl))):       # rows of equal lengths go through cross_core together: all full = one call
        group = [r for r in range(b) if (ql[r], kl[r]) == lens]
        if 0 in lens:
            o = q.new_zeros(len(group), c, tq)
        else:
            at = slice(None) if len(group) == b else group
            o = F.pad(cross_core(q[at, :, :lens[0]], kv[at, :, :lens[1]], slopes, heads, head_dim, scale_div), (0, tq - lens[0]))
        for n, r in enumerate(group):
            rows[r] = o[n:n + 1]
    return torch.cat(rows, dim=0)


def ragged_transformer(x: Tensor, y: Optional[Tensor], sd: Dict[str, Tensor], n_heads: int, depth: int,
                       lengths: Optional[Sequence[int]] = None, y_lengths: Optional[Sequence[int]] = None) -> Tensor:
    """Reference layout: x (B, T, dim) [, y (B, Ty, dim)] -> (B, T, dim).  Row b is ``oracle.attention.transformer`` (``y`` None)
    or ``cross_transformer`` of the row cropped to ``lengths[b]`` (and ``y_lengths[b]``), zeros behind it.  A row of length 0
    is all zeros.  A cross row whose ``y`` is empty attends to nothing in layer 0: the attention adds 0 there, which is what
    the kernels define -- the frozen checker has no such case, so it is not offered here (asserted)."""
    b, t, dim = x.shape
    xl = _lens(lengths, b, t)
    yl = None if y is None else _lens(y_lengths, b, y.shape[1])
    rows = []
    for r in range(b):
        if xl[r] == 0:
            rows.append(x.new_zeros(1, t, dim))
            continue
        xr = x[r:r + 1, :xl[r]]
        if y is None:
            o = oattn.transformer(xr, sd, n_heads, depth)
        else:
            assert yl[r] > 0, "an empty second sequence has no frozen definition"
            o = cross_transformer(xr, y[r:r + 1, :yl[r]], sd, n_heads, depth)
        rows.append(F.pad(o, (0, 0, 0, t - xl[r])))
    return torch.cat(rows, dim=0)


# (kind, B, H, Dh, tq, tk, q_len, k_len): the smallest shapes that cross every boundary the kernels have -- the 64-key block,
# the 128-query workgroup, the 16-query dQ block, the three head-dim tiles and a head dim that fills no tile, lengths 0, 1, 64,
# 65 and full.  "self" runs on one (B, 3*H*Dh, T) qkv tensor with k_len = q_len.  Case 3 leaves one row with whole empty
# trailing workgroups and key blocks.
CASES = [
    ("self", 3, 2, 16, 37, 37, [37, 1, 20], [37, 1, 20]),
    ("self", 4, 2, 64, 130, 130, [130, 64, 65, 0], [130, 64, 65, 0]),
    ("self", 2, 2, 128, 257, 257, [257, 100], [257, 100]),
    ("cross", 3, 3, 20, 70, 200, [70, 5, 33], [200, 64, 129]),
    ("cross", 2, 2, 100, 130, 65, [130, 17], [1, 65]),
    ("cross", 2, 1, 8, 5, 9, [5, 5], [0, 9]),
]
CASE_IDS = [f"{i + 1}-{c[0]}-B{c[1]}H{c[2]}Dh{c[3]}-{c[4]}x{c[5]}" for i, c in enumerate(CASES)]


def case_inputs(b: int, heads: int, dh: int, tq: int, tk: int):
    """(q, kv, dout, slopes) in float32 on the CPU, generated as ``tests/test_gpu_cross_attention._inputs``."""
    gen = torch.Generator().manual_seed(1000 * tq + 10 * tk + dh)
    q = 0.7 * torch.randn(b, heads * dh, tq, generator=gen)
    kv = 0.7 * torch.randn(b, 2 * heads * dh, tk, generator=gen)
    dout = torch.randn(b, heads * dh, tq, generator=gen)
    return q, kv, dout, oattn.alibi_slopes(heads)


def pad_mask(lengths: Sequence[int], t: int) -> Tensor:
    """(B, 1, t) bool: True at the padded positions ``i >= lengths[b]``."""
    return torch.arange(t).reshape(1, 1, t) >= torch.tensor(list(lengths)).reshape(-1, 1, 1)
