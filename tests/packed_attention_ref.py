"""CPU checker for packed variable-length batches (TEST INFRASTRUCTURE, beside the frozen ``oracle/``): sequences concatenated
along the time axis, ``cu[s]`` the first column of sequence ``s`` and ``cu[-1]`` the end of the last.

A packed batch has no definition of its own: sequence ``s`` of the result IS the existing definition applied to that sequence
cropped out of the concatenation, and the columns no sequence owns (the slack behind ``cu[-1]``) are zero.  So the checkers
crop, call the frozen checkers (``tests/cross_attention_ref.cross_core``, ``oracle.attention.transformer``,
``tests/cross_attention_ref.cross_transformer``) sequence by sequence, and concatenate.  What lies outside a sequence is never
read for it.  Pinned by ``tests/test_packed_attention_cpu.py``.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from oracle import attention as oattn
from tests.cross_attention_ref import cross_core, cross_transformer

Tensor = torch.Tensor


def cu_of(lengths: Sequence[int]) -> list:
    """[0, l0, l0 + l1, ...]"""
    cu = [0]
    for v in lengths:
        assert int(v) >= 0
        cu.append(cu[-1] + int(v))
    return cu


def _spans(cu: Sequence[int], n: int) -> list:
    cu = [int(v) for v in cu]
    assert cu[0] == 0 and all(b >= a for a, b in zip(cu, cu[1:])) and cu[-1] <= n, (cu, n)
    return list(zip(cu, cu[1:]))


def packed_core(q: Tensor, kv: Tensor, slopes: Tensor, heads: int, head_dim: int, scale_div: float, cu_q: Sequence[int],
                cu_k: Sequence[int]) -> Tensor:
    """q (1, H*Dh, Nq), kv (1, 2*H*Dh, Nk) -> (1, H*Dh, Nq) in the dtype of ``q`` (differentiable): the columns of sequence s are
    ``cross_core`` of ``q[:, :, cu_q[s]:cu_q[s+1]]`` and ``kv[:, :, cu_k[s]:cu_k[s+1]]``; zeros for a sequence without keys
    and in the columns behind ``cu_q[-1]``."""
    assert q.shape[0] == 1 and kv.shape[0] == 1 and len(cu_q) == len(cu_k)
    nq = q.shape[-1]
    parts = []
    for (a, b), (c, d) in zip(_spans(cu_q, nq), _spans(cu_k, kv.shape[-1])):
        if b == a:
            continue
        if d == c:
            parts.append(q.new_zeros(1, q.shape[1], b - a))
        else:
            parts.append(cross_core(q[:, :, a:b], kv[:, :, c:d], slopes, heads, head_dim, scale_div))
    parts.append(q.new_zeros(1, q.shape[1], nq - int(cu_q[-1])))
    return torch.cat(parts, dim=-1)


def packed_transformer(x: Tensor, y: Optional[Tensor], sd: Dict[str, Tensor], n_heads: int, depth: int, cu: Sequence[int],
                       y_cu: Optional[Sequence[int]] = None) -> Tensor:
    """Reference layout: x (1, N, dim) [, y (1, Ny, dim)] -> (1, N, dim).  The rows of sequence s are
    ``oracle.attention.transformer`` (``y`` None) or ``cross_transformer`` of that sequence (and of sequence s of ``y``) alone;
    zeros behind ``cu[-1]``.  An empty second sequence has no frozen definition and is not offered (asserted)."""
    assert x.shape[0] == 1
    n = x.shape[1]
    spans = _spans(cu, n)
    yspans = [None] * len(spans) if y is None else _spans(y_cu, y.shape[1])
    assert len(yspans) == len(spans)
    parts = []
    for (a, b), ys in zip(spans, yspans):
        if b == a:
            continue
        if y is None:
            parts.append(oattn.transformer(x[:, a:b], sd, n_heads, depth))
        else:
            assert ys[1] > ys[0], "an empty second sequence has no frozen definition"
            parts.append(cross_transformer(x[:, a:b], y[:, ys[0]:ys[1]], sd, n_heads, depth))
    parts.append(x.new_zeros(1, n - int(cu[-1]), x.shape[2]))
    return torch.cat(parts, dim=1)


def pack_ref(x: Tensor, lengths: Sequence[int], total: Optional[int] = None) -> Tensor:
    """(B, C, T) -> (1, C, total): the valid columns of every row back to back, zeros behind them."""
    lengths = [int(v) for v in lengths]
    n = sum(lengths) if total is None else int(total)
    parts = [x[r:r + 1, :, :lengths[r]] for r in range(x.shape[0])] + [x.new_zeros(1, x.shape[1], n - sum(lengths))]
    return torch.cat(parts, dim=-1)


def unpack_ref(xp: Tensor, cu: Sequence[int], t: int) -> Tensor:
    """(1, C, N) -> (B, C, t): row b is the columns of sequence b, zeros behind them."""
    rows = []
    for a, b in _spans(cu, xp.shape[-1]):
        rows.append(torch.cat([xp[:, :, a:b], xp.new_zeros(1, xp.shape[1], t - (b - a))], dim=-1))
    return torch.cat(rows, dim=0)


# (kind, H, Dh, q_lens, k_lens, nq, max_q): the smallest shapes that cross every boundary the kernels have -- the 64-key block,
# the 128-query workgroup, the 16-query dQ block, the three head-dim tiles and a head dim that fills none, starts at unaligned
# columns, lengths 0, 1, 64 and 65.  "self" runs on one (1, 3*H*Dh, N) qkv tensor with cu_k = cu_q.  nq is the capacity of the
# packed query tensor (None: the sum of the lengths) and max_q the bound passed to the kernels (None: the longest sequence):
# case 4 has 5 slack columns and a bound that leaves whole empty workgroups.
CASES = [
    ("self", 2, 16, [37, 1, 20], None, None, None),
    ("self", 2, 64, [130, 64, 0, 65], None, None, None),
    ("self", 2, 128, [257, 100], None, None, None),
    ("self", 2, 64, [5, 70], None, 80, 128),
    ("cross", 3, 20, [70, 5, 33], [200, 64, 129], None, None),
    ("cross", 2, 100, [130, 17], [1, 65], None, None),
    ("cross", 1, 8, [5, 5], [0, 9], None, None),
]
CASE_IDS = [f"{i + 1}-{c[0]}-H{c[1]}Dh{c[2]}-{'+'.join(map(str, c[3]))}" for i, c in enumerate(CASES)]


def case_shape(case):
    """(kind, heads, dh, q_lens, k_lens, nq, nk, max_q, max_k) with the defaults of ``CASES`` filled in."""
    kind, heads, dh, ql, kl, nq, max_q = case
    kl = ql if kl is None else kl
    nq = sum(ql) if nq is None else nq
    nk = nq if kind == "self" else sum(kl)
    max_q = max(ql) if max_q is None else max_q
    max_k = max_q if kind == "self" else max(kl)
    return kind, heads, dh, ql, kl, nq, nk, max_q, max_k


def case_inputs(heads: int, dh: int, nq: int, nk: int):
    """(q, kv, dout, slopes) in float32 on the CPU: q (1, H*Dh, nq), kv (1, 2*H*Dh, nk), dout (1, H*Dh, nq)."""
    gen = torch.Generator().manual_seed(1000 * nq + 10 * nk + dh)
    q = 0.7 * torch.randn(1, heads * dh, nq, generator=gen)
    kv = 0.7 * torch.randn(1, 2 * heads * dh, nk, generator=gen)
    dout = torch.randn(1, heads * dh, nq, generator=gen)
    return q, kv, dout, oattn.alibi_slopes(heads)
