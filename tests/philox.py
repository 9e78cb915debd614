"""CPU mirror of the dropout masks of ``include/agx.h`` ("Dropout masks"), in vectorised numpy (TEST INFRASTRUCTURE).

Philox4x32-10 with the standard constants; ``thresh_scale`` is the keep rule; ``attention_keep`` and ``elementwise_keep`` are
the two counter packings.  ``tests/test_dropout_cpu.py`` pins the generator against three known-answer vectors; the GPU tests
compare the kernels' masks with this mirror element by element.
"""
from __future__ import annotations

import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Four uint32 arrays (broadcast together) -> the four output words, uint32 arrays of the broadcast shape."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & _MASK for v in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + np.uint64(W0)) & _MASK, (k1 + np.uint64(W1)) & _MASK
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def thresh_scale(p: float):
    """(thresh, scale): keep iff word >= thresh = min(2^32 - 1, floor(p 2^32 + 1/2)); scale = float32(1 / (1 - p))."""
    assert 0.0 <= p < 1.0
    return min(2 ** 32 - 1, int(math.floor(p * 2.0 ** 32 + 0.5))), np.float32(1.0 / (1.0 - p))


def _key(seed: int):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def attention_words(seed: int, stream_id: int, b: int, heads: int, tq: int, tk: int) -> np.ndarray:
    """uint32 (b, heads, tq, tk): the word of element (b, h, i, j) -- counter (j >> 2, i, b * heads + h, stream_id), word j & 3."""
    nq = (tk + 3) // 4
    bh = np.arange(b * heads, dtype=np.uint64).reshape(-1, 1, 1)
    i = np.arange(tq, dtype=np.uint64).reshape(1, -1, 1)
    jq = np.arange(nq, dtype=np.uint64).reshape(1, 1, -1)
    words = np.stack(philox4x32_10(jq, i, bh, stream_id, *_key(seed)), axis=-1)      # (b h, tq, nq, 4)
    return words.reshape(b, heads, tq, 4 * nq)[..., :tk]


def attention_keep(seed: int, stream_id: int, p: float, b: int, heads: int, tq: int, tk: int) -> np.ndarray:
    return attention_words(seed, stream_id, b, heads, tq, tk) >= np.uint32(thresh_scale(p)[0])


def elementwise_words(seed: int, stream_id: int, n: int) -> np.ndarray:
    """uint32 (n,): the word of linear index e -- counter (low32(e >> 2), high32(e >> 2), 0, stream_id), word e & 3."""
    qd = np.arange((n + 3) // 4, dtype=np.uint64)
    words = np.stack(philox4x32_10(qd & _MASK, qd >> np.uint64(32), 0, stream_id, *_key(seed)), axis=-1)
    return words.reshape(-1)[:n]


def elementwise_keep(seed: int, stream_id: int, p: float, n: int) -> np.ndarray:
    return elementwise_words(seed, stream_id, n) >= np.uint32(thresh_scale(p)[0])
