"""Float64 / exact mirrors of the code-prior kernels (include/agx.h "Code prior"; TEST INFRASTRUCTURE).

``embed`` is the binary32 chain of ``agx_codes_embed`` (exact: the GPU test asks for equality), ``embed_backward`` and
``cross_entropy`` are float64, and ``sample`` walks the sampler's contract literally on ``tests/philox.py``.

``sample`` also returns **decided** per row.  The contract forms its prefix sums in binary64 and lets the kernel add them in any
order, so a row's code is pinned only where no decision sits on a rounding error.  The margin is M = 2^-36 of the kept mass:
binary64 ``exp`` is within a few ulp (2^-52 each) and a sum of at most 4096 terms in any order is within 4096 * 2^-53 = 2^-41
relative of the exact sum, so two correct evaluations of any C_j differ by less than 2^-40 of the mass; 2^-36 leaves a factor of
more than 16 on top.  A row is decided when (a) every prefix length that top_p admits within +-M -- the lengths from
``1 + #{C_j / C_all < top_p - M}`` to ``1 + #{C_j / C_all < top_p + M}`` -- gives the same code, and (b) for each of them
``u * C_kept`` lies more than ``M * C_kept`` from both ends of the chosen interval (an end with no neighbour cannot be crossed).
"""
from __future__ import annotations

import numpy as np

from tests import philox

SAMPLE_STREAM = 0x53414D50
MARGIN = 2.0 ** -36
MAX_K = 2048

# (temperature, top_k, top_p): greedy; top_k = 1 (equal to greedy); top_k >= size; top_p -> 0 (keeps one); the four of the issue
SETTINGS = ((0.0, 0, 1.0), (1.0, 1, 1.0), (1.0, 4096, 1.0), (1.0, 0, 1e-9),
            (1.0, 0, 1.0), (0.7, 50, 1.0), (1.0, 0, 0.9), (1.3, 200, 0.95))


def _clamp(v, b, hi):
    return hi if v is None else int(min(max(int(v[b]), 0), hi))


def embed(tables: np.ndarray, index: np.ndarray, counts=None) -> np.ndarray:
    """tables (Q, R, D) float32, index (B, n, Q) -> (B, D, n) float32: ((0 + t_0) + t_1) + ... in binary32, stage order."""
    tables = np.asarray(tables, dtype=np.float32)
    n_q, r, d = tables.shape
    b, n, _ = index.shape
    out = np.zeros((b, n, d), dtype=np.float32)
    for q in range(n_q):
        idx = index[:, :, q]
        ok = (idx >= 0) & (idx < r)
        rows = tables[q][np.where(ok, idx, 0)]
        out = np.where(ok[:, :, None], (out + rows).astype(np.float32), out)
    for row in range(b):
        out[row, _clamp(counts, row, n):] = 0.0
    return np.ascontiguousarray(out.transpose(0, 2, 1))


def embed_backward(dout: np.ndarray, index: np.ndarray, rows: int, counts=None) -> np.ndarray:
    """dout (B, D, n), index (B, n, Q) -> dtables (Q, rows, D) float64."""
    b, d, n = dout.shape
    n_q = index.shape[2]
    dt = np.zeros((n_q, rows, d), dtype=np.float64)
    for row in range(b):
        for i in range(_clamp(counts, row, n)):
            for q in range(n_q):
                r = int(index[row, i, q])
                if 0 <= r < rows:
                    dt[q, r] += dout[row, :, i].astype(np.float64)
    return dt


def cross_entropy(logits: np.ndarray, target: np.ndarray, sizes, g: float = 1.0):
    """logits (B, Q K, T), target (B, T, Q) -> (loss, nll (B, T, Q), dlogits (B, Q K, T), n_live), float64."""
    logits = np.asarray(logits, dtype=np.float64)
    b, c, t = logits.shape
    n_q = target.shape[2]
    k = c // n_q
    nll = np.zeros((b, t, n_q))
    soft = np.zeros_like(logits)
    live = np.zeros((b, t, n_q), dtype=bool)
    for q in range(n_q):
        size = int(sizes[q])
        l = logits[:, q * k:q * k + size, :]                       # (B, size, T)
        m = l.max(axis=1, keepdims=True)
        lse = (m + np.log(np.exp(l - m).sum(axis=1, keepdims=True)))[:, 0, :]   # (B, T)
        y = target[:, :, q]
        ok = (y >= 0) & (y < size)
        picked = np.take_along_axis(l, np.where(ok, y, 0)[:, None, :], axis=1)[:, 0, :]
        nll[:, :, q] = np.where(ok, lse - picked, 0.0)
        p = np.exp(l - lse[:, None, :])
        onehot = (np.arange(size)[None, :, None] == y[:, None, :])
        soft[:, q * k:q * k + size, :] = np.where(ok[:, None, :], p - onehot, 0.0)
        live[:, :, q] = ok
    n_live = int(live.sum())
    if n_live == 0:
        return 0.0, nll, np.zeros_like(logits), 0
    return float(nll.sum() / n_live), nll, g * soft / n_live, n_live


def uniforms(seeds, frame0, n: int, n_q: int) -> np.ndarray:
    """u (B, n, Q) float64 = (w + 0.5) / 2^32, w = word 0 of Philox at (lo32(f), hi32(f), q, SAMPLE_STREAM) under seeds[b]."""
    seeds = np.asarray(seeds, dtype=np.int64).astype(np.uint64)
    f = (np.asarray(frame0, dtype=np.int64)[:, None] + np.arange(n, dtype=np.int64)[None, :]).astype(np.uint64)[:, :, None]
    q = np.arange(n_q, dtype=np.uint64)[None, None, :]
    mask = np.uint64(0xFFFFFFFF)
    k0, k1 = (seeds & mask)[:, None, None], (seeds >> np.uint64(32))[:, None, None]
    w = philox.philox4x32_10(f & mask, f >> np.uint64(32), q, SAMPLE_STREAM, k0, k1)[0]
    return (w.astype(np.float64) + 0.5) / 2.0 ** 32


def _pick(cum: np.ndarray, kept: int, u: float):
    """(position in the order, decided) of step 7 on the first ``kept`` prefix sums."""
    thr = u * cum[kept - 1]
    j = min(int(np.searchsorted(cum[:kept], thr, side="left")), kept - 1)
    m = MARGIN * cum[kept - 1]
    lower_ok = j == 0 or thr - cum[j - 1] > m
    upper_ok = j == kept - 1 or cum[j] - thr > m
    return j, bool(lower_ok and upper_ok)


def sample_row(l: np.ndarray, tau: float, top_k: int, top_p: float, u: float):
    """One sampler row over the float32 logits ``l`` of a stage -> (code, decided)."""
    l = np.asarray(l, dtype=np.float32)
    l = np.where(np.isnan(l), np.float32(-np.inf), l)
    size = l.shape[0]
    tau, top_p = float(np.float32(tau)), float(np.float32(top_p))
    if not tau > 0.0:
        return int(np.argmax(l)), True
    l64 = l.astype(np.float64) + 0.0                          # -0 counts as +0
    order = np.lexsort((np.arange(size), -l64))               # l descending, k ascending
    kept0 = min(int(top_k), size) if top_k > 0 else size
    z = l64[order][:kept0] / tau
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.where(z == z[0], 1.0, np.exp(z - z[0]))
    cum = np.cumsum(e)
    lengths = [kept0]
    if top_p < 1.0:
        ratio = cum / cum[-1]
        lengths = [min(1 + int((ratio < top_p).sum()), kept0)]
        lo = min(1 + int((ratio < top_p - MARGIN).sum()), kept0)
        hi = min(1 + int((ratio < top_p + MARGIN).sum()), kept0)
        lengths += [v for v in range(lo, hi + 1) if v != lengths[0]]
    picks = [_pick(cum, kept, u) for kept in lengths]
    code = int(order[picks[0][0]])
    decided = all(ok and int(order[j]) == code for j, ok in picks)
    return code, decided


def sample(logits: np.ndarray, sizes, seeds, frame0, temperature, top_k, top_p, counts=None, stages=None, carry=None):
    """logits (B, Q K, n) float32 -> (codes (B, n, Q) int64, decided (B, n, Q) bool, carry (B, Q) int64 or None)."""
    logits = np.asarray(logits, dtype=np.float32)
    b, c, n = logits.shape
    n_q = len(sizes)
    k = c // n_q
    u = uniforms(seeds, frame0, n, n_q)
    codes = np.full((b, n, n_q), -1, dtype=np.int64)
    decided = np.ones((b, n, n_q), dtype=bool)
    carry = None if carry is None else np.array(carry, dtype=np.int64)
    for row in range(b):
        cnt, qb = _clamp(counts, row, n), _clamp(stages, row, n_q)
        for i in range(cnt):
            for q in range(qb):
                codes[row, i, q], decided[row, i, q] = sample_row(logits[row, q * k:q * k + int(sizes[q]), i], temperature[row],
                                                                  int(top_k[row]), top_p[row], u[row, i, q])
        if carry is not None and cnt >= 1:
            carry[row] = codes[row, cnt - 1]
    return codes, decided, carry


def _settings(b: int, first: int):
    rows = [SETTINGS[(first + r) % len(SETTINGS)] for r in range(b)]
    return (np.array([s[0] for s in rows], dtype=np.float32), np.array([s[1] for s in rows], dtype=np.int64),
            np.array([s[2] for s in rows], dtype=np.float32))


def sampler_cases():
    """The input sets of the GPU sampler tests, by name: dicts of ``logits``, ``sizes``, ``seeds``, ``frame0``, ``temperature``,
    ``top_k``, ``top_p``, ``counts``, ``stages``.  Built once per process (``cases()``); nothing mutates them."""
    rng = np.random.default_rng(2027)
    out = {}

    def add(name, b, n, sizes, kind, first, counts=None, stages=None):
        n_q, k = len(sizes), max(sizes)
        l = (3.0 * rng.standard_normal((b, n_q * k, n))).astype(np.float32)
        if kind == "ties":
            l = (np.round(l * 2.0) / 2.0).astype(np.float32)
        elif kind == "inf":
            l[rng.random(l.shape) < 0.3] = -np.inf
            l[:, ::k, :] = 0.25                                # code 0 of every stage stays finite
        elif kind == "equal":
            l[:] = 1.5
        tau, tk, tp = _settings(b, first)
        out[name] = dict(logits=l, sizes=tuple(sizes), seeds=rng.integers(-2 ** 63, 2 ** 63 - 1, b, dtype=np.int64),
                         frame0=rng.integers(0, 2 ** 40, b, dtype=np.int64), temperature=tau, top_k=tk, top_p=tp,
                         counts=None if counts is None else np.array(counts, dtype=np.int64),
                         stages=None if stages is None else np.array(stages, dtype=np.int64))

    first = 0
    for n in (1, 3):
        for kind in ("randn", "ties", "inf", "equal"):
            add(f"mixed-n{n}-{kind}", 3, n, (1024, 100, 1), kind, first)
            first += 3
    for kind in ("randn", "ties"):
        add(f"edge-{kind}", 3, 2, (65, 64, 63), kind, first)
        first += 3
    add("counted", 3, 3, (65, 64, 63), "randn", 4, counts=(5, 2, 0), stages=(3, 1, 2))
    add("large", 16, 4, (1024,) * 8, "randn", 0)
    add("max-k", 2, 1, (MAX_K, MAX_K - 1), "randn", 6)
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = sampler_cases()
    return _CASES


_RESULTS = {}


def reference(name: str):
    """(codes, decided, carry) of case ``name`` with a start carry of -7 everywhere: computed once, shared, never mutated."""
    if name not in _RESULTS:
        c = cases()[name]
        b, n_q = c["logits"].shape[0], len(c["sizes"])
        _RESULTS[name] = sample(c["logits"], c["sizes"], c["seeds"], c["frame0"], c["temperature"], c["top_k"], c["top_p"],
                                c["counts"], c["stages"], np.full((b, n_q), -7, dtype=np.int64))
    return _RESULTS[name]
