"""A numpy / Python-int mirror of the three contracts of include/agx.h "Entropy coding" (DESIGN 4.28).

``tables``: logits -> frequency tables, every decision in float64, with a ``decided`` mask: a non-argmax frequency ``1 +
floor(r)`` is decided unless ``r`` lies within ``MARGIN = 2^-24`` of an integer it could cross -- ``r - floor(r) < MARGIN`` with
``floor(r) >= 1`` (a share below 1 cannot fall under 0), or ``floor(r) + 1 - r < MARGIN``.  ``r <= 65536`` is a quotient of
float64 values whose only free part is the order of the sum ``S`` over at most 2048 terms: a relative error below ``2048 * 2^-53
+ 3 * 2^-53`` plus one ulp of ``exp`` on either side, under ``1e-9`` absolute -- the margin is generous by a factor of 50.  The
argmax takes the rest, so it is compared through the device's own other frequencies.

``encode`` / ``decode``: the byte-wise rANS chain in Python ints, byte for byte what the kernels must write and read."""
import numpy as np

SCALE_BITS = 16
M = 1 << SCALE_BITS
L = 1 << 23
MARGIN = 2.0 ** -24
MAX_K = 2048
MAX_SYMBOLS = 8192


def _clamp(v, b, hi):
    return hi if v is None else int(min(max(int(v[b]), 0), hi))


def table_row(l: np.ndarray):
    """One live entry: float32 logits of the ``size`` codes -> (f int64 (size,), decided bool (size,), argmax)."""
    l = np.asarray(l, dtype=np.float32)
    size = l.shape[0]
    a = int(np.argmax(l))                                   # the lowest index of the maximum (-0 == +0)
    e = np.exp(l.astype(np.float64) - np.float64(l[a]))
    r = (M - size) * e / e.sum()
    fl = np.floor(r)
    f = 1 + fl.astype(np.int64)
    decided = ~(((r - fl < MARGIN) & (fl >= 1)) | (fl + 1 - r < MARGIN))
    f[a] += M - int(f.sum())
    decided[a] = True
    return f, decided, a


def tables(logits: np.ndarray, n_q: int, sizes=None, counts=None, stages=None):
    """logits (B, n_q K, n) -> (cum int64 (B, n, n_q, K + 1), decided bool (B, n, n_q, K), argmax int64 (B, n, n_q), -1 if dead)."""
    b, c, n = logits.shape
    k = c // n_q
    sizes = [k] * n_q if sizes is None else list(sizes)
    cum = np.zeros((b, n, n_q, k + 1), dtype=np.int64)
    decided = np.ones((b, n, n_q, k), dtype=bool)
    arg = np.full((b, n, n_q), -1, dtype=np.int64)
    for bi in range(b):
        cb, qb = _clamp(counts, bi, n), _clamp(stages, bi, n_q)
        for i in range(cb):
            for q in range(qb):
                f, d, a = table_row(logits[bi, q * k:q * k + sizes[q], i])
                cum[bi, i, q, 1:sizes[q] + 1] = np.cumsum(f)
                cum[bi, i, q, sizes[q] + 1:] = M
                decided[bi, i, q, :sizes[q]] = d
                arg[bi, i, q] = a
    return cum, decided, arg


def encode_symbols(pairs):
    """The chain over ``pairs`` = [(start, f), ...] in coding order s_1 .. s_N -> the packet as bytes (empty when N == 0)."""
    if not pairs:
        return b""
    x, out = L, []
    for start, f in reversed(pairs):
        x_max = ((L >> SCALE_BITS) << 8) * f
        while x >= x_max:
            out.append(x & 255)
            x >>= 8
        assert x < 1 << 31
        x = ((x // f) << SCALE_BITS) + (x % f) + start
    out += [(x >> (8 * j)) & 255 for j in range(4)]
    return bytes(reversed(out))


def encode(cum: np.ndarray, codes: np.ndarray, sizes=None, counts=None, stages=None):
    """cum (B, n, Q, K + 1), codes (B, n, Q) -> (packets uint8 (B, 2 n Q + 4), nbytes int64 (B,), status int64 (B,))."""
    b, n, n_q, k1 = cum.shape
    sizes = [k1 - 1] * n_q if sizes is None else list(sizes)
    width = 2 * n * n_q + 4
    packets = np.zeros((b, width), dtype=np.uint8)
    nbytes, status = np.zeros(b, dtype=np.int64), np.zeros(b, dtype=np.int64)
    for bi in range(b):
        pairs = []
        for i in range(_clamp(counts, bi, n)):
            for q in range(_clamp(stages, bi, n_q)):
                c = int(codes[bi, i, q])
                if not 0 <= c < sizes[q]:
                    status[bi] |= 1
                    continue
                start, f = int(cum[bi, i, q, c]), int(cum[bi, i, q, c + 1] - cum[bi, i, q, c])
                if start < 0 or f < 1 or start + f > M:
                    status[bi] |= 1
                    continue
                pairs.append((start, f))
        pkt = encode_symbols(pairs)
        assert len(pkt) <= width
        packets[bi, :len(pkt)] = np.frombuffer(pkt, dtype=np.uint8)
        nbytes[bi] = len(pkt)
    return packets, nbytes, status


def decode(cum: np.ndarray, packets: np.ndarray, nbytes, sizes=None, counts=None, stages=None, carry=None):
    """cum (B, hop, Q, K + 1) and the packets -> (codes int64 (B, hop, Q), state int64 (B, 2), status int64 (B,), carry): the
    whole hop in one pass.  ``carry`` (B, Q) is returned updated (a copy) when one is given."""
    b, hop, n_q, k1 = cum.shape
    sizes = [k1 - 1] * n_q if sizes is None else list(sizes)
    codes = np.full((b, hop, n_q), -1, dtype=np.int64)
    state, status = np.zeros((b, 2), dtype=np.int64), np.zeros(b, dtype=np.int64)
    carry = None if carry is None else np.array(carry, dtype=np.int64)
    for bi in range(b):
        cb, qb = _clamp(counts, bi, hop), _clamp(stages, bi, n_q)
        if cb == 0 or qb == 0:
            if carry is not None and cb > 0:
                carry[bi] = -1
            continue
        nb = int(min(max(int(nbytes[bi]), 0), packets.shape[1]))
        cur, st = 0, 0

        def byte():
            nonlocal cur, st
            v = 0
            if cur < nb:
                v = int(packets[bi, cur])
            else:
                st |= 2
            cur += 1
            return v
        x = 0
        for _ in range(4):
            x = (x << 8) | byte()
        for i in range(cb):
            for q in range(qb):
                t = cum[bi, i, q]
                slot = x & 0xffff
                c = int((t[1:sizes[q]] <= slot).sum())
                start, f = int(t[c]), int(t[c + 1] - t[c])
                x = (f * (x >> SCALE_BITS) + slot - start) & 0xffffffff
                for _ in range(2):
                    if x < L:
                        x = ((x << 8) | byte()) & 0xffffffff
                if x < L:
                    st |= 4
                codes[bi, i, q] = c
        if not (x == L and cur == int(nbytes[bi])):
            st |= 4
        if carry is not None:
            carry[bi] = codes[bi, cb - 1]
        state[bi], status[bi] = (x, cur), st
    return codes, state, status, carry


# ---------------------------------------------------------------------------------------------------------------- test inputs
SHAPES = {
    # name: (B, n, Q, K, sizes, counts, stages)
    "base": (2, 3, 3, 16, (16, 16, 5), [3, 1], [3, 2]),
    "k2048": (2, 2, 2, 2048, (2048, 1500), [2, 5], None),
    "k1": (2, 2, 2, 1, (1, 1), None, [2, 1]),
    "q64": (2, 2, 64, 2, None, [2, 0], [64, 33]),
}
SIGMAS = (0.1, 1.0, 4.0)
_CACHE = {}


def case(name: str, sigma: float):
    """The inputs of one shape at one logit scale and their mirror results: computed once, never modified.  -> dict(logits, n_q,
    k, sizes, counts, stages, codes, cum, decided, arg)."""
    key = (name, sigma)
    if key not in _CACHE:
        b, n, n_q, k, sizes, counts, stages = SHAPES[name]
        rng = np.random.default_rng(1000 + 100 * list(SHAPES).index(name) + int(sigma * 10))
        logits = (sigma * rng.standard_normal((b, n_q * k, n))).astype(np.float32)
        sz = [k] * n_q if sizes is None else list(sizes)
        codes = np.stack([rng.integers(0, s, (b, n)) for s in sz], axis=-1).astype(np.int64)
        cnt = None if counts is None else np.array(counts, dtype=np.int64)
        stg = None if stages is None else np.array(stages, dtype=np.int64)
        cum, decided, arg = tables(logits, n_q, sizes, cnt, stg)
        _CACHE[key] = dict(logits=logits, n_q=n_q, k=k, sizes=sizes, counts=cnt, stages=stg, codes=codes, cum=cum, decided=decided, arg=arg)
    return _CACHE[key]


def live_mask(c):
    """bool (B, n, Q): the entries below their row's frame and stage counts."""
    b, n, n_q = c["codes"].shape
    live = np.zeros((b, n, n_q), dtype=bool)
    for bi in range(b):
        live[bi, :_clamp(c["counts"], bi, n), :_clamp(c["stages"], bi, n_q)] = True
    return live
