"""CPU statement of the RVQ streaming step (``agx_rvq_step_encode`` / ``agx_rvq_step_decode``): the defining search
stage by stage (``oracle.rvq.exact_search``), the outputs behind a row's count, and the packet layout on ``oracle.bitstream``."""
import numpy as np
import torch

from oracle import bitstream, rvq


def taken(counts, batch: int, n: int):
    """``c_b = clamp(counts[b], 0, n)``; ``n`` for every row when ``counts`` is None."""
    return [n] * batch if counts is None else [min(max(int(c), 0), n) for c in counts]


def packet_bytes(n: int, q_used: int, bits: int) -> int:
    return -((-n * q_used * bits) // 8)


def packets(index, counts, bits: int) -> np.ndarray:
    """index (B, n, Q) -> (B, P) uint8: row b's first ``ceil(c_b Q bits / 8)`` bytes are ``oracle.bitstream.pack`` of its c_b Q
    codes, frame-major and stage-minor; every byte behind them is 0.  Rows are packed one by one: they never share a byte."""
    index = np.asarray(index, dtype=np.int64)
    b, n, q = index.shape
    out = np.zeros((b, packet_bytes(n, q, bits)), np.uint8)
    for r, c in enumerate(taken(counts, b, n)):
        if c * q:
            row = bitstream.pack(index[r, :c].reshape(-1), bits)
            assert row.shape[0] == packet_bytes(c, q, bits)
            out[r, :row.shape[0]] = row
    return out


def unpack_row(row, c: int, q: int, bits: int) -> np.ndarray:
    """The (c, q) codes of one packet row."""
    return bitstream.unpack(np.asarray(row, np.uint8), c * q, bits).reshape(c, q)


def exact_reference(z: torch.Tensor, cbs: torch.Tensor, sizes=None, q_used=None):
    """The definition on (B, D, n) latents: per stage the full exact search over the stage's own codewords, r <- r - c and
    out <- out + c in binary32 -> (zq (B, D, n), index (B, n, q_used))."""
    b, d, n = z.shape
    q_used = cbs.shape[0] if q_used is None else q_used
    r = z.transpose(1, 2).reshape(-1, d).numpy().astype(np.float32).copy()
    out = np.zeros_like(r)
    idx = np.empty((r.shape[0], q_used), np.int64)
    for q in range(q_used):
        cb = cbs[q].numpy().astype(np.float32)
        cb = cb if sizes is None else cb[:int(sizes[q])]
        i = rvq.exact_search(r, cb)
        idx[:, q] = i
        r = (r - cb[i]).astype(np.float32)
        out = (out + cb[i]).astype(np.float32)
    return torch.from_numpy(out).reshape(b, n, d).transpose(1, 2).contiguous(), torch.from_numpy(idx).reshape(b, n, q_used)


def behind_counts(zq: torch.Tensor, index: torch.Tensor, counts):
    """What the step stores: zq exact 0 and index -1 at the frames behind a row's count."""
    zq, index = zq.clone(), index.clone()
    for r, c in enumerate(taken(counts, zq.shape[0], zq.shape[2])):
        zq[r, :, c:] = 0.0
        index[r, c:] = -1
    return zq, index
