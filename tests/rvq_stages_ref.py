"""CPU statement of the per-row stage counts of the RVQ streaming step (``agx_rvq_step_encode_staged``,
``agx_rvq_step_decode_staged``, ``agx_rvq_packets_restage``), built on tests/rvq_step_ref.py: a row with ``q_b`` stages is that row
quantised with ``q_used = q_b``, and its packet is ``oracle.bitstream.pack`` of its own ``c_b q_b`` codes."""
import numpy as np
import torch

from oracle import bitstream
from tests import rvq_step_ref as ref


def taken_stages(stages, batch: int, q_used: int):
    """``q_b = clamp(stages[b], 0, q_used)``; ``q_used`` for every row when ``stages`` is None."""
    return [q_used] * batch if stages is None else [min(max(int(s), 0), q_used) for s in stages]


def live_bytes(c: int, q: int, bits: int) -> int:
    """Bytes of a row's packet: ``ceil(c q bits / 8)``."""
    return -((-c * q * bits) // 8)


def packets(index, counts, stages, bits: int, q_used: int) -> np.ndarray:
    """index (B, n, >= q_b) -> (B, P) uint8, ``P = ceil(n q_used bits / 8)``: row r's first ``ceil(c_r q_r bits / 8)`` bytes are
    ``oracle.bitstream.pack`` of ``index[r, :c_r, :q_r]``, frame-major and stage-minor over the row's own q_r; every byte behind
    them is 0.  Rows are packed one by one: they never share a byte."""
    index = np.asarray(index, dtype=np.int64)
    b, n = index.shape[:2]
    out = np.zeros((b, ref.packet_bytes(n, q_used, bits)), np.uint8)
    for r, (c, q) in enumerate(zip(ref.taken(counts, b, n), taken_stages(stages, b, q_used))):
        if c * q:
            row = bitstream.pack(index[r, :c, :q].reshape(-1), bits)
            assert row.shape[0] == live_bytes(c, q, bits)
            out[r, :row.shape[0]] = row
    return out


def unpacked(packets_, counts, stages, bits: int, q_used: int, n: int) -> np.ndarray:
    """The inverse of ``packets``: (B, n, q_used) int64, -1 where a stage is not live."""
    packets_ = np.asarray(packets_, np.uint8)
    b = packets_.shape[0]
    index = np.full((b, n, q_used), -1, np.int64)
    for r, (c, q) in enumerate(zip(ref.taken(counts, b, n), taken_stages(stages, b, q_used))):
        if c * q:
            index[r, :c, :q] = ref.unpack_row(packets_[r, :live_bytes(c, q, bits)], c, q, bits)
    return index


def restaged(packets_, counts, stages_in, stages_to, bits: int, q_used: int, n=None):
    """Packets of ``stages_in`` -> (packets of ``min(q_in, q_to)`` stages per row, those minima): unpack, slice, pack.  ``n``:
    the frames per row the counts clamp to; by default the most that P bytes hold, which is n whenever ``q_used bits >= 8``."""
    packets_ = np.asarray(packets_, np.uint8)
    b = packets_.shape[0]
    if n is None:
        n = 8 * packets_.shape[1] // (q_used * bits) if q_used else 1
    assert packets_.shape[1] == ref.packet_bytes(n, q_used, bits)
    q_out = [min(a, t) for a, t in zip(taken_stages(stages_in, b, q_used), taken_stages(stages_to, b, q_used))]
    index = unpacked(packets_, counts, stages_in, bits, q_used, n)
    return packets(index, counts, q_out, bits, q_used), q_out


def reference(z: torch.Tensor, cbs: torch.Tensor, sizes, counts, stages):
    """The definition, row by row: row r is ``rvq_step_ref.exact_reference(z[r:r+1], cbs, sizes, q_used=q_r)``; zq is exact 0
    and index -1 wherever nothing is live -> (zq (B, D, n), index (B, n, Q))."""
    b, d, n = z.shape
    q_used = cbs.shape[0]
    zq = torch.zeros(b, d, n, dtype=torch.float32)
    index = torch.full((b, n, q_used), -1, dtype=torch.int64)
    for r, (c, q) in enumerate(zip(ref.taken(counts, b, n), taken_stages(stages, b, q_used))):
        if c * q:
            row_q, row_i = ref.exact_reference(z[r:r + 1, :, :c].contiguous(), cbs, sizes, q_used=q)
            zq[r, :, :c] = row_q[0]
            index[r, :c, :q] = row_i[0]
    return zq, index
