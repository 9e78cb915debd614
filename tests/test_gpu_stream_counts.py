"""The counted forms of the streaming ops (``counts=``; include/agx.h "Per-row frame counts") against their uncounted forms.

One layer of every streaming kind -- causal k = 7 d = 3, causal stride 2 k = 4, upsampling s = 2 k = 5, transposed k = 3, a residual
unit -- at C_in = 20 (two weight groups, the second partly padded), C_out = 70 (past one 64-row block), B = 3, chunks of n = 5 frames
at 2 base positions per frame: nt = 10 crosses an NT = 8 tile, a count of 4 ends exactly on the tile edge and 5 one past it.

Per row: the valid columns are ``torch.equal`` to the uncounted op fed that row's frames alone (a row of a batch equals the row
alone and schedules are bit-identical: tests/test_gpu_conv_stream.py); a plain destination is exact 0 behind the count; a ring
destination still holds the poison written before the step.  The chunk holds NaN behind every row's count.
"""
import pytest
import torch

from audio_generation_amd import ops
from oracle import attention as oattn
from tests import codec_stream_ref as ref
from tests.test_gpu_conv_stream import DEV, GpuOp, _block

pytestmark = pytest.mark.gpu
B, N, C_IN, C_OUT = 3, 5, 20, 70
COUNTS = ([5, 0, 4], [1, 4, 0], [0, 0, 0], [2, 5, 5], [4, 1, 3])
POISON = 12345.0


def _unit(name):
    """(ops of the unit, rate_in)."""
    if name == "causal":
        return [GpuOp("causal", C_IN, C_OUT, 7, d=3)], 2
    if name == "strided":
        return [GpuOp("causal", C_IN, C_OUT, 4, s=2, pre=ref.SLOPE)], 4
    if name == "up":
        return [GpuOp("up", C_IN, C_OUT, 5, s=2, pre=ref.SLOPE)], 2
    if name == "convt":
        return [GpuOp("convt", C_IN, C_OUT, 3)], 2
    return [GpuOp("causal", C_IN, C_OUT, 7, d=3, pre=ref.SLOPE), GpuOp("causal", C_OUT, C_IN, 1, residual=True, post=ref.SLOPE, seed=1)], 2


UNITS = ("causal", "strided", "up", "convt", "res")


def _launch(unit, src, dst, dst_ring, pos, n, rate_in, counts):
    first, last = unit[0], unit[-1]
    kw = {} if counts is None else dict(counts=counts)
    if len(unit) == 2:
        hid = torch.empty(src.shape[0], first.c_out, n * rate_in, device=DEV)
        first.launch(src, hid, pos, None, n, rate_in, 0, dst_ring=False, **kw)
        if counts is not None:                              # the hidden activation: a plain destination, zero behind the count
            for r, c in enumerate(counts.tolist()):
                assert float(hid[r, :, c * rate_in:].abs().max() if c < n else 0.0) == 0.0
        return last.launch(hid, dst, pos, None, n, rate_in, 0, src_ring=False, dst_ring=dst_ring, res=src, **kw)
    return first.launch(src, dst, pos, None, n, rate_in, 0, dst_ring=dst_ring, **kw)


def _geometry(unit, rate_in):
    first = unit[0]
    reach = first.d * (first.k - 1) if len(unit) == 2 else first.ref.reach
    rate_out, delay_out = (rate_in, 0) if len(unit) == 2 else first.ref.rates(rate_in, 0)
    return reach + N * rate_in, N * rate_out + 3, rate_out, delay_out, unit[-1].c_out


def _row_alone(unit, rate_in, x_row, takes):
    """The uncounted op on one row's frames, in the chunks the row took: (1, c_out, frames * rate_out)."""
    cap, _, rate_out, _, c_out = _geometry(unit, rate_in)
    src = torch.zeros(1, unit[0].c_in, cap, device=DEV)
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    outs, at = [], 0
    for c in takes:
        if c == 0:
            continue
        ops.ring_write_rate(src, x_row[:, :, at * rate_in:(at + c) * rate_in].contiguous(), pos, rate_in)
        dst = torch.empty(1, c_out, c * rate_out, device=DEV)
        outs.append(_launch(unit, src, dst, False, pos, c, rate_in, None).clone())
        ops.stream_advance(pos, c)
        at += c
    return torch.cat(outs, dim=2), src, pos


@pytest.mark.parametrize("name", UNITS)
def test_counted_step_equals_the_rows_own_uncounted_stream(name):
    unit, rate_in = _unit(name)
    cap, cap_out, rate_out, delay_out, c_out = _geometry(unit, rate_in)
    total = [sum(c[r] for c in COUNTS) for r in range(B)]
    x = torch.randn(B, C_IN, max(total) * rate_in, generator=torch.Generator().manual_seed(3)).to(DEV)
    src = torch.zeros(B, C_IN, cap, device=DEV)
    pos = torch.zeros(B, dtype=torch.int64, device=DEV)
    host_pos = [0] * B
    valid = [[] for _ in range(B)]
    for step in COUNTS:
        counts = torch.tensor(step, dtype=torch.int64, device=DEV)
        chunk = torch.full((B, C_IN, N * rate_in), float("nan"), device=DEV)             # NaN behind every row's count
        for r, c in enumerate(step):
            chunk[r, :, :c * rate_in] = x[r, :, host_pos[r] * rate_in:(host_pos[r] + c) * rate_in]
        before = src.clone()
        ops.ring_write_rate(src, chunk, pos, rate_in, counts=counts)
        for r, c in enumerate(step):                                                       # the source ring: only the row's own columns
            cols = torch.remainder(torch.arange(host_pos[r] * rate_in, (host_pos[r] + c) * rate_in), cap).to(DEV)
            keep = torch.ones(cap, dtype=torch.bool, device=DEV)
            keep[cols] = False
            assert torch.equal(src[r][:, keep], before[r][:, keep]) and torch.equal(src[r][:, cols], chunk[r, :, :c * rate_in])
        plain = torch.full((B, c_out, N * rate_out), POISON, device=DEV)
        ring = torch.full((B, c_out, cap_out), POISON, device=DEV)
        _launch(unit, src, plain, False, pos, N, rate_in, counts)
        _launch(unit, src, ring, True, pos, N, rate_in, counts)
        block = _block(ring, host_pos, N * rate_out, rate_out, delay_out)
        for r, c in enumerate(step):
            v = c * rate_out
            assert not torch.isnan(plain[r]).any()
            assert torch.equal(block[r, :, :v], plain[r, :, :v]), (name, step, r)        # ring and plain destinations agree
            assert float(plain[r, :, v:].abs().max() if c < N else 0.0) == 0.0, (name, step, r)
            assert bool((block[r, :, v:] == POISON).all()), (name, step, r)                # a ring behind the count keeps its poison
            assert int((ring[r] == POISON).sum()) == c_out * (cap_out - v), (name, step, r)
            valid[r].append(plain[r:r + 1, :, :v].clone())
        ops.stream_advance(pos, N, counts=counts)
        host_pos = [p + c for p, c in zip(host_pos, step)]
        assert pos.tolist() == host_pos
    for r in range(B):
        want, src_alone, _ = _row_alone(unit, rate_in, x[r:r + 1], [c[r] for c in COUNTS])
        got = torch.cat(valid[r], dim=2)
        assert got.shape == want.shape and float(want.abs().max()) > 1e-3
        assert torch.equal(got, want), (name, r, float((got - want).abs().max()))
        assert torch.equal(src[r:r + 1], src_alone), (name, r)                            # and the ring the stream leaves behind


def test_counted_ring_write_pos_and_advance():
    """``ring_write_pos`` / ``stream_advance`` with counts: a column behind the count keeps its poison, positions move by the count."""
    hd, n, ring_cols = 8, 4, 11
    gen = torch.Generator().manual_seed(5)
    qkv = torch.randn(B, 3 * hd, n, generator=gen).to(DEV)
    pos = torch.tensor([0, 9, (1 << 40) + 3], dtype=torch.int64, device=DEV)
    for step in ([4, 0, 2], [0, 0, 0], [1, 4, 3]):
        counts = torch.tensor(step, dtype=torch.int64, device=DEV)
        buf = torch.full((B, 2 * hd, ring_cols), POISON, device=DEV)
        want = buf.clone()
        p = pos.tolist()
        for r, c in enumerate(step):
            for t in range(c):
                want[r, :, (p[r] + t) % ring_cols] = qkv[r, hd:, t]
        ops.ring_write_pos(buf, qkv[:, hd:, :], pos, ring_cols, counts=counts)
        assert torch.equal(buf, want), step
        ops.stream_advance(pos, n, counts=counts)
        assert pos.tolist() == [a + c for a, c in zip(p, step)]


@pytest.mark.parametrize("dh", [16, 64])
def test_counted_stream_attention(dh):
    """``attention_alibi_stream(counts=)``: the ring holds NaN wherever the row's own frames are not -- the columns of the chunk
    behind the count included, where a masked key would otherwise meet its V as 0 * NaN.  The queries below the count are the
    uncounted op on the row's ``c_b`` frames, bit for bit."""
    heads, tq, w, ring_cols = 2, 4, 5, 12
    hd = heads * dh
    gen = torch.Generator().manual_seed(6 + dh)
    slopes = oattn.alibi_slopes(heads).to(DEV)
    positions = [0, 9, (1 << 40) + 7]
    pos = torch.tensor(positions, dtype=torch.int64, device=DEV)
    for step in ([4, 0, 2], [1, 4, 3], [0, 0, 0]):
        q = (0.7 * torch.randn(B, hd, tq, generator=gen)).to(DEV)
        kv = torch.full((B, 2 * hd, ring_cols), float("nan"))
        for r, (p, c) in enumerate(zip(positions, step)):
            for j in range(max(0, p - w + 1), p + c):
                kv[r, :, j % ring_cols] = 0.7 * torch.randn(2 * hd, generator=gen)
        kv = kv.to(DEV)
        before = kv.clone()
        got = ops.attention_alibi_stream(q, kv, pos, slopes, heads, dh, dh ** 0.5, w, ring_cols,
                                         counts=torch.tensor(step, dtype=torch.int64, device=DEV))
        assert tuple(got.shape) == (B, hd, tq) and torch.equal(kv.view(torch.int32), before.view(torch.int32))
        for r, c in enumerate(step):
            if c:
                one = ops.attention_alibi_stream(q[r:r + 1, :, :c].contiguous(), kv[r:r + 1], pos[r:r + 1], slopes, heads, dh, dh ** 0.5,
                                                 w, ring_cols)
                assert bool(torch.isfinite(one).all()) and torch.equal(got[r:r + 1, :, :c], one), (step, r)


@pytest.mark.parametrize("k", [1, 4])
def test_counted_glu_step(k):
    """``glu_dwconv_step(counts=)``: the valid outputs and the history are those of the uncounted step on the row's own frames; the
    outputs behind the count are exact 0 with NaN planted there; a row with count 0 keeps its history."""
    c, n = 37, 4
    gen = torch.Generator().manual_seed(8)
    w, bias = torch.randn(c, 1, k, generator=gen).to(DEV), torch.randn(c, generator=gen).to(DEV)
    bn = tuple(t.to(DEV) for t in (torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen), torch.randn(c, generator=gen),
                                   torch.rand(c, generator=gen) + 0.5))
    schedule = ([4, 0, 3], [1, 4, 0], [0, 0, 0], [2, 1, 4])
    total = [sum(s[r] for s in schedule) for r in range(B)]
    u = torch.randn(B, 2 * c, max(total), generator=gen).to(DEV)
    hist = torch.zeros(B, c, k - 1, device=DEV) if k > 1 else None
    alone = [torch.zeros(1, c, k - 1, device=DEV) if k > 1 else None for _ in range(B)]
    at = [0] * B
    for step in schedule:
        counts = torch.tensor(step, dtype=torch.int64, device=DEV)
        chunk = torch.full((B, 2 * c, n), float("nan"), device=DEV)
        for r, cnt in enumerate(step):
            chunk[r, :, :cnt] = u[r, :, at[r]:at[r] + cnt]
        before = None if hist is None else hist.clone()
        y = ops.glu_dwconv_step(chunk, w, bias, bn, hist, counts=counts)
        for r, cnt in enumerate(step):
            assert float(y[r, :, cnt:].abs().max() if cnt < n else 0.0) == 0.0 and not torch.isnan(y[r]).any()
            if cnt:
                want = ops.glu_dwconv_step(u[r:r + 1, :, at[r]:at[r] + cnt].contiguous(), w, bias, bn, alone[r])
                assert torch.equal(y[r:r + 1, :, :cnt], want), (step, r)
            elif hist is not None:
                assert torch.equal(hist[r], before[r])
            if hist is not None:
                assert torch.equal(hist[r:r + 1], alone[r]), (step, r)
            at[r] += cnt
