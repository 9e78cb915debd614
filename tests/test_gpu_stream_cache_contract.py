"""Memory contract of ``ops.attention_alibi_stream``, ``ops.ring_write_pos`` and ``ops.stream_advance`` on the guarded, poisoned
arena of ``tests/guarded.py`` (modelled on tests/test_gpu_window_attention_contract.py): queries, slopes, positions, the ring and
the outputs sit between guard bands, and every byte the ops do not own holds 0x00, 0xFF or 0x7F in turn.  Guards must stay
intact; the attention allocates its output only and writes neither the positions nor the ring; the ring write allocates nothing
and writes n columns per row and nothing else; the advance writes the positions only; and the results are bitwise the same on
every pattern, with the ring columns outside every window left as the arena's poison.  Tolerance: that of
tests/test_gpu_window_attention.py for the op."""
import pytest
import torch

from audio_generation_amd import ops
from oracle import attention as oattn
from tests.guarded import Out, routed, run_contract
from tests.window_attention_ref import window_core

pytestmark = pytest.mark.gpu
DEV = "cuda"
scale = lambda t: max(1.0, float(t.abs().max()))   # noqa: E731


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_stream_attention_memory_contract():
    """33 new queries per row with a window of 40 on a ring of 96 columns in rows of pitch 100; the rows sit at 0 (63 ring
    columns never written), at 224 (the chunk wraps the ring) and at 224 + 9600 * 2^30 (beyond int32; lcm(64, 96) = 192 divides
    it).  Every ring column outside a row's window and the 4 columns beyond the ring keep the arena's poison (0x00, 0xFF = NaN,
    0x7F = 3.4e38) in every K and V row."""
    b, heads, dh, tq, w, ring, pitch = 3, 2, 64, 33, 40, 96, 100
    positions = (0, 224, 224 + 9600 * 2 ** 30)
    hd = heads * dh
    gen = torch.Generator().manual_seed(81)
    q = 0.7 * torch.randn(b, hd, tq, generator=gen)
    slopes = oattn.alibi_slopes(heads)
    pos = torch.tensor(positions, dtype=torch.int64)
    want = torch.empty(b, hd, tq, dtype=torch.float64)
    cols, vals = [], []
    for r, p in enumerate(positions):
        near = p % (9600 * 2 ** 30) if p > 2 ** 31 else p          # the same columns, blocks and distances
        tk, lo = near + tq, max(0, near - w + 1)
        kv = 0.7 * torch.randn(1, 2 * hd, tk, generator=gen)
        want[r] = window_core(q[r:r + 1].double(), kv.double(), slopes, heads, dh, dh ** 0.5, w, q_pos0=near)[0]
        cols.append(torch.tensor([j % ring for j in range(lo, tk)]))
        vals.append(kv[0, :, lo:])
        assert len(set(cols[-1].tolist())) == tk - lo <= ring
    assert int(cols[1][0]) > int(cols[1][-1])                       # the span of the row at 224 wraps

    def run(arena):
        qd, sd, pd = arena.place(q), arena.place(slopes), arena.place(pos)
        buf = arena.empty((b, 2 * hd, pitch))
        for r in range(b):
            buf[r][:, cols[r].to(buf.device)] = vals[r].to(buf.device)
        ring_before = _bits(buf).clone()
        first = len(arena.allocs)
        with routed(arena, ops):
            out = ops.attention_alibi_stream(qd, buf, pd, sd, heads, dh, dh ** 0.5, w, ring)
        assert len(arena.allocs) == first + 1                       # the output and nothing else
        assert torch.equal(_bits(buf), ring_before)                 # poison included: the ring is not written
        return [Out("out", out, want, 3e-5 * scale(want)), Out("pos", pd, pos, exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


@pytest.mark.parametrize("n", [1, 9])
def test_ring_write_pos_memory_contract(n):
    """The K / V rows of a (3, 3*48, n) qkv tensor, read in place, into a poisoned ring of 13 columns in rows of pitch 16: exactly
    n columns per row change, to the source's bits; everything else is still the arena's fill."""
    b, hd, ring, pitch = 3, 48, 13, 16
    positions = (0, 11, 7 + 13 * 2 ** 35)
    gen = torch.Generator().manual_seed(90 + n)
    qkv = torch.randn(b, 3 * hd, n, generator=gen)
    pos = torch.tensor(positions, dtype=torch.int64)
    written = torch.tensor([[(p + t) % ring for t in range(n)] for p in positions])           # (b, n) columns
    assert n == 1 or int(written[1][0]) > int(written[1][-1])                                   # row 1 wraps

    def run(arena):
        qd, pd = arena.place(qkv), arena.place(pos)
        buf = arena.empty((b, 2 * hd, pitch))
        fill = _bits(buf).clone()
        first = len(arena.allocs)
        with routed(arena, ops):
            ops.ring_write_pos(buf, qd[:, hd:, :], pd, ring)
        assert len(arena.allocs) == first                           # nothing is allocated
        got = torch.stack([buf[r][:, written[r].to(buf.device)] for r in range(b)])          # (b, 2*hd, n)
        untouched = torch.ones(b, 2 * hd, pitch, dtype=torch.bool, device=buf.device)
        for r in range(b):
            untouched[r][:, written[r].to(buf.device)] = False
        assert int(untouched.sum()) == b * 2 * hd * (pitch - n)
        assert torch.equal(_bits(buf)[untouched], fill[untouched])  # every other element keeps its bits
        return [Out("written", got, qkv[:, hd:, :], exact=True), Out("pos", pd, pos, exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


def test_stream_advance_memory_contract():
    start = [0, 2 ** 31 - 1, 2 ** 40, 5] + list(range(300))         # two workgroups, the second one partly out of range
    pos = torch.tensor(start, dtype=torch.int64)
    want = torch.tensor([p + 7 for p in start], dtype=torch.int64)

    def run(arena):
        pd = arena.place(pos)
        first = len(arena.allocs)
        with routed(arena, ops):
            ops.stream_advance(pd, 7)
        assert len(arena.allocs) == first
        return [Out("pos", pd, want, exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]
