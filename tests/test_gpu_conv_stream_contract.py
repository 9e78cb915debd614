"""Memory contract (tests/guarded.py) of the streaming step, the rate-aware ring write and ``stream_mark_end``: guard bands intact,
results independent of the poison in memory the op does not own, and -- beyond ``run_contract`` -- every byte of a destination
ring outside the step's block, and ``pos`` / ``end``, left exactly as they were.

The source ring has the capacity of ``max_chunk = 4`` and the step takes 3 frames, so the columns of the fourth frame hold the
arena's poison (0x00, NaN, 3.4e38) and are never read.  Every grid has a partly empty last workgroup: 3 / 12 / 33 rows of 64,
and 9 / 6 base positions in tiles of 8."""
import pytest
import torch

from audio_generation_amd import ops
from tests import codec_stream_ref as ref
from tests.guarded import Out, routed, run_contract
from tests.test_gpu_conv_stream import GpuOp, _unit

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, MAX_CHUNK = 3, 4
POS, END = [5, 1 << 33], [6, ref.LIVE]           # row 0 ends inside the step's block; row 1 is live and far along


def _columns(pos, n_cols, rate, delay, cap):
    return [torch.remainder(torch.arange(p * rate - delay, p * rate - delay + n_cols), cap) for p in pos]


def _poisoned_ring(arena, values, pos, rate, cap):
    """A ring of ``cap`` columns whose newest ``values.shape[2]`` columns (ending at the step's newest) hold ``values``; the rest
    keeps the arena's fill."""
    b, c, have = values.shape
    ring = arena.empty((b, c, cap))
    for r, p in enumerate(pos):
        cols = torch.remainder(torch.arange((p + N) * rate - have, (p + N) * rate), cap)
        ring[r][:, cols.to(ring.device)] = values[r].to(ring.device)
    return ring


@pytest.mark.parametrize("name", ["causal", "up", "res33"])
def test_step_memory_contract(name):
    unit, rate_in = _unit(name)
    first, last = unit[0], unit[-1]
    reach = first.d * (first.k - 1) if len(unit) == 2 else first.ref.reach
    rate_out, delay_out = first.ref.rates(rate_in, 0)
    cap, cap_out = reach + MAX_CHUNK * rate_in, MAX_CHUNK * rate_out + 3
    have = reach + N * rate_in                                    # what the step reads: the ring's other columns are poison
    gen = torch.Generator().manual_seed(17)
    values = torch.randn(2, first.c_in, have, generator=gen)
    clean = torch.zeros(2, first.c_in, cap, dtype=torch.float64)
    for r, cols in enumerate(_columns([p + N for p in POS], have, rate_in, have, cap)):
        clean[r][:, cols] = values[r].double()
    scratch = torch.zeros(2, last.c_out, cap_out, dtype=torch.float64)
    if len(unit) == 2:
        want, bound = ref.res_unit_step(first.ref, last.ref, clean, scratch, POS, END, N, rate_in, 0)
    else:
        want, bound = ref.step(first.ref, clean, scratch, POS, END, N, rate_in, 0)
    assert float(want[0].abs().max()) > 0 and float(want[0, :, -1].abs().max()) == 0.0      # row 0 crosses its end
    out_cols = _columns(POS, N * rate_out, rate_out, delay_out, cap_out)

    def run(arena):
        src = _poisoned_ring(arena, values, POS, rate_in, cap)
        dst = arena.empty((2, last.c_out, cap_out))
        pos, end = arena.place(torch.tensor(POS)), arena.place(torch.tensor(END))
        packed = [arena.place(op.packed.cpu()) for op in unit]
        bias = [arena.place(op.bias.cpu()) for op in unit]
        before = dst.clone()
        with routed(arena, ops):
            if len(unit) == 2:
                hid = arena.empty((2, first.c_out, N * rate_in))
                first.packed, first.bias, last.packed, last.bias = packed[0], bias[0], packed[1], bias[1]
                first.launch(src, hid, pos, None, N, rate_in, 0, dst_ring=False)
                last.launch(hid, dst, pos, end, N, rate_in, 0, src_ring=False, res=src)
            else:
                first.packed, first.bias = packed[0], bias[0]
                first.launch(src, dst, pos, end, N, rate_in, 0)
        torch.cuda.synchronize()
        keep = torch.ones(2, cap_out, dtype=torch.bool)
        for r, cols in enumerate(out_cols):
            keep[r, cols] = False
        keep = keep[:, None, :].expand(-1, last.c_out, -1).to(DEV)
        assert torch.equal(dst[keep].view(torch.int32), before[keep].view(torch.int32)), "columns outside the step's block were written"
        got = torch.stack([dst[r][:, cols.to(DEV)] for r, cols in enumerate(out_cols)])
        return [Out("block", got, want, 2.0 * float(bound.max())), Out("pos", pos, torch.tensor(POS), exact=True),
                Out("end", end, torch.tensor(END), exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


def test_plain_destination_is_written_whole():
    """The last layer of a stack: a plain (B, c_out, n * rate_out) tensor from poisoned memory, every element written."""
    op = GpuOp("causal", 6, 10, 11, s=5, pre=ref.SLOPE)
    rate_in, reach = 10, 6
    cap, have = reach + MAX_CHUNK * rate_in, reach + N * rate_in
    values = torch.randn(2, 6, have, generator=torch.Generator().manual_seed(23))
    clean = torch.zeros(2, 6, cap, dtype=torch.float64)
    for r, cols in enumerate(_columns([p + N for p in POS], have, rate_in, have, cap)):
        clean[r][:, cols] = values[r].double()
    want, bound = ref.step(op.ref, clean, torch.zeros(2, 10, N * 2, dtype=torch.float64), POS, None, N, rate_in, 0, dst_ring=False)

    def run(arena):
        src = _poisoned_ring(arena, values, POS, rate_in, cap)
        pos = arena.place(torch.tensor(POS))
        op.packed, op.bias = arena.place(op.packed.cpu()), arena.place(op.bias.cpu())
        with routed(arena, ops):
            out = op.launch(src, arena.empty((2, 10, N * 2)), pos, None, N, rate_in, 0, dst_ring=False)
        return [Out("out", out, want, 2.0 * float(bound.max())), Out("pos", pos, torch.tensor(POS), exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


def test_ring_write_rate_and_mark_end_memory_contract():
    b, c, rate, n, cap = 2, 5, 3, 3, 14
    x = torch.randn(b, c, n * rate, generator=torch.Generator().manual_seed(31))
    cols = _columns(POS, n * rate, rate, 0, cap)

    def run(arena):
        ring = arena.empty((b, c, cap))
        before = ring.clone()
        src, pos = arena.place(x), arena.place(torch.tensor(POS))
        end = arena.place(torch.tensor([ref.LIVE, 77, ref.LIVE]))
        pos3 = arena.place(torch.tensor([4, 9, 1 << 40]))
        rows = arena.place(torch.tensor([2, 0]))
        with routed(arena, ops):
            ops.ring_write_rate(ring, src, pos, rate)
            ops.stream_mark_end(pos3, end, rows)
        torch.cuda.synchronize()
        keep = torch.ones(b, cap, dtype=torch.bool)
        for r, cc in enumerate(cols):
            keep[r, cc] = False
        keep = keep[:, None, :].expand(-1, c, -1).to(DEV)
        assert torch.equal(ring[keep].view(torch.int32), before[keep].view(torch.int32))
        got = torch.stack([ring[r][:, cc.to(DEV)] for r, cc in enumerate(cols)])
        return [Out("written", got, x, exact=True), Out("pos", pos, torch.tensor(POS), exact=True),
                Out("end", end, torch.tensor([4, 77, 1 << 40]), exact=True), Out("pos3", pos3, torch.tensor([4, 9, 1 << 40]), exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]
