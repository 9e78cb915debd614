"""Memory contract (tests/guarded.py) of the five entry points of the streaming wavelet block -- ``wavelet_fold_table``, the in-step
and the out-step and their counted forms: guard bands intact, results independent of the poison in memory the op does not own, every
byte of a destination ring outside the step's block (and, counted, behind a row's count) and ``pos`` / ``end`` / ``counts`` left
exactly as they were.

As in tests/test_gpu_conv_stream_contract.py the source ring has the capacity of ``max_chunk = 4`` and the step takes 3 frames, so
the columns of the fourth frame hold the arena's poison (0x00, NaN, 3.4e38) and are never read.  Row 0 ends inside the step's block
-- for the out-step that puts the raw tail and the unread column L of h into the step -- row 1 is live and far along."""
import pytest
import torch

from audio_generation_amd import ops
from tests import wavelet_stream_ref as ref
from tests.guarded import Out, routed, run_contract
from tests.test_gpu_conv_stream_contract import MAX_CHUNK, N, _columns, _poisoned_ring
from tests.test_gpu_wavelet_stream import Block

pytestmark = pytest.mark.gpu
DEV = "cuda"
POS = [5, 1 << 33]
COUNTS = [2, 3]


def _case(name):
    k = Block(name)
    end0 = ((POS[0] + N) * k.rate_out - k.delay_out - 1) // k.rate_out      # row 0's last column is past its end, the others not
    assert POS[0] * k.rate_out - k.delay_out < end0 * k.rate_out
    end = [end0, ref.LIVE]
    cap, cap_out = k.reach + MAX_CHUNK * k.r, MAX_CHUNK * k.rate_out + 3
    have = k.reach + N * k.r
    values = torch.randn(2, k.c_src, have, generator=torch.Generator().manual_seed(17))
    clean = torch.zeros(2, k.c_src, cap, dtype=torch.float64)
    # the step's newest source column is (pos + N) r - d - 1
    for row, p in enumerate(POS):
        cols = torch.remainder(torch.arange((p + N) * k.r - k.d - have, (p + N) * k.r - k.d), cap)
        clean[row][:, cols] = values[row].double()
    want, bound = k.reference(clean, torch.zeros(2, k.c_dst, cap_out, dtype=torch.float64), POS, end, N)
    assert float(want[0, :, 0].abs().min()) > 0 and float(want[0, :, -1].abs().max()) == 0.0
    return k, end, cap, cap_out, values, want, bound


def _source(arena, k, values, cap):
    """``_poisoned_ring`` places the values so that they end at column (pos + N) rate: shift the positions by the delay."""
    assert k.d % k.r == 0
    return _poisoned_ring(arena, values, [p - k.d // k.r for p in POS], k.r, cap)


def _place_block(arena, k):
    k.img_in, k.img_out = arena.place(k.img_in.cpu()), arena.place(k.img_out.cpu())
    k.b_in, k.b_out, k.table = arena.place(k.b_in.cpu()), arena.place(k.b_out.cpu()), arena.place(k.table.cpu())


@pytest.mark.parametrize("counted", [False, True])
@pytest.mark.parametrize("name", ["in6", "in40", "out24", "out80sC", "out20"])
def test_step_memory_contract(name, counted):
    k, end_l, cap, cap_out, values, want, bound = _case(name)
    taken = [c if counted else N for c in COUNTS]
    out_cols = _columns(POS, N * k.rate_out, k.rate_out, k.delay_out, cap_out)

    def run(arena):
        src = _source(arena, k, values, cap)
        dst = arena.empty((2, k.c_dst, cap_out))
        pos, end = arena.place(torch.tensor(POS)), arena.place(torch.tensor(end_l))
        counts = arena.place(torch.tensor(COUNTS)) if counted else None
        _place_block(arena, k)
        before = dst.clone()
        with routed(arena, ops):
            k.launch(src, dst, pos, end, N, counts=counts)
        torch.cuda.synchronize()
        keep = torch.ones(2, cap_out, dtype=torch.bool)
        for row, cols in enumerate(out_cols):
            keep[row, cols[:taken[row] * k.rate_out]] = False
        keep = keep[:, None, :].expand(-1, k.c_dst, -1).to(DEV)
        assert torch.equal(dst[keep].view(torch.int32), before[keep].view(torch.int32)), "columns outside the step's block were written"
        outs = [Out(f"block row {row}", dst[row][:, cols[:taken[row] * k.rate_out].to(DEV)], want[row][:, :taken[row] * k.rate_out],
                    2.0 * float(bound.max())) for row, cols in enumerate(out_cols)]
        outs += [Out("pos", pos, torch.tensor(POS), exact=True), Out("end", end, torch.tensor(end_l), exact=True)]
        if counted:
            outs.append(Out("counts", counts, torch.tensor(COUNTS), exact=True))
        return outs
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


@pytest.mark.parametrize("counted", [False, True])
def test_plain_destination_is_written_whole(counted):
    """The last unit of a stack: a plain (B, c_out, n r s) tensor from poisoned memory, every element written -- exact 0 behind a
    row's count."""
    k, end_l, cap, cap_out, values, want, bound = _case("out24")
    want = want.clone()
    if counted:
        want[0, :, COUNTS[0] * k.rate_out:] = 0.0

    def run(arena):
        src = _source(arena, k, values, cap)
        pos, end = arena.place(torch.tensor(POS)), arena.place(torch.tensor(end_l))
        counts = arena.place(torch.tensor(COUNTS)) if counted else None
        _place_block(arena, k)
        with routed(arena, ops):
            out = k.launch(src, arena.empty((2, k.c_dst, N * k.rate_out)), pos, end, N, dst_ring=False, counts=counts)
        if counted:
            assert bool((out[0, :, COUNTS[0] * k.rate_out:] == 0).all())
        return [Out("out", out, want, 2.0 * float(bound.max())), Out("pos", pos, torch.tensor(POS), exact=True),
                Out("end", end, torch.tensor(end_l), exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


@pytest.mark.parametrize("hidden,s,p,sig_len", [(24, 4, 32, 24), (80, 2, 16, 1), (5, 8, 256, 5)])
def test_fold_table_memory_contract(hidden, s, p, sig_len):
    space = torch.linspace(-10, 10, p)
    sigma = 20.0 + 30.0 * torch.rand(sig_len, generator=torch.Generator().manual_seed(3))
    want = ref.fold_table64(space, sigma, hidden, s)
    tol = float((p + 4) * ref.U * ref.kern64(space, sigma, hidden).abs().sum(1).max())

    def run(arena):
        sp, sg = arena.place(space), arena.place(sigma)
        with routed(arena, ops):
            table = ops.wavelet_fold_table(sp, sg, hidden, s)
        return [Out("table", table, want, tol), Out("space", sp, space, exact=True), Out("sigma", sg, sigma, exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]
