"""Memory contract (tests/guarded.py) of the four entry points of DESIGN 4.24 -- ``multires_stream_step``,
``conv_stream_step_affine`` and their counted forms -- exactly as tests/test_gpu_wavelet_stream_contract.py does it: guard bands
intact, results independent of the poison in memory the op does not own, every byte of a destination ring outside the step's block
(and, counted, behind a row's count) and ``pos`` / ``end`` / ``counts`` left exactly as they were.

The source ring has the capacity of ``max_chunk = 4`` and the step takes 3 frames, so the columns of the fourth frame hold the
arena's poison (0x00, NaN, 3.4e38) and are never read; counted, neither are the columns behind a row's count.  Row 0 ends inside the
step's block; row 1 is live at ``pos = 1 << 33``."""
import pytest
import torch

from audio_generation_amd import ops
from audio_generation_amd._lib import CONV_CAUSAL, EPI_LEAKY_PRE
from tests import codec_stream_ref as cref
from tests import multires_stream_ref as ref
from tests.guarded import Out, routed, run_contract
from tests.test_gpu_conv_stream_contract import MAX_CHUNK, N, POS, _columns, _poisoned_ring
from tests.test_gpu_multires_stream import MULTIRES_TOL, _case

pytestmark = pytest.mark.gpu
DEV = "cuda"
COUNTS = [2, 3]
CASES = ("mr6", "mr33wide", "mr3tiles", "dw33", "dw16")       # the cases of tests/test_gpu_multires_stream.py at delay 0


def _setup(name, counted):
    """The values the step reads, the clean float64 ring, the expected block and its tolerance."""
    k = _case(name)
    assert k.delay == 0
    end = [POS[0] + N - 1, cref.LIVE] if k.kind == "multires" else None       # row 0's last frame is past its end
    cap, cap_out = k.reach + MAX_CHUNK * k.rate, MAX_CHUNK * k.rate + 3
    have = k.reach + N * k.rate
    values = torch.randn(2, k.c, have, generator=torch.Generator().manual_seed(17))
    taken = [c if counted else N for c in COUNTS]
    clean = torch.zeros(2, k.c, cap, dtype=torch.float64)
    for r, cols in enumerate(_columns([p + N for p in POS], have, k.rate, have, cap)):
        clean[r][:, cols] = values[r].double()
    counts = COUNTS if counted else None
    if k.kind == "multires":
        want = ref.multires_step(k.h0.double(), k.h1.double(), k.w.double(), k.depth, clean, torch.zeros(2, k.c, cap_out, dtype=torch.float64),
                                 POS, end, N, k.rate, 0, counts=counts)
        tol = torch.full_like(want, MULTIRES_TOL / 2.0)
        assert float(want[0, :, :k.rate].abs().min()) > 0 and float(want[0, :, (N - 1) * k.rate:].abs().max()) == 0.0
    else:
        want, tol = ref.affine_step(k.op1, k.scale, k.shift, clean, torch.zeros(2, k.c, N * k.rate, dtype=torch.float64), POS, N, k.rate, 0,
                                    counts=counts)
    return k, end, cap, cap_out, values, taken, want, tol


def _poisoned_source(arena, k, values, cap, taken):
    """``_poisoned_ring``, and the arena's fill again in the columns behind a row's count."""
    ring = _poisoned_ring(arena, values, POS, k.rate, cap)
    fill = arena.empty((2, k.c, cap))
    for r, p in enumerate(POS):
        cols = torch.remainder(torch.arange((p + taken[r]) * k.rate, (p + N) * k.rate), cap).to(DEV)
        ring[r][:, cols] = fill[r][:, cols]
    return ring


@pytest.mark.parametrize("counted", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_step_memory_contract(name, counted):
    """The multires step into a ring; the affine conv into its plain scratch (it has no other use in a stream), written whole."""
    k, end_l, cap, cap_out, values, taken, want, tol = _setup(name, counted)
    ring_dst = k.kind == "multires"
    out_cols = _columns(POS, N * k.rate, k.rate, 0, cap_out)

    def run(arena):
        src = _poisoned_source(arena, k, values, cap, taken)
        dst = arena.empty((2, k.c, cap_out if ring_dst else N * k.rate))
        pos = arena.place(torch.tensor(POS))
        end = arena.place(torch.tensor(end_l)) if end_l is not None else None
        counts = arena.place(torch.tensor(COUNTS)) if counted else None
        before = dst.clone()
        with routed(arena, ops):
            if ring_dst:
                h0, h1, w = (arena.place(t) for t in (k.h0, k.h1, k.w))
                ops.multires_stream_step(h0, h1, w, k.depth, src, dst, pos, N, k.rate, 0, end=end, counts=counts)
            else:
                img, b1, sc, sh = (arena.place(t.cpu()) for t in (k.img1, k.b1, k.sc, k.sh))
                ops.conv_stream_step_affine(k.c, k.c, k.k, k.d, img, b1, sc, sh, src, dst, pos, N, k.rate, 0, dst_ring=False,
                                            epilogue=EPI_LEAKY_PRE, slope=cref.SLOPE, counts=counts)
        torch.cuda.synchronize()
        outs = [Out("pos", pos, torch.tensor(POS), exact=True)]
        if ring_dst:
            keep = torch.ones(2, cap_out, dtype=torch.bool)
            for r, cols in enumerate(out_cols):
                keep[r, cols[:taken[r] * k.rate]] = False
            keep = keep[:, None, :].expand(-1, k.c, -1).to(DEV)
            assert torch.equal(dst[keep].view(torch.int32), before[keep].view(torch.int32)), "columns outside the step's block were written"
            outs += [Out(f"block row {r}", dst[r][:, cols[:taken[r] * k.rate].to(DEV)], want[r][:, :taken[r] * k.rate],
                         2.0 * float(tol.max())) for r, cols in enumerate(out_cols)]
            outs.append(Out("end", end, torch.tensor(end_l), exact=True))
        else:
            for r in range(2):
                assert bool((dst[r, :, taken[r] * k.rate:] == 0).all())                      # exact 0 behind the count
            outs.append(Out("hidden", dst, want, 2.0 * float(tol.max())))
        if counted:
            outs.append(Out("counts", counts, torch.tensor(COUNTS), exact=True))
        return outs
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


@pytest.mark.parametrize("counted", [False, True])
def test_multires_plain_destination_is_written_whole(counted):
    """The last unit of a stack: a plain (B, C, n rate) tensor from poisoned memory, every element written -- exact 0 behind a
    row's count and past row 0's end."""
    k, end_l, cap, cap_out, values, taken, want, tol = _setup("mr33wide", counted)

    def run(arena):
        src = _poisoned_source(arena, k, values, cap, taken)
        pos, end = arena.place(torch.tensor(POS)), arena.place(torch.tensor(end_l))
        counts = arena.place(torch.tensor(COUNTS)) if counted else None
        h0, h1, w = (arena.place(t) for t in (k.h0, k.h1, k.w))
        with routed(arena, ops):
            out = ops.multires_stream_step(h0, h1, w, k.depth, src, arena.empty((2, k.c, N * k.rate)), pos, N, k.rate, 0, dst_ring=False,
                                           end=end, counts=counts)
        assert bool((out[0, :, min(taken[0], N - 1) * k.rate:] == 0).all())
        return [Out("out", out, want, 2.0 * float(tol.max())), Out("pos", pos, torch.tensor(POS), exact=True),
                Out("end", end, torch.tensor(end_l), exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


def test_depthwise_unit_into_a_ring_memory_contract():
    """The two launches of a depthwise unit as a stream runs them, counted, into the consumer's ring; row 0 ends inside the block."""
    k = _case("dw33")
    end_l = [POS[0] + N - 1, cref.LIVE]
    cap, cap_out = k.reach + MAX_CHUNK * k.rate, MAX_CHUNK * k.rate + 3
    have = k.reach + N * k.rate
    values = torch.randn(2, k.c, have, generator=torch.Generator().manual_seed(19))
    clean = torch.zeros(2, k.c, cap, dtype=torch.float64)
    for r, cols in enumerate(_columns([p + N for p in POS], have, k.rate, have, cap)):
        clean[r][:, cols] = values[r].double()
    want, bound = ref.resdw_unit_step(k.op1, k.op2, k.scale, k.shift, clean, torch.zeros(2, k.c, cap_out, dtype=torch.float64), POS, end_l,
                                      N, k.rate, 0, counts=COUNTS)
    out_cols = _columns(POS, N * k.rate, k.rate, 0, cap_out)

    def run(arena):
        src = _poisoned_source(arena, k, values, cap, COUNTS)
        dst, hid = arena.empty((2, k.c, cap_out)), arena.empty((2, k.c, N * k.rate))
        pos, end, counts = arena.place(torch.tensor(POS)), arena.place(torch.tensor(end_l)), arena.place(torch.tensor(COUNTS))
        img1, img2, b1, b2, sc, sh = (arena.place(t.cpu()) for t in (k.img1, k.img2, k.b1, k.b2, k.sc, k.sh))
        before = dst.clone()
        with routed(arena, ops):
            ops.conv_stream_step_affine(k.c, k.c, k.k, k.d, img1, b1, sc, sh, src, hid, pos, N, k.rate, 0, dst_ring=False,
                                        epilogue=EPI_LEAKY_PRE, slope=cref.SLOPE, counts=counts)
            ops.conv_stream_step(CONV_CAUSAL, k.c, k.c, 1, 1, 1, img2, b2, hid, dst, pos, N, k.rate, 0, src_ring=False, res=src, end=end,
                                 epilogue=ops.EPI_RESIDUAL | ops.EPI_LEAKY_POST, slope=cref.SLOPE, counts=counts)
        torch.cuda.synchronize()
        keep = torch.ones(2, cap_out, dtype=torch.bool)
        for r, cols in enumerate(out_cols):
            keep[r, cols[:COUNTS[r] * k.rate]] = False
        keep = keep[:, None, :].expand(-1, k.c, -1).to(DEV)
        assert torch.equal(dst[keep].view(torch.int32), before[keep].view(torch.int32)), "columns outside the step's block were written"
        outs = [Out(f"block row {r}", dst[r][:, cols[:COUNTS[r] * k.rate].to(DEV)], want[r][:, :COUNTS[r] * k.rate],
                    2.0 * float(bound.max())) for r, cols in enumerate(out_cols)]
        return outs + [Out("pos", pos, torch.tensor(POS), exact=True), Out("end", end, torch.tensor(end_l), exact=True),
                       Out("counts", counts, torch.tensor(COUNTS), exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]
