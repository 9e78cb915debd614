"""Memory contract (tests/guarded.py) of the per-row stage counts: ``ops.rvq_step_encode(stages=)``,
``ops.rvq_step_decode(stages=)`` and ``ops.rvq_packets_restage`` at (B, n, D, K, Q) = (3, 4, 20, 24, 2) with sizes (24, 17), counts
(5, 2, -1) and stages (2, 1, 2).  Outputs, workspace and inputs sit between guard bands and start as poison; the latents behind a
row's count and the packet bytes behind a row's live bytes ARE the poison (NaN, 3.4e38, 0xFF codes that lie past every stage), so
a frame or a byte that must not be read shows as a changed result."""
import pytest
import torch

from audio_generation_amd import ops
from tests import rvq_stages_ref as sref
from tests import rvq_step_ref as ref
from tests.guarded import Out, routed, run_contract

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, N, D, K, Q, BITS = 3, 4, 20, 24, 2, 5
SIZES = (24, 17)
COUNTS = [N + 1, 2, -1]
TAKEN = [N, 2, 0]
STAGES = [2, 1, 2]
RESTAGE_TO = [1, 2, 0]
STAGES_OUT = [1, 1, 0]


@pytest.fixture(scope="module")
def case():
    gen = torch.Generator().manual_seed(81)
    z = torch.randn(B, D, N, generator=gen)
    cbs = torch.randn(Q, K, D, generator=gen) * torch.tensor([1.0, 0.6])[:, None, None]
    zq, index = sref.reference(z, cbs, SIZES, COUNTS, STAGES)
    packets = torch.from_numpy(sref.packets(index.numpy(), COUNTS, STAGES, BITS, Q))
    index_out = sref.reference(z, cbs, SIZES, COUNTS, STAGES_OUT)[1]
    restaged = torch.from_numpy(sref.packets(index_out.numpy(), COUNTS, STAGES_OUT, BITS, Q))
    assert sref.restaged(packets.numpy(), COUNTS, STAGES, RESTAGE_TO, BITS, Q, n=N)[1] == STAGES_OUT
    return z, cbs, zq, index, packets, restaged


def _poisoned_packets(arena, want_p):
    """The packets in the arena: a row's live bytes, and the arena's poison behind them."""
    pd = arena.empty(tuple(want_p.shape), dtype=torch.uint8)
    for r, (c, q) in enumerate(zip(TAKEN, STAGES)):
        live = sref.live_bytes(c, q, BITS)
        pd[r, :live] = want_p[r, :live].to(DEV)
    return pd


def test_staged_encode_memory_contract(case):
    z, cbs, want_q, want_i, want_p, _ = case

    def run(arena):
        zd = arena.empty((B, D, N))                              # behind a row's count: the arena's poison
        for r, c in enumerate(TAKEN):
            zd[r, :, :c] = z[r, :, :c].to(DEV)
        cd, counts, stages = arena.place(cbs), arena.place(torch.tensor(COUNTS)), arena.place(torch.tensor(STAGES))
        with routed(arena, ops):                                 # zq, index, packets and the workspace come from the arena
            zq, index, packets = ops.rvq_step_encode(zd, cd, Q, sizes=SIZES, counts=counts, stages=stages)
        return [Out("zq", zq, want_q, exact=True), Out("index", index, want_i, exact=True), Out("packets", packets, want_p, exact=True),
                Out("counts", counts, torch.tensor(COUNTS), exact=True), Out("stages", stages, torch.tensor(STAGES), exact=True),
                Out("codebooks", cd, cbs, exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


def test_staged_decode_memory_contract(case):
    _, cbs, want_q, want_i, want_p, _ = case

    def run(arena):
        pd = _poisoned_packets(arena, want_p)
        before = pd.clone()
        cd, counts, stages = arena.place(cbs), arena.place(torch.tensor(COUNTS)), arena.place(torch.tensor(STAGES))
        with routed(arena, ops):
            zq, index = ops.rvq_step_decode(pd, N, cd, Q, BITS, sizes=SIZES, counts=counts, want_index=True, stages=stages)
        torch.cuda.synchronize()
        assert torch.equal(pd, before), "the decode step wrote its packets"
        return [Out("zq", zq, want_q, exact=True), Out("index", index, want_i, exact=True),
                Out("counts", counts, torch.tensor(COUNTS), exact=True), Out("stages", stages, torch.tensor(STAGES), exact=True),
                Out("codebooks", cd, cbs, exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


def test_restage_memory_contract(case):
    _, _, _, _, want_p, want_r = case

    def run(arena):
        pd = _poisoned_packets(arena, want_p)
        before = pd.clone()
        counts, stages, to = arena.place(torch.tensor(COUNTS)), arena.place(torch.tensor(STAGES)), arena.place(torch.tensor(RESTAGE_TO))
        with routed(arena, ops):                                 # the packets and the stage counts it returns come from the arena
            packets, stages_out = ops.rvq_packets_restage(pd, N, Q, BITS, to, stages, counts)
        torch.cuda.synchronize()
        assert torch.equal(pd, before), "restage wrote its input packets"
        return [Out("packets", packets, want_r, exact=True), Out("stages_out", stages_out, torch.tensor(STAGES_OUT), exact=True),
                Out("counts", counts, torch.tensor(COUNTS), exact=True), Out("stages", stages, torch.tensor(STAGES), exact=True),
                Out("stages_to", to, torch.tensor(RESTAGE_TO), exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]
