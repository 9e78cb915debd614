"""Memory contract (tests/guarded.py) of the RVQ streaming step: ``ops.rvq_step_encode`` and ``ops.rvq_step_decode`` at
(B, n, D, K, Q) = (3, 4, 20, 24, 2) with sizes (24, 17) and mixed counts -- all four frames, two, and -1 (nothing).  Outputs,
workspace and inputs sit between guard bands and start as poison; the latents and the packet bytes behind a row's count ARE the
poison (NaN, 3.4e38, 0xFF codes that lie past every stage), so a frame or a byte that must not be read shows as a changed result."""
import pytest
import torch

from audio_generation_amd import ops
from tests import rvq_step_ref as ref
from tests.guarded import Out, routed, run_contract

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, N, D, K, Q, BITS = 3, 4, 20, 24, 2, 5
SIZES = (24, 17)
COUNTS = [N + 1, 2, -1]
TAKEN = [N, 2, 0]


@pytest.fixture(scope="module")
def case():
    gen = torch.Generator().manual_seed(61)
    z = torch.randn(B, D, N, generator=gen)
    cbs = torch.randn(Q, K, D, generator=gen) * torch.tensor([1.0, 0.6])[:, None, None]
    zq, index = ref.behind_counts(*ref.exact_reference(z, cbs, SIZES), COUNTS)
    packets = torch.from_numpy(ref.packets(ref.exact_reference(z, cbs, SIZES)[1].numpy(), COUNTS, BITS))
    return z, cbs, zq, index, packets


def test_step_encode_memory_contract(case):
    z, cbs, want_q, want_i, want_p = case

    def run(arena):
        zd = arena.empty((B, D, N))                              # behind a row's count: the arena's poison
        for r, c in enumerate(TAKEN):
            zd[r, :, :c] = z[r, :, :c].to(DEV)
        cd, counts = arena.place(cbs), arena.place(torch.tensor(COUNTS))
        with routed(arena, ops):                                 # zq, index, packets and the workspace come from the arena
            zq, index, packets = ops.rvq_step_encode(zd, cd, Q, sizes=SIZES, counts=counts)
        return [Out("zq", zq, want_q, exact=True), Out("index", index, want_i, exact=True), Out("packets", packets, want_p, exact=True),
                Out("counts", counts, torch.tensor(COUNTS), exact=True), Out("codebooks", cd, cbs, exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


def test_step_decode_memory_contract(case):
    _, cbs, want_q, want_i, want_p = case

    def run(arena):
        pd = arena.empty(tuple(want_p.shape), dtype=torch.uint8)  # behind a row's packet: the arena's poison
        for r, c in enumerate(TAKEN):
            live = ref.packet_bytes(c, Q, BITS) if c else 0
            pd[r, :live] = want_p[r, :live].to(DEV)
        before = pd.clone()
        cd, counts = arena.place(cbs), arena.place(torch.tensor(COUNTS))
        with routed(arena, ops):
            zq, index = ops.rvq_step_decode(pd, N, cd, Q, BITS, sizes=SIZES, counts=counts, want_index=True)
        torch.cuda.synchronize()
        assert torch.equal(pd, before), "the decode step wrote its packets"
        return [Out("zq", zq, want_q, exact=True), Out("index", index, want_i, exact=True),
                Out("counts", counts, torch.tensor(COUNTS), exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]
