"""The RVQ streaming step (``ops.rvq_step_encode`` / ``ops.rvq_step_decode``) on the GPU, bit for bit.

The search is the definition: ``index`` and ``zq`` equal the stage-by-stage ``oracle.rvq.exact_search`` reference
(tests/rvq_step_ref.py), on plain shapes, on planted decisions that only the defining arithmetic gets right (each one verified here
on the CPU before the kernel is asked), and on the operand families of tests/test_gpu_rvq_adversarial.py.  Then the per-row counts
and the packets.  No tolerance anywhere.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

from audio_generation_amd import ops
from audio_generation_amd._lib import AgxError
from oracle import rvq
from tests import rvq_step_ref as ref
from tests.test_gpu_rvq_adversarial import _plant_near_ties

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _strided(x: torch.Tensor) -> torch.Tensor:
    """(B, n, D) frames on the device -> the (B, D, n) view of a transposition (strides (n D, 1, D))."""
    return x.to(DEV).transpose(1, 2)


def _check(x: torch.Tensor, cbs: torch.Tensor, sizes=None, bits=None):
    """Encode (B, n, D) frames and hold index and zq against the definition; -> (zq, index, packets) on the device."""
    want_q, want_i = ref.exact_reference(x.transpose(1, 2), cbs, sizes)
    zq, index, packets = ops.rvq_step_encode(_strided(x), cbs.to(DEV), cbs.shape[0], sizes=sizes, bits=bits)
    n_bad = int((index.cpu() != want_i).sum())
    assert n_bad == 0, f"{n_bad} of {want_i.numel()} indices differ from the full defining search"
    assert zq.shape == want_q.shape and zq.is_contiguous() and torch.equal(zq.cpu(), want_q), "zq is not bit-identical"
    return zq, index, packets


def _codebooks(q, k, d, gen):
    return torch.randn(q, k, d, generator=gen) * (0.6 ** torch.arange(q, dtype=torch.float32))[:, None, None]


# ------------------------------------------------------------------------------------------------ 1. the search is the definition
@pytest.mark.parametrize("b,n,d,k,q", [(1, 1, 16, 32, 2), (2, 3, 16, 65, 3), (9, 4, 512, 1024, 8), (2, 2, 560, 130, 2)])
def test_search_is_the_definition(b, n, d, k, q):
    """One frame, K one past a wave, config S's quantiser on 36 frames, and the widest D ``agx_rvq_forward`` takes."""
    gen = torch.Generator().manual_seed(1000 + d + k)
    _check(torch.randn(b, n, d, generator=gen), _codebooks(q, k, d, gen))


def test_search_with_a_short_stage_never_reads_behind_it():
    """(3, 4, 20, 24, 2) with sizes (24, 17): D no multiple of 4 or 8, K below a wave.  The rows behind stage 1's 17 codewords
    hold the stage-1 residuals of the first frames themselves -- distance 0 -- so a search that looked there would take them."""
    gen = torch.Generator().manual_seed(7)
    b, n, d, k, q, sizes = 3, 4, 20, 24, 2, (24, 17)
    x, cbs = torch.randn(b, n, d, generator=gen), _codebooks(q, k, d, gen)
    _, idx = ref.exact_reference(x.transpose(1, 2), cbs, sizes)
    r1 = x.reshape(-1, d) - cbs[0][idx.reshape(-1, q)[:, 0]]
    cbs[1, 17:] = r1[:k - 17]
    assert int(rvq.exact_search(r1.numpy(), cbs[1].numpy())[0]) == 17          # the bait works on an unsized search
    zq, index, packets = _check(x, cbs, sizes)
    assert int(index[..., 1].max()) < 17 and packets.shape == (b, ref.packet_bytes(n, q, 5))


# ------------------------------------------------------------------------------------------------ 2. planted decisions, D = 16
def _far(k, d, gen, offset):
    """Codewords nobody chooses: ``offset`` away from the origin in every dimension."""
    return torch.randn(1, k, d, generator=gen) + offset


def _dist_defining(r, c):
    acc = 0.0
    for a, b in zip(r.tolist(), c.tolist()):
        diff = a - b
        sq = diff * diff
        acc = acc + sq
    return acc


def _dist_fused(r, c):
    """The same chain with a fused multiply-add: ``acc <- fl64(acc + diff^2)``, the square never rounded (exact, ``fractions``)."""
    acc = 0.0
    for a, b in zip(r.tolist(), c.tolist()):
        diff = a - b
        acc = float(Fraction(acc) + Fraction(diff) ** 2)
    return acc


def _decide(r, cbs, want):
    """One frame ``r`` (D,) against one stage: the CPU definition says ``want``, and so must the kernel."""
    assert int(rvq.exact_search(r[None].numpy(), cbs[0].numpy())[0]) == want
    _, index, _ = _check(r[None, None], cbs)
    assert int(index[0, 0, 0]) == want


def test_planted_duplicate_in_another_workgroup_takes_the_lower_index():
    gen = torch.Generator().manual_seed(21)
    k, d = 1024, 16
    cbs = torch.randn(1, k, d, generator=gen)
    cbs[0, k - 2] = cbs[0, 3]
    r = cbs[0, 3] + 2.0 ** -6 * torch.randn(d, generator=gen)
    assert _dist_defining(r, cbs[0, 3]) == _dist_defining(r, cbs[0, k - 2]) < min(
        _dist_defining(r, cbs[0, j]) for j in range(k) if j not in (3, k - 2))
    _decide(r, cbs, 3)


def test_planted_pair_equal_in_binary32_apart_in_binary64():
    gen = torch.Generator().manual_seed(22)
    k, d = 128, 16
    cbs = _far(k, d, gen, 8.0)
    cbs[0, 3], cbs[0, 7] = 0.0, 0.0
    cbs[0, 3, 0], cbs[0, 3, 1], cbs[0, 7, 0] = 1.0, 2.0 ** -13, 1.0
    r = torch.zeros(d)
    d3, d7 = _dist_defining(r, cbs[0, 3]), _dist_defining(r, cbs[0, 7])
    assert d3 == 1.0 + 2.0 ** -26 and d7 == 1.0 and np.float32(d3) == np.float32(d7)
    _decide(r, cbs, 7)


def test_planted_pair_that_only_the_d_order_separates():
    gen = torch.Generator().manual_seed(23)
    k, d = 128, 16
    cbs = _far(k, d, gen, 2.0 ** 28)
    cbs[0, 2], cbs[0, 9] = 0.0, 0.0
    cbs[0, 2, 0], cbs[0, 2, 1] = 2.0 ** 27, 2.0
    cbs[0, 9, 0] = 2.0 ** 27
    cbs[0, 9, 1:5] = 1.0
    r = torch.zeros(d)
    d2, d9 = _dist_defining(r, cbs[0, 2]), _dist_defining(r, cbs[0, 9])
    assert d9 == 2.0 ** 54 < d2 == 2.0 ** 54 + 4.0                               # the four ones are lost one by one
    assert _dist_defining(r.flip(0), cbs[0, 9].flip(0)) == d2                    # any order that adds them first ties and takes 2
    _decide(r, cbs, 9)


def _fused_pair():
    """Seeded search for (r, c_a, c_b) with dist(c_a) < dist(c_b) under the defining arithmetic and the opposite strict order under
    a fused multiply-add.  r is constant over d and c_b a permutation of c_a, so the two distances are equal in exact arithmetic
    and only the roundings order them."""
    d = 16
    for seed in range(400):
        gen = torch.Generator().manual_seed(5000 + seed)
        r = torch.full((d,), float(torch.randn((), generator=gen)))
        ca = torch.randn(d, generator=gen)
        cb = ca[torch.randperm(d, generator=gen)]
        da, db = _dist_defining(r, ca), _dist_defining(r, cb)
        fa, fb = _dist_fused(r, ca), _dist_fused(r, cb)
        if da < db and fa > fb:
            return r, ca, cb
        if db < da and fb > fa:
            return r, cb, ca
    return None


def test_planted_pair_whose_order_a_fused_multiply_add_reverses():
    found = _fused_pair()
    assert found is not None, "no pair in 400 seeds"
    r, win, lose = found
    gen = torch.Generator().manual_seed(24)
    cbs = _far(64, 16, gen, 16.0)
    cbs[0, 5], cbs[0, 41] = lose, win            # the defining winner at the higher index: no tie rule can rescue a fused search
    _decide(r, cbs, 41)


def _family(name, gen, b=2, n=2, d=64, k=96, q=2):
    """The operand families of tests/test_gpu_rvq_adversarial.py at (2, 2, 64, 96, 2)."""
    if name == "magnitudes":
        scale = torch.pow(2.0, -20.0 * torch.rand(d, generator=gen))
        cbs = torch.randn(q, k, d, generator=gen) * scale
        cbs[1:] *= 0.5
        _plant_near_ties(cbs, gen, 2.0 ** -12)
        x = torch.randn(b, n, d, generator=gen) * scale
        x[0, 0] = cbs[0, 11] * (1 + 2.0 ** -10 * torch.randn(d, generator=gen))
    elif name == "cancellation":
        alt = torch.tensor([1.0, -1.0]).repeat((d + 1) // 2)[:d]
        cbs = (1.0 + 2.0 ** -9 * torch.randn(q, k, d, generator=gen)) * torch.ones(d)
        cbs[:, ::3] *= -1.0
        _plant_near_ties(cbs, gen, 2.0 ** -14)
        x = alt * (1.0 + 2.0 ** -9 * torch.randn(b, n, d, generator=gen))
    else:
        cbs = torch.randn(q, k, d, generator=gen) * 2.0 ** -6
        big = 37 % d
        cbs[:, :, big] = torch.randn(q, k, generator=gen).sign() * 1024.0 * (1 + 0.01 * torch.randn(q, k, generator=gen))
        cbs[:, 1::2] = cbs[:, 0::2]
        cbs[:, 1::2, :big] += 2.0 ** -12 * torch.randn(q, k // 2, big, generator=gen)
        x = torch.randn(b, n, d, generator=gen) * 2.0 ** -6
        x[..., big] = torch.randn(b, n, generator=gen).sign() * 1024.0
    return x, cbs


@pytest.mark.parametrize("name", ["magnitudes", "cancellation", "huge"])
def test_adversarial_operand_families(name):
    x, cbs = _family(name, torch.Generator().manual_seed({"magnitudes": 31, "cancellation": 32, "huge": 33}[name]))
    _check(x, cbs)


# ------------------------------------------------------------------------------------------------ 3. counts
COUNTS = (0, 1, 4, 9, -3)
TAKEN = (0, 1, 4, 4, 0)


@pytest.fixture(scope="module")
def counted():
    """B = 5, n = 4, D = 20, K = 24 with sizes (24, 17), 5-bit codes: the clean frames, the codebooks, the uncounted call."""
    gen = torch.Generator().manual_seed(41)
    b, n, d, k, q, sizes = len(COUNTS), 4, 20, 24, 2, (24, 17)
    x, cbs = torch.randn(b, n, d, generator=gen), _codebooks(q, k, d, gen)
    zq, index, packets = _check(x, cbs, sizes)
    return x, cbs, sizes, zq, index, packets


def test_counts_keep_dead_frames_out_of_every_output(counted):
    x, cbs, sizes, zq_all, index_all, _ = counted
    b, n, d = x.shape
    q, bits = cbs.shape[0], 5
    assert ref.taken(COUNTS, b, n) == list(TAKEN)
    dirty = x.clone()
    for r, c in enumerate(TAKEN):
        dirty[r, c:] = float("nan")                            # NaN latents behind every count
    counts = torch.tensor(COUNTS, dtype=torch.int64, device=DEV)
    zq, index, packets = ops.rvq_step_encode(_strided(dirty), cbs.to(DEV), q, sizes=sizes, counts=counts)
    assert not torch.isnan(zq).any()
    want_q, want_i = ref.behind_counts(zq_all.cpu(), index_all.cpu(), COUNTS)
    assert torch.equal(zq.cpu(), want_q) and torch.equal(index.cpu(), want_i)      # live: the uncounted call; dead: exact 0 and -1
    for r, c in enumerate(TAKEN):
        assert float(zq[r, :, c:].abs().max() if c < n else 0.0) == 0.0 and bool((index[r, c:] == -1).all())
    assert np.array_equal(packets.cpu().numpy(), ref.packets(index_all.cpu().numpy(), COUNTS, bits))
    for r, c in enumerate(TAKEN):
        live = ref.packet_bytes(c, q, bits) if c else 0
        assert not packets[r, live:].any(), r
    assert not packets[0].any() and not packets[4].any()        # a row with count 0 leaves its whole packet row 0
    no_zq, index2, packets2 = ops.rvq_step_encode(_strided(dirty), cbs.to(DEV), q, sizes=sizes, counts=counts, want_zq=False)
    assert no_zq is None and torch.equal(index2, index) and torch.equal(packets2, packets)


# ------------------------------------------------------------------------------------------------ 4. packets
def _packet_round_trip(x, cbs, sizes, bits, counts_list):
    b, n, d = x.shape
    q = cbs.shape[0]
    cd = cbs.to(DEV)
    counts = None if counts_list is None else torch.tensor(counts_list, dtype=torch.int64, device=DEV)
    zq, index, packets = ops.rvq_step_encode(_strided(x), cd, q, sizes=sizes, counts=counts, bits=bits)
    assert packets.dtype == torch.uint8 and packets.shape == (b, ref.packet_bytes(n, q, bits))
    for r, c in enumerate(ref.taken(counts_list, b, n)):
        if c:
            lead = ops.codes_pack(index[r, :c], bits)
            assert torch.equal(packets[r, :lead.numel()], lead) and not packets[r, lead.numel():].any(), r
        else:
            assert not packets[r].any()
    back_q, back_i = ops.rvq_step_decode(packets, n, cd, q, bits, sizes=sizes, counts=counts, want_index=True)
    assert torch.equal(back_i, index) and torch.equal(back_q, zq)
    assert torch.equal(ops.rvq_step_decode(packets, n, cd, q, bits, sizes=sizes, counts=counts), zq)
    return zq, index, packets


def test_packets_of_10_bit_codes_round_trip_and_equal_rvq_forward():
    gen = torch.Generator().manual_seed(51)
    b, n, d, k, q = 3, 4, 64, 1024, 3
    x, cbs = torch.randn(b, n, d, generator=gen), _codebooks(q, k, d, gen)
    zq, index, _ = _packet_round_trip(x, cbs, None, 10, None)
    cd = cbs.to(DEV)
    xq, idx, _, _ = ops.rvq_forward(_strided(x), cd, ops.rvq_pack(cd), q, layout="b c l")
    assert torch.equal(idx, index) and torch.equal(xq, zq)
    _packet_round_trip(x, cbs, None, 10, [2, 0, 7])


def test_packets_of_5_bit_codes_round_trip_and_equal_rvq_forward():
    gen = torch.Generator().manual_seed(52)
    b, n, d, k, q, sizes = 3, 3, 20, 24, 2, (24, 17)         # 10-bit frames: every row's packet ends mid-byte at counts 1 and 3
    x, cbs = torch.randn(b, n, d, generator=gen), _codebooks(q, k, d, gen)
    zq, index, _ = _packet_round_trip(x, cbs, sizes, 5, None)
    cd = cbs.to(DEV)
    xq, idx, _, _ = ops.rvq_forward(_strided(x), cd, ops.rvq_pack(cd, sizes), q, layout="b c l")
    assert torch.equal(idx, index) and torch.equal(xq, zq)
    _packet_round_trip(x, cbs, sizes, 5, [1, 3, 0])


def test_codes_past_a_stage_select_no_codeword():
    """A packet of 0xFF bytes at K = 24: every 5-bit code is 31 >= 24.  The contract says such a code adds nothing and reads
    nothing, so zq is exact 0 -- an in-bounds check of the decode step."""
    gen = torch.Generator().manual_seed(53)
    b, n, d, k, q = 2, 3, 20, 24, 2
    cd = _codebooks(q, k, d, gen).to(DEV)
    packets = torch.full((b, ref.packet_bytes(n, q, 5)), 0xFF, dtype=torch.uint8, device=DEV)
    zq, index = ops.rvq_step_decode(packets, n, cd, q, 5, want_index=True)
    assert float(zq.abs().max()) == 0.0 and bool((index == 31).all())
    zq, index = ops.rvq_step_decode(packets, n, cd, q, 5, sizes=(24, 17), want_index=True)
    assert float(zq.abs().max()) == 0.0 and bool((index == 31).all())


def test_no_stage_and_refusals():
    gen = torch.Generator().manual_seed(54)
    x, cd = torch.randn(2, 3, 16, generator=gen), _codebooks(2, 32, 16, gen).to(DEV)
    zq, index, packets = ops.rvq_step_encode(_strided(x), cd, 0)
    assert float(zq.abs().max()) == 0.0 and index.shape == (2, 3, 0) and packets.shape == (2, 0)
    assert float(ops.rvq_step_decode(packets, 3, cd, 0, 5).abs().max()) == 0.0
    with pytest.raises(AgxError, match=f"n={ops.RVQ_STEP_MAX_N + 1}"):
        ops.rvq_step_encode(torch.zeros(1, 16, ops.RVQ_STEP_MAX_N + 1, device=DEV), cd, 2)
    with pytest.raises(AgxError, match="cannot hold"):
        ops.rvq_step_encode(_strided(x), cd, 2, bits=4)                                  # 32 codewords in 4-bit codes
    with pytest.raises(AgxError, match="frame dim"):
        ops.rvq_step_encode(torch.zeros(1, 8, 2, device=DEV), cd, 2)
    with pytest.raises(AgxError, match="counts"):
        ops.rvq_step_encode(_strided(x), cd, 2, counts=torch.zeros(3, dtype=torch.int64, device=DEV))
    with pytest.raises(AgxError, match=r"uint8 \(B, 4\)"):
        ops.rvq_step_decode(torch.zeros(2, 5, dtype=torch.uint8, device=DEV), 3, cd, 2, 5)
    zq, index, _ = ops.rvq_step_encode(torch.zeros(1, 16, ops.RVQ_STEP_MAX_N, device=DEV), cd, 2)     # the widest step
    assert index.shape == (1, ops.RVQ_STEP_MAX_N, 2) and bool((index[0] == index[0, 0]).all())
