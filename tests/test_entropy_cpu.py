"""Entropy coding without a GPU: the mirror of tests/entropy_ref.py against what the contract promises -- tables
that sum to M with every code present, a coder that round-trips, the packet lengths that can be worked out by hand -- and the
refusals the wrappers and the library make on the host, before any launch."""
import numpy as np
import pytest
import torch

from audio_generation_amd import _lib, ops
from tests import entropy_ref as ref


def _cum_of(fs):
    return np.concatenate([[0], np.cumsum(fs)]).astype(np.int64)


@pytest.mark.parametrize("size", [1, 5, 16, 1024, 2048])
def test_mirror_tables_sum_to_m_and_the_coder_round_trips(size):
    rng = np.random.default_rng(size)
    n, n_q, k = 6, 2, size
    logits = (2.0 * rng.standard_normal((1, n_q * k, n))).astype(np.float32)
    cum, decided, arg = ref.tables(logits, n_q)
    f = np.diff(cum, axis=-1)
    assert np.all(cum[..., 0] == 0) and np.all(cum[..., -1] == ref.M) and f.min() >= 1
    assert np.all(arg == logits.reshape(1, n_q, k, n).argmax(axis=2).transpose(0, 2, 1))
    assert (~decided).sum() <= 1e-4 * decided.size
    codes = rng.integers(0, size, (1, n, n_q))
    packets, nbytes, status = ref.encode(cum, codes)
    assert status[0] == 0 and 4 <= nbytes[0] <= 2 * n * n_q + 4 and not packets[0, nbytes[0]:].any()
    got, state, st, _ = ref.decode(cum, packets, nbytes)
    assert np.array_equal(got, codes) and st[0] == 0 and tuple(state[0]) == (ref.L, nbytes[0])
    # the coded length follows the model: within 4 + 1 bytes of the sum of -log2(f / M)
    bits = -np.log2(np.take_along_axis(f, codes[..., None], axis=-1) / ref.M).sum()
    assert abs(int(nbytes[0]) - 4 - bits / 8) <= 1.0 + 0.01 * bits / 8


def test_mirror_lengths_that_can_be_worked_out_by_hand():
    # every coded f is 1: two bytes per symbol, 2 N + 4 in all -- the row width P is reached and never exceeded
    n_sym = 9
    l = np.zeros(16, dtype=np.float32)
    l[3] = 60.0                                             # exp(-60) * 65520 < 1: every other code has f = 1
    f, decided, a = ref.table_row(l)
    assert a == 3 and decided.all() and f[3] == ref.M - 15 and np.all(np.delete(f, 3) == 1)
    cum = np.broadcast_to(_cum_of(f), (1, n_sym, 1, 17))
    codes = np.full((1, n_sym, 1), 7)
    packets, nbytes, _ = ref.encode(cum, codes)
    assert nbytes[0] == 2 * n_sym + 4 == packets.shape[1]
    assert np.array_equal(ref.decode(cum, packets, nbytes)[0], codes)
    # an exactly uniform table of 16 codes: zero logits give f = 4096 each, 4 bits a symbol, a byte every second symbol
    f, _, _ = ref.table_row(np.zeros(16, dtype=np.float32))       # r = 65520 / 16 = 4095, exact in any arithmetic
    assert np.all(f == 4096)
    for n_sym in (1, 2, 3, 8, 11):
        cum = np.broadcast_to(_cum_of(f), (1, n_sym, 1, 17))
        codes = (np.arange(n_sym) % 16).reshape(1, n_sym, 1)
        packets, nbytes, _ = ref.encode(cum, codes)
        assert nbytes[0] == 4 + (4 * n_sym) // 8
        assert np.array_equal(ref.decode(cum, packets, nbytes)[0], codes)


def test_mirror_rows_that_code_nothing_and_codes_outside_their_stage():
    rng = np.random.default_rng(4)
    logits = rng.standard_normal((3, 2 * 8, 2)).astype(np.float32)
    counts, stages = np.array([0, 2, 2]), np.array([2, 0, 2])
    cum, _, _ = ref.tables(logits, 2, (8, 5), counts, stages)
    assert not cum[0].any() and not cum[1].any() and np.all(cum[2, :, 1, 5:] == ref.M)
    codes = rng.integers(0, 5, (3, 2, 2))
    codes[2, 1, 1] = 5                                      # outside its stage of 5 codes: skipped, bit 0
    packets, nbytes, status = ref.encode(cum, codes, (8, 5), counts, stages)
    assert list(nbytes[:2]) == [0, 0] and not packets[:2].any() and list(status) == [0, 0, 1]
    got, _, st, _ = ref.decode(cum, packets, nbytes, (8, 5), counts, stages)
    assert np.all(got[:2] == -1) and list(st[:2]) == [0, 0]
    assert np.array_equal(got[2, 0], codes[2, 0]) and st[2] != 0      # one symbol short: the receiver notices
    # a truncated and a damaged packet: a nonzero status, codes inside their stages
    codes[2, 1, 1] = 4
    packets, nbytes, status = ref.encode(cum, codes, (8, 5), counts, stages)
    assert status[2] == 0
    for damage in ("short", "flip"):
        p, nb = packets.copy(), nbytes.copy()
        if damage == "short":
            nb[2] -= 1
        else:
            p[2, 1] ^= 0x5A
        got, _, st, _ = ref.decode(cum, p, nb, (8, 5), counts, stages)
        assert st[2] != 0 and got[2].min() >= 0 and np.all(got[2] < np.array([8, 5]))


def test_undecided_frequencies_on_the_gpu_inputs_are_rare():
    total = undecided = 0
    for name in ref.SHAPES:
        for sigma in ref.SIGMAS:
            c = ref.case(name, sigma)
            live = ref.live_mask(c)
            total += int(live.sum()) * c["k"]
            undecided += int((~c["decided"]).sum())
    print(f"undecided frequencies: {undecided} of {total}")
    assert total > 10000 and undecided <= 1e-4 * total


def test_symbols_constants_and_host_refusals():
    lib = _lib.load()
    for name in ("agx_codes_cum", "agx_codes_rans_encode", "agx_codes_rans_decode"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.agx_version() == 122
    assert (ops.RANS_SCALE_BITS, ops.RANS_M, ops.RANS_L) == (ref.SCALE_BITS, ref.M, ref.L) == (16, 65536, 1 << 23)
    assert ops.CODES_CUM_MAX_K == ref.MAX_K == 2048 and ops.RANS_MAX_SYMBOLS == ref.MAX_SYMBOLS
    # the library, before it looks at a pointer: the supported K, the stage count, the symbols of a row, a stage larger than K
    assert lib.agx_codes_cum(None, None, None, None, None, 1, 1, 1, 2049, 1, 0, None) == -5 and b"2048" in lib.agx_last_error()
    assert lib.agx_codes_cum(None, None, None, None, None, 1, 1, 65, 4, 1, 0, None) == -5
    assert lib.agx_codes_cum(None, None, None, None, None, 1, 2, 1, 4, 2, 1, None) == -1           # frames 1 .. 2 of a buffer of 2
    assert lib.agx_codes_cum(None, None, None, None, None, 1, 1, 1, 4, 1, 0, None) == -2           # NULL, last of all
    assert lib.agx_codes_rans_encode(None, None, None, None, None, None, None, None, 1, 1, 1, 2049, None) == -5
    assert lib.agx_codes_rans_encode(None, None, None, None, None, None, None, None, 1, 129, 64, 4, None) == -5
    assert b"8192" in lib.agx_last_error()
    assert lib.agx_codes_rans_encode(None, None, None, None, None, None, None, None, 1, 1, 65, 4, None) == -5
    assert lib.agx_codes_rans_decode(None, None, None, None, None, None, None, None, None, None, 1, 2, 0, 1, 65, 4, 8, None) == -5
    assert lib.agx_codes_rans_decode(None, None, None, None, None, None, None, None, None, None, 1, 2, 0, 1, 1, 2049, 8, None) == -5
    assert lib.agx_codes_rans_decode(None, None, None, None, None, None, None, None, None, None, 1, 2, 2, 1, 1, 4, 8, None) == -1
    assert lib.agx_codes_rans_decode(None, None, None, None, None, None, None, None, None, None, 1, 2, 1, 1, 1, 4, 8, None) == -2
    # the wrappers: dtype, shape and the limits are refused in their own words, not as "this is a CPU tensor"
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    with pytest.raises(_lib.AgxError, match="logits must be a torch.float32"):
        ops.codes_cum(torch.zeros(1, 8, 2, dtype=torch.float64), 2)
    with pytest.raises(_lib.AgxError, match=r"not \(B, Q K, n\)"):
        ops.codes_cum(torch.zeros(1, 9, 2, dtype=f32), 2)
    with pytest.raises(_lib.AgxError, match="CODES_CUM_MAX_K"):
        ops.codes_cum(torch.zeros(1, 2049, 1, dtype=f32), 1)
    with pytest.raises(_lib.AgxError, match="at most 64 stages"):
        ops.codes_cum(torch.zeros(1, 130, 1, dtype=f32), 65)
    with pytest.raises(_lib.AgxError, match="table buffer"):
        ops.codes_cum(torch.zeros(1, 8, 2, dtype=f32), 2, out=torch.zeros(1, 3, 2, 5, dtype=i32), frame0=2)
    with pytest.raises(_lib.AgxError, match="cum must be"):
        ops.codes_rans_encode(torch.zeros(1, 2, 2, 5, dtype=i64), torch.zeros(1, 2, 2, dtype=i64))
    with pytest.raises(_lib.AgxError, match="codes must be"):
        ops.codes_rans_encode(torch.zeros(1, 2, 2, 5, dtype=i32), torch.zeros(1, 3, 2, dtype=i64))
    with pytest.raises(_lib.AgxError, match="CODES_CUM_MAX_K"):
        ops.codes_rans_encode(torch.zeros(1, 1, 1, 2050, dtype=i32), torch.zeros(1, 1, 1, dtype=i64))
    with pytest.raises(_lib.AgxError, match="at most 64 stages"):
        ops.codes_rans_encode(torch.zeros(1, 1, 65, 3, dtype=i32), torch.zeros(1, 1, 65, dtype=i64))
    with pytest.raises(_lib.AgxError, match="RANS_MAX_SYMBOLS"):
        ops.codes_rans_encode(torch.zeros(1, 129, 64, 3, dtype=i32), torch.zeros(1, 129, 64, dtype=i64))
    cum, state, status, nb = torch.zeros(1, 2, 2, 5, dtype=i32), torch.zeros(1, 2, dtype=i64), torch.zeros(1, dtype=i64), torch.zeros(1, dtype=i64)
    with pytest.raises(_lib.AgxError, match="packets must be"):
        ops.codes_rans_decode(cum, torch.zeros(1, 12, dtype=i64), nb, state, status)
    with pytest.raises(_lib.AgxError, match="state must be"):
        ops.codes_rans_decode(cum, torch.zeros(1, 12, dtype=torch.uint8), nb, torch.zeros(1, 3, dtype=i64), status)
    with pytest.raises(_lib.AgxError, match="do not lie in a hop"):
        ops.codes_rans_decode(cum, torch.zeros(1, 12, dtype=torch.uint8), nb, state, status, i0=2, n=1)
    with pytest.raises(_lib.AgxError, match="MI355X only"):       # and with everything in order: there is no CPU fallback
        ops.codes_rans_decode(cum, torch.zeros(1, 12, dtype=torch.uint8), nb, state, status)
    from audio_generation_amd.entropy import PriorCoder
    from audio_generation_amd.prior import CodePrior
    prior = CodePrior(3, (16, 16, 5), 64, 2, 2, 32, 8, 32)
    with pytest.raises(_lib.AgxError, match="eval"):
        PriorCoder(prior.train())
    coder = PriorCoder(prior.eval())
    assert sum(p.numel() for p in coder.parameters()) == sum(p.numel() for p in prior.parameters())
    with pytest.raises(_lib.AgxError):
        coder.encode(None, torch.zeros(1, 2, 3, dtype=i64))
