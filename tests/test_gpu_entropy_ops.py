"""The entropy-coding ops on the GPU against the mirror of tests/entropy_ref.py: ``ops.codes_cum`` -- the exact
invariants of a table, every decided frequency, the cases that are exact in any arithmetic --, ``ops.codes_rans_encode`` byte for
byte on the DEVICE's tables, and ``ops.codes_rans_decode``: the round trip, one call against one call per frame, ``carry``, and
packets that were damaged on the way.

Shapes (tests/entropy_ref.py ``SHAPES``): B = 2, n = 3, Q = 3, K = 16 with sizes (16, 16, 5), counts [3, 1], stages [3, 2]; K =
2048 (every thread of the scan holds eight codes; a stage of 1500); K = 1, where a table is (0, M); Q = 64 stages of 2 codes with a
row that codes nothing.  Logits are N(0, sigma), sigma in {0.1, 1, 4}."""
import numpy as np
import pytest
import torch

from audio_generation_amd import ops
from tests import entropy_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(name, sigma) for name in ref.SHAPES for sigma in ref.SIGMAS]
_DEVICE = {}


def _t(a):
    return None if a is None else torch.from_numpy(np.asarray(a)).to(DEV)


def _device_case(name, sigma):
    """The case with the device's own tables and packets, computed once per (shape, sigma) and never modified."""
    key = (name, sigma)
    if key not in _DEVICE:
        c = dict(ref.case(name, sigma))
        c["d_counts"], c["d_stages"], c["d_codes"] = _t(c["counts"]), _t(c["stages"]), _t(c["codes"])
        c["d_cum"] = ops.codes_cum(_t(c["logits"]), c["n_q"], c["sizes"], c["d_counts"], c["d_stages"])
        c["d_packets"], c["d_nbytes"], c["d_status"] = ops.codes_rans_encode(c["d_cum"], c["d_codes"], c["sizes"], c["d_counts"], c["d_stages"])
        c["cum_dev"] = c["d_cum"].cpu().numpy().astype(np.int64)
        _DEVICE[key] = c
    return _DEVICE[key]


def _sizes(c):
    return [c["k"]] * c["n_q"] if c["sizes"] is None else list(c["sizes"])


def _decode(c, packets, nbytes, i0=0, n=None, state=None, status=None, carry=None):
    b = c["codes"].shape[0]
    state = torch.full((b, 2), -3, dtype=torch.int64, device=DEV) if state is None else state
    status = torch.full((b,), -3, dtype=torch.int64, device=DEV) if status is None else status
    codes = ops.codes_rans_decode(c["d_cum"], packets, nbytes, state, status, i0, n, c["sizes"], c["d_counts"], c["d_stages"], carry)
    return codes, state, status


@pytest.mark.parametrize("name,sigma", CASES)
def test_tables_exact_invariants_and_decided_frequencies(name, sigma):
    c = _device_case(name, sigma)
    cum, want, live, sizes = c["cum_dev"], c["cum"], ref.live_mask(c), _sizes(c)
    assert c["d_cum"].dtype == torch.int32 and cum.shape == want.shape
    assert not cum[~live].any()                                  # dead tables: exact 0
    compared = undecided = 0
    for q, size in enumerate(sizes):
        t, w, lv = cum[:, :, q][live[:, :, q]], want[:, :, q][live[:, :, q]], live[:, :, q]
        if not len(t):
            continue
        f, fw = np.diff(t[:, :size + 1], axis=1), np.diff(w[:, :size + 1], axis=1)
        assert np.all(t[:, 0] == 0) and f.min() >= 1 and np.all(t[:, size:] == ref.M)
        arg, dec = c["arg"][:, :, q][lv], c["decided"][:, :, q][lv][:, :size]
        others = np.ones_like(f, dtype=bool)
        others[np.arange(len(arg)), arg] = False
        assert np.array_equal(f[others & dec], fw[others & dec])
        assert np.abs(f - fw)[others & ~dec].max(initial=0) <= 1
        assert np.array_equal(f[~others], ref.M - np.where(others, f, 0).sum(axis=1))
        compared += int(others.sum())
        undecided += int((others & ~dec).sum())
    print(f"tables {name} sigma {sigma}: {undecided} undecided of {compared} compared")
    assert undecided <= 1e-4 * max(compared, 1)


def test_tables_exact_cases():
    b, n, n_q, k = 2, 2, 3, 16
    sizes = (16, 16, 5)
    zero = ops.codes_cum(torch.zeros(b, n_q * k, n, device=DEV), n_q, sizes).cpu().numpy().astype(np.int64)
    f = np.diff(zero, axis=-1)
    assert np.all(f[:, :, :2] == 4096)                           # r = 65520 / 16 = 4095 exactly
    assert np.all(f[:, :, 2, :5] == [13108, 13107, 13107, 13107, 13107]) and not f[:, :, 2, 5:].any()   # 65531 / 5 = 13106.2, the rest to code 0
    logits = torch.zeros(b, n_q * k, n)
    logits[:, 3] = 60.0
    logits[:, 16 + 9] = 60.0
    logits[:, 32 + 4] = 60.0
    f = np.diff(ops.codes_cum(logits.to(DEV), n_q, sizes).cpu().numpy().astype(np.int64), axis=-1)
    for q, (a, size) in enumerate(((3, 16), (9, 16), (4, 5))):
        want = np.ones(k, dtype=np.int64)
        want[a], want[size:] = ref.M - (size - 1), 0
        assert np.all(f[:, :, q] == want)
    # a table buffer: the call's frames land where they are sent and nothing else is touched
    buf = torch.full((b, 5, n_q, k + 1), -9, dtype=torch.int32, device=DEV)
    out = ops.codes_cum(logits.to(DEV), n_q, sizes, out=buf, frame0=2)
    assert out is buf and bool((buf[:, :2] == -9).all()) and bool((buf[:, 4:] == -9).all())
    assert torch.equal(buf[:, 2:4], ops.codes_cum(logits.to(DEV), n_q, sizes))


@pytest.mark.parametrize("name,sigma", CASES)
def test_encoder_bytes_equal_the_mirror_on_the_device_tables(name, sigma):
    c = _device_case(name, sigma)
    packets, nbytes, status = ref.encode(c["cum_dev"], c["codes"], c["sizes"], c["counts"], c["stages"])
    got_p, got_n = c["d_packets"].cpu().numpy(), c["d_nbytes"].cpu().numpy()
    b, n, n_q = c["codes"].shape
    assert got_p.shape == (b, 2 * n * n_q + 4) and np.array_equal(got_n, nbytes)
    assert np.array_equal(got_p, packets) and np.array_equal(c["d_status"].cpu().numpy(), status) and not status.any()
    for bi in range(b):
        assert not got_p[bi, got_n[bi]:].any()
    live = ref.live_mask(c)
    assert all((got_n[bi] == 0) == (not live[bi].any()) for bi in range(b))


def test_encoder_fills_the_row_when_every_frequency_is_one_and_skips_codes_outside_their_stage():
    b, n, n_q, k = 2, 3, 2, 16
    logits = torch.zeros(b, n_q * k, n)
    logits[:, 3] = 60.0
    logits[:, 16 + 9] = 60.0
    cum = ops.codes_cum(logits.to(DEV), n_q)
    codes = torch.full((b, n, n_q), 7, dtype=torch.int64)
    packets, nbytes, status = ops.codes_rans_encode(cum, codes.to(DEV))
    want_p, want_n, _ = ref.encode(cum.cpu().numpy().astype(np.int64), codes.numpy())
    assert nbytes.tolist() == [2 * n * n_q + 4] * b == [packets.shape[1]] * b and status.tolist() == [0, 0]
    assert np.array_equal(packets.cpu().numpy(), want_p) and np.array_equal(nbytes.cpu().numpy(), want_n)
    codes[1, 1, 0], codes[1, 2, 1] = 16, -1                      # outside [0, 16): skipped, bit 0 of the row's status
    packets, nbytes, status = ops.codes_rans_encode(cum, codes.to(DEV))
    want_p, want_n, want_s = ref.encode(cum.cpu().numpy().astype(np.int64), codes.numpy())
    assert status.tolist() == [0, 1] == want_s.tolist() and nbytes.tolist() == [16, 12] == want_n.tolist()
    assert np.array_equal(packets.cpu().numpy(), want_p)


def test_encoder_keeps_the_skipped_code_flag_over_rows_of_more_than_64_symbols():
    """n Q = 80: a lane of the gathering wave takes entries e and e + 64.  Row 0 has a bad code at entry 3 and valid ones at 67
    and beyond, and a second bad one at entry 70, another lane's last; row 1 has the one at entry 3 only; row 2 has none."""
    b, n, n_q, k = 3, 5, 16, 8
    rng = np.random.default_rng(80)
    logits = rng.standard_normal((b, n_q * k, n)).astype(np.float32)
    cum = ops.codes_cum(_t(logits), n_q)
    codes = rng.integers(0, k, (b, n, n_q))
    codes[0, 0, 3], codes[0, 4, 6], codes[1, 0, 3] = k, -1, k + 5           # entries 3, 4 * 16 + 6 = 70, 3
    packets, nbytes, status = ops.codes_rans_encode(cum, _t(codes))
    want_p, want_n, want_s = ref.encode(cum.cpu().numpy().astype(np.int64), codes)
    assert want_s.tolist() == [1, 1, 0] and status.tolist() == [1, 1, 0]
    assert np.array_equal(nbytes.cpu().numpy(), want_n) and np.array_equal(packets.cpu().numpy(), want_p)
    # the receiver of such a hop is told too: its packet is symbols short
    state, st = torch.zeros(b, 2, dtype=torch.int64, device=DEV), torch.zeros(b, dtype=torch.int64, device=DEV)
    back = ops.codes_rans_decode(cum, packets, nbytes, state, st)
    assert bool((st[:2] != 0).all()) and int(st[2]) == 0 and np.array_equal(back[2].cpu().numpy(), codes[2])


@pytest.mark.parametrize("name,sigma", CASES)
def test_decoder_round_trip_in_one_call_and_frame_by_frame(name, sigma):
    c = _device_case(name, sigma)
    b, n, n_q = c["codes"].shape
    live = ref.live_mask(c)
    want = np.where(live, c["codes"], -1)
    carry0 = torch.full((b, n_q), -7, dtype=torch.int64)
    carry = carry0.to(DEV)
    codes, state, status = _decode(c, c["d_packets"], c["d_nbytes"], carry=carry)
    assert np.array_equal(codes.cpu().numpy(), want)
    decoded = torch.from_numpy(live.any(axis=(1, 2))).to(DEV)
    assert bool((status[decoded] == 0).all())
    assert torch.equal(state[decoded], torch.stack([torch.full_like(c["d_nbytes"], ref.L), c["d_nbytes"]], dim=1)[decoded])
    m_codes, m_state, m_status, m_carry = ref.decode(c["cum_dev"], c["d_packets"].cpu().numpy(), c["d_nbytes"].cpu().numpy(), c["sizes"],
                                                     c["counts"], c["stages"], carry0.numpy())
    assert np.array_equal(m_codes, want) and np.array_equal(carry.cpu().numpy(), m_carry)
    for bi in range(b):                                          # carry as the sampler leaves it: the row's last frame, or untouched
        cb = ref._clamp(c["counts"], bi, n)
        assert np.array_equal(carry[bi].cpu().numpy(), want[bi, cb - 1] if cb else carry0[bi].numpy())
    # one call per frame: the same bits everywhere, states and statuses included (rows that decode nothing keep what they held)
    state2, status2 = torch.full_like(state, -3), torch.full_like(status, -3)
    carry2 = carry0.to(DEV)
    parts = [_decode(c, c["d_packets"], c["d_nbytes"], i, 1, state2, status2, carry2)[0] for i in range(n)]
    assert torch.equal(torch.cat(parts, dim=1), codes) and torch.equal(carry2, carry)
    assert torch.equal(state2, state) and torch.equal(status2, status)
    if n > 1:                                                    # and a split in two calls
        state3, status3 = torch.full_like(state, -3), torch.full_like(status, -3)
        carry3 = carry0.to(DEV)
        parts = [_decode(c, c["d_packets"], c["d_nbytes"], 0, 1, state3, status3, carry3)[0],
                 _decode(c, c["d_packets"], c["d_nbytes"], 1, n - 1, state3, status3, carry3)[0]]
        assert torch.equal(torch.cat(parts, dim=1), codes) and torch.equal(state3, state) and torch.equal(carry3, carry)


@pytest.mark.parametrize("name", ["base", "k2048"])
@pytest.mark.parametrize("damage", ["short", "flip", "empty", "wide"])
def test_damaged_packets_give_a_status_and_codes_inside_their_stages(name, damage):
    c = _device_case(name, 1.0)
    b, n, n_q = c["codes"].shape
    packets, nbytes = c["d_packets"].clone(), c["d_nbytes"].clone()
    if damage == "short":
        nbytes -= 1
    elif damage == "flip":
        packets[:, 1] ^= 0x5A                                    # a byte of the final state: inside every packet, however short
    elif damage == "empty":
        nbytes.zero_()
    else:
        nbytes += 1000                                           # behind the row: clamped, and not where the coder ended
    codes, state, status = _decode(c, packets, nbytes)
    m_codes, m_state, m_status, _ = ref.decode(c["cum_dev"], packets.cpu().numpy(), nbytes.cpu().numpy(), c["sizes"], c["counts"], c["stages"])
    assert np.array_equal(codes.cpu().numpy(), m_codes) and np.array_equal(status.cpu().numpy(), m_status)
    assert bool((status != 0).all())
    hi = torch.tensor(_sizes(c), device=DEV)
    assert int(codes.min()) >= -1 and bool((codes < hi).all())
    live = torch.from_numpy(ref.live_mask(c)).to(DEV)
    assert bool((codes[~live] == -1).all()) and bool((codes[live] >= 0).all())
