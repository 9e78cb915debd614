"""Memory contract (tests/guarded.py) of the entropy-coding ops: every output of ``ops.codes_cum``,
``ops.codes_rans_encode`` and ``ops.codes_rans_decode`` sits between guard bands and starts as poison; so do the inputs, and what
a kernel must not read IS the poison -- the logits of dead frames, dead stages and codes behind a stage's size, the codes and
tables of dead entries, the packet bytes behind ``nbytes``, the receiver's state before frame 0.  A read of any of it shows as a
changed result, a stray store as a damaged guard.  Each case runs under the plain fills and with its operands 4, 8 and 12 bytes
off alignment (the int64 operands round that down to 8: tests/guarded.py)."""
import numpy as np
import pytest
import torch

from audio_generation_amd import ops
from tests import entropy_ref as ref
from tests.guarded import PLACEMENT_RUNS, RUNS, Out, routed, run_contract

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCHEDULES = [pytest.param(RUNS, id="fills"), pytest.param(PLACEMENT_RUNS, id="placement")]


@pytest.fixture(scope="module")
def case():
    """The base shape of the op tests with its mirror tables, packets and decoded codes: computed once, never modified."""
    c = dict(ref.case("base", 1.0))
    c["packets"], c["nbytes"], c["status"] = ref.encode(c["cum"], c["codes"], c["sizes"], c["counts"], c["stages"])
    carry0 = np.full((2, 3), -7, dtype=np.int64)
    c["decoded"], c["state"], c["dstatus"], c["carry"] = ref.decode(c["cum"], c["packets"], c["nbytes"], c["sizes"], c["counts"], c["stages"],
                                                                     carry0)
    c["carry0"], c["live"] = carry0, ref.live_mask(c)
    assert (~c["decided"]).sum() == 0 and not c["dstatus"].any()
    return c


def _rows(arena, c):
    return arena.place(torch.from_numpy(c["counts"])), arena.place(torch.from_numpy(c["stages"]))


def _partly(arena, full: np.ndarray, keep: np.ndarray):
    """``full`` in the arena with everything outside ``keep`` left as the arena's poison."""
    host = torch.from_numpy(full)
    t = arena.empty(tuple(host.shape), dtype=host.dtype)
    mask = torch.from_numpy(np.broadcast_to(keep, full.shape).copy()).to(DEV)
    t[mask] = host.to(DEV)[mask]
    return t


@pytest.mark.parametrize("runs", SCHEDULES)
def test_codes_cum_memory_contract(case, runs):
    c = case
    b, n, n_q = c["codes"].shape
    k = c["k"]
    read = np.zeros((b, n_q, k, n), dtype=bool)                   # the logits of live entries, below the stage's size
    for q, size in enumerate(c["sizes"]):
        read[:, q, :size] = c["live"][:, :, q][:, None, :]
    read = read.reshape(b, n_q * k, n)

    def run(arena):
        ld = _partly(arena, c["logits"], read)
        counts, stages = _rows(arena, c)
        with routed(arena, ops):
            cum = ops.codes_cum(ld, n_q, c["sizes"], counts, stages)
        return [Out("cum", cum, torch.from_numpy(c["cum"]), exact=True), Out("counts", counts, torch.from_numpy(c["counts"]), exact=True),
                Out("stages", stages, torch.from_numpy(c["stages"]), exact=True)]
    assert run_contract(run, DEV, runs)["reproducible"]


@pytest.mark.parametrize("runs", SCHEDULES)
def test_codes_cum_into_a_table_buffer_touches_its_frames_only(case, runs):
    c = case
    b, n, n_q = c["codes"].shape
    want = np.full((b, n + 2, n_q, c["k"] + 1), -5, dtype=np.int32)
    want[:, 1:1 + n] = c["cum"]

    def run(arena):
        ld = arena.place(torch.from_numpy(c["logits"]))
        counts, stages = _rows(arena, c)
        buf = arena.place(torch.full((b, n + 2, n_q, c["k"] + 1), -5, dtype=torch.int32))
        ops.codes_cum(ld, n_q, c["sizes"], counts, stages, out=buf, frame0=1)
        return [Out("buffer", buf, torch.from_numpy(want), exact=True), Out("logits", ld, torch.from_numpy(c["logits"]), exact=True)]
    assert run_contract(run, DEV, runs)["reproducible"]


@pytest.mark.parametrize("runs", SCHEDULES)
def test_rans_encode_memory_contract(case, runs):
    c = case
    cum32 = c["cum"].astype(np.int32)

    def run(arena):
        cum = _partly(arena, cum32, c["live"][..., None])
        codes = _partly(arena, c["codes"], c["live"])
        counts, stages = _rows(arena, c)
        with routed(arena, ops):
            packets, nbytes, status = ops.codes_rans_encode(cum, codes, c["sizes"], counts, stages)
        return [Out("packets", packets, torch.from_numpy(c["packets"]), exact=True), Out("nbytes", nbytes, torch.from_numpy(c["nbytes"]), exact=True),
                Out("status", status, torch.from_numpy(c["status"]), exact=True), Out("counts", counts, torch.from_numpy(c["counts"]), exact=True)]
    assert run_contract(run, DEV, runs)["reproducible"]


@pytest.mark.parametrize("runs", SCHEDULES)
@pytest.mark.parametrize("split", [False, True])
def test_rans_decode_memory_contract(case, runs, split):
    c = case
    cum32 = c["cum"].astype(np.int32)
    b, n, n_q = c["codes"].shape
    sent = np.arange(c["packets"].shape[1])[None, :] < c["nbytes"][:, None]

    def run(arena):
        cum = _partly(arena, cum32, c["live"][..., None])
        packets = _partly(arena, c["packets"], sent)
        nbytes = arena.place(torch.from_numpy(c["nbytes"]))
        counts, stages = _rows(arena, c)
        carry = arena.place(torch.from_numpy(c["carry0"]))
        state, status = arena.empty((b, 2), dtype=torch.int64), arena.empty((b,), dtype=torch.int64)     # poison: frame 0 starts them
        with routed(arena, ops):
            if split:
                parts = [ops.codes_rans_decode(cum, packets, nbytes, state, status, i, 1, c["sizes"], counts, stages, carry) for i in range(n)]
            else:
                parts = [ops.codes_rans_decode(cum, packets, nbytes, state, status, 0, None, c["sizes"], counts, stages, carry)]
        outs = [Out(f"codes{i}", p, torch.from_numpy(c["decoded"][:, i:i + p.shape[1]]), exact=True) for i, p in enumerate(parts)]
        return outs + [Out("state", state, torch.from_numpy(c["state"]), exact=True), Out("status", status, torch.from_numpy(c["dstatus"]), exact=True),
                       Out("carry", carry, torch.from_numpy(c["carry"]), exact=True), Out("nbytes", nbytes, torch.from_numpy(c["nbytes"]), exact=True)]
    assert run_contract(run, DEV, runs)["reproducible"]


@pytest.mark.parametrize("runs", SCHEDULES)
@pytest.mark.parametrize("damage", ["short", "flip", "wide"])
def test_rans_decode_of_damaged_packets_writes_nothing_outside_its_outputs(case, runs, damage):
    """A packet one byte short, one with a flipped byte, and one whose ``nbytes`` points 1000 bytes behind the row: the outputs
    are the mirror's (codes inside their stages, a nonzero status), every guard band holds, and the bytes at or behind
    ``min(nbytes, P)`` are poison that is never read."""
    c = case
    cum32 = c["cum"].astype(np.int32)
    b, n, n_q = c["codes"].shape
    packets, nbytes = c["packets"].copy(), c["nbytes"].copy()
    if damage == "short":
        nbytes -= 1
    elif damage == "flip":
        packets[:, 1] ^= 0x5A
    else:
        nbytes += 1000
    want, state, status, carry = ref.decode(c["cum"], packets, nbytes, c["sizes"], c["counts"], c["stages"], c["carry0"])
    assert status.all() and want.min() >= -1 and np.all(want < np.array(c["sizes"]))
    readable = np.arange(packets.shape[1])[None, :] < nbytes[:, None]

    def run(arena):
        cum = _partly(arena, cum32, c["live"][..., None])
        pk = _partly(arena, packets, readable)
        nb = arena.place(torch.from_numpy(nbytes))
        counts, stages = _rows(arena, c)
        cr = arena.place(torch.from_numpy(c["carry0"]))
        st8, st = arena.empty((b, 2), dtype=torch.int64), arena.empty((b,), dtype=torch.int64)
        with routed(arena, ops):
            codes = ops.codes_rans_decode(cum, pk, nb, st8, st, 0, None, c["sizes"], counts, stages, cr)
        return [Out("codes", codes, torch.from_numpy(want), exact=True), Out("state", st8, torch.from_numpy(state), exact=True),
                Out("status", st, torch.from_numpy(status), exact=True), Out("carry", cr, torch.from_numpy(carry), exact=True),
                Out("nbytes", nb, torch.from_numpy(nbytes), exact=True)]
    assert run_contract(run, DEV, runs)["reproducible"]
