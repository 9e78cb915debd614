"""The guarded arena of tests/guarded.py is not vacuous: on CPU tensors, with fake ops written in this module (so that this
module's ``torch`` global is what ``routed`` swaps), every planted violation is reported with the right allocation and side,
and a correct op passes under all three fill patterns."""
import sys

import pytest
import torch

from audio_generation_amd import ops
from tests import guarded
from tests.guarded import Arena, Out, routed, run_contract

ME = sys.modules[__name__]


def _neighbour(t, where):
    """One element just outside ``t``'s payload: -1 = before, +1 = after (same storage, so it lands in the guard band)."""
    off = t.storage_offset() - 1 if where < 0 else t.storage_offset() + t.numel()
    return t.as_strided((1,), (1,), off)


def fake_scale(x, bug=None):
    """y = 2 x through a workspace, like a wrapper of ops.py: ``torch.empty`` output and workspace, then the 'kernel'."""
    y = torch.empty_like(x)
    ws = torch.empty(x.numel(), dtype=torch.float32, device=x.device)
    if bug == "uncleared_workspace":
        ws += x.reshape(-1)                      # accumulates into a workspace it assumes is clear
    else:
        ws.copy_(x.reshape(-1))
    y.copy_((2.0 * ws).reshape(x.shape))
    if bug == "write_before_output":
        _neighbour(y, -1).fill_(1.0)
    elif bug == "write_after_output":
        _neighbour(y, +1).fill_(1.0)
    elif bug == "write_past_workspace":
        _neighbour(ws, +1).fill_(1.0)
    elif bug == "unwritten_tail":
        y.reshape(-1)[-1:] = torch.empty(1, dtype=torch.float32, device=x.device)      # what fresh memory holds
    elif bug == "masked_overread":
        y.reshape(-1)[-1:] += 0.0 * _neighbour(x, +1)                                  # "garbage x 0"
    elif bug == "overread":
        y.reshape(-1)[-1:] += _neighbour(x, +1)
    return y


def _case(bug):
    x_cpu = torch.randn(3, 5, 7, generator=torch.Generator().manual_seed(1))

    def case(arena):
        x = arena.place(x_cpu)
        with routed(arena, ME):
            y = fake_scale(x, bug)
        return [Out("y", y, 2.0 * x_cpu.double(), 1e-6)]
    return case


def test_correct_fake_op_passes_under_all_three_patterns():
    report = run_contract(_case(None), "cpu")
    assert report == {"reproducible": True, "irreproducible": {}}
    for fill in guarded.PATTERNS:
        arena = Arena("cpu", fill)
        _case(None)(arena)
        arena.check()
        assert len(arena.allocs) == 3            # the placed input, the output, the workspace


@pytest.mark.parametrize("bug,order,side,offset", [
    ("write_before_output", 1, "before", -4), ("write_after_output", 1, "after", 3 * 5 * 7 * 4),
    ("write_past_workspace", 2, "after", 3 * 5 * 7 * 4)])
def test_stray_write_is_reported_with_allocation_and_side(bug, order, side, offset):
    arena = Arena("cpu", 0x7F)
    _case(bug)(arena)
    found = arena.violations()
    assert len(found) == 1
    shape = "(3, 5, 7)" if order == 1 else "(105,)"
    assert f"allocation #{order} (empty, shape {shape}, torch.float32, 420 bytes)" in found[0]
    assert f"guard {side} the payload" in found[0] and f"first at payload offset {offset}," in found[0]
    assert f"last at {offset + 3} " in found[0]
    with pytest.raises(AssertionError, match=f"allocation #{order} .*guard {side}"):
        arena.check()
    with pytest.raises(AssertionError, match=f"allocation #{order} .*guard {side}"):
        run_contract(_case(bug), "cpu")


def test_stray_write_of_the_fill_value_itself_is_caught_by_another_pattern():
    """1.0f is 00 00 80 3F: under fill 0x00 only two of its four bytes show, and a stray zero would not show at all -- three
    patterns, not one."""
    arena = Arena("cpu", 0x00)
    _case("write_after_output")(arena)
    assert "2 bytes" in arena.violations()[0]


def test_unwritten_output_element_is_reported():
    with pytest.raises(AssertionError) as e:
        run_contract(_case("unwritten_tail"), "cpu")
    msg = str(e.value)
    assert "run 0 (fill 0x00): y is" in msg                    # 0 is not the reference value
    assert "run 2 (fill 0xFF): y holds 1 NaN/Inf, first at flat index 104" in msg
    assert "run 3 (fill 0x7F): y differs bitwise from run 0" in msg


def test_uncleared_workspace_is_reported():
    with pytest.raises(AssertionError) as e:
        run_contract(_case("uncleared_workspace"), "cpu")
    msg = str(e.value)
    assert "fill 0x00" not in msg.replace("run 0 (fill 0x00)", "")    # clean memory hides it: the suite's situation today
    assert "run 2 (fill 0xFF): y holds 105 NaN/Inf" in msg
    assert "run 3 (fill 0x7F): y" in msg


@pytest.mark.parametrize("bug", ["masked_overread", "overread"])
def test_read_past_an_input_is_reported(bug):
    with pytest.raises(AssertionError) as e:
        run_contract(_case(bug), "cpu")
    msg = str(e.value)
    assert "run 2 (fill 0xFF): y holds 1 NaN/Inf, first at flat index 104" in msg
    assert ("run 3 (fill 0x7F)" in msg) == (bug == "overread")       # finite garbage x 0 is 0: only NaN shows the masked read


def test_irreproducible_op_falls_back_to_the_reference_check():
    calls = []

    def case(arena, poisoned_steady=False):
        calls.append(arena.fill)
        y = arena.place(torch.full((4,), 1.0 + 1e-7 * len(calls)))
        z = arena.place(torch.full((4,), 2.0 + (1e-6 if poisoned_steady and arena.fill else 0.0)))
        return [Out("y", y, torch.ones(4, dtype=torch.float64), 1e-5), Out("z", z, torch.full((4,), 2.0), 1e-5)]
    report = run_contract(case, "cpu")
    assert report["reproducible"] is False and list(report["irreproducible"]) == ["y"]
    assert 0.0 < report["irreproducible"]["y"] < 1e-6
    assert calls == [0x00, 0x00, 0xFF, 0x7F]
    # per buffer: y's jitter does not excuse z, which is steady on clean memory and moves with the poison
    with pytest.raises(AssertionError, match="run 2 .*: z differs bitwise from run 0") as e:
        run_contract(lambda arena: case(arena, True), "cpu")
    assert ": y differs" not in str(e.value)


def test_a_buffer_that_changes_size_between_runs_is_reported():
    def case(arena):
        return [Out("y", arena.place(torch.ones(4 if arena.fill == 0 else 5)), torch.ones(4 if arena.fill == 0 else 5), 1e-6)]
    with pytest.raises(AssertionError, match="run 2 .*: y has 20 bytes, run 0 had 16"):
        run_contract(case, "cpu")


def test_out_needs_a_tolerance_or_exact():
    t = torch.ones(2)
    Out("a", t, t, exact=True), Out("b", t, t, 1e-6)
    for bad in (dict(), dict(tol=0.0), dict(tol=1e-6, exact=True)):
        with pytest.raises(AssertionError):
            Out("c", t, t, **bad)


@pytest.mark.parametrize("dtype", guarded.DTYPES)
@pytest.mark.parametrize("shape", [(), (1,), (3,), (7, 1, 13), (129, 5), (0,), (70001,)])
def test_payload_size_is_exact_and_payload_is_512_aligned(dtype, shape):
    for fill in guarded.PATTERNS:
        arena = Arena("cpu", fill)
        t = arena.empty(shape, dtype)
        a = arena.allocs[-1]
        assert t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()
        assert a.nbytes == t.numel() * t.element_size()
        if t.numel():                                          # an empty tensor has no address, here as in production
            assert t.data_ptr() % 512 == 0 and t.data_ptr() == a.raw.data_ptr() + a.lead
        before, after = a.lead, a.raw.numel() - a.lead - a.nbytes
        need = max(64 * 1024, -(-a.nbytes // 512) * 512)
        assert before >= need and after >= need
        assert bool((a.raw == fill).all())                     # payload poisoned as well as the guards
        src = torch.arange(t.numel()).reshape(shape).to(dtype)
        p = arena.place(src)
        assert torch.equal(p, src) and p.data_ptr() % 512 == 0
        arena.check()
        if t.numel():
            t.fill_(1)                                         # the whole payload is writable without touching a guard
            arena.check()


def test_dtype_list_is_the_one_need_gpu_accepts():
    """``_need_gpu`` refuses every dtype outside ``ops._DTYPES``."""
    assert guarded.DTYPES is ops._DTYPES and len(set(guarded.DTYPES)) == 5
    assert ops._DEVICE_CACHES == (ops._STFT_IMAGES,)


def test_proxy_forwards_everything_else_and_restores_the_module():
    real = ops.torch
    assert real is torch
    ops._STFT_IMAGES["stale"] = object()
    arena = Arena("cpu", 0xFF)
    with routed(arena, ops):
        assert ops.torch is not torch
        assert not ops._STFT_IMAGES                            # device caches are cleared on entry
        assert ops.torch.zeros is torch.zeros and ops.torch.float32 is torch.float32 and ops.torch.Tensor is torch.Tensor
        a = ops.torch.empty(3, 4, dtype=torch.int64, device="cpu")
        b = ops.torch.empty((2, 5), device="cpu")
        c = ops.torch.empty_like(a)
        d = ops.torch.empty((), dtype=torch.float32)
        e = ops.torch.empty(torch.Size([2, 2]), dtype=torch.bfloat16)
        assert [tuple(t.shape) for t in (a, b, c, d, e)] == [(3, 4), (2, 5), (3, 4), (), (2, 2)]
        assert [t.dtype for t in (a, b, c, d, e)] == [torch.int64, torch.float32, torch.int64, torch.float32, torch.bfloat16]
        assert bool((a == -1).all()) and bool(torch.isnan(b).all())
        assert len(arena.allocs) == 5
        z = ops.torch.zeros(4)                                 # passes through untouched
        assert len(arena.allocs) == 5 and bool((z == 0).all())
        with pytest.raises(AssertionError, match="routed allocation on 'cuda'"):
            ops.torch.empty(1, device="cuda")
    assert ops.torch is real
    assert torch.empty is real.empty                           # torch itself was never patched


def test_proxy_restores_the_module_when_the_body_raises():
    with pytest.raises(RuntimeError, match="boom"):
        with routed(Arena("cpu", 0x00), ops):
            assert ops.torch is not torch
            raise RuntimeError("boom")
    assert ops.torch is torch


# ---------------------------------------------------------------------- skewed placement
def fake_accumulate(acc, x, bug=None):
    """acc += x in place on a caller's buffer, like ``rvq_dequantize(out=, accumulate=True)``.  ``round_down``: the store
    address is the 16-byte boundary at or below ``acc`` (a float4 store through a pointer the kernel took for aligned);
    ``order``: the checksum it returns beside peels a head off the sum when ``x`` does not start on a 16-byte boundary."""
    back = (acc.data_ptr() % 16) // acc.element_size() if bug == "round_down" else 0
    acc.as_strided(acc.shape, acc.stride(), acc.storage_offset() - back).copy_(acc + x)
    total = torch.empty(1, dtype=torch.float32, device=x.device)
    flat = x.reshape(-1)
    if bug == "order" and x.data_ptr() % 16 != 0:
        total.copy_(flat[1:].sum() + flat[0])
    else:
        total.copy_(flat.sum())
    return acc, total


def _placed_case(bug=None):
    gen = torch.Generator().manual_seed(2)
    acc_cpu, x_cpu = torch.randn(5, 8, generator=gen), torch.randn(5, 8, generator=gen)
    want_total = x_cpu.double().sum().reshape(1)

    def case(arena):
        acc, x = arena.place(acc_cpu), arena.place(x_cpu)
        with routed(arena, ME):
            got, total = fake_accumulate(acc, x, bug)
        return [Out("acc", got, acc_cpu.double() + x_cpu.double(), 1e-6), Out("total", total, want_total, 1e-4)]
    return case


def _rounded(skew, dtype):
    size = torch.empty((), dtype=dtype).element_size()
    return skew // size * size


@pytest.mark.parametrize("dtype", guarded.DTYPES)
@pytest.mark.parametrize("skew", [0, 4, 8, 12])
@pytest.mark.parametrize("shape", [(), (3,), (7, 1, 13), (0,), (70001,)])
def test_placed_payload_starts_at_the_rounded_skew_and_is_exact(dtype, skew, shape):
    arena = Arena("cpu", 0x7F, skew)
    numel = 1
    for n in shape:
        numel *= n
    src = torch.arange(numel).reshape(shape).to(dtype)
    p = arena.place(src)
    a = arena.allocs[-1]
    want = _rounded(skew, dtype)
    assert want == {1: skew, 2: skew, 4: skew, 8: skew // 8 * 8}[p.element_size()]
    assert (a.skew, a.asked, a.what) == (want, skew, "place")
    assert p.dtype == dtype and tuple(p.shape) == shape and p.is_contiguous() and torch.equal(p, src)
    assert a.nbytes == p.numel() * p.element_size()
    if p.numel():
        assert p.data_ptr() % 512 == want and p.data_ptr() == a.raw.data_ptr() + a.lead
    need = max(64 * 1024, -(-a.nbytes // 512) * 512)
    assert a.lead >= need and a.raw.numel() - a.lead - a.nbytes >= need
    arena.check()
    if p.numel():
        p.fill_(1)                                             # the whole payload is writable without touching a guard
        arena.check()
        a.raw[a.lead - 1] = 0                                  # the guard before ends at the payload's first byte ...
        a.raw[a.lead + a.nbytes] = 0                           # ... and the guard after begins at its last
        found = arena.violations()
        assert len(found) == 2 and "first at payload offset -1," in found[0] and f"first at payload offset {a.nbytes}," in found[1]


def test_skews_cycle_in_the_order_of_place_calls_and_empty_is_unskewed():
    arena = Arena("cpu", 0x00, (4, 8, 12, 0))
    x = torch.ones(6)
    got = []
    for n in range(6):
        if n == 2:
            e = arena.empty((6,), torch.float32)               # does not move the cycle
            assert e.data_ptr() % 512 == 0 and (arena.allocs[-1].skew, arena.allocs[-1].asked) == (0, 0)
        got.append(arena.place(x).data_ptr() % 512)
    assert got == [4, 8, 12, 0, 4, 8]
    assert [a.skew for a in arena.allocs if a.what == "place"] == got
    idx = arena.place(torch.ones(3, dtype=torch.int64))        # call 7 of the cycle: 12 bytes, 8 for an 8-byte type
    assert idx.data_ptr() % 512 == 8 and (arena.allocs[-1].skew, arena.allocs[-1].asked) == (8, 12)
    whole = arena.place(x, skew=0)                             # the override takes its turn in the cycle
    assert whole.data_ptr() % 512 == 0 and arena.place(x).data_ptr() % 512 == 4
    for skew in (4, 8, 12):
        with routed(Arena("cpu", 0xFF, skew), ME) as a:
            assert torch.empty(5).data_ptr() % 512 == 0 and torch.empty_like(x).data_ptr() % 512 == 0
            assert a.place(x).data_ptr() % 512 == skew


def test_store_rounded_down_to_16_bytes_damages_the_guard_before_the_payload():
    for skew, back in ((0, 0), (4, 4), (8, 8), (12, 12)):
        arena = Arena("cpu", 0x7F, skew)
        _placed_case("round_down")(arena)
        found = arena.violations()
        if skew == 0:
            assert not found
            continue
        assert len(found) == 1
        assert f"allocation #0 (place, shape (5, 8), torch.float32, 160 bytes, {skew} bytes off alignment)" in found[0]
        assert "guard before the payload" in found[0] and f"{back} bytes, first at payload offset {-back}, last at -1 " in found[0]


def test_placement_runs_catch_the_rounded_store_and_the_fill_runs_do_not():
    """The new schedule, not the old one, carries the check."""
    assert guarded.PLACEMENT_RUNS == ((0x00, 0), (0xFF, 4), (0x7F, 8), (0xFF, 12), (0x7F, (4, 8, 12, 0)))
    assert run_contract(_placed_case("round_down"), "cpu") == {"reproducible": True, "irreproducible": {}}
    with pytest.raises(AssertionError) as e:
        run_contract(_placed_case("round_down"), "cpu", guarded.PLACEMENT_RUNS)
    msg = str(e.value)
    assert "\n  run 0 (" not in msg                             # the aligned run itself is clean
    for n, fill, skew in ((1, "FF", 4), (2, "7F", 8), (3, "FF", 12), (4, "7F", "(4, 8, 12, 0)")):
        assert f"run {n} (fill 0x{fill}, skew {skew}): allocation #0 (place, " in msg and f"run {n} (fill 0x{fill}, skew {skew}): acc " in msg
    assert "guard before the payload damaged, 4 bytes, first at payload offset -4, last at -1 (fill 0xFF)" in msg
    assert "guard after" not in msg


def test_alignment_dependent_result_fails_invariance_under_placement_runs():
    calls = []

    def case(arena):
        outs = _placed_case("order")(arena)
        calls.append((arena.fill, arena.skews, float(outs[1].got)))
        return outs
    assert run_contract(case, "cpu") == {"reproducible": True, "irreproducible": {}}          # aligned operands: nothing to see
    del calls[:]
    with pytest.raises(AssertionError) as e:
        run_contract(case, "cpu", guarded.PLACEMENT_RUNS)
    assert [c[:2] for c in calls] == [(0x00, (0,)), (0xFF, (4,)), (0x7F, (8,)), (0xFF, (12,)), (0x7F, (4, 8, 12, 0))]
    assert calls[1][2] != calls[0][2] and abs(calls[1][2] - calls[0][2]) < 1e-4               # the premise: other bits, in tolerance
    msg = str(e.value)
    for n in (1, 2, 3, 4):                                    # in run 4 x is the second placement: 8 bytes off
        assert f"run {n} " in msg
    assert msg.count("total differs bitwise from run 0 (fill 0x00, skew 0)") == 4 and "where its operands start" in msg
    assert ": acc " not in msg and "guard" not in msg and "tolerance" not in msg
    # a buffer the caller names keeps the reference check only, and the report says what was seen
    report = run_contract(case, "cpu", guarded.PLACEMENT_RUNS, irreproducible=("total",))
    assert report["reproducible"] is False and list(report["irreproducible"]) == ["total"] and 0.0 < report["irreproducible"]["total"] < 1e-4
    with pytest.raises(AssertionError, match="acc differs bitwise"):          # ... and excuses no other buffer
        run_contract(_placed_case("round_down"), "cpu", guarded.PLACEMENT_RUNS, irreproducible=("total",))


def test_placement_runs_have_no_probe_and_fill_runs_keep_theirs():
    """Under RUNS a difference between the two 0x00 runs is jitter; under PLACEMENT_RUNS the same op is a failure in every run."""
    def case(arena, calls=[]):
        calls.append(1)
        return [Out("y", arena.place(torch.full((4,), 1.0 + 1e-7 * len(calls))), torch.ones(4, dtype=torch.float64), 1e-4)]
    assert list(run_contract(case, "cpu")["irreproducible"]) == ["y"]
    with pytest.raises(AssertionError) as e:
        run_contract(case, "cpu", guarded.PLACEMENT_RUNS)
    assert str(e.value).count("y differs bitwise from run 0") == 4
    assert run_contract(_placed_case(None), "cpu", guarded.PLACEMENT_RUNS) == {"reproducible": True, "irreproducible": {}}
    with pytest.raises(AssertionError, match="finds its irreproducible buffers itself"):
        run_contract(_placed_case(None), "cpu", guarded.RUNS, irreproducible=("acc",))
    assert run_contract(_placed_case(None), "cpu", ((0x00, 0), (0x00, 0), (0xFF, 0), (0x7F, 0))) == {"reproducible": True, "irreproducible": {}}
