"""A guarded, poisoned arena for memory-contract tests of the C-ABI wrappers.

The value tests of this suite cannot see what a kernel does to memory that is not its result, or what it takes from memory
that is not its input: the caching allocator rounds every block up, fresh device memory is mostly zeros, and an over-read
picks up a neighbour's finite values.  This module takes those three comforts away:

* ``Arena(device, fill_byte, skew=0)`` hands out tensors whose payload is exactly ``numel * itemsize`` bytes and sits between
  two guard bands of at least 64 KiB.  Payload and guards are filled with ``fill_byte``; ``check()`` finds every guard byte
  that changed.  ``empty`` stays on the 512-byte boundary: what a wrapper allocates itself (outputs, workspaces, packed
  images) is what ``torch.empty`` gives it in production; only caller-supplied operands are skewed.  ``place`` starts its
  payload ``skew`` bytes past such a boundary (a byte count, or a sequence of them cycled once per ``place`` call), rounded
  down to the item size: a view ``wave[s:s + L]``, a batch slice, a parameter carved out of a flat buffer.  The guard before
  the payload ends at the payload's first byte, so a store rounded down to a 16-byte boundary damages it.
* ``routed(arena, module, ...)`` sends the ``torch.empty`` / ``torch.empty_like`` calls made inside the given modules
  (``audio_generation_amd.ops``) through the arena, by swapping the module's ``torch`` global for a thin proxy.
* ``run_contract(case, device)`` runs a case under the fill patterns 0x00, 0x00, 0xFF, 0x7F and asserts guards, reference
  and invariance (see its docstring); under ``PLACEMENT_RUNS`` the runs also differ in where the operands start, and every
  output must keep the bits of the aligned run.

Device-agnostic: everything works with ``device="cpu"`` (tests/test_guarded_cpu.py proves the harness on fake ops).
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Union

import torch

from audio_generation_amd.ops import _DTYPES

ALIGN = 512                  # what the caching allocator gives every tensor it allocates
GUARD_MIN = 64 * 1024
PATTERNS = (0x00, 0xFF, 0x7F)    # today's clean memory; NaN / -1 as an index; a huge finite value in every float type
RUNS = (0x00, 0x00, 0xFF, 0x7F)  # the first two establish bitwise reproducibility
# (fill, skew) runs: run 0 is the aligned one; 4, 8, 12 bytes off; the last gives neighbouring operands unequal alignment
PLACEMENT_RUNS = ((0x00, 0), (0xFF, 4), (0x7F, 8), (0xFF, 12), (0x7F, (4, 8, 12, 0)))
DTYPES = _DTYPES                 # every dtype _need_gpu lets through


def _round_up(n: int, m: int) -> int:
    return -(-n // m) * m


def _shape(shape) -> tuple:
    if isinstance(shape, (int,)):
        return (int(shape),)
    return tuple(int(s) for s in shape)


@dataclass
class _Alloc:
    order: int
    what: str           # "empty" or "place"
    shape: tuple
    dtype: torch.dtype
    raw: torch.Tensor   # uint8: [guard before | payload | guard after]
    lead: int           # bytes before the payload
    nbytes: int         # payload bytes
    skew: int = 0       # bytes the payload starts past a 512-byte boundary: ``asked`` rounded down to the item size
    asked: int = 0      # the skew of the ``place`` call

    def describe(self) -> str:
        at = f", {self.skew} bytes off alignment" if self.skew else ""
        return f"allocation #{self.order} ({self.what}, shape {self.shape}, {self.dtype}, {self.nbytes} bytes{at})"


class Arena:
    def __init__(self, device, fill_byte: int, skew: Union[int, Sequence[int]] = 0):
        self.device = torch.device(device)
        self.fill = int(fill_byte)
        assert 0 <= self.fill <= 255
        self.skews = (int(skew),) if isinstance(skew, int) else tuple(int(s) for s in skew)
        assert self.skews and all(0 <= s < ALIGN for s in self.skews), self.skews
        self.placed = 0              # ``place`` calls so far: the position in the skew cycle
        self.allocs: List[_Alloc] = []

    # ------------------------------------------------------------------ allocation
    def _allocate(self, shape, dtype, what: str, asked: int = 0) -> torch.Tensor:
        shape = _shape(shape)
        itemsize = torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * itemsize
        guard = max(GUARD_MIN, _round_up(nbytes, ALIGN))
        skew = asked // itemsize * itemsize
        # 2 * ALIGN spare bytes: the base pointer of a CPU tensor is only 64-byte aligned, and the skew is below ALIGN; the
        # spare bytes join the guards
        raw = torch.empty(guard + nbytes + guard + 2 * ALIGN, dtype=torch.uint8, device=self.device)
        raw.fill_(self.fill)
        lead = guard + (-(raw.data_ptr() + guard)) % ALIGN + skew
        assert lead % itemsize == 0 and (raw.data_ptr() + lead) % ALIGN == skew
        assert lead >= guard and raw.numel() - lead - nbytes >= guard
        self.allocs.append(_Alloc(len(self.allocs), what, shape, dtype, raw, lead, nbytes, skew, asked))
        return raw[lead:lead + nbytes].view(dtype).reshape(shape)

    def empty(self, shape, dtype=torch.float32) -> torch.Tensor:
        """A contiguous tensor of exactly ``numel * itemsize`` poisoned bytes between two poisoned guard bands."""
        return self._allocate(shape, dtype, "empty")

    def place(self, cpu_tensor: torch.Tensor, skew: Optional[int] = None) -> torch.Tensor:
        """A copy of the tensor in a payload of its shape and dtype (inputs, in/out buffers), this call's skew of the arena's
        cycle past a 512-byte boundary.  ``skew`` overrides the cycle for one call: ``skew=0`` is for what production always
        allocates whole, and the call says why."""
        asked = self.skews[self.placed % len(self.skews)] if skew is None else int(skew)
        self.placed += 1
        out = self._allocate(cpu_tensor.shape, cpu_tensor.dtype, "place", asked)
        out.copy_(cpu_tensor)
        return out

    # ------------------------------------------------------------------ guards
    def violations(self) -> List[str]:
        found = []
        for a in self.allocs:
            for side, band, base in (("before", a.raw[:a.lead], -a.lead), ("after", a.raw[a.lead + a.nbytes:], a.nbytes)):
                bad = band != self.fill            # on the device
                if bool(bad.any()):
                    at = bad.nonzero().flatten()
                    first, last = int(at[0]) + base, int(at[-1]) + base
                    found.append(f"{a.describe()}: guard {side} the payload damaged, {int(at.numel())} bytes, first at payload "
                                 f"offset {first}, last at {last} (fill 0x{self.fill:02X})")
        return found

    def check(self) -> None:
        """Every guard byte of every allocation still equals the fill byte."""
        found = self.violations()
        assert not found, "guard bands damaged:\n  " + "\n  ".join(found)


# ---------------------------------------------------------------------- routing a module's allocations
class _TorchProxy:
    """Stands in for a module's ``torch`` global: everything is the real torch's except ``empty`` and ``empty_like``."""

    def __init__(self, arena: Arena):
        self.__dict__["_arena"] = arena

    def __getattr__(self, name):
        return getattr(torch, name)

    def _check_device(self, device):
        if device is not None and torch.device(device).type != self._arena.device.type:
            raise AssertionError(f"routed allocation on '{device}', arena is on '{self._arena.device}'")

    def empty(self, *size, dtype=None, device=None, **kwargs):
        assert not kwargs, f"routed torch.empty: unexpected arguments {sorted(kwargs)}"
        self._check_device(device)
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        return self._arena.empty(size, torch.float32 if dtype is None else dtype)

    def empty_like(self, t, dtype=None, device=None, **kwargs):
        assert not kwargs, f"routed torch.empty_like: unexpected arguments {sorted(kwargs)}"
        self._check_device(t.device if device is None else device)
        return self._arena.empty(t.shape, t.dtype if dtype is None else dtype)


def _device_caches(module):
    """The caches a module declares in ``_DEVICE_CACHES`` (dicts that keep device buffers across calls, such as
    ``ops._STFT_IMAGES``): cleared on entry so that the pack kernels behind them run under every fill pattern."""
    return tuple(getattr(module, "_DEVICE_CACHES", ()))


@contextlib.contextmanager
def routed(arena: Arena, *modules):
    """Route ``torch.empty`` / ``torch.empty_like`` inside ``modules`` through ``arena`` for the duration."""
    saved = [(m, m.torch) for m in modules]
    proxy = _TorchProxy(arena)
    for m in modules:
        for cache in _device_caches(m):
            cache.clear()
    try:
        for m in modules:
            m.torch = proxy
        yield arena
    finally:
        for m, real in saved:
            m.torch = real
        for m in modules:              # what the body cached lives in this arena: do not leak it into later callers
            for cache in _device_caches(m):
                cache.clear()


# ---------------------------------------------------------------------- the contract
@dataclass
class Out:
    """One checked buffer of a case: an output, or an in/out buffer the case initialised.  Either ``tol`` (absolute, against
    ``want`` in float64) or ``exact=True`` (equality: indices, packed codes, gathers) must be given."""
    name: str
    got: torch.Tensor
    want: torch.Tensor
    tol: Optional[float] = None
    exact: bool = False

    def __post_init__(self):
        assert (self.tol is None) == self.exact, f"{self.name}: give a tolerance or exact=True, not both and not neither"
        assert self.exact or self.tol > 0.0, f"{self.name}: a tolerance of {self.tol} -- say exact=True"


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().cpu().reshape(-1).view(torch.uint8)


def _check_reference(outs: Sequence[Out], run: str, problems: List[str]) -> None:
    for o in outs:
        got = o.got.detach().cpu()
        want = torch.as_tensor(o.want).detach().cpu()
        if tuple(got.shape) != tuple(want.shape):
            problems.append(f"{run}: {o.name} has shape {tuple(got.shape)}, reference {tuple(want.shape)}")
            continue
        if got.is_floating_point():
            bad = ~torch.isfinite(got.float() if got.dtype == torch.bfloat16 else got)
            if bool(bad.any()):
                at = bad.reshape(-1).nonzero().flatten()
                problems.append(f"{run}: {o.name} holds {int(at.numel())} NaN/Inf, first at flat index {int(at[0])}, last at "
                                f"{int(at[-1])}")
                continue
        if got.numel() == 0:
            continue
        if o.exact:
            if not torch.equal(got, want.to(got.dtype)):
                n = int((got != want.to(got.dtype)).sum())
                problems.append(f"{run}: {o.name} is not equal to the reference ({n} of {got.numel()} elements differ)")
        else:
            err = float((got.double() - want.double()).abs().max())
            if not err < o.tol:
                problems.append(f"{run}: {o.name} is {err:.3e} from the reference (tolerance {o.tol:.3e})")


def _is_placement(runs) -> bool:
    return any(not isinstance(r, int) for r in runs)


def run_contract(case: Callable[[Arena], Sequence[Out]], device, runs: Sequence = RUNS,
                 irreproducible: Sequence[str] = ()) -> dict:
    """Run ``case(arena)`` once per fill pattern of ``runs`` and assert the memory contract:

    1. guards: ``arena.check()`` passes after every run;
    2. reference: every checked buffer is free of NaN/Inf and within its tolerance of its float64 reference, in every run;
    3. invariance: the checked buffers of the poisoned runs are bitwise those of the first 0x00 run.  The two 0x00 runs show
       whether each buffer is bitwise reproducible at all; for one that is not, invariance falls back to (2) alone -- for that
       buffer only -- and the returned report names it with the largest difference seen.  A caller must look at the report: an
       op that is not reproducible belongs on an explicit list, not in silence.

    A case builds its inputs on the CPU from a seeded generator, ``place``s them, calls the wrapper under ``routed`` and returns
    the ``Out`` list.  Raises ``AssertionError`` naming every violation; returns {"reproducible": bool, "irreproducible": {buffer
    name: largest difference between the two clean runs}}.

    A schedule with ``(fill, skew)`` runs (``PLACEMENT_RUNS``) also moves the placed operands off alignment, and has no probe:
    every bitwise difference from run 0 is a problem, whatever the fill, except in the buffers the caller names in
    ``irreproducible`` -- for those only (1) and (2) apply, and the report gives the largest difference seen.  A schedule of
    plain fills takes no ``irreproducible``: it finds such buffers itself.
    """
    problems: List[str] = []
    base = None
    placement = _is_placement(runs)
    assert placement or not irreproducible, "a schedule of plain fills finds its irreproducible buffers itself"
    runs = [(r, 0) if isinstance(r, int) else (int(r[0]), r[1]) for r in runs]
    jitter = {}
    for n, (fill, skew) in enumerate(runs):
        run = f"run {n} (fill 0x{fill:02X})" if not placement else f"run {n} (fill 0x{fill:02X}, skew {skew})"
        arena = Arena(device, fill, skew)
        outs = list(case(arena))
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize()
        for v in arena.violations():
            problems.append(f"{run}: {v}")
        _check_reference(outs, run, problems)
        bits = {o.name: _bits(o.got) for o in outs}
        if base is None:
            base = {o.name: (bits[o.name], o.got.detach().cpu()) for o in outs}
            continue
        for o in outs:
            if o.name not in base or bits[o.name].shape != base[o.name][0].shape:
                problems.append(f"{run}: {o.name} has {bits[o.name].numel()} bytes, run 0 had "
                                f"{base[o.name][0].numel() if o.name in base else 'no such buffer'}")
                continue
            if torch.equal(bits[o.name], base[o.name][0]):
                continue
            a, b = o.got.detach().cpu().double(), base[o.name][1].double()
            diff = float((a - b).abs().nan_to_num(nan=float("inf")).max())
            n_diff = int((bits[o.name] != base[o.name][0]).sum())
            if placement:
                if o.name in irreproducible:
                    jitter[o.name] = max(jitter.get(o.name, 0.0), diff)
                else:
                    problems.append(f"{run}: {o.name} differs bitwise from run 0 (fill 0x{runs[0][0]:02X}, skew {runs[0][1]}): "
                                    f"{n_diff} bytes, largest difference {diff:.3e} -- the result depends on memory the op does "
                                    f"not own or on where its operands start")
            elif fill == runs[0][0]:     # same pattern, different bits: this buffer is not reproducible
                jitter[o.name] = max(jitter.get(o.name, 0.0), diff)
            elif o.name not in jitter:
                problems.append(f"{run}: {o.name} differs bitwise from run 0 (fill 0x{runs[0][0]:02X}): {n_diff} bytes, largest "
                                f"difference {diff:.3e} -- the result depends on memory the op does not own")
    assert not problems, "memory contract broken:\n  " + "\n  ".join(problems)
    return {"reproducible": not jitter, "irreproducible": jitter}
