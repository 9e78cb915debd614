"""Memory contract of the snake ops (``ops.snake_forward``, ``ops.snake_backward`` in its three forms) on the guarded, poisoned
arena of ``tests/guarded.py``: every operand sits between guard bands, and every byte the ops do not own holds 0x00, 0xFF or
0x7F in turn.  Guards must stay intact, every element of ``out``, ``dx``, ``dalpha`` and of the workspace must be written (a
poisoned one misses the reference), inputs must come back untouched, and the results must be bitwise the same on every
pattern and on both clean runs.  The in-place forms (``out is x``, and ``dx`` written over ``dout`` through the C entry point)
are included.  Tolerances: the derived bounds of tests/snake_ref.py at their largest element, times 2."""
import pytest
import torch

from audio_generation_amd import _lib, ops
from tests import snake_ref as ref
from tests.guarded import Out, routed, run_contract

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(2, 5, 37), (1, 130, 1029)]       # (B, C, T)
ALPHAS = (1.0, -2.5, 7.3, 1e-3, 40.0)       # alpha = 0 (exact facts, and a bound of 1 / eps) is in tests/test_gpu_snake.py


def _tol(bound):
    return 2.0 * float(bound.max()) + 1e-30


@pytest.mark.parametrize("relu", [False, True], ids=["snek", "snekrelu"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_snake_memory_contract(shape, relu):
    b, c, t = shape
    variant = ops.SNAKE_RELU if relu else ops.SNAKE_PLAIN
    gen = torch.Generator().manual_seed(b + c + t)
    x, dout = 2.0 * torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    x[0, 0, 0], x[0, 1, t - 1] = 0.0, -0.0
    alpha = torch.tensor([ALPHAS[ch % len(ALPHAS)] for ch in range(c)])
    x64, a64, d64 = ref.f64(x, alpha, dout)
    d_out, d_dx, d_dalpha = ref.bounds(x64, a64, d64, relu)
    want_dx, want_dalpha = ref.snake_backward(x64, a64, d64, relu)
    want_out, want_ws = ref.snake(x64, a64, relu), ref.partial_sums(x64, a64, d64, relu)
    n, rows = 4 * x.numel(), b * c
    segs = -(-t // ref.SEGMENT)

    def run(arena):
        xd, ad, dd, xi, di = (arena.place(v) for v in (x, alpha, dout, x, dout))
        first = len(arena.allocs)
        with routed(arena, ops):
            out = ops.snake_forward(xd, ad, variant)
            ops.snake_forward(xi, ad, variant, out=xi)
            dx, dalpha = ops.snake_backward(xd, ad, dd, variant)
            dx_only, none = ops.snake_backward(xd, ad, dd, variant, want_dalpha=False)
            none2, dalpha_only = ops.snake_backward(xd, ad, dd, variant, want_dx=False)
        assert none is None and none2 is None
        made = arena.allocs[first:]
        assert [(a.dtype, a.nbytes) for a in made] == [
            (torch.float32, n), (torch.float32, n), (torch.float32, 4 * c), (torch.uint8, 4 * rows * segs), (torch.float32, n),
            (torch.float32, 4 * c), (torch.uint8, 4 * rows * segs)], made
        ws1, ws2 = (a.raw[a.lead:a.lead + a.nbytes].view(torch.float32) for a in (made[3], made[6]))
        # dx over dout through the C entry point (the wrapper always allocates dx): frozen alphas, then the full call
        lib = _lib.load()
        ws3, dalpha3, di2 = arena.empty(rows * segs), arena.empty(c), arena.place(dout)
        for buf, da, ws in ((di, None, None), (di2, dalpha3, ws3)):
            _lib.check(lib.agx_snake_backward(ops._ptr(xd), ops._ptr(ad), ops._ptr(buf), ops._ptr(buf), ops._ptr(da), ops._ptr(ws),
                                              0 if ws is None else 4 * ws.numel(), rows, c, t, variant, 1e-6, ops._stream()),
                       "agx_snake_backward")
        ws_tol = _tol(d_dalpha)          # a partial sum is part of one channel's sum: the channel's bound covers it
        return [Out("out", out, want_out, _tol(d_out)), Out("inplace", xi, want_out, _tol(d_out)),
                Out("dx", dx, want_dx, _tol(d_dx)), Out("dx_only", dx_only, want_dx, _tol(d_dx)),
                Out("dx_over_dout", di, want_dx, _tol(d_dx)), Out("dx_over_dout_full", di2, want_dx, _tol(d_dx)),
                Out("dalpha", dalpha, want_dalpha, _tol(d_dalpha)), Out("dalpha_only", dalpha_only, want_dalpha, _tol(d_dalpha)),
                Out("dalpha_inplace", dalpha3, want_dalpha, _tol(d_dalpha)),
                Out("workspace", ws1, want_ws, ws_tol), Out("workspace_only", ws2, want_ws, ws_tol),
                Out("workspace_inplace", ws3, want_ws, ws_tol),
                Out("x", xd, x, exact=True), Out("alpha", ad, alpha, exact=True), Out("dout", dd, dout, exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]
