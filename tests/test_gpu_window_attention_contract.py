"""Memory contract of ``ops.attention_alibi_window`` and ``ops.attention_alibi_window_backward`` on the guarded, poisoned arena
of ``tests/guarded.py`` (modelled on tests/test_gpu_causal_attention_contract.py): qkv, slopes, out, dout, dqkv and the
workspace sit between guard bands, and every byte the ops do not own holds 0x00, 0xFF or 0x7F in turn.  Guards must stay intact,
every element of the outputs must be written (a poisoned one is NaN or huge and misses the float64 definition), the results
must be bitwise the same on every pattern, and the allocations are exactly the output (forward) and dqkv + the workspace
(backward).  The ring case reads a key/value ring whose columns outside the window were never written: they hold the arena's
poison and must not reach the output.  Tolerances: those of tests/test_gpu_window_attention.py."""
import pytest
import torch

from audio_generation_amd import ops
from oracle import attention as oattn
from tests.guarded import Out, routed, run_contract
from tests.window_attention_ref import window_core

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (B, H, Dh, T, W): the three head-dim tiles, tails past a 64-key and a 128-query boundary, a leading all-masked block
CASES = [(2, 3, 16, 37, 5), (1, 2, 64, 130, 3), (1, 2, 128, 257, 100)]
_BUILT = {}
scale = lambda t: max(1.0, float(t.abs().max()))   # noqa: E731


def _build(case):
    if case not in _BUILT:
        b, heads, dh, t, w = case
        hd = heads * dh
        gen = torch.Generator().manual_seed(sum(case))
        qkv = 0.7 * torch.randn(b, 3 * hd, t, generator=gen)
        dout = torch.randn(b, hd, t, generator=gen)
        slopes = oattn.alibi_slopes(heads)
        qkv64 = qkv.double().requires_grad_()
        out = window_core(qkv64[:, :hd], qkv64[:, hd:], slopes, heads, dh, dh ** 0.5, w)
        out.backward(dout.double())
        _BUILT[case] = dict(qkv=qkv, dout=dout, slopes=slopes, out=out.detach(), dqkv=qkv64.grad)
    return _BUILT[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_window_attention_memory_contract(case):
    b, heads, dh, t, w = case
    c = _build(case)

    def run(arena):
        qkv, dout, slopes = (arena.place(c[key]) for key in ("qkv", "dout", "slopes"))
        first = len(arena.allocs)
        with routed(arena, ops):
            out = ops.attention_alibi_window(qkv, None, slopes, heads, dh, dh ** 0.5, w)
            assert len(arena.allocs) == first + 1                       # the forward allocates its output and nothing else
            dqkv = ops.attention_alibi_window_backward(qkv, slopes, out, dout, heads, dh, dh ** 0.5, w)
        made = [(a.dtype, a.nbytes) for a in arena.allocs[first + 1:]]
        assert made == [(torch.float32, qkv.numel() * 4), (torch.uint8, 2 * b * heads * t * 4)], made
        return [Out("out", out, c["out"], 3e-5 * scale(c["out"])), Out("dqkv", dqkv, c["dqkv"], 5e-5 * scale(c["dqkv"]))]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


def test_ring_step_memory_contract():
    """33 new queries at positions 224.. with a window of 40 on a ring of 96 columns in rows of pitch 100: the keys 185 .. 256
    sit at j mod 96 (the chunk wraps the ring), and the 24 ring columns outside the window as well as the 4 columns beyond the
    ring keep the arena's poison (0x00, 0xFF = NaN, 0x7F = 3.4e38) in every K and V row."""
    b, heads, dh, tq, q_pos0, w, ring, pitch = 2, 2, 64, 33, 224, 40, 96, 100
    hd = heads * dh
    tk = q_pos0 + tq
    gen = torch.Generator().manual_seed(78)
    q = 0.7 * torch.randn(b, hd, tq, generator=gen)
    kv = 0.7 * torch.randn(b, 2 * hd, tk, generator=gen)
    slopes = oattn.alibi_slopes(heads)
    want = window_core(q.double(), kv.double(), slopes, heads, dh, dh ** 0.5, w, q_pos0=q_pos0)
    lo = q_pos0 - w + 1
    cols = torch.tensor([j % ring for j in range(lo, tk)])
    assert len(set(cols.tolist())) == tk - lo == 72 and int(cols[0]) > int(cols[-1])      # distinct columns; the span wraps

    def run(arena):
        qd, sd = arena.place(q), arena.place(slopes)
        buf = arena.empty((b, 2 * hd, pitch))
        buf[..., cols.to(buf.device)] = kv[..., lo:].to(buf.device)
        first = len(arena.allocs)
        with routed(arena, ops):
            out = ops.attention_alibi_window(qd, buf, sd, heads, dh, dh ** 0.5, w, q_pos0=q_pos0, ring=ring)
        assert len(arena.allocs) == first + 1
        return [Out("out", out, want, 3e-5 * scale(want))]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]
