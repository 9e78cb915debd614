"""Memory contract of ``ops.attention_alibi_dropout``, ``ops.attention_alibi_dropout_backward`` and ``ops.dropout_add`` on the
guarded, poisoned arena of ``tests/guarded.py``, as tests/test_gpu_cross_attention_contract.py does for cross-attention: every
operand sits between guard bands, and every byte the ops do not own holds 0x00, 0xFF or 0x7F in turn.  Guards must stay intact,
every element of the outputs must be written (a poisoned one misses the reference; the workspace is exactly the bytes the
library asks for, and lse / delta feed every element of dq / dkv), and the results must be bitwise the same on every pattern.
One cross case per head-dim tile plus the self-attention pointers and strides, where q, k and v (dq, dk and dv) are thirds of
one allocation.  Tolerances: those of tests/test_gpu_dropout.py."""
import numpy as np
import pytest
import torch

from audio_generation_amd import ops
from oracle import attention as oattn
from tests import philox
from tests.dropout_ref import attention_factor, drop_core
from tests.guarded import Out, routed, run_contract

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (B, H, Dh, Tq, Tk, self): the three head-dim tiles, tails past a 64-key and a 128-query boundary, the qkv form
CASES = [(2, 3, 24, 37, 37, True), (1, 2, 64, 130, 70, False), (2, 2, 128, 17, 129, False)]
P, SEED, STREAM = 0.25, 0x1F2E3D4C5B6A7988, 2
_BUILT = {}


def _build(case):
    if case not in _BUILT:
        b, heads, dh, tq, tk, _ = case
        gen = torch.Generator().manual_seed(sum(case[:5]))
        q = 0.7 * torch.randn(b, heads * dh, tq, generator=gen)
        kv = 0.7 * torch.randn(b, 2 * heads * dh, tk, generator=gen)
        dout = torch.randn(b, heads * dh, tq, generator=gen)
        slopes = oattn.alibi_slopes(heads)
        q64, kv64 = q.double().requires_grad_(), kv.double().requires_grad_()
        out = drop_core(q64, kv64, slopes, heads, dh, dh ** 0.5, attention_factor(SEED, STREAM, P, b, heads, tq, tk))
        out.backward(dout.double())
        _BUILT[case] = dict(q=q, kv=kv, dout=dout, slopes=slopes, out=out.detach(), dq=q64.grad, dkv=kv64.grad)
        if case[5]:      # the qkv form: tq == tk
            _BUILT[case].update(qkv=torch.cat([q, kv], dim=1), dqkv=torch.cat([q64.grad, kv64.grad], dim=1))
    return _BUILT[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:5])) + ("-self" if c[5] else ""))
def test_attention_dropout_memory_contract(case):
    b, heads, dh, tq, tk, self_attention = case
    c = _build(case)
    scale = lambda t: max(1.0, float(t.abs().max()))   # noqa: E731
    drop = (P, SEED, STREAM)

    def run(arena):
        dout, slopes = arena.place(c["dout"]), arena.place(c["slopes"])
        q, kv = (arena.place(c["qkv"]), None) if self_attention else (arena.place(c["q"]), arena.place(c["kv"]))
        first = len(arena.allocs)
        with routed(arena, ops):
            out = ops.attention_alibi_dropout(q, kv, slopes, heads, dh, dh ** 0.5, *drop)
            assert len(arena.allocs) == first + 1                       # the forward allocates its output and nothing else
            grads = ops.attention_alibi_dropout_backward(q, kv, slopes, out, dout, heads, dh, dh ** 0.5, *drop)
        made = [(a.dtype, a.nbytes) for a in arena.allocs[first + 1:]]
        ws = (torch.uint8, 2 * b * heads * tq * 4)
        if self_attention:
            assert made == [(torch.float32, q.numel() * 4), ws], made
            return [Out("out", out, c["out"], 3e-5 * scale(c["out"])), Out("dqkv", grads, c["dqkv"], 5e-5 * scale(c["dqkv"]))]
        assert made == [(torch.float32, q.numel() * 4), (torch.float32, kv.numel() * 4), ws], made
        return [Out("out", out, c["out"], 3e-5 * scale(c["out"])),
                Out("dq", grads[0], c["dq"], 5e-5 * scale(c["dq"])),
                Out("dkv", grads[1], c["dkv"], 5e-5 * scale(c["dkv"]))]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


@pytest.mark.parametrize("n", [5, 1027])
def test_dropout_add_memory_contract(n):
    """A new output, an in-place call, and a call without residual: exact against the mirror (the scalar tail and the 16-byte
    path both end at the payload's last byte)."""
    gen = torch.Generator().manual_seed(n)
    x, res = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    thresh, scale = philox.thresh_scale(P)
    masked = np.where(philox.elementwise_keep(SEED, STREAM, P, n), x.numpy() * scale, np.float32(0.0)).astype(np.float32)
    with_res, without = torch.from_numpy(res.numpy() + masked), torch.from_numpy(masked)

    def run(arena):
        xd, rd, xi = arena.place(x), arena.place(res), arena.place(x)
        first = len(arena.allocs)
        with routed(arena, ops):
            new = ops.dropout_add(xd, rd, P, SEED, STREAM)
            bare = ops.dropout_add(xd, None, P, SEED, STREAM)
            ops.dropout_add(xi, rd, P, SEED, STREAM, out=xi)
        assert [(a.dtype, a.nbytes) for a in arena.allocs[first:]] == [(torch.float32, 4 * n)] * 2
        return [Out("new", new, with_res, exact=True), Out("bare", bare, without, exact=True), Out("inplace", xi, with_res, exact=True),
                Out("x", xd, x, exact=True), Out("res", rd, res, exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]
