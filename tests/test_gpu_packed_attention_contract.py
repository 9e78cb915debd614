"""Memory contract of ``ops.attention_alibi_packed``, ``ops.attention_alibi_packed_backward``, ``ops.pack_rows`` and
``ops.unpack_rows`` on the guarded, poisoned arena of ``tests/guarded.py`` (modelled on
tests/test_gpu_ragged_attention_contract.py): the inputs, the cu arrays, out, dout, the gradients and the workspace sit between
guard bands, and every byte the ops do not own holds 0x00, 0xFF or 0x7F in turn.  Guards must stay intact, every element of
out / dq / dkv and of the workspace must be written (a poisoned one is NaN or huge and misses its float64 reference), the results
must be bitwise the same on every pattern, and the allocations are exactly the output (forward) and the gradients + the workspace
(backward).

The workspace has a reference of its own: lse_i = logsumexp_{j < kl} of the logits taken relative to the sequence's nearest key
(``attn_packed_bwd_logit``) and delta_i = sum_d dout[d, i] out[d, i], both 0 for a sequence without keys and in slack.  Its
tolerance, 1e-4 of max(1, max|reference|), is that of fp32 sums of at most 257 + 128 terms of that size (n * 2^-24 = 2.3e-5 in the
worst case): it is there to tell a written float from a poisoned one (NaN, 3.4e38, 0), not to measure accuracy.  Other
tolerances: those of tests/test_gpu_packed_attention.py."""
import pytest
import torch

from audio_generation_amd import ops
from tests.guarded import Out, routed, run_contract
from tests.packed_attention_ref import CASE_IDS, CASES, case_inputs, case_shape, cu_of, pack_ref, packed_core, unpack_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
PICKED = (1, 3, 4)             # a self case with an empty sequence, the slack case, a cross case
_BUILT = {}
scale = lambda t: max(1.0, float(t.abs().max()))   # noqa: E731


def _workspace_reference(q, kv, dout, out, slopes, heads, dh, ql, kl):
    """(2, H, Nq) float64: lse of the relative logits, then delta."""
    nq = q.shape[-1]
    ws = torch.zeros(2, heads, nq, dtype=torch.float64)
    cq, ck = cu_of(ql), cu_of(kl)
    for s in range(len(ql)):
        a, b, c, d = cq[s], cq[s + 1], ck[s], ck[s + 1]
        if b == a or d == c:
            continue
        qh = q[0, :, a:b].reshape(heads, dh, b - a)
        kh = kv[0, :heads * dh, c:d].reshape(heads, dh, d - c)
        i = torch.arange(b - a, dtype=torch.float64).reshape(-1, 1)
        j = torch.arange(d - c, dtype=torch.float64).reshape(1, -1)
        dist = (i - j).abs() - (i - (d - c - 1)).clamp(min=0)
        sc = torch.einsum("hdi,hdj->hij", qh, kh) / dh ** 0.5 - dist.unsqueeze(0) * slopes.double().reshape(-1, 1, 1)
        ws[0, :, a:b] = sc.logsumexp(-1)
        ws[1, :, a:b] = (dout[0, :, a:b] * out[0, :, a:b]).reshape(heads, dh, b - a).sum(1)
    return ws


def _build(n):
    if n not in _BUILT:
        kind, heads, dh, ql, kl, nq, nk, max_q, max_k = case_shape(CASES[n])
        q, kv, dout, slopes = case_inputs(heads, dh, nq, nk)
        q64, kv64 = q.double().requires_grad_(), kv.double().requires_grad_()
        out = packed_core(q64, kv64, slopes, heads, dh, dh ** 0.5, cu_of(ql), cu_of(kl))
        out.backward(dout.double())
        ws = _workspace_reference(q.double(), kv.double(), dout.double(), out.detach(), slopes, heads, dh, ql, kl)
        _BUILT[n] = dict(q=q, kv=kv, dout=dout, slopes=slopes, out=out.detach(), dq=q64.grad, dkv=kv64.grad, ws=ws,
                         cu_q=torch.tensor(cu_of(ql), dtype=torch.int32), cu_k=torch.tensor(cu_of(kl), dtype=torch.int32))
    return _BUILT[n]


@pytest.mark.parametrize("n", PICKED, ids=[CASE_IDS[n] for n in PICKED])
def test_packed_attention_memory_contract(n):
    kind, heads, dh, ql, kl, nq, nk, max_q, max_k = case_shape(CASES[n])
    c = _build(n)
    hd = heads * dh

    def run(arena):
        dout, slopes, cu_q, cu_k = (arena.place(c[key]) for key in ("dout", "slopes", "cu_q", "cu_k"))
        if kind == "self":
            q, kv, part = arena.place(torch.cat([c["q"], c["kv"]], dim=1)), None, dict(cu_q=cu_q, max_q=max_q)
        else:
            q, kv, part = arena.place(c["q"]), arena.place(c["kv"]), dict(cu_q=cu_q, max_q=max_q, cu_k=cu_k, max_k=max_k)
        first = len(arena.allocs)
        with routed(arena, ops):
            out = ops.attention_alibi_packed(q, kv, slopes, heads, dh, dh ** 0.5, **part)
            assert len(arena.allocs) == first + 1                       # the forward allocates its output and nothing else
            got = ops.attention_alibi_packed_backward(q, kv, slopes, out, dout, heads, dh, dh ** 0.5, **part)
        made = [(a.dtype, a.nbytes) for a in arena.allocs[first + 1:]]
        grads = [(torch.float32, 3 * hd * nq * 4)] if kind == "self" else [(torch.float32, hd * nq * 4), (torch.float32, 2 * hd * nk * 4)]
        assert made == grads + [(torch.uint8, 2 * heads * nq * 4)], made
        w = arena.allocs[-1]
        ws = w.raw[w.lead:w.lead + w.nbytes].view(torch.float32).reshape(2, heads, nq)
        dq, dkv = (got[:, :hd], got[:, hd:]) if kind == "self" else got
        return [Out("out", out, c["out"], 3e-5 * scale(c["out"])), Out("dq", dq, c["dq"], 5e-5 * scale(c["dq"])),
                Out("dkv", dkv, c["dkv"], 5e-5 * scale(c["dkv"])), Out("workspace", ws, c["ws"], 1e-4 * scale(c["ws"]))]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


@pytest.mark.parametrize("shape,lengths,total", [((3, 5, 37), [37, 0, 20], 57), ((2, 3, 5), [5, 2], 12), ((2, 64, 225), [1, 100], 101)])
def test_pack_and_unpack_rows_memory_contract(shape, lengths, total):
    """The padding of x and the slack of xp hold the arena's poison: neither is read into a result, and every element of both
    outputs is written."""
    b, c, t = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=gen)
    pads = (torch.arange(t).reshape(1, 1, t) >= torch.tensor(lengths).reshape(-1, 1, 1)).expand(shape)
    packed = pack_ref(x, lengths, total)
    slack = (torch.arange(total) >= sum(lengths)).reshape(1, 1, total).expand(1, c, total)
    padded = unpack_ref(packed, cu_of(lengths), t)

    def run(arena):
        poison = torch.full((1,), arena.fill, dtype=torch.uint8).repeat(4).view(torch.float32).item()
        xd = arena.place(torch.where(pads, torch.full_like(x, poison), x))
        xpd = arena.place(torch.where(slack, torch.full_like(packed, poison), packed))
        cu = arena.place(torch.tensor(cu_of(lengths), dtype=torch.int32))
        first = len(arena.allocs)
        with routed(arena, ops):
            xp = ops.pack_rows(xd, cu, total)
            back = ops.unpack_rows(xpd, cu, t)
            assert len(arena.allocs) == first + 2                       # one output each
        return [Out("packed", xp, packed, exact=True), Out("padded", back, padded, exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]
