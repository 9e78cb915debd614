"""Memory contract of ``ops.attention_alibi_ragged``, ``ops.attention_alibi_ragged_backward`` and ``ops.mask_tail`` on the
guarded, poisoned arena of ``tests/guarded.py`` (modelled on tests/test_gpu_window_attention_contract.py): the inputs, the two
length arrays, out, dout, the gradients and the workspace sit between guard bands, and every byte the ops do not own holds 0x00,
0xFF or 0x7F in turn.  Guards must stay intact, every element of out / dq / dkv and of the workspace must be written (a poisoned
one is NaN or huge and misses its float64 reference), the results must be bitwise the same on every pattern, and the
allocations are exactly the output (forward) and the gradients + the workspace (backward).

The workspace has a reference of its own: lse_i = logsumexp_{j < kl} of the logits taken relative to the row's nearest key
(``attn_ragged_bwd_logit``) and delta_i = sum_d dout[d, i] out[d, i], both 0 for a masked query and for a row without keys.
Its tolerance, 1e-4 of max(1, max|reference|), is that of fp32 sums of at most 257 + 128 terms of that size (n * 2^-24 = 2.3e-5
in the worst case): it is there to tell a written float from a poisoned one (NaN, 3.4e38, 0), not to measure accuracy.
Other tolerances: those of tests/test_gpu_ragged_attention.py."""
import pytest
import torch

from audio_generation_amd import ops
from tests.guarded import Out, routed, run_contract
from tests.ragged_attention_ref import CASE_IDS, CASES, case_inputs, pad_mask, ragged_core

pytestmark = pytest.mark.gpu
DEV = "cuda"
PICKED = (1, 2, 4)             # cases 2, 3 and 5
_BUILT = {}
scale = lambda t: max(1.0, float(t.abs().max()))   # noqa: E731


def _workspace_reference(q, kv, dout, out, slopes, heads, dh, q_len, k_len):
    """(2, B, H, Tq) float64: lse of the relative logits, then delta."""
    b, _, tq = q.shape
    ws = torch.zeros(2, b, heads, tq, dtype=torch.float64)
    for r in range(b):
        ql, kl = q_len[r], k_len[r]
        if ql == 0 or kl == 0:
            continue
        qh = q[r, :, :ql].reshape(heads, dh, ql)
        kh = kv[r, :heads * dh, :kl].reshape(heads, dh, kl)
        i = torch.arange(ql, dtype=torch.float64).reshape(-1, 1)
        j = torch.arange(kl, dtype=torch.float64).reshape(1, -1)
        dist = (i - j).abs() - (i - (kl - 1)).clamp(min=0)
        s = torch.einsum("hdi,hdj->hij", qh, kh) / dh ** 0.5 - dist.unsqueeze(0) * slopes.double().reshape(-1, 1, 1)
        ws[0, r, :, :ql] = s.logsumexp(-1)
        ws[1, r, :, :ql] = (dout[r, :, :ql] * out[r, :, :ql]).reshape(heads, dh, ql).sum(1)
    return ws


def _build(n):
    if n not in _BUILT:
        kind, b, heads, dh, tq, tk, q_len, k_len = CASES[n]
        q, kv, dout, slopes = case_inputs(b, heads, dh, tq, tk)
        q64, kv64 = q.double().requires_grad_(), kv.double().requires_grad_()
        out = ragged_core(q64, kv64, slopes, heads, dh, dh ** 0.5, q_len, k_len)
        out.backward(dout.double())
        ws = _workspace_reference(q.double(), kv.double(), dout.double(), out.detach(), slopes, heads, dh, q_len, k_len)
        _BUILT[n] = dict(q=q, kv=kv, dout=dout, slopes=slopes, out=out.detach(), dq=q64.grad, dkv=kv64.grad, ws=ws,
                         q_len=torch.tensor(q_len, dtype=torch.int32), k_len=torch.tensor(k_len, dtype=torch.int32))
    return _BUILT[n]


@pytest.mark.parametrize("n", PICKED, ids=[CASE_IDS[n] for n in PICKED])
def test_ragged_attention_memory_contract(n):
    kind, b, heads, dh, tq, tk, _, _ = CASES[n]
    c = _build(n)
    hd = heads * dh

    def run(arena):
        dout, slopes, q_len, k_len = (arena.place(c[key]) for key in ("dout", "slopes", "q_len", "k_len"))
        if kind == "self":
            q, kv = arena.place(torch.cat([c["q"], c["kv"]], dim=1)), None
        else:
            q, kv = arena.place(c["q"]), arena.place(c["kv"])
        first = len(arena.allocs)
        with routed(arena, ops):
            out = ops.attention_alibi_ragged(q, kv, slopes, heads, dh, dh ** 0.5, q_len=q_len, k_len=k_len)
            assert len(arena.allocs) == first + 1                       # the forward allocates its output and nothing else
            got = ops.attention_alibi_ragged_backward(q, kv, slopes, out, dout, heads, dh, dh ** 0.5, q_len=q_len, k_len=k_len)
        made = [(a.dtype, a.nbytes) for a in arena.allocs[first + 1:]]
        grads = [(torch.float32, 3 * hd * tq * b * 4)] if kind == "self" else [(torch.float32, hd * tq * b * 4), (torch.float32, 2 * hd * tk * b * 4)]
        assert made == grads + [(torch.uint8, 2 * b * heads * tq * 4)], made
        w = arena.allocs[-1]
        ws = w.raw[w.lead:w.lead + w.nbytes].view(torch.float32).reshape(2, b, heads, tq)
        dq, dkv = (got[:, :hd], got[:, hd:]) if kind == "self" else got
        return [Out("out", out, c["out"], 3e-5 * scale(c["out"])), Out("dq", dq, c["dq"], 5e-5 * scale(c["dq"])),
                Out("dkv", dkv, c["dkv"], 5e-5 * scale(c["dkv"])), Out("workspace", ws, c["ws"], 1e-4 * scale(c["ws"]))]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


@pytest.mark.parametrize("shape,lengths", [((3, 5, 37), [37, 0, 20]), ((2, 3, 5), [5, 2]), ((2, 64, 225), [1, 100])])
def test_mask_tail_memory_contract(shape, lengths):
    """Out of place and in place; the padded tail of x holds the arena's poison (it is overwritten here with the fill byte)."""
    b, c, t = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=gen)
    pads = pad_mask(lengths, t).expand(shape)
    want = x.masked_fill(pads, 0.0)

    def run(arena):
        poison = torch.full((1,), arena.fill, dtype=torch.uint8).repeat(4).view(torch.float32).item()
        xd = arena.place(torch.where(pads, torch.full_like(x, poison), x))
        ld = arena.place(torch.tensor(lengths, dtype=torch.int32))
        first = len(arena.allocs)
        with routed(arena, ops):
            out = ops.mask_tail(xd, ld)
            assert len(arena.allocs) == first + 1
            same = ops.mask_tail(xd, ld, out=xd)
            assert same is xd and len(arena.allocs) == first + 1        # in place: no allocation
        return [Out("out", out, want, exact=True), Out("in place", xd, want, exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]
