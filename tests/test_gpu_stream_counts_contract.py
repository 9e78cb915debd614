"""Memory contract (tests/guarded.py) of the counted streaming ops: every output, ring, history and position sits between guard
bands and starts as poison (0x00, NaN, 3.4e38); the poison survives wherever a counted op must not write; and ``counts`` holds
-1 and n + 1, which must behave as 0 and n -- a missing clamp shows as a damaged guard band or a changed poison byte, not as a
fault.  Four rows: count -1 (nothing), n + 1 (everything), 2 of 3 frames, and 0.

The conv step is held against the float64 restatement (tests/codec_stream_ref.py) within twice its derived bound, as
tests/test_gpu_conv_stream_contract.py does; the data movers and the GLU step against the uncounted op on the row's own frames,
exactly."""
import pytest
import torch

from audio_generation_amd import ops
from tests import codec_stream_ref as ref
from tests.guarded import Out, routed, run_contract
from tests.test_gpu_conv_stream import _unit
from tests.test_gpu_conv_stream_contract import MAX_CHUNK, N, _columns, _poisoned_ring

pytestmark = pytest.mark.gpu
DEV = "cuda"
POS = [5, 1 << 33, 2, 7]
COUNTS = [-1, N + 1, 2, 0]
TAKEN = [0, N, 2, 0]                     # what the kernels make of COUNTS
B = len(POS)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _kept(cap, cols_per_row, channels):
    """Mask (B, channels, cap) of the ring elements a counted op must leave alone: everything but the given columns."""
    keep = torch.ones(B, cap, dtype=torch.bool)
    for r, cols in enumerate(cols_per_row):
        keep[r, cols] = False
    return keep[:, None, :].expand(-1, channels, -1).to(DEV)


@pytest.mark.parametrize("name", ["causal", "up", "res33"])
def test_counted_step_memory_contract(name):
    unit, rate_in = _unit(name)
    first, last = unit[0], unit[-1]
    reach = first.d * (first.k - 1) if len(unit) == 2 else first.ref.reach
    rate_out, delay_out = first.ref.rates(rate_in, 0)
    cap, cap_out = reach + MAX_CHUNK * rate_in, MAX_CHUNK * rate_out + 3
    have = reach + N * rate_in
    values = torch.randn(B, first.c_in, have, generator=torch.Generator().manual_seed(41))
    clean = torch.zeros(B, first.c_in, cap, dtype=torch.float64)
    for r, cols in enumerate(_columns([p + N for p in POS], have, rate_in, have, cap)):
        clean[r][:, cols] = values[r].double()
    scratch = torch.zeros(B, last.c_out, cap_out, dtype=torch.float64)
    if len(unit) == 2:
        want, bound = ref.res_unit_step(first.ref, last.ref, clean, scratch, POS, None, N, rate_in, 0)
    else:
        want, bound = ref.step(first.ref, clean, scratch, POS, None, N, rate_in, 0)
    want = want.clone()
    for r, c in enumerate(TAKEN):
        want[r, :, c * rate_out:] = 0.0                     # a plain destination: exact zeros behind the count
    assert float(want[1].abs().min()) > 0 and float(want[2, :, :2 * rate_out].abs().min()) > 0
    out_cols = [cols[:c * rate_out] for cols, c in zip(_columns(POS, N * rate_out, rate_out, delay_out, cap_out), TAKEN)]

    def run(arena):
        src = _poisoned_ring(arena, values, POS, rate_in, cap)
        ring, plain = arena.empty((B, last.c_out, cap_out)), arena.empty((B, last.c_out, N * rate_out))
        pos, counts = arena.place(torch.tensor(POS)), arena.place(torch.tensor(COUNTS))
        packed = [arena.place(op.packed.cpu()) for op in unit]
        bias = [arena.place(op.bias.cpu()) for op in unit]
        before, src_before = ring.clone(), src.clone()
        with routed(arena, ops):
            for dst, dst_ring in ((ring, True), (plain, False)):
                if len(unit) == 2:
                    hid = arena.empty((B, first.c_out, N * rate_in))
                    first.packed, first.bias, last.packed, last.bias = packed[0], bias[0], packed[1], bias[1]
                    first.launch(src, hid, pos, None, N, rate_in, 0, dst_ring=False, counts=counts)
                    last.launch(hid, dst, pos, None, N, rate_in, 0, src_ring=False, dst_ring=dst_ring, res=src, counts=counts)
                else:
                    first.packed, first.bias = packed[0], bias[0]
                    first.launch(src, dst, pos, None, N, rate_in, 0, dst_ring=dst_ring, counts=counts)
        torch.cuda.synchronize()
        keep = _kept(cap_out, out_cols, last.c_out)
        assert torch.equal(_bits(ring[keep]), _bits(before[keep])), "a ring column behind a row's count was written"
        assert torch.equal(_bits(src), _bits(src_before)), "the source ring was written"
        for r, c in enumerate(TAKEN):
            assert float(plain[r, :, c * rate_out:].abs().max() if c < N else 0.0) == 0.0, r
        got = torch.cat([ring[r][:, cols.to(DEV)] for r, cols in enumerate(out_cols)], dim=1)
        want_ring = torch.cat([want[r, :, :c * rate_out] for r, c in enumerate(TAKEN)], dim=1)
        tol = 2.0 * float(bound.max())
        return [Out("ring block", got, want_ring, tol), Out("plain", plain, want, tol), Out("pos", pos, torch.tensor(POS), exact=True),
                Out("counts", counts, torch.tensor(COUNTS), exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


def test_counted_data_movers_memory_contract():
    """``ring_write_rate``, ``ring_write_pos``, ``stream_advance`` and ``mask_tail`` with counts."""
    c, rate, cap, ring_cols = 5, 3, 14, 11
    gen = torch.Generator().manual_seed(43)
    x = torch.randn(B, c, N * rate, generator=gen)
    kv = torch.randn(B, c, N, generator=gen)
    rate_cols = [cols[:t * rate] for cols, t in zip(_columns(POS, N * rate, rate, 0, cap), TAKEN)]
    pos_cols = [torch.remainder(torch.arange(p, p + t), ring_cols) for p, t in zip(POS, TAKEN)]
    masked = x.clone()
    for r, t in enumerate(TAKEN):
        masked[r, :, t * rate:] = 0.0

    def run(arena):
        ring, buf = arena.empty((B, c, cap)), arena.empty((B, c, ring_cols))
        before, buf_before = ring.clone(), buf.clone()
        src, src_kv = arena.empty((B, c, N * rate)), arena.empty((B, c, N))         # behind a row's count: the arena's poison
        for r, t in enumerate(TAKEN):
            src[r, :, :t * rate] = x[r, :, :t * rate].to(DEV)
            src_kv[r, :, :t] = kv[r, :, :t].to(DEV)
        pos, pos2 = arena.place(torch.tensor(POS)), arena.place(torch.tensor(POS))
        counts = arena.place(torch.tensor(COUNTS))
        with routed(arena, ops):
            ops.ring_write_rate(ring, src, pos, rate, counts=counts)
            ops.ring_write_pos(buf, src_kv, pos, ring_cols, counts=counts)
            ops.stream_advance(pos2, N, counts=counts)
            out = ops.mask_tail(src, None, counts=torch.mul(counts, rate))          # (-3, 12, 6, 0) against T = 9
            ops.mask_tail(src, None, out=src, counts=torch.mul(counts, rate))
        torch.cuda.synchronize()
        assert torch.equal(_bits(ring[_kept(cap, rate_cols, c)]), _bits(before[_kept(cap, rate_cols, c)]))
        assert torch.equal(_bits(buf[_kept(ring_cols, pos_cols, c)]), _bits(buf_before[_kept(ring_cols, pos_cols, c)]))
        got = torch.cat([ring[r][:, cc.to(DEV)] for r, cc in enumerate(rate_cols)], dim=1)
        got_kv = torch.cat([buf[r][:, cc.to(DEV)] for r, cc in enumerate(pos_cols)], dim=1)
        return [Out("rate columns", got, torch.cat([x[r, :, :t * rate] for r, t in enumerate(TAKEN)], dim=1), exact=True),
                Out("pos columns", got_kv, torch.cat([kv[r, :, :t] for r, t in enumerate(TAKEN)], dim=1), exact=True),
                Out("pos", pos, torch.tensor(POS), exact=True), Out("counts", counts, torch.tensor(COUNTS), exact=True),
                Out("advanced", pos2, torch.tensor([p + t for p, t in zip(POS, TAKEN)]), exact=True),
                Out("masked", out, masked, exact=True), Out("masked in place", src, masked, exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


@pytest.mark.parametrize("k", [4, 1])
def test_counted_glu_step_memory_contract(k):
    c = 37
    gen = torch.Generator().manual_seed(47 + k)
    u = torch.randn(B, 2 * c, N, generator=gen)
    hist = torch.randn(B, c, k - 1, generator=gen)
    w, bias = torch.randn(c, 1, k, generator=gen).to(DEV), torch.randn(c, generator=gen).to(DEV)
    bn = tuple(t.to(DEV) for t in (torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen), torch.randn(c, generator=gen),
                                   torch.rand(c, generator=gen) + 0.5))
    want_y, want_h = torch.zeros(B, c, N), hist.clone()
    for r, t in enumerate(TAKEN):                           # the uncounted step on the row's own frames
        if t:
            h = hist[r:r + 1].to(DEV).contiguous() if k > 1 else None
            want_y[r, :, :t] = ops.glu_dwconv_step(u[r:r + 1, :, :t].contiguous().to(DEV), w, bias, bn, h)[0].cpu()
            if k > 1:
                want_h[r] = h[0].cpu()

    def run(arena):
        ud = arena.empty((B, 2 * c, N))                     # behind a row's count: the arena's poison
        for r, t in enumerate(TAKEN):
            ud[r, :, :t] = u[r, :, :t].to(DEV)
        hd = arena.place(hist) if k > 1 else None
        counts = arena.place(torch.tensor(COUNTS))
        with routed(arena, ops):
            y = ops.glu_dwconv_step(ud, w, bias, bn, hd, counts=counts)
        outs = [Out("y", y, want_y, exact=True), Out("counts", counts, torch.tensor(COUNTS), exact=True)]
        return outs + ([Out("hist", hd, want_h, exact=True)] if k > 1 else [])
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


def test_counted_stream_attention_memory_contract():
    """``attention_alibi_stream(counts=)`` on a ring that holds the row's own frames and the arena's poison everywhere else, the
    columns of the chunk behind the count included: the queries below the count are the uncounted op on those frames, exactly."""
    from oracle import attention as oattn
    heads, dh, w, ring_cols = 2, 16, 5, 11
    hd = heads * dh
    gen = torch.Generator().manual_seed(53)
    q = 0.7 * torch.randn(B, hd, N, generator=gen)
    frames = {(r, j): 0.7 * torch.randn(2 * hd, generator=gen) for r, (p, t) in enumerate(zip(POS, TAKEN))
              for j in range(max(0, p - w + 1), p + t)}
    slopes = oattn.alibi_slopes(heads).to(DEV)

    def ring_of(make):
        kv = make((B, 2 * hd, ring_cols))
        for (r, j), v in frames.items():
            kv[r, :, j % ring_cols] = v.to(DEV)
        return kv

    clean = ring_of(lambda shape: torch.zeros(shape, device=DEV))
    want = []
    for r, t in enumerate(TAKEN):
        if t:
            want.append(ops.attention_alibi_stream(q[r:r + 1, :, :t].contiguous().to(DEV), clean[r:r + 1],
                                                   torch.tensor(POS[r:r + 1], device=DEV), slopes, heads, dh, dh ** 0.5, w, ring_cols)[0].cpu())
    want = torch.cat(want, dim=1)

    def run(arena):
        kv = ring_of(arena.empty)
        before = kv.clone()
        qd = arena.empty((B, hd, N))                        # behind a row's count: the arena's poison
        for r, t in enumerate(TAKEN):
            qd[r, :, :t] = q[r, :, :t].to(DEV)
        pos, counts = arena.place(torch.tensor(POS)), arena.place(torch.tensor(COUNTS))
        with routed(arena, ops):
            out = ops.attention_alibi_stream(qd, kv, pos, slopes, heads, dh, dh ** 0.5, w, ring_cols, counts=counts)
        torch.cuda.synchronize()
        assert torch.equal(_bits(kv), _bits(before)), "the attention wrote its ring"
        got = torch.cat([out[r, :, :t] for r, t in enumerate(TAKEN)], dim=1)
        return [Out("valid queries", got, want, exact=True), Out("pos", pos, torch.tensor(POS), exact=True),
                Out("counts", counts, torch.tensor(COUNTS), exact=True)]
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]
