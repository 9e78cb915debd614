"""Sliding-window causal ALiBi self-attention on the GPU (csrc/attention_window.hip): the op against the float64 definition of
``tests/window_attention_ref.py`` -- forward, ring buffers with poisoned and stale columns, the exact window, backward -- and the
modules (``window=``, the ring key/value cache, an unbounded stream) against the float64 checker.

Tolerances are the ones tests/test_gpu_causal_attention.py states for the same arithmetic: 3e-5 of max(1, max|o|) for the fp32
flash forward, 5e-5 / 1e-5 (max / rms) for the split backward, 2e-5 of max(1, max|y|) for a block on other values, 2e-4 / 5e-4
for input / parameter gradients of a block."""
import copy
import ctypes

import pytest
import torch

from audio_generation_amd import _lib, ops
from audio_generation_amd._lib import AgxError
from audio_generation_amd.transformers import Transformer, TransformerBottleneck, TransformerCache
from oracle import attention as oattn
from tests.helpers import max_abs, rms
from tests.window_attention_ref import window_core, window_transformer

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _qkv(b, heads, dh, t, seed=0):
    gen = torch.Generator().manual_seed(1000 * t + dh + seed)
    qkv = 0.7 * torch.randn(b, 3 * heads * dh, t, generator=gen)
    dout = torch.randn(b, heads * dh, t, generator=gen)
    return qkv, dout, oattn.alibi_slopes(heads)


def _core64(qkv, slopes, heads, dh, w, **kw):
    hd = heads * dh
    return window_core(qkv[:, :hd].double(), qkv[:, hd:].double(), slopes, heads, dh, dh ** 0.5, w, **kw)


# the three head-dim tiles; T = 130, W = 3: query 127 of workgroup 0 meets block 0 before it has seen a key; the window edge on a
# key-block boundary from both sides; left blocks skipped in the third workgroup; W >= T (the causal op)
@pytest.mark.parametrize("b,heads,dh,t,w", [(2, 1, 8, 1, 1), (2, 3, 16, 37, 5), (1, 2, 64, 130, 3), (1, 2, 64, 130, 64),
                                            (1, 2, 64, 130, 65), (1, 2, 100, 257, 128), (1, 2, 128, 300, 200), (2, 8, 64, 130, 130),
                                            (2, 8, 64, 130, 1000)])
def test_window_forward_against_the_definition(b, heads, dh, t, w):
    qkv, _, slopes = _qkv(b, heads, dh, t)
    want = _core64(qkv, slopes, heads, dh, w)
    got = ops.attention_alibi_window(qkv.to(DEV), None, slopes.to(DEV), heads, dh, dh ** 0.5, w)
    assert tuple(got.shape) == (b, heads * dh, t)
    assert bool(torch.isfinite(got).all())          # an unhandled leading all-masked block is NaN
    err, scale = max_abs(got.cpu(), want), float(want.abs().max())
    print(f"window forward {(b, heads, dh, t, w)}: max err {err:.3e}, max|o| {scale:.3e}")
    assert err < 3e-5 * max(1.0, scale)
    if w >= t:
        causal = ops.attention_alibi_causal(qkv.to(DEV), None, slopes.to(DEV), heads, dh, dh ** 0.5)
        diff = max_abs(got.cpu(), causal.cpu().double())
        print(f"window forward {(b, heads, dh, t, w)}: max difference from attention_alibi_causal {diff:.3e}")
        assert diff < 3e-5 * max(1.0, scale)
    if w == 1:
        assert torch.equal(got.cpu(), qkv[:, 2 * heads * dh:])      # softmax over one key is 1: v_p itself


@pytest.mark.parametrize("dh,tq,q_pos0,w,ring", [(64, 1, 69, 16, 32), (16, 5, 125, 40, 64), (128, 33, 224, 32, 64), (64, 64, 0, 64, 64)])
def test_ring_buffers_with_poisoned_and_stale_columns(dh, tq, q_pos0, w, ring):
    """The keys of the linear sequence 0 .. q_pos0 + tq - 1 that the queries see sit at column j mod ring.  Every other column
    holds NaN in one run, and in a second the frame a real stream left there (the latest older position of that column; 0 where
    the stream has not been yet).  Nothing of them may reach the output: finite, within tolerance, bitwise the same."""
    b, heads = 2, 2
    hd = heads * dh
    tk = q_pos0 + tq
    gen = torch.Generator().manual_seed(tq + 7 * tk + dh)
    q = 0.7 * torch.randn(b, hd, tq, generator=gen)
    kv = 0.7 * torch.randn(b, 2 * hd, tk, generator=gen)
    slopes = oattn.alibi_slopes(heads)
    want = window_core(q.double(), kv.double(), slopes, heads, dh, dh ** 0.5, w, q_pos0=q_pos0)
    lo = max(0, q_pos0 - w + 1)
    assert tk - lo <= ring
    outs = []
    for stale in (False, True):
        buf = torch.full((b, 2 * hd, ring), float("nan"))
        if stale:
            buf.zero_()
            for j in range(lo):                     # ascending: the latest older frame of a column stays
                buf[..., j % ring] = kv[..., j]
        for j in range(lo, tk):
            buf[..., j % ring] = kv[..., j]
        outs.append(ops.attention_alibi_window(q.to(DEV), buf.to(DEV), slopes.to(DEV), heads, dh, dh ** 0.5, w, q_pos0=q_pos0,
                                               ring=ring))
    got = outs[0].cpu()
    assert tuple(got.shape) == (b, hd, tq) and bool(torch.isfinite(got).all())
    err, scale = max_abs(got, want), float(want.abs().max())
    print(f"window ring {(dh, tq, q_pos0, w, ring)}: max err {err:.3e}, max|o| {scale:.3e}")
    assert err < 3e-5 * max(1.0, scale)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("t", [64, 129, 199])
def test_the_window_is_exact(t):
    """Other finite values at the positions <= t - W -- the frames at least W behind every query >= t -- leave out[..., t:]
    bitwise unchanged: a masked probability is exactly 0, 0 * finite = 0, and a skipped block and a no-op block are both the
    identity on (m, l, o).  The causal op on the same tensors does change, so this test can fail.  Causality likewise:
    other values at the positions >= t leave out[..., :t] unchanged."""
    b, heads, dh, total, w = 2, 4, 64, 200, 37
    qkv, _, slopes = _qkv(b, heads, dh, total)
    far = qkv.clone()
    far[..., :t - w + 1] = 3.0 * torch.randn(b, 3 * heads * dh, t - w + 1, generator=torch.Generator().manual_seed(t))
    a, f, s = qkv.to(DEV), far.to(DEV), slopes.to(DEV)
    one = ops.attention_alibi_window(a, None, s, heads, dh, dh ** 0.5, w)
    two = ops.attention_alibi_window(f, None, s, heads, dh, dh ** 0.5, w)
    assert torch.equal(one[..., t:], two[..., t:])
    assert not torch.equal(one[..., :t], two[..., :t])
    c1 = ops.attention_alibi_causal(a, None, s, heads, dh, dh ** 0.5)
    c2 = ops.attention_alibi_causal(f, None, s, heads, dh, dh ** 0.5)
    assert not torch.equal(c1[..., t:], c2[..., t:])
    later = qkv.clone()
    later[..., t:] = 3.0 * torch.randn(b, 3 * heads * dh, total - t, generator=torch.Generator().manual_seed(t + 1))
    three = ops.attention_alibi_window(later.to(DEV), None, s, heads, dh, dh ** 0.5, w)
    assert torch.equal(one[..., :t], three[..., :t]) and not torch.equal(one[..., t:], three[..., t:])


@pytest.mark.parametrize("b,heads,dh,t,w", [(2, 8, 64, 130, 3), (1, 4, 16, 257, 100), (1, 2, 128, 65, 64), (1, 1, 8, 1, 1),
                                            (1, 5, 33, 64, 17)])
def test_window_backward_against_float64_autograd(b, heads, dh, t, w):
    qkv, dout, slopes = _qkv(b, heads, dh, t)
    hd = heads * dh
    qkv64 = qkv.double().requires_grad_()
    window_core(qkv64[:, :hd], qkv64[:, hd:], slopes, heads, dh, dh ** 0.5, w).backward(dout.double())
    qd, sd, dd = qkv.to(DEV), slopes.to(DEV), dout.to(DEV)
    out = ops.attention_alibi_window(qd, None, sd, heads, dh, dh ** 0.5, w)
    dqkv = ops.attention_alibi_window_backward(qd, sd, out, dd, heads, dh, dh ** 0.5, w)
    assert dqkv.shape == qkv.shape and bool(torch.isfinite(dqkv).all())
    for name, rows in (("dq", slice(0, hd)), ("dk", slice(hd, 2 * hd)), ("dv", slice(2 * hd, 3 * hd))):
        got, want = dqkv[:, rows].cpu(), qkv64.grad[:, rows]
        e_max, e_rms = max_abs(got, want), rms(got, want)
        s_max, s_rms = float(want.abs().max()), float(want.pow(2).mean().sqrt())
        print(f"window backward {(b, heads, dh, t, w)} {name}: max err {e_max:.3e} (max {s_max:.3e}), rms err {e_rms:.3e} (rms {s_rms:.3e})")
        assert e_max < 5e-5 * max(1.0, s_max) and e_rms < 1e-5 * max(1.0, s_rms), name
    assert torch.equal(dqkv, ops.attention_alibi_window_backward(qd, sd, out, dd, heads, dh, dh ** 0.5, w))   # deterministic: no atomics
    # dout nonzero at the queries [lo, hi) only: dq is exactly 0 outside [lo, hi), dk and dv outside [lo - W + 1, hi)
    lo, hi = t // 3, 2 * t // 3 + 1
    part = torch.zeros_like(dd)
    part[..., lo:hi] = dd[..., lo:hi]
    g = ops.attention_alibi_window_backward(qd, sd, out, part, heads, dh, dh ** 0.5, w).cpu()
    klo = max(0, lo - w + 1)
    dq, dk, dv = g[:, :hd], g[:, hd:2 * hd], g[:, 2 * hd:]
    for name, z, first in (("dq", dq, lo), ("dk", dk, klo), ("dv", dv, klo)):
        outside = torch.cat([z[..., :first], z[..., hi:]], dim=-1)
        assert outside.numel() == 0 or float(outside.abs().max()) == 0.0, name
    assert bool((dv[..., klo:hi].abs().amax(dim=(0, 1)) > 0).all())        # every key in the band is seen by a query with dout
    if w > 1:                                                               # W = 1: softmax over one key has no gradient
        assert bool((dk[..., klo:hi].abs().amax(dim=(0, 1)) > 0).all()) and bool((dq[..., lo:hi].abs().amax(dim=(0, 1)) > 0).all())


def test_window_refusals_launch_nothing():
    lib = _lib.load()
    b, heads, dh, t, w = 1, 2, 16, 37, 5
    hd = heads * dh
    qkv, dout, slopes = (z.to(DEV) for z in _qkv(b, heads, dh, t))
    out = ops.attention_alibi_window(qkv, None, slopes, heads, dh, 4.0, w)
    dqkv, fresh = torch.zeros_like(qkv), torch.zeros_like(out)
    need = lib.agx_attention_window_backward_workspace_bytes(b, heads, t)
    assert need == 2 * b * heads * t * 4
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    p = lambda z, off=0: ctypes.c_void_p(z.data_ptr() + 4 * off)   # noqa: E731
    s3 = 3 * hd * t
    bwd = lambda nbytes, d, win=w: lib.agx_attention_alibi_window_backward(   # noqa: E731
        p(qkv), p(qkv, hd * t), s3, s3, p(slopes), p(out), p(dout), p(dqkv), p(dqkv, hd * t), s3, s3, p(ws), nbytes, b, heads, d, t,
        win, 4.0, None)
    fwd = lambda d, pos, pitch, win=w, ring=0, sq=s3: lib.agx_attention_alibi_window(   # noqa: E731
        p(qkv), p(qkv, hd * t), sq, s3, pitch, p(slopes), p(fresh), b, heads, d, t, pos, win, ring, 4.0, None)
    assert bwd(need - 4, dh) == -3 and bwd(need, 129) == -5 and bwd(need, dh, 0) == -1
    assert fwd(129, 0, t) == -5 and fwd(dh, -1, t) == -1 and fwd(dh, 0, t - 1) == -1 and fwd(dh, 0, t, sq=hd * t - 1) == -1
    assert fwd(dh, 0, t, win=0) == -1 and fwd(dh, 0, t, ring=t - 1) == -1 and fwd(dh, 0, t, ring=t + 1) == -1
    torch.cuda.synchronize()
    assert float(dqkv.abs().max()) == 0.0 and float(fresh.abs().max()) == 0.0 and int(ws.max()) == 0     # nothing was launched
    assert bwd(need, dh) == 0 and fwd(dh, 0, t) == 0
    torch.cuda.synchronize()
    assert torch.equal(fresh, out) and float(dqkv.abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------- modules
DIM, HEADS, DH, CTX, W = 64, 4, 16, 50, 12
STREAM = 170                                  # more than 3 context_x
CHUNKS = (39, 1, 20, 39, 7, 33, 31)           # mixed, at most 39 = CTX - W + 1, wrapping the ring of 50 several times


@pytest.fixture(scope="module")
def block2():
    """The depth-2 windowed block, its inputs and the float64 checker's outputs and gradients, computed once."""
    sd = oattn.init_state_dict(DIM, HEADS, DH, depth=2, seed=131)
    gen = torch.Generator().manual_seed(132)
    x, w = torch.randn(2, DIM, CTX, generator=gen), torch.randn(2, DIM, CTX, generator=gen)
    long = torch.randn(2, DIM, STREAM, generator=gen)
    sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    x64 = x.double().requires_grad_()
    want = window_transformer(x64.transpose(1, 2), sd64, HEADS, W, depth=2).transpose(1, 2)
    (want * w.double()).sum().backward()
    with torch.no_grad():
        want_long = window_transformer(long.double().transpose(1, 2), sd64, HEADS, W, depth=2).transpose(1, 2)
    tf = Transformer(DIM, depth=2, heads=HEADS, head_dim=DH, context_x=CTX, causal=True, window=W)
    tf.load_state_dict(sd)
    return dict(tf=tf.to(DEV), sd=sd, x=x, w=w, long=long, want=want.detach(), want_long=want_long, dx=x64.grad,
                dparams={k: v.grad for k, v in sd64.items()})


def _scaled(want, tol=2e-5):
    return tol * max(1.0, float(want.abs().max()))


def _poisoned(tf, capacity=None):
    cache = tf.new_cache(2, capacity)
    for kv in cache.kv:
        kv.fill_(float("nan"))          # torch.empty promises nothing: make the unwritten ring as bad as it can be
    return cache


def _chunked(tf, cache, x, sizes):
    outs, at = [], 0
    start = cache.length
    with torch.no_grad():
        for n in sizes:
            outs.append(tf.run_bct(x[..., at:at + n].contiguous(), cache=cache))
            at += n
            assert cache.length == start + at
    return torch.cat(outs, dim=-1)


def test_depth2_eval_and_it_is_not_the_causal_block(block2):
    tf, x, want = block2["tf"].eval(), block2["x"], block2["want"]
    with torch.no_grad():
        out = tf.run_bct(x.to(DEV))
        assert torch.equal(tf(x.to(DEV).transpose(1, 2).contiguous()), out.transpose(1, 2))
    err = max_abs(out.cpu(), want)
    print(f"window depth-2 block: err {err:.3e}, max|y| {float(want.abs().max()):.3e}")
    assert err < _scaled(want)
    causal = Transformer(DIM, depth=2, heads=HEADS, head_dim=DH, context_x=CTX, causal=True)
    causal.load_state_dict(block2["sd"])
    with torch.no_grad():
        apart = max_abs(causal.to(DEV).eval().run_bct(x.to(DEV)).cpu(), want)
    print(f"window depth-2 block: the causal model on the same weights is {apart:.3e} away")
    assert apart > 1e-3


def test_depth2_training_against_float64_autograd(block2):
    tf, x, w = block2["tf"].train(), block2["x"], block2["w"]
    for p in tf.parameters():
        p.grad = None
    xd = x.to(DEV).requires_grad_()
    out = tf.run_bct(xd)
    (out * w.to(DEV)).sum().backward()
    assert max_abs(out.detach().cpu(), block2["want"]) < _scaled(block2["want"])
    err, scale = max_abs(xd.grad.cpu(), block2["dx"]), float(block2["dx"].abs().max())
    print(f"window training dx: err {err:.3e}, max|ref| {scale:.3e}")
    assert err < 2e-4 * max(1.0, scale)
    params = dict(tf.named_parameters())
    assert list(params) == list(block2["sd"])
    for name, p in params.items():
        assert p.grad is not None, name
        ref = block2["dparams"][name]
        err, scale = max_abs(p.grad.cpu(), ref), float(ref.abs().max())
        print(f"window training {name}: err {err:.3e}, max|ref| {scale:.3e}")
        assert err < 5e-4 * max(1.0, scale), name


def test_every_chunking_equals_the_uncached_run(block2):
    """Key blocks are aligned to absolute positions and a block a row sees nothing of is the exact identity, so a query's result
    does not depend on the chunk that delivered it.  A call of n frames needs n + min(W - 1, length) <= capacity: at the start
    of a stream the default ring of 50 takes all 50 frames, later chunks of up to 39."""
    tf, x, want = block2["tf"].eval(), block2["x"].to(DEV), block2["want"]
    with torch.no_grad():
        full = tf.run_bct(x)
    assert tf.new_cache(2).capacity == CTX
    runs = {"(1 x 50)": _chunked(tf, _poisoned(tf), x, [1] * CTX), "(7, 1, 30, 12)": _chunked(tf, _poisoned(tf), x, [7, 1, 30, 12]),
            "(50)": _chunked(tf, _poisoned(tf), x, [CTX])}
    for name, got in runs.items():
        err = max_abs(got.cpu(), want)
        print(f"ring cache {name}: err {err:.3e} against the float64 checker, bitwise the uncached run: {torch.equal(got, full)}")
        assert bool(torch.isfinite(got).all()) and err < _scaled(want), name
        assert torch.equal(got, full), name
    cache = _poisoned(tf)
    _chunked(tf, cache, x, [7, 1, 30])
    before = [kv.clone() for kv in cache.kv]
    with torch.no_grad(), pytest.raises(AgxError, match=r"40 new frames \+ the 11 cached frames their window reaches exceed the "
                                                        r"ring's capacity 50"):
        tf.run_bct(x[..., :40].contiguous(), cache=cache)            # 40 + 11 > 50
    assert cache.length == 38
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, cache.kv))     # NaNs included


def test_a_stream_longer_than_the_context(block2):
    tf, long, want = block2["tf"].eval(), block2["long"].to(DEV), block2["want_long"]
    assert sum(CHUNKS) == STREAM > 3 * CTX and max(CHUNKS) == CTX - W + 1
    cache = _poisoned(tf)
    got = _chunked(tf, cache, long, CHUNKS)
    assert cache.length == STREAM
    err = max_abs(got.cpu(), want)
    print(f"ring cache, {STREAM} frames in chunks {CHUNKS}: err {err:.3e} against the float64 checker, max|y| {float(want.abs().max()):.3e}")
    assert bool(torch.isfinite(got).all()) and err < _scaled(want)
    cache.reset()
    assert torch.equal(_chunked(tf, cache, long, [1] * STREAM), got)         # frame by frame: the same bits
    with torch.no_grad(), pytest.raises(AgxError, match=r"sequence length 170 exceeds the ALiBi context 50 \(the reference fails "
                                                        r"here too, transformers.py:88-93\)"):
        tf.run_bct(long)


def test_positions_beyond_int32_and_the_bottleneck(block2):
    tf, long = block2["tf"].eval(), block2["long"].to(DEV)
    cache = _poisoned(tf)
    _chunked(tf, cache, long, [39, 21])
    far = TransformerCache([kv.clone() for kv in cache.kv], cache.batch, cache.capacity, cache.window)
    far.length = cache.length + 1600 * 2 ** 21          # a multiple of lcm(64, 50) = 1600, beyond 2^31: the same columns and blocks
    third = copy.copy(cache)
    third.kv = [kv.clone() for kv in cache.kv]
    nxt = long[..., 60:77].contiguous()
    with torch.no_grad():
        a = tf.run_bct(nxt, cache=cache)
        b = tf.run_bct(nxt, cache=far)
        c, idx, loss = TransformerBottleneck(tf)(nxt.transpose(1, 2).contiguous(), cache=third)
    assert cache.length == 77 and far.length == 77 + 1600 * 2 ** 21 and third.length == 77
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert torch.equal(c, a.transpose(1, 2)) and idx is None and float(loss) == 0.0
    err = max_abs(a.cpu(), block2["want_long"][..., 60:77])
    assert err < _scaled(block2["want_long"])
