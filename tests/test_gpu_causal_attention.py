"""Causal ALiBi self-attention on the GPU (csrc/attention_causal.hip): the op against the float64 definition of
``tests/causal_attention_ref.py`` -- forward, cached shapes on a poisoned buffer, exact causality, backward -- and the modules
(``causal=True``, the key/value cache) against the float64 checker.

Tolerances are the ones the suite states for the same arithmetic (tests/test_gpu_cross_attention.py): 3e-5 of max(1, max|o|)
for the fp32 flash forward, 5e-5 / 1e-5 (max / rms) for the split backward, 1e-5 / 2e-5 absolute for the attention sub-block
and the block at the g9 sizes with the g9 weights and inputs, 2e-5 of max(1, max|y|) for a block on other values
(tests/test_gpu_blocks.py), 2e-4 / 5e-4 for input / parameter gradients of a block (tests/test_gpu_training.py)."""
import ctypes

import pytest
import torch

from audio_generation_amd import _lib, ops
from audio_generation_amd._lib import AgxError
from audio_generation_amd.transformers import Attention, Transformer, TransformerBottleneck
from oracle import attention as oattn
from tests.causal_attention_ref import causal_attention, causal_core, causal_transformer
from tests.helpers import load_npz, max_abs, rms, sub_sd

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _qkv(b, heads, dh, t, seed=0):
    gen = torch.Generator().manual_seed(1000 * t + dh + seed)
    qkv = 0.7 * torch.randn(b, 3 * heads * dh, t, generator=gen)
    dout = torch.randn(b, heads * dh, t, generator=gen)
    return qkv, dout, oattn.alibi_slopes(heads)


def _core64(qkv, slopes, heads, dh, **kw):
    hd = heads * dh
    return causal_core(qkv[:, :hd].double(), qkv[:, hd:].double(), slopes, heads, dh, dh ** 0.5, **kw)


# the three head-dim tiles, a 64-key boundary from both sides, a 128-query boundary with two and three workgroups
@pytest.mark.parametrize("b,heads,dh,t", [(2, 1, 8, 1), (2, 3, 16, 37), (1, 2, 64, 64), (1, 2, 64, 65), (2, 8, 64, 130),
                                          (1, 2, 100, 257), (1, 2, 128, 300)])
def test_causal_forward_against_the_definition(b, heads, dh, t):
    qkv, _, slopes = _qkv(b, heads, dh, t)
    want = _core64(qkv, slopes, heads, dh)
    got = ops.attention_alibi_causal(qkv.to(DEV), None, slopes.to(DEV), heads, dh, dh ** 0.5)
    assert tuple(got.shape) == (b, heads * dh, t)
    err, scale = max_abs(got.cpu(), want), float(want.abs().max())
    print(f"causal forward {(b, heads, dh, t)}: max err {err:.3e}, max|o| {scale:.3e}")
    assert err < 3e-5 * max(1.0, scale)


@pytest.mark.parametrize("dh,tq,tk,q_pos0,pitch", [(64, 1, 70, 69, 70), (16, 5, 130, 125, 192), (128, 33, 257, 224, 320),
                                                   (64, 64, 64, 0, 64)])
def test_cached_shapes_on_a_buffer_with_a_poisoned_tail(dh, tq, tk, q_pos0, pitch):
    """The kv buffer is a cache of pitch ``pitch`` whose columns >= tk were never written: NaN here.  Nothing of them may
    reach the output -- it is finite, within tolerance, and bitwise what the zeroed tail gives."""
    b, heads = 2, 2
    hd = heads * dh
    gen = torch.Generator().manual_seed(tq + 7 * tk + dh)
    q = 0.7 * torch.randn(b, hd, tq, generator=gen)
    kv = 0.7 * torch.randn(b, 2 * hd, tk, generator=gen)
    slopes = oattn.alibi_slopes(heads)
    want = causal_core(q.double(), kv.double(), slopes, heads, dh, dh ** 0.5, q_pos0=q_pos0)
    outs = []
    for tail in (float("nan"), 0.0):
        buf = torch.full((b, 2 * hd, pitch), tail)
        buf[..., :tk] = kv
        outs.append(ops.attention_alibi_causal(q.to(DEV), buf.to(DEV), slopes.to(DEV), heads, dh, dh ** 0.5, q_pos0=q_pos0, tk=tk))
    got = outs[0].cpu()
    assert tuple(got.shape) == (b, hd, tq) and bool(torch.isfinite(got).all())
    err, scale = max_abs(got, want), float(want.abs().max())
    print(f"causal cached {(dh, tq, tk, q_pos0, pitch)}: max err {err:.3e}, max|o| {scale:.3e}")
    assert err < 3e-5 * max(1.0, scale)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("t", [1, 63, 64, 129])
def test_causality_is_exact(t):
    """Other finite values at the positions >= t leave out[..., :t] bitwise unchanged: a masked probability is exactly 0,
    0 * finite = 0, and a skipped block and a no-op block are both the identity on (m, l, o).  The symmetric kernel on the same
    tensors does change, so this test can fail."""
    b, heads, dh, total = 2, 4, 64, 200
    qkv, _, slopes = _qkv(b, heads, dh, total)
    other = qkv.clone()
    other[..., t:] = 3.0 * torch.randn(b, 3 * heads * dh, total - t, generator=torch.Generator().manual_seed(t))
    a, o, s = qkv.to(DEV), other.to(DEV), slopes.to(DEV)
    one = ops.attention_alibi_causal(a, None, s, heads, dh, dh ** 0.5)
    two = ops.attention_alibi_causal(o, None, s, heads, dh, dh ** 0.5)
    assert torch.equal(one[..., :t], two[..., :t])
    assert not torch.equal(one[..., t:], two[..., t:])
    sym1 = ops.attention_alibi(a, s, heads, dh, dh ** 0.5, flash=True)
    sym2 = ops.attention_alibi(o, s, heads, dh, dh ** 0.5, flash=True)
    assert not torch.equal(sym1[..., :t], sym2[..., :t])


@pytest.mark.parametrize("b,heads,dh,t", [(2, 8, 64, 130), (1, 4, 16, 257), (1, 2, 128, 65), (1, 1, 8, 1), (1, 5, 33, 64)])
def test_causal_backward_against_float64_autograd(b, heads, dh, t):
    qkv, dout, slopes = _qkv(b, heads, dh, t)
    hd = heads * dh
    qkv64 = qkv.double().requires_grad_()
    causal_core(qkv64[:, :hd], qkv64[:, hd:], slopes, heads, dh, dh ** 0.5).backward(dout.double())
    qd, sd, dd = qkv.to(DEV), slopes.to(DEV), dout.to(DEV)
    out = ops.attention_alibi_causal(qd, None, sd, heads, dh, dh ** 0.5)
    dqkv = ops.attention_alibi_causal_backward(qd, sd, out, dd, heads, dh, dh ** 0.5)
    assert dqkv.shape == qkv.shape
    for name, rows in (("dq", slice(0, hd)), ("dk", slice(hd, 2 * hd)), ("dv", slice(2 * hd, 3 * hd))):
        got, want = dqkv[:, rows].cpu(), qkv64.grad[:, rows]
        e_max, e_rms = max_abs(got, want), rms(got, want)
        s_max, s_rms = float(want.abs().max()), float(want.pow(2).mean().sqrt())
        print(f"causal backward {(b, heads, dh, t)} {name}: max err {e_max:.3e} (max {s_max:.3e}), rms err {e_rms:.3e} (rms {s_rms:.3e})")
        assert e_max < 5e-5 * max(1.0, s_max) and e_rms < 1e-5 * max(1.0, s_rms), name
    assert torch.equal(dqkv, ops.attention_alibi_causal_backward(qd, sd, out, dd, heads, dh, dh ** 0.5))   # deterministic: no atomics
    # dout nonzero at the queries < cut only: nothing flows to a query, key or value at a position >= cut
    cut = t // 2
    part = dd.clone()
    part[..., cut:] = 0.0
    g = ops.attention_alibi_causal_backward(qd, sd, out, part, heads, dh, dh ** 0.5)
    assert float(g[..., cut:].abs().max()) == 0.0 if cut < t else True
    if cut > 0:
        assert float(g[..., :cut].abs().max()) > 0.0


def test_causal_refusals_launch_nothing():
    lib = _lib.load()
    b, heads, dh, t = 1, 2, 16, 37
    hd = heads * dh
    qkv, dout, slopes = (z.to(DEV) for z in _qkv(b, heads, dh, t))
    out = ops.attention_alibi_causal(qkv, None, slopes, heads, dh, 4.0)
    dqkv, fresh = torch.zeros_like(qkv), torch.zeros_like(out)
    need = lib.agx_attention_causal_backward_workspace_bytes(b, heads, t)
    assert need == 2 * b * heads * t * 4
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    p = lambda z, off=0: ctypes.c_void_p(z.data_ptr() + 4 * off)   # noqa: E731
    s3 = 3 * hd * t
    bwd = lambda nbytes, d: lib.agx_attention_alibi_causal_backward(   # noqa: E731
        p(qkv), p(qkv, hd * t), s3, s3, p(slopes), p(out), p(dout), p(dqkv), p(dqkv, hd * t), s3, s3, p(ws), nbytes, b, heads, d, t,
        4.0, None)
    fwd = lambda d, pos, pitch, sq=s3: lib.agx_attention_alibi_causal(   # noqa: E731
        p(qkv), p(qkv, hd * t), sq, s3, pitch, p(slopes), p(fresh), b, heads, d, t, t, pos, 4.0, None)
    assert bwd(need - 4, dh) == -3 and bwd(need, 129) == -5
    assert fwd(129, 0, t) == -5 and fwd(dh, -1, t) == -1 and fwd(dh, 0, t - 1) == -1 and fwd(dh, 0, t, hd * t - 1) == -1
    torch.cuda.synchronize()
    assert float(dqkv.abs().max()) == 0.0 and float(fresh.abs().max()) == 0.0 and int(ws.max()) == 0     # nothing was launched
    assert bwd(need, dh) == 0 and fwd(dh, 0, t) == 0
    torch.cuda.synchronize()
    assert torch.equal(fresh, out) and float(dqkv.abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------- modules
DIM, HEADS, DH, CTX = 64, 4, 16, 50      # the sizes of the g9 module tests


@pytest.fixture(scope="module")
def g9():
    return load_npz("g9_cross_attention.npz")


def _scaled(want, tol=2e-5):
    return tol * max(1.0, float(want.abs().max()))


def test_causal_modules_at_the_g9_sizes(g9):
    """The g9 weights and input of the square model (a checkpoint loads into the causal modules as it is): the sub-block and
    the block against the float64 checker at the tolerances the g9 tests use for these magnitudes."""
    sd = sub_sd(g9, "square50/sd/")
    x = torch.from_numpy(g9["square50/full/x"])
    assert tuple(x.shape) == (2, CTX, DIM)
    sd64 = {k: v.double() for k, v in sd.items()}
    tf = Transformer(DIM, depth=1, heads=HEADS, head_dim=DH, context_x=CTX, causal=True)
    tf.load_state_dict(sd)
    tf = tf.to(DEV).eval()
    att = Attention(DIM, dim_head=DH, n_heads=HEADS, context_x=CTX, causal=True)
    att.load_state_dict({k[len("layers.0.0."):]: v for k, v in sd.items() if k.startswith("layers.0.0.")})
    att = att.to(DEV).eval()
    xd = x.to(DEV)
    with torch.no_grad():
        sub, out, (bott, idx, loss) = att(xd), tf(xd), TransformerBottleneck(tf)(xd)
        out_bct = tf.run_bct(xd.transpose(1, 2).contiguous())
        sub_bct = att.run_bct(xd.transpose(1, 2).contiguous())
    want_sub = causal_attention(x.double(), sd64, "layers.0.0.", HEADS)
    want = causal_transformer(x.double(), sd64, HEADS, depth=1)
    e_sub, e_out = max_abs(sub.cpu(), want_sub), max_abs(out.cpu(), want)
    print(f"causal modules, g9 sizes: sub-block err {e_sub:.3e}, block err {e_out:.3e}")
    assert e_sub < 1e-5 and e_out < 2e-5
    assert torch.equal(out, out_bct.transpose(1, 2)) and torch.equal(sub, sub_bct.transpose(1, 2))
    assert torch.equal(bott, out) and idx is None and float(loss) == 0.0
    # it is not the symmetric block
    sym = Transformer(DIM, depth=1, heads=HEADS, head_dim=DH, context_x=CTX)
    sym.load_state_dict(sd)
    with torch.no_grad():
        assert max_abs(sym.to(DEV).eval()(xd).cpu(), want) > 1e-3


@pytest.fixture(scope="module")
def block2():
    """The depth-2 causal block, its input and the float64 checker's output and gradients, computed once."""
    sd = oattn.init_state_dict(DIM, HEADS, DH, depth=2, seed=131)
    gen = torch.Generator().manual_seed(132)
    x, w = torch.randn(2, DIM, CTX, generator=gen), torch.randn(2, DIM, CTX, generator=gen)
    sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    x64 = x.double().requires_grad_()
    want = causal_transformer(x64.transpose(1, 2), sd64, HEADS, depth=2).transpose(1, 2)
    (want * w.double()).sum().backward()
    tf = Transformer(DIM, depth=2, heads=HEADS, head_dim=DH, context_x=CTX, causal=True)
    tf.load_state_dict(sd)
    return dict(tf=tf.to(DEV), sd=sd, x=x, w=w, want=want.detach(), dx=x64.grad, dparams={k: v.grad for k, v in sd64.items()})


def test_depth2_eval_and_the_prefix_property(block2):
    tf, x, want = block2["tf"].eval(), block2["x"], block2["want"]
    with torch.no_grad():
        out = tf.run_bct(x.to(DEV))
        assert torch.equal(tf(x.to(DEV).transpose(1, 2).contiguous()), out.transpose(1, 2))
    err = max_abs(out.cpu(), want)
    print(f"causal depth-2 block: err {err:.3e}, max|y| {float(want.abs().max()):.3e}")
    assert err < _scaled(want)
    for t in (1, 17, 49):
        other = x.clone()
        other[..., t:] = 10.0 * torch.randn(2, DIM, CTX - t, generator=torch.Generator().manual_seed(t))
        with torch.no_grad():
            got = tf.run_bct(other.to(DEV))
        e = max_abs(got[..., :t].cpu(), want[..., :t])       # a leak of the replaced frames would show at O(0.1)
        print(f"causal prefix t={t}: err {e:.3e} against the unperturbed checker, bitwise {torch.equal(got[..., :t], out[..., :t])}")
        assert e < _scaled(want)


def test_depth2_training_against_float64_autograd(block2):
    tf, x, w = block2["tf"].train(), block2["x"], block2["w"]
    for p in tf.parameters():
        p.grad = None
    xd = x.to(DEV).requires_grad_()
    out = tf.run_bct(xd)
    (out * w.to(DEV)).sum().backward()
    assert max_abs(out.detach().cpu(), block2["want"]) < _scaled(block2["want"])
    err, scale = max_abs(xd.grad.cpu(), block2["dx"]), float(block2["dx"].abs().max())
    print(f"causal training dx: err {err:.3e}, max|ref| {scale:.3e}")
    assert err < 2e-4 * max(1.0, scale)
    params = dict(tf.named_parameters())
    assert list(params) == list(block2["sd"])
    for name, p in params.items():
        assert p.grad is not None, name
        ref = block2["dparams"][name]
        err, scale = max_abs(p.grad.cpu(), ref), float(ref.abs().max())
        print(f"causal training {name}: err {err:.3e}, max|ref| {scale:.3e}")
        assert err < 5e-4 * max(1.0, scale), name


def test_the_cache_equals_the_full_run(block2):
    tf, x, want = block2["tf"].eval(), block2["x"].to(DEV), block2["want"]
    cache = tf.new_cache(2)
    assert cache.capacity == CTX and all(tuple(kv.shape) == (2, 2 * HEADS * DH, CTX) for kv in cache.kv)
    for kv in cache.kv:
        kv.fill_(float("nan"))          # torch.empty promises nothing: make the unwritten tail as bad as it can be

    def chunked(sizes):
        cache.reset()
        outs, at = [], 0
        with torch.no_grad():
            for n in sizes:
                outs.append(tf.run_bct(x[..., at:at + n].contiguous(), cache=cache))
                at += n
                assert cache.length == at
        return torch.cat(outs, dim=-1)

    with torch.no_grad():
        full = tf.run_bct(x)
    runs = {"(50)": chunked([CTX]), "(1 x 50)": chunked([1] * CTX), "(7, 1, 30, 12)": chunked([7, 1, 30, 12])}
    for name, got in runs.items():
        err = max_abs(got.cpu(), want)
        print(f"cache {name}: err {err:.3e} against the float64 checker")
        assert bool(torch.isfinite(got).all()) and err < _scaled(want), name
    assert torch.equal(runs["(50)"], full)
    print("cache: max difference between chunkings", max(max_abs(a.cpu(), b.cpu()) for a in runs.values() for b in runs.values()))
    assert torch.equal(chunked([7, 1, 30, 12]), runs["(7, 1, 30, 12)"])       # reset() and a rerun reproduce bitwise
    with torch.no_grad(), pytest.raises(AgxError, match="exceed"):               # cache.length is 50 = context_x
        tf.run_bct(x[..., :1].contiguous(), cache=cache)
    assert cache.length == CTX
    with torch.no_grad():                                                         # the reference layout takes the cache too
        cache.reset()
        got = tf(x.transpose(1, 2).contiguous(), cache=cache)
    assert torch.equal(got, full.transpose(1, 2)) and cache.length == CTX
