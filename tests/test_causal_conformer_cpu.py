"""The causal Conformer on the host: the float64 restatement of ``tests/causal_conformer_ref.py`` pinned to a float64 composition
of ``F.pad(g, (K - 1, 0))`` + ``F.conv1d(groups=C)`` under autograd (gradients included, 1e-12 relative), its chunked form and
its causality; every error return of the four C entry points (host pointers: nothing launches); and the surface of the causal
modules: state dicts, caches, refusals.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from audio_generation_amd import _lib, ops
from audio_generation_amd._lib import AgxError
from audio_generation_amd.transformers import (ConformerBlock, ConformerCache, ConformerConvBlock, ConformerStreamCache)
from tests import causal_conformer_ref as cref

OK, BAD_SHAPE, NULL_POINTER, WORKSPACE = 0, -1, -2, -3
MAX_K, MAX_STEP = ops.CONFORMER_MAX_K, ops.CONFORMER_MAX_STEP


@pytest.fixture(scope="module")
def lib():
    from audio_generation_amd import build
    build.build()
    return _lib.load()


def _close(got, want, tol, what):
    err, scale = float((got - want).abs().max()) if got.numel() else 0.0, float(want.abs().max()) if want.numel() else 0.0
    print(f"{what}: err {err:.3e}, max|ref| {scale:.3e}")
    assert got.shape == want.shape and err <= tol * max(1.0, scale), what


def _rand(k, b=3, c=5, t=11, seed=0):
    gen = torch.Generator().manual_seed(seed + k)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    return r(b, 2 * c, t), r(c, 1, k), r(c), r(b, c, t), r(b, c, k - 1)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("k", [1, 2, 4, 17, 31, 64])
@pytest.mark.parametrize("t", [1, 3, 37])
def test_the_restatement_is_autograds(k, t):
    c = 5
    u, w, bias, dz, hist = _rand(k, c=c, t=t)
    u, w, bias = (v.requires_grad_() for v in (u, w, bias))
    z = F.conv1d(F.pad(F.glu(u, dim=-2), (k - 1, 0)), w, bias, groups=c)
    (z * dz).sum().backward()
    ud, wd, bd = u.detach(), w.detach(), bias.detach()
    _close(cref.glu_dwconv(ud, wd, bd), z.detach(), 1e-12, "z")
    du, dw, dbias = cref.glu_dwconv_backward(dz, ud, wd)
    _close(du, u.grad, 1e-12, "du")
    _close(dw, w.grad.reshape(c, k), 1e-12, "dw")
    _close(dbias, bias.grad, 1e-12, "dbias")
    # with a history: the conv of [hist | g] without padding
    z_h = F.conv1d(torch.cat([hist, F.glu(ud, dim=-2)], dim=-1), wd, bd, groups=c)
    _close(cref.glu_dwconv(ud, wd, bd, hist), z_h, 1e-12, "z (hist)")
    _close(cref.glu_dwconv(ud, wd, bd, torch.zeros_like(hist)), z.detach(), 1e-12, "z (zero hist)")
    for bound in (cref.bound_z(ud, wd, bd), cref.bound_z(ud, wd, bd, hist), *cref.bound_conv_backward(dz, ud, wd)):
        # a tap that only ever meets the zero padding (T < K - 1) has an exact 0 for its dw, and the bound says so
        assert bool(torch.isfinite(bound).all()) and float(bound.min()) >= 0.0 and 0.0 < float(bound.max()) < 1e-3


@pytest.mark.parametrize("k", [1, 2, 17])
def test_chunked_restatement_is_the_whole_one(k):
    u, w, bias, _, _ = _rand(k, t=40)
    whole = cref.glu_dwconv(u, w, bias)
    hist, outs, at = None, [], 0
    for n in (1, 3, 1, 16, 2, 17):
        chunk = u[..., at:at + n]
        outs.append(cref.glu_dwconv(chunk, w, bias, hist))
        hist = cref.next_hist(chunk, k, hist)
        at += n
    assert at == 40
    _close(torch.cat(outs, -1), whole, 1e-13, "chunked")
    _close(hist, cref.glu(u)[..., 40 - (k - 1):], 1e-15, "hist")    # torch's vectorised float64 sigmoid differs by an ulp with the slice


def test_the_restatement_is_causal():
    k, t0 = 17, 20
    u, w, bias, dz, _ = _rand(k, t=37)
    u2 = u.clone()
    u2[..., t0 + 1:] += 1.0
    assert torch.equal(cref.glu_dwconv(u, w, bias)[..., :t0 + 1], cref.glu_dwconv(u2, w, bias)[..., :t0 + 1])
    assert not torch.equal(cref.glu_dwconv(u, w, bias)[..., t0 + 1], cref.glu_dwconv(u2, w, bias)[..., t0 + 1])
    dz2 = dz.clone()
    dz2[..., :t0] += 1.0           # the gradient runs the other way: dg at >= t0 sees no dz before t0
    c = w.shape[0]
    assert torch.equal(cref.correlate(dz, w.reshape(c, k))[..., t0:], cref.correlate(dz2, w.reshape(c, k))[..., t0:])


def test_the_step_kernels_reciprocal_quotient_is_exact_over_its_domain():
    """``quot(i, inv) = int((float(i) + 0.5f) * inv)`` of ``csrc/conformer.hip`` with ``inv = 1.f / float(d)``, restated in float32:
    equal to ``i // d`` for every divisor the kernels use (n, K - 1, K: 1 <= d <= 64) and every i below 2^15.  The kernels' largest
    index is 256 rows x 64 = 16384 elements, and a workgroup holds at most 256 rows: both inside the checked domain."""
    assert 256 * max(MAX_K, MAX_STEP) <= 2 ** 15 and MAX_K <= 64 and MAX_STEP <= 64
    i = torch.arange(2 ** 15, dtype=torch.int32)
    for d in range(1, 65):
        inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(d), dtype=torch.float32)
        got = ((i.to(torch.float32) + torch.tensor(0.5, dtype=torch.float32)) * inv).to(torch.int32)      # float -> int truncates, as in C
        assert torch.equal(got, torch.div(i, d, rounding_mode="floor").to(torch.int32)), d


# ------------------------------------------------------------------------------------------------ the C entry points
def test_entry_points_validate_on_the_host(lib):
    buf = ctypes.create_string_buffer(64)          # never dereferenced: every call below is refused or empty
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd, bwd, step, upd = (lib.agx_glu_dwconv_causal_forward, lib.agx_glu_dwconv_causal_backward, lib.agx_glu_dwconv_step,
                           lib.agx_glu_hist_update)
    ws_bytes = lib.agx_glu_dwconv_causal_backward_workspace_bytes
    big = 2 ** 20
    for b, c, t, k in ((0, 2, 8, 3), (1, 0, 8, 3), (1, 2, 0, 3), (-1, 2, 8, 3), (1, 2, 8, 0), (1, 2, 8, MAX_K + 1), (big, big, 1, 3),
                       (big, 4096, 1025, 3)):
        assert fwd(p, p, p, None, None, None, None, 1e-5, p, p, b, c, t, k, None) == BAD_SHAPE, (b, c, t, k)
        assert bwd(p, p, p, p, p, p, p, 1 << 30, b, c, t, k, None) == BAD_SHAPE
        assert ws_bytes(b, c, t, k) == 0
        assert upd(p, p, b, c, t, k, None) == BAD_SHAPE
    assert b"grid" in lib.agx_last_error()
    # the step: B, C, then n outside [1, MAX_STEP], then K outside [1, MAX_K], then the grid
    for b, c, n, k in ((0, 2, 1, 3), (1, 0, 1, 3), (1, 2, 0, 3), (1, 2, -1, 3), (1, 2, MAX_STEP + 1, 3), (1, 2, 1, 0), (1, 2, 1, MAX_K + 1),
                       (1, 2, 1, 65), (2 ** 30, 2 ** 30, 64, 3)):
        assert step(p, p, p, p, p, p, p, 1e-5, p, p, b, c, n, k, None) == BAD_SHAPE, (b, c, n, k)
    assert step(p, p, p, p, p, p, p, 1e-5, p, p, 1, 2, MAX_STEP + 1, 3, None) == BAD_SHAPE and b"outside [1, 64]" in lib.agx_last_error()
    # NULL pointers
    assert fwd(None, p, p, None, None, None, None, 1e-5, None, p, 1, 2, 8, 3, None) == NULL_POINTER
    assert fwd(p, p, p, None, None, None, None, 1e-5, p, None, 1, 2, 8, 3, None) == NULL_POINTER
    assert fwd(p, p, p, p, None, None, None, 1e-5, None, p, 1, 2, 8, 3, None) == NULL_POINTER        # statistics come together
    assert bwd(p, p, p, p, p, None, p, 1 << 20, 1, 2, 8, 3, None) == NULL_POINTER                    # dw without dbias
    assert bwd(None, p, p, p, None, None, None, 0, 1, 2, 8, 3, None) == NULL_POINTER
    assert bwd(p, p, p, None, None, None, None, 0, 1, 2, 8, 3, None) == OK                           # nothing asked for
    for missing in range(10):                      # u, w, bias, gamma, beta, mean, var | hist, out
        args = [p] * 7 + [1e-5, p, p]
        if missing == 7:
            continue                               # eps
        args[missing] = None
        assert step(*args, 1, 2, 1, 3, None) == NULL_POINTER, missing
    assert step(p, p, p, p, p, p, p, 1e-5, None, p, 1, 2, 1, 3, None) == NULL_POINTER                # NULL hist with K > 1
    assert upd(None, p, 1, 2, 8, 3, None) == NULL_POINTER and upd(p, None, 1, 2, 8, 3, None) == NULL_POINTER
    assert upd(None, None, 1, 2, 8, 1, None) == OK                                                   # K == 1: nothing to do
    # the workspace
    tile = cref.TILE
    assert ws_bytes(3, 5, tile, 17) == 4 * 15 * 18 == lib.agx_glu_dwconv_backward_workspace_bytes(3, 5, tile, 17)
    assert ws_bytes(3, 5, tile + 1, 4) == 4 * 30 * 5
    assert bwd(p, p, p, p, p, p, p, 4 * 15 * 18 - 1, 3, 5, tile, 17, None) == WORKSPACE and b"workspace" in lib.agx_last_error()
    assert bwd(p, p, p, p, p, p, None, 1 << 20, 3, 5, tile, 17, None) == WORKSPACE
    assert MAX_STEP == cref.MAX_STEP == 64 and MAX_K == 64


def test_wrappers_refuse_on_the_host(monkeypatch):
    z = torch.zeros
    for call in (lambda: ops.glu_dwconv_causal(z(1, 4, 8), z(2, 1, 3), z(2)), lambda: ops.glu_dwconv_causal_backward(z(1, 2, 8), z(1, 4, 8), z(2, 1, 3)),
                 lambda: ops.glu_dwconv_step(z(1, 4, 1), z(2, 1, 3), z(2), (z(2),) * 4, z(1, 2, 2)), lambda: ops.glu_hist_update(z(1, 4, 8), z(1, 2, 2))):
        with pytest.raises(AgxError, match="MI355X only"):
            call()
    monkeypatch.setattr(ops, "_need_gpu", lambda *tensors: None)
    bn = (z(2),) * 4
    with pytest.raises(AgxError, match="2 C, T"):
        ops.glu_dwconv_causal(z(1, 3, 8), z(1, 1, 3), z(1))
    with pytest.raises(AgxError, match="hist must be"):
        ops.glu_dwconv_causal(z(1, 4, 8), z(2, 1, 3), z(2), hist=z(1, 2, 3))
    with pytest.raises(AgxError, match="dz is"):
        ops.glu_dwconv_causal_backward(z(1, 2, 7), z(1, 4, 8), z(2, 1, 3))
    with pytest.raises(AgxError, match=r"outside \[1, 64\]"):
        ops.glu_dwconv_step(z(1, 4, MAX_STEP + 1), z(2, 1, 3), z(2), bn, z(1, 2, 2))
    with pytest.raises(AgxError, match=r"outside \[1, 64\]"):
        ops.glu_dwconv_step(z(1, 4, 0), z(2, 1, 3), z(2), bn, z(1, 2, 2))
    with pytest.raises(AgxError, match="eval form"):
        ops.glu_dwconv_step(z(1, 4, 1), z(2, 1, 3), z(2), None, z(1, 2, 2))
    with pytest.raises(AgxError, match="needs hist"):
        ops.glu_dwconv_step(z(1, 4, 1), z(2, 1, 3), z(2), bn, None)
    with pytest.raises(AgxError, match="hist must be"):
        ops.glu_dwconv_step(z(1, 4, 1), z(2, 1, 3), z(2), bn, z(2, 2, 2))
    with pytest.raises(AgxError, match="hist must be"):
        ops.glu_hist_update(z(1, 4, 8), z(1, 3, 2))
    with pytest.raises(AgxError, match="hist is"):
        ops.glu_hist_update(z(1, 4, 8), z(1, 2, MAX_K))


# ------------------------------------------------------------------------------------------------ the modules
def test_state_dicts_of_causal_and_non_causal_blocks_are_equal():
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}
    for k in (1, 4, 17):
        a, b = ConformerConvBlock(8, kernel_size=k), ConformerConvBlock(8, kernel_size=k, causal=True)
        assert shapes(a) == shapes(b) and list(a.state_dict()) == list(b.state_dict())
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
        b.load_state_dict(a.state_dict())
        assert b.net[3].padding == (0,) and b.net[3].groups == 8 and b.net[3].kernel_size == (k,) and b.causal and not a.causal
        assert a.net[3].padding == "same"
    a, b = ConformerBlock(16, heads=2), ConformerBlock(16, heads=2, causal=True, window=8)
    assert shapes(a) == shapes(b) and list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict())
    assert b.causal and b.window == 8 and b.attention.causal and b.attention.window == 8 and b.conv_block.causal
    assert not a.causal and a.window is None and not a.attention.causal and not a.conv_block.causal
    assert ConformerBlock(16, heads=2, causal=True).window is None
    with pytest.raises(TypeError):
        ConformerConvBlock(8, 17, 0.1, nn.SiLU, True)           # causal is keyword-only
    with pytest.raises(ValueError):
        ConformerBlock(16, heads=2, window=8)                   # a window needs causal=True


def test_conv_state_and_its_refusals():
    conv = ConformerConvBlock(8, kernel_size=5, dropout=0.0, causal=True).eval()
    state = conv.new_conv_state(3)
    assert state.shape == (3, 8, 4) and state.dtype == torch.float32 and not state.any()
    assert ConformerConvBlock(8, kernel_size=1, causal=True).new_conv_state(2).shape == (2, 8, 0)
    x = torch.zeros(3, 8, 6)
    with pytest.raises(AgxError, match="new_conv_state: a conv state needs a causal block"):
        ConformerConvBlock(8).new_conv_state(1)
    with pytest.raises(AgxError, match="batch = 0"):
        conv.new_conv_state(0)
    with torch.no_grad():
        with pytest.raises(AgxError, match="a conv state needs a causal block"):
            ConformerConvBlock(8, kernel_size=5).eval().run_bct(x, conv_state=state)
        with pytest.raises(AgxError, match="BatchNorm in training mode"):
            conv.train().run_bct(x, conv_state=state)
        conv.eval()
        with pytest.raises(AgxError, match="no backward through a cached call"):
            conv.run_bct(x, keep={}, conv_state=state)
        for bad in (torch.zeros(2, 8, 4), torch.zeros(3, 8, 3), torch.zeros(3, 4, 8).transpose(1, 2), torch.zeros(3, 8, 4, dtype=torch.float64),
                    "state"):
            with pytest.raises(AgxError, match="conv state: expected"):
                conv.run_bct(x, conv_state=bad)
        with pytest.raises(AgxError, match="MI355X only"):      # every refusal passed: the first op is reached
            conv.run_bct(x, conv_state=state)
    with pytest.raises(AgxError, match="no backward through a cached call"):
        conv.run_bct(x, conv_state=state)                       # autograd on, parameters require grad


def test_block_caches_and_their_refusals():
    block = ConformerBlock(16, heads=2, dropout=0.1, kernel_size=5, context_x=32, causal=True, window=8).eval()
    cache = block.new_cache(3)
    assert isinstance(cache, ConformerCache) and cache.kv.shape == (3, 2 * 16, 32) and cache.length == 0 and cache.window == 8
    assert cache.conv_state.shape == (3, 16, 4) and not cache.conv_state.any()
    stream = block.new_stream_cache(3, capacity=20)
    assert isinstance(stream, ConformerStreamCache) and stream.kv.shape == (3, 32, 20) and stream.max_chunk == 13
    assert stream.pos.dtype == torch.int64 and stream.positions() == [0, 0, 0] and stream.conv_state.shape == (3, 16, 4)
    stream.pos += 5
    stream.conv_state += 1.0
    stream.reset(rows=[1])
    assert stream.positions() == [5, 0, 5] and not stream.conv_state[1].any() and bool(stream.conv_state[[0, 2]].all())
    stream.reset()
    assert stream.positions() == [0, 0, 0] and not stream.conv_state.any()
    with pytest.raises(AgxError, match="not rows of a cache"):
        stream.reset(rows=[3])
    cache.length, _ = 4, cache.conv_state.add_(1.0)
    cache.reset()
    assert cache.length == 0 and not cache.conv_state.any()

    plain, causal = ConformerBlock(16, heads=2).eval(), ConformerBlock(16, heads=2, kernel_size=5, causal=True).eval()
    with pytest.raises(AgxError, match="new_cache: a cache needs a causal"):
        plain.new_cache(1)
    with pytest.raises(AgxError, match="new_stream_cache: device-held positions need a windowed causal"):
        causal.new_stream_cache(1)
    with pytest.raises(AgxError, match="cannot hold a window"):
        block.new_cache(1, capacity=7)
    with pytest.raises(AgxError, match="batch = 0"):
        block.new_stream_cache(0)

    x = torch.zeros(3, 16, 4)
    with torch.no_grad():
        with pytest.raises(AgxError, match="a cache needs a causal ConformerBlock"):
            plain.run_bct(x, cache=cache)
        with pytest.raises(AgxError, match="a stream cache needs a windowed causal"):
            causal.run_bct(x, cache=stream)
        with pytest.raises(AgxError, match="cache= takes a ConformerCache"):
            block.run_bct(x, cache=(cache.kv, 0))
        with pytest.raises(AgxError, match="active dropout site"):
            block.train().run_bct(x, cache=cache)
        block.eval()
        block.conv_block.net[4].train()
        with pytest.raises(AgxError, match="BatchNorm in training mode"):
            block.run_bct(x, cache=cache)
        block.eval()
        with pytest.raises(AgxError, match="the cache was made for batch 3"):
            block.run_bct(torch.zeros(2, 16, 4), cache=cache)
        with pytest.raises(AgxError, match="the cache was made for window 8"):
            ConformerBlock(16, heads=2, kernel_size=5, causal=True, window=4).eval().run_bct(x, cache=cache)
        with pytest.raises(AgxError, match="conv state is"):
            ConformerBlock(16, heads=2, kernel_size=7, causal=True, window=8).eval().run_bct(x, cache=cache)
        with pytest.raises(AgxError, match="max_chunk = 13"):
            block.run_bct(torch.zeros(3, 16, 14), cache=stream)
        cache.length = 10
        with pytest.raises(AgxError, match="exceed the ring's capacity 32"):
            block.run_bct(torch.zeros(3, 16, 26), cache=cache)
        cache.length = 0
        linear = causal.new_cache(3, capacity=16)
        linear.length = 14
        with pytest.raises(AgxError, match="14 cached \\+ 4 new frames exceed"):
            causal.run_bct(x, cache=linear)
        block.attention.attention_dtype = "bf16"
        with pytest.raises(AgxError, match="causal attention runs in fp32"):
            block.run_bct(x, cache=cache)
        block.attention.attention_dtype = "fp32"
        with pytest.raises(AgxError, match="MI355X only"):      # every refusal passed: the first op is reached
            block.run_bct(x, cache=cache)
        assert cache.length == 0
        # a causal block whose attention dropout is active has no kernel
        with pytest.raises(AgxError, match="attention dropout > 0 in training mode"):
            block.train().run_bct(x)
    with pytest.raises(AgxError, match="no backward through a cached call"):
        block.eval().run_bct(x, cache=cache)                    # autograd on


# ------------------------------------------------------------------------------------------------ the launches
from tests.test_conformer_cpu import ATTN, CONV_EVAL, FF, NEW_OPS, Recorder, TRANSFORMER_STANDINS  # noqa: E402

CAUSAL_OPS = ("glu_dwconv_causal", "glu_dwconv_causal_backward", "glu_dwconv_step", "glu_hist_update")


class CausalRecorder(Recorder):
    def result(self, op, a):
        z = torch.zeros
        if op in ("glu_dwconv_causal", "glu_dwconv_step"):
            return z(a["u"].shape[0], a["u"].shape[1] // 2, a["u"].shape[2])
        if op == "glu_hist_update":
            return a["hist"]
        if op == "glu_dwconv_causal_backward":
            return super().result("glu_dwconv_backward", a)
        return super().result(op, a)


def _walk(model, call, mp):
    import json
    real = {op: getattr(ops, op) for op in TRANSFORMER_STANDINS + NEW_OPS + CAUSAL_OPS}
    rec = CausalRecorder(model)
    for op in real:
        mp.setattr(ops, op, rec.standin(op))
    rec.start()
    with torch.no_grad():
        call()
    for op, fn in real.items():
        mp.setattr(ops, op, fn)
    log = [json.loads(e) for e in rec.log]
    return [op for op, _ in log if op not in ("conv_pack", "conv_pack_bwd")], log


def test_cached_walks(monkeypatch):
    conv = ConformerConvBlock(8, kernel_size=5, dropout=0.0, causal=True).eval()
    state = conv.new_conv_state(2)
    step = [op if op != "glu_dwconv" else "glu_dwconv_step" for op in CONV_EVAL]
    names, log = _walk(conv, lambda: conv.run_bct(torch.zeros(2, 8, MAX_STEP), conv_state=state), monkeypatch)
    assert names == step
    names, _ = _walk(conv, lambda: conv.run_bct(torch.zeros(2, 8, MAX_STEP + 1), conv_state=state), monkeypatch)
    assert names == ["layernorm_ct", "conv_forward", "glu_dwconv_causal", "glu_hist_update", "conv_forward"]
    names, _ = _walk(conv, lambda: conv.run_bct(torch.zeros(2, 8, 11)), monkeypatch)
    assert names == [op if op != "glu_dwconv" else "glu_dwconv_causal" for op in CONV_EVAL]
