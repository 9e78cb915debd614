"""Sliding-window causal ALiBi self-attention on the host (no kernel is launched): the checker of
``tests/window_attention_ref.py`` pinned to the causal checker, the four C-ABI symbols of csrc/attention_window.hip (declared,
exported, bound, the name query and the refusal codes), and the module surface: ``window=`` changes no ``state_dict`` key, the
construction errors, the refusals come before any op, ``window=None`` makes exactly the recorded calls, the windowed walk
differs from the causal walk in the attention ops alone, and the ring walk of a cached call."""
import ctypes
import json
import os

import pytest
import torch

from audio_generation_amd import _lib, ops
from audio_generation_amd import transformers as tr
from audio_generation_amd._lib import AgxError
from oracle import attention as oattn
from tests.causal_attention_ref import causal_core
from tests.test_causal_attention_cpu import CAUSAL_OPS, CausalRecorder
from tests.test_transformer_walk_cpu import FIXTURE, STANDINS, digest
from tests.window_attention_ref import window_core

UNSUPPORTED, WORKSPACE, NULL_POINTER, BAD_SHAPE = -5, -3, -2, -1
BWD_NAME = "attn_window_bwd_stats+attn_window_bwd_dq+attn_window_bwd_dkv"
SYMBOLS = ("agx_attention_alibi_window", "agx_attention_window_backward_workspace_bytes", "agx_attention_alibi_window_backward",
           "agx_attention_window_kernel_name")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from audio_generation_amd import build
    build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------- 1. the checker
def test_the_checker_is_the_causal_definition_on_every_window():
    """Query i of the windowed definition sees the keys lo..i, lo = max(0, i - W + 1), at distances i - j: exactly what the one
    query at position i - lo of the causal definition sees on the keys lo..i.  Both sides are the same mathematics in float64,
    so the difference is round-off: < 1e-12.  W >= T is the causal definition; W = 16 is far from it (a kernel that ignores the
    window cannot pass); W = 1 returns v_i."""
    b, heads, dh, t = 2, 3, 8, 37
    gen = torch.Generator().manual_seed(5)
    q = torch.randn(b, heads * dh, t, generator=gen, dtype=torch.float64)
    kv = torch.randn(b, 2 * heads * dh, t, generator=gen, dtype=torch.float64)
    slopes = oattn.alibi_slopes(heads)
    causal = causal_core(q, kv, slopes, heads, dh, dh ** 0.5)
    for w in (1, 3, 16, 37, 100):
        full = window_core(q, kv, slopes, heads, dh, dh ** 0.5, w)
        worst = 0.0
        for i in range(t):
            lo = max(0, i - w + 1)
            want = causal_core(q[..., i:i + 1], kv[..., lo:i + 1], slopes, heads, dh, dh ** 0.5, q_pos0=i - lo)[..., 0]
            worst = max(worst, float((full[..., i] - want).abs().max()))
        apart = float((full - causal).abs().max())
        print(f"window_core W={w} vs causal_core on the windows: max difference {worst:.3e}; from causal_core {apart:.3e}")
        assert worst < 1e-12
        if w >= t:
            assert torch.equal(full, causal)
        if w == 16:
            assert apart > 0.5
        if w == 1:
            assert torch.equal(full, kv[:, heads * dh:])
        for t0 in (1, 17, 36):
            part = window_core(q[..., t0:], kv, slopes, heads, dh, dh ** 0.5, w, q_pos0=t0)
            assert float((part - full[..., t0:]).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------- 2. the ABI
def test_the_abi_only_grew(lib):
    assert lib.agx_version() == 122
    header = open(os.path.join(ROOT, "include", "agx.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name


@pytest.mark.parametrize("dh,dvt", [(16, 1), (64, 2), (128, 4)])
def test_window_kernel_names(lib, dh, dvt):
    assert ops.attention_window_kernel_name(2, 4, dh, 130, 3) == f"attention_window<{dvt}>"
    assert ops.attention_window_kernel_name(2, 4, dh, 1, 1000) == f"attention_window<{dvt}>"
    assert ops.attention_window_kernel_name(2, 4, dh, 130, 64, backward=True) == BWD_NAME
    for empty in ((0, 4, dh, 5, 5), (2, 0, dh, 5, 5), (2, 4, dh, 0, 5)):
        assert ops.attention_window_kernel_name(*empty) == "none"
        assert ops.attention_window_kernel_name(*empty, backward=True) == "none"


def test_refusal_codes_precede_every_use_of_a_pointer(lib):
    buf = ctypes.create_string_buffer(96)
    assert lib.agx_attention_window_kernel_name(1, 2, 129, 5, 5, 0, buf, len(buf)) == UNSUPPORTED
    assert lib.agx_last_error().decode() == "attention_alibi_window: head_dim=129 > 128"
    assert lib.agx_attention_window_kernel_name(1, 2, 0, 5, 5, 1, buf, len(buf)) == BAD_SHAPE
    assert lib.agx_attention_window_kernel_name(1, 65536, 64, 5, 5, 0, buf, len(buf)) == BAD_SHAPE
    assert lib.agx_attention_window_kernel_name(1, 2, 64, 5, 0, 0, buf, len(buf)) == BAD_SHAPE
    assert lib.agx_last_error().decode() == "attention_alibi_window: window=0 < 1"
    assert lib.agx_attention_window_kernel_name(1, 2, 64, 5, 5, 0, None, 10) == NULL_POINTER
    fwd = lambda dh, tq, pos, w, ring, pitch, sq=None, skv=None: lib.agx_attention_alibi_window(   # noqa: E731
        None, None, 2 * dh * tq if sq is None else sq, 4 * dh * pitch if skv is None else skv, pitch, None, None, 1, 2, dh, tq,
        pos, w, ring, 4.0, None)
    assert fwd(129, 5, 0, 3, 0, 5) == UNSUPPORTED
    assert fwd(64, 5, -1, 3, 0, 5) == BAD_SHAPE
    assert fwd(64, 5, 0, 0, 0, 5) == BAD_SHAPE and fwd(64, 5, 0, -7, 0, 5) == BAD_SHAPE           # window < 1
    assert "window=" in lib.agx_last_error().decode()
    assert fwd(64, 5, 65, 3, 0, 69) == BAD_SHAPE                    # linear: kv_row_stride < q_pos0 + tq
    assert "row stride" in lib.agx_last_error().decode()
    assert fwd(64, 5, 65, 3, 0, 70) == NULL_POINTER                 # a good linear shape reaches the pointer check
    assert fwd(64, 5, 65, 16, 5 + 16 - 2, 64) == BAD_SHAPE          # a ring one column short of tq + window - 1
    assert "kv_ring=19 < tq + min(window - 1, q_pos0) = 20" in lib.agx_last_error().decode()
    assert fwd(64, 64, 0, 64, 64, 64) == NULL_POINTER and fwd(64, 64, 1, 64, 64, 64) == BAD_SHAPE    # the start of a stream: nothing older to keep
    assert fwd(64, 5, 65, 16, 20, 64) == NULL_POINTER               # the smallest ring that holds the chunk and its window
    assert fwd(64, 5, 65, 16, 65, 64) == BAD_SHAPE                  # a ring longer than the row
    assert fwd(64, 5, 65, 16, -1, 64) == BAD_SHAPE
    assert fwd(64, 5, 1600 * 2 ** 21 + 60, 12, 50, 50) == NULL_POINTER      # a 64-bit position on a ring is a good shape
    assert fwd(64, 5, 2 ** 40, 12, 0, 50) == BAD_SHAPE                      # and no linear buffer is that long
    assert fwd(64, 0, 65, 3, 0, 70) == 0 and fwd(64, 0, 0, 3, 8, 8) == 0    # empty: AGX_OK, nothing launched
    one = ctypes.c_void_p(64)                                       # never dereferenced: the strides are refused first
    bad = lambda sq, skv: lib.agx_attention_alibi_window(one, one, sq, skv, 70, one, one, 1, 2, 64, 5, 65, 3, 0, 4.0, None)  # noqa: E731
    assert bad(2 * 64 * 5 - 1, 4 * 64 * 70) == BAD_SHAPE and bad(2 * 64 * 5, 4 * 64 * 70 - 1) == BAD_SHAPE
    assert lib.agx_attention_window_backward_workspace_bytes(2, 3, 37) == 2 * 2 * 3 * 37 * 4
    assert lib.agx_attention_window_backward_workspace_bytes(0, 3, 37) == 0
    bwd = lambda dh, w, ws: lib.agx_attention_alibi_window_backward(None, None, 0, 0, None, None, None, None, None, 0, 0, None, ws,  # noqa: E731
                                                                    1, 2, dh, 37, w, 4.0, None)
    assert bwd(129, 5, 1 << 20) == UNSUPPORTED and bwd(64, 0, 1 << 20) == BAD_SHAPE and bwd(64, 5, 1 << 20) == NULL_POINTER
    ws = lambda nbytes: lib.agx_attention_alibi_window_backward(one, one, 0, 0, one, one, one, one, one, 0, 0, one, nbytes, 1, 2,  # noqa: E731
                                                                64, 37, 5, 4.0, None)
    assert ws(2 * 2 * 37 * 4 - 1) == WORKSPACE and ws(2 * 2 * 37 * 4) == BAD_SHAPE      # then the strides (0 here)


def test_the_observer_counts_the_blocks_that_run():
    """The block counts of the measured shapes: 34 of the causal forward's 90 at T = 1125, W = 128; a cached step
    3 of 18; W >= T is the causal count."""
    per_block = 2 * 64 * 128 * 64
    assert ops._window_macs(1, 1, 64, 1125, 0, 128) == 34 * per_block and ops._causal_macs(1, 1, 64, 1125, 1125, 0) == 90 * per_block
    assert ops._window_macs(1, 1, 64, 1, 1124, 128) == 3 * per_block and ops._causal_macs(1, 1, 64, 1, 1125, 1124) == 18 * per_block
    assert ops._window_macs(2, 3, 64, 300, 0, 300) == ops._causal_macs(2, 3, 64, 300, 300, 0)


# ------------------------------------------------------------------------------------------------- 3. the module surface
def _block(**kw):
    torch.manual_seed(0)
    model = tr.Transformer(64, 2, heads=2, head_dim=32, context_x=64, **kw)
    with torch.no_grad():           # as tests/test_transformer_walk_cpu.build_model: make every parameter its own
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p))
    return model


def test_window_changes_no_parameter_and_no_state_dict_key():
    causal, win = _block(causal=True), _block(causal=True, window=12)
    assert list(win.state_dict()) == list(causal.state_dict())
    assert [n for n, _ in win.named_parameters()] == [n for n, _ in causal.named_parameters()]
    win.load_state_dict(causal.state_dict())          # strict: a checkpoint loads either way
    assert win.window == 12 and all(a.window == 12 and a.causal for a, _ in win.layers)
    assert causal.window is None and all(a.window is None for a, _ in causal.layers)
    att = tr.Attention(64, dim_head=32, n_heads=2, context_x=64, causal=True, window=64)
    assert sorted(att.state_dict()) == sorted(tr.Attention(64, dim_head=32, n_heads=2, context_x=64).state_dict())


@pytest.mark.parametrize("make", [lambda **kw: tr.Transformer(64, 2, heads=2, head_dim=32, context_x=64, **kw),
                                  lambda **kw: tr.Attention(64, dim_head=32, n_heads=2, context_x=64, **kw)],
                         ids=["Transformer", "Attention"])
def test_construction_errors(make):
    with pytest.raises(ValueError, match="window= needs causal=True"):
        make(window=12)
    with pytest.raises(ValueError, match="window= needs causal=True"):
        make(causal=False, window=12)
    for w in (0, -3):
        with pytest.raises(ValueError, match=r"window >= 1"):
            make(causal=True, window=w)
    with pytest.raises(ValueError, match="window = 65 exceeds context_x = 64"):
        make(causal=True, window=65)
    assert make(causal=True, window=64).window == 64 and make(causal=True, window=1).window == 1


class WindowRecorder(CausalRecorder):
    def result(self, op, a):
        if op == "attention_alibi_window":
            b, _, t = a["q"].shape
            return torch.zeros(b, a["heads"] * a["head_dim"], t)
        if op == "attention_alibi_window_backward":
            return torch.zeros_like(a["qkv"])
        if op == "ring_write":
            return None
        return super().result(op, a)


WINDOW_OPS = ("attention_alibi_window", "attention_alibi_window_backward", "ring_write")
WALK = ["layernorm_ct", "conv_forward", "attention_alibi_window", "conv_forward", "layernorm_ct", "conv_forward", "conv_forward"]


def _recorded(model, mp):
    rec = WindowRecorder(model)
    for op in STANDINS + CAUSAL_OPS + WINDOW_OPS:
        mp.setattr(ops, op, rec.standin(op))
    return rec


def _trace(model, mp):
    """{"eval": [...], "train": [...]}: as ``tests/test_causal_attention_cpu._trace``."""
    rec, out = _recorded(model, mp), {}
    for step in ("eval", "train"):
        model.train(step == "train")
        for p in model.parameters():
            p.grad = None
        rec.start()
        if step == "eval":
            with torch.no_grad():
                model.run_bct(torch.zeros(2, 64, 50))
        else:
            y = model.run_bct(torch.zeros(2, 64, 50, requires_grad=True))
            rec.mark_backward()
            y.sum().backward()
        out[step] = rec.log
    return out


def test_window_none_makes_exactly_the_recorded_calls(lib, monkeypatch):
    """The symmetric block against the golden recording, and the causal block against itself built without the keyword."""
    fixture = json.load(open(FIXTURE))
    rows, want = fixture["rows"], fixture["models"]["block"]
    got = _trace(_block(causal=False, window=None), monkeypatch)
    for step in ("eval", "train"):
        assert [digest(g) for g in got[step]] == [rows[w] for w in want[step]], step
    monkeypatch.undo()
    with pytest.MonkeyPatch.context() as mp:
        a = _trace(_block(causal=True), mp)
    with pytest.MonkeyPatch.context() as mp:
        b = _trace(_block(causal=True, window=None), mp)
    assert a == b
    assert not any(json.loads(e)[0] in WINDOW_OPS for step in a for e in a[step])


def test_the_windowed_walk_differs_in_the_attention_ops_alone(lib):
    with pytest.MonkeyPatch.context() as mp:
        causal = _trace(_block(causal=True), mp)
    with pytest.MonkeyPatch.context() as mp:
        win = _trace(_block(causal=True, window=12), mp)
    swapped = {"attention_alibi_causal": "attention_alibi_window", "attention_alibi_causal_backward": "attention_alibi_window_backward"}
    for step in ("eval", "train"):
        assert len(causal[step]) == len(win[step])
        seen = []
        for c, w in zip(causal[step], win[step]):
            (c_op, c_args), (w_op, w_args) = json.loads(c), json.loads(w)
            if c_op in swapped:
                assert w_op == swapped[c_op]
                seen.append(w_op)
                for key in ("q", "qkv", "kv", "slopes", "heads", "head_dim", "scale_div", "dout", "out"):     # the same operands
                    assert c_args.get(key) == w_args.get(key), (w_op, key)
                assert w_args["window"] == 12
                if w_op == "attention_alibi_window":
                    assert w_args["kv"] is None and w_args["q_pos0"] == 0 and w_args["ring"] == 0
            else:
                assert c == w
        assert seen == ["attention_alibi_window"] * 2 + (["attention_alibi_window_backward"] * 2 if step == "train" else [])
    launches = [json.loads(e)[0] for e in win["eval"] if json.loads(e)[0] != "conv_pack"]     # the first eval packs as it goes
    assert launches == WALK * 2


def test_window_refusals_come_before_any_op(lib, monkeypatch):
    x = torch.zeros(2, 64, 50)
    model = _block(causal=True, window=12)
    rec = _recorded(model, monkeypatch)
    rec.start()
    for a, _ in model.layers:
        a.attention_dtype = "bf16"
    with torch.no_grad(), pytest.raises(AgxError, match="causal attention runs in fp32"):
        model.eval().run_bct(x)
    with torch.no_grad(), pytest.raises(AgxError, match="causal attention runs in fp32"):
        model.layers[0][0].run_bct(x)
    for a, _ in model.layers:
        a.attention_dtype = "fp32"
    with torch.no_grad(), pytest.raises(AgxError, match=r"sequence length 65 exceeds the ALiBi context 64 \(the reference fails "
                                                        r"here too, transformers.py:88-93\)"):
        model.run_bct(torch.zeros(2, 64, 65))
    wide = tr.Transformer(512, 1, heads=2, head_dim=256, context_x=32, causal=True, window=8)
    with pytest.raises(AgxError, match="the attention backward kernels cover head_dim <= 128"):
        wide.run_bct(torch.zeros(2, 512, 20))
    drop = tr.Transformer(64, 2, heads=2, head_dim=32, context_x=64, dropout=0.1, causal=True, window=12)
    for grad in (False, True):
        with torch.set_grad_enabled(grad), pytest.raises(AgxError, match="dropout > 0 in training mode has no kernel"):
            drop.train().run_bct(x)
    with torch.no_grad(), pytest.raises(AgxError, match="dropout > 0 in training mode has no kernel"):
        drop.layers[0][0].run_bct(x)
    assert drop.last_dropout_seed is None          # no seed was drawn
    assert rec.log == []
    monkeypatch.undo()          # a stand-in takes its signature from the op it replaces: the real one
    rec2 = _recorded(drop, monkeypatch)
    rec2.start()
    with torch.no_grad():
        drop.eval().run_bct(x)
    assert [json.loads(e)[0] for e in rec2.log if "pack" not in json.loads(e)[0]] == WALK * 2


def test_ring_cache_refusals_and_the_ring_walk(lib, monkeypatch):
    x = torch.zeros(2, 64, 5)
    model = _block(causal=True, window=12).eval()
    causal = _block(causal=True).eval()
    rec = _recorded(model, monkeypatch)
    rec.start()
    with pytest.raises(AgxError, match="a ring of capacity = 11 cannot hold a window of 12 frames"):
        model.new_cache(2, capacity=11)
    cache = model.new_cache(2)
    assert cache.length == 0 and cache.capacity == 64 and cache.window == 12 and len(cache.kv) == 2
    assert all(tuple(kv.shape) == (2, 2 * 64, 64) and kv.dtype == torch.float32 for kv in cache.kv)
    assert model.new_cache(3, capacity=12).kv[0].shape == (3, 128, 12)
    assert causal.new_cache(2).window is None
    with torch.no_grad():
        with pytest.raises(AgxError, match="the cache was made for batch 2"):
            model.run_bct(torch.zeros(3, 64, 5), cache=cache)
        cache.length = 100
        with pytest.raises(AgxError, match=r"54 new frames \+ the 11 cached frames their window reaches exceed the ring's capacity 64"):
            model.run_bct(torch.zeros(2, 64, 54), cache=cache)
        cache.length = 3                # the start of a stream: only 3 cached frames to keep
        with pytest.raises(AgxError, match=r"62 new frames \+ the 3 cached frames their window reaches exceed the ring's capacity 64"):
            model.run_bct(torch.zeros(2, 64, 62), cache=cache)
        cache.length = 0
        with pytest.raises(AgxError, match=r"5 new frames \+ the 11 cached frames their window reaches exceed the ring's 15 columns"):
            model.layers[0][0].run_bct(x, kv_cache=(torch.zeros(2, 128, 15), 40))
        with pytest.raises(AgxError, match="the cache was made for window None"):
            model.run_bct(x, cache=causal.new_cache(2))
        # a transformer without window keeps its linear cache, its limit and its message
        linear = causal.new_cache(2, capacity=100)
        linear.length = 60
        with pytest.raises(AgxError, match=r"60 cached \+ 5 new frames exceed min\(capacity 100, context_x 64\) = 64"):
            causal.run_bct(x, cache=linear)
    with pytest.raises(AgxError, match="no backward through a cached call"):      # grad mode on, parameters require a gradient
        model.run_bct(x, cache=cache)
    drop = tr.Transformer(64, 1, heads=2, head_dim=32, context_x=64, dropout=0.1, causal=True, window=12).train()
    with torch.no_grad(), pytest.raises(AgxError, match="active dropout site"):
        drop.run_bct(x, cache=drop.new_cache(2))
    assert cache.length == 0 and rec.log == []

    # the ring walk on the recorder: per layer the chunk's K / V rows go to columns (length + t) mod capacity -- one copy, two
    # when the chunk wraps -- and the op reads the ring from q_pos0 = length; length advances past context_x and keeps counting
    def step(n):
        rec.start()
        with torch.no_grad():
            model.run_bct(torch.zeros(2, 64, n), cache=cache)
        calls = [json.loads(e) for e in rec.log]
        names = [c[0] for c in calls if "pack" not in c[0]]
        writes = [(c[1]["col0"], c[1]["src"]) for c in calls if c[0] == "ring_write"]
        attn = [(c[1]["q_pos0"], c[1]["ring"], c[1]["window"], c[1]["kv"]) for c in calls if c[0] == "attention_alibi_window"]
        return names, writes, attn

    cache.length = 7
    names, writes, attn = step(5)                       # columns 7..11: no wrap
    assert cache.length == 12
    assert names == ["layernorm_ct", "conv_forward", "ring_write"] + WALK[2:] + ["layernorm_ct", "conv_forward", "ring_write"] + WALK[2:]
    assert writes == [(7, "tensor[2, 128, 5]")] * 2 and attn == [(7, 64, 12, "tensor[2, 128, 64]")] * 2
    cache.length = 60
    names, writes, attn = step(10)                      # columns 60..63, then 0..5: the chunk wraps
    assert cache.length == 70 > model.context_x
    assert names.count("ring_write") == 4 and names.count("attention_alibi_window") == 2
    assert writes == [(60, "tensor[2, 128, 4]"), (0, "tensor[2, 128, 6]")] * 2 and attn == [(60, 64, 12, "tensor[2, 128, 64]")] * 2
    names, writes, attn = step(53)                      # the longest chunk: 53 + 11 = 64; columns 6..58
    assert cache.length == 123 and writes == [(6, "tensor[2, 128, 53]")] * 2 and attn[0][:2] == (70, 64)
    cache.length = 1600 * 2 ** 21 + 60                  # beyond 2^31: a Python int, passed on as it is
    names, writes, attn = step(4)
    assert attn == [(1600 * 2 ** 21 + 60, 64, 12, "tensor[2, 128, 64]")] * 2 and cache.length == 1600 * 2 ** 21 + 64
    assert writes == [((1600 * 2 ** 21 + 60) % 64, "tensor[2, 128, 4]")] * 2
    cache.reset()
    assert cache.length == 0


def test_the_bottleneck_passes_the_cache_on(lib, monkeypatch):
    model = _block(causal=True, window=12).eval()
    neck = tr.TransformerBottleneck(model)
    rec = _recorded(model, monkeypatch)
    rec.start()
    cache = model.new_cache(2)
    with torch.no_grad():
        y, idx, loss = neck(torch.zeros(2, 5, 64), cache=cache)
        assert tuple(y.shape) == (2, 5, 64) and idx is None and float(loss) == 0.0 and cache.length == 5
        neck.quantize_bcl(torch.zeros(2, 64, 3), cache=cache)
        assert cache.length == 8
        neck(torch.zeros(2, 5, 64))                     # the default is the uncached call
    assert cache.length == 8
    attn = [json.loads(e)[1] for e in rec.log if json.loads(e)[0] == "attention_alibi_window"]
    assert [(a["q_pos0"], a["ring"]) for a in attn] == [(0, 64)] * 2 + [(5, 64)] * 2 + [(0, 0)] * 2
