"""Causal ALiBi self-attention on the host (no kernel is launched): the checker of ``tests/causal_attention_ref.py`` pinned to
the frozen cross-attention definition, the four C-ABI symbols of csrc/attention_causal.hip (declared, exported, bound, the
name query and the refusal codes), and the module surface: ``causal=`` changes no ``state_dict`` key, the refusals come before
any op, ``causal=False`` makes exactly the recorded calls, and the causal walk differs from it in the attention ops alone."""
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
from tests.cross_attention_ref import cross_core
from tests.test_transformer_walk_cpu import FIXTURE, STANDINS, Recorder, digest

UNSUPPORTED, NULL_POINTER, BAD_SHAPE = -5, -2, -1
BWD_NAME = "attn_causal_bwd_stats+attn_causal_bwd_dq+attn_causal_bwd_dkv"
SYMBOLS = ("agx_attention_alibi_causal", "agx_attention_causal_backward_workspace_bytes", "agx_attention_alibi_causal_backward",
           "agx_attention_causal_kernel_name")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from audio_generation_amd import build
    build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------- 1. the checker
def test_the_checker_is_the_frozen_definition_on_every_prefix():
    """Query i of the causal definition sees keys 0..i at distances i - j: exactly what the LAST query of the frozen
    cross-attention definition sees on the prefix 0..i.  Both sides are the same mathematics in float64, so the difference is
    round-off: < 1e-12."""
    b, heads, dh, t = 2, 3, 8, 37
    gen = torch.Generator().manual_seed(5)
    q = torch.randn(b, heads * dh, t, generator=gen, dtype=torch.float64)
    kv = torch.randn(b, 2 * heads * dh, t, generator=gen, dtype=torch.float64)
    slopes = oattn.alibi_slopes(heads)
    full = causal_core(q, kv, slopes, heads, dh, dh ** 0.5)
    worst = 0.0
    for i in range(t):
        want = cross_core(q[..., :i + 1], kv[..., :i + 1], slopes, heads, dh, dh ** 0.5)[..., i]
        worst = max(worst, float((full[..., i] - want).abs().max()))
    print(f"causal_core vs cross_core on prefixes: max difference {worst:.3e}")
    assert worst < 1e-12
    for t0 in (1, 17, 36):
        part = causal_core(q[..., t0:], kv, slopes, heads, dh, dh ** 0.5, q_pos0=t0)
        diff = float((part - full[..., t0:]).abs().max())
        print(f"causal_core q_pos0={t0}: max difference from the full result {diff:.3e}")
        assert diff < 1e-12


# ------------------------------------------------------------------------------------------------- 2. the ABI
def test_the_abi_only_grew(lib):
    assert lib.agx_version() == 122
    header = open(os.path.join(ROOT, "include", "agx.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name


@pytest.mark.parametrize("dh,dvt", [(16, 1), (64, 2), (128, 4)])
def test_causal_kernel_names(lib, dh, dvt):
    assert ops.attention_causal_kernel_name(2, 4, dh, 130, 130) == f"attention_causal<{dvt}>"
    assert ops.attention_causal_kernel_name(2, 4, dh, 1, 70) == f"attention_causal<{dvt}>"
    assert ops.attention_causal_kernel_name(2, 4, dh, 130, 130, backward=True) == BWD_NAME
    for empty in ((0, 4, dh, 5, 5), (2, 0, dh, 5, 5), (2, 4, dh, 0, 5), (2, 4, dh, 5, 0)):
        assert ops.attention_causal_kernel_name(*empty) == "none"
        assert ops.attention_causal_kernel_name(*empty, backward=True) == "none"


def test_refusal_codes_precede_every_use_of_a_pointer(lib):
    buf = ctypes.create_string_buffer(96)
    assert lib.agx_attention_causal_kernel_name(1, 2, 129, 5, 5, 0, buf, len(buf)) == UNSUPPORTED
    assert lib.agx_last_error().decode() == "attention_alibi_causal: head_dim=129 > 128"
    assert lib.agx_attention_causal_kernel_name(1, 2, 0, 5, 5, 1, buf, len(buf)) == BAD_SHAPE
    assert lib.agx_attention_causal_kernel_name(1, 65536, 64, 5, 5, 0, buf, len(buf)) == BAD_SHAPE
    assert lib.agx_attention_causal_kernel_name(1, 2, 64, 5, 5, 0, None, 10) == NULL_POINTER
    fwd = lambda dh, tq, tk, pos, pitch, sq=None, skv=None: lib.agx_attention_alibi_causal(   # noqa: E731
        None, None, 2 * dh * tq if sq is None else sq, 4 * dh * pitch if skv is None else skv, pitch, None, None, 1, 2, dh, tq, tk,
        pos, 4.0, None)
    assert fwd(129, 5, 5, 0, 5) == UNSUPPORTED
    assert fwd(64, 5, 5, -1, 5) == BAD_SHAPE
    assert fwd(64, 5, 70, 65, 69) == BAD_SHAPE                      # kv_row_stride < tk
    assert "row stride" in lib.agx_last_error().decode()
    assert fwd(64, 5, 70, 65, 70) == NULL_POINTER                   # a good shape reaches the pointer check
    assert fwd(64, 0, 70, 65, 70) == 0 and fwd(64, 5, 0, 0, 0) == 0   # empty: AGX_OK, nothing launched
    one = ctypes.c_void_p(64)                                       # never dereferenced: the strides are refused first
    bad = lambda sq, skv: lib.agx_attention_alibi_causal(one, one, sq, skv, 70, one, one, 1, 2, 64, 5, 70, 65, 4.0, None)  # noqa: E731
    assert bad(2 * 64 * 5 - 1, 4 * 64 * 70) == BAD_SHAPE and bad(2 * 64 * 5, 4 * 64 * 70 - 1) == BAD_SHAPE
    assert lib.agx_attention_causal_backward_workspace_bytes(2, 3, 37) == 2 * 2 * 3 * 37 * 4
    assert lib.agx_attention_causal_backward_workspace_bytes(0, 3, 37) == 0
    bwd = lambda dh, ws: lib.agx_attention_alibi_causal_backward(None, None, 0, 0, None, None, None, None, None, 0, 0, None, ws, 1, 2,  # noqa: E731
                                                                 dh, 37, 4.0, None)
    assert bwd(129, 1 << 20) == UNSUPPORTED and bwd(64, 1 << 20) == NULL_POINTER


# ------------------------------------------------------------------------------------------------- 3. the module surface
def _block(**kw):
    torch.manual_seed(0)
    model = tr.Transformer(64, 2, heads=2, head_dim=32, context_x=64, **kw)
    with torch.no_grad():           # as tests/test_transformer_walk_cpu.build_model: make every parameter its own
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p))
    return model


def test_causal_changes_no_parameter_and_no_state_dict_key():
    plain, causal = _block(), _block(causal=True)
    assert list(causal.state_dict()) == list(plain.state_dict())
    assert [n for n, _ in causal.named_parameters()] == [n for n, _ in plain.named_parameters()]
    causal.load_state_dict(plain.state_dict())          # strict: a checkpoint loads either way
    assert causal.causal and all(a.causal for a, _ in causal.layers) and not plain.causal
    att = tr.Attention(64, dim_head=32, n_heads=2, context_x=64, causal=True)
    assert sorted(att.state_dict()) == sorted(tr.Attention(64, dim_head=32, n_heads=2, context_x=64).state_dict())
    with pytest.raises(ValueError, match="causal=True with context_y"):
        tr.Transformer(64, 2, heads=2, head_dim=32, context_x=64, context_y=32, causal=True)
    with pytest.raises(ValueError, match="causal=True with context_y"):
        tr.Attention(64, dim_head=32, n_heads=2, context_x=64, context_y=32, causal=True)


class CausalRecorder(Recorder):
    def result(self, op, a):
        if op == "attention_alibi_causal":
            b, _, t = a["q"].shape
            return torch.zeros(b, a["heads"] * a["head_dim"], t)
        if op == "attention_alibi_causal_backward":
            return torch.zeros_like(a["qkv"])
        return super().result(op, a)


CAUSAL_OPS = ("attention_alibi_causal", "attention_alibi_causal_backward")


def _recorded(model, mp):
    rec = CausalRecorder(model)
    for op in STANDINS + CAUSAL_OPS:
        mp.setattr(ops, op, rec.standin(op))
    return rec


def _trace(model, mp):
    """{"eval": [...], "train": [...]}: as ``tests/test_transformer_walk_cpu.trace_of`` for these two steps."""
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


def test_causal_false_makes_exactly_the_recorded_calls(lib, monkeypatch):
    fixture = json.load(open(FIXTURE))
    rows, want = fixture["rows"], fixture["models"]["block"]
    got = _trace(_block(causal=False), monkeypatch)
    for step in ("eval", "train"):
        assert [digest(g) for g in got[step]] == [rows[w] for w in want[step]], step


def test_the_causal_walk_differs_in_the_attention_ops_alone(lib):
    with pytest.MonkeyPatch.context() as mp:
        plain = _trace(_block(), mp)
    with pytest.MonkeyPatch.context() as mp:
        causal = _trace(_block(causal=True), mp)
    swapped = {"attention_alibi": "attention_alibi_causal", "attention_alibi_backward": "attention_alibi_causal_backward"}
    for step in ("eval", "train"):
        assert len(plain[step]) == len(causal[step])
        seen = []
        for p, c in zip(plain[step], causal[step]):
            (p_op, p_args), (c_op, c_args) = json.loads(p), json.loads(c)
            if p_op in swapped:
                assert c_op == swapped[p_op]
                seen.append(c_op)
                for key in ("slopes", "heads", "head_dim", "scale_div", "dout", "out"):     # the same operands
                    assert p_args.get(key) == c_args.get(key), (c_op, key)
                assert c_args.get("qkv", c_args.get("q")) == p_args["qkv"]
                if c_op == "attention_alibi_causal":
                    assert c_args["kv"] is None and c_args["q_pos0"] == 0 and c_args["tk"] is None
            else:
                assert p == c
        assert seen == ["attention_alibi_causal"] * 2 + (["attention_alibi_causal_backward"] * 2 if step == "train" else [])
    launches = [json.loads(e)[0] for e in causal["eval"] if json.loads(e)[0] != "conv_pack"]     # the first eval packs as it goes
    assert launches == ["layernorm_ct", "conv_forward", "attention_alibi_causal", "conv_forward", "layernorm_ct", "conv_forward",
                        "conv_forward"] * 2


def test_causal_refusals_come_before_any_op(lib, monkeypatch):
    x = torch.zeros(2, 64, 50)
    model = _block(causal=True)
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
    wide = tr.Transformer(512, 1, heads=2, head_dim=256, context_x=32, causal=True)
    with pytest.raises(AgxError, match="the attention backward kernels cover head_dim <= 128"):
        wide.run_bct(torch.zeros(2, 512, 20))
    drop = tr.Transformer(64, 2, heads=2, head_dim=32, context_x=64, dropout=0.1, causal=True)
    for grad in (False, True):
        with torch.set_grad_enabled(grad), pytest.raises(AgxError, match="dropout > 0 in training mode has no kernel"):
            drop.train().run_bct(x)
    with torch.no_grad(), pytest.raises(AgxError, match="dropout > 0 in training mode has no kernel"):
        drop.layers[0][0].run_bct(x)
    assert drop.last_dropout_seed is None          # no seed was drawn
    assert rec.log == []
    # eval mode with dropout > 0 runs (on the recorder): the 7 launches per layer, no dropout op
    monkeypatch.undo()          # a stand-in takes its signature from the op it replaces: the real one
    rec2 = _recorded(drop, monkeypatch)
    rec2.start()
    with torch.no_grad():
        drop.eval().run_bct(x)
    assert [json.loads(e)[0] for e in rec2.log if "pack" not in json.loads(e)[0]] == [
        "layernorm_ct", "conv_forward", "attention_alibi_causal", "conv_forward", "layernorm_ct", "conv_forward", "conv_forward"] * 2


def test_cache_refusals_come_before_any_op(lib, monkeypatch):
    x = torch.zeros(2, 64, 5)
    plain, cross = _block(), tr.Transformer(64, 1, heads=2, head_dim=32, context_x=64, context_y=32)
    model = _block(causal=True).eval()
    rec = _recorded(model, monkeypatch)
    rec.start()
    for other in (plain, cross):
        with pytest.raises(AgxError, match="needs a causal self-attention Transformer"):
            other.new_cache(2)
    cache = model.new_cache(2)
    assert cache.length == 0 and cache.capacity == 64 and len(cache.kv) == 2
    assert all(tuple(kv.shape) == (2, 2 * 64, 64) and kv.dtype == torch.float32 for kv in cache.kv)
    assert model.new_cache(3, capacity=10).kv[0].shape == (3, 128, 10)
    with torch.no_grad():
        for other in (plain.eval(), cross.eval()):
            with pytest.raises(AgxError, match="needs a causal self-attention Transformer"):
                other.run_bct(x, cache=cache)
        with pytest.raises(AgxError, match="needs a causal self-attention layer"):
            plain.layers[0][0].run_bct(x, kv_cache=(cache.kv[0], 0))
        with pytest.raises(AgxError, match="the cache was made for batch 2"):
            model.run_bct(torch.zeros(3, 64, 5), cache=cache)
        with pytest.raises(AgxError, match=r"0 cached \+ 65 new frames exceed"):
            model.run_bct(torch.zeros(2, 64, 65), cache=cache)
        small = model.new_cache(2, capacity=4)
        with pytest.raises(AgxError, match=r"exceed min\(capacity 4, context_x 64\) = 4"):
            model.run_bct(x, cache=small)
        big = model.new_cache(2, capacity=100)
        big.length = 60
        with pytest.raises(AgxError, match=r"60 cached \+ 5 new frames exceed min\(capacity 100, context_x 64\) = 64"):
            model.run_bct(x, cache=big)
        assert big.length == 60
    with pytest.raises(AgxError, match="no backward through a cached call"):      # grad mode on, parameters require a gradient
        model.run_bct(x, cache=cache)
    drop = tr.Transformer(64, 1, heads=2, head_dim=32, context_x=64, dropout=0.1, causal=True).train()
    with torch.no_grad(), pytest.raises(AgxError, match="active dropout site"):
        drop.run_bct(x, cache=drop.new_cache(2))
    assert cache.length == 0 and rec.log == []
    # the cached walk on the recorder: the causal op on the layer's buffer, from the cached length, and the length advances
    cache.length = 7
    with torch.no_grad():
        model.run_bct(x, cache=cache)
    assert cache.length == 12
    calls = [json.loads(e) for e in rec.log if json.loads(e)[0] == "attention_alibi_causal"]
    assert [(c[1]["q_pos0"], c[1]["tk"], c[1]["kv"]) for c in calls] == [(7, 12, "tensor[2, 128, 64]")] * 2
    assert [json.loads(e)[0] for e in rec.log if "pack" not in json.loads(e)[0]] == [
        "layernorm_ct", "conv_forward", "attention_alibi_causal", "conv_forward", "layernorm_ct", "conv_forward", "conv_forward"] * 2
    cache.reset()
    assert cache.length == 0
