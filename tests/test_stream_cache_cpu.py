"""Device-held stream positions on the host (no kernel is launched): the four C-ABI symbols of csrc/attention_stream.hip
(declared, exported, bound, the name query, the refusal codes before any pointer is used), and the module surface of
``Transformer.new_stream_cache`` / ``TransformerStreamCache``: construction, ``max_chunk``, every refusal before any op with
the cache left as it was, the walk on the recorder (one ``ring_write_pos`` and one ``attention_alibi_stream`` per layer, one
``stream_advance`` per call), and the host-position cache still being what it was."""
import ctypes
import json
import os

import pytest
import torch

from audio_generation_amd import _lib, ops
from audio_generation_amd import transformers as tr
from audio_generation_amd._lib import AgxError
from tests.test_causal_attention_cpu import CAUSAL_OPS
from tests.test_transformer_walk_cpu import STANDINS
from tests.test_window_attention_cpu import WALK, WINDOW_OPS, WindowRecorder, _block

UNSUPPORTED, NULL_POINTER, BAD_SHAPE = -5, -2, -1
SYMBOLS = ("agx_attention_alibi_stream", "agx_ring_write_pos", "agx_stream_advance", "agx_attention_stream_kernel_name")
STREAM_OPS = ("attention_alibi_stream", "ring_write_pos", "stream_advance")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from audio_generation_amd import build
    build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------- 1. the ABI
def test_the_abi_only_grew(lib):
    assert lib.agx_version() == 122
    header = open(os.path.join(ROOT, "include", "agx.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name


@pytest.mark.parametrize("dh,dvt", [(16, 1), (32, 1), (33, 2), (64, 2), (65, 4), (128, 4)])
def test_stream_kernel_names(lib, dh, dvt):
    assert ops.attention_stream_kernel_name(3, 4, dh, 1, 12) == f"attention_stream<{dvt}>"
    assert ops.attention_stream_kernel_name(3, 4, dh, 130, 3) == f"attention_stream<{dvt}>"
    for empty in ((0, 4, dh, 5, 5), (2, 0, dh, 5, 5), (2, 4, dh, 0, 5)):
        assert ops.attention_stream_kernel_name(*empty) == "none"
    with pytest.raises(AgxError, match="window=0 < 1"):
        ops.attention_stream_kernel_name(3, 4, dh, 5, 0)


def test_refusal_codes_precede_every_use_of_a_pointer(lib):
    buf = ctypes.create_string_buffer(96)
    assert lib.agx_attention_stream_kernel_name(1, 2, 129, 5, 5, buf, len(buf)) == UNSUPPORTED
    assert lib.agx_last_error().decode() == "attention_alibi_stream: head_dim=129 > 128"
    assert lib.agx_attention_stream_kernel_name(1, 2, 0, 5, 5, buf, len(buf)) == BAD_SHAPE
    assert lib.agx_attention_stream_kernel_name(1, 65536, 64, 5, 5, buf, len(buf)) == BAD_SHAPE
    assert lib.agx_attention_stream_kernel_name(1, 2, 64, 5, 0, buf, len(buf)) == BAD_SHAPE
    assert lib.agx_last_error().decode() == "attention_alibi_stream: window=0 < 1"
    assert lib.agx_attention_stream_kernel_name(1, 2, 64, 5, 5, None, 10) == NULL_POINTER
    # every pointer NULL: whatever is refused is refused before a pointer is looked at; a good shape reaches the pointer check
    fwd = lambda dh, tq, w, ring, pitch, sq=None, skv=None: lib.agx_attention_alibi_stream(   # noqa: E731
        None, None, 2 * dh * tq if sq is None else sq, 4 * dh * pitch if skv is None else skv, pitch, None, None, None, 1, 2, dh, tq,
        w, ring, 4.0, None)
    assert fwd(129, 5, 3, 8, 8) == UNSUPPORTED
    assert fwd(64, 5, 0, 8, 8) == BAD_SHAPE and fwd(64, 5, -7, 8, 8) == BAD_SHAPE                 # window < 1
    assert "window=" in lib.agx_last_error().decode()
    assert fwd(64, 5, 16, 5 + 16 - 2, 64) == BAD_SHAPE              # a ring one column short of tq + window - 1
    assert "kv_ring=19 < tq + window - 1 = 20" in lib.agx_last_error().decode()
    assert fwd(64, 5, 16, 20, 64) == NULL_POINTER                   # the smallest ring that holds the chunk and its window
    assert fwd(64, 64, 64, 64, 64) == BAD_SHAPE                     # no start-of-stream allowance: the host reads no position
    assert fwd(64, 1, 64, 64, 64) == NULL_POINTER
    assert fwd(64, 5, 16, 0, 64) == BAD_SHAPE and fwd(64, 5, 16, -1, 64) == BAD_SHAPE             # the ring is mandatory
    assert "kv_ring=" in lib.agx_last_error().decode()
    assert fwd(64, 5, 16, 65, 64) == BAD_SHAPE                      # a ring longer than the row
    assert "kv_ring=65 > kv row stride 64" in lib.agx_last_error().decode()
    odd = 2 ** 25 + 1                                               # lcm(64, odd) = 64 * odd > 2^31
    assert fwd(64, 5, 16, odd, odd) == BAD_SHAPE
    assert "beyond int32" in lib.agx_last_error().decode()
    assert fwd(64, 5, 16, 2 ** 25, 2 ** 25) == NULL_POINTER         # lcm(64, 2^25) = 2^25: a good shape
    assert fwd(64, 0, 3, 8, 8) == 0 and fwd(64, 0, 3, 0, 8) == 0    # empty: AGX_OK, nothing launched
    one = ctypes.c_void_p(64)                                       # never dereferenced: the strides are refused first
    bad = lambda sq, skv: lib.agx_attention_alibi_stream(one, one, sq, skv, 70, one, one, one, 1, 2, 64, 5, 3, 70, 4.0, None)  # noqa: E731
    assert bad(2 * 64 * 5 - 1, 4 * 64 * 70) == BAD_SHAPE and bad(2 * 64 * 5, 4 * 64 * 70 - 1) == BAD_SHAPE
    assert "batch stride" in lib.agx_last_error().decode()

    wr = lambda n, ring, pitch, rows=8, batch=2: lib.agx_ring_write_pos(None, None, rows * pitch, pitch, rows * n, None, batch,  # noqa: E731
                                                                        rows, n, ring, None)
    assert wr(5, 50, 50) == NULL_POINTER
    assert wr(5, 0, 50) == BAD_SHAPE and wr(51, 50, 50) == BAD_SHAPE and wr(5, 51, 50) == BAD_SHAPE
    assert "ring=51 > buf row stride 50" in lib.agx_last_error().decode()
    assert wr(5, 50, 50, batch=65536) == BAD_SHAPE
    assert wr(0, 50, 50) == 0 and wr(5, 50, 50, rows=0) == 0 and wr(5, 50, 50, batch=0) == 0
    short = lambda sb, ss: lib.agx_ring_write_pos(one, one, sb, 50, ss, one, 2, 8, 5, 50, None)   # noqa: E731
    assert short(8 * 50 - 1, 8 * 5) == BAD_SHAPE and short(8 * 50, 8 * 5 - 1) == BAD_SHAPE

    assert lib.agx_stream_advance(None, 3, 1, None) == NULL_POINTER
    assert lib.agx_stream_advance(one, 3, -1, None) == BAD_SHAPE
    assert lib.agx_stream_advance(None, 0, 1, None) == 0


def test_pos_must_be_a_contiguous_int64_device_tensor(lib):
    """The ops refuse every other ``pos`` with ``AgxError`` before the library is called (a CPU tensor included: there is no
    CPU path)."""
    for bad in ([0, 0], torch.zeros(2, dtype=torch.int32), torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)[::2],
                torch.zeros(2, 1, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)):
        with pytest.raises(AgxError):
            ops._checked_pos("attention_alibi_stream", bad, 2, torch.device("cuda"))
    with pytest.raises(AgxError, match="pos must be a contiguous int64 device tensor"):
        ops.stream_advance([1, 2], 1)
    with pytest.raises(AgxError):
        ops.stream_advance(torch.zeros(2, dtype=torch.int64), 1)


def test_the_observer_counts_the_steady_state_blocks():
    """W = 128, tq = 1 at pos = 127: keys 0..127, two blocks; the config-3 cached step at a later alignment walks 3."""
    per_block = 2 * 64 * 128 * 64
    assert ops._window_macs(1, 1, 64, 1, 127, 128) == 2 * per_block
    assert "steady state" in ops.attention_alibi_stream.__doc__


# ------------------------------------------------------------------------------------------------- 2. the module surface
class StreamRecorder(WindowRecorder):
    def result(self, op, a):
        if op == "attention_alibi_stream":
            b, _, t = a["q"].shape
            return torch.zeros(b, a["heads"] * a["head_dim"], t)
        if op in ("ring_write_pos", "stream_advance"):
            return None
        return super().result(op, a)


def _recorded(model, mp):
    rec = StreamRecorder(model)
    for op in STANDINS + CAUSAL_OPS + WINDOW_OPS + STREAM_OPS:
        mp.setattr(ops, op, rec.standin(op))
    return rec


def test_new_stream_cache_and_max_chunk():
    model = _block(causal=True, window=12).eval()           # dim 64, depth 2, heads 2, head_dim 32, context_x 64
    cache = model.new_stream_cache(3)
    assert isinstance(cache, tr.TransformerStreamCache) and not isinstance(cache, tr.TransformerCache)
    assert (cache.batch, cache.capacity, cache.window, cache.max_chunk) == (3, 64, 12, 53) and len(cache.kv) == 2
    assert all(tuple(kv.shape) == (3, 2 * 64, 64) and kv.dtype == torch.float32 for kv in cache.kv)
    assert cache.pos.dtype == torch.int64 and tuple(cache.pos.shape) == (3,) and cache.pos.is_contiguous()
    assert cache.positions() == [0, 0, 0]
    assert model.new_stream_cache(2, capacity=12).max_chunk == 1                    # capacity = window: frame by frame
    assert model.new_stream_cache(2, capacity=200).max_chunk == 64                  # never more than context_x
    assert model.new_stream_cache(2, capacity=70).max_chunk == 59
    with pytest.raises(AgxError, match="a ring of capacity = 11 cannot hold a window of 12 frames"):
        model.new_stream_cache(2, capacity=11)
    with pytest.raises(AgxError, match="batch = 0"):
        model.new_stream_cache(0)
    cache.pos += torch.tensor([5, 2 ** 40, 7])
    cache.reset(rows=[1])
    assert cache.positions() == [5, 0, 7]
    with pytest.raises(AgxError, match="not rows of a cache of batch 3"):
        cache.reset(rows=[3])
    assert cache.positions() == [5, 0, 7]
    cache.reset()
    assert cache.positions() == [0, 0, 0]


def test_only_a_windowed_causal_self_attention_transformer_has_one():
    for kw in (dict(), dict(causal=True), dict(context_y=16)):
        model = _block(**kw)
        with pytest.raises(AgxError, match="new_stream_cache: device-held positions need a windowed causal self-attention"):
            model.new_stream_cache(2)
    causal = _block(causal=True)
    cache = causal.new_cache(2)                            # the host-position cache is what it was
    assert type(cache) is tr.TransformerCache and cache.window is None and cache.length == 0
    win = _block(causal=True, window=12).new_cache(2)
    assert type(win) is tr.TransformerCache and win.window == 12 and win.length == 0 and not hasattr(win, "pos")


def test_stream_cache_refusals_come_before_any_op(lib, monkeypatch):
    x = torch.zeros(2, 64, 5)
    model = _block(causal=True, window=12).eval()
    rec = _recorded(model, monkeypatch)
    rec.start()
    cache = model.new_stream_cache(2)
    cache.pos += 9
    kept = [kv.clone() for kv in cache.kv]
    with torch.no_grad():
        for other in (_block(), _block(causal=True)):
            with pytest.raises(AgxError, match="a stream cache needs a windowed causal self-attention Transformer"):
                other.eval().run_bct(x, cache=cache)
        for a, _ in model.layers:
            a.attention_dtype = "bf16"
        with pytest.raises(AgxError, match="causal attention runs in fp32: attention_dtype = 'bf16' has no kernel"):
            model.run_bct(x, cache=cache)
        for a, _ in model.layers:
            a.attention_dtype = "fp32"
        with pytest.raises(AgxError, match="lengths= with cache="):
            model.run_bct(x, cache=cache, lengths=[5, 3])
        with pytest.raises(AgxError, match="takes no second sequence y"):
            model.run_bct(x, torch.zeros(2, 64, 5), cache=cache)
        with pytest.raises(AgxError, match="takes no second sequence y"):
            model(x.transpose(1, 2), torch.zeros(2, 5, 64), cache=cache)
        with pytest.raises(AgxError, match="the cache holds 2 layers, this Transformer has 1"):
            tr.Transformer(64, 1, heads=2, head_dim=32, context_x=64, causal=True, window=12).eval().run_bct(x, cache=cache)
        with pytest.raises(AgxError, match="the cache was made for batch 2"):
            model.run_bct(torch.zeros(3, 64, 5), cache=cache)
        with pytest.raises(AgxError, match="the cache was made for window 12, this Transformer has window 13"):
            _block(causal=True, window=13).eval().run_bct(x, cache=cache)
        assert cache.max_chunk == 53
        for n in (0, 54, 64):
            with pytest.raises(AgxError, match=rf"1 <= n <= max_chunk = 53 frames .* got {n}"):
                model.run_bct(torch.zeros(2, 64, n), cache=cache)
        with pytest.raises(AgxError, match="device-held positions need a windowed layer"):
            _block(causal=True).layers[0][0].run_bct(x, kv_cache=(cache.kv[0], cache.pos))
        with pytest.raises(AgxError, match=r"5 new frames \+ the 11 cached frames their window reaches exceed the ring's 15 columns"):
            model.layers[0][0].run_bct(x, kv_cache=(torch.zeros(2, 128, 15), cache.pos))
    with pytest.raises(AgxError, match="no backward through a cached call"):      # grad mode on, parameters require a gradient
        model.run_bct(x, cache=cache)
    drop = tr.Transformer(64, 2, heads=2, head_dim=32, context_x=64, dropout=0.1, causal=True, window=12).train()
    with torch.no_grad(), pytest.raises(AgxError, match="active dropout site"):
        drop.run_bct(x, cache=cache)
    assert rec.log == [] and cache.positions() == [9, 9]
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(kept, cache.kv))


def test_the_stream_walk_differs_at_three_places(lib, monkeypatch):
    """Per layer LN1 -> QKV -> ring write -> attention -> W_o -> LN2 -> FFN-in -> FFN-out with the two stream ops reading
    ``cache.pos`` itself, then one advance per call by the chunk's frames; the host-position walk next to it."""
    model = _block(causal=True, window=12).eval()
    rec = _recorded(model, monkeypatch)
    cache, host = model.new_stream_cache(2), model.new_cache(2)

    def step(n, c):
        rec.start()
        with torch.no_grad():
            model.run_bct(torch.zeros(2, 64, n), cache=c)
        return [json.loads(e) for e in rec.log if "pack" not in json.loads(e)[0]]

    layer = ["layernorm_ct", "conv_forward", "ring_write_pos", "attention_alibi_stream"] + WALK[3:]
    for n in (5, 1, 53):
        calls = step(n, cache)
        assert [c[0] for c in calls] == layer * 2 + ["stream_advance"]
        writes = [c[1] for c in calls if c[0] == "ring_write_pos"]
        attn = [c[1] for c in calls if c[0] == "attention_alibi_stream"]
        assert [(w["src"], w["pos"], w["ring"]) for w in writes] == [(f"tensor[2, 128, {n}]", "tensor[2]", 64)] * 2
        assert [(a["pos"], a["ring"], a["window"], a["kv"]) for a in attn] == [("tensor[2]", 64, 12, "tensor[2, 128, 64]")] * 2
        assert calls[-1][1]["n"] == n and calls[-1][1]["pos"] == "tensor[2]"
    assert cache.positions() == [0, 0]              # the stand-in advanced nothing: the host never adds to a position itself
    calls = step(5, host)
    assert [c[0] for c in calls] == (["layernorm_ct", "conv_forward", "ring_write"] + WALK[2:]) * 2 and host.length == 5


def test_the_bottleneck_passes_the_stream_cache_on(lib, monkeypatch):
    model = _block(causal=True, window=12).eval()
    neck = tr.TransformerBottleneck(model)
    rec = _recorded(model, monkeypatch)
    rec.start()
    cache = model.new_stream_cache(2)
    with torch.no_grad():
        y, idx, loss = neck(torch.zeros(2, 5, 64), cache=cache)
        assert tuple(y.shape) == (2, 5, 64) and idx is None and float(loss) == 0.0
        neck.quantize_bcl(torch.zeros(2, 64, 3), cache=cache)
    names = [json.loads(e)[0] for e in rec.log]
    assert names.count("attention_alibi_stream") == 4 and names.count("stream_advance") == 2
    assert [json.loads(e)[1]["n"] for e in rec.log if json.loads(e)[0] == "stream_advance"] == [5, 3]
