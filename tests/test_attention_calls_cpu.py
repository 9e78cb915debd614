"""Every library call the attention wrappers of ``ops.py`` make, pinned against a recording (no kernel is launched).

``attention_alibi`` and its ``_cross``, ``_dropout``, ``_ragged``, ``_packed``, ``_causal``, ``_window`` and ``_stream`` variants
hand a (q, kv) pair to the C ABI as two pointers and two batch strides, in one of three layouts: a qkv tensor read in place, a
separate q and kv, or q (or the Q rows of a qkv tensor) against a key/value buffer.  ``tests/golden/attention_call_trace.json``
was recorded on the commit named inside it, BEFORE that arithmetic and the shape checks around it were given one home, and says
what the wrappers have to reproduce call for call.

The wrappers run on CPU tensors: ``_need_gpu`` and ``_stream`` are replaced, the int32 length and cu tensors say they are on the
device (``OnDevice``), and ``_lib.load`` answers ``FakeLib``, whose every symbol records its arguments and returns 0 --
``*_workspace_bytes`` answers ``WORKSPACE`` bytes, ``agx_attention_kernel_name`` writes the name the case chose, and
``agx_attention_backward_kernel_name`` returns the code the case chose.  An entry is the symbol, every scalar as passed (a ctypes
scalar with its type) and every pointer as ``<name>+<byte offset>``: the name of the input the case gave, ``<ret>`` (``<ret0>``,
``<ret1>`` of a pair) for what the wrapper returned, else ``alloc<k>`` for the k-th ``torch.empty`` / ``empty_like`` of the call
or ``copy<k>`` for the k-th copy ``_f32c`` made, each with its shape and dtype.  The observer's ``begin`` / ``end`` / ``macs``
sit in the same list with the whole ``info`` tuple, a refusal is ``["raises", <message>]`` -- after no library call but a name
query -- and the last entry of a call that returned is the shapes of what it returned.  Every case runs with an observer and
without one.  The recording keeps every distinct entry's text once: a differing entry is reported with the text the head
produced.

Regenerate (on the recording commit only): ``python -m tests.test_attention_calls_cpu <commit hash>``.
"""
import ctypes
import json
import os
import sys

import pytest
import torch

from audio_generation_amd import _lib, ops
from audio_generation_amd._lib import AgxError

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_call_trace.json")
WORKSPACE = 4096
SINGLE_PASS, FLASH = b"attention_alibi<16, 1>", b"attention_flash<16, 1>"
UNSUPPORTED = -5
B, H, DH, HD, TQ, TK, CAP, N, NK = 2, 2, 16, 32, 5, 7, 20, 5, 7
A = (H, DH, 4.0)                    # heads, head_dim, scale_div
DROP = (0.25, (1 << 63) + 5, 7)     # p, seed, stream_id
MODES = ("observed", "plain")


class OnDevice(torch.Tensor):
    """An int32 length or cu tensor that says it is on the device; pointer, dtype and contiguity stay real."""
    is_cuda = True


def _span(t):
    return (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) if t.is_contiguous() else (0, 0)


def _what(t):
    return f"{list(t.shape)} {str(t.dtype)[6:]}"


class Trace:
    """The entries of one call of a wrapper, and the tensors its pointers are named by."""

    def __init__(self, lib_name, backward_code):
        self.log, self.inputs, self.made, self.keep = [], {}, [], []
        self.lib_name, self.backward_code = lib_name, backward_code

    # ------------------------------------------------------------------ the case's inputs
    def named(self, name, t):
        self.inputs[name] = t
        return t

    def f(self, name, *shape, dtype=torch.float32):
        return self.named(name, torch.zeros(*shape, dtype=dtype))

    def dev(self, name, values, dtype=torch.int32):
        return self.named(name, torch.tensor(values, dtype=dtype).as_subclass(OnDevice))

    def i64(self, name, values):
        return self.named(name, torch.tensor(values, dtype=torch.int64))

    # ------------------------------------------------------------------ what the wrapper makes
    def make(self, kind, t):
        n = sum(1 for k, _ in self.made if k.startswith(kind))
        self.made.append((f"{kind}{n} {_what(t)}", t))
        return t

    def resolve(self, addr, returned):
        ret = [returned] if isinstance(returned, torch.Tensor) else list(returned or ())
        names = list(self.inputs.items()) + [("ret" + (str(i) if len(ret) > 1 else ""), t) for i, t in enumerate(ret)] + self.made
        for name, t in names:
            lo, hi = _span(t)
            if lo <= addr < hi:
                return f"<{name}>+{addr - lo}"
        return "<?>"

    def value(self, v):
        if isinstance(v, ctypes.c_void_p):
            return "null" if v.value is None else ("ptr", v.value)
        if isinstance(v, (ctypes.c_double, ctypes.c_uint64, ctypes.c_uint32)):
            return f"{type(v).__name__}({v.value})"
        if isinstance(v, ctypes.Array):
            return f"char[{len(v)}]"
        assert v is None or type(v) in (int, float, bool), (type(v), v)
        return v

    def finish(self, returned):
        """The entries as text: pointers resolved now that the returned tensors are known."""
        def fix(v):
            return self.resolve(v[1], returned) if isinstance(v, tuple) else v
        return [json.dumps([fix(v) for v in e], separators=(",", ":")) for e in self.log]

    # ------------------------------------------------------------------ the observer
    def begin(self, kind, info):
        self.log.append(["begin", kind, *info])
        return len(self.log)

    def end(self, token):
        self.log.append(["end"])

    def macs(self, kind, n):
        self.log.append(["macs", kind, n])


class FakeLib:
    def __init__(self, trace):
        self.trace = trace

    def __getattr__(self, symbol):
        def call(*args):
            self.trace.log.append([symbol, *map(self.trace.value, args)])
            if symbol.endswith("_workspace_bytes"):
                return WORKSPACE
            if symbol == "agx_attention_kernel_name":
                args[-2].value = self.trace.lib_name
            if symbol == "agx_attention_backward_kernel_name":
                return self.trace.backward_code
            return 0
        return call


class TorchProxy:
    """``ops.torch`` with ``empty`` / ``empty_like`` seen by the trace (as ``tests/guarded.py`` routes them)."""

    def __init__(self, trace):
        self.__dict__["_trace"] = trace

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *a, **k):
        return self._trace.make("alloc", torch.empty(*a, **k))

    def empty_like(self, *a, **k):
        return self._trace.make("alloc", torch.empty_like(*a, **k))


def run(case, observed, mp):
    """The entries of ``CASES[case]`` as text, with an observer or without."""
    call, lib_name, backward_code = CASES[case]
    trace = Trace(lib_name, backward_code)
    real_f32c = ops._f32c

    def f32c(t):
        r = real_f32c(t)
        return r if r is t else trace.make("copy", r)
    mp.setattr(ops, "_need_gpu", lambda *tensors: None)
    mp.setattr(ops, "_stream", lambda: ctypes.c_void_p(0))
    mp.setattr(ops, "_f32c", f32c)
    mp.setattr(ops, "torch", TorchProxy(trace))
    mp.setattr(ops, "_observer", trace if observed else None)
    mp.setattr(_lib, "load", lambda: FakeLib(trace))
    try:
        returned = call(trace)
    except AgxError as e:
        assert all(entry[0].endswith("_kernel_name") for entry in trace.log), (case, trace.log)
        return trace.finish(None) + [json.dumps(["raises", str(e)])]
    ret = [returned] if isinstance(returned, torch.Tensor) else list(returned)
    return trace.finish(returned) + [json.dumps(["returns", *map(_what, ret)], separators=(",", ":"))]


# ------------------------------------------------------------------------------------------------- the cases
CASES = {}       # name: (call(trace), the answer of agx_attention_kernel_name, the answer of agx_attention_backward_kernel_name)


def case(name, call, lib_name=SINGLE_PASS, backward_code=0):
    assert name not in CASES, name
    CASES[name] = (call, lib_name, backward_code)


def qkv(t, c=3 * HD, b=B, n=TQ, name="qkv"):
    return t.f(name, b, c, n)


def q_kv(t, cq=HD, ckv=2 * HD, bk=B, tk=TK, b=B, tq=TQ):
    return t.f("q", b, cq, tq), t.f("kv", bk, ckv, tk)


def slopes(t):
    return t.f("slopes", H)


def o_do(t, b=B, tq=TQ, out=None, dout=None):
    return t.f("out", *(out or (b, HD, tq))), t.f("dout", *(dout or (b, HD, tq)))


def lens(t, given):
    return dict(q_len=t.dev("q_len", [5, 2]), k_len=t.dev("k_len", [7, 0])) if given else {}


def cu(t, keys=False, **more):
    kw = dict(cu_q=t.dev("cu_q", [0, 3, 5]), max_q=3)
    if keys:
        kw.update(cu_k=t.dev("cu_k", [0, 4, 7]), max_k=4)
    kw.update(more)
    return kw


for name, lib_name in (("single_pass", SINGLE_PASS), ("flash_name", FLASH)):
    case(f"alibi fp32, {name}", lambda t: ops.attention_alibi(qkv(t), slopes(t), *A), lib_name)
    case(f"alibi bf16 flash, {name}", lambda t: ops.attention_alibi(qkv(t), slopes(t), *A, precision=ops.ATTN_BF16, flash=True), lib_name)
case("alibi_backward single launch", lambda t: ops.attention_alibi_backward(qkv(t), slopes(t), t.f("dout", B, HD, TQ), *A))
case("alibi_backward ex", lambda t: ops.attention_alibi_backward(qkv(t), slopes(t), t.f("dout", B, HD, TQ), *A, out=t.f("out", B, HD, TQ)),
     backward_code=UNSUPPORTED)
case("alibi_backward ex without out", lambda t: ops.attention_alibi_backward(qkv(t), slopes(t), t.f("dout", B, HD, TQ), *A),
     backward_code=UNSUPPORTED)
case("alibi wrong channels", lambda t: ops.attention_alibi(qkv(t, 64), slopes(t), *A))

case("cross", lambda t: ops.attention_alibi_cross(*q_kv(t), slopes(t), *A))
case("cross_backward", lambda t: ops.attention_alibi_cross_backward(*q_kv(t), slopes(t), *o_do(t), *A))
case("cross, q a non-contiguous view",
     lambda t: ops.attention_alibi_cross(t.named("q", torch.zeros(B, TQ, HD).transpose(1, 2)), t.f("kv", B, 2 * HD, TK), slopes(t), *A))

# the three two-form variants: (q, kv) and (qkv, None); extra: the arguments after scale_div
TWO_FORM = {
    "dropout": (ops.attention_alibi_dropout, ops.attention_alibi_dropout_backward, {"": lambda t: dict(zip(("p", "seed", "stream_id"), DROP))}),
    "ragged": (ops.attention_alibi_ragged, ops.attention_alibi_ragged_backward, {" lengths": lambda t: lens(t, True), " full": lambda t: lens(t, False)}),
}
for name, (fwd, bwd, extras) in TWO_FORM.items():
    for tag, extra in extras.items():
        case(f"{name} q kv{tag}", lambda t, fwd=fwd, extra=extra: fwd(*q_kv(t), slopes(t), *A, **extra(t)))
        case(f"{name} qkv{tag}", lambda t, fwd=fwd, extra=extra: fwd(qkv(t), None, slopes(t), *A, **extra(t)))
        case(f"{name}_backward q kv{tag}", lambda t, bwd=bwd, extra=extra: bwd(*q_kv(t), slopes(t), *o_do(t), *A, **extra(t)))
        case(f"{name}_backward qkv{tag}", lambda t, bwd=bwd, extra=extra: bwd(qkv(t), None, slopes(t), *o_do(t), *A, **extra(t)))
case("dropout_backward, kv and dout non-contiguous views",
     lambda t: ops.attention_alibi_dropout_backward(t.f("q", B, HD, TQ), t.named("kv", torch.zeros(B, TK, 2 * HD).transpose(1, 2)), slopes(t),
                                                    t.f("out", B, HD, TQ), t.named("dout", torch.zeros(B, TQ, HD).transpose(1, 2)), *A, *DROP))

PACKED = {"packed": ops.attention_alibi_packed, "packed_backward": ops.attention_alibi_packed_backward}


def packed(t, name, q, kv, **kw):
    grads = ()
    if name == "packed_backward":
        grads = (kw.pop("out"), kw.pop("dout")) if "out" in kw else o_do(t, b=1, tq=N)
    return PACKED[name](q, kv, slopes(t), *grads, *A, **kw)


for name in PACKED:
    case(f"{name} qkv, keys defaulted", lambda t, name=name: packed(t, name, qkv(t, b=1, n=N), None, **cu(t)))
    case(f"{name} qkv, keys given", lambda t, name=name: packed(t, name, qkv(t, b=1, n=N), None, **cu(t, cu_k=t.dev("cu_k", [0, 2, 5]), max_k=4)))
    case(f"{name} q kv", lambda t, name=name: packed(t, name, *q_kv(t, b=1, bk=1, tq=N, tk=NK), **cu(t, keys=True)))

# the cached forms: (qkv, None), (q, buffer), (qkv as q, buffer)
case("causal qkv", lambda t: ops.attention_alibi_causal(qkv(t), None, slopes(t), *A))
case("causal qkv, tk = T", lambda t: ops.attention_alibi_causal(qkv(t), None, slopes(t), *A, tk=TQ))
case("causal q buffer", lambda t: ops.attention_alibi_causal(*q_kv(t, tk=CAP), slopes(t), *A, q_pos0=9, tk=14))
case("causal q buffer, defaults", lambda t: ops.attention_alibi_causal(*q_kv(t, tk=CAP), slopes(t), *A))
case("causal qkv as q, buffer", lambda t: ops.attention_alibi_causal(*q_kv(t, cq=3 * HD, tk=CAP), slopes(t), *A, q_pos0=9, tk=14))
case("causal q buffer, tk = 0", lambda t: ops.attention_alibi_causal(*q_kv(t, tk=CAP), slopes(t), *A, q_pos0=9, tk=0))
case("causal_backward", lambda t: ops.attention_alibi_causal_backward(qkv(t), slopes(t), *o_do(t), *A))
case("window qkv", lambda t: ops.attention_alibi_window(qkv(t), None, slopes(t), *A, window=4))
case("window q buffer", lambda t: ops.attention_alibi_window(*q_kv(t, tk=CAP), slopes(t), *A, window=4, q_pos0=9, ring=16))
case("window qkv as q, buffer", lambda t: ops.attention_alibi_window(*q_kv(t, cq=3 * HD, tk=CAP), slopes(t), *A, window=4, q_pos0=9, ring=16))
case("window q buffer, q_pos0 = 2^40", lambda t: ops.attention_alibi_window(*q_kv(t, tk=CAP), slopes(t), *A, window=4, q_pos0=1 << 40, ring=16))
case("window q buffer, window = 2^40", lambda t: ops.attention_alibi_window(*q_kv(t, tk=CAP), slopes(t), *A, window=1 << 40, q_pos0=9))
case("window q buffer, window = 0", lambda t: ops.attention_alibi_window(*q_kv(t, tk=CAP), slopes(t), *A, window=0, q_pos0=9))
case("window_backward", lambda t: ops.attention_alibi_window_backward(qkv(t), slopes(t), *o_do(t), *A, window=4))
case("window_backward, window = 2^40", lambda t: ops.attention_alibi_window_backward(qkv(t), slopes(t), *o_do(t), *A, window=1 << 40))


def stream(t, cq=HD, counts=False, pos=None, **kw):
    q, kv = q_kv(t, cq=cq, tk=CAP, **kw)
    pos = t.i64("pos", [3, 1 << 40]) if pos is None else pos
    return ops.attention_alibi_stream(q, kv, pos, slopes(t), *A, window=4, ring=16, **(dict(counts=t.i64("counts", [5, 0])) if counts else {}))


for cq in (HD, 3 * HD):
    for counts in (False, True):
        case(f"stream q of {cq} channels{', counted' if counts else ''}", lambda t, cq=cq, counts=counts: stream(t, cq, counts))
case("stream, window = 2^40", lambda t: ops.attention_alibi_stream(*q_kv(t, tk=CAP), t.i64("pos", [3, 4]), slopes(t), *A, window=1 << 40, ring=16))

# ------------------------------------------------------------------------------------------------- refusals
# wrong qkv channels in every kv=None form
QKV_FORMS = {
    "dropout": lambda t, q: ops.attention_alibi_dropout(q, None, slopes(t), *A, *DROP),
    "dropout_backward": lambda t, q: ops.attention_alibi_dropout_backward(q, None, slopes(t), *o_do(t), *A, *DROP),
    "ragged": lambda t, q: ops.attention_alibi_ragged(q, None, slopes(t), *A),
    "ragged_backward": lambda t, q: ops.attention_alibi_ragged_backward(q, None, slopes(t), *o_do(t), *A),
    "packed": lambda t, q: packed(t, "packed", q, None, **cu(t)),
    "packed_backward": lambda t, q: packed(t, "packed_backward", q, None, **cu(t)),
    "causal": lambda t, q: ops.attention_alibi_causal(q, None, slopes(t), *A),
    "causal_backward": lambda t, q: ops.attention_alibi_causal_backward(q, slopes(t), *o_do(t), *A),
    "window": lambda t, q: ops.attention_alibi_window(q, None, slopes(t), *A, window=4),
    "window_backward": lambda t, q: ops.attention_alibi_window_backward(q, slopes(t), *o_do(t), *A, window=4),
}
for name, call in QKV_FORMS.items():
    case(f"{name} qkv: wrong channels", lambda t, call=call, name=name: call(t, qkv(t, HD, b=1 if "packed" in name else B)))
    case(f"{name} qkv: float64", lambda t, call=call, name=name: call(t, t.f("qkv", 1 if "packed" in name else B, 3 * HD, TQ, dtype=torch.float64)))

# wrong q channels, wrong kv channels and a batch mismatch in every (q, kv) form
QKV_AS_Q = ("causal", "window", "stream")
KV_FORMS = {
    "cross": lambda t, q, kv: ops.attention_alibi_cross(q, kv, slopes(t), *A),
    "cross_backward": lambda t, q, kv: ops.attention_alibi_cross_backward(q, kv, slopes(t), *o_do(t), *A),
    "dropout": lambda t, q, kv: ops.attention_alibi_dropout(q, kv, slopes(t), *A, *DROP),
    "dropout_backward": lambda t, q, kv: ops.attention_alibi_dropout_backward(q, kv, slopes(t), *o_do(t), *A, *DROP),
    "ragged": lambda t, q, kv: ops.attention_alibi_ragged(q, kv, slopes(t), *A),
    "ragged_backward": lambda t, q, kv: ops.attention_alibi_ragged_backward(q, kv, slopes(t), *o_do(t), *A),
    "packed": lambda t, q, kv: packed(t, "packed", q, kv, **cu(t, keys=True)),
    "packed_backward": lambda t, q, kv: packed(t, "packed_backward", q, kv, **cu(t, keys=True)),
    "causal": lambda t, q, kv: ops.attention_alibi_causal(q, kv, slopes(t), *A, q_pos0=9, tk=14),
    "window": lambda t, q, kv: ops.attention_alibi_window(q, kv, slopes(t), *A, window=4, q_pos0=9, ring=16),
    "stream": lambda t, q, kv: ops.attention_alibi_stream(q, kv, t.i64("pos", [3, 4]), slopes(t), *A, window=4, ring=16),
}
for name, call in KV_FORMS.items():
    one = dict(b=1, bk=1) if "packed" in name else {}
    case(f"{name} q kv: wrong q channels", lambda t, call=call, one=one: call(t, *q_kv(t, cq=2 * HD, **one)))
    case(f"{name} q kv: wrong kv channels", lambda t, call=call, one=one: call(t, *q_kv(t, ckv=3 * HD, **one)))
    case(f"{name} q kv: wrong q and kv channels", lambda t, call=call, one=one: call(t, *q_kv(t, cq=2 * HD, ckv=3 * HD, **one)))
    case(f"{name} q kv: kv bfloat16", lambda t, call=call, one=one: call(t, t.f("q", one.get("b", B), HD, TQ),
                                                                          t.f("kv", one.get("b", B), 2 * HD, TK, dtype=torch.bfloat16)))
    if "packed" not in name:
        case(f"{name} q kv: batch mismatch", lambda t, call=call: call(t, *q_kv(t, bk=3)))
        case(f"{name} q kv: wrong kv channels and batch mismatch", lambda t, call=call: call(t, *q_kv(t, ckv=HD, bk=3)))
    if name not in QKV_AS_Q:
        case(f"{name} q kv: q of qkv channels", lambda t, call=call, one=one: call(t, *q_kv(t, cq=3 * HD, **one)))

case("causal: tk with kv=None", lambda t: ops.attention_alibi_causal(qkv(t), None, slopes(t), *A, tk=4))
case("causal: tk beyond the buffer", lambda t: ops.attention_alibi_causal(*q_kv(t, tk=CAP), slopes(t), *A, tk=CAP + 1))
case("causal: tk negative", lambda t: ops.attention_alibi_causal(*q_kv(t, tk=CAP), slopes(t), *A, tk=-1))
case("causal: batch mismatch and tk beyond the buffer", lambda t: ops.attention_alibi_causal(*q_kv(t, tk=CAP, bk=3), slopes(t), *A, tk=CAP + 1))
case("causal: wrong channels and tk with kv=None", lambda t: ops.attention_alibi_causal(qkv(t, HD), None, slopes(t), *A, tk=4))
case("window: q_pos0 with kv=None", lambda t: ops.attention_alibi_window(qkv(t), None, slopes(t), *A, window=4, q_pos0=3))
case("window: ring with kv=None", lambda t: ops.attention_alibi_window(qkv(t), None, slopes(t), *A, window=4, ring=16))
case("window: wrong channels and ring with kv=None", lambda t: ops.attention_alibi_window(qkv(t, HD), None, slopes(t), *A, window=4, ring=16))

# out / dout of the wrong shape in every backward; a second fault behind it; a dtype in front of it
BACKWARDS = {
    "cross_backward": lambda t, g: ops.attention_alibi_cross_backward(*q_kv(t), slopes(t), *g, *A),
    "dropout_backward q kv": lambda t, g: ops.attention_alibi_dropout_backward(*q_kv(t), slopes(t), *g, *A, *DROP),
    "dropout_backward qkv": lambda t, g: ops.attention_alibi_dropout_backward(qkv(t), None, slopes(t), *g, *A, *DROP),
    "ragged_backward q kv": lambda t, g: ops.attention_alibi_ragged_backward(*q_kv(t), slopes(t), *g, *A, q_len=t.dev("q_len", [1, 2, 3])),
    "ragged_backward qkv": lambda t, g: ops.attention_alibi_ragged_backward(qkv(t), None, slopes(t), *g, *A, q_len=t.dev("q_len", [1, 2, 3])),
    "causal_backward": lambda t, g: ops.attention_alibi_causal_backward(qkv(t), slopes(t), *g, *A),
    "window_backward": lambda t, g: ops.attention_alibi_window_backward(qkv(t), slopes(t), *g, *A, window=4),
}
for name, call in BACKWARDS.items():
    case(f"{name}: wrong out", lambda t, call=call: call(t, o_do(t, out=(B, HD, TQ + 1))))
    case(f"{name}: wrong dout", lambda t, call=call: call(t, o_do(t, dout=(B, 2 * HD, TQ))))
    case(f"{name}: out of kv's length", lambda t, call=call: call(t, o_do(t, tq=TK)))
for name, q_of in (("q kv", lambda t: q_kv(t, b=1, bk=1, tq=N, tk=NK)), ("qkv", lambda t: (qkv(t, b=1, n=N), None))):
    for bad, shapes in (("wrong out", dict(out=(1, HD, N + 1))), ("wrong dout", dict(dout=(2, HD, N)))):
        case(f"packed_backward {name}: {bad}",
             lambda t, q_of=q_of, shapes=shapes: packed(t, "packed_backward", *q_of(t), **dict(zip(("out", "dout"), o_do(t, b=1, tq=N, **shapes))),
                                                        **cu(t, keys=True)))
case("packed_backward: wrong out and a bad cu_q",
     lambda t: packed(t, "packed_backward", qkv(t, b=1, n=N), None, out=t.f("out", 1, HD, N + 1), dout=t.f("dout", 1, HD, N),
                      cu_q=t.dev("cu_q", [0]), max_q=3))
case("cross_backward: wrong kv channels before wrong out",
     lambda t: ops.attention_alibi_cross_backward(*q_kv(t, ckv=HD), slopes(t), *o_do(t, out=(B, HD, TQ + 1)), *A))
case("dropout_backward: wrong channels before wrong out",
     lambda t: ops.attention_alibi_dropout_backward(qkv(t, HD), None, slopes(t), *o_do(t, out=(B, HD, TQ + 1)), *A, *DROP))
case("causal_backward: wrong channels before wrong out",
     lambda t: ops.attention_alibi_causal_backward(qkv(t, HD), slopes(t), *o_do(t, out=(B, HD, TQ + 1)), *A))
case("window_backward: wrong channels before wrong out",
     lambda t: ops.attention_alibi_window_backward(qkv(t, HD), slopes(t), *o_do(t, out=(B, HD, TQ + 1)), *A, window=4))
case("cross_backward: dout float64 and wrong q channels",
     lambda t: ops.attention_alibi_cross_backward(*q_kv(t, cq=2 * HD), slopes(t), t.f("out", B, HD, TQ), t.f("dout", B, HD, TQ, dtype=torch.float64), *A))
case("dropout_backward: out float64 and kv bfloat16",
     lambda t: ops.attention_alibi_dropout_backward(t.f("q", B, HD, TQ), t.f("kv", B, 2 * HD, TK, dtype=torch.bfloat16), slopes(t),
                                                    t.f("out", B, HD, TQ, dtype=torch.float64), t.f("dout", B, HD, TQ), *A, *DROP))
case("ragged_backward: q bfloat16 and out float64",
     lambda t: ops.attention_alibi_ragged_backward(t.f("q", B, HD, TQ, dtype=torch.bfloat16), t.f("kv", B, 2 * HD, TK), slopes(t),
                                                   t.f("out", B, HD, TQ, dtype=torch.float64), t.f("dout", B, HD, TQ), *A))
case("causal_backward: dout float64 and wrong channels",
     lambda t: ops.attention_alibi_causal_backward(qkv(t, HD), slopes(t), t.f("out", B, HD, TQ), t.f("dout", B, HD, TQ, dtype=torch.float64), *A))
case("packed_backward: dout float64 and two rows",
     lambda t: packed(t, "packed_backward", qkv(t, n=N), None, out=t.f("out", 1, HD, N), dout=t.f("dout", 1, HD, N, dtype=torch.float64), **cu(t)))

# packed: one row, separate keys, the bounds, the cu tensors
case("packed: two rows", lambda t: packed(t, "packed", qkv(t, n=N), None, **cu(t)))
case("packed: kv of two rows", lambda t: packed(t, "packed", *q_kv(t, b=1, tq=N, tk=NK), **cu(t, keys=True)))
case("packed: q without a batch dim", lambda t: packed(t, "packed", t.f("q", 3 * HD, N), None, **cu(t)))
case("packed: two rows before wrong channels", lambda t: packed(t, "packed", qkv(t, HD, n=N), None, **cu(t)))
case("packed_backward: two rows before wrong channels", lambda t: packed(t, "packed_backward", qkv(t, HD, n=N), None, **cu(t)))
case("packed: separate keys need cu_k and max_k", lambda t: packed(t, "packed", *q_kv(t, b=1, bk=1, tq=N, tk=NK), **cu(t)))
case("packed: separate keys with cu_k alone", lambda t: packed(t, "packed", *q_kv(t, b=1, bk=1, tq=N, tk=NK), **cu(t, cu_k=t.dev("cu_k", [0, 4, 7]))))
case("packed: separate keys before a bad cu_q",
     lambda t: packed(t, "packed", *q_kv(t, b=1, bk=1, tq=N, tk=NK), cu_q=t.named("cu_q", torch.tensor([0, 3, 5])), max_q=3))
case("packed: wrong channels before separate keys", lambda t: packed(t, "packed", *q_kv(t, cq=2 * HD, b=1, bk=1, tq=N, tk=NK), **cu(t)))
case("packed: negative max_q", lambda t: packed(t, "packed", qkv(t, b=1, n=N), None, **cu(t, max_q=-1)))
case("packed: negative max_k", lambda t: packed(t, "packed", *q_kv(t, b=1, bk=1, tq=N, tk=NK), **cu(t, keys=True, max_k=-2)))
case("packed: max_q not an integer", lambda t: packed(t, "packed", qkv(t, b=1, n=N), None, **cu(t, max_q=2.5)))
case("packed: cu_q on the host", lambda t: packed(t, "packed", qkv(t, b=1, n=N), None, cu_q=t.named("cu_q", torch.tensor([0, 3, 5], dtype=torch.int32)), max_q=3))
case("packed: cu_q a list", lambda t: packed(t, "packed", qkv(t, b=1, n=N), None, cu_q=[0, 3, 5], max_q=3))
case("packed: cu_q int64", lambda t: packed(t, "packed", qkv(t, b=1, n=N), None, cu_q=t.dev("cu_q", [0, 3, 5], torch.int64), max_q=3))
case("packed: cu_k of another count", lambda t: packed(t, "packed", *q_kv(t, b=1, bk=1, tq=N, tk=NK), **cu(t, cu_k=t.dev("cu_k", [0, 4, 6, 7]), max_k=4)))
case("packed: a bad cu_q before a negative bound", lambda t: packed(t, "packed", qkv(t, b=1, n=N), None, cu_q=t.dev("cu_q", [0]), max_q=-1))

# ragged: the length tensors
case("ragged: q_len int64", lambda t: ops.attention_alibi_ragged(*q_kv(t), slopes(t), *A, q_len=t.dev("q_len", [5, 2], torch.int64)))
case("ragged: k_len on the host", lambda t: ops.attention_alibi_ragged(*q_kv(t), slopes(t), *A, k_len=t.named("k_len", torch.tensor([5, 2], dtype=torch.int32))))
case("ragged: k_len of another batch", lambda t: ops.attention_alibi_ragged(qkv(t), None, slopes(t), *A, k_len=t.dev("k_len", [5, 2, 1])))
case("ragged: q_len before k_len", lambda t: ops.attention_alibi_ragged(qkv(t), None, slopes(t), *A, q_len=t.dev("q_len", [5]), k_len=t.dev("k_len", [5, 2, 1])))
case("ragged: wrong channels before q_len", lambda t: ops.attention_alibi_ragged(qkv(t, HD), None, slopes(t), *A, q_len=t.dev("q_len", [5])))
case("ragged_backward: q_len int64", lambda t: ops.attention_alibi_ragged_backward(*q_kv(t), slopes(t), *o_do(t), *A, q_len=t.dev("q_len", [5, 2], torch.int64)))

# stream: pos and counts
case("stream: pos int32", lambda t: stream(t, pos=t.named("pos", torch.tensor([3, 4], dtype=torch.int32))))
case("stream: pos of another batch", lambda t: stream(t, pos=t.i64("pos", [3, 4, 5])))
case("stream: pos a list", lambda t: stream(t, pos=[3, 4]))
case("stream: counts of another batch", lambda t: ops.attention_alibi_stream(*q_kv(t, tk=CAP), t.i64("pos", [3, 4]), slopes(t), *A, window=4, ring=16,
                                                                             counts=t.i64("counts", [5, 0, 1])))
case("stream: counts int32", lambda t: ops.attention_alibi_stream(*q_kv(t, tk=CAP), t.i64("pos", [3, 4]), slopes(t), *A, window=4, ring=16,
                                                                  counts=t.named("counts", torch.tensor([5, 0], dtype=torch.int32))))
case("stream: counts not contiguous", lambda t: ops.attention_alibi_stream(*q_kv(t, tk=CAP), t.i64("pos", [3, 4]), slopes(t), *A, window=4, ring=16,
                                                                          counts=t.named("counts", torch.zeros(4, dtype=torch.int64)[::2])))
case("stream: pos before counts", lambda t: ops.attention_alibi_stream(*q_kv(t, tk=CAP), t.i64("pos", [3]), slopes(t), *A, window=4, ring=16,
                                                                       counts=t.i64("counts", [5])))
case("stream: wrong channels before pos", lambda t: stream(t, cq=2 * HD, pos=t.i64("pos", [3])))


# ------------------------------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_the_recording_holds_exactly_these_cases(fixture):
    assert sorted(fixture["cases"]) == sorted(CASES)
    assert len(fixture["recorded_on"]) == 40


@pytest.mark.parametrize("name", sorted(CASES))
def test_attention_calls_match_the_recording(name, fixture, monkeypatch):
    rows = fixture["rows"]
    for mode in MODES:
        want = [rows[i] for i in fixture["cases"][name][mode]]
        with monkeypatch.context() as mp:
            got = run(name, mode == "observed", mp)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (name, mode, i, g)
        assert len(got) == len(want), (name, mode, got[len(want):])


def test_the_recording_reaches_every_path(fixture):
    """The trace has teeth only where the recorded runs went: every launching symbol of the section is called, every refusal
    text of the issue is there, a qkv tensor's keys start ``HD * T`` floats in, the gradients of a pair are named as the
    returned pair, a copy shows, and ``attention_alibi`` asks for a kernel name only under an observer."""
    rows, cases = fixture["rows"], fixture["cases"]
    entries = {name: {mode: [json.loads(rows[i]) for i in cases[name][mode]] for mode in MODES} for name in cases}
    called = {e[0] for c in entries.values() for e in c["plain"]}
    launching = {"agx_attention_alibi_ex", "agx_attention_alibi_backward", "agx_attention_alibi_backward_ex"} | {
        f"agx_attention_alibi_{v}{b}" for v in ("cross", "dropout", "ragged", "packed", "causal", "window") for b in ("", "_backward")} | {
        "agx_attention_alibi_stream", "agx_attention_alibi_stream_counted"}
    assert launching <= called, launching - called
    for name in cases:
        if name.startswith("alibi "):
            assert not any(e[0] == "agx_attention_kernel_name" for e in entries[name]["plain"]), name
    assert any(e[0] == "agx_attention_kernel_name" for e in entries["alibi fp32, single_pass"]["observed"])
    assert [e[2] for e in entries["alibi fp32, flash_name"]["observed"] if e[0] == "begin"] == ["attention_alibi:flash"]
    assert [e[2] for e in entries["alibi bf16 flash, single_pass"]["observed"] if e[0] == "begin"] == ["attention_alibi:bf16"]
    raised = [e[1] for c in entries.values() for e in c["plain"] if e[0] == "raises"]
    for text in ("qkv has 32 channels, expected 96", "q has 64 channels, expected 32", "expected 32 (or a 96-channel qkv tensor)",
                 "kv has 96 channels, expected 64", "q has batch 2, kv has batch 3", "tk = 4 with kv=None", "tk = 21 is outside the kv buffer's 20 columns",
                 "q_pos0 = 3, ring = 0 with kv=None", "are not q's (2, 32, 5)", "are not (2, 32, 5)", "are not (1, 32, 5)", "a packed batch is one row",
                 "separate keys need cu_k and max_k", "max_q = -1", "q_len must be a contiguous int32 device tensor, got torch.int64",
                 "pos must be a contiguous int64 device tensor of 2 entries", "counts must be a contiguous int64 device tensor of 2 entries",
                 "needs the forward output (out=)", "expected float32, got torch.float64"):
        assert any(text in r for r in raised), text
    assert len(raised) > 100
    call = entries["dropout_backward qkv"]["plain"][1]
    assert call[:5] == ["agx_attention_alibi_dropout_backward", "<qkv>+0", f"<qkv>+{4 * HD * TQ}", 3 * HD * TQ, 3 * HD * TQ]
    assert call[8:12] == ["<ret>+0", f"<ret>+{4 * HD * TQ}", 3 * HD * TQ, 3 * HD * TQ]
    call = entries["dropout_backward q kv"]["plain"][1]
    assert call[1:5] == ["<q>+0", "<kv>+0", HD * TQ, 2 * HD * TK] and call[8:12] == ["<ret0>+0", "<ret1>+0", HD * TQ, 2 * HD * TK]
    call = entries["causal qkv as q, buffer"]["plain"][0]
    assert call[1:6] == ["<q>+0", "<kv>+0", 3 * HD * TQ, 2 * HD * CAP, CAP]
    call = entries["cross, q a non-contiguous view"]["plain"][0]
    assert call[1] == f"<copy0 [{B}, {HD}, {TQ}] float32>+0"
    call = entries["window q buffer, window = 2^40"]["plain"][0]
    assert 0x7fffffff in call and (1 << 40) not in call


def record(commit):
    index, cases = {}, {}
    for name in CASES:
        cases[name] = {}
        for mode in MODES:
            with pytest.MonkeyPatch.context() as mp:
                cases[name][mode] = [index.setdefault(e, len(index)) for e in run(name, mode == "observed", mp)]
    rows = sorted(index, key=index.get)
    blob = {"recorded_on": commit,
            "format": "cases[name][mode][i] is an index into rows; a row is the JSON text of one entry: [symbol, argument, ...] of a library "
                      "call, [begin, kind, *info] / [end] / [macs, kind, n] of the observer, [raises, message] or [returns, shape and dtype, "
                      "...] (tests/test_attention_calls_cpu.py: Trace, FakeLib, run)",
            "rows": rows, "cases": cases}
    with open(FIXTURE, "w") as fh:
        json.dump(blob, fh, separators=(",", ":"))
    print(len(CASES), "cases,", len(rows), "rows,", os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    record(sys.argv[1])
