"""Every library call the attention bottleneck makes, pinned against a recording (no kernel is launched).

``transformers.py`` describes a layer once and walks it for inference, for the training forward and -- by the names the walk gave
its intermediates -- for the backward.  ``tests/golden/transformer_launch_trace.json`` was recorded on the commit named inside
it, BEFORE that walk replaced the three hand-kept copies (``Attention.run_bct`` + ``FeedForward.run_bct``, the inlined
``_TransformerNative.forward``, and the backward with its positional ``saved[7 * li:7 * li + 7]``), and says what the walk has
to reproduce call for call.

Every ``ops`` function of ``STANDINS`` -- the ones ``transformers.py`` calls that launch a kernel -- is replaced by a recorder
that returns zeros of the real shape (the ``Recorder`` of ``tests/test_disc_chain_cpu.py``, with the results of the attention
block's ops added).  An entry is the op, every field of its descriptor, every scalar argument, and per tensor argument its
``state_dict`` key, the tag of the pack call that made the image, ``out<k>@<i>`` for output k of call i of the same step, or
else its shape; a stack of ``nn.Linear`` weights or biases (``_PackedLinear`` concatenates them) is named by the keys of its
parts, ``cat(layers.0.0.W_q.weight,...)``, found by value: two layers of one shape do not look alike.  The recording keeps the
op and a digest of each entry, not its text: a differing entry is reported with the text the head produced.

``MODELS``: the two-layer block through ``STEPS``; a T = 300 block (the split backward kernels take ``out=``); a head_dim 128
block; the standalone ``Attention`` / ``FeedForward`` in the reference layout (no residual epilogue); the bottleneck adapter.

Regenerate (on the recording commit only): ``python -m tests.test_transformer_walk_cpu <commit hash>``.
"""
import hashlib
import json
import os
import sys

import pytest
import torch

from audio_generation_amd import ops
from audio_generation_amd import transformers as tr
from audio_generation_amd._lib import AgxError
from tests.test_disc_chain_cpu import Recorder as ChainRecorder

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transformer_launch_trace.json")

STANDINS = ("layernorm_ct", "conv_pack", "conv_forward", "attention_alibi", "conv_pack_bwd", "conv_bwd_weight", "conv_bwd_data",
            "conv_bwd_data_gelu", "layernorm_ct_backward", "attention_alibi_backward")
OPS = STANDINS + ("-- backward --",)
STEPS = ("eval", "eval_again", "eval_bf16", "train", "train_input_without_grad", "train_bf16")
# name: (constructor, input shape, steps)
MODELS = {
    "block": (lambda: tr.Transformer(64, depth=2, heads=2, head_dim=32, context_x=64), (2, 64, 50), STEPS),
    "long": (lambda: tr.Transformer(64, 1, heads=2, head_dim=32, context_x=320), (2, 64, 300), ("train",)),
    "wide_heads": (lambda: tr.Transformer(256, 1, heads=2, head_dim=128, context_x=32), (2, 256, 20), ("train",)),
    "attention": (lambda: tr.Attention(64, dim_head=32, n_heads=2, bias=True, context_x=64), (2, 50, 64), ("forward",)),
    "feedforward": (lambda: tr.FeedForward(64, 64), (2, 50, 64), ("forward",)),
    "bottleneck": (lambda: tr.TransformerBottleneck(tr.Transformer(64, 1, heads=2, head_dim=32, context_x=64)), (2, 50, 64),
                   ("forward", "forward_with_grad")),
}


def build_model(name):
    torch.manual_seed(0)
    model = MODELS[name][0]()
    with torch.no_grad():           # LayerNorm gains and biases start as ones and zeros: make every parameter its own
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p))
    return model


def digest(entry):
    """What the recording keeps of a trace entry: the op (its index in ``OPS``) and 40 bits of the SHA-256 of its text."""
    return f"{OPS.index(json.loads(entry)[0])} {hashlib.sha256(entry.encode()).hexdigest()[:10]}"


class Recorder(ChainRecorder):
    def __init__(self, model):
        super().__init__(model)
        self.state = {k: t.detach() for k, t in model.state_dict(keep_vars=True).items()}

    def describe(self, v):
        text = super().describe(v)
        if isinstance(v, torch.Tensor) and isinstance(text, str) and text.startswith("tensor["):
            return self.stack_of(v) or text
        return text

    def stack_of(self, t):
        """"cat(key,...)" when ``t`` is state_dict tensors stacked along dim 0 (a trailing k = 1 axis aside), else None."""
        if t.dim() == 3 and t.shape[-1] == 1:
            t = t[..., 0]
        parts, row = [], 0
        while t.dim() in (1, 2) and row < t.shape[0]:
            hit = [k for k, w in self.state.items() if w.dim() == t.dim() and w.shape[1:] == t.shape[1:]
                   and torch.equal(t[row:row + w.shape[0]], w)]
            if len(hit) != 1:
                return None
            parts.append(hit[0])
            row += self.state[hit[0]].shape[0]
        return f"cat({','.join(parts)})" if parts else None

    def result(self, op, a):
        z = torch.zeros
        if op == "layernorm_ct":
            return torch.zeros_like(a["x"])
        if op == "attention_alibi":
            b, _, t = a["qkv"].shape
            return z(b, a["heads"] * a["head_dim"], t)
        if op == "conv_bwd_data_gelu":
            return z(a["desc"].batch, a["desc"].c_in, a["desc"].l_in)
        if op == "layernorm_ct_backward":
            return torch.zeros_like(a["x"]), z(a["x"].shape[1]), z(a["x"].shape[1])
        if op == "attention_alibi_backward":
            return torch.zeros_like(a["qkv"])
        return super().result(op, a)


def recorded(model, mp):
    rec = Recorder(model)
    for op in STANDINS:
        mp.setattr(ops, op, rec.standin(op))
    return rec


def _attention_modules(model):
    return [m for m in model.modules() if isinstance(m, tr.Attention)]


def trace_of(name, mp):
    """{step: [entry, ...]} of one model of ``MODELS``; ``mp`` is a ``pytest.MonkeyPatch``."""
    model = build_model(name)
    rec = recorded(model, mp)
    shape, steps = MODELS[name][1:]
    run = model.run_bct if isinstance(model, tr.Transformer) else model

    def infer():
        with torch.no_grad():
            run(torch.zeros(shape))

    def train(input_grad=True):
        y = run(torch.zeros(shape, requires_grad=input_grad))
        y = y[0] if isinstance(y, tuple) else y
        rec.mark_backward()
        y.sum().backward()

    out = {}
    for step in steps:
        model.train(step.startswith(("train", "forward_with_grad")))
        for a in _attention_modules(model):
            a.attention_dtype = "bf16" if step.endswith("bf16") else "fp32"
        for p in model.parameters():
            p.grad = None
        rec.start()
        if step.startswith(("eval", "forward")) and step != "forward_with_grad":
            infer()
        else:
            train(input_grad=step != "train_input_without_grad")
        out[step] = rec.log
    return out


@pytest.mark.parametrize("name", sorted(MODELS))
def test_launch_trace_matches_the_recording(name, monkeypatch):
    fixture = json.load(open(FIXTURE))
    rows, want = fixture["rows"], fixture["models"][name]
    got = trace_of(name, monkeypatch)
    assert sorted(got) == sorted(want)
    for step in MODELS[name][2]:
        for i, (g, w) in enumerate(zip(got[step], want[step])):
            assert digest(g) == rows[w], (step, i, g, rows[w])
        assert len(got[step]) == len(want[step]), step


def test_the_recording_reaches_every_path():
    """The trace has teeth only where the recorded runs went: every stand-in was called, the second eval packed nothing, the
    bf16 switch reaches the inference entries and no training entry, every backward repacks its bwd-data images, and an entry
    names the layer whose weights it reads."""
    fixture = json.load(open(FIXTURE))
    rows, models = fixture["rows"], fixture["models"]
    ops_of = lambda name, step: [OPS[int(rows[i].split()[0])] for i in models[name][step]]   # noqa: E731
    assert {op for name in models for step in models[name] for op in ops_of(name, step)} == set(OPS)
    block = models["block"]
    assert ops_of("block", "eval").count("conv_pack") == 8 and "conv_pack" not in ops_of("block", "eval_again")
    assert ops_of("block", "eval_again") == ["layernorm_ct", "conv_forward", "attention_alibi", "conv_forward", "layernorm_ct",
                                             "conv_forward", "conv_forward"] * 2
    differ = [i for i, (a, b) in enumerate(zip(block["eval_again"], block["eval_bf16"])) if a != b]
    assert differ == [2, 9]                                   # the two attention calls, and nothing else
    assert block["train_bf16"] == block["train"] == block["train_input_without_grad"]    # fp32 attention; layer 0's dx all the same
    assert block["train"][:14] == block["eval_again"]
    assert ops_of("block", "train").count("conv_pack_bwd") == 8 and ops_of("block", "train").count("conv_bwd_data_gelu") == 2
    assert len(set(block["eval_again"][:7]) & set(block["eval_again"][7:])) == 0         # layer 1 reads layer 1's parameters
    with pytest.MonkeyPatch.context() as mp:
        got = trace_of("block", mp)["train_bf16"]
    attn = [json.loads(e)[1] for e in got if json.loads(e)[0] == "attention_alibi"]
    assert [a["precision"] for a in attn] == [ops.ATTN_FP32] * 2
    assert json.loads(got[1])[1]["packed"].startswith("conv_pack(cat(layers.0.0.W_q.weight,layers.0.0.W_k.weight,layers.0.0.W_v.weight)")
    with pytest.MonkeyPatch.context() as mp:
        long = trace_of("long", mp)["train"]
    back = [json.loads(e)[1] for e in long if json.loads(e)[0] == "attention_alibi_backward"]
    assert len(back) == 1 and back[0]["out"].startswith("out0@")


@pytest.mark.parametrize("grad", [False, True])
def test_a_sequence_longer_than_the_context_is_refused(grad, monkeypatch):
    model = build_model("block")
    rec = recorded(model, monkeypatch)
    with torch.set_grad_enabled(grad), pytest.raises(AgxError, match=r"sequence length 65 exceeds the ALiBi context 64 \(the "
                                                                     r"reference fails here too, transformers.py:88-93\)"):
        model.run_bct(torch.zeros(2, 64, 65))
    with torch.no_grad(), pytest.raises(AgxError, match="sequence length 65 exceeds the ALiBi context 64"):
        model.layers[0][0].run_bct(torch.zeros(2, 64, 65))
    assert rec.log == []


def test_heads_wider_than_128_have_no_backward_and_no_forward(monkeypatch):
    """With a gradient asked for the block refuses before anything is launched; without one the walk reaches the attention op
    and the library refuses the head width (the real wrapper and the real library here: the refusal precedes any use of the
    pointers, so host tensors do)."""
    model = tr.Transformer(512, 1, heads=2, head_dim=256, context_x=32)
    rec = recorded(model, monkeypatch)
    with pytest.raises(AgxError, match=r"Transformer: the attention backward kernels cover head_dim <= 128 "
                                       r"\(agx_attention_alibi_backward_ex\); larger heads run forward only -- there is no ATen fallback"):
        model.run_bct(torch.zeros(2, 512, 20))
    assert rec.log == []
    monkeypatch.undo()
    rec = Recorder(model)
    for op in STANDINS:
        if op != "attention_alibi":
            monkeypatch.setattr(ops, op, rec.standin(op))
    monkeypatch.setattr(ops, "_need_gpu", lambda *tensors: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    with torch.no_grad(), pytest.raises(AgxError, match=r"agx_attention_alibi_ex failed \(-5\): attention_alibi: head_dim=256 > 128"):
        model.run_bct(torch.zeros(2, 512, 20))
    assert [json.loads(e)[0] for e in rec.log] == ["layernorm_ct", "conv_pack", "conv_forward"]


def record(commit):
    index, models = {}, {}
    for name in sorted(MODELS):
        with pytest.MonkeyPatch.context() as mp:
            trace = trace_of(name, mp)
        models[name] = {step: [index.setdefault(digest(e), len(index)) for e in entries] for step, entries in trace.items()}
        print(name, {step: len(entries) for step, entries in trace.items()})
    rows = sorted(index, key=index.get)
    blob = {"recorded_on": commit,
            "format": "models[name][step][i] is an index into rows; a row is the op's index in OPS and the digest of the JSON of [op, {argument: "
                      "value}] of one call (tests/test_transformer_walk_cpu.py: Recorder, digest)",
            "rows": rows, "models": models}
    with open(FIXTURE, "w") as fh:
        json.dump(blob, fh, separators=(",", ":"))
    print(len(rows), "rows,", os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    record(sys.argv[1])
