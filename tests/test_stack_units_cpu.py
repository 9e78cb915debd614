"""The unit list of the conv stacks and every library call the stacks make, pinned against recordings (no kernel is launched).

``CausalVQAE._units`` is the one description of a stack that inference, training and the long-form planner read.  Two recordings,
taken on the commit named inside them BEFORE the unit list replaced the three separate walks of the module tree, say what it has
to reproduce:

* ``tests/golden/stack_units.json``: per model of ``WIRING`` and per stack the units -- kind, slopes, the ``state_dict`` key of
  every tensor of ``params()`` in order, ``primitives()`` -- and ``longform.receptive_field(model)``.  On the recording commit
  ``primitives()`` was the concatenation of ``longform._primitives`` over the unit's modules, and equal to the planner's own walk
  of the stack.
* ``tests/golden/stack_launch_trace.json``: the same wirings at the config-S widths (32 first-block channels, 512 latent channels:
  the bf16x3 layers and the activation-plane head exist only there) with every ``ops`` function of ``STANDINS`` replaced by a
  recorder that returns zeros of the right shape, run through ``STEPS``: inference twice (the second call pins the cache hits),
  training forward + backward with the hidden activation saved and re-materialised, inference on the bf16x3 decoders twice,
  training with ``impl`` pinned on every conv by hand, and inference back on fp32.  An entry is the op, every field of its
  descriptor in the order of ``_lib.ConvDesc``, every scalar argument, and per tensor argument the ``state_dict`` key, the
  packed image's tag (op, source keys, kind, impl of its pack call), or the shape of an activation.  The recording keeps the
  op and a digest of each entry (``digest``), not its text: a differing entry is reported with the text the head produced.
  ``ops.conv_out_len``, ``ops.conv_planes_supported`` and ``ops.conv_kernel_name`` stay real: host-only queries.

Regenerate (on the recording commit only): ``python -m tests.test_stack_units_cpu <commit hash>``.
"""
import dataclasses
import hashlib
import inspect
import json
import os
import sys

import pytest
import torch

from audio_generation_amd import longform, native_backward, ops
from audio_generation_amd._lib import IMPL_MFMA_BF16X3, ConvDesc
from audio_generation_amd.vae import CausalDecoderBlock, CausalVQAE
from tests.test_longform_cpu import CASES, S_KW

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UNITS_FIXTURE = os.path.join(GOLDEN, "stack_units.json")
TRACE_FIXTURE = os.path.join(GOLDEN, "stack_launch_trace.json")

WIRING = {
    "config_s": CASES["config_s"],
    "depthwise": dict(S_KW, wavelet_decoders=False, depthwise=True),
    "reference_default": CASES["reference_default"],
    "multires": CASES["multires"],
    # no constructor argument of CausalVQAE reaches CausalDecoderBlock(upsample=False): the blocks are swapped in below
    "convt_blocks": dict(S_KW, wavelet_decoders=False),
}
WIDE = dict(first_block_channels=32, codebook_dim=512)
STANDINS = ("conv_pack", "conv_pack_bwd", "conv_forward", "resblock_forward", "planes_split", "conv_forward_planes", "conv_bwd_data",
            "conv_bwd_weight", "conv_grouped_bwd_data", "conv_grouped_bwd_weight", "multires_forward", "multires_backward",
            "wavelet_fold", "wavelet_fold_backward")
OPS = STANDINS + ("-- backward --",)
STEPS = ("inference", "inference_again", "train_hidden_saved", "train_hidden_rematerialised", "bf16x3_decoders",
         "bf16x3_decoders_again", "train_every_impl_pinned", "fp32_restored")


def build_model(name, wide=False):
    torch.manual_seed(0)
    kw = dict(WIRING[name], **(WIDE if wide else {}))
    model = CausalVQAE(num_quantizers=1, codebook_size=8, input_format="n c l", **kw)
    if name == "convt_blocks":
        for i, blk in enumerate(model.decoders):
            if isinstance(blk, CausalDecoderBlock):
                c = blk.in_conv[0].conv
                model.decoders[i] = CausalDecoderBlock(c.in_channels, c.out_channels, c.stride[0], upsample=False)
    return model


def _keys(model):
    return {t.data_ptr(): k for k, t in model.state_dict(keep_vars=True).items()}


def _grouped(names):
    """["a.b.weight_v", "a.b.weight_g", "c.weight"] -> "a.b:weight_v,weight_g c:weight" (same order, nothing dropped)."""
    out = []
    for module, leaf in (n.rsplit(".", 1) for n in names):
        if out and out[-1][0] == module:
            out[-1][1].append(leaf)
        else:
            out.append((module, [leaf]))
    return " ".join(f"{module}:{','.join(leaves)}" for module, leaves in out)


def units_of(model):
    """Per stack a list of [kind, slope, inner_slope, state_dict keys of params() in order, primitives()], and the receptive field."""
    keys = _keys(model)
    out = {which: [[u.kind, u.slope, u.inner_slope, _grouped([keys[p.data_ptr()] for p in u.params()]), [list(p) for p in u.primitives()]]
                   for u in model._units(which)] for which in ("encoders", "decoders")}
    out["receptive_field"] = list(dataclasses.astuple(longform.receptive_field(model)))
    return out


def digest(entry):
    """What the recording keeps of a trace entry: the op (its index in ``OPS``) and 40 bits of the SHA-256 of its text."""
    return f"{OPS.index(json.loads(entry)[0])} {hashlib.sha256(entry.encode()).hexdigest()[:10]}"


class Recorder:
    """Stand-ins for the ``ops`` functions of ``STANDINS``: log the call, return zeros of the shape the real op returns."""

    def __init__(self, model):
        self.keys = _keys(model)
        self.images = {}          # id(packed image) -> tag
        self.keep = []            # the images stay alive, so an id is never reused
        self.log = []

    def describe(self, v):
        if isinstance(v, ConvDesc):
            return [getattr(v, f) for f, _ in ConvDesc._fields_]      # kind, batch, c_in, c_out, l_in, kernel, stride, ... (_lib.py)
        if isinstance(v, torch.Tensor):
            if id(v) in self.images:
                return self.images[id(v)]
            return self.keys.get(v.data_ptr()) or f"tensor{list(v.shape)}"
        return v

    def standin(self, op):
        sig = inspect.signature(getattr(ops, op))

        def call(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            a = bound.arguments
            self.log.append(json.dumps([op, {k: self.describe(v) for k, v in a.items()}], sort_keys=True, separators=(",", ":")))
            return self.result(op, a)
        return call

    def result(self, op, a):
        d, z = a.get("desc"), torch.zeros
        if op in ("conv_pack", "conv_pack_bwd"):
            image = z(1)
            self.images[id(image)] = f"{op}({self.describe(a['v'])}, {self.describe(a['g'])}, kind={d.kind}, impl={d.impl})"
            self.keep.append(image)
            return image
        if op == "conv_forward":
            return z(d.batch, d.c_out, ops.conv_out_len(d))
        if op in ("resblock_forward", "multires_forward"):
            return torch.zeros_like(a["x"])
        if op == "planes_split":
            b, c, length = a["x"].shape
            return z(b, c // 8, 3, length, 8, dtype=torch.bfloat16)
        if op == "conv_forward_planes":
            if a["out_planes"]:
                return z(d.batch, d.c_out // 8, 3, ops.conv_out_len(d), 8, dtype=torch.bfloat16)
            return z(d.batch, d.c_out, ops.conv_out_len(d))
        if op in ("conv_bwd_data", "conv_grouped_bwd_data"):
            return z(d.batch, d.c_in, d.l_in)
        if op == "conv_bwd_weight":
            return (torch.zeros_like(a["v"]), None if a["g"] is None else torch.zeros_like(a["g"]),
                    z(d.c_out) if a["want_bias"] else None)
        if op == "conv_grouped_bwd_weight":
            return z(d.c_out, d.c_in // max(d.groups, 1), d.kernel), z(d.c_out) if a["want_bias"] else None
        if op == "multires_backward":
            return tuple(torch.zeros_like(a[k]) for k in ("x", "h0", "h1", "w"))
        if op == "wavelet_fold":
            b, c, length = a["h"].shape
            return z(b, c, length * a["scale"])
        if op == "wavelet_fold_backward":
            return torch.zeros_like(a["h"]), torch.zeros_like(a["sigma"])
        raise AssertionError(op)


def trace_of(name, mp):
    """{step: [entry, ...]} of one model of ``WIRING`` at the config-S widths; ``mp`` is a ``pytest.MonkeyPatch``."""
    model = build_model(name, wide=True)
    rec = Recorder(model)
    for op in STANDINS:
        mp.setattr(ops, op, rec.standin(op))
    x = torch.zeros(2, model.in_channels, 640)
    zq = torch.zeros(2, model.codebook_dim, 2)

    def infer():
        with torch.no_grad():
            model._run_encoders(x)
            model._run_decoders(zq)

    def train():
        for run, inp in ((model._run_encoders, x), (model._run_decoders, zq)):
            y = run(inp)
            rec.log.append(json.dumps(["-- backward --", {}], separators=(",", ":")))
            y.sum().backward()

    out = {}
    for step in STEPS:
        rec.log = []
        if step.startswith("train"):
            if step == "train_every_impl_pinned":         # as tests and tools do between calls: read live, the grouped layer included
                for m in model.modules():
                    if hasattr(m, "impl"):
                        m.impl = IMPL_MFMA_BF16X3
            mp.setattr(native_backward, "SAVE_HIDDEN", step != "train_hidden_rematerialised")
            train()
        else:
            if step == "bf16x3_decoders":
                model.set_conv_arithmetic("bf16x3", "fp32")
            elif step == "fp32_restored":
                model.set_conv_arithmetic("fp32", "fp32")
            infer()
        out[step] = rec.log
    return out


@pytest.mark.parametrize("name", sorted(WIRING))
def test_units_match_the_recording(name):
    want = json.load(open(UNITS_FIXTURE))["models"][name]
    got = json.loads(json.dumps(units_of(build_model(name))))
    for which in ("encoders", "decoders"):
        assert len(got[which]) == len(want[which]), which
        for i, (g, w) in enumerate(zip(got[which], want[which])):
            assert g == w, (which, i)
    assert got["receptive_field"] == want["receptive_field"]


@pytest.mark.parametrize("name", sorted(WIRING))
def test_launch_trace_matches_the_recording(name, monkeypatch):
    fixture = json.load(open(TRACE_FIXTURE))
    rows, want = fixture["rows"], fixture["models"][name]
    got = trace_of(name, monkeypatch)
    assert sorted(got) == sorted(want)
    for step in STEPS:
        for i, (g, w) in enumerate(zip(got[step], want[step])):
            assert digest(g) == rows[w], (step, i, g, rows[w])
        assert len(got[step]) == len(want[step]), step


def test_the_recording_reaches_every_path():
    """The trace has teeth only where the recorded runs went: every stand-in was called, the planes head ran, the second calls
    packed nothing and the arithmetic switches repacked."""
    fixture = json.load(open(TRACE_FIXTURE))
    rows, models = fixture["rows"], fixture["models"]
    ops_of = lambda name, step: [OPS[int(rows[i].split()[0])] for i in models[name][step]]   # noqa: E731
    assert {op for name in models for step in STEPS for op in ops_of(name, step)} == set(OPS)
    for name in models:
        assert "conv_pack" in ops_of(name, "inference") and "conv_pack_bwd" in ops_of(name, "train_hidden_saved")
        for step in ("inference_again", "train_hidden_rematerialised", "bf16x3_decoders_again"):
            assert not {"conv_pack", "conv_pack_bwd"} & set(ops_of(name, step)), (name, step)
        assert "conv_pack" in ops_of(name, "bf16x3_decoders") and "conv_pack" in ops_of(name, "fp32_restored")
    assert "conv_forward_planes" in ops_of("config_s", "bf16x3_decoders") and "planes_split" in ops_of("config_s", "bf16x3_decoders")


def test_inference_accepts_a_block_the_backward_does_not_cover(monkeypatch):
    """A residual block around ``nn.Identity`` is listed and runs (two launches); only asking for a gradient raises."""
    from audio_generation_amd._lib import AgxError
    model = build_model("config_s")
    model.encoders[1].layers[0][0].activation = torch.nn.Identity()
    rec = Recorder(model)
    for op in STANDINS:
        monkeypatch.setattr(ops, op, rec.standin(op))
    x = torch.zeros(2, 1, 640)
    assert [u.no_backward is None for u in model._units("encoders")[:3]] == [True, False, True]
    with torch.no_grad():
        model._run_encoders(x)
    assert [op for op in (json.loads(e)[0] for e in rec.log) if op != "conv_pack"][:4] == ["conv_forward"] * 3 + ["resblock_forward"]
    n = len(rec.log)
    with pytest.raises(AgxError, match="no backward kernels for"):
        model._run_encoders(x)
    assert len(rec.log) == n


def record(commit):
    with open(UNITS_FIXTURE, "w") as fh:
        json.dump({"recorded_on": commit, "models": {name: units_of(build_model(name)) for name in sorted(WIRING)}}, fh,
                  separators=(",", ":"))
    rows, models = [], {}
    index = {}
    for name in sorted(WIRING):
        with pytest.MonkeyPatch.context() as mp:
            trace = trace_of(name, mp)
        models[name] = {step: [index.setdefault(digest(e), len(index)) for e in entries] for step, entries in trace.items()}
        print(name, {step: len(entries) for step, entries in trace.items()})
    rows = sorted(index, key=index.get)
    blob = {"recorded_on": commit,
            "format": "models[name][step][i] is an index into rows; a row is the op's index in OPS and the digest of the JSON of [op, {argument: "
                      "value}] of one call (tests/test_stack_units_cpu.py: Recorder, digest)",
            "rows": rows, "models": models}
    with open(TRACE_FIXTURE, "w") as fh:
        json.dump(blob, fh, separators=(",", ":"))
    print(len(rows), "rows,", os.path.getsize(UNITS_FIXTURE), "+", os.path.getsize(TRACE_FIXTURE), "bytes")


if __name__ == "__main__":
    record(sys.argv[1])
