"""Every library call the discriminators make, pinned against a recording (no kernel is launched).

``discriminator.py`` describes each discriminator body once, as a chain of links, and walks it once forward and once backward.
``tests/golden/disc_launch_trace.json`` was recorded on the commit named inside it, BEFORE the chain replaced the five
hand-kept walks (two ``no_grad`` forwards, two ``torch.autograd.Function`` forwards, two backwards), and says what the chain
has to reproduce call for call.

Every ``ops`` function of ``STANDINS`` -- the ones ``discriminator.py`` calls that launch a kernel -- is replaced by a recorder
that returns zeros of the real shape.  An entry is the op, every field of its descriptor in the order of ``_lib.ConvDesc`` /
``_lib.Conv2dDesc``, every scalar argument, and per tensor argument its ``state_dict`` key, the tag of the pack call that made
the image, ``out<k>@<i>`` for output k of call i of the same step, or else its shape.  The recording keeps the op and a digest
of each entry (``digest``), not its text: a differing entry is reported with the text the head produced.  Host-only queries
stay real: ``ops.conv_out_len``, ``ops.conv2d_kernel_name``, ``ops.conv2d_bwd_data_kernel_name`` and the library's out-shape /
frame-count queries.

``MODELS`` x ``STEPS``: a two-block waveform discriminator at the small widths of ``tests/golden/meta_g7.json`` and an STFT
discriminator (16 first channels, window 256); the ``norm="weight"`` and ``norm=None`` variants run the loss step only.  Inputs
are (2, 1, 4096) for the STFT discriminator and (2, 1, 16384) for the waveform one: its scale-2 block leaves 3 samples of a
4096- or 8192-sample clip in front of the 5-tap conv and the library refuses the layer ("input too short"), so 16384 is the
shortest power of two the chain accepts.

Regenerate (on the recording commit only): ``python -m tests.test_disc_chain_cpu <commit hash>``.
"""
import ctypes
import hashlib
import inspect
import json
import os
import sys
import warnings

import pytest
import torch

from audio_generation_amd import _lib, ops
from audio_generation_amd import discriminator as ad
from audio_generation_amd._lib import AgxError, Conv2dDesc, ConvDesc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "disc_launch_trace.json")

STANDINS = ("avgpool1d", "avgpool1d_backward", "stft", "stft_backward", "spectral_sigma", "spectral_grad_",
            "conv_pack", "conv_pack_bwd", "conv_pack_sigma", "conv_pack_bwd_sigma", "conv2d_pack", "conv2d_pack_bwd",
            "conv_forward", "conv2d_forward", "conv_bwd_weight", "conv_bwd_data", "conv_grouped_bwd_weight",
            "conv_grouped_bwd_data", "conv2d_bwd_weight", "conv2d_bwd_data", "conv2d_bwd_data_fewchannels",
            "sigmoid", "sigmoid_backward", "reduce_mean", "reduce_mean_backward", "feature_means", "feature_means_backward")
PACKS = STANDINS[6:12]
OPS = STANDINS + ("-- backward --",)
MODELS = ("wave", "stft", "wave_weight", "wave_plain", "stft_weight", "stft_plain")
STEPS = ("eval", "eval_again", "train_no_grad", "loss", "loss_unscaled", "mid_feature_alone", "first_feature_alone",
         "output_alone", "input_without_grad")
STFT_STEPS = ("bf16x3", "bf16x3_ring", "fp32_restored")
LENGTH = {"wave": 16384, "stft": 4096}
MID_FEATURE = 3          # wave: the output of block 0's third conv (below an activation); STFT: the output of blocks[2]


def steps_of(name):
    if "_" in name:
        return ("loss",)
    return STEPS + (STFT_STEPS if name == "stft" else ())


def build_model(name):
    torch.manual_seed(0)
    kind, _, norm = name.partition("_")
    norm = {"": "spectral", "weight": "weight", "plain": None}[norm]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if kind == "stft":
            return ad.STFTDiscriminator(first_channel_size=16, win_length=256, norm=norm)
        with open(os.path.join(GOLDEN, "meta_g7.json")) as f:
            kw = json.load(f)["wave"]["kwargs"]
        disc = ad.WaveFormDiscriminator(1, n_blocks=2, norm=norm)
        disc.layers = torch.nn.ModuleList([ad.WaveformDiscriminatorBlock(1, channel_sizes=kw["channel_sizes"], groups=kw["groups"],
                                                                         scale=s, norm=norm) for s in (1, 2)])
        return disc


def digest(entry):
    """What the recording keeps of a trace entry: the op (its index in ``OPS``) and 40 bits of the SHA-256 of its text."""
    return f"{OPS.index(json.loads(entry)[0])} {hashlib.sha256(entry.encode()).hexdigest()[:10]}"


class Recorder:
    """Stand-ins for the ``ops`` functions of ``STANDINS``: log the call, return zeros of the shape the real op returns."""

    def __init__(self, model):
        self.keys = {t.data_ptr(): k for k, t in model.state_dict(keep_vars=True).items()}
        self.images = {}          # data_ptr of a packed image -> tag of the pack call that made it
        self.outputs = {}         # data_ptr of any other tensor a stand-in returned during this step -> "out<k>@<call>"
        self.keep = []            # the images, and this step's outputs, stay alive: an address is never reused
        self.log = []

    def start(self):
        self.log, self.outputs = [], {}
        self.keep = [t for t in self.keep if t.data_ptr() in self.images]

    def mark_backward(self):
        self.log.append(json.dumps(["-- backward --", {}], separators=(",", ":")))

    def describe(self, v):
        if isinstance(v, (ConvDesc, Conv2dDesc)):
            return [getattr(v, f) for f, _ in v._fields_]
        if isinstance(v, torch.Tensor):
            if v.data_ptr() in self.keys:
                return self.keys[v.data_ptr()]
            return self.images.get(v.data_ptr()) or self.outputs.get(v.data_ptr()) or f"tensor{list(v.shape)}"
        return v

    def standin(self, op):
        sig = inspect.signature(getattr(ops, op))

        def call(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            a = bound.arguments
            described = {k: self.describe(v) for k, v in a.items()}
            index = len(self.log)
            self.log.append(json.dumps([op, described], sort_keys=True, separators=(",", ":")))
            res = self.result(op, a)
            if op in PACKS:       # (desc, weight, g or sigma)
                self.images[res.data_ptr()] = f"{op}({', '.join(str(v) for v in list(described.values())[1:])}, impl={a['desc'].impl})"
            for k, t in enumerate(res if isinstance(res, tuple) else (res,)):
                if t is not None and op != "spectral_grad_":
                    self.outputs[t.data_ptr()] = f"out{k}@{index}"
                    self.keep.append(t)
            return res
        return call

    def result(self, op, a):
        d, z, lib = a.get("desc"), torch.zeros, _lib.load()
        if op in PACKS or op == "spectral_sigma":
            return z(1)
        if op == "avgpool1d":
            return z(*a["x"].shape[:-1], int(lib.agx_avgpool1d_out_len(a["x"].shape[-1], a["kernel"], a["stride"], a["padding"])))
        if op == "avgpool1d_backward":
            return z(*a["dy"].shape[:-1], a["l_in"])
        if op == "stft":
            return z(a["x"].shape[0], 2, int(lib.agx_stft_frames(a["x"].shape[1], a["n_fft"])), a["n_fft"])
        if op == "stft_backward":
            return z(a["dy"].shape[0], a["length"])
        if op == "spectral_grad_":
            return a["g"]
        if op == "conv_forward":
            return z(d.batch, d.c_out, ops.conv_out_len(d))
        if op == "conv2d_forward":
            ho, wo = ctypes.c_int32(), ctypes.c_int32()
            _lib.check(lib.agx_conv2d_out_shape(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)), "agx_conv2d_out_shape")
            return z(d.batch, d.c_out, ho.value, wo.value)
        if op == "conv_bwd_weight":
            return (torch.zeros_like(a["v"]), None if a["g"] is None else torch.zeros_like(a["g"]),
                    z(d.c_out) if a["want_bias"] else None)
        if op == "conv_grouped_bwd_weight":
            return z(d.c_out, d.c_in // max(d.groups, 1), d.kernel), z(d.c_out) if a["want_bias"] else None
        if op in ("conv_bwd_data", "conv_grouped_bwd_data"):
            return z(d.batch, d.c_in, d.l_in)
        if op == "conv2d_bwd_weight":
            return z(d.c_out, d.c_in, d.kh, d.kw), z(d.c_out) if a["want_bias"] else None
        if op in ("conv2d_bwd_data", "conv2d_bwd_data_fewchannels"):
            return z(d.batch, d.c_in, d.h_in, d.w_in)
        if op == "sigmoid":
            return torch.zeros_like(a["x"])
        if op == "sigmoid_backward":
            return torch.zeros_like(a["s"])
        if op == "reduce_mean":
            return z(1)[0]
        if op == "reduce_mean_backward":
            return torch.zeros_like(a["x"]), torch.zeros_like(a["x"]) if a["want_dy"] else None
        if op == "feature_means":
            return z(2)
        if op == "feature_means_backward":
            return (torch.zeros_like(a["x"]) if a["want_dx"] else None, torch.zeros_like(a["x"]) if a["want_dy"] else None)
        raise AssertionError(op)


def _flat(ret):
    """(out, feats) of a block or ([out, ...], feats) of a discriminator -> outputs, features."""
    outs, feats = ret
    return (outs if isinstance(outs, list) else [outs]), feats


def trace_of(name, mp):
    """{step: [entry, ...]} of one model of ``MODELS``; ``mp`` is a ``pytest.MonkeyPatch``."""
    model = build_model(name)
    rec = Recorder(model)
    for op in STANDINS:
        mp.setattr(ops, op, rec.standin(op))
    length = LENGTH[name.partition("_")[0]]
    orig = torch.zeros(2, 1, length)

    def no_grad():
        with torch.no_grad():
            model(orig)

    def loss(**kw):
        recon = torch.zeros(2, 1, length, requires_grad=True)
        gl, dl = ad.discriminator_generator_loss(orig, recon, model, **kw)
        rec.mark_backward()
        (gl + dl).backward()

    def alone(pick):
        outs, feats = _flat(model(torch.zeros(2, 1, length, requires_grad=True)))
        rec.mark_backward()
        pick(outs, feats).sum().backward()

    def input_without_grad():
        outs, feats = _flat(model(orig))
        rec.mark_backward()
        sum(t.sum() for t in outs + feats).backward()

    def arithmetic(mode):
        ad.set_arithmetic(model, mode)
        loss()

    run = {"eval": no_grad, "eval_again": no_grad, "train_no_grad": no_grad, "loss": loss,
           "loss_unscaled": lambda: loss(scale_feature_loss=False),
           "mid_feature_alone": lambda: alone(lambda outs, feats: feats[MID_FEATURE]),
           "first_feature_alone": lambda: alone(lambda outs, feats: feats[0]),
           "output_alone": lambda: alone(lambda outs, feats: outs[0]),
           "input_without_grad": input_without_grad,
           "bf16x3": lambda: arithmetic("bf16x3"), "bf16x3_ring": lambda: arithmetic("bf16x3_ring"),
           "fp32_restored": lambda: arithmetic("fp32")}
    out = {}
    for step in steps_of(name):
        model.train(not step.startswith("eval"))
        for p in model.parameters():
            p.grad = None
        rec.start()
        run[step]()
        out[step] = rec.log
    return out


@pytest.mark.parametrize("name", MODELS)
def test_launch_trace_matches_the_recording(name, monkeypatch):
    fixture = json.load(open(FIXTURE))
    rows, want = fixture["rows"], fixture["models"][name]
    got = trace_of(name, monkeypatch)
    assert sorted(got) == sorted(want)
    for step in steps_of(name):
        for i, (g, w) in enumerate(zip(got[step], want[step])):
            assert digest(g) == rows[w], (step, i, g, rows[w])
        assert len(got[step]) == len(want[step]), step


def test_the_recording_reaches_every_path():
    """The trace has teeth only where the recorded runs went: every stand-in was called, the second eval forward packed nothing,
    the loss step walks every layer three times, and the arithmetic switches changed the descriptors.  (Autograd hands a
    ``Function`` zeros for the outputs nothing was asked of, so a feature's gradient alone still walks the whole chain.)"""
    fixture = json.load(open(FIXTURE))
    rows, models = fixture["rows"], fixture["models"]
    ops_of = lambda name, step: [OPS[int(rows[i].split()[0])] for i in models[name][step]]   # noqa: E731
    assert {op for name in models for step in models[name] for op in ops_of(name, step)} == set(OPS)
    for name in ("wave", "stft"):
        assert set(PACKS) & set(ops_of(name, "eval")) and not set(PACKS) & set(ops_of(name, "eval_again"))
        assert "spectral_sigma" not in ops_of(name, "eval_again") and "spectral_sigma" in ops_of(name, "train_no_grad")
        dw = ("conv2d_bwd_weight",) if name == "stft" else ("conv_bwd_weight", "conv_grouped_bwd_weight")
        count = lambda step: sum(op in dw for op in ops_of(name, step))   # noqa: E731
        assert count("input_without_grad") == 14 and count("loss") == 3 * 14      # 14 Conv2d layers; two blocks of 7 Conv1d
        assert count("mid_feature_alone") == count("output_alone") == (14 if name == "stft" else 7)   # block 0 of the two
        head_adjoint = "stft_backward" if name == "stft" else "avgpool1d_backward"
        assert head_adjoint in ops_of(name, "first_feature_alone") and head_adjoint not in ops_of(name, "input_without_grad")
    assert models["stft"]["bf16x3"] != models["stft"]["loss"] and models["stft"]["bf16x3_ring"] != models["stft"]["bf16x3"]
    assert "conv2d_bwd_data_fewchannels" in ops_of("stft", "loss")


@pytest.mark.parametrize("name", ["wave", "stft"])
def test_an_activation_other_than_leaky_relu_has_no_backward(name, monkeypatch):
    """Asking for a gradient through another activation raises ``AgxError`` before anything is launched.  Without a gradient the
    walk reaches the layer and the conv wrappers refuse it: only LeakyReLU is fused into the conv kernels and there is no
    eager fallback (so on the recording commit, and since: ``NotImplementedError``, whatever the ``AgxError`` text holds out)."""
    model = build_model(name)
    seq = model.layers[0].layers[2] if name == "wave" else model.blocks[1].layers
    seq[1] = torch.nn.ELU()
    rec = Recorder(model)
    for op in STANDINS:
        monkeypatch.setattr(ops, op, rec.standin(op))
    x = torch.zeros(2, 1, LENGTH[name])
    with pytest.raises(AgxError, match="the backward kernels fuse the LeakyReLU gradient only"):
        model(x)
    with pytest.raises(AgxError, match="the backward kernels fuse the LeakyReLU gradient only"):
        model(x.clone().requires_grad_(True))
    assert rec.log == []
    with torch.no_grad(), pytest.raises(NotImplementedError, match="only LeakyReLU is fused"):
        model(x)
    assert not {"conv_bwd_weight", "conv2d_bwd_weight"} & {json.loads(e)[0] for e in rec.log}


def record(commit):
    index, models = {}, {}
    for name in MODELS:
        with pytest.MonkeyPatch.context() as mp:
            trace = trace_of(name, mp)
        models[name] = {step: [index.setdefault(digest(e), len(index)) for e in entries] for step, entries in trace.items()}
        print(name, {step: len(entries) for step, entries in trace.items()})
    rows = sorted(index, key=index.get)
    blob = {"recorded_on": commit,
            "format": "models[name][step][i] is an index into rows; a row is the op's index in OPS and the digest of the JSON of [op, {argument: "
                      "value}] of one call (tests/test_disc_chain_cpu.py: Recorder, digest)",
            "rows": rows, "models": models}
    with open(FIXTURE, "w") as fh:
        json.dump(blob, fh, separators=(",", ":"))
    print(len(rows), "rows,", os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    record(sys.argv[1])
