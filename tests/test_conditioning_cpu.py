"""``audio_generation_amd.conditioning`` on the host: surface, state dicts, refusals, the launches of both modules on a
recording stand-in (no kernel is launched), the return codes of the six C entry points, and the float64 checker of
``tests/conditioning_ref.py`` pinned to the goldens of the reference (``tests/golden/make_goldens_conditioning.py``)."""
import ctypes
import json
import os

import pytest
import torch

from audio_generation_amd import _lib, conditioning as cd, ops
from audio_generation_amd._lib import AgxError
from tests import conditioning_ref as ref
from tests.helpers import GOLDEN, load_npz, sub_sd
from tests.test_disc_chain_cpu import Recorder as ChainRecorder

STANDINS = ("conv_pack", "conv_forward", "conv_pack_bwd", "conv_bwd_weight", "conv_bwd_data", "film_params", "film_apply",
            "film_backward", "film_params_backward", "sigmoid_gate", "sigmoid_gate_backward")
OK, BAD_SHAPE, NULL_POINTER = 0, -1, -2


@pytest.fixture(scope="module")
def lib():
    from audio_generation_amd import build
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def g10():
    with open(os.path.join(GOLDEN, "meta_g10.json")) as f:
        return load_npz("g10_conditioning.npz"), json.load(f)


def _build(meta, name):
    m = meta["models"][name]
    return getattr(cd, m["class"])(*m["args"], **m["kwargs"])


class Recorder(ChainRecorder):
    def result(self, op, a):
        z = torch.zeros
        if op == "film_params":
            return z(a["cond"].shape[0], a["w"].shape[0])
        if op in ("film_apply", "sigmoid_gate"):
            return torch.zeros_like(a["x"]) if a["out"] is None else a["out"]
        if op == "film_backward":
            return torch.zeros_like(a["x"]), torch.zeros_like(a["gb"])
        if op == "film_params_backward":
            return torch.zeros_like(a["w"]), z(a["w"].shape[0]), torch.zeros_like(a["cond"]) if a["want_dcond"] else None
        if op == "sigmoid_gate_backward":
            return torch.zeros_like(a["x"]), torch.zeros_like(a["x"])
        return super().result(op, a)


def recorded(model, mp):
    rec = Recorder(model)
    for op in STANDINS:
        mp.setattr(ops, op, rec.standin(op))
    return rec


def names(rec):
    return [json.loads(e)[0] for e in rec.log]


# ------------------------------------------------------------------------------------------------ surface
@pytest.mark.parametrize("name", ["film", "film_nobias", "se"])
def test_construction_and_state_dict_are_the_references(name, g10):
    blob, meta = g10
    model = _build(meta, name)
    want = meta["models"][name]["state_dict"]
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == want
    assert [n for n, _ in model.named_parameters()] == list(want)           # parameters() order, the order of the gradients
    missing, unexpected = model.load_state_dict(sub_sd(blob, f"{name}/sd/"), strict=True)
    assert missing == [] and unexpected == []
    assert torch.equal(model.state_dict()[list(want)[0]], torch.from_numpy(blob[f"{name}/sd/{list(want)[0]}"]))


def test_attributes_and_keys():
    f = cd.FiLM(20, 24)
    assert (f.dim, f.out_dim, f.bias) == (20, 24, True) and list(f.state_dict()) == ["gamma.weight", "gamma.bias", "beta.weight", "beta.bias"]
    f = cd.FiLM(20, 24, bias=False)
    assert f.bias is False and list(f.state_dict()) == ["gamma.weight", "gamma.bias"] and not hasattr(f, "beta")
    assert cd.FiLM(16).out_dim == 16
    s = cd.SqueezeExcite(24)
    assert (s.dim, s.scale_factor, s.hidden_dim) == (24, 2, 12)
    assert list(s.state_dict()) == ["squeeze.weight", "squeeze.bias", "excite.weight", "excite.bias"]
    assert isinstance(s.first_activation, torch.nn.ReLU) and isinstance(s.second_activation, torch.nn.Sigmoid)
    assert cd.SqueezeExcite(130, 4).hidden_dim == 32
    import audio_generation_amd
    assert "conditioning" in audio_generation_amd.__all__


def test_other_activations_and_an_empty_hidden_layer_are_refused_at_construction():
    with pytest.raises(NotImplementedError, match="only ReLU then Sigmoid"):
        cd.SqueezeExcite(24, first_activation=torch.nn.GELU())
    with pytest.raises(NotImplementedError, match="only ReLU then Sigmoid"):
        cd.SqueezeExcite(24, second_activation=torch.nn.Tanh())
    with pytest.raises(NotImplementedError):
        cd.SqueezeExcite(24, first_activation=torch.nn.LeakyReLU(0.0))
    with pytest.raises(ValueError, match="dim // scale_factor == 0"):
        cd.SqueezeExcite(3, 4)


# ------------------------------------------------------------------------------------------------ walks and refusals
def test_none_condition_returns_the_same_object_and_launches_nothing(monkeypatch):
    f = cd.FiLM(20, 24)
    rec = recorded(f, monkeypatch)
    x = torch.zeros(3, 37, 24)
    assert f(x, None) is x and f.run_bct(x, None) is x
    bad = torch.zeros(5)                 # nothing is looked at, as in the reference
    assert f(bad, None) is bad
    assert rec.log == []


@pytest.mark.parametrize("entry,x_shape,cond_shape,match", [
    ("forward", (3, 37, 24), (3, 1, 20), "expected \\(B, 20\\)"),         # a condition that is not 2-D
    ("forward", (3, 37, 24), (20,), "expected \\(B, 20\\)"),
    ("forward", (3, 37, 24), (2, 20), "expected \\(3, 20\\)"),            # wrong batch
    ("forward", (3, 37, 24), (3, 24), "expected \\(3, 20\\)"),            # wrong width
    ("forward", (37, 24), (3, 20), "expected \\(B, L, dim\\)"),           # x that is not 3-D
    ("forward", (3, 24, 37), (3, 20), "has 37 channels"),                 # the other layout's tensor
    ("run_bct", (3, 24, 37), (3, 1, 20), "expected \\(B, 20\\)"),
    ("run_bct", (3, 24, 37), (4, 20), "expected \\(3, 20\\)"),
    ("run_bct", (3, 24, 37), (3, 21), "expected \\(3, 20\\)"),
    ("run_bct", (3, 24, 37, 1), (3, 20), "expected \\(B, dim, T\\)"),
    ("run_bct", (3, 37, 24), (3, 20), "has 37 channels"),
])
@pytest.mark.parametrize("grad", [False, True])
def test_film_refusals_come_before_the_first_launch(entry, x_shape, cond_shape, match, grad, monkeypatch):
    f = cd.FiLM(20, 24)
    rec = recorded(f, monkeypatch)
    with pytest.raises(AgxError, match=match):
        getattr(f, entry)(torch.zeros(x_shape, requires_grad=grad), torch.zeros(cond_shape))
    assert rec.log == []


def test_squeeze_excite_refusals_come_before_the_first_launch(monkeypatch):
    s = cd.SqueezeExcite(24)
    rec = recorded(s, monkeypatch)
    for entry, shape in (("run_bct", (3, 37, 24)), ("run_bct", (24, 37)), ("forward", (3, 24, 37)), ("forward", (37, 24))):
        with pytest.raises(AgxError, match="SqueezeExcite: x is"):
            getattr(s, entry)(torch.zeros(shape))
    assert rec.log == []


def test_cpu_tensors_are_refused(lib):
    with pytest.raises(AgxError, match="MI355X only"):
        cd.FiLM(20, 24)(torch.zeros(3, 37, 24), torch.zeros(3, 20))
    with pytest.raises(AgxError, match="MI355X only"):
        cd.FiLM(20, 24, bias=False).run_bct(torch.zeros(3, 24, 37, requires_grad=True), torch.zeros(3, 20))
    with pytest.raises(AgxError, match="MI355X only"):
        cd.SqueezeExcite(24).run_bct(torch.zeros(3, 24, 37))
    with pytest.raises(AgxError, match="MI355X only"):
        ops.sigmoid_gate(torch.zeros(5), torch.zeros(5))
    with pytest.raises(AgxError, match="MI355X only"):
        ops.film_backward(torch.zeros(2, 5, 7), torch.zeros(2, 10), torch.zeros(2, 5, 7), True, ops.FILM_CT)


@pytest.mark.parametrize("bias", [True, False])
def test_film_makes_two_launches_and_stacks_its_image_once(bias, monkeypatch, lib):
    f = cd.FiLM(20, 24, bias=bias)
    rec = recorded(f, monkeypatch)
    with torch.no_grad():
        out = f.run_bct(torch.zeros(3, 24, 37), torch.zeros(3, 20))
    assert names(rec) == ["film_params", "film_apply"] and tuple(out.shape) == (3, 24, 37)
    params, apply = (json.loads(e)[1] for e in rec.log)
    assert params["w"] == ("tensor[48, 20]" if bias else "gamma.weight") and apply["has_beta"] is bias
    assert apply["layout"] == ops.FILM_CT and apply["gb"] == "out0@0" and apply["out"] is None
    w0 = f._stacked.get()[0]
    rec.start()
    with torch.no_grad():
        f(torch.zeros(3, 37, 24), torch.zeros(3, 20))
    assert names(rec) == ["film_params", "film_apply"] and json.loads(rec.log[1])[1]["layout"] == ops.FILM_TC
    assert f._stacked.get()[0] is w0                                 # the stacked image is cached ...
    with torch.no_grad():
        f.gamma.weight.add_(1.0)
    w1 = f._stacked.get()[0]
    assert torch.equal(w1[:24], f.gamma.weight) and (w1 is not w0 or not bias)     # ... by version


def test_film_backward_walk_runs_only_what_is_asked_for(monkeypatch, lib):
    f = cd.FiLM(20, 24)
    rec = recorded(f, monkeypatch)

    def walk(x_grad, cond_grad, param_grad):
        f.requires_grad_(param_grad)
        x, cond = torch.zeros(3, 24, 37, requires_grad=x_grad), torch.zeros(3, 20, requires_grad=cond_grad)
        rec.start()
        out = f.run_bct(x, cond)
        rec.mark_backward()
        out.sum().backward()
        return names(rec)[3:], x.grad, cond.grad
    back, dx, dcond = walk(True, True, True)
    assert back == ["film_backward", "film_params_backward"] and dx is not None and dcond is not None
    assert all(p.grad is not None and p.grad.shape == p.shape for p in f.parameters())
    back, dx, dcond = walk(True, False, False)
    assert back == ["film_apply"] and dx is not None and dcond is None          # dx = dout * gamma alone
    back, dx, dcond = walk(False, True, False)
    assert back == ["film_backward", "film_params_backward"] and dx is None and dcond is not None
    assert json.loads(rec.log[-1])[1]["want_dcond"] is True
    back, dx, dcond = walk(False, False, True)
    assert back == ["film_backward", "film_params_backward"] and dx is None and dcond is None
    assert json.loads(rec.log[-1])[1]["want_dcond"] is False


def test_squeeze_excite_makes_three_launches(monkeypatch, lib):
    s = cd.SqueezeExcite(24)
    rec = recorded(s, monkeypatch)
    with torch.no_grad():
        s.run_bct(torch.zeros(3, 24, 37))
    assert names(rec) == ["conv_pack", "conv_forward", "conv_pack", "conv_forward", "sigmoid_gate"]      # the first call packs
    rec.start()
    with torch.no_grad():
        out = s.run_bct(torch.zeros(3, 24, 37))
    assert names(rec) == ["conv_forward", "conv_forward", "sigmoid_gate"] and tuple(out.shape) == (3, 24, 37)
    squeeze, excite, gate = (json.loads(e)[1] for e in rec.log)
    fields = [f for f, _ in _lib.ConvDesc._fields_]
    d1, d2 = dict(zip(fields, squeeze["desc"])), dict(zip(fields, excite["desc"]))
    assert (d1["c_in"], d1["c_out"], d1["kernel"], d1["epilogue"], d1["slope"]) == (24, 12, 1, _lib.EPI_LEAKY_PRE, 0.0)    # ReLU
    assert (d2["c_in"], d2["c_out"], d2["kernel"], d2["epilogue"]) == (12, 24, 1, 0) and abs(d2["slope"] - 0.1) < 1e-7
    assert squeeze["packed"].startswith("conv_pack(") and squeeze["bias"] == "tensor[12]" and excite["bias"] == "tensor[24]"
    assert excite["x"] == "out0@0" and squeeze["res"] is None and excite["res"] is None
    assert gate["z"] == "out0@1" and gate["out"] is None
    rec.start()
    with torch.no_grad():
        assert tuple(s(torch.zeros(3, 37, 24)).shape) == (3, 37, 24)
    assert names(rec) == ["conv_forward", "conv_forward", "sigmoid_gate"]


def test_squeeze_excite_backward_walk(monkeypatch, lib):
    s = cd.SqueezeExcite(24)
    rec = recorded(s, monkeypatch)
    x = torch.zeros(3, 24, 37, requires_grad=True)
    out = s.run_bct(x)
    rec.mark_backward()
    out.sum().backward()
    log = [json.loads(e) for e in rec.log]
    back = log[[e[0] for e in log].index("-- backward --") + 1:]
    assert [e[0] for e in back] == ["sigmoid_gate_backward", "conv_bwd_weight", "conv_pack_bwd", "conv_bwd_data", "conv_bwd_weight",
                                    "conv_pack_bwd", "conv_bwd_data"]
    excite_dx, squeeze_dx = back[3][1], back[6][1]
    assert excite_dx["mask"] == "out0@1" and excite_dx["slope"] == 0.0 and excite_dx["add"] is None      # the ReLU gradient at hidden
    assert squeeze_dx["add"].startswith("out0@") and squeeze_dx["mask"] is None                          # the gate's direct dx
    assert x.grad is not None and all(p.grad is not None and p.grad.shape == p.shape for p in s.parameters())
    rec.start()
    s.run_bct(torch.zeros(3, 24, 37)).sum().backward()               # parameters only: no backward-data of the squeeze layer
    assert names(rec).count("conv_bwd_data") == 1


# ------------------------------------------------------------------------------------------------ the C entry points
def test_entry_points_validate_on_the_host(lib):
    assert lib.agx_version() == 122
    buf = ctypes.create_string_buffer(64)          # never dereferenced: every call below is refused or empty
    p = ctypes.cast(buf, ctypes.c_void_p)
    CT, TC = _lib.FILM_CT, _lib.FILM_TC
    # an empty shape: AGX_OK and nothing launched, whatever the pointers
    for shape in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4)):
        assert lib.agx_film_params(None, None, None, None, *shape, None) == OK
        assert lib.agx_film_params_backward(None, None, None, None, None, None, *shape, None) == OK
        for layout in (CT, TC):
            assert lib.agx_film_apply(None, None, None, *shape, 1, layout, None) == OK
            assert lib.agx_film_backward(None, None, None, None, None, *shape, 0, layout, None) == OK
    for n in (0, -5):
        assert lib.agx_sigmoid_gate(None, None, None, n, None) == OK
        assert lib.agx_sigmoid_gate_backward(None, None, None, None, None, n, None) == OK
    # a NULL required pointer
    assert lib.agx_film_params(p, None, p, p, 2, 3, 4, None) == NULL_POINTER and b"film_params" in lib.agx_last_error()
    assert lib.agx_film_params(p, p, p, None, 2, 3, 4, None) == NULL_POINTER
    assert lib.agx_film_apply(None, p, p, 2, 3, 4, 1, CT, None) == NULL_POINTER
    assert lib.agx_film_apply(p, None, p, 2, 3, 4, 0, TC, None) == NULL_POINTER
    assert lib.agx_film_apply(p, p, None, 2, 3, 4, 0, TC, None) == NULL_POINTER
    assert lib.agx_film_backward(p, p, p, p, None, 2, 3, 4, 1, CT, None) == NULL_POINTER
    assert lib.agx_film_backward(p, p, None, p, p, 2, 3, 4, 1, TC, None) == NULL_POINTER
    assert lib.agx_film_params_backward(p, p, p, None, p, p, 2, 3, 4, None) == NULL_POINTER
    assert lib.agx_film_params_backward(p, None, p, p, p, p, 2, 3, 4, None) == NULL_POINTER      # dcond asked for needs w
    assert lib.agx_sigmoid_gate(p, None, p, 5, None) == NULL_POINTER
    assert lib.agx_sigmoid_gate_backward(p, p, p, p, None, 5, None) == NULL_POINTER
    # a layout that does not exist, before anything else
    for layout in (2, -1):
        assert lib.agx_film_apply(p, p, p, 2, 3, 4, 1, layout, None) == BAD_SHAPE and b"layout" in lib.agx_last_error()
        assert lib.agx_film_backward(p, p, p, p, p, 2, 3, 4, 1, layout, None) == BAD_SHAPE
        assert lib.agx_film_apply(None, None, None, 0, 3, 4, 1, layout, None) == BAD_SHAPE
    # a shape beyond the one-dimensional grid is refused, not folded into y or z
    big = 2 ** 31 - 1
    assert lib.agx_film_params(p, p, p, p, big, 3, big, None) == BAD_SHAPE and b"grid" in lib.agx_last_error()
    assert lib.agx_film_apply(p, p, p, big, big, 4, 1, CT, None) == BAD_SHAPE
    assert lib.agx_film_backward(p, p, p, p, p, 1 << 16, 1 << 16, 4, 1, CT, None) == BAD_SHAPE
    assert lib.agx_film_backward(p, p, p, p, p, big, 1 << 10, 4, 1, TC, None) == BAD_SHAPE
    assert lib.agx_film_params_backward(p, p, p, p, p, None, 2, big, big, None) == BAD_SHAPE


def test_wrappers_refuse_mismatched_operands(monkeypatch):
    monkeypatch.setattr(ops, "_need_gpu", lambda *tensors: None)
    z = torch.zeros
    with pytest.raises(AgxError, match="gb is"):
        ops.film_apply(z(2, 5, 7), z(2, 5), True, ops.FILM_CT)
    with pytest.raises(AgxError, match="gb is"):
        ops.film_apply(z(2, 5, 7), z(2, 10), True, ops.FILM_TC)
    with pytest.raises(AgxError, match="layout"):
        ops.film_apply(z(2, 5, 7), z(2, 10), True, 2)
    with pytest.raises(AgxError, match="contiguous"):
        ops.film_apply(z(2, 7, 5).transpose(1, 2), z(2, 10), True, ops.FILM_CT)
    with pytest.raises(AgxError, match="dout is"):
        ops.film_backward(z(2, 5, 7), z(2, 10), z(2, 7, 5), True, ops.FILM_CT)
    with pytest.raises(AgxError, match="expected"):
        ops.film_params(z(2, 3), z(4, 5), None)
    with pytest.raises(AgxError, match="z of its shape"):
        ops.sigmoid_gate(z(5), z(6))
    with pytest.raises(AgxError, match="out must be"):
        ops.sigmoid_gate(z(5), z(5), out=z(6))


# ------------------------------------------------------------------------------------------------ the checker
def _close(got, want):
    want = torch.from_numpy(want)
    torch.testing.assert_close(got.float(), want, rtol=1e-6, atol=1e-6 * float(want.abs().max()))


@pytest.mark.parametrize("name", ["film", "film_nobias"])
def test_the_film_checker_reproduces_the_reference(name, g10):
    blob, _ = g10
    sd = sub_sd(blob, f"{name}/sd/")
    x, cond = torch.from_numpy(blob[f"{name}/x"]), torch.from_numpy(blob[f"{name}/cond"])
    ops64 = ref.f64(x, cond, sd["gamma.weight"], sd["gamma.bias"], sd.get("beta.weight"), sd.get("beta.bias"))
    _close(ref.film(*ops64), blob[f"{name}/out"])
    _close(ref.bct(ref.film(*ops64)), blob[f"{name}/out"].transpose(0, 2, 1).copy())


def test_the_squeeze_excite_checker_reproduces_the_reference(g10):
    blob, _ = g10
    sd = sub_sd(blob, "se/sd/")
    ops64 = ref.f64(torch.from_numpy(blob["se/x"]), sd["squeeze.weight"], sd["squeeze.bias"], sd["excite.weight"], sd["excite.bias"])
    _close(ref.squeeze_excite(*ops64), blob["se/out"])


def test_the_checkers_gradients_are_autograds_of_torchs_own_modules():
    """The gradients the device tests compare against come from autograd on the checker: the same through torch's modules."""
    torch.manual_seed(3)
    lin1, lin2 = torch.nn.Linear(6, 3).double(), torch.nn.Linear(3, 6).double()
    x, dout = torch.randn(2, 5, 6, dtype=torch.float64), torch.randn(2, 5, 6, dtype=torch.float64)
    _, grads = ref.with_grads(ref.squeeze_excite, [x, lin1.weight, lin1.bias, lin2.weight, lin2.bias], dout)
    xt = x.clone().requires_grad_(True)
    (xt * torch.sigmoid(lin2(torch.relu(lin1(xt))))).backward(dout)
    for got, want in zip(grads, [xt.grad, lin1.weight.grad, lin1.bias.grad, lin2.weight.grad, lin2.bias.grad]):
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
