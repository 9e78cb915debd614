"""``audio_generation_amd.activations`` on the host: surface, state dicts, refusals, the launches of the modules on a recording
stand-in (no kernel is launched), the return codes of the three C entry points that need no launch, and the float64 checker of
``tests/snake_ref.py`` pinned to the goldens of the reference (``tests/golden/make_goldens_snake.py``), gradients included."""
import ctypes
import json
import os

import pytest
import torch

from audio_generation_amd import _lib, activations as act, ops
from audio_generation_amd._lib import AgxError
from tests import snake_ref as ref
from tests.helpers import GOLDEN, load_npz, sub_sd
from tests.test_disc_chain_cpu import Recorder as ChainRecorder

STANDINS = ("snake_forward", "snake_backward")
OK, BAD_SHAPE, NULL_POINTER, WORKSPACE = 0, -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from audio_generation_amd import build
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def g11():
    with open(os.path.join(GOLDEN, "meta_g11.json")) as f:
        return load_npz("g11_snake.npz"), json.load(f)


def _build(meta, name):
    m = meta["models"][name]
    return getattr(act, m["class"])(m["in_channels"], dim=m["dim"])


class Recorder(ChainRecorder):
    def result(self, op, a):
        if op == "snake_forward":
            return torch.zeros_like(a["x"]) if a["out"] is None else a["out"]
        if op == "snake_backward":
            return (torch.zeros_like(a["x"]) if a["want_dx"] else None,
                    torch.zeros(a["alpha"].numel()) if a["want_dalpha"] else None)
        return super().result(op, a)


def recorded(model, mp):
    rec = Recorder(model)
    for op in STANDINS:
        mp.setattr(ops, op, rec.standin(op))
    return rec


def calls(rec):
    return [tuple(json.loads(e)) for e in rec.log]


# ------------------------------------------------------------------------------------------------ surface
@pytest.mark.parametrize("name", ["snek1", "snek2", "snekrelu1", "snekrelu2", "snek1_shared"])
def test_construction_and_state_dict_are_the_references(name, g11):
    blob, meta = g11
    model, m = _build(meta, name), meta["models"][name]
    assert type(model).__name__ == m["class"]
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == m["state_dict"]
    assert [n for n, _ in model.named_parameters()] == m["parameters"] == ["alphas"]
    assert sorted(set(model.alphas.detach().reshape(-1).tolist())) == m["initial_alphas"] == [1.0]
    assert isinstance(model.alphas, torch.nn.Parameter) and model.alphas.requires_grad
    missing, unexpected = model.load_state_dict(sub_sd(blob, f"{name}/sd/"), strict=True)
    assert missing == [] and unexpected == []
    assert torch.equal(model.alphas.detach(), torch.from_numpy(blob[f"{name}/sd/alphas"]))


def test_shapes_exports_and_the_value_error():
    assert tuple(act.Snek(7).alphas.shape) == (1, 7, 1) and tuple(act.Snek(7, dim=2).alphas.shape) == (1, 7, 1, 1)
    assert tuple(act.SnekReLU(7, 1).alphas.shape) == (1, 7, 1) and tuple(act.SnekReLU(7, 2).alphas.shape) == (1, 7, 1, 1)
    for cls in (act.Snek, act.SnekReLU):
        for dim in (0, 3, None):
            with pytest.raises(ValueError, match="Snek cannot handle such dims"):
                cls(4, dim=dim)
    import audio_generation_amd
    assert "activations" in audio_generation_amd.__all__
    assert (_lib.SNAKE_PLAIN, _lib.SNAKE_RELU) == (ops.SNAKE_PLAIN, ops.SNAKE_RELU) == (0, 1)
    import inspect
    for fn in (act.snake_activation, act.snake_relu_activation):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["x", "alpha", "eps"] and sig.parameters["eps"].default == 1e-6


# ------------------------------------------------------------------------------------------------ walks and refusals
@pytest.mark.parametrize("cls,dim,shape,match", [
    ("Snek", 1, (3, 4, 37), "has 4 channels, this layer holds 5"),
    ("SnekReLU", 1, (3, 37, 5), "has 37 channels"),
    ("Snek", 1, (3, 5, 3, 7), "expected \\(B, C, T\\)"),
    ("Snek", 2, (3, 5, 37), "expected \\(B, C, H, W\\)"),
    ("SnekReLU", 2, (3, 6, 3, 7), "has 6 channels"),
    ("Snek", 1, (5, 37), "expected \\(B, C, T\\)"),
])
@pytest.mark.parametrize("grad", [False, True])
def test_module_refusals_come_before_the_first_launch(cls, dim, shape, match, grad, monkeypatch):
    model = getattr(act, cls)(5, dim=dim)
    rec = recorded(model, monkeypatch)
    with pytest.raises(AgxError, match=match):
        model(torch.zeros(shape, requires_grad=grad))
    assert rec.log == []


def test_function_refusals(monkeypatch):
    rec = recorded(act.Snek(5), monkeypatch)
    for alpha_shape in ((1, 4, 1), (5,), (1, 5), (5, 1, 1), (1, 1, 5)):
        with pytest.raises(AgxError, match="one alpha per channel"):
            act.snake_activation(torch.zeros(3, 5, 37), torch.ones(alpha_shape))
    with pytest.raises(AgxError, match="one alpha per channel"):
        act.snake_relu_activation(torch.zeros(5, 37), torch.ones(1, 5))
    assert rec.log == []
    act.snake_activation(torch.zeros(3, 5, 37), torch.ones(1, 1, 1))         # a single alpha, as the reference broadcasts it
    act.snake_relu_activation(torch.zeros(3, 5, 37), torch.ones(()))
    assert [c[0] for c in calls(rec)] == ["snake_forward", "snake_forward"]


def test_cpu_tensors_are_refused(lib):
    for model, shape in ((act.Snek(5), (3, 5, 37)), (act.SnekReLU(5, dim=2), (3, 5, 3, 7)), (act.Snek(1), (3, 5, 37))):
        with pytest.raises(AgxError, match="MI355X only"):
            model(torch.zeros(shape))
        with pytest.raises(AgxError, match="MI355X only"):
            model(torch.zeros(shape, requires_grad=True))
    with pytest.raises(AgxError, match="MI355X only"):
        ops.snake_forward(torch.zeros(3, 5, 37), torch.ones(5), ops.SNAKE_PLAIN)
    with pytest.raises(AgxError, match="MI355X only"):
        ops.snake_backward(torch.zeros(3, 5, 37), torch.ones(5), torch.zeros(3, 5, 37), ops.SNAKE_RELU)


def test_wrappers_refuse_mismatched_operands(monkeypatch):
    monkeypatch.setattr(ops, "_need_gpu", lambda *tensors: None)
    z, one = torch.zeros, torch.ones
    with pytest.raises(AgxError, match="variant"):
        ops.snake_forward(z(2, 5, 7), one(5), 2)
    with pytest.raises(AgxError, match="\\(2, 5, 7\\) and has 5 channels, alpha \\(1, 4, 1\\) holds 4"):
        ops.snake_forward(z(2, 5, 7), one(1, 4, 1), 0)
    with pytest.raises(AgxError, match="contiguous float32"):
        ops.snake_forward(z(2, 7, 5).transpose(1, 2), one(5), 0)
    with pytest.raises(AgxError, match="contiguous float32"):
        ops.snake_forward(z(2, 5, 7, dtype=torch.float64), one(5), 0)
    with pytest.raises(AgxError, match="expected \\(B, C, ...\\)"):
        ops.snake_forward(z(7), one(1), 0)
    with pytest.raises(AgxError, match="out must be"):
        ops.snake_forward(z(2, 5, 7), one(5), 0, out=z(2, 5, 8))
    with pytest.raises(AgxError, match="out must be"):
        ops.snake_forward(z(2, 5, 7), one(5), 0, out=z(2, 5, 7, dtype=torch.float64))
    with pytest.raises(AgxError, match="dout is \\(2, 7, 5\\), x is \\(2, 5, 7\\)"):
        ops.snake_backward(z(2, 5, 7), one(5), z(2, 7, 5), 1)
    with pytest.raises(AgxError, match="expected float32"):
        ops.snake_backward(z(2, 5, 7), one(5, dtype=torch.float64), z(2, 5, 7), 1)
    with pytest.raises(AgxError, match="variant"):
        ops.snake_backward(z(2, 5, 7), one(5), z(2, 5, 7), -1)


@pytest.mark.parametrize("cls,variant", [("Snek", 0), ("SnekReLU", 1)])
@pytest.mark.parametrize("dim,shape", [(1, (3, 5, 37)), (2, (3, 5, 3, 7))])
def test_one_forward_launch_without_grad(cls, variant, dim, shape, monkeypatch):
    model = getattr(act, cls)(5, dim=dim)
    rec = recorded(model, monkeypatch)
    with torch.no_grad():
        out = model(torch.zeros(shape))
    model.requires_grad_(False)
    out2 = model(torch.zeros(shape))                       # nothing asks for a gradient: the same single launch
    log = calls(rec)
    assert [c[0] for c in log] == ["snake_forward", "snake_forward"] and out.shape == out2.shape == torch.Size(shape)
    assert log[0][1] == {"x": f"tensor{list(shape)}", "alpha": "alphas", "variant": variant, "eps": 1e-6, "out": None}
    assert not out.requires_grad and not out2.requires_grad
    rec.start()
    with torch.no_grad():
        model(torch.zeros(shape[::-1]).permute(*range(len(shape) - 1, -1, -1)))        # made contiguous, not refused
    assert [c[0] for c in calls(rec)] == ["snake_forward"]


@pytest.mark.parametrize("cls,variant", [("Snek", 0), ("SnekReLU", 1)])
def test_backward_walk_asks_only_for_what_is_needed(cls, variant, monkeypatch):
    model = getattr(act, cls)(5)
    rec = recorded(model, monkeypatch)

    def walk(x_grad, alpha_grad):
        model.requires_grad_(alpha_grad)
        model.alphas.grad = None
        x = torch.zeros(3, 5, 37, requires_grad=x_grad)
        rec.start()
        out = model(x)
        rec.mark_backward()
        out.sum().backward()
        log = calls(rec)
        assert [c[0] for c in log] == ["snake_forward", "-- backward --", "snake_backward"]          # one launch each way
        back = log[2][1]
        assert (back["variant"], back["eps"], back["alpha"], back["x"]) == (variant, 1e-6, "alphas", "tensor[3, 5, 37]")
        return back["want_dx"], back["want_dalpha"], x.grad, model.alphas.grad
    assert walk(True, True)[:2] == (True, True)
    want_dx, want_dalpha, dx, dalpha = walk(True, False)            # frozen alphas: the dx-only kernel
    assert (want_dx, want_dalpha) == (True, False) and dx is not None and dalpha is None
    want_dx, want_dalpha, dx, dalpha = walk(False, True)            # an input without grad
    assert (want_dx, want_dalpha) == (False, True) and dx is None and tuple(dalpha.shape) == (1, 5, 1)


# ------------------------------------------------------------------------------------------------ the C entry points
def test_entry_points_validate_on_the_host(lib):
    assert lib.agx_version() == 122
    buf = ctypes.create_string_buffer(64)          # never dereferenced: every call below is refused or empty
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd, bwd, query = lib.agx_snake_forward, lib.agx_snake_backward, lib.agx_snake_backward_workspace_bytes
    # an empty shape: AGX_OK and nothing launched, whatever the pointers
    for rows, n in ((0, 4), (4, 0), (-4, 4), (4, -1)):
        assert fwd(None, None, None, rows, 2, n, 0, 1e-6, None) == OK
        assert bwd(None, None, None, None, None, None, 0, rows, 2, n, 1, 1e-6, None) == OK
        assert query(rows, 2, n) == 0
    # channels, divisibility, variant
    for variant in (0, 1):
        assert fwd(p, p, p, 6, 0, 4, variant, 1e-6, None) == BAD_SHAPE and b"channels" in lib.agx_last_error()
        assert fwd(p, p, p, 6, -3, 4, variant, 1e-6, None) == BAD_SHAPE
        assert fwd(p, p, p, 6, 4, 4, variant, 1e-6, None) == BAD_SHAPE and b"multiple" in lib.agx_last_error()
        assert bwd(p, p, p, p, p, p, 64, 6, 0, 4, variant, 1e-6, None) == BAD_SHAPE
        assert bwd(p, p, p, p, p, p, 64, 6, 4, 4, variant, 1e-6, None) == BAD_SHAPE
    for variant in (2, -1):
        assert fwd(p, p, p, 6, 3, 4, variant, 1e-6, None) == BAD_SHAPE and b"variant" in lib.agx_last_error()
        assert bwd(p, p, p, p, p, p, 64, 6, 3, 4, variant, 1e-6, None) == BAD_SHAPE
    assert query(6, 4, 4) == 0 and query(6, 0, 4) == 0
    # a NULL required pointer
    assert fwd(None, p, p, 6, 3, 4, 0, 1e-6, None) == NULL_POINTER and b"snake_forward" in lib.agx_last_error()
    assert fwd(p, None, p, 6, 3, 4, 0, 1e-6, None) == NULL_POINTER
    assert fwd(p, p, None, 6, 3, 4, 0, 1e-6, None) == NULL_POINTER
    assert bwd(p, p, None, p, p, p, 64, 6, 3, 4, 0, 1e-6, None) == NULL_POINTER
    assert bwd(None, p, p, p, None, None, 0, 6, 3, 4, 0, 1e-6, None) == NULL_POINTER
    assert bwd(p, p, p, None, None, None, 0, 6, 3, 4, 0, 1e-6, None) == OK          # neither gradient asked for
    # the workspace: one float per (row, segment), asked for only with dalpha
    assert query(6, 3, 4) == 4 * 6 and query(6, 3, ref.SEGMENT) == 4 * 6 and query(6, 3, ref.SEGMENT + 1) == 4 * 12
    assert query(32, 32, 72000) == 4 * 32 * 36 and query(6, 1, 4) == 4 * 6
    assert bwd(p, p, p, p, p, p, 4 * 6 - 1, 6, 3, 4, 0, 1e-6, None) == WORKSPACE and b"workspace" in lib.agx_last_error()
    assert bwd(p, p, p, None, p, p, 0, 6, 3, 4, 1, 1e-6, None) == WORKSPACE
    assert bwd(p, p, p, p, p, None, 64, 6, 3, 4, 1, 1e-6, None) == WORKSPACE
    # a shape beyond the one-dimensional grid is refused before anything is launched
    big = 2 ** 31
    assert fwd(p, p, p, 4 * big, 1, 1, 0, 1e-6, None) == BAD_SHAPE and b"grid" in lib.agx_last_error()
    assert fwd(p, p, p, 8, 1, 1024 * big, 0, 1e-6, None) == BAD_SHAPE
    assert bwd(p, p, p, p, None, None, 0, 4 * big, 1, 1, 0, 1e-6, None) == BAD_SHAPE
    assert bwd(p, p, p, p, p, p, 64, big, 1, 1, 0, 1e-6, None) == BAD_SHAPE and b"grid" in lib.agx_last_error()
    assert bwd(p, p, p, p, p, p, 64, 2, 1, ref.SEGMENT * big, 0, 1e-6, None) == BAD_SHAPE
    assert query(big, 1, 1) == 0


# ------------------------------------------------------------------------------------------------ the checker
def _within(got, want, bound, what):
    err = (got - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: worst error / bound = {worst:.3f}")
    assert bool((err <= bound).all()), (what, worst)


@pytest.mark.parametrize("name", ["snek1", "snek2", "snekrelu1", "snekrelu2", "snek1_shared"])
def test_the_checker_reproduces_the_reference(name, g11):
    """The float64 formulas against the reference's fp32 forward and autograd, within 1 x the fp32 bounds of tests/snake_ref.py
    (``split=True``: autograd sums the two halves of dalpha apart).  SnekReLU's gradient at both zeros is the incoming one."""
    blob, meta = g11
    m = meta["models"][name]
    relu = m["class"] == "SnekReLU"
    x, alpha, dout = ref.f64(blob[f"{name}/x"], blob[f"{name}/sd/alphas"], blob[f"{name}/dout"])
    assert float(x.reshape(-1)[0]) == 0.0 and float(x.reshape(-1)[1]) == 0.0 and meta["eps"] == ref.EPS
    d_out, d_dx, d_dalpha = ref.bounds(x, alpha, dout, relu, split=True)
    dx, dalpha = ref.snake_backward(x, alpha, dout, relu)
    _within(ref.snake(x, alpha, relu), ref.f64(blob[f"{name}/out"]), d_out, "out")
    _within(dx, ref.f64(blob[f"{name}/dx"]), d_dx, "dx")
    _within(dalpha, ref.f64(blob[f"{name}/dalphas"]).reshape(-1), d_dalpha, "dalpha")
    assert torch.equal(torch.from_numpy(blob[f"{name}/dx"]).reshape(-1)[:2], torch.from_numpy(blob[f"{name}/dout"]).reshape(-1)[:2])
    assert torch.equal(dx.reshape(-1)[:2], dout.reshape(-1)[:2])


def test_the_checkers_gradients_are_autograds():
    torch.manual_seed(3)
    x = torch.randn(2, 3, 4, 5, dtype=torch.float64)
    x.view(-1)[:2] = torch.tensor([0.0, -0.0], dtype=torch.float64)
    dout = torch.randn_like(x)
    for relu in (False, True):
        for alpha in (torch.tensor([0.7, -1.3, 2.1], dtype=torch.float64), torch.tensor([0.9], dtype=torch.float64)):
            xt, at = x.clone().requires_grad_(True), alpha.clone().requires_grad_(True)
            a = at.reshape(1, -1, 1, 1)
            ((torch.clamp(xt, 0) if relu else xt) + (1 / (a + 1e-6)) * torch.sin(a * xt) ** 2).backward(dout)
            dx, dalpha = ref.snake_backward(x, alpha, dout, relu)
            torch.testing.assert_close(dx, xt.grad, rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(dalpha, at.grad, rtol=1e-11, atol=1e-11)
            torch.testing.assert_close(ref.partial_sums(x, alpha, dout, relu).reshape(2, alpha.numel() if alpha.numel() > 1 else 3, -1)
                                       .sum((0, 2) if alpha.numel() > 1 else (0, 1, 2)).reshape(-1), dalpha, rtol=1e-11, atol=1e-11)
