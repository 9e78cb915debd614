"""``Snek`` / ``SnekReLU`` on the device against the float64 checker of ``tests/snake_ref.py``.

Tolerances are derived, not measured: the docstring of ``tests/snake_ref.py`` states them term by term (the rounding of
theta = a x carried through sin^2 and sin 2 theta, the error K_SIN = 24 u of the device's sine pair from OCML's 4 ulp, the
roundings of 1 / (a + eps) and of the products, and (N + 2) u sum |term| for the N summed terms of dalpha).  Every right-hand
side is evaluated in float64 from the operands and a check allows 2 x it.  Against the goldens the allowance is the device's
2 x plus 1 x the same bound for the reference's own fp32 evaluation (``split=True`` for its dalpha).  The shipped sine is
libm's on every argument, so there is no fast-path threshold to straddle.

Cases are (B, C, inner, shared): B in {1, 3}, C in {1, 5, 130}, T in {1, 3, 37, 1029, 2049} for ``dim=1`` and (H, W) in
{(3, 5), (7, 37)} for ``dim=2``; T = 1 a single element per row, 3 a ragged tail, 37 misaligned rows, 1029 more than one
1024-float segment of the element-wise walk, 2049 one float more than a reduction segment.  ``shared``: one alpha for every
channel.  The alpha of channel c is ALPHAS[(c + case) % 6]; x is 2 * randn with, at the head of every row, exact +-0, both
signs, theta within 1e-3 of multiples of pi / 2 and (in every other case) |theta| up to 1e6.
"""
import json
import math
import os

import pytest
import torch

from audio_generation_amd import activations as act, ops
from tests import snake_ref as ref
from tests.helpers import GOLDEN, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALPHAS = (0.0, 1.0, -2.5, 7.3, 1e-3, 40.0)
CASES = [(1, 1, (1,), False), (3, 5, (3,), False), (1, 130, (37,), False), (3, 5, (1029,), False), (1, 5, (2049,), False),
         (3, 130, (1,), False), (1, 1, (1029,), False), (3, 1, (37,), False), (3, 130, (2049,), False), (3, 5, (37,), True),
         (3, 5, (3, 5), False), (1, 130, (7, 37), False), (3, 1, (7, 37), False), (1, 5, (7, 37), True)]
_CASES = {}


def _ids(case):
    return "x".join(map(str, case[:2] + case[2])) + ("-shared" if case[3] else "")


def _specials(a, far):
    if a == 0.0:
        return [0.0, -0.0, 5.0, -5.0, 1e4]
    s = [0.0, -0.0] + [(k * math.pi / 2 + d) / a for k, d in ((1, 5e-4), (2, -5e-4), (-3, 2e-4), (101, -1e-3), (-200, 1e-4))]
    return s + ([1e6 / a, -0.999e6 / a, 3.1e4 / a] if far else [60.0 / a])


def _case(case):
    """Operands and the float64 results of both variants, computed once per case."""
    if case not in _CASES:
        b, c, inner, shared = case
        k = CASES.index(case)
        gen = torch.Generator().manual_seed(100 + k)
        channels = 1 if shared else c
        alpha = torch.tensor([ALPHAS[(ch + k) % len(ALPHAS)] for ch in range(channels)])
        n = math.prod(inner)
        x, dout = 2.0 * torch.randn(b * c, n, generator=gen), torch.randn(b * c, n, generator=gen)
        for row in range(b * c):
            s = _specials(float(alpha[row % channels]), far=(k % 2 == 0))
            for j in range(min(n, len(s))):
                x[row, j] = s[(j + row) % len(s)]
        x, dout = x.reshape(b, c, *inner), dout.reshape(b, c, *inner)
        x64, a64, d64 = ref.f64(x, alpha, dout)
        want = {}
        for relu in (False, True):
            dx, dalpha = ref.snake_backward(x64, a64, d64, relu)
            want[relu] = dict(out=ref.snake(x64, a64, relu), dx=dx, dalpha=dalpha, bounds=ref.bounds(x64, a64, d64, relu))
        _CASES[case] = dict(x=x, alpha=alpha, dout=dout, want=want)
    return _CASES[case]


def _within(got, want, bound, what):
    """|got - want| <= 2 * bound elementwise (float64), and no NaN / Inf."""
    got = got.detach().cpu().double()
    assert bool(torch.isfinite(got).all()), what
    err, allow = (got - want).abs(), 2.0 * bound
    worst = float((err / allow.clamp_min(1e-300)).max())
    print(f"{what}: worst error / allowance = {worst:.3f}, largest error {float(err.max()):.3e}")
    assert bool((err <= allow).all()), (what, worst)


@pytest.mark.parametrize("relu", [False, True], ids=["snek", "snekrelu"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_forward_and_backward_against_the_checker(case, relu):
    k = _case(case)
    variant = ops.SNAKE_RELU if relu else ops.SNAKE_PLAIN
    x, alpha, dout = k["x"].to(DEV), k["alpha"].to(DEV), k["dout"].to(DEV)
    want, (d_out, d_dx, d_dalpha) = k["want"][relu], k["want"][relu]["bounds"]
    out = ops.snake_forward(x, alpha, variant)
    dx, dalpha = ops.snake_backward(x, alpha, dout, variant)
    assert out.shape == x.shape and dx.shape == x.shape and tuple(dalpha.shape) == (alpha.numel(),)
    _within(out, want["out"], d_out, "out")
    _within(dx, want["dx"], d_dx, "dx")
    _within(dalpha, want["dalpha"], d_dalpha, "dalpha")

    # two identical calls, the partial calls and the in-place forms: the same bits
    dx2, dalpha2 = ops.snake_backward(x, alpha, dout, variant)
    assert torch.equal(ops.snake_forward(x, alpha, variant), out) and torch.equal(dx2, dx) and torch.equal(dalpha2, dalpha)
    dx_only, none = ops.snake_backward(x, alpha, dout, variant, want_dalpha=False)
    assert none is None and torch.equal(dx_only, dx)
    none, dalpha_only = ops.snake_backward(x, alpha, dout, variant, want_dx=False)
    assert none is None and torch.equal(dalpha_only, dalpha)
    assert ops.snake_backward(x, alpha, dout, variant, want_dx=False, want_dalpha=False) == (None, None)
    inplace = x.clone()
    assert ops.snake_forward(inplace, alpha, variant, out=inplace) is inplace and torch.equal(inplace, out)

    # exact facts: a channel with alpha == 0, and the zero point of the clamp
    xc, dc, outc, dxc = x.cpu(), dout.cpu(), out.cpu(), dx.cpu()
    mask = (xc >= 0).float() if relu else torch.ones_like(xc)
    zero_rows = (k["alpha"].reshape(1, -1, *[1] * len(case[2])) == 0).expand_as(xc)
    if bool(zero_rows.any()):
        assert torch.equal(outc[zero_rows], torch.clamp(xc, min=0.0)[zero_rows] if relu else xc[zero_rows])
        assert torch.equal(dxc[zero_rows], (dc * mask)[zero_rows])
        assert bool((dalpha.cpu()[k["alpha"] == 0] == 0).all())
    at_zero = xc == 0
    assert int(at_zero.sum()) >= 1 or math.prod(case[2]) < 2
    assert torch.equal(dxc[at_zero], dc[at_zero])                                   # both variants: sin 0 = 0 and [0 >= 0] = 1

    # dim = 1 on (B, C, H * W) and dim = 2 on (B, C, H, W): the same data, the same bits
    if len(case[2]) == 2:
        flat = lambda v: v.reshape(*v.shape[:2], -1)        # noqa: E731
        assert torch.equal(ops.snake_forward(flat(x), alpha, variant), flat(out))
        dx1, dalpha1 = ops.snake_backward(flat(x), alpha, flat(dout), variant)
        assert torch.equal(dx1, flat(dx)) and torch.equal(dalpha1, dalpha)


@pytest.mark.parametrize("relu", [False, True], ids=["snek", "snekrelu"])
def test_unequally_aligned_operands_give_the_same_bits(relu):
    """x, dout and the outputs at different offsets from a 16-byte boundary (the all-scalar walk, and every head length of the
    vector walk): out and dx are the same bits, and dalpha too -- its order goes by index, not by address.  Nothing outside
    the outputs is written."""
    k = _case(CASES[3])
    variant = ops.SNAKE_RELU if relu else ops.SNAKE_PLAIN
    x, alpha, dout = k["x"].to(DEV), k["alpha"].to(DEV), k["dout"].to(DEV)
    out = ops.snake_forward(x, alpha, variant)
    dx, dalpha = ops.snake_backward(x, alpha, dout, variant)

    def shifted(v, off):
        buf = torch.full((v.numel() + 8,), 7.0, device=DEV)
        buf[off:off + v.numel()] = v.reshape(-1)
        return buf, buf[off:off + v.numel()].view(v.shape)
    for x_off, d_off, out_off in ((1, 1, 1), (0, 0, 1), (1, 0, 0), (3, 3, 3), (2, 1, 3), (0, 2, 0)):
        (_, xs), (_, ds) = shifted(x, x_off), shifted(dout, d_off)
        obuf, o = shifted(torch.zeros_like(x), out_off)
        ops.snake_forward(xs, alpha, variant, out=o)
        assert torch.equal(o, out), (x_off, out_off)
        assert bool((obuf[:out_off] == 7.0).all()) and bool((obuf[out_off + x.numel():] == 7.0).all())
        dx_only, _ = ops.snake_backward(xs, alpha, ds, variant, want_dalpha=False)
        dx2, dalpha2 = ops.snake_backward(xs, alpha, ds, variant)
        assert torch.equal(dx_only, dx) and torch.equal(dx2, dx) and torch.equal(dalpha2, dalpha), (x_off, d_off)


@pytest.mark.parametrize("relu", [False, True], ids=["snek", "snekrelu"])
def test_a_nan_and_an_inf_stay_where_they_are(relu):
    k = _case(CASES[3])                                   # (3, 5, 1029)
    variant = ops.SNAKE_RELU if relu else ops.SNAKE_PLAIN
    x, alpha, dout = k["x"].to(DEV), k["alpha"].to(DEV), k["dout"].to(DEV)
    out = ops.snake_forward(x, alpha, variant)
    dx, dalpha = ops.snake_backward(x, alpha, dout, variant)
    bad = x.clone()
    bad[1, 1, 500] = float("nan")
    bad[2, 3, 1028] = float("-inf")
    planted = torch.zeros_like(x, dtype=torch.bool)
    planted[1, 1, 500] = planted[2, 3, 1028] = True
    out_b = ops.snake_forward(bad, alpha, variant)
    dx_b, dalpha_b = ops.snake_backward(bad, alpha, dout, variant)
    dx_only, _ = ops.snake_backward(bad, alpha, dout, variant, want_dalpha=False)
    torch.cuda.synchronize()                              # the calls return
    for got, clean in ((out_b, out), (dx_b, dx), (dx_only, dx)):
        assert not bool(torch.isfinite(got[planted]).any())
        assert torch.equal(got[~planted].view(torch.int32), clean[~planted].view(torch.int32))
    hit = torch.tensor([False, True, False, True, False], device=DEV)
    assert bool(torch.isnan(dalpha_b[hit]).all())
    assert torch.equal(dalpha_b[~hit].view(torch.int32), dalpha[~hit].view(torch.int32))


# ------------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize("name", ["snek1", "snek2", "snekrelu1", "snekrelu2", "snek1_shared"])
def test_goldens_through_the_hip_modules(name):
    """The reference's own inputs, alphas, outputs and gradients.  The device is within 2 x its bound of the exact result and
    the golden, an fp32 evaluation, within 1 x its own."""
    blob = load_npz("g11_snake.npz")
    with open(os.path.join(GOLDEN, "meta_g11.json")) as f:
        m = json.load(f)["models"][name]
    relu = m["class"] == "SnekReLU"
    model = getattr(act, m["class"])(m["in_channels"], dim=m["dim"])
    model.load_state_dict({"alphas": torch.from_numpy(blob[f"{name}/sd/alphas"])}, strict=True)
    model = model.to(DEV)
    x = torch.from_numpy(blob[f"{name}/x"]).to(DEV).requires_grad_(True)
    out = model(x)
    out.backward(torch.from_numpy(blob[f"{name}/dout"]).to(DEV))
    x64, a64, d64 = ref.f64(blob[f"{name}/x"], blob[f"{name}/sd/alphas"], blob[f"{name}/dout"])
    dev, gold = ref.bounds(x64, a64, d64, relu), ref.bounds(x64, a64, d64, relu, split=True)
    dx64, dalpha64 = ref.snake_backward(x64, a64, d64, relu)
    got = (out.detach(), x.grad, model.alphas.grad.reshape(-1))
    for what, g, exact, key, bd, bg in zip(("out", "dx", "dalpha"), got, (ref.snake(x64, a64, relu), dx64, dalpha64),
                                           ("out", "dx", "dalphas"), dev, gold):
        _within(g, exact, bd, f"{name} {what} vs checker")
        _within(g, ref.f64(blob[f"{name}/{key}"]).reshape(exact.shape), bd + 0.5 * bg, f"{name} {what} vs golden")
    assert model.alphas.grad.shape == model.alphas.shape


# ------------------------------------------------------------------------------------------------ autograd plumbing, graphs
@pytest.mark.parametrize("cls,variant", [(act.Snek, ops.SNAKE_PLAIN), (act.SnekReLU, ops.SNAKE_RELU)], ids=["snek", "snekrelu"])
@pytest.mark.parametrize("case", [CASES[3], CASES[9], CASES[11]], ids=_ids)
def test_modules_are_the_ops_through_autograd(case, cls, variant):
    k = _case(case)
    b, c, inner, shared = case
    model = cls(1 if shared else c, dim=len(inner)).to(DEV)
    with torch.no_grad():
        model.alphas.copy_(k["alpha"].reshape(model.alphas.shape))
    x, dout = k["x"].to(DEV), k["dout"].to(DEV)
    out = ops.snake_forward(x, model.alphas.detach(), variant)
    dx, dalpha = ops.snake_backward(x, model.alphas.detach(), dout, variant)
    xg = x.clone().requires_grad_(True)
    got = model(xg)
    got.backward(dout)
    assert torch.equal(got, out) and torch.equal(xg.grad, dx) and torch.equal(model.alphas.grad, dalpha.view(model.alphas.shape))
    with torch.no_grad():
        assert torch.equal(model(x), out) and not model(x).requires_grad
    model.alphas.grad = None                              # an input without grad: the sums alone
    model(x).backward(dout)
    assert torch.equal(model.alphas.grad, dalpha.view(model.alphas.shape))
    model.requires_grad_(False)                           # frozen alphas: dx alone
    xg = x.clone().requires_grad_(True)
    model(xg).backward(dout)
    assert torch.equal(xg.grad, dx) and model.alphas.grad is not None and not model(x).requires_grad
    xt = x.transpose(0, 1).contiguous().transpose(0, 1)   # not contiguous: made contiguous
    assert not xt.is_contiguous() or b == 1
    assert torch.equal(model(xt), out)
    fn = act.snake_relu_activation if variant else act.snake_activation
    assert torch.equal(fn(x, model.alphas), out)


def test_a_captured_forward_and_backward_replay_on_new_data():
    """One capture of ``Snek`` -> ``SnekReLU(dim=2)`` forward and of the full backward op at (2, 5, 2049): a single-branch graph
    with no host reads (the workspace comes from the allocator's graph pool).  The operands are overwritten in place and the
    replay equals the eager result bitwise."""
    torch.manual_seed(4)
    s1, s2 = act.Snek(5).to(DEV), act.SnekReLU(5, dim=2).to(DEV)
    with torch.no_grad():
        s1.alphas.copy_(torch.tensor([0.0, 1.0, -2.5, 7.3, 40.0], device=DEV).view(1, 5, 1))
    x, dout = torch.randn(2, 5, 2049, device=DEV), torch.randn(2, 5, 2049, device=DEV)

    def run():
        out = s2(s1(x).view(2, 5, 3, 683))
        return (out,) + ops.snake_backward(x, s1.alphas.detach(), dout, ops.SNAKE_PLAIN)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            first = run()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = run()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs, first))
        x.copy_(2.0 * torch.randn(2, 5, 2049, device=DEV))
        dout.copy_(torch.randn(2, 5, 2049, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in outs]
        assert all(torch.equal(a, b) for a, b in zip(replayed, run())) and not torch.equal(replayed[0], first[0])
