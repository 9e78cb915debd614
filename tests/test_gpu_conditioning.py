"""``FiLM`` and ``SqueezeExcite`` on the device against the float64 checker of ``tests/conditioning_ref.py``.

Tolerances are derived, not measured.  With u = 2^-24, an fp32 sum of n products in any order, with or without fma, is within
(n + 2) u sum|a_i b_i| of the exact one; every right-hand side below is evaluated in float64 and a check allows 2 x it.

FiLM (``_film_bounds``):
    gb    n = D + 1 over |cond| |w| + |bias|
    out   |x| d_gamma + d_beta + 3 u (|x gamma| + |beta|)                  (the projections' errors carried through one fma)
    dx    |dout| d_gamma + u |dout gamma|                                   (one rounded product of the device's gamma)
    dgb   n = T over |dout x| and over |dout|                               (the operands are exact: x and dout)
    dw, dbias  n = B;   dcond  n = R                                        (against float64 arithmetic on the device's dgb)
The gate: 16 u relative on out and dx (plus 2^-126: below the smallest normal fp32 has no relative precision, and a sigmoid
that is 4e-44 in float64 is exactly 0 in fp32), 16 u |dout x| absolute on dz because s (1 - s) <= 1 / 4.
SqueezeExcite forward (``_se_bound``): d_h <= (C + 2) u (|W1| |x| + |b1|), d_z <= (Hd + 2) u (|W2| |h| + |b2|) + |W2| d_h,
d_out <= |x| (d_z / 4 + 16 u).  Its gradients: the criterion of tests/test_gpu_training.py, restated in ``_grad_close``.
"""
import json
import os

import pytest
import torch

from audio_generation_amd import conditioning as cd, ops
from tests import conditioning_ref as ref
from tests.conditioning_ref import U
from tests.helpers import GOLDEN, load_npz, sub_sd

pytestmark = pytest.mark.gpu
DEV = "cuda"
TINY = 2.0 ** -126

# (B, C, T, D, bias): every value of B in {1, 3}, C in {1, 5, 24, 130}, T in {1, 3, 37, 1029}, D in {1, 20, 130} and both
# bias settings; each case runs in both layouts.  T = 1 a single element per row, 3 a ragged tail, 37 misaligned CT rows,
# 1029 more than one pass of a 256-thread workgroup (and of a 1024-float segment) over a row.
FILM_CASES = [(1, 1, 1, 1, True), (3, 5, 3, 20, True), (1, 24, 37, 20, False), (3, 130, 1029, 130, True), (1, 5, 1029, 1, False),
              (3, 1, 37, 130, True), (1, 130, 3, 20, False), (3, 24, 1, 130, True), (1, 24, 1029, 20, True), (3, 5, 37, 1, False),
              (1, 130, 37, 130, True), (3, 1, 1029, 20, False)]


def _within(got, want, bound, what):
    """|got - want| <= 2 * bound elementwise (float64), and no NaN / Inf."""
    got = got.detach().cpu().double()
    assert bool(torch.isfinite(got).all()), what
    err, allow = (got - want).abs(), 2.0 * bound
    worst = float((err / allow.clamp_min(1e-300)).max())
    print(f"{what}: worst error / allowance = {worst:.3f}, largest error {float(err.max()):.3e}")
    assert bool((err <= allow).all()), (what, worst)


def _film(case, seed=0):
    b, c, t, d, bias = case
    torch.manual_seed(seed + sum(case[:4]))
    film = cd.FiLM(d, c, bias=bias)
    return film, torch.randn(b, t, c), torch.randn(b, d), torch.randn(b, t, c)


def _film_run(film, x, cond, dout, layout):
    """The module on the device in one layout: everything moved back to the reference layout (B, L, C)."""
    film = film.to(DEV)
    for p in film.parameters():
        p.grad = None
    xd = (x if layout == ops.FILM_TC else ref.bct(x)).clone().to(DEV).requires_grad_(True)
    cd_ = cond.clone().to(DEV).requires_grad_(True)
    out = film(xd, cd_) if layout == ops.FILM_TC else film.run_bct(xd, cd_)
    out.backward((dout if layout == ops.FILM_TC else ref.bct(dout)).to(DEV))
    back = (lambda v: v) if layout == ops.FILM_TC else ref.bct
    return dict(out=back(out.detach()), dx=back(xd.grad), dcond=cd_.grad, params=[p.grad.clone() for p in film.parameters()])


@pytest.mark.parametrize("case", FILM_CASES, ids=lambda c: "x".join(map(str, c[:4])) + ("" if c[4] else "-nobeta"))
def test_film_forward_and_backward_in_both_layouts(case):
    b, c, t, d, bias = case
    film, x, cond, dout = _film(case)
    tc, ct = _film_run(film, x, cond, dout, ops.FILM_TC), _film_run(film, x, cond, dout, ops.FILM_CT)
    # the two layouts: the same arithmetic per element and the same reduction order per (b, c), hence the same bits
    for key in ("out", "dx", "dcond"):
        assert torch.equal(tc[key], ct[key]), key
    assert all(torch.equal(p, q) for p, q in zip(tc["params"], ct["params"]))

    wg, bg = film.gamma.weight.detach().cpu(), film.gamma.bias.detach().cpu()
    wb, bb = (film.beta.weight.detach().cpu(), film.beta.bias.detach().cpu()) if bias else (None, None)
    x64, cond64, dout64, wg64, bg64, wb64, bb64 = ref.f64(x, cond, dout, wg, bg, wb, bb)
    gamma, beta = ref.film_gb(cond64, wg64, bg64, wb64, bb64)
    d_gamma = (d + 3) * U * (cond64.abs() @ wg64.abs().T + bg64.abs())
    d_beta = (d + 3) * U * (cond64.abs() @ wb64.abs().T + bb64.abs()) if bias else torch.zeros_like(gamma)
    beta0 = beta if bias else torch.zeros_like(gamma)

    # the projections (the op the module ran, with the module's stacked image: deterministic, so the same bits)
    w, bvec = film._stacked.get()
    gb = ops.film_params(cond.to(DEV), w, bvec)
    _within(gb[:, :c], gamma, d_gamma, "gamma")
    if bias:
        _within(gb[:, c:], beta, d_beta, "beta")
    # forward
    want = ref.film(x64, cond64, wg64, bg64, wb64, bb64)
    bound = x64.abs() * d_gamma[:, None, :] + d_beta[:, None, :] + 3 * U * ((x64 * gamma[:, None, :]).abs() + beta0[:, None, :].abs())
    _within(tc["out"], want, bound, "out")
    # dx = dout * gamma
    _within(tc["dx"], dout64 * gamma[:, None, :], dout64.abs() * d_gamma[:, None, :] + U * (dout64 * gamma[:, None, :]).abs(), "dx")
    # the per-(b, c) sums: exact operands
    dx_op, dgb = ops.film_backward(x.to(DEV), gb, dout.to(DEV), bias, ops.FILM_TC)
    assert torch.equal(dx_op, tc["dx"])
    _within(dgb[:, :c], (dout64 * x64).sum(1), (t + 2) * U * (dout64 * x64).abs().sum(1), "dgamma")
    if bias:
        _within(dgb[:, c:], dout64.sum(1), (t + 2) * U * dout64.abs().sum(1), "dbeta")
    # the projections' backward against float64 arithmetic on the device's dgb
    dgb64, w64 = ref.f64(dgb.cpu(), w.cpu())
    r = w64.shape[0]
    dw, dbias, dcond = (v.cpu() for v in ops.film_params_backward(cond.to(DEV), w, dgb))
    _within(dw, dgb64.T @ cond64, (b + 2) * U * (dgb64.abs().T @ cond64.abs()), "dw")
    _within(dbias, dgb64.sum(0), (b + 2) * U * dgb64.abs().sum(0), "dbias")
    _within(dcond, dgb64 @ w64, (r + 2) * U * (dgb64.abs() @ w64.abs()), "dcond")
    # ... which is what the module returned, in parameters() order
    assert torch.equal(dcond, tc["dcond"].cpu())
    grads = [dw[:c], dbias[:c]] + ([dw[c:], dbias[c:]] if bias else [])
    assert all(torch.equal(g, p.cpu()) for g, p in zip(grads, tc["params"])) and len(grads) == len(tc["params"])


@pytest.mark.parametrize("layout", [ops.FILM_CT, ops.FILM_TC])
def test_film_apply_in_place_and_on_unequally_aligned_operands(layout):
    """``out is x``, and x / out at different offsets from a 16-byte boundary (the all-scalar path): the same bits."""
    torch.manual_seed(5)
    b, c, t = 2, 5, 1029
    shape = (b, c, t) if layout == ops.FILM_CT else (b, t, c)
    x, gb = torch.randn(shape, device=DEV), torch.randn(b, 2 * c, device=DEV)
    want = ops.film_apply(x, gb, True, layout)
    g = gb[:, :c].reshape(b, c, 1) if layout == ops.FILM_CT else gb[:, :c].reshape(b, 1, c)
    be = gb[:, c:].reshape(b, c, 1) if layout == ops.FILM_CT else gb[:, c:].reshape(b, 1, c)
    _within(want, (x.double() * g.double() + be.double()).cpu(), (3 * U * ((x.double() * g.double()).abs() + be.double().abs())).cpu(), "apply")
    for x_off, out_off in ((0, 1), (1, 0), (1, 1), (3, 2)):
        xs = torch.zeros(x.numel() + 4, device=DEV)
        xs[x_off:x_off + x.numel()] = x.reshape(-1)
        outs = torch.full((x.numel() + 8,), 7.0, device=DEV)
        out = outs[out_off:out_off + x.numel()].view(shape)
        ops.film_apply(xs[x_off:x_off + x.numel()].view(shape), gb, True, layout, out=out)
        assert torch.equal(out, want), (x_off, out_off)
        assert bool((outs[:out_off] == 7.0).all()) and bool((outs[out_off + x.numel():] == 7.0).all())
    inplace = x.clone()
    assert ops.film_apply(inplace, gb, True, layout, out=inplace) is inplace and torch.equal(inplace, want)


# ------------------------------------------------------------------------------------------------ the gate
def _gate_operands(n):
    gen = torch.Generator().manual_seed(n)
    x, dout = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    z = 3.0 * torch.randn(n, generator=gen)
    special = torch.tensor([0.0, 20.0, -20.0, 100.0, -100.0])[:n]
    z[:special.numel()] = special
    return x, z, dout


@pytest.mark.parametrize("n", [1, 3, 1029])
def test_sigmoid_gate_and_its_backward(n):
    x, z, dout = _gate_operands(n)
    x64, z64, d64 = ref.f64(x, z, dout)
    s = ref.sigmoid(z64)
    xd, zd, dd = x.to(DEV), z.to(DEV), dout.to(DEV)
    out = ops.sigmoid_gate(xd, zd)
    dx, dz = ops.sigmoid_gate_backward(xd, zd, dd)
    _within(out, x64 * s, 0.5 * (16 * U * (x64 * s).abs() + TINY), "gate out")       # _within allows 2 x its bound
    _within(dx, d64 * s, 0.5 * (16 * U * (d64 * s).abs() + TINY), "gate dx")
    _within(dz, d64 * x64 * s * (1 - s), 0.5 * 16 * U * (d64 * x64).abs(), "gate dz")
    hi, lo = (z == 100.0), (z == -100.0)         # expf overflows to inf or underflows to 0: the sigmoid is exactly 1 or 0
    assert torch.equal(out.cpu()[hi], x[hi]) and torch.equal(dx.cpu()[hi], dout[hi]) and bool((dz.cpu()[hi] == 0).all())
    assert bool((out.cpu()[lo] == 0).all()) and bool((dx.cpu()[lo] == 0).all()) and bool((dz.cpu()[lo] == 0).all())
    inplace = xd.clone()
    assert ops.sigmoid_gate(inplace, zd, out=inplace) is inplace and torch.equal(inplace, out)
    if n > 4:                                    # operands off the 16-byte boundary: the scalar path, the same bits
        pad = lambda v: torch.cat([torch.zeros(1), v]).to(DEV)[1:]     # noqa: E731
        assert torch.equal(ops.sigmoid_gate(pad(x), pad(z)), out)
        dx2, dz2 = ops.sigmoid_gate_backward(pad(x), pad(z), pad(dout))
        assert torch.equal(dx2, dx) and torch.equal(dz2, dz)


# ------------------------------------------------------------------------------------------------ SqueezeExcite
SE_CASES = [(24, 2, 3, 1), (130, 4, 37, 3), (512, 2, 225, 1), (24, 2, 225, 3)]      # (dim, scale_factor, T, B)
_SE = {}


def _se_case(case):
    """Operands, the float64 result and gradients, and the fp32 CPU evaluation of the same restatement: computed once."""
    if case not in _SE:
        dim, scale, t, b = case
        torch.manual_seed(sum(case))
        se = cd.SqueezeExcite(dim, scale)
        x, dout = torch.randn(b, t, dim), torch.randn(b, t, dim)
        params = [p.detach().clone() for p in se.parameters()]
        out64, g64 = ref.with_grads(ref.squeeze_excite, list(ref.f64(x, *params)), dout)
        _, g32 = ref.with_grads(ref.squeeze_excite, [x] + params, dout)
        _SE[case] = dict(se=se, x=x, dout=dout, params=params, out64=out64, g64=g64, g32=g32)
    return _SE[case]


def _se_bound(x, w1, b1, w2, b2):
    x, w1, b1, w2, b2 = ref.f64(x, w1, b1, w2, b2)
    c, hd = w1.shape[1], w1.shape[0]
    hidden = torch.clamp(x @ w1.T + b1, min=0.0)
    d_h = (c + 2) * U * (x.abs() @ w1.abs().T + b1.abs())
    d_z = (hd + 2) * U * (hidden.abs() @ w2.abs().T + b2.abs()) + d_h @ w2.abs().T
    return x.abs() * (d_z / 4 + 16 * U)


def _grad_close(name, got, w32, w64):
    """tests/test_gpu_training.py's criterion: within 2e-4 of the exact gradient relative to its largest element, or no
    further from it than 3 x the fp32 CPU evaluation's own distance."""
    got, w32 = got.detach().cpu().double(), w32.double()
    scale = float(w64.abs().max()) + 1e-12
    err, noise = float((got - w64).abs().max()), float((w32 - w64).abs().max())
    print(f"{name}: err / scale = {err / scale:.3e}, fp32 noise / scale = {noise / scale:.3e}")
    assert err <= max(2e-4 * scale, 3.0 * noise) + 1e-9, (name, err / scale, noise / scale)


@pytest.mark.parametrize("case", SE_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("entry", ["run_bct", "forward"])
def test_squeeze_excite_forward_and_gradients(case, entry):
    k = _se_case(case)
    se = k["se"].to(DEV)
    for p in se.parameters():
        p.grad = None
    to, back = (ref.bct, ref.bct) if entry == "run_bct" else ((lambda v: v), (lambda v: v))
    xd = to(k["x"]).clone().to(DEV).requires_grad_(True)
    out = getattr(se, entry)(xd)
    out.backward(to(k["dout"]).to(DEV))
    _within(back(out.detach().cpu()), k["out64"], _se_bound(k["x"], *k["params"]), "se out")
    names = ["x"] + [n for n, _ in se.named_parameters()]
    got = [back(xd.grad)] + [p.grad for p in se.parameters()]
    for name, g, w32, w64 in zip(names, got, k["g32"], k["g64"]):
        _grad_close(name, g, w32, w64)
    with torch.no_grad():                         # the inference walk (no autograd Function): the same kernels, the same bits
        assert torch.equal(getattr(se, entry)(xd.detach()), out.detach())


# ------------------------------------------------------------------------------------------------ goldens
def test_goldens_through_the_hip_modules():
    """The reference's own inputs, parameters and outputs.  The checker (pinned to the goldens on the host) under the bounds
    above; the golden itself is an fp32 evaluation within 1 x the bound of the exact result, so the device is within 3 x of it."""
    blob = load_npz("g10_conditioning.npz")
    with open(os.path.join(GOLDEN, "meta_g10.json")) as f:
        meta = json.load(f)["models"]
    for name in ("film", "film_nobias"):
        film = cd.FiLM(*meta[name]["args"], **meta[name]["kwargs"])
        film.load_state_dict(sub_sd(blob, f"{name}/sd/"), strict=True)
        sd = film.state_dict()
        x, cond = torch.from_numpy(blob[f"{name}/x"]), torch.from_numpy(blob[f"{name}/cond"])
        x64, c64, wg, bg, wb, bb = ref.f64(x, cond, sd["gamma.weight"], sd["gamma.bias"], sd.get("beta.weight"), sd.get("beta.bias"))
        gamma, beta = ref.film_gb(c64, wg, bg, wb, bb)
        d = c64.shape[1]
        d_gamma = (d + 3) * U * (c64.abs() @ wg.abs().T + bg.abs())
        d_beta = (d + 3) * U * (c64.abs() @ wb.abs().T + bb.abs()) if wb is not None else torch.zeros_like(gamma)
        beta0 = beta if beta is not None else torch.zeros_like(gamma)
        bound = x64.abs() * d_gamma[:, None, :] + d_beta[:, None, :] + 3 * U * ((x64 * gamma[:, None, :]).abs() + beta0[:, None, :].abs())
        film = film.to(DEV)
        with torch.no_grad():
            out = film(x.to(DEV), cond.to(DEV)).cpu()
            out_ct = film.run_bct(ref.bct(x).to(DEV), cond.to(DEV)).cpu()
        assert torch.equal(ref.bct(out_ct), out)
        _within(out, ref.film(x64, c64, wg, bg, wb, bb), bound, f"{name} vs checker")
        _within(out, torch.from_numpy(blob[f"{name}/out"]).double(), 1.5 * bound, f"{name} vs golden")
    se = cd.SqueezeExcite(*meta["se"]["args"], **meta["se"]["kwargs"])
    se.load_state_dict(sub_sd(blob, "se/sd/"), strict=True)
    params = [p.detach().clone() for p in se.parameters()]
    x = torch.from_numpy(blob["se/x"])
    bound = _se_bound(x, *params)
    with torch.no_grad():
        out = se.to(DEV)(x.to(DEV)).cpu()
    _within(out, ref.squeeze_excite(*ref.f64(x, *params)), bound, "se vs checker")
    _within(out, torch.from_numpy(blob["se/out"]).double(), 1.5 * bound, "se vs golden")


# ------------------------------------------------------------------------------------------------ autograd plumbing
@pytest.mark.parametrize("entry", ["run_bct", "forward"])
@pytest.mark.parametrize("which", ["condition", "x", "parameters"])
def test_film_returns_only_the_gradients_asked_for(which, entry):
    torch.manual_seed(1)
    film = cd.FiLM(20, 24).to(DEV)
    full = cd.FiLM(20, 24).to(DEV)
    full.load_state_dict(film.state_dict())
    shape = (3, 24, 37) if entry == "run_bct" else (3, 37, 24)
    x, cond, dout = torch.randn(shape, device=DEV), torch.randn(3, 20, device=DEV), torch.randn(shape, device=DEV)
    xf, cf = x.clone().requires_grad_(True), cond.clone().requires_grad_(True)
    getattr(full, entry)(xf, cf).backward(dout)                     # everything asked for: the values to reproduce
    film.requires_grad_(which == "parameters")
    xg, cg = x.clone().requires_grad_(which == "x"), cond.clone().requires_grad_(which == "condition")
    out = getattr(film, entry)(xg, cg)
    assert out.requires_grad
    out.backward(dout)
    assert (xg.grad is None) == (which != "x") and (cg.grad is None) == (which != "condition")
    assert all((p.grad is None) == (which != "parameters") for p in film.parameters())
    if which == "x":
        assert torch.equal(xg.grad, xf.grad)
    if which == "condition":
        assert torch.equal(cg.grad, cf.grad)
    if which == "parameters":
        assert all(torch.equal(p.grad, q.grad) for p, q in zip(film.parameters(), full.parameters()))
    with torch.no_grad():
        assert not getattr(film, entry)(xg, cg).requires_grad
    assert getattr(film, entry)(xg, None) is xg


@pytest.mark.parametrize("which", ["x", "parameters"])
def test_squeeze_excite_returns_only_the_gradients_asked_for(which):
    torch.manual_seed(2)
    se = cd.SqueezeExcite(24).to(DEV)
    se.requires_grad_(which == "parameters")
    x = torch.randn(3, 24, 37, device=DEV, requires_grad=(which == "x"))
    se.run_bct(x).sum().backward()
    assert (x.grad is None) == (which != "x")
    assert all((p.grad is None) == (which != "parameters") for p in se.parameters())


# ------------------------------------------------------------------------------------------------ graph capture
def test_film_then_squeeze_excite_replays_from_a_graph():
    """One capture of ``FiLM.run_bct`` -> ``SqueezeExcite.run_bct`` at (2, 24, 37): a single-branch graph with no host reads.
    ``condition`` and ``x`` are overwritten in place and the replay equals the eager result bitwise."""
    torch.manual_seed(4)
    film, se = cd.FiLM(20, 24).to(DEV), cd.SqueezeExcite(24).to(DEV)
    x, cond = torch.randn(2, 24, 37, device=DEV), torch.randn(2, 20, device=DEV)
    run = lambda: se.run_bct(film.run_bct(x, cond))     # noqa: E731
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            first = run()                               # warm-up: the weight images are packed outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = run()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, first)
        x.copy_(torch.randn(2, 24, 37, device=DEV))
        cond.copy_(torch.randn(2, 20, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        replayed = out.clone()
        assert torch.equal(replayed, run()) and not torch.equal(replayed, first)
