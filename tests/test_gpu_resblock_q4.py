"""The channel-quad variants of the fp32 ring residual block (csrc/resblock_p.hip, include/agx.h "Channel quads").

The claim is BIT IDENTITY: the reference of every case is the standard-layout ring kernel of the same build, the quad tensors
converted with ``permute`` / ``reshape`` here, compared with ``torch.equal``.  One case per channel count is also held
against ``oracle.codec.residual_block`` with the bound of tests/test_gpu_resblock_p.py.

A channel count whose row opted out of the quad variants (``agx_resblock_q4_supported`` answers 0: C = 256, whose variants
spill) has no kernels to compare; its cases assert the opt-out contract instead -- the query says 0, ``agx_resblock_forward_q4``
returns ``AGX_ERR_UNSUPPORTED`` without writing, and the unit walk runs the plain calls."""
import ctypes

import pytest
import torch

from audio_generation_amd import _lib, ops
from audio_generation_amd.graph import GraphedForward
from audio_generation_amd.vae import CausalEncoderBlock, CausalResidualBlock1d, _run_units
from oracle import codec
from tests.helpers import max_abs

pytestmark = pytest.mark.gpu
DEV = "cuda"
BN = {32: 512, 64: 256, 128: 128, 256: 128}
ERR_UNSUPPORTED = -5                                        # AGX_ERR_UNSUPPORTED (include/agx.h)
VARIANTS = ((False, True), (True, True), (True, False))      # (x in quads, y in quads)


def _block(c, d, seed, depthwise=False):
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for name, k in (("conv1", 7), ("conv2", 1)):
        v = torch.randn(c, c, k, generator=gen) / (c * k) ** 0.5
        sd[f"{name}.conv.weight_v"] = v
        sd[f"{name}.conv.weight_g"] = v.reshape(c, -1).norm(dim=1).reshape(-1, 1, 1) * 1.1
        sd[f"{name}.conv.bias"] = torch.randn(c, generator=gen) * 0.1
    m = CausalResidualBlock1d(c, c, dilation=d, depthwise=depthwise)
    if not depthwise:
        m.load_state_dict(sd)
    return m.to(DEV).eval(), sd, gen


def _set(knob, v):
    assert _lib.load().agx_set_tuning(knob.encode(), v) == 0


def to_q4(x):
    b, c, length = x.shape
    return x.reshape(b, c // 4, 4, length).permute(0, 1, 3, 2).contiguous()


def from_q4(q):
    b, c4, length, _ = q.shape
    return q.permute(0, 1, 3, 2).reshape(b, c4 * 4, length).contiguous()


def _desc(m, x):
    return m.conv1.desc(x.shape, 0, 0.1)


def _raw_q4(m, desc, x, y, post, xq, yq):
    """``agx_resblock_forward_q4`` on caller-owned memory; returns its status."""
    c1, c2, impl = m.conv1.conv, m.conv2.conv, m.conv1.impl
    p1, p2 = c1.packed(_lib.CONV_CAUSAL, impl), c2.packed(_lib.CONV_CAUSAL, impl)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    return _lib.load().agx_resblock_forward_q4(ctypes.byref(desc), ptr(x), ptr(p1), ptr(c1.bias.detach()), ptr(p2), ptr(c2.bias.detach()),
                                               ptr(y), int(post), int(xq), int(yq), None, 0,
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def _opted_out(m, x):
    """The opt-out contract of a row without quad variants.  True when ``m`` is such a block."""
    desc = _desc(m, x)
    if ops.resblock_q4_supported(desc):
        return False
    y = torch.full((x.shape[0], x.shape[1] // 4, x.shape[2], 4), 7.0, device=DEV)
    assert _raw_q4(m, desc, x, y, 1, 0, 1) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert not m.takes_quads(x.shape, 0.1)
    return True


@pytest.mark.parametrize("c", [32, 64, 128, 256])
@pytest.mark.parametrize("d", [1, 3, 9])
def test_every_variant_at_small_shapes(c, d):
    """A clip shorter than the halo, one shorter than a tile, an exactly full tile, a ragged second tile whose halo comes from
    the first, several tiles."""
    m, sd, gen = _block(c, d, 300 + c + d)
    for b, length in ((1, 4), (2, 60), (3, BN[c]), (2, BN[c] + 36), (1, 2052)):
        x = torch.randn(b, c, length, generator=gen)
        xd = x.to(DEV)
        if _opted_out(m, xd):
            continue
        desc, xq4 = _desc(m, xd), to_q4(xd)
        assert ops.resblock_kernel_name(desc).startswith("resblock_p")
        for post in (True, False):
            with torch.no_grad():
                want = m.run(xd, 0.1 if post else None)
                for xq, yq in VARIANTS:
                    got = m.run_quads(xq4 if xq else xd, 0.1 if post else None, xq, yq)
                    assert got.shape == ((b, c // 4, length, 4) if yq else (b, c, length))
                    assert torch.equal(from_q4(got) if yq else got, want), (c, d, b, length, post, xq, yq)
        if d == 3 and length == BN[c] + 36:     # one case per channel count against the oracle
            ref = codec.leaky(codec.residual_block(x, sd, "", d))
            with torch.no_grad():
                got = from_q4(m.run_quads(xq4, 0.1, True, True))
            assert max_abs(got.cpu(), ref) < 3e-5 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("c,d,b,length", [(32, 9, 8, 36000), (64, 3, 6, 24000), (128, 1, 4, 17000), (256, 3, 20, 3400)])
def test_pipeline_across_tile_boundaries(c, d, b, length):
    """More tiles than resident workgroups: chunk ring, DMA cursor and operand prefetch run over tile boundaries in quads."""
    m, sd, gen = _block(c, d, 11 + c)
    assert b * -(-length // BN[c]) > 512
    x = torch.randn(b, c, length, generator=gen).to(DEV)
    if _opted_out(m, x):
        return
    with torch.no_grad():
        want = m.run(x, 0.1)
        got = from_q4(m.run_quads(to_q4(x), 0.1, True, True))
    assert torch.equal(got, want)


def _stage(c, seed):
    """Three blocks d = 1, 3, 9 as an encoder block lists them (its strided conv left out)."""
    torch.manual_seed(seed)
    blk = CausalEncoderBlock(c, 2 * c, 2).to(DEV).eval()
    return [u for layer, act in list(blk.layers)[:3] for u in layer.units(act)]


def test_chain_through_the_unit_walk(monkeypatch):
    units = _stage(64, 3)
    assert [u.kind for u in units] == ["res"] * 3 and [u.layer.conv1.dilation for u in units] == [1, 3, 9]
    x = torch.randn(2, 64, 2052, generator=torch.Generator().manual_seed(4)).to(DEV)
    calls = []
    real = ops.resblock_forward_q4
    monkeypatch.setattr(ops, "resblock_forward_q4", lambda *a, **k: (calls.append((k["x_is_q4"], k["y_is_q4"])), real(*a, **k))[1])
    try:
        with torch.no_grad():
            _set("rb_q4", 1)
            y1 = _run_units(units, x)
            assert calls == [(False, True), (True, True), (True, False)]
            g1 = GraphedForward(lambda t: _run_units(units, t), x)
            _set("rb_q4", 0)
            y0 = _run_units(units, x)
            assert len(calls) == 3 * 4                      # eager + two warm-ups + the capture; none with the knob at 0
            g0 = GraphedForward(lambda t: _run_units(units, t), x)
            assert len(calls) == 3 * 4
        assert y1.shape == y0.shape == x.shape and torch.equal(y1, y0)
        x2 = torch.randn(2, 64, 2052, generator=torch.Generator().manual_seed(5)).to(DEV)
        with torch.no_grad():
            want = _run_units(units, x2)
        assert torch.equal(g1(x2), want) and torch.equal(g0(x2), want)
        assert not torch.equal(want, y0)
    finally:
        _set("rb_q4", 1)


def test_a_single_block_and_gradients_take_the_plain_call(monkeypatch):
    units = _stage(64, 6)
    x = torch.randn(1, 64, 512, generator=torch.Generator().manual_seed(7)).to(DEV)
    monkeypatch.setattr(ops, "resblock_forward_q4", lambda *a, **k: pytest.fail("quads taken"))
    with torch.no_grad():
        _run_units(units[:1], x)
        _run_units(units, x, quads=False)
        units[1].layer.split_launches = True
        try:
            _run_units(units, x)                            # runs of length 1 on both sides of the split block
        finally:
            del units[1].layer.split_launches
    _run_units(units, x)                                    # autograd on


def test_fallbacks():
    """``L % 4 != 0``, a bf16x3 block, a depthwise block and ``rb_q4 = 0`` answer 0 and run the plain path with equal results;
    ``agx_resblock_forward_q4`` on an unsupported descriptor returns the error code without launching."""
    gen = torch.Generator().manual_seed(8)
    m, sd, _ = _block(64, 3, 21)
    x = torch.randn(2, 64, 512, generator=gen).to(DEV)
    assert ops.resblock_q4_supported(_desc(m, x)) and m.takes_quads(x.shape, 0.1)
    with torch.no_grad():
        want = m.run(x, 0.1)

    def plain_only(units, inp):
        assert not any(u.layer.takes_quads(inp.shape, u.slope) for u in units)
        with torch.no_grad():
            return _run_units(units, inp)

    # rb_q4 = 0
    try:
        _set("rb_q4", 0)
        assert not ops.resblock_q4_supported(_desc(m, x))
        y = torch.full((2, 16, 512, 4), 7.0, device=DEV)
        assert _raw_q4(m, _desc(m, x), x, y, 1, 0, 1) == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((y == 7.0).all())                       # nothing was launched
        with pytest.raises(_lib.AgxError):
            m.run_quads(x, 0.1, False, True)
        units = _stage(64, 9)
        y0 = plain_only(units, x)
    finally:
        _set("rb_q4", 1)
    with torch.no_grad():
        assert torch.equal(_run_units(units, x), y0)
    with torch.no_grad():
        assert torch.equal(m.run(x, 0.1), want)

    # L % 4 != 0: the first kernel
    x3 = torch.randn(1, 64, 515, generator=gen).to(DEV)
    assert not ops.resblock_q4_supported(_desc(m, x3))
    y3 = plain_only(units, x3)
    with torch.no_grad():
        assert torch.equal(_run_units(units, x3, quads=False), y3)

    # bf16x3 arithmetic
    for u in units:
        u.layer.conv1.impl = u.layer.conv2.impl = _lib.IMPL_MFMA_BF16X3
    assert not ops.resblock_q4_supported(units[0].layer.conv1.desc(x.shape, 0, 0.1))
    yb = plain_only(units, x)
    with torch.no_grad():
        assert torch.equal(_run_units(units, x, quads=False), yb)

    # depthwise blocks
    torch.manual_seed(10)
    dw = CausalEncoderBlock(64, 128, 2, depthwise=True).to(DEV).eval()
    dwu = [u for layer, act in list(dw.layers)[:3] for u in layer.units(act)]
    assert [u.kind for u in dwu] == ["resdw"] * 3
    yd = plain_only(dwu, x)
    with torch.no_grad():
        assert torch.equal(_run_units(dwu, x, quads=False), yd)
    # the descriptor of a grouped conv has no fused block at all
    gd = ops.conv_desc(_lib.CONV_CAUSAL, 2, 64, 64, 512, 7, 1, 3, groups=64)
    assert not ops.resblock_q4_supported(gd)


@pytest.mark.parametrize("c", [32, 64, 128, 256])
def test_untouched_memory(c):
    """(x, y) both in quads at a ragged second tile: a poisoned band on both sides of ``y`` stays as it was and every element of
    ``y`` is written (NaN poison: the activation of a real number is never NaN)."""
    m, sd, gen = _block(c, 3, 40 + c)
    b, length = 2, BN[c] + 36
    x = torch.randn(b, c, length, generator=gen).to(DEV)
    if _opted_out(m, x):
        return
    n, band = b * c * length, 4096
    buf = torch.full((n + 2 * band,), float("nan"), device=DEV)
    bits = buf.view(torch.int32)
    bits[:band] = 0x7FC0BEEF
    bits[n + band:] = 0x7FC0BEEF
    y = buf[band:band + n]
    assert y.data_ptr() % 16 == 0
    assert _raw_q4(m, _desc(m, x), to_q4(x), y, 1, 1, 1) == 0
    torch.cuda.synchronize()
    assert bool((bits[:band] == 0x7FC0BEEF).all()) and bool((bits[n + band:] == 0x7FC0BEEF).all())
    assert not bool(torch.isnan(y).any())
    with torch.no_grad():
        assert torch.equal(from_q4(y.view(b, c // 4, length, 4)), m.run(x, 0.1))
