"""Dropout kernels on the GPU (csrc/attention_dropout.hip): the masks against the CPU mirror of ``tests/philox.py`` element by
element, attention with dropout on the probabilities against the float64 definition with the mask as a constant (forward and
backward), and ``agx_dropout_add`` bit for bit.

Shapes (B, H, Dh, Tq, Tk): the smallest that cross every boundary -- one query and one key; the self-attention pointers and
strides on a qkv tensor (Dh = 24: no multiple of 32, Tq = 37: no multiple of 16, three heads, two items); Tq past one 128-query
workgroup with Tk past one 64-key block (ragged last block); Dh = 128 with Tk = 2 * 64 + 1; Tq = 257 > Tk.
Tolerances are the suite's own for this arithmetic (tests/test_gpu_cross_attention.py): 3e-5 of max(1, max|o|) for the
forward, 5e-5 / 1e-5 (max / rms, each times max(1, .)) for the split backward."""
import numpy as np
import pytest
import torch

from audio_generation_amd import AgxError, ops
from oracle import attention as oattn
from tests import philox
from tests.dropout_ref import attention_factor, drop_core
from tests.helpers import max_abs, rms

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(2, 1, 8, 1, 1), (2, 3, 24, 37, 37), (1, 2, 64, 130, 70), (2, 2, 128, 17, 129), (1, 2, 16, 257, 40)]
SELF = {(2, 3, 24, 37, 37)}          # run through q = qkv, kv = qkv + H Dh T and the 3 H Dh T strides
PS = [0.1, 0.5]
SEED, STREAM = 0x9E3779B97F4A7C15, 6
_REF = {}


def _case_id(c):
    return "x".join(map(str, c))


def _inputs(case):
    b, heads, dh, tq, tk = case
    gen = torch.Generator().manual_seed(1000 * tq + 10 * tk + dh)
    q = 0.7 * torch.randn(b, heads * dh, tq, generator=gen)
    kv = 0.7 * torch.randn(b, 2 * heads * dh, tk, generator=gen)
    dout = torch.randn(b, heads * dh, tq, generator=gen)
    return q, kv, dout, oattn.alibi_slopes(heads)


def _reference(case, p):
    """Computed once per (case, p), shared by the forward and the backward test, never modified."""
    if (case, p) not in _REF:
        b, heads, dh, tq, tk = case
        q, kv, dout, slopes = _inputs(case)
        q64, kv64 = q.double().requires_grad_(), kv.double().requires_grad_()
        out = drop_core(q64, kv64, slopes, heads, dh, dh ** 0.5, attention_factor(SEED, STREAM, p, b, heads, tq, tk))
        out.backward(dout.double())
        _REF[(case, p)] = dict(out=out.detach(), dq=q64.grad, dkv=kv64.grad)
    return _REF[(case, p)]


def _device_inputs(case):
    """(q, kv) as the op takes them -- for a self-attention case (qkv, None) -- plus dout and slopes, on the device."""
    q, kv, dout, slopes = _inputs(case)
    if case in SELF:
        return torch.cat([q, kv], dim=1).to(DEV), None, dout.to(DEV), slopes.to(DEV)
    return q.to(DEV), kv.to(DEV), dout.to(DEV), slopes.to(DEV)


# ------------------------------------------------------------------------------------------------- 1. the mask
MASK_SHAPE = (2, 2, 128, 37, 100)     # B, H, Dh, Tq, Tk: Tk <= Dh, so V can hold one unit row per key
MASK_DRAWS = [(0x0123456789ABCDEF, 3), (0x0123456789ABCDEF, 4), (0xFEDCBA9876543210, 3)]     # (seed, stream id)


@pytest.mark.parametrize("p", PS)
def test_the_mask_is_the_definition(p):
    """q = 0: every key of a row has a nonzero probability; V = the first Tk rows of an identity: out[b, h, j, i] = P~[i, j],
    nonzero exactly where (b, h, i, j) is kept."""
    b, heads, dh, tq, tk = MASK_SHAPE
    q = torch.zeros(b, heads * dh, tq, device=DEV)
    v = torch.zeros(heads, dh, tk)
    v[:, torch.arange(tk), torch.arange(tk)] = 1.0
    kv = torch.cat([torch.zeros(b, heads * dh, tk), v.reshape(1, heads * dh, tk).expand(b, -1, -1)], dim=1).contiguous().to(DEV)
    slopes = oattn.alibi_slopes(heads).to(DEV)
    masks = []
    for seed, stream in MASK_DRAWS:
        want = philox.attention_keep(seed, stream, p, b, heads, tq, tk)                      # (b, h, i, j)
        out = ops.attention_alibi_dropout(q, kv, slopes, heads, dh, dh ** 0.5, p, seed, stream)
        got = (out.reshape(b, heads, dh, tq)[:, :, :tk] != 0).permute(0, 1, 3, 2).cpu().numpy()
        assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} mask elements differ (seed {seed:#x}, stream {stream})"
        assert float(out.reshape(b, heads, dh, tq)[:, :, tk:].abs().max()) == 0.0
        n, frac = want.size, float(want.mean())
        sigma = (p * (1 - p) / n) ** 0.5
        print(f"mask p={p} seed={seed:#x} stream={stream}: kept {frac:.5f}, expected {1 - p} +- {sigma:.5f}")
        assert abs(frac - (1 - p)) < 4 * sigma
        masks.append(want)
    assert not np.array_equal(masks[0], masks[1])          # streams
    assert not np.array_equal(masks[0], masks[2])          # seeds
    flat = masks[0].reshape(b * heads, -1)
    for a in range(b * heads):                             # (b, h) pairs
        for c in range(a + 1, b * heads):
            assert not np.array_equal(flat[a], flat[c]), (a, c)


# ------------------------------------------------------------------------------------------------- 2. forward
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_forward_against_the_definition(case, p):
    b, heads, dh, tq, tk = case
    want = _reference(case, p)["out"]
    q, kv, _, slopes = _device_inputs(case)
    got = ops.attention_alibi_dropout(q, kv, slopes, heads, dh, dh ** 0.5, p, SEED, STREAM)
    assert tuple(got.shape) == (b, heads * dh, tq)
    err, scale = max_abs(got.cpu(), want), float(want.abs().max())
    print(f"dropout forward {case} p={p}: max err {err:.3e}, max|o| {scale:.3e}")
    assert err < 3e-5 * max(1.0, scale)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_p_zero_is_cross_attention(case):
    b, heads, dh, tq, tk = case
    q, kv, _, slopes = _inputs(case)
    want = ops.attention_alibi_cross(q.to(DEV), kv.to(DEV), slopes.to(DEV), heads, dh, dh ** 0.5)
    qd, kvd, _, sd = _device_inputs(case)
    got = ops.attention_alibi_dropout(qd, kvd, sd, heads, dh, dh ** 0.5, 0.0, SEED, STREAM)
    err, scale = max_abs(got, want), float(want.abs().max())
    print(f"dropout forward {case} p=0 vs attention_alibi_cross: max diff {err:.3e}")
    assert err < 3e-5 * max(1.0, scale)


# ------------------------------------------------------------------------------------------------- 3. backward
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_backward_against_float64_autograd(case, p):
    b, heads, dh, tq, tk = case
    ref = _reference(case, p)
    q, kv, dout, slopes = _device_inputs(case)
    out = ops.attention_alibi_dropout(q, kv, slopes, heads, dh, dh ** 0.5, p, SEED, STREAM)
    run = lambda: ops.attention_alibi_dropout_backward(q, kv, slopes, out, dout, heads, dh, dh ** 0.5, p, SEED, STREAM)  # noqa: E731
    first, second = run(), run()
    if kv is None:       # self-attention: one dqkv tensor, written in place through the strides
        assert first.shape == q.shape and torch.equal(first, second)
        dq, dkv = first[:, :heads * dh], first[:, heads * dh:]
    else:
        (dq, dkv), (dq2, dkv2) = first, second
        assert dq.shape == q.shape and dkv.shape == kv.shape
        assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2)          # deterministic: no atomics
    for name, got, want in (("dq", dq, ref["dq"]), ("dkv", dkv, ref["dkv"])):
        e_max, e_rms = max_abs(got.cpu(), want), rms(got.cpu(), want)
        s_max, s_rms = float(want.abs().max()), float(want.pow(2).mean().sqrt())
        print(f"dropout backward {case} p={p} {name}: max err {e_max:.3e} (max {s_max:.3e}), rms err {e_rms:.3e} (rms {s_rms:.3e})")
        assert e_max < 5e-5 * max(1.0, s_max) and e_rms < 1e-5 * max(1.0, s_rms), name


# ------------------------------------------------------------------------------------------------- 3b. one source
# The dropout backward, the cross backward and the self-attention three-kernel backward are instances of the same three bodies
# (csrc/attention_masked.hpp): where they compute the same thing, they compute the same bits.
@pytest.mark.parametrize("case", [(1, 2, 64, 130, 70), (2, 2, 128, 17, 129), (2, 1, 8, 1, 1)], ids=_case_id)
def test_p_zero_backward_is_the_cross_backward_bit_for_bit(case):
    """A partial last key block, more than one query block, Tq > Tk (the relative logit is live), DVT 1 / 2 / 4.  At p = 0 every
    factor is exactly 1.0f and every other operation is an explicit fmaf chain."""
    b, heads, dh, tq, tk = case
    q, kv, dout, slopes = (t.to(DEV) for t in _inputs(case))
    out = ops.attention_alibi_cross(q, kv, slopes, heads, dh, dh ** 0.5)
    want_dq, want_dkv = ops.attention_alibi_cross_backward(q, kv, slopes, out, dout, heads, dh, dh ** 0.5)
    dq, dkv = ops.attention_alibi_dropout_backward(q, kv, slopes, out, dout, heads, dh, dh ** 0.5, 0.0, SEED, STREAM)
    assert torch.equal(dq, want_dq), f"dq differs by {max_abs(dq, want_dq):.3e}"
    assert torch.equal(dkv, want_dkv), f"dkv differs by {max_abs(dkv, want_dkv):.3e}"


@pytest.mark.parametrize("dh,t", [(24, 257), (128, 130)], ids=["dh24xT257", "dh128xT130"])
def test_self_attention_split_backward_is_the_cross_backward_bit_for_bit(dh, t):
    """qkv split into q and kv, the result split the same way; T > 256 or head_dim > 64 selects the three-kernel path."""
    b, heads = 1, 2
    hd = heads * dh
    gen = torch.Generator().manual_seed(1000 * t + dh)
    qkv = (0.7 * torch.randn(b, 3 * hd, t, generator=gen)).to(DEV)
    dout = torch.randn(b, hd, t, generator=gen).to(DEV)
    slopes = oattn.alibi_slopes(heads).to(DEV)
    assert ops.attention_backward_kernel_name(heads, dh, t, split=True) == "attn_bwd_stats+attn_bwd_dq+attn_bwd_dkv"
    with pytest.raises(AgxError):
        ops.attention_backward_kernel_name(heads, dh, t)          # no single-launch kernel for this shape
    q, kv = qkv[:, :hd].contiguous(), qkv[:, hd:].contiguous()
    out = ops.attention_alibi_cross(q, kv, slopes, heads, dh, dh ** 0.5)
    want_dq, want_dkv = ops.attention_alibi_cross_backward(q, kv, slopes, out, dout, heads, dh, dh ** 0.5)
    dqkv = ops.attention_alibi_backward(qkv, slopes, dout, heads, dh, dh ** 0.5, out=out)
    assert torch.equal(dqkv[:, :hd], want_dq), f"dq differs by {max_abs(dqkv[:, :hd], want_dq):.3e}"
    assert torch.equal(dqkv[:, hd:], want_dkv), f"dkv differs by {max_abs(dqkv[:, hd:], want_dkv):.3e}"


# ------------------------------------------------------------------------------------------------- 4. elementwise
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
@pytest.mark.parametrize("p", PS)
def test_dropout_add_is_the_definition_bit_for_bit(n, p):
    seed, stream = 0xA5A5A5A55A5A5A5A, 9
    gen = torch.Generator().manual_seed(n)
    x, res = torch.randn(n + 1, generator=gen), torch.randn(n + 1, generator=gen)
    thresh, scale = philox.thresh_scale(p)
    keep = philox.elementwise_keep(seed, stream, p, n)

    def want(xs, rs):        # the exact fp32 product, then the fp32 add
        masked = np.where(keep, xs.numpy() * scale, np.float32(0.0)).astype(np.float32)
        return torch.from_numpy(masked if rs is None else rs.numpy() + masked)

    xd, rd = x.to(DEV), res.to(DEV)
    assert torch.equal(ops.dropout_add(xd[:n].clone(), rd[:n].clone(), p, seed, stream).cpu(), want(x[:n], res[:n]))
    assert torch.equal(ops.dropout_add(xd[:n].clone(), None, p, seed, stream).cpu(), want(x[:n], None))
    inplace = xd[:n].clone()
    assert ops.dropout_add(inplace, rd[:n].clone(), p, seed, stream, out=inplace) is inplace
    assert torch.equal(inplace.cpu(), want(x[:n], res[:n]))
    # views offset by one float: no 16-byte alignment, the scalar path; the mask is indexed from the view's first element
    xo, ro, oo = xd.clone()[1:], rd.clone()[1:], torch.full((n + 1,), 7.0, device=DEV)
    assert xo.data_ptr() % 16 == 4
    ops.dropout_add(xo, ro, p, seed, stream, out=oo[1:])
    assert torch.equal(oo[1:].cpu(), want(x[1:], res[1:])) and float(oo[0]) == 7.0
    # its own backward: the same mask on a gradient
    g = torch.randn(n, generator=gen)
    assert torch.equal(ops.dropout_add(g.to(DEV), None, p, seed, stream).cpu(), want(g, None))
