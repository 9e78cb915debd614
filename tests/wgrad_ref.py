"""Float64 references of the weight-gradient ops (dW, dbias) for any descriptor, and the exact-operand helpers.

Two forms of the same contraction:

* ``oracle_*``: autograd through the oracle's layer definitions (``oracle/codec.py``; ``F.conv1d`` / ``F.conv2d`` for the
  discriminators' padded and grouped layers), meant for the CPU at moderate sizes;
* ``fast_*``: explicit unfold + ``matmul`` chunked over the batch, for full-size operands on the device (ATen has no
  float64 MIOpen path; this keeps the reference on rocBLAS).

With operands in {-1, 0, +1} every product is exact and, while sum |dy| |x| per output element stays below 2^24, so is
every fp32 partial sum in any order: a correct kernel then matches the float64 reference bit for bit, and a dropped,
repeated or misplaced item shows up as a nonzero integer.  ``fast_*`` on (|x|, |dy|) gives that bound.
"""
import ctypes

import torch
import torch.nn.functional as F

from audio_generation_amd import _lib, ops
from oracle import codec

EXACT = 2 ** 24
CHUNK_BYTES = 1 << 30       # float64 im2col bytes per matmul of the fast reference


def ternary(shape, gen, p_nonzero=2.0 / 3.0, device="cuda"):
    """float32 tensor of -1 / 0 / +1 (each sign with probability p_nonzero / 2)."""
    u = torch.rand(shape, generator=gen, device=device)
    return torch.where(u < p_nonzero / 2, -1.0, torch.where(u < p_nonzero, 1.0, 0.0)).to(torch.float32)


def out_len(desc):
    return ops.conv_out_len(desc)


def out_shape_2d(desc):
    ho, wo = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(_lib.load().agx_conv2d_out_shape(ctypes.byref(desc), ctypes.byref(ho), ctypes.byref(wo)), "agx_conv2d_out_shape")
    return ho.value, wo.value


def weight_shape_1d(desc):
    k = desc.kernel
    if desc.kind == _lib.CONV_TRANSPOSED:
        return (desc.c_in, desc.c_out, k)
    return (desc.c_out, desc.c_in // max(desc.groups, 1), k)


# ---------------------------------------------------------------------------------------------- oracle (autograd)
def _oracle_forward_1d(desc, x, w):
    k, s, d = desc.kernel, desc.stride, desc.dilation
    if desc.kind == _lib.CONV_CAUSAL:
        return codec.causal_conv1d(x, w, None, stride=s, dilation=d)
    if desc.kind == _lib.CONV_TRANSPOSED:
        return codec.causal_conv_t1d(x, w, None, stride=s)
    if desc.kind == _lib.CONV_UPSAMPLE:
        return codec.upsample_conv1d(x, w, None, s)
    if desc.kind == _lib.CONV_SAME:
        return F.conv1d(x, w, None, padding="same", dilation=d)
    return F.conv1d(x, w, None, stride=s, padding=desc.padding, dilation=d, groups=max(desc.groups, 1))


def oracle_1d(desc, x, dy):
    """(dW, dbias) of the 1-D layer ``desc`` by float64 autograd (any device; meant for the CPU)."""
    x = x.to(torch.float64)
    dy = dy.to(torch.float64)
    w = torch.zeros(weight_shape_1d(desc), dtype=torch.float64, device=x.device, requires_grad=True)
    y = _oracle_forward_1d(desc, x, w)
    assert y.shape == dy.shape, (y.shape, dy.shape)
    (dw,) = torch.autograd.grad(y, w, dy)
    return dw, dy.sum(dim=(0, 2))


def oracle_2d(desc, x, dy):
    x = x.to(torch.float64)
    dy = dy.to(torch.float64)
    w = torch.zeros(desc.c_out, desc.c_in, desc.kh, desc.kw, dtype=torch.float64, device=x.device, requires_grad=True)
    y = F.conv2d(x, w, None, stride=(desc.stride_h, desc.stride_w), padding=(desc.pad_h, desc.pad_w))
    assert y.shape == dy.shape, (y.shape, dy.shape)
    (dw,) = torch.autograd.grad(y, w, dy)
    return dw, dy.sum(dim=(0, 2, 3))


# ---------------------------------------------------------------------------------------------- fast (unfold + matmul)
def _chunks(b, per_item_bytes):
    step = max(1, min(b, CHUNK_BYTES // max(per_item_bytes, 1)))
    return [(b0, min(b, b0 + step)) for b0 in range(0, b, step)]


def _padded_input_1d(desc, x):
    """(xp, stride, dilation) with y = conv1d(xp, W, stride, dilation) for the non-transposed kinds."""
    k, s, d, length = desc.kernel, desc.stride, desc.dilation, x.shape[-1]
    if desc.kind == _lib.CONV_CAUSAL:
        left, right = codec.causal_pads(length, k, s, d)
        return F.pad(x, (left, right)), s, d
    if desc.kind == _lib.CONV_SAME:
        total = d * (k - 1)
        return F.pad(x, (total // 2, total - total // 2)), 1, d
    if desc.kind == _lib.CONV_UPSAMPLE:
        up = x.repeat_interleave(s, dim=-1)
        return F.pad(up, ((k - 1) // 2, k - 1 - (k - 1) // 2)), 1, 1
    return F.pad(x, (desc.padding, desc.padding)), s, d


def fast_1d(desc, x, dy):
    """(dW, dbias) in float64 of the 1-D layer (grouped layers included), chunked over the batch."""
    b, k = x.shape[0], desc.kernel
    dev = x.device
    dw = torch.zeros(weight_shape_1d(desc), dtype=torch.float64, device=dev)
    if desc.kind == _lib.CONV_TRANSPOSED:
        # dW[i, o, k] = sum_{b, l} x[b, i, l] dyf[b, o, l s + k], dyf = dy with the K - s cropped steps restored as zeros
        s, lin = desc.stride, x.shape[-1]
        for b0, b1 in _chunks(b, 8 * desc.c_out * lin * k):
            dyf = F.pad(dy[b0:b1].to(torch.float64), (0, k - s))
            cols = dyf.unfold(2, k, s)[:, :, :lin]                                   # (nb, Cout, Lin, K)
            cols = cols.permute(0, 2, 1, 3).reshape(-1, desc.c_out * k)             # (nb Lin, Cout K)
            xs = x[b0:b1].to(torch.float64).permute(1, 0, 2).reshape(desc.c_in, -1)  # (Cin, nb Lin)
            dw += (xs @ cols).reshape(dw.shape)
        return dw, dy.to(torch.float64).sum(dim=(0, 2))
    g = max(desc.groups, 1)
    cpg, opg = desc.c_in // g, desc.c_out // g
    lout = dy.shape[-1]
    for b0, b1 in _chunks(b, 8 * desc.c_in * lout * k):
        xp, s, d = _padded_input_1d(desc, x[b0:b1].to(torch.float64))
        cols = xp.unfold(2, d * (k - 1) + 1, s)[:, :, :lout, ::d]                  # (nb, Cin, Lout, K)
        assert cols.shape[2] == lout, (cols.shape, lout)
        nb = b1 - b0
        cols = cols.reshape(nb, g, cpg, lout, k).permute(1, 0, 3, 2, 4).reshape(g, nb * lout, cpg * k)
        dys = dy[b0:b1].to(torch.float64).reshape(nb, g, opg, lout).permute(1, 2, 0, 3).reshape(g, opg, nb * lout)
        dw += torch.bmm(dys, cols).reshape(dw.shape)
    return dw, dy.to(torch.float64).sum(dim=(0, 2))


def fast_2d(desc, x, dy):
    b = x.shape[0]
    nk = desc.c_in * desc.kh * desc.kw
    hw = dy.shape[2] * dy.shape[3]
    dw = torch.zeros(desc.c_out, nk, dtype=torch.float64, device=x.device)
    for b0, b1 in _chunks(b, 8 * nk * hw):
        cols = F.unfold(x[b0:b1].to(torch.float64), (desc.kh, desc.kw), padding=(desc.pad_h, desc.pad_w),
                        stride=(desc.stride_h, desc.stride_w))                       # (nb, NK, Hout Wout)
        assert cols.shape[2] == hw
        cols = cols.permute(0, 2, 1).reshape(-1, nk)
        dys = dy[b0:b1].to(torch.float64).reshape(b1 - b0, desc.c_out, hw).permute(1, 0, 2).reshape(desc.c_out, -1)
        dw += dys @ cols
    return dw.reshape(desc.c_out, desc.c_in, desc.kh, desc.kw), dy.to(torch.float64).sum(dim=(0, 2, 3))


def parse_plan(name):
    """"<kernel> [cfg=..] op=.. slices=.. items=.." -> dict (kernel, cfg, op, slices, items, per)."""
    head, *fields = name.split(" ")
    out = {"kernel": head, "cfg": None}
    for f in fields:
        key, _, val = f.partition("=")
        out[key] = val if key == "op" else int(val)
    out["per"] = -(-out["items"] // out["slices"])
    return out
