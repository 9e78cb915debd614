"""Tensor-level wrappers over the C ABI: allocate outputs with torch, pass raw
device pointers + the current HIP stream to ``libagx``.  PyTorch is plumbing
here (memory, streams); all arithmetic happens in the HIP kernels.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import (CONV_CAUSAL, CONV_SAME, CONV_TRANSPOSED, CONV_UPSAMPLE, EPI_LEAKY_POST,
                   EPI_GELU_PRE, EPI_LEAKY_PRE, EPI_RESIDUAL, IMPL_AUTO, IMPL_DIRECT, IMPL_MFMA, AgxError, ConvDesc)

Tensor = torch.Tensor

# Optional launch observer (bench.py / profiling): an object with
# ``begin(kind, info) -> token`` and ``end(token)`` called around every C-ABI
# compute call.  None (the default) costs one global lookup per call.
_observer = None


def set_observer(obs) -> None:
    global _observer
    _observer = obs


def count_macs(kind: str, macs: int, desc=None) -> None:
    """Report the executed multiply-accumulates of a launch that has no timing hook (backward, 2-D and spectral ops) to the
    observer's optional ``macs(kind, n)`` method -- bench.py's FLOP account of the training step.  A layer whose descriptor
    asks for the bf16x3 arithmetic is reported as ``kind + ":bf16x3"`` (its products run on the bf16 matrix pipe at six
    bf16 flops per fp32-equivalent flop: a different roofline)."""
    if _observer is not None and hasattr(_observer, "macs"):
        if desc is not None and getattr(desc, "impl", 0) == _lib.IMPL_MFMA_BF16X3:
            kind += ":bf16x3"
        _observer.macs(kind, int(macs))


def _conv_macs(desc: "ConvDesc") -> int:
    """Executed (polyphase) MACs of a 1-D conv layer: B * Cin/groups * J * (q * Cout) * Lt."""
    b, cin, cout, lin, k, s = desc.batch, desc.c_in, desc.c_out, desc.l_in, desc.kernel, desc.stride
    g = max(getattr(desc, "groups", 1), 1)
    if desc.kind == CONV_UPSAMPLE:
        pl = (k - 1) // 2
        jmin, jmax = (-pl) // s, (s - 1 + k - 1 - pl) // s
        return b * cin * (jmax - jmin + 1) * s * cout * lin
    if desc.kind == CONV_TRANSPOSED:
        return b * cin * (-(-k // s)) * s * cout * lin
    return b * (cin // g) * cout * k * conv_out_len(desc)


def _conv2d_macs(desc) -> int:
    ho = (desc.h_in + 2 * desc.pad_h - desc.kh) // desc.stride_h + 1
    wo = (desc.w_in + 2 * desc.pad_w - desc.kw) // desc.stride_w + 1
    return desc.batch * desc.c_in * desc.c_out * desc.kh * desc.kw * ho * wo


def _kernel_name(symbol: str, *what, size: int = 96) -> str:
    """The answer of one of the library's host-only name queries (``agx_*_kernel_name``) for a descriptor or a shape."""
    buf = ctypes.create_string_buffer(size)
    args = [ctypes.byref(w) if isinstance(w, ctypes.Structure) else w if isinstance(w, float) else int(w) for w in what]
    _lib.check(getattr(_lib.load(), symbol)(*args, buf, len(buf)), symbol)
    return buf.value.decode()


def conv_kernel_name(desc: "ConvDesc") -> str:
    return _kernel_name("agx_conv_kernel_name", desc)


def resblock_kernel_name(desc: "ConvDesc") -> str:
    return _kernel_name("agx_resblock_kernel_name", desc)


def _ptr(t: Optional[Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_DTYPES = (torch.float32, torch.int64, torch.float64, torch.uint8, torch.bfloat16)   # bfloat16: activation planes


def _need_gpu(*tensors: Optional[Tensor]) -> None:
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise AgxError("audio_generation_amd runs on the MI355X only: got a tensor on "
                           f"'{t.device}'.  There is no CPU / eager fallback.")
        if t.dtype not in _DTYPES:
            raise AgxError(f"unsupported dtype {t.dtype}")


def _f32c(t: Tensor) -> Tensor:
    if t.dtype != torch.float32:
        raise AgxError(f"expected float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _checked_image(op: str, what: str, packed: Tensor, size: str, desc) -> None:
    """``packed`` is the image ``size`` (``agx_conv_packed_floats`` / ``agx_conv_bwd_packed_floats``) describes for ``desc``:
    float32, contiguous and exactly as long.  A kernel reads an image to its end wherever it is, so a short one is an
    over-read that nothing downstream can see."""
    need = getattr(_lib.load(), size)(ctypes.byref(desc))
    if need < 0:
        _lib.check(int(need), size)
    if packed.dtype != torch.float32 or not packed.is_contiguous():
        raise AgxError(f"{op}: {what} must be contiguous float32, got {packed.dtype}"
                       + ("" if packed.is_contiguous() else ", not contiguous"))
    if packed.numel() != need:
        raise AgxError(f"{op}: {what} has {packed.numel()} floats, the layer's has {int(need)}")


def _checked_bias(op: str, what: str, bias: Optional[Tensor], c_out: int) -> Optional[Tensor]:
    if bias is None:
        return None
    bias = _f32c(bias)
    if bias.numel() != c_out:
        raise AgxError(f"{op}: {what} has {bias.numel()} entries for c_out={c_out}")
    return bias


def _workspace(nbytes: int, device, query: str) -> Tensor:
    """Exactly the bytes a ``*_workspace_bytes`` query of the library answered (a negative answer is its error code)."""
    nbytes = int(nbytes)
    if nbytes < 0:
        _lib.check(nbytes, query)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


# --------------------------------------------------------------------------- conv
def conv_desc(kind: int, batch: int, c_in: int, c_out: int, l_in: int, kernel: int, stride: int = 1,
              dilation: int = 1, epilogue: int = 0, slope: float = 0.1, impl: int = IMPL_AUTO, groups: int = 1,
              padding: int = 0) -> ConvDesc:
    return ConvDesc(kind, batch, c_in, c_out, l_in, kernel, stride, dilation, epilogue, slope, impl, groups, padding)


def conv_out_len(desc: ConvDesc) -> int:
    n = _lib.load().agx_conv_out_len(ctypes.byref(desc))
    if n < 0:
        _lib.check(int(n), "agx_conv_out_len")
    return int(n)


def _pack(size: str, pack: str, desc, w: Tensor, aux: Optional[Tensor], aux_f32c: bool = False) -> Tensor:
    """The image the library's ``pack`` makes of ``w`` (and ``aux``: the weight-norm gain or sigma), ``size`` floats long."""
    lib = _lib.load()
    _need_gpu(w, aux)
    n = getattr(lib, size)(ctypes.byref(desc))
    if n < 0:
        _lib.check(int(n), size)
    w = _f32c(w)
    if aux is not None and aux_f32c:
        aux = _f32c(aux)
    packed = torch.empty(int(n), dtype=torch.float32, device=w.device)
    _lib.check(getattr(lib, pack)(ctypes.byref(desc), _ptr(w), _ptr(aux), _ptr(packed), _stream()), pack)
    return packed


def conv_pack(desc: ConvDesc, v: Tensor, g: Optional[Tensor] = None) -> Tensor:
    """Weight-norm fold + repack (``agx_conv_pack``).  Returns the packed image."""
    return _pack("agx_conv_packed_floats", "agx_conv_pack", desc, v, g, aux_f32c=True)


def conv_forward(desc: ConvDesc, x: Tensor, packed: Tensor, bias: Optional[Tensor],
                 res: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    lib = _lib.load()
    _need_gpu(x, packed, bias, res)
    x = _f32c(x)
    if tuple(x.shape) != (desc.batch, desc.c_in, desc.l_in):
        raise AgxError(f"conv_forward: x is {tuple(x.shape)}, descriptor says "
                       f"{(desc.batch, desc.c_in, desc.l_in)}")
    l_out = conv_out_len(desc)
    _checked_image("conv_forward", "the packed image", packed, "agx_conv_packed_floats", desc)
    if out is not None and (tuple(out.shape) != (desc.batch, desc.c_out, l_out) or out.dtype != torch.float32
                            or out.device != x.device or not out.is_contiguous()):
        raise AgxError(f"conv_forward: out is {tuple(out.shape)} {out.dtype} on '{out.device}'"
                       f"{'' if out.is_contiguous() else ', not contiguous'}; the layer writes contiguous float32 "
                       f"{(desc.batch, desc.c_out, l_out)} on '{x.device}'")
    y = out if out is not None else torch.empty((desc.batch, desc.c_out, l_out), dtype=torch.float32,
                                                 device=x.device)
    if res is not None:
        res = _f32c(res)
        if res.shape != y.shape:
            raise AgxError(f"conv_forward: residual is {tuple(res.shape)}, output is {tuple(y.shape)}")
    bias = _checked_bias("conv_forward", "bias", bias, desc.c_out)
    tok = _observer.begin("conv", desc) if _observer is not None else None
    _lib.check(lib.agx_conv_forward(ctypes.byref(desc), _ptr(x), _ptr(packed), _ptr(bias), _ptr(res),
                                    _ptr(y), _stream()), "agx_conv_forward")
    if tok is not None:
        _observer.end(tok)
    return y


# ---------------------------------------------------------------- activation planes (bf16x3, include/agx.h)
def planes_split(x: Tensor) -> Tensor:
    """fp32 (B, C, L) -> activation planes: bf16 (B, C / 8, 3, L, 8), h + m + l == x exactly."""
    lib = _lib.load()
    _need_gpu(x)
    x = _f32c(x)
    b, c, length = x.shape
    if c % 8:
        raise AgxError(f"planes_split: {c} channels (must be a multiple of 8)")
    planes = torch.empty((b, c // 8, 3, length, 8), dtype=torch.bfloat16, device=x.device)
    tok = _observer.begin("other", ("planes_split", 10 * x.numel())) if _observer is not None else None
    _lib.check(lib.agx_planes_split(_ptr(x), _ptr(planes), b, c, length, _stream()), "agx_planes_split")
    if tok is not None:
        _observer.end(tok)
    return planes


def planes_join(planes: Tensor) -> Tensor:
    """The fp32 activation a planes tensor stands for (h + m + l; host-side helper for tests and debugging, torch arithmetic)."""
    b, g, _, length, _ = planes.shape
    p = planes.float()
    return ((p[:, :, 0] + p[:, :, 1]) + p[:, :, 2]).permute(0, 1, 3, 2).reshape(b, g * 8, length).contiguous()


def conv_planes_supported(desc: ConvDesc) -> int:
    """0: no planes path; 1: the layer can read planes; 2: it can also write its output as planes."""
    return int(_lib.load().agx_conv_planes_supported(ctypes.byref(desc)))


def conv_forward_planes(desc: ConvDesc, x_planes: Tensor, packed: Tensor, bias: Optional[Tensor],
                        out_planes: bool = False) -> Tensor:
    """``conv_forward`` of a bf16x3 ring layer whose input is given as activation planes; ``out_planes``: the output is
    returned as planes as well (one-phase layers only)."""
    lib = _lib.load()
    _need_gpu(x_planes, packed, bias)
    if x_planes.dtype != torch.bfloat16 or tuple(x_planes.shape) != (desc.batch, desc.c_in // 8, 3, desc.l_in, 8) \
            or not x_planes.is_contiguous():
        raise AgxError(f"conv_forward_planes: planes are {tuple(x_planes.shape)} {x_planes.dtype}, descriptor says "
                       f"{(desc.batch, desc.c_in // 8, 3, desc.l_in, 8)} bfloat16")
    l_out = conv_out_len(desc)
    _checked_image("conv_forward_planes", "the packed image", packed, "agx_conv_packed_floats", desc)
    bias = _checked_bias("conv_forward_planes", "bias", bias, desc.c_out)
    if out_planes:
        y = torch.empty((desc.batch, desc.c_out // 8, 3, l_out, 8), dtype=torch.bfloat16, device=x_planes.device)
    else:
        y = torch.empty((desc.batch, desc.c_out, l_out), dtype=torch.float32, device=x_planes.device)
    tok = _observer.begin("conv", desc) if _observer is not None else None
    _lib.check(lib.agx_conv_forward_planes(ctypes.byref(desc), _ptr(x_planes), _ptr(packed), _ptr(bias),
                                           None if out_planes else _ptr(y), _ptr(y) if out_planes else None, _stream()),
               "agx_conv_forward_planes")
    if tok is not None:
        _observer.end(tok)
    return y


def conv_pack_bwd(desc: ConvDesc, v: Tensor, g: Optional[Tensor] = None) -> Tensor:
    """Packed image of the layer's backward-data op (``agx_conv_pack_bwd``)."""
    return _pack("agx_conv_bwd_packed_floats", "agx_conv_pack_bwd", desc, v, g, aux_f32c=True)


def conv_bwd_data(desc: ConvDesc, dy: Tensor, packed_bwd: Tensor, add: Optional[Tensor] = None,
                  mask: Optional[Tensor] = None, slope: float = 0.1) -> Tensor:
    """Gradient w.r.t. the input of the layer ``desc`` describes (forward descriptor)."""
    lib = _lib.load()
    _need_gpu(dy, packed_bwd, add, mask)
    dy = _f32c(dy)
    l_out = conv_out_len(desc)
    if tuple(dy.shape) != (desc.batch, desc.c_out, l_out):
        raise AgxError(f"conv_bwd_data: dy is {tuple(dy.shape)}, expected {(desc.batch, desc.c_out, l_out)}")
    _checked_image("conv_bwd_data", "the packed image", packed_bwd, "agx_conv_bwd_packed_floats", desc)
    dx = torch.empty((desc.batch, desc.c_in, desc.l_in), dtype=torch.float32, device=dy.device)
    for t, nm in ((add, "add"), (mask, "mask")):
        if t is not None and tuple(t.shape) != tuple(dx.shape):
            raise AgxError(f"conv_bwd_data: {nm} is {tuple(t.shape)}, dx is {tuple(dx.shape)}")
    add = None if add is None else _f32c(add)
    mask = None if mask is None else _f32c(mask)
    count_macs("conv_bwd_data", _conv_macs(desc), desc)
    _lib.check(lib.agx_conv_bwd_data(ctypes.byref(desc), _ptr(dy), _ptr(packed_bwd), _ptr(add), _ptr(mask),
                                     float(slope), _ptr(dx), _stream()), "agx_conv_bwd_data")
    return dx


def conv_bwd_weight(desc: ConvDesc, x: Tensor, dy: Tensor, v: Tensor, g: Optional[Tensor], want_bias: bool = True):
    """(dv, dg or None, dbias or None) of the layer ``desc`` describes."""
    lib = _lib.load()
    _need_gpu(x, dy, v, g)
    x, dy, v = _f32c(x), _f32c(dy), _f32c(v)
    g = None if g is None else _f32c(g)
    k, groups = desc.kernel, max(1, desc.groups)
    want_v = (desc.c_in, desc.c_out, k) if desc.kind == _lib.CONV_TRANSPOSED else (desc.c_out, desc.c_in // groups, k)
    for t, nm, want in ((x, "x", (desc.batch, desc.c_in, desc.l_in)), (dy, "dy", (desc.batch, desc.c_out, conv_out_len(desc))),
                        (v, "v", want_v)):
        if tuple(t.shape) != want:
            raise AgxError(f"conv_bwd_weight: {nm} is {tuple(t.shape)}, descriptor says {want}")
    dv = torch.empty_like(v)
    dg = None if g is None else torch.empty_like(g)
    db = torch.empty(desc.c_out, dtype=torch.float32, device=x.device) if want_bias else None
    ws_bytes = int(lib.agx_conv_bwd_weight_workspace_bytes(ctypes.byref(desc)))
    ws = _workspace(ws_bytes, x.device, "agx_conv_bwd_weight_workspace_bytes")
    count_macs("conv_bwd_weight", _conv_macs(desc), desc)
    _lib.check(lib.agx_conv_bwd_weight(ctypes.byref(desc), _ptr(x), _ptr(dy), _ptr(v), _ptr(g), _ptr(dv), _ptr(dg),
                                       _ptr(db), _ptr(ws), ws_bytes, _stream()), "agx_conv_bwd_weight")
    return dv, dg, db


def conv_bwd_weight_kernel_name(desc: ConvDesc) -> str:
    """What ``conv_bwd_weight`` runs: "<kernel> cfg=.. op=.. slices=.. items=.." (include/agx.h)."""
    return _kernel_name("agx_conv_bwd_weight_kernel_name", desc, size=128)


def _checked_block(op: str, desc: ConvDesc, packed1: Tensor, bias1, packed2: Tensor, bias2):
    """The images and biases of a fused residual block: ``packed1`` is the image of ``desc`` (the dilated k = 7 conv),
    ``packed2`` that of the block's k = 1 conv in the same arithmetic.  Returns the two biases."""
    c = desc.c_in
    _checked_image(op, "packed1", packed1, "agx_conv_packed_floats", desc)
    _checked_image(op, "packed2", packed2, "agx_conv_packed_floats",
                   conv_desc(CONV_CAUSAL, desc.batch, c, c, desc.l_in, 1, 1, 1, impl=desc.impl))
    return _checked_bias(op, "bias1", bias1, c), _checked_bias(op, "bias2", bias2, c)


def resblock_forward(desc: ConvDesc, x: Tensor, packed1: Tensor, bias1: Optional[Tensor],
                     packed2: Tensor, bias2: Optional[Tensor], post_act: bool = True) -> Tensor:
    lib = _lib.load()
    _need_gpu(x, packed1, packed2, bias1, bias2)
    x = _f32c(x)
    if tuple(x.shape) != (desc.batch, desc.c_in, desc.l_in):
        raise AgxError(f"resblock_forward: x is {tuple(x.shape)}, descriptor says "
                       f"{(desc.batch, desc.c_in, desc.l_in)}")
    bias1, bias2 = _checked_block("resblock_forward", desc, packed1, bias1, packed2, bias2)
    y = torch.empty_like(x)
    ws_bytes = int(lib.agx_resblock_workspace_bytes(ctypes.byref(desc)))
    ws = _workspace(ws_bytes, x.device, "agx_resblock_workspace_bytes")
    tok = _observer.begin("resblock", desc) if _observer is not None else None
    _lib.check(lib.agx_resblock_forward(ctypes.byref(desc), _ptr(x), _ptr(packed1), _ptr(bias1),
                                        _ptr(packed2), _ptr(bias2), _ptr(y), int(bool(post_act)),
                                        _ptr(ws), ws_bytes, _stream()), "agx_resblock_forward")
    if tok is not None:
        _observer.end(tok)
    return y


def resblock_q4_supported(desc: ConvDesc) -> bool:
    """The block has the channel-quad variants of the fp32 ring kernel (``agx_resblock_q4_supported``; host-only query)."""
    return bool(_lib.load().agx_resblock_q4_supported(ctypes.byref(desc)))


def resblock_forward_q4(desc: ConvDesc, x: Tensor, packed1: Tensor, bias1: Optional[Tensor], packed2: Tensor,
                        bias2: Optional[Tensor], post_act: bool = True, x_is_q4: bool = False, y_is_q4: bool = False) -> Tensor:
    """``resblock_forward`` with the input and / or the output in channel quads (include/agx.h): a quad tensor is
    ``(B, C / 4, L, 4)``, a standard one ``(B, C, L)``."""
    lib = _lib.load()
    _need_gpu(x, packed1, packed2, bias1, bias2)
    x = _f32c(x)
    b, c, length = desc.batch, desc.c_in, desc.l_in
    if tuple(x.shape) != ((b, c // 4, length, 4) if x_is_q4 else (b, c, length)):
        raise AgxError(f"resblock_forward_q4: x is {tuple(x.shape)}, descriptor says {(b, c, length)}, x_is_q4={bool(x_is_q4)}")
    bias1, bias2 = _checked_block("resblock_forward_q4", desc, packed1, bias1, packed2, bias2)
    y = torch.empty((b, c // 4, length, 4) if y_is_q4 else (b, c, length), dtype=torch.float32, device=x.device)
    ws_bytes = int(lib.agx_resblock_workspace_bytes(ctypes.byref(desc)))
    ws = _workspace(ws_bytes, x.device, "agx_resblock_workspace_bytes")
    tok = _observer.begin("resblock", desc) if _observer is not None else None
    _lib.check(lib.agx_resblock_forward_q4(ctypes.byref(desc), _ptr(x), _ptr(packed1), _ptr(bias1), _ptr(packed2), _ptr(bias2),
                                           _ptr(y), int(bool(post_act)), int(bool(x_is_q4)), int(bool(y_is_q4)),
                                           _ptr(ws), ws_bytes, _stream()), "agx_resblock_forward_q4")
    if tok is not None:
        _observer.end(tok)
    return y


# ---------------------------------------------------------------------------- rvq
def _stage_sizes(op: str, sizes: Optional[Sequence[int]], n_q: int, k: int):
    """``sizes`` as a host int32 array (None: every stage has ``k`` codes) for every op that takes one -- the quantiser, its step,
    the code prior, the entropy coder --, refused here when there are more than 64 stages or a stage lies outside 1 .. k."""
    if n_q > 64:
        raise AgxError(f"{op}: at most 64 stages, got {n_q}")
    if sizes is None:
        return None
    sizes = [int(v) for v in sizes]
    if len(sizes) != n_q or any(not 1 <= v <= k for v in sizes):
        raise AgxError(f"{op}: sizes {sizes} for {n_q} stages of at most {k} codes")
    return (ctypes.c_int32 * n_q)(*sizes)


def _arr_ptr(arr):
    return None if arr is None else ctypes.cast(arr, ctypes.c_void_p)


def rvq_pack(codebooks: Tensor, sizes: Optional[Sequence[int]] = None) -> Tensor:
    """Stage images of (Q, K, D) codebooks; ``sizes[q] <= K`` = real codewords of stage q (rows beyond are padding
    the search can never select) for quantizers with one codebook size per stage."""
    lib = _lib.load()
    _need_gpu(codebooks)
    codebooks = _f32c(codebooks)
    q, k, d = codebooks.shape
    n = lib.agx_rvq_packed_floats(q, k, d)
    if n < 0:
        _lib.check(int(n), "agx_rvq_packed_floats")
    packed = torch.empty(int(n), dtype=torch.float32, device=codebooks.device)
    if sizes is None:
        _lib.check(lib.agx_rvq_pack(_ptr(codebooks), q, k, d, _ptr(packed), _stream()), "agx_rvq_pack")
    else:
        arr = _stage_sizes("rvq_pack", sizes, q, k)
        _lib.check(lib.agx_rvq_pack_sized(_ptr(codebooks), _arr_ptr(arr), q, k, d, _ptr(packed), _stream()), "agx_rvq_pack_sized")
    return packed


def rvq_forward(x: Tensor, codebooks: Tensor, packed: Tensor, q_used: int,
                layout: str = "b l c", *, stages: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """x: (B,T,D) for layout "b l c" or (B,D,T) for "b c l" (any strides).
    Returns (x_q in the same layout/shape, index (B,T,q_used) int64, sq_err (q_used) f64, commit): the commit loss
    sum(sq_err) / x.numel() is a 0-d f32 tensor written by the same launch.

    ``stages`` (int64 (B,), device; ``agx_rvq_forward_staged``): row b keeps its first
    ``q_b = clamp(stages[b], 0, q_used)`` stages and is exactly that row quantised alone with ``q_used = q_b`` -- index is -1 at its
    other stages, x_q sums its live stages only (exact 0 for ``q_b == 0``), sq_err[q] sums the frames live at q.  The kernel reads
    the tensor, the host never does; None is the unstaged call, bit for bit."""
    lib = _lib.load()
    _, stages = _checked_rows("rvq_forward", x.shape[0] if x.dim() == 3 else -1, x.device, stages=stages, on="the inputs are on")
    _need_gpu(x, codebooks, packed)
    if x.dtype != torch.float32:
        raise AgxError(f"rvq_forward: expected float32, got {x.dtype}")
    codebooks = _f32c(codebooks)
    q_total, k, d = codebooks.shape
    if not 0 <= q_used <= q_total:
        raise AgxError(f"rvq_forward: q_used={q_used} outside [0, {q_total}]")
    if layout == "b l c":
        b, t, dim = x.shape
        sb, st, sd = x.stride()
    elif layout == "b c l":
        b, dim, t = x.shape
        sb, sd, st = x.stride()
    else:
        raise AgxError(f"rvq_forward: unknown layout {layout!r}")
    if dim != d:
        raise AgxError(f"rvq_forward: frame dim {dim} != codebook dim {d}")
    xq = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    if layout == "b l c":
        qb, qt, qd = xq.stride()
    else:
        qb, qd, qt = xq.stride()
    index = torch.empty((b, t, q_used), dtype=torch.int64, device=x.device)
    # one f64 buffer: [q_used per-stage sums | per-workgroup partials (the library's workspace)]; the commit loss is a
    # separate f32 scalar -- all three written by the launch, nothing to zero, no reduction on the torch side
    ws_bytes = int(lib.agx_rvq_workspace_bytes(b, t, d, k, q_used))
    buf = torch.empty(q_used + ws_bytes // 8, dtype=torch.float64, device=x.device)
    commit = torch.empty((), dtype=torch.float32, device=x.device)
    tok = _observer.begin("rvq", (b, t, d, k, q_used)) if _observer is not None else None
    head = (_ptr(x), sb, st, sd, _ptr(codebooks), _ptr(packed), b, t, d, k, q_used, _ptr(xq), qb, qt, qd, _ptr(index))
    tail = (_ptr(buf), _ptr(commit), ctypes.c_void_p(buf.data_ptr() + 8 * q_used), ws_bytes, _stream())
    if stages is None:
        _lib.check(lib.agx_rvq_forward_ex(*head, *tail), "agx_rvq_forward_ex")
    else:
        _lib.check(lib.agx_rvq_forward_staged(*head, _ptr(stages), *tail), "agx_rvq_forward_staged")
    if tok is not None:
        _observer.end(tok)
    if q_used == 0:
        xq.zero_()
        commit.zero_()
    return xq, index, buf[:q_used], commit


def rvq_ema_stats(frames: Tensor, codebooks: Tensor, index: Tensor) -> Tensor:
    """Per-stage, per-code assignment counts and residual sums of the EMA codebook update: frames (N, D),
    codebooks (Q, K, D), index (N, q_used) -> stats (q_used, K, D + 1); sums in frame order (deterministic)."""
    lib = _lib.load()
    _need_gpu(frames, codebooks, index)
    frames, codebooks = _f32c(frames), _f32c(codebooks)
    index = index.contiguous().to(torch.int64)
    n, d = frames.shape
    q_used = index.shape[1]
    k = codebooks.shape[1]
    stats = torch.empty(q_used, k, d + 1, dtype=torch.float32, device=frames.device)
    nbytes = int(lib.agx_rvq_ema_workspace_bytes(n, d, q_used))
    ws = _workspace(nbytes, frames.device, "agx_rvq_ema_workspace_bytes")
    _lib.check(lib.agx_rvq_ema_stats(_ptr(frames), _ptr(codebooks), _ptr(index), _ptr(stats), n, d, k, q_used, _ptr(ws), nbytes,
                                     _stream()), "agx_rvq_ema_stats")
    return stats


def rvq_backward(x: Tensor, codebooks: Tensor, index: Tensor, g_xq: Optional[Tensor], g_commit: Optional[Tensor],
                 layout: str = "b l c", want_codebook_grad: bool = False, *,
                 stages: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """Backward of the quantiser's training call (``agx_rvq_backward``): x and g_xq (any strides, ``None`` = zero) in
    ``layout`` as for ``rvq_forward``, index (B, T, q_used) as the forward returned it, g_commit a 0-d device tensor (``None`` =
    zero; never read on the host) -> (dx contiguous in x's shape, d codebooks (Q, K, D) or ``None``).

    ``stages``: the tensor the forward took (``agx_rvq_backward_staged``) -- the residual chain and the suffix sums of
    row b's frames run over its ``q_b`` live stages only, so dx of a ``q_b == 0`` row is g_xq alone and a stage no row runs gets an
    exactly zero codebook gradient.  Not the unstaged backward on the masked index, where a stage with index -1 still enters the
    loss."""
    lib = _lib.load()
    _, stages = _checked_rows("rvq_backward", x.shape[0] if x.dim() == 3 else -1, x.device, stages=stages, on="the inputs are on")
    _need_gpu(x, codebooks, index, g_xq, g_commit)
    for t_ in (x, g_xq, g_commit):
        if t_ is not None and t_.dtype != torch.float32:
            raise AgxError(f"rvq_backward: expected float32, got {t_.dtype}")
    if index.dtype != torch.int64 or not index.is_contiguous():
        raise AgxError("rvq_backward: index must be the contiguous int64 tensor rvq_forward returned")
    codebooks = _f32c(codebooks)
    q_total, k, d = codebooks.shape
    if layout == "b l c":
        perm = (0, 1, 2)
    elif layout == "b c l":
        perm = (0, 2, 1)
    else:
        raise AgxError(f"rvq_backward: unknown layout {layout!r}")
    b, t, dim = (x.shape[p] for p in perm)
    q_used = index.shape[-1]
    if dim != d or tuple(index.shape) != (b, t, q_used) or not 0 <= q_used <= q_total:
        raise AgxError(f"rvq_backward: x {tuple(x.shape)} ({layout}), index {tuple(index.shape)}, codebooks {tuple(codebooks.shape)}")
    if g_xq is not None and g_xq.shape != x.shape:
        raise AgxError(f"rvq_backward: g_xq {tuple(g_xq.shape)} for x {tuple(x.shape)}")
    if g_commit is not None and g_commit.numel() != 1:
        raise AgxError("rvq_backward: g_commit must hold one element")
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    dcb = torch.empty(codebooks.shape, dtype=torch.float32, device=x.device) if want_codebook_grad else None
    nbytes = int(lib.agx_rvq_backward_workspace_bytes(b * t, d, q_used)) if want_codebook_grad else 0
    ws = _workspace(nbytes, x.device, "agx_rvq_backward_workspace_bytes") if nbytes else None

    def strides(t_):
        return [0, 0, 0] if t_ is None else [t_.stride(p) for p in perm]
    head = (_ptr(x), *strides(x), _ptr(codebooks), _ptr(index))
    tail = (_ptr(g_xq), *strides(g_xq), _ptr(g_commit), b, t, d, k, q_total, q_used, _ptr(dx), *strides(dx), _ptr(dcb),
            _ptr(ws), nbytes, _stream())
    if stages is None:
        _lib.check(lib.agx_rvq_backward(*head, *tail), "agx_rvq_backward")
    else:
        _lib.check(lib.agx_rvq_backward_staged(*head, _ptr(stages), *tail), "agx_rvq_backward_staged")
    return dx, dcb


def rvq_dequantize(codebook: Tensor, idx: Tensor, out: Optional[Tensor] = None,
                   accumulate: bool = False) -> Tensor:
    """``codebook[idx]``: idx (...,) int64 -> (..., D)."""
    lib = _lib.load()
    _need_gpu(codebook, idx)
    codebook = _f32c(codebook)
    k, d = codebook.shape
    idx_c = idx.contiguous().to(torch.int64)
    n = idx_c.numel()
    if out is None:
        out = torch.empty((*idx.shape, d), dtype=torch.float32, device=codebook.device)
        accumulate = False
    flat = out.view(n, d)
    _lib.check(lib.agx_rvq_dequantize(_ptr(codebook), _ptr(idx_c), n, k, d, _ptr(flat), flat.stride(0),
                                      flat.stride(1), int(accumulate), _stream()), "agx_rvq_dequantize")
    return out


RVQ_STEP_MAX_N = 32    # AGX_RVQ_STEP_MAX_N: the frames per row one step takes


def _step_operands(op: str, codebooks: Tensor, q_used: int, sizes: Optional[Sequence[int]], bits: Optional[int]):
    """What the two step wrappers share -> (codebooks, Q, K, D, sizes as a host int32 array or None, bits)."""
    codebooks = _f32c(codebooks)
    if codebooks.dim() != 3:
        raise AgxError(f"{op}: codebooks are {tuple(codebooks.shape)}, expected (Q, K, D)")
    q_total, k, d = codebooks.shape
    if not 0 <= q_used <= q_total:
        raise AgxError(f"{op}: q_used={q_used} outside [0, {q_total}]")
    arr = _stage_sizes(op, sizes, q_total, k)
    if bits is None:
        bits = max(1, (max(arr or [k]) - 1).bit_length())
    return codebooks, q_total, k, d, arr, int(bits)


def rvq_step_packet_bytes(n: int, q_used: int, bits: int) -> int:
    """Bytes of one row's packet: ``ceil(n q_used bits / 8)`` (``agx_rvq_step_packet_bytes``)."""
    nbytes = int(_lib.load().agx_rvq_step_packet_bytes(n, q_used, bits))
    if nbytes < 0:
        raise AgxError(f"rvq_step_packet_bytes: bad arguments (n={n} outside 1 .. {RVQ_STEP_MAX_N}, q_used={q_used} outside 0 .. 64 or "
                       f"bits={bits} outside 1 .. 16)")
    return nbytes


def rvq_step_encode(z: Tensor, codebooks: Tensor, q_used: int, sizes: Optional[Sequence[int]] = None, counts: Optional[Tensor] = None,
                    bits: Optional[int] = None, want_zq: bool = True, *, stages: Optional[Tensor] = None):
    """The quantiser of a streaming chunk (``agx_rvq_step_encode``): z (B, D, n) fp32, any strides, n <= ``RVQ_STEP_MAX_N`` ->
    (zq (B, D, n) or None, index (B, n, q_used) int64, packets (B, P) uint8).  Every frame below its row's count (``counts``:
    int64 (B,), device; None: all n) gets the full defining search; behind the count zq is exact 0, index is -1 and the packet
    bytes are 0.  Row b's first ``ceil(c_b q_used bits / 8)`` bytes are ``codes_pack(index[b, :c_b], bits)``.  ``bits`` defaults
    to the width of the widest stage.

    ``stages`` (int64 (B,), device; ``agx_rvq_step_encode_staged``): row b sends its first ``q_b = clamp(stages[b], 0, q_used)``
    stages.  Only those are searched; zq is their sum, index is -1 at the others, and the row's packet is
    ``codes_pack(index[b, :c_b, :q_b], bits)`` -- all of it what ``q_used = q_b`` gives for that row.  P does not change."""
    lib = _lib.load()
    _need_gpu(z, codebooks)
    if z.dtype != torch.float32 or z.dim() != 3:
        raise AgxError(f"rvq_step_encode: expected a float32 (B, D, n) tensor, got {z.dtype} {tuple(z.shape)}")
    codebooks, q_total, k, d, arr, bits = _step_operands("rvq_step_encode", codebooks, q_used, sizes, bits)
    b, dim, n = z.shape
    if dim != d:
        raise AgxError(f"rvq_step_encode: frame dim {dim} != codebook dim {d}")
    counts, stages = _checked_rows("rvq_step_encode", b, z.device, counts, stages)
    p = rvq_step_packet_bytes(n, q_used, bits)
    zq = torch.empty((b, d, n), dtype=torch.float32, device=z.device) if want_zq else None
    index = torch.empty((b, n, q_used), dtype=torch.int64, device=z.device)
    packets = torch.empty((b, p), dtype=torch.uint8, device=z.device)
    nbytes = int(lib.agx_rvq_step_workspace_bytes(b, n, d, k, q_used))
    ws = _workspace(nbytes, z.device, "agx_rvq_step_workspace_bytes") if nbytes else None
    zsb, zsd, zst = z.stride()
    qsb, qsd, qst = zq.stride() if want_zq else (0, 0, 0)
    head = (_ptr(z), zsb, zst, zsd, _ptr(codebooks), _arr_ptr(arr), _ptr(counts))
    tail = (b, n, d, k, q_total, q_used, bits, _ptr(zq), qsb, qst, qsd, _ptr(index), _ptr(packets) if p else None, _ptr(ws), nbytes,
            _stream())
    if stages is None:
        _lib.check(lib.agx_rvq_step_encode(*head, *tail), "agx_rvq_step_encode")
    else:
        _lib.check(lib.agx_rvq_step_encode_staged(*head, _ptr(stages), *tail), "agx_rvq_step_encode_staged")
    return zq, index, packets


def _checked_packets(op: str, packets, n: int, q_used: int, bits: int) -> int:
    """``packets`` as the step kernels read it: a contiguous uint8 (B, P) tensor, P = ``rvq_step_packet_bytes`` -> B."""
    p = rvq_step_packet_bytes(n, q_used, bits)
    if not isinstance(packets, Tensor) or packets.dtype != torch.uint8 or packets.dim() != 2 or packets.shape[1] != p \
            or not packets.is_contiguous():
        got = f"{packets.dtype} {tuple(packets.shape)}" if isinstance(packets, Tensor) else type(packets).__name__
        raise AgxError(f"{op}: packets must be a contiguous uint8 (B, {p}) tensor (n={n}, q_used={q_used}, bits={bits}), got {got}")
    return packets.shape[0]


def rvq_step_decode(packets: Tensor, n: int, codebooks: Tensor, q_used: int, bits: int, sizes: Optional[Sequence[int]] = None,
                    counts: Optional[Tensor] = None, want_index: bool = False, *, stages: Optional[Tensor] = None):
    """Packets of ``rvq_step_encode`` -> zq (B, D, n), or (zq, index (B, n, q_used)) with ``want_index``: one launch
    (``agx_rvq_step_decode``).  Behind a row's count zq is exact 0 and index -1, and the packet bytes there are not read; a code
    ``>= sizes[q]`` adds nothing.  ``stages``: the tensor the sender (or ``rvq_packets_restage``) used -- row b's packet holds
    ``q_b`` codes per frame, and index is -1 at the stages it does not hold (``agx_rvq_step_decode_staged``)."""
    lib = _lib.load()
    _need_gpu(packets, codebooks)
    codebooks, q_total, k, d, arr, bits = _step_operands("rvq_step_decode", codebooks, q_used, sizes, bits)
    b = _checked_packets("rvq_step_decode", packets, n, q_used, bits)
    p = packets.shape[1]
    counts, stages = _checked_rows("rvq_step_decode", b, packets.device, counts, stages)
    zq = torch.empty((b, d, n), dtype=torch.float32, device=packets.device)
    index = torch.empty((b, n, q_used), dtype=torch.int64, device=packets.device) if want_index else None
    qsb, qsd, qst = zq.stride()
    head = (_ptr(packets) if p else None, bits, _ptr(codebooks), _arr_ptr(arr), _ptr(counts))
    tail = (b, n, d, k, q_total, q_used, _ptr(zq), qsb, qst, qsd, _ptr(index), _stream())
    if stages is None:
        _lib.check(lib.agx_rvq_step_decode(*head, *tail), "agx_rvq_step_decode")
    else:
        _lib.check(lib.agx_rvq_step_decode_staged(*head, _ptr(stages), *tail), "agx_rvq_step_decode_staged")
    return (zq, index) if want_index else zq


def rvq_packets_restage(packets: Tensor, n: int, q_used: int, bits: int, stages_to: Tensor, stages_from: Optional[Tensor] = None,
                        counts: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """Drop enhancement stages from packets that are already encoded (``agx_rvq_packets_restage``: one launch, no codebooks):
    packets (B, P) of ``rvq_step_encode`` with ``stages=stages_from`` (None: ``q_used`` stages in every row) -> (packets (B, P),
    stages (B,) int64), row b re-packed to ``q_out = min(q_in, clamp(stages_to[b], 0, q_used))`` stages -- byte for byte what the
    encoder writes with ``q_out``, zero tail included.  ``stages`` is written by the kernel: hand it to ``rvq_step_decode`` or to
    the next hop.  It never restages upward.  ``out``: a (B, P) uint8 tensor to write, sharing no byte with ``packets``."""
    op = "rvq_packets_restage"
    b = _checked_packets(op, packets, n, q_used, bits)                    # every refusal precedes the launch
    stages_to = _checked_stages(op, stages_to, b, packets.device, on="the packets are on", name="stages_to")
    if stages_from is not None:
        stages_from = _checked_stages(op, stages_from, b, packets.device, on="the packets are on", name="stages_from")
    counts, _ = _checked_rows(op, b, packets.device, counts, on="the packets are on")
    if out is not None and (not isinstance(out, Tensor) or out.dtype != torch.uint8 or out.shape != packets.shape
                            or not out.is_contiguous() or out.device != packets.device):
        raise AgxError(f"{op}: out must be a contiguous uint8 {tuple(packets.shape)} tensor on '{packets.device}'")
    lib = _lib.load()
    _need_gpu(packets)
    if out is None:
        out = torch.empty_like(packets)
    stages_out = torch.empty(b, dtype=torch.int64, device=packets.device)
    _lib.check(lib.agx_rvq_packets_restage(_ptr(packets), _ptr(stages_from), _ptr(stages_to), _ptr(counts), b, n, q_used, bits,
                                           _ptr(out), _ptr(stages_out), _stream()), "agx_rvq_packets_restage")
    return out, stages_out


# ------------------------------------------------------------------ attention block
def layernorm_ct(x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], eps: float = 1e-5) -> Tensor:
    """LayerNorm over the channel dim of a (B, C, T) tensor."""
    lib = _lib.load()
    _need_gpu(x, weight, bias)
    x = _f32c(x)
    b, c, t = x.shape
    y = torch.empty_like(x)
    tok = _observer.begin("other", ("layernorm_ct", 8 * x.numel())) if _observer is not None else None
    _lib.check(lib.agx_layernorm_ct(_ptr(x), _ptr(None if weight is None else _f32c(weight)),
                                    _ptr(None if bias is None else _f32c(bias)), _ptr(y), b, c, t, float(eps),
                                    _stream()), "agx_layernorm_ct")
    if tok is not None:
        _observer.end(tok)
    return y


ATTN_FP32, ATTN_BF16 = 0, 1


def _attn_operands(op: str, q: Tensor, kv: Optional[Tensor], heads: int, head_dim: int, qkv_q: bool = False, self_form: bool = True):
    """The (q, kv) pair of an attention call as the launchers take it -- the one place that knows the three layouts:

    * ``kv`` None: ``q`` is a (B, 3*H*Dh, T) qkv tensor read in place.  The K rows start ``hd * T`` floats into each batch row
      (the V rows follow them) and both batch strides are ``3 * hd * T``.
    * ``q`` (B, H*Dh, Tq) and ``kv`` (B, 2*H*Dh, Tk), each at its own batch stride.
    * ``qkv_q``: beside ``kv`` -- a (B, 2*H*Dh, cap) key/value buffer -- ``q`` may also be a (B, 3*H*Dh, Tq) qkv tensor of which
      only the Q rows, the first H*Dh of every batch row, are read: the q batch stride is that of the tensor given.

    Both tensors are made contiguous fp32 (``_f32c``: a wrapper that has to refuse another dtype first converts that tensor
    first; a second conversion changes nothing), then the channel counts and the batch are checked.  ``self_form`` False: the
    op has no in-place form and ``kv`` is a tensor.  Returns the view ``(b, tq, tk, hd, q, kv, qp, kp, sq, skv)``, one flat tuple (the
    cached decode step comes through here once per layer and step): ``tk`` the columns of the kv tensor (T, Tk or cap), ``q`` /
    ``kv`` the contiguous tensors, and the four C arguments -- q pointer, kv pointer, q batch stride, kv batch stride (in floats)."""
    q = _f32c(q)
    hd = heads * head_dim
    b, cq, tq = q.shape
    if kv is None and self_form:
        if cq != 3 * hd:
            raise AgxError(f"{op}: qkv has {cq} channels, expected {3 * hd}")
        at = q.data_ptr()
        return b, tq, tq, hd, q, None, ctypes.c_void_p(at), ctypes.c_void_p(at + 4 * hd * tq), 3 * hd * tq, 3 * hd * tq
    kv = _f32c(kv)
    bk, ckv, tk = kv.shape
    if cq != hd and not (qkv_q and cq == 3 * hd):
        raise AgxError(f"{op}: q has {cq} channels, expected {hd}" + (f" (or a {3 * hd}-channel qkv tensor)" if qkv_q else ""))
    if ckv != 2 * hd:
        raise AgxError(f"{op}: kv has {ckv} channels, expected {2 * hd}")
    if bk != b:
        raise AgxError(f"{op}: q has batch {b}, kv has batch {bk}")
    return b, tq, tk, hd, q, kv, ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(kv.data_ptr()), cq * tq, 2 * hd * tk


def _attn_grads(view):
    """The uninitialised gradients of a view of ``_attn_operands``, laid out as its tensors are: ``(abi, grads)`` with ``abi`` the
    view's four C arguments for the gradients and ``grads`` what the backward returns -- the one dqkv tensor of the in-place form,
    written through pointers and strides, else ``(dq, dkv)``."""
    _, tq, _, hd, q, kv, _, _, sq, skv = view
    dq = torch.empty_like(q)
    if kv is None:
        return (_ptr(dq), ctypes.c_void_p(dq.data_ptr() + 4 * hd * tq), sq, skv), dq
    dkv = torch.empty_like(kv)
    return (_ptr(dq), _ptr(dkv), sq, skv), (dq, dkv)


def _attn_same_out(op: str, view, out: Tensor, dout: Tensor, of: str = "") -> None:
    """A backward's ``out`` and ``dout`` are both (B, H*Dh, Tq) of the view (``of``: whose shape that is, in the op's words)."""
    b, tq, _, hd, *_ = view
    want = (b, hd, tq)
    if tuple(out.shape) != want or dout.shape != out.shape:
        raise AgxError(f"{op}: out {tuple(out.shape)} / dout {tuple(dout.shape)} are not {of}{want}")


def attention_alibi(qkv: Tensor, slopes: Tensor, heads: int, head_dim: int, scale_div: float,
                    precision: int = ATTN_FP32, flash: bool = False) -> Tensor:
    """softmax(QK^T/scale_div + ALiBi) V on a (B, 3*H*Dh, T) tensor -> (B, H*Dh, T), any T.
    ``precision``: ATTN_FP32 (exact fp32 MFMA) or ATTN_BF16 (bf16 MFMA, fp32 accumulate and softmax: BASELINE
    config 3); ``flash`` forces the online-softmax form for fp32 at T <= 256 as well."""
    lib = _lib.load()
    _need_gpu(qkv, slopes)
    b, t, _, hd, qkv, *_ = _attn_operands("attention_alibi", qkv, None, heads, head_dim)
    out = torch.empty((b, hd, t), dtype=torch.float32, device=qkv.device)
    tok = None
    if _observer is not None:    # the label tools/config_bench.py keys on: [:bf16][:flash], flash = any online-softmax kernel
        single_pass = attention_kernel_name(b, heads, head_dim, t, precision, flash).startswith("attention_alibi<")
        name = "attention_alibi" + (":bf16" if precision == ATTN_BF16 else "") + ("" if single_pass else ":flash")
        # algorithmic work: QK^T and PV, 2 * B * H * T * T * Dh MACs; bytes: qkv read once + out written once
        tok = _observer.begin("other", (name, 4 * (qkv.numel() + out.numel()), 2 * b * heads * t * t * head_dim))
    _lib.check(lib.agx_attention_alibi_ex(_ptr(qkv), _ptr(_f32c(slopes)), _ptr(out), b, heads, head_dim, t,
                                          float(scale_div), int(precision), int(bool(flash)), _stream()),
               "agx_attention_alibi_ex")
    if tok is not None:
        _observer.end(tok)
    return out


def layernorm_ct_backward(x: Tensor, weight: Optional[Tensor], dy: Tensor, eps: float = 1e-5,
                          add: Optional[Tensor] = None):
    """(dx [+ add], dweight, dbias) of ``layernorm_ct``."""
    lib = _lib.load()
    _need_gpu(x, weight, dy, add)
    x, dy = _f32c(x), _f32c(dy)
    add = None if add is None else _f32c(add)
    b, c, t = x.shape
    dx = torch.empty_like(x)
    dw = torch.empty(c, dtype=torch.float32, device=x.device)
    db = torch.empty(c, dtype=torch.float32, device=x.device)
    ws = torch.empty(2 * b * ((t + 63) // 64) * c, dtype=torch.float32, device=x.device)
    _lib.check(lib.agx_layernorm_ct_backward(_ptr(x), _ptr(None if weight is None else _f32c(weight)), _ptr(dy),
                                             _ptr(add), _ptr(dx), _ptr(dw), _ptr(db), _ptr(ws), b, c, t, float(eps),
                                             _stream()), "agx_layernorm_ct_backward")
    return dx, dw, db


def attention_kernel_name(batch: int, heads: int, head_dim: int, t: int, precision: int = ATTN_FP32, flash: bool = False) -> str:
    """The kernel ``attention_alibi`` runs for this shape (host-only); ``AgxError`` with the launcher's message if it refuses."""
    return _kernel_name("agx_attention_kernel_name", batch, heads, head_dim, t, precision, bool(flash))


def attention_backward_kernel_name(heads: int, head_dim: int, t: int, split: bool = False) -> str:
    """The single-launch kernel of ``agx_attention_alibi_backward`` (or ``AgxError``: the shape is beyond it), with ``split``
    the three kernels of ``agx_attention_alibi_backward_ex`` (host-only)."""
    return _kernel_name("agx_attention_backward_kernel_name", heads, head_dim, t, bool(split))


def attention_alibi_backward(qkv: Tensor, slopes: Tensor, dout: Tensor, heads: int, head_dim: int,
                             scale_div: float, out: Optional[Tensor] = None) -> Tensor:
    """dqkv of ``attention_alibi``: the single-launch kernel where the library has one for the shape
    (``attention_backward_kernel_name``), otherwise the flash-style split (``agx_attention_alibi_backward_ex``), which needs
    ``out`` = the forward's output."""
    lib = _lib.load()
    _need_gpu(qkv, slopes, dout, out)
    qkv, dout = _f32c(qkv), _f32c(dout)
    b, _, t = qkv.shape
    dqkv = torch.empty_like(qkv)
    buf = ctypes.create_string_buffer(96)
    if lib.agx_attention_backward_kernel_name(heads, head_dim, t, 0, buf, len(buf)) == 0:
        _lib.check(lib.agx_attention_alibi_backward(_ptr(qkv), _ptr(_f32c(slopes)), _ptr(dout), _ptr(dqkv), b, heads,
                                                    head_dim, t, float(scale_div), _stream()),
                   "agx_attention_alibi_backward")
        return dqkv
    if out is None:
        raise AgxError("attention_alibi_backward: T > 256 or head_dim > 64 needs the forward output (out=)")
    nbytes = int(lib.agx_attention_backward_workspace_bytes(b, heads, t))
    ws = _workspace(nbytes, qkv.device, "agx_attention_backward_workspace_bytes")
    _lib.check(lib.agx_attention_alibi_backward_ex(_ptr(qkv), _ptr(_f32c(slopes)), _ptr(_f32c(out)), _ptr(dout), _ptr(dqkv),
                                                   _ptr(ws), nbytes, b, heads, head_dim, t, float(scale_div), _stream()),
               "agx_attention_alibi_backward_ex")
    return dqkv


def attention_cross_kernel_name(batch: int, heads: int, head_dim: int, tq: int, tk: int, backward: bool = False) -> str:
    """The kernel ``attention_alibi_cross`` runs for this shape, with ``backward`` the three kernels of
    ``attention_alibi_cross_backward`` (host-only); ``AgxError`` with the launcher's message if it refuses."""
    return _kernel_name("agx_attention_cross_kernel_name", batch, heads, head_dim, tq, tk, bool(backward))


def attention_alibi_cross(q: Tensor, kv: Tensor, slopes: Tensor, heads: int, head_dim: int, scale_div: float) -> Tensor:
    """softmax(Q K^T / scale_div + ALiBi) V with queries ``q`` (B, H*Dh, Tq) and keys / values ``kv`` (B, 2*H*Dh, Tk: K rows,
    then V rows) -> (B, H*Dh, Tq); the bias is ``-slope_h |i - j|`` on the absolute positions.  fp32, any Tq, Tk >= 1."""
    lib = _lib.load()
    _need_gpu(q, kv, slopes)
    b, tq, tk, hd, q, kv, *_ = _attn_operands("attention_alibi_cross", q, kv, heads, head_dim, self_form=False)
    out = torch.empty((b, hd, tq), dtype=torch.float32, device=q.device)
    tok = None
    if _observer is not None:    # work: QK^T and PV, 2 * B * H * Tq * Tk * Dh MACs; bytes: q, kv read once + out written once
        tok = _observer.begin("other", ("attention_alibi_cross:flash", 4 * (q.numel() + kv.numel() + out.numel()),
                                        2 * b * heads * tq * tk * head_dim))
    _lib.check(lib.agx_attention_alibi_cross(_ptr(q), _ptr(kv), _ptr(_f32c(slopes)), _ptr(out), b, heads, head_dim, tq, tk,
                                             float(scale_div), _stream()), "agx_attention_alibi_cross")
    if tok is not None:
        _observer.end(tok)
    return out


def attention_alibi_cross_backward(q: Tensor, kv: Tensor, slopes: Tensor, out: Tensor, dout: Tensor, heads: int, head_dim: int,
                                   scale_div: float) -> Tuple[Tensor, Tensor]:
    """(dq, dkv) of ``attention_alibi_cross`` from its inputs, its output ``out`` and ``dout`` (both (B, H*Dh, Tq))."""
    lib = _lib.load()
    _need_gpu(q, kv, slopes, out, dout)
    q, kv, out, dout = _f32c(q), _f32c(kv), _f32c(out), _f32c(dout)
    view = b, tq, tk, _, q, kv, *_ = _attn_operands("attention_alibi_cross_backward", q, kv, heads, head_dim, self_form=False)
    _attn_same_out("attention_alibi_cross_backward", view, out, dout, of="q's ")
    _, (dq, dkv) = _attn_grads(view)
    nbytes = int(lib.agx_attention_cross_backward_workspace_bytes(b, heads, tq))
    ws = _workspace(nbytes, q.device, "agx_attention_cross_backward_workspace_bytes")
    _lib.check(lib.agx_attention_alibi_cross_backward(_ptr(q), _ptr(kv), _ptr(_f32c(slopes)), _ptr(out), _ptr(dout), _ptr(dq),
                                                      _ptr(dkv), _ptr(ws), nbytes, b, heads, head_dim, tq, tk, float(scale_div),
                                                      _stream()), "agx_attention_alibi_cross_backward")
    return dq, dkv


# ------------------------------------------------------------------ dropout (include/agx.h "Dropout masks")
def draw_dropout_seed() -> int:
    """A 64-bit mask seed from torch's default CPU generator, so that ``torch.manual_seed`` reproduces a run."""
    hi, lo = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
    return (hi << 32) | lo


def _drop_args(p: float, seed: int, stream_id: int):
    return ctypes.c_double(float(p)), ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), ctypes.c_uint32(int(stream_id) & 0xFFFFFFFF)


def attention_dropout_kernel_name(batch: int, heads: int, head_dim: int, tq: int, tk: int, p: float, backward: bool = False) -> str:
    """The kernel ``attention_alibi_dropout`` runs for this shape, with ``backward`` the three kernels of its backward
    (host-only); ``AgxError`` with the launcher's message if it refuses (head_dim > 128, p outside [0, 1))."""
    return _kernel_name("agx_attention_dropout_kernel_name", batch, heads, head_dim, tq, tk, float(p), bool(backward))


def attention_alibi_dropout(q: Tensor, kv: Optional[Tensor], slopes: Tensor, heads: int, head_dim: int, scale_div: float,
                            p: float, seed: int, stream_id: int) -> Tensor:
    """(mask * 1/(1-p) o softmax(Q K^T / scale_div + ALiBi)) V -> (B, H*Dh, Tq), the mask that of include/agx.h for
    (``seed``, ``stream_id``).  ``q`` (B, H*Dh, Tq) and ``kv`` (B, 2*H*Dh, Tk), or ``kv=None`` and ``q`` a self-attention
    (B, 3*H*Dh, T) qkv tensor (no copy).  fp32, head_dim <= 128, 0 <= p < 1."""
    lib = _lib.load()
    _need_gpu(q, kv, slopes)
    b, tq, tk, hd, q, kv, qp, kp, sq, skv = _attn_operands("attention_alibi_dropout", q, kv, heads, head_dim)
    out = torch.empty((b, hd, tq), dtype=torch.float32, device=q.device)
    tok = None
    if _observer is not None:
        tok = _observer.begin("other", ("attention_alibi_dropout:flash", 4 * (q.numel() + (0 if kv is None else kv.numel()) + out.numel()),
                                        2 * b * heads * tq * tk * head_dim))
    _lib.check(lib.agx_attention_alibi_dropout(qp, kp, sq, skv, _ptr(_f32c(slopes)), _ptr(out), b, heads, head_dim, tq, tk,
                                               float(scale_div), *_drop_args(p, seed, stream_id), _stream()),
               "agx_attention_alibi_dropout")
    if tok is not None:
        _observer.end(tok)
    return out


def attention_alibi_dropout_backward(q: Tensor, kv: Optional[Tensor], slopes: Tensor, out: Tensor, dout: Tensor, heads: int,
                                     head_dim: int, scale_div: float, p: float, seed: int, stream_id: int):
    """Backward of ``attention_alibi_dropout`` with the same (p, seed, stream_id): (dq, dkv), or with ``kv=None`` the one
    (B, 3*H*Dh, T) dqkv tensor, written in place through pointers and strides."""
    lib = _lib.load()
    _need_gpu(q, kv, slopes, out, dout)
    q, out, dout = _f32c(q), _f32c(out), _f32c(dout)
    view = b, tq, tk, _, q, kv, *abi = _attn_operands("attention_alibi_dropout_backward", q, kv, heads, head_dim)
    _attn_same_out("attention_alibi_dropout_backward", view, out, dout)
    dabi, grads = _attn_grads(view)
    nbytes = int(lib.agx_attention_dropout_backward_workspace_bytes(b, heads, tq))
    ws = _workspace(nbytes, q.device, "agx_attention_dropout_backward_workspace_bytes")
    _lib.check(lib.agx_attention_alibi_dropout_backward(*abi, _ptr(_f32c(slopes)), _ptr(out), _ptr(dout), *dabi, _ptr(ws), nbytes,
                                                        b, heads, head_dim, tq, tk, float(scale_div),
                                                        *_drop_args(p, seed, stream_id), _stream()),
               "agx_attention_alibi_dropout_backward")
    return grads


# ------------------------------------------------------------------ ragged batches (include/agx.h "Ragged batches")
def attention_ragged_kernel_name(batch: int, heads: int, head_dim: int, tq: int, tk: int, backward: bool = False) -> str:
    """The kernel ``attention_alibi_ragged`` runs for this shape, with ``backward`` the three kernels of
    ``attention_alibi_ragged_backward`` (host-only); ``AgxError`` with the launcher's message if it refuses."""
    return _kernel_name("agx_attention_ragged_kernel_name", batch, heads, head_dim, tq, tk, bool(backward))


def _len_arg(op: str, lengths: Optional[Tensor], batch: int, what: str) -> Optional[Tensor]:
    """A per-row length array as the kernels read it: None (every row full), or ``batch`` contiguous int32 entries on the
    device.  The values stay on the device -- the kernels clamp them -- so nothing here synchronises."""
    if lengths is None:
        return None
    if not lengths.is_cuda or lengths.dtype != torch.int32 or lengths.dim() != 1 or not lengths.is_contiguous():
        raise AgxError(f"{op}: {what} must be a contiguous int32 device tensor, got {lengths.dtype} {tuple(lengths.shape)} on "
                       f"'{lengths.device}'")
    if lengths.numel() != batch:
        raise AgxError(f"{op}: {what} has {lengths.numel()} entries, the batch is {batch}")
    return lengths


def attention_alibi_ragged(q: Tensor, kv: Optional[Tensor], slopes: Tensor, heads: int, head_dim: int, scale_div: float,
                           q_len: Optional[Tensor] = None, k_len: Optional[Tensor] = None) -> Tensor:
    """softmax(Q K^T / scale_div + ALiBi) V over the first ``k_len[b]`` keys of every batch row, for its first ``q_len[b]``
    queries; exactly 0 behind them (include/agx.h "Ragged batches") -> (B, H*Dh, Tq).  ``q`` (B, H*Dh, Tq) and ``kv``
    (B, 2*H*Dh, Tk), or ``kv=None`` and ``q`` a self-attention (B, 3*H*Dh, T) qkv tensor (no copy).  The lengths are
    contiguous int32 device tensors of B entries (None: every row is full), read by the kernel: no sync.  What lies at or
    beyond a row's length may hold anything, NaN included.  fp32, head_dim <= 128."""
    lib = _lib.load()
    op = "attention_alibi_ragged"
    _need_gpu(q, kv, slopes)
    b, tq, tk, hd, q, kv, qp, kp, sq, skv = _attn_operands(op, q, kv, heads, head_dim)
    q_len, k_len = _len_arg(op, q_len, b, "q_len"), _len_arg(op, k_len, b, "k_len")
    out = torch.empty((b, hd, tq), dtype=torch.float32, device=q.device)
    tok = None
    if _observer is not None:    # the full shape: the lengths live on the device
        tok = _observer.begin("other", ("attention_alibi_ragged:flash", 4 * (q.numel() + (0 if kv is None else kv.numel()) + out.numel()),
                                        2 * b * heads * tq * tk * head_dim))
    _lib.check(lib.agx_attention_alibi_ragged(qp, kp, sq, skv, _ptr(_f32c(slopes)), _ptr(q_len), _ptr(k_len), _ptr(out), b, heads,
                                              head_dim, tq, tk, float(scale_div), _stream()), "agx_attention_alibi_ragged")
    if tok is not None:
        _observer.end(tok)
    return out


def attention_alibi_ragged_backward(q: Tensor, kv: Optional[Tensor], slopes: Tensor, out: Tensor, dout: Tensor, heads: int,
                                    head_dim: int, scale_div: float, q_len: Optional[Tensor] = None,
                                    k_len: Optional[Tensor] = None):
    """Backward of ``attention_alibi_ragged`` with the same lengths: (dq, dkv), or with ``kv=None`` the one (B, 3*H*Dh, T)
    dqkv tensor, written in place through pointers and strides.  Exactly 0 at and beyond a row's lengths; ``dout`` there may
    hold anything.  Deterministic."""
    lib = _lib.load()
    op = "attention_alibi_ragged_backward"
    _need_gpu(q, kv, slopes, out, dout)
    q, out, dout = _f32c(q), _f32c(out), _f32c(dout)
    view = b, tq, tk, _, q, kv, *abi = _attn_operands(op, q, kv, heads, head_dim)
    _attn_same_out(op, view, out, dout)
    q_len, k_len = _len_arg(op, q_len, b, "q_len"), _len_arg(op, k_len, b, "k_len")
    dabi, grads = _attn_grads(view)
    nbytes = int(lib.agx_attention_ragged_backward_workspace_bytes(b, heads, tq))
    ws = _workspace(nbytes, q.device, "agx_attention_ragged_backward_workspace_bytes")
    count_macs("attention_bwd", 5 * b * heads * tq * tk * head_dim)
    _lib.check(lib.agx_attention_alibi_ragged_backward(*abi, _ptr(_f32c(slopes)), _ptr(q_len), _ptr(k_len), _ptr(out), _ptr(dout),
                                                       *dabi, _ptr(ws), nbytes, b, heads, head_dim, tq, tk, float(scale_div),
                                                       _stream()), "agx_attention_alibi_ragged_backward")
    return grads


def mask_tail(x: Tensor, lengths: Optional[Tensor], out: Optional[Tensor] = None, *, counts: Optional[Tensor] = None) -> Tensor:
    """``out[b, c, i] = x[b, c, i] if i < lengths[b] else 0`` over fp32 (B, C, T): a select, so a NaN tail becomes 0.
    ``out`` may be ``x`` (in place); default: a new tensor.  It is its own backward.  ``counts`` (keyword-only, in place of
    ``lengths``): the int64 (B,) frame counts of a counted streaming step, clamped to [0, T] by the kernel
    (``agx_mask_tail_counted``)."""
    lib = _lib.load()
    _need_gpu(x, out)
    if x.dim() != 3:
        raise AgxError(f"mask_tail: x is {tuple(x.shape)}, expected (B, C, T)")
    x = _f32c(x)
    b, c, t = x.shape
    if counts is not None:
        if lengths is not None:
            raise AgxError("mask_tail: lengths= or counts=, not both")
        counts = _checked_counts("mask_tail", counts, b, x.device)
    lengths = _len_arg("mask_tail", lengths, b, "lengths")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise AgxError(f"mask_tail: out must be a contiguous float32 tensor of x's shape {tuple(x.shape)}")
    if counts is not None:
        _lib.check(lib.agx_mask_tail_counted(_ptr(x), _ptr(counts), _ptr(out), b, c, t, _stream()), "agx_mask_tail_counted")
        return out
    _lib.check(lib.agx_mask_tail(_ptr(x), _ptr(lengths), _ptr(out), b, c, t, _stream()), "agx_mask_tail")
    return out


# ------------------------------------------------------------------ packed batches (include/agx.h "Packed variable-length batches")
def attention_packed_kernel_name(n_seq: int, heads: int, head_dim: int, nq: int, nk: int, max_q: int, max_k: int,
                                 backward: bool = False) -> str:
    """The kernel ``attention_alibi_packed`` runs for this shape, with ``backward`` the three kernels of
    ``attention_alibi_packed_backward`` (host-only); ``AgxError`` with the launcher's message if it refuses."""
    return _kernel_name("agx_attention_packed_kernel_name", n_seq, heads, head_dim, nq, nk, max_q, max_k, bool(backward))


def _cu_arg(op: str, cu: Optional[Tensor], what: str, n_seq: Optional[int] = None) -> Tensor:
    """A ``cu_seqlens`` array as the kernels read it: contiguous int32 device tensor of ``n_seq + 1`` entries (``n_seq`` None:
    any count of at least one sequence).  The values stay on the device -- the kernels clamp them -- so nothing here
    synchronises."""
    if not isinstance(cu, Tensor):
        raise AgxError(f"{op}: {what} must be a contiguous int32 device tensor, got {type(cu).__name__}")
    if not cu.is_cuda or cu.dtype != torch.int32 or cu.dim() != 1 or not cu.is_contiguous():
        raise AgxError(f"{op}: {what} must be a contiguous int32 device tensor, got {cu.dtype} {tuple(cu.shape)} on '{cu.device}'")
    if cu.numel() < 2 or (n_seq is not None and cu.numel() != n_seq + 1):
        raise AgxError(f"{op}: {what} has {cu.numel()} entries, expected " +
                       ("n_seq + 1 >= 2" if n_seq is None else f"n_seq + 1 = {n_seq + 1}"))
    return cu


def _packed_args(op: str, q: Tensor, kv: Optional[Tensor], heads: int, head_dim: int, cu_q, cu_k, max_q, max_k):
    """(view, cu_q, cu_k, n_seq, max_q, max_k) of a packed call, ``view`` that of ``_attn_operands`` with (nq, nk) for (tq, tk);
    ``kv`` None: ``q`` is a (1, 3*H*Dh, N) qkv tensor and ``cu_k`` / ``max_k`` default to the queries'."""
    q, kv = _f32c(q), None if kv is None else _f32c(kv)      # a dtype is refused before the rows are counted
    if q.dim() != 3 or q.shape[0] != 1 or (kv is not None and (kv.dim() != 3 or kv.shape[0] != 1)):
        raise AgxError(f"{op}: a packed batch is one row, q (1, C, N)" + ("" if kv is None else " and kv (1, 2*H*Dh, Nk)") +
                       f": got {tuple(q.shape)}" + ("" if kv is None else f" / {tuple(kv.shape)}"))
    view = _attn_operands(op, q, kv, heads, head_dim)
    if kv is None:
        cu_k, max_k = (cu_q if cu_k is None else cu_k), (max_q if max_k is None else max_k)
    elif cu_k is None or max_k is None:
        raise AgxError(f"{op}: separate keys need cu_k and max_k")
    cu_q = _cu_arg(op, cu_q, "cu_q")
    n_seq = cu_q.numel() - 1
    cu_k = _cu_arg(op, cu_k, "cu_k", n_seq)
    if int(max_q) != max_q or int(max_k) != max_k or max_q < 0 or max_k < 0:
        raise AgxError(f"{op}: max_q = {max_q}, max_k = {max_k}: the bounds of the sequence lengths are integers >= 0")
    return view, cu_q, cu_k, n_seq, int(max_q), int(max_k)


def attention_alibi_packed(q: Tensor, kv: Optional[Tensor], slopes: Tensor, heads: int, head_dim: int, scale_div: float,
                           cu_q: Tensor, max_q: int, cu_k: Optional[Tensor] = None, max_k: Optional[int] = None) -> Tensor:
    """softmax(Q K^T / scale_div + ALiBi) V of every sequence of a packed batch on its own (include/agx.h "Packed
    variable-length batches") -> (1, H*Dh, Nq).  Sequence ``s`` owns the query columns ``[cu_q[s], cu_q[s+1])`` and the key
    columns ``[cu_k[s], cu_k[s+1])``; positions are relative to its start.  ``q`` (1, H*Dh, Nq) and ``kv`` (1, 2*H*Dh, Nk), or
    ``kv=None`` and ``q`` a self-attention (1, 3*H*Dh, N) qkv tensor (no copy; ``cu_k`` / ``max_k`` default to the queries').
    The cu arrays are contiguous int32 device tensors of n_seq + 1 entries, read by the kernel: no sync.  ``max_q`` /
    ``max_k``: host-known upper bounds of the sequence lengths (they size the grid).  Exactly 0 in the columns no sequence
    owns; what the neighbours and the slack of the inputs hold never reaches a result.  fp32, head_dim <= 128."""
    lib = _lib.load()
    op = "attention_alibi_packed"
    _need_gpu(q, kv, slopes)
    view, cu_q, cu_k, n_seq, max_q, max_k = _packed_args(op, q, kv, heads, head_dim, cu_q, cu_k, max_q, max_k)
    _, nq, nk, hd, q, kv, qp, kp, _, _ = view        # one row: the kernels take the row strides (nq, nk), not batch strides
    out = torch.empty((1, hd, nq), dtype=torch.float32, device=q.device)
    tok = None
    if _observer is not None:    # an upper bound of the work, n_seq * max_q * max_k pairs: the lengths live on the device
        tok = _observer.begin("other", ("attention_alibi_packed:flash", 4 * (q.numel() + (0 if kv is None else kv.numel()) + out.numel()),
                                        2 * heads * min(nq, n_seq * max_q) * min(nk, max_k) * head_dim))
    _lib.check(lib.agx_attention_alibi_packed(qp, kp, nq, nk, _ptr(_f32c(slopes)), _ptr(cu_q), _ptr(cu_k), _ptr(out), n_seq, heads,
                                              head_dim, nq, nk, max_q, max_k, float(scale_div), _stream()),
               "agx_attention_alibi_packed")
    if tok is not None:
        _observer.end(tok)
    return out


def attention_alibi_packed_backward(q: Tensor, kv: Optional[Tensor], slopes: Tensor, out: Tensor, dout: Tensor, heads: int,
                                    head_dim: int, scale_div: float, cu_q: Tensor, max_q: int, cu_k: Optional[Tensor] = None,
                                    max_k: Optional[int] = None):
    """Backward of ``attention_alibi_packed`` with the same partition: (dq, dkv), or with ``kv=None`` the one (1, 3*H*Dh, N)
    dqkv tensor, written in place through pointers and strides.  Exactly 0 in the columns no sequence owns; ``dout`` there
    may hold anything.  Deterministic."""
    lib = _lib.load()
    op = "attention_alibi_packed_backward"
    _need_gpu(q, kv, slopes, out, dout)
    q, out, dout = _f32c(q), _f32c(out), _f32c(dout)
    view, cu_q, cu_k, n_seq, max_q, max_k = _packed_args(op, q, kv, heads, head_dim, cu_q, cu_k, max_q, max_k)
    _, nq, nk, _, q, kv, qp, kp, _, _ = view         # one row: the kernels take the row strides (nq, nk), not batch strides
    _attn_same_out(op, view, out, dout)
    (dqp, dkp, _, _), grads = _attn_grads(view)
    nbytes = int(lib.agx_attention_packed_backward_workspace_bytes(heads, nq))
    ws = _workspace(nbytes, q.device, "agx_attention_packed_backward_workspace_bytes")
    count_macs("attention_bwd", 5 * heads * min(nq, n_seq * max_q) * min(nk, max_k) * head_dim)
    _lib.check(lib.agx_attention_alibi_packed_backward(qp, kp, nq, nk, _ptr(_f32c(slopes)), _ptr(cu_q), _ptr(cu_k), _ptr(out), _ptr(dout),
                                                       dqp, dkp, nq, nk, _ptr(ws), nbytes, n_seq, heads, head_dim, nq, nk, max_q, max_k,
                                                       float(scale_div), _stream()), "agx_attention_alibi_packed_backward")
    return grads


def pack_rows(x: Tensor, cu: Tensor, total: int) -> Tensor:
    """A right-padded fp32 (B, C, T) batch -> its packed form (1, C, total): ``out[0, c, cu[b] + i] = x[b, c, i]`` for
    ``i < cu[b+1] - cu[b]``, exactly 0 in the columns no row owns; the padding of ``x`` is never read.  ``cu``: B + 1 int32
    entries on the device.  The adjoint of ``unpack_rows``."""
    lib = _lib.load()
    _need_gpu(x)
    if x.dim() != 3:
        raise AgxError(f"pack_rows: x is {tuple(x.shape)}, expected (B, C, T)")
    x = _f32c(x)
    b, c, t = x.shape
    if int(total) != total or total < 0:
        raise AgxError(f"pack_rows: total = {total}: the packed length is an integer >= 0")
    cu = _cu_arg("pack_rows", cu, "cu", b)
    out = torch.empty((1, c, int(total)), dtype=torch.float32, device=x.device)
    _lib.check(lib.agx_pack_rows(_ptr(x), _ptr(cu), _ptr(out), b, c, t, int(total), _stream()), "agx_pack_rows")
    return out


def unpack_rows(xp: Tensor, cu: Tensor, t: int) -> Tensor:
    """A packed fp32 (1, C, N) batch -> the right-padded (B, C, t) form: ``out[b, c, i] = xp[0, c, cu[b] + i]`` for
    ``i < cu[b+1] - cu[b]``, exactly 0 at padded positions (a select: the slack of ``xp`` is never read).  ``cu``: B + 1
    int32 entries on the device.  The adjoint of ``pack_rows``."""
    lib = _lib.load()
    _need_gpu(xp)
    if xp.dim() != 3 or xp.shape[0] != 1:
        raise AgxError(f"unpack_rows: xp is {tuple(xp.shape)}, expected (1, C, N)")
    xp = _f32c(xp)
    _, c, n = xp.shape
    if int(t) != t or t < 0:
        raise AgxError(f"unpack_rows: t = {t}: the padded length is an integer >= 0")
    cu = _cu_arg("unpack_rows", cu, "cu")
    b = cu.numel() - 1
    out = torch.empty((b, c, int(t)), dtype=torch.float32, device=xp.device)
    _lib.check(lib.agx_unpack_rows(_ptr(xp), _ptr(cu), _ptr(out), b, c, int(t), n, _stream()), "agx_unpack_rows")
    return out


# ------------------------------------------------------------------ causal attention (include/agx.h "Causal self-attention")
def attention_causal_kernel_name(batch: int, heads: int, head_dim: int, tq: int, tk: int, backward: bool = False) -> str:
    """The kernel ``attention_alibi_causal`` runs for this shape, with ``backward`` the three kernels of
    ``attention_alibi_causal_backward`` (host-only); ``AgxError`` with the launcher's message if it refuses."""
    return _kernel_name("agx_attention_causal_kernel_name", batch, heads, head_dim, tq, tk, bool(backward))


def _causal_macs(b: int, heads: int, head_dim: int, tq: int, tk: int, q_pos0: int) -> int:
    """The MACs the causal forward executes: per workgroup of 128 queries, both contractions over the 64-key blocks up to the
    last one any of its queries sees (the blocks above the diagonal are skipped)."""
    blocks = sum(min(tk - 1, q0 + 127 + q_pos0) // 64 + 1 for q0 in range(0, tq, 128))
    return 2 * b * heads * head_dim * 128 * 64 * blocks


def attention_alibi_causal(q: Tensor, kv: Optional[Tensor], slopes: Tensor, heads: int, head_dim: int, scale_div: float,
                           q_pos0: int = 0, tk: Optional[int] = None) -> Tensor:
    """Causal attention with the one-sided ALiBi bias: query ``i`` sits at position ``i + q_pos0`` and sees the keys
    ``j <= i + q_pos0`` at the bias ``-slope_h (i + q_pos0 - j)`` -> (B, H*Dh, Tq).  ``kv=None``: ``q`` is a (B, 3*H*Dh, T) qkv
    tensor read in place (full causal self-attention with ``q_pos0 = 0``).  Otherwise ``q`` holds the queries in its first
    H*Dh rows (a (B, H*Dh, Tq) tensor, or a (B, 3*H*Dh, Tq) qkv tensor whose Q rows are read in place) and ``kv`` is a
    (B, 2*H*Dh, cap) key/value buffer with ``tk <= cap`` valid columns (default ``cap``); columns >= ``tk`` are never read.
    fp32, head_dim <= 128."""
    lib = _lib.load()
    _need_gpu(q, kv, slopes)
    b, tq, cap, hd, q, kv, qp, kp, sq, skv = _attn_operands("attention_alibi_causal", q, kv, heads, head_dim, qkv_q=True)
    if kv is None:
        if tk not in (None, tq):
            raise AgxError(f"attention_alibi_causal: tk = {tk} with kv=None (the keys are the {tq} columns of qkv)")
        tk = tq
        nbytes = 4 * q.numel()
    else:
        tk = cap if tk is None else int(tk)
        if not 0 <= tk <= cap:
            raise AgxError(f"attention_alibi_causal: tk = {tk} is outside the kv buffer's {cap} columns")
        nbytes = 4 * (b * hd * tq + 2 * b * hd * tk)
    out = torch.empty((b, hd, tq), dtype=torch.float32, device=q.device)
    tok = None
    if _observer is not None and min(b, heads, tq, tk) > 0 and q_pos0 >= 0:
        tok = _observer.begin("other", ("attention_alibi_causal:flash", nbytes + 4 * out.numel(),
                                        _causal_macs(b, heads, head_dim, tq, tk, int(q_pos0))))
    _lib.check(lib.agx_attention_alibi_causal(qp, kp, sq, skv, cap, _ptr(_f32c(slopes)), _ptr(out), b, heads, head_dim, tq, tk,
                                              int(q_pos0), float(scale_div), _stream()), "agx_attention_alibi_causal")
    if tok is not None:
        _observer.end(tok)
    return out


def attention_alibi_causal_backward(qkv: Tensor, slopes: Tensor, out: Tensor, dout: Tensor, heads: int, head_dim: int,
                                    scale_div: float) -> Tensor:
    """dqkv of the full causal self-attention ``attention_alibi_causal(qkv, None, ...)`` from qkv (B, 3*H*Dh, T), the forward's
    ``out`` and ``dout`` (both (B, H*Dh, T)); qkv is read and dqkv written in place through pointers and strides."""
    lib = _lib.load()
    _need_gpu(qkv, slopes, out, dout)
    qkv, out, dout = _f32c(qkv), _f32c(out), _f32c(dout)
    view = b, t, _, _, qkv, _, *abi = _attn_operands("attention_alibi_causal_backward", qkv, None, heads, head_dim)
    _attn_same_out("attention_alibi_causal_backward", view, out, dout)
    dabi, dqkv = _attn_grads(view)
    nbytes = int(lib.agx_attention_causal_backward_workspace_bytes(b, heads, t))
    ws = _workspace(nbytes, qkv.device, "agx_attention_causal_backward_workspace_bytes")
    _lib.check(lib.agx_attention_alibi_causal_backward(*abi, _ptr(_f32c(slopes)), _ptr(out), _ptr(dout), *dabi, _ptr(ws), nbytes,
                                                       b, heads, head_dim, t, float(scale_div), _stream()),
               "agx_attention_alibi_causal_backward")
    return dqkv


# ------------------------------------------------------------------ sliding-window attention (include/agx.h "Sliding-window")
def attention_window_kernel_name(batch: int, heads: int, head_dim: int, tq: int, window: int, backward: bool = False) -> str:
    """The kernel ``attention_alibi_window`` runs for this shape, with ``backward`` the three kernels of
    ``attention_alibi_window_backward`` (host-only); ``AgxError`` with the launcher's message if it refuses."""
    return _kernel_name("agx_attention_window_kernel_name", batch, heads, head_dim, tq, window, bool(backward))


def _window_macs(b: int, heads: int, head_dim: int, tq: int, q_pos0: int, window: int) -> int:
    """The MACs the windowed forward executes: per workgroup of 128 queries, both contractions over the 64-key blocks from the
    one that holds the first key any of its queries sees to the one that holds the last."""
    blocks = sum((min(q0 + 127, tq - 1) + q_pos0) // 64 - max(0, q0 + q_pos0 - window + 1) // 64 + 1 for q0 in range(0, tq, 128))
    return 2 * b * heads * head_dim * 128 * 64 * blocks


def attention_alibi_window(q: Tensor, kv: Optional[Tensor], slopes: Tensor, heads: int, head_dim: int, scale_div: float,
                           window: int, q_pos0: int = 0, ring: int = 0) -> Tensor:
    """Sliding-window causal attention with the one-sided ALiBi bias: query ``i`` sits at position ``p = i + q_pos0`` and sees
    the keys ``max(0, p - window + 1) <= j <= p`` at the bias ``-slope_h (p - j)`` -> (B, H*Dh, Tq).  ``kv=None``: ``q`` is a
    (B, 3*H*Dh, T) qkv tensor read in place (full self-attention: ``q_pos0 = 0``, ``ring = 0``).  Otherwise ``q`` holds the
    queries in its first H*Dh rows (a (B, H*Dh, Tq) tensor, or a (B, 3*H*Dh, Tq) qkv tensor whose Q rows are read in place) and
    ``kv`` is a (B, 2*H*Dh, cap) key/value buffer: key ``j`` in column ``j`` (``ring = 0``, ``cap >= q_pos0 + Tq``) or in
    column ``j mod ring`` (``Tq + min(window - 1, q_pos0) <= ring <= cap``); a column outside the window may hold anything.  ``q_pos0`` is
    a 64-bit position.  fp32, head_dim <= 128."""
    lib = _lib.load()
    _need_gpu(q, kv, slopes)
    b, tq, cap, hd, q, kv, qp, kp, sq, skv = _attn_operands("attention_alibi_window", q, kv, heads, head_dim, qkv_q=True)
    if kv is None:
        if q_pos0 != 0 or ring != 0:
            raise AgxError(f"attention_alibi_window: q_pos0 = {q_pos0}, ring = {ring} with kv=None (the keys are the {tq} columns of qkv)")
        nbytes = 4 * q.numel()
    else:
        nbytes = 4 * (b * hd * tq + 2 * b * hd * min(cap, tq + max(int(window), 1) - 1))
    out = torch.empty((b, hd, tq), dtype=torch.float32, device=q.device)
    tok = None
    if _observer is not None and min(b, heads, tq) > 0 and q_pos0 >= 0 and window >= 1:
        tok = _observer.begin("other", ("attention_alibi_window:flash", nbytes + 4 * out.numel(),
                                        _window_macs(b, heads, head_dim, tq, int(q_pos0), int(window))))
    _lib.check(lib.agx_attention_alibi_window(qp, kp, sq, skv, cap, _ptr(_f32c(slopes)), _ptr(out), b, heads, head_dim, tq,
                                              int(q_pos0), min(int(window), 0x7fffffff), int(ring), float(scale_div), _stream()),
               "agx_attention_alibi_window")
    if tok is not None:
        _observer.end(tok)
    return out


def attention_alibi_window_backward(qkv: Tensor, slopes: Tensor, out: Tensor, dout: Tensor, heads: int, head_dim: int,
                                    scale_div: float, window: int) -> Tensor:
    """dqkv of the full windowed self-attention ``attention_alibi_window(qkv, None, ..., window)`` from qkv (B, 3*H*Dh, T), the
    forward's ``out`` and ``dout`` (both (B, H*Dh, T)); qkv is read and dqkv written in place through pointers and strides."""
    lib = _lib.load()
    _need_gpu(qkv, slopes, out, dout)
    qkv, out, dout = _f32c(qkv), _f32c(out), _f32c(dout)
    view = b, t, _, _, qkv, _, *abi = _attn_operands("attention_alibi_window_backward", qkv, None, heads, head_dim)
    _attn_same_out("attention_alibi_window_backward", view, out, dout)
    dabi, dqkv = _attn_grads(view)
    nbytes = int(lib.agx_attention_window_backward_workspace_bytes(b, heads, t))
    ws = _workspace(nbytes, qkv.device, "agx_attention_window_backward_workspace_bytes")
    _lib.check(lib.agx_attention_alibi_window_backward(*abi, _ptr(_f32c(slopes)), _ptr(out), _ptr(dout), *dabi, _ptr(ws), nbytes,
                                                       b, heads, head_dim, t, min(int(window), 0x7fffffff), float(scale_div), _stream()),
               "agx_attention_alibi_window_backward")
    return dqkv


def ring_write(buf: Tensor, src: Tensor, col0: int) -> None:
    """``buf[:, :, col0:col0 + n] = src`` for src (B, C, n): one strided device copy (``Tensor.copy_``) of a chunk's K / V rows
    into a ring cache.  The caller splits a chunk that wraps the ring into two."""
    n = src.shape[-1]
    if not 0 <= col0 <= buf.shape[-1] - n or buf.shape[:2] != src.shape[:2]:
        raise AgxError(f"ring_write: columns [{col0}, {col0 + n}) of {tuple(src.shape)} do not fit {tuple(buf.shape)}")
    buf[:, :, col0:col0 + n].copy_(src)


# ------------------------------------------------------------------ device-held stream positions (include/agx.h "Device-held")
def attention_stream_kernel_name(batch: int, heads: int, head_dim: int, tq: int, window: int) -> str:
    """The kernel ``attention_alibi_stream`` runs for this shape (host-only); ``AgxError`` with the launcher's message if it
    refuses."""
    return _kernel_name("agx_attention_stream_kernel_name", batch, heads, head_dim, tq, window)


def _checked_pos(op: str, pos, b: int, device) -> Tensor:
    """``pos`` as the kernels read it: a contiguous int64 device tensor of B entries, on the operands' device."""
    if not isinstance(pos, Tensor) or pos.dtype != torch.int64 or pos.dim() != 1 or pos.numel() != b or not pos.is_contiguous():
        what = f"{tuple(pos.shape)} {pos.dtype}" if isinstance(pos, Tensor) else type(pos).__name__
        raise AgxError(f"{op}: pos must be a contiguous int64 device tensor of {b} entries (one position per batch row), got {what}")
    _need_gpu(pos)
    if pos.device != device:
        raise AgxError(f"{op}: pos is on '{pos.device}', the operands are on '{device}'")
    return pos


def _checked_counts(op: str, counts, b: int, device, on: Optional[str] = None, name: str = "counts", per: str = "frame count") -> Tensor:
    """``counts`` as the counted kernels read it (include/agx.h "Per-row frame counts"): a contiguous int64 device tensor of B
    entries on the operands' device -- the one place that inspects it, for the ops and for the models and streams above them.
    The values stay on the device -- the kernels clamp them to [0, n] -- so nothing here synchronises or checks one.  ``on``:
    what ``device`` belongs to in the caller's words ("the cache on", "the stream on", "the conv state on"); None is an op, whose
    operands must also be on the GPU.  ``name`` / ``per``: what the message calls the tensor (``_checked_stages``)."""
    if not isinstance(counts, Tensor) or counts.dtype != torch.int64 or counts.dim() != 1 or counts.numel() != b:
        what = f"{tuple(counts.shape)} {counts.dtype}" if isinstance(counts, Tensor) else type(counts).__name__
        raise AgxError(f"{op}: {name} must be a contiguous int64 device tensor of {b} entries (one {per} per batch row), got {what}")
    if not counts.is_contiguous():
        raise AgxError(f"{op}: {name} is not contiguous (stride {tuple(counts.stride())}): the kernels read {b} adjacent int64")
    if on is None:
        _need_gpu(counts)
    if counts.device != device:
        raise AgxError(f"{op}: {name} is on '{counts.device}', {on or 'the operands are on'} '{device}'")
    return counts


def _checked_stages(op: str, stages, b: int, device, on: Optional[str] = None, name: str = "stages") -> Tensor:
    """``stages`` as the staged RVQ step kernels read it (include/agx.h "Per-row stage counts"): ``_checked_counts`` under its own
    name.  The kernels clamp the values to [0, q_used]; the host never reads one."""
    return _checked_counts(op, stages, b, device, on, name=name, per="stage count")


def _checked_rows(op: str, b: int, device, counts=None, stages=None, on: Optional[str] = None):
    """The two per-row tensors of a call, each None or checked (``_checked_counts``, then ``_checked_stages``) -> (counts, stages)."""
    if counts is not None:
        counts = _checked_counts(op, counts, b, device, on)
    if stages is not None:
        stages = _checked_stages(op, stages, b, device, on)
    return counts, stages


def _row_slices(what: str, rows, batch: int, of: str) -> list:
    """The slices a per-row reset fills, one per entry of ``rows`` (None: the one slice of every row), for a cache or stream
    (``of``) of ``batch`` rows; a row outside it is refused before anything is filled."""
    if rows is None:
        return [slice(None)]
    rows = [int(r) for r in rows]
    if any(not 0 <= r < batch for r in rows):
        raise AgxError(f"{what}: rows {rows} are not rows of a {of} of batch {batch}")
    return [slice(r, r + 1) for r in rows]


def attention_alibi_stream(q: Tensor, kv: Tensor, pos: Tensor, slopes: Tensor, heads: int, head_dim: int, scale_div: float,
                           window: int, ring: int, counts: Optional[Tensor] = None) -> Tensor:
    """``attention_alibi_window`` on a ring with the positions in device memory: row ``b``'s query ``i`` sits at
    ``p = i + pos[b]`` and sees the keys ``max(0, p - window + 1) <= j <= p``, key ``j`` in column ``j mod ring`` of ``kv``
    (B, 2*H*Dh, cap) -> (B, H*Dh, Tq).  ``q`` holds the queries in its first H*Dh rows ((B, H*Dh, Tq), or a (B, 3*H*Dh, Tq) qkv
    tensor read in place).  ``pos``: a contiguous int64 device tensor of B entries, read by the kernel and never written -- no
    sync, and a captured graph replays with the positions of the replay.  ``Tq + window - 1 <= ring <= cap``: the worst case
    over every position, since the host reads none.  Row ``b`` is bit for bit ``attention_alibi_window(..., q_pos0=pos[b])``.
    fp32, head_dim <= 128.

    ``counts`` (int64 (B,), device; ``agx_attention_alibi_stream_counted``): row ``b``'s chunk holds ``c_b = clamp(counts[b], 0,
    Tq)`` frames, whose K / V rows ``ring_write_pos(counts=)`` wrote.  The keys end at ``pos[b] + c_b - 1``: the ring columns
    behind them are never multiplied as stored.  The queries below the count are bit for bit the uncounted call on ``c_b``
    frames; the others are written and mean nothing (NaN where no key is live): mask them (``mask_tail(counts=)``).

    The bench observer cannot know the positions without a sync: it is told the blocks of the steady state (every row at
    ``pos >= window - 1``), counted at ``pos = window - 1``; a row younger than that walks fewer blocks, and another alignment
    of the window to the 64-key blocks can touch one block more or fewer."""
    lib = _lib.load()
    _need_gpu(q, kv, slopes)
    b, tq, cap, hd, q, kv, qp, kp, sq, skv = _attn_operands("attention_alibi_stream", q, kv, heads, head_dim, qkv_q=True, self_form=False)
    pos = _checked_pos("attention_alibi_stream", pos, b, q.device)
    if counts is not None:
        counts = _checked_counts("attention_alibi_stream", counts, b, q.device)
    window = min(int(window), 0x7fffffff)
    out = torch.empty((b, hd, tq), dtype=torch.float32, device=q.device)
    tok = None
    if _observer is not None and min(b, heads, tq) > 0 and window >= 1:
        nbytes = 4 * (b * hd * tq + 2 * b * hd * min(cap, tq + window - 1))
        tok = _observer.begin("other", ("attention_alibi_stream:flash", nbytes + 4 * out.numel(),
                                        _window_macs(b, heads, head_dim, tq, window - 1, window)))
    if counts is not None:
        _lib.check(lib.agx_attention_alibi_stream_counted(qp, kp, sq, skv, cap, _ptr(pos), _ptr(counts), _ptr(_f32c(slopes)), _ptr(out), b, heads,
                                                          head_dim, tq, window, int(ring), float(scale_div), _stream()),
                   "agx_attention_alibi_stream_counted")
    else:
        _lib.check(lib.agx_attention_alibi_stream(qp, kp, sq, skv, cap, _ptr(pos), _ptr(_f32c(slopes)), _ptr(out), b, heads, head_dim, tq, window,
                                                  int(ring), float(scale_div), _stream()), "agx_attention_alibi_stream")
    if tok is not None:
        _observer.end(tok)
    return out


def ring_write_pos(buf: Tensor, src: Tensor, pos: Tensor, ring: int, counts: Optional[Tensor] = None) -> None:
    """``buf[b, :, (pos[b] + t) mod ring] = src[b, :, t]`` for src (B, C, n) and buf (B, C, cap), ``n <= ring <= cap``: a chunk's
    K / V rows into a ring cache at every row's own position, one launch, wrap included.  ``src`` is read in place: rows of
    pitch ``n`` at any batch stride (the K / V rows ``qkv[:, H*Dh:]`` of a qkv tensor).  ``pos`` as in
    ``attention_alibi_stream``; it is not written.  Allocates nothing.  ``counts`` (int64 (B,), device): only the first
    ``clamp(counts[b], 0, n)`` columns of row ``b`` are written; the ring columns behind them are left as they are."""
    lib = _lib.load()
    _need_gpu(buf, src)
    if buf.dtype != torch.float32 or src.dtype != torch.float32 or buf.dim() != 3 or src.dim() != 3 or not buf.is_contiguous():
        raise AgxError("ring_write_pos: buf must be a contiguous float32 (B, C, cap) tensor and src a float32 (B, C, n) tensor")
    b, c, n = src.shape
    if tuple(buf.shape[:2]) != (b, c) or src.device != buf.device:
        raise AgxError(f"ring_write_pos: src {tuple(src.shape)} does not match buf {tuple(buf.shape)}")
    if b == 0 or c == 0 or n == 0:
        return
    if (n > 1 and src.stride(2) != 1) or (c > 1 and src.stride(1) != n) or (b > 1 and src.stride(0) < c * n):
        raise AgxError(f"ring_write_pos: src {tuple(src.shape)} with strides {tuple(src.stride())} is not rows of pitch {n}")
    pos = _checked_pos("ring_write_pos", pos, b, buf.device)
    cap = buf.shape[-1]
    if counts is not None:
        counts = _checked_counts("ring_write_pos", counts, b, buf.device)
        _lib.check(lib.agx_ring_write_pos_counted(_ptr(buf), _ptr(src), c * cap, cap, src.stride(0) if b > 1 else c * n, _ptr(pos),
                                                  _ptr(counts), b, c, n, int(ring), _stream()), "agx_ring_write_pos_counted")
        return
    _lib.check(lib.agx_ring_write_pos(_ptr(buf), _ptr(src), c * cap, cap, src.stride(0) if b > 1 else c * n, _ptr(pos), b, c, n,
                                      int(ring), _stream()), "agx_ring_write_pos")


def stream_advance(pos: Tensor, n: int, counts: Optional[Tensor] = None) -> None:
    """``pos[b] += n`` on the device (exact int64 arithmetic): the advance of every row's stream by the ``n`` frames of a call.
    ``counts`` (int64 (B,), device): ``pos[b] += clamp(counts[b], 0, n)``, the frames every row took of a counted call."""
    lib = _lib.load()
    if not isinstance(pos, Tensor):
        raise AgxError(f"stream_advance: pos must be a contiguous int64 device tensor, got {type(pos).__name__}")
    pos = _checked_pos("stream_advance", pos, pos.numel(), pos.device)
    if counts is not None:
        counts = _checked_counts("stream_advance", counts, pos.numel(), pos.device)
        _lib.check(lib.agx_stream_advance_counted(_ptr(pos), _ptr(counts), pos.numel(), int(n), _stream()), "agx_stream_advance_counted")
        return
    _lib.check(lib.agx_stream_advance(_ptr(pos), pos.numel(), int(n), _stream()), "agx_stream_advance")


def dropout_add(x: Tensor, res: Optional[Tensor], p: float, seed: int, stream_id: int, out: Optional[Tensor] = None) -> Tensor:
    """``res + mask * x / (1 - p)`` (``res`` None: no residual) over a contiguous tensor, the mask that of include/agx.h for
    (``seed``, ``stream_id``) on the linear index.  ``out`` may be ``x`` (in place).  With ``res=None`` and the forward's
    arguments it is its own backward."""
    lib = _lib.load()
    _need_gpu(x, res, out)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise AgxError("dropout_add: x must be a contiguous float32 tensor (the mask is indexed by the linear position)")
    if res is not None:
        res = _f32c(res)
        if res.shape != x.shape:
            raise AgxError(f"dropout_add: residual is {tuple(res.shape)}, x is {tuple(x.shape)}")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise AgxError("dropout_add: out must be a contiguous float32 tensor of x's shape")
    tok = _observer.begin("other", ("dropout_add", 4 * x.numel() * (2 if res is None else 3))) if _observer is not None else None
    _lib.check(lib.agx_dropout_add(_ptr(x), _ptr(res), _ptr(out), x.numel(), *_drop_args(p, seed, stream_id), _stream()),
               "agx_dropout_add")
    if tok is not None:
        _observer.end(tok)
    return out


def conv_bwd_data_gelu(desc: ConvDesc, dy: Tensor, packed_bwd: Tensor, pre: Tensor, add: Optional[Tensor] = None) -> Tensor:
    """``conv_bwd_data`` followed (in the epilogue) by the exact-GELU gradient at the pre-activation ``pre``."""
    lib = _lib.load()
    _need_gpu(dy, packed_bwd, pre, add)
    dy, pre = _f32c(dy), _f32c(pre)
    add = None if add is None else _f32c(add)
    dx = torch.empty(desc.batch, desc.c_in, desc.l_in, dtype=torch.float32, device=dy.device)
    count_macs("conv_bwd_data", _conv_macs(desc), desc)
    _lib.check(lib.agx_conv_bwd_data_gelu(ctypes.byref(desc), _ptr(dy), _ptr(packed_bwd), _ptr(add), _ptr(pre), _ptr(dx),
                                          _stream()), "agx_conv_bwd_data_gelu")
    return dx


# ------------------------------------------------------------------ wavelet layers
def multires_forward(x: Tensor, h0: Tensor, h1: Tensor, w: Tensor, depth: int) -> Tensor:
    lib = _lib.load()
    _need_gpu(x, h0, h1, w)
    x = _f32c(x)
    b, c, length = x.shape
    k = h0.shape[-1]
    if tuple(h0.shape) != (c, 1, k) or tuple(h1.shape) != (c, 1, k) or tuple(w.shape) != (c, depth + 2):
        raise AgxError("multires_forward: parameter shapes do not match (C,1,K) / (C,depth+2)")
    y = torch.empty_like(x)
    _lib.check(lib.agx_multires_forward(_ptr(x), _ptr(_f32c(h0)), _ptr(_f32c(h1)), _ptr(_f32c(w)), _ptr(y),
                                        b, c, length, k, depth, _stream()), "agx_multires_forward")
    return y


def multires_backward(x: Tensor, dout: Tensor, h0: Tensor, h1: Tensor, w: Tensor, depth: int):
    """(dx, dh0, dh1, dw) of ``multires_forward``."""
    lib = _lib.load()
    _need_gpu(x, dout, h0, h1, w)
    x, dout = _f32c(x), _f32c(dout)
    b, c, length = x.shape
    k = h0.shape[-1]
    if dout.shape != x.shape or tuple(h0.shape) != (c, 1, k) or tuple(h1.shape) != (c, 1, k) or tuple(w.shape) != (c, depth + 2):
        raise AgxError("multires_backward: shapes do not match (B,C,L) / (C,1,K) / (C,depth+2)")
    dx, dh0, dh1, dw = torch.empty_like(x), torch.empty_like(h0), torch.empty_like(h1), torch.empty_like(w)
    nbytes = int(lib.agx_multires_backward_workspace_bytes(b, c, length, k, depth))
    ws = _workspace(nbytes, x.device, "agx_multires_backward_workspace_bytes")
    _lib.check(lib.agx_multires_backward(_ptr(x), _ptr(dout), _ptr(_f32c(h0)), _ptr(_f32c(h1)), _ptr(_f32c(w)), _ptr(dx),
                                         _ptr(dh0), _ptr(dh1), _ptr(dw), _ptr(ws), nbytes, b, c, length, k, depth,
                                         _stream()), "agx_multires_backward")
    return dx, dh0, dh1, dw


def group_sum(g: Tensor, group: int, gelu_pre: Optional[Tensor] = None) -> Tensor:
    """out[..., l] = sum_{j < group} g[..., l * group + j]  (adjoint of a nearest-neighbour upsample), times the exact-GELU
    derivative at ``gelu_pre[..., l]`` when given."""
    lib = _lib.load()
    _need_gpu(g, gelu_pre)
    g = _f32c(g)
    length = g.shape[-1]
    if group <= 0 or length % group:
        raise AgxError(f"group_sum: last dim {length} is not a multiple of {group}")
    out = torch.empty(*g.shape[:-1], length // group, dtype=torch.float32, device=g.device)
    if gelu_pre is not None:
        gelu_pre = _f32c(gelu_pre)
        if gelu_pre.shape != out.shape:
            raise AgxError(f"group_sum: gelu_pre is {tuple(gelu_pre.shape)}, output is {tuple(out.shape)}")
    _lib.check(lib.agx_group_sum(_ptr(g), _ptr(gelu_pre), _ptr(out), out.numel(), group, _stream()), "agx_group_sum")
    return out


def wavelet_fold(h: Tensor, space: Tensor, sigma: Tensor, scale: int) -> Tensor:
    lib = _lib.load()
    _need_gpu(h, space, sigma)
    h = _f32c(h)
    b, c, length = h.shape
    space = _f32c(space.reshape(-1))
    sigma = _f32c(sigma.reshape(-1))
    y = torch.empty((b, c, length * scale), dtype=torch.float32, device=h.device)
    _lib.check(lib.agx_wavelet_fold(_ptr(h), _ptr(space), _ptr(sigma), sigma.numel(), _ptr(y), b, c, length,
                                    space.numel(), scale, _stream()), "agx_wavelet_fold")
    return y


def wavelet_fold_backward(h: Tensor, dout: Tensor, space: Tensor, sigma: Tensor, scale: int):
    """(dh, dsigma) of ``wavelet_fold``; dsigma has sigma's number of elements."""
    lib = _lib.load()
    _need_gpu(h, dout, space, sigma)
    h, dout = _f32c(h), _f32c(dout)
    b, c, length = h.shape
    space = _f32c(space.reshape(-1))
    sig = _f32c(sigma.reshape(-1))
    dh = torch.empty_like(h)
    dsig = torch.empty_like(sig)
    ws = torch.empty(b * c, dtype=torch.float32, device=h.device)
    _lib.check(lib.agx_wavelet_fold_backward(_ptr(h), _ptr(dout), _ptr(space), _ptr(sig), sig.numel(), _ptr(dh),
                                             _ptr(dsig), _ptr(ws), b, c, length, space.numel(), scale, _stream()),
               "agx_wavelet_fold_backward")
    return dh, dsig.reshape(sigma.shape)


# ------------------------------------------------------------------ discriminators
def spectral_sigma(w: Tensor, u: Tensor, v: Tensor, power_iterations: int, eps: float = 1e-12) -> Tensor:
    """sigma (1-element device tensor) of ``w`` viewed as (dim 0, rest); ``u`` / ``v`` are updated IN PLACE
    when ``power_iterations > 0`` (torch spectral_norm in training mode)."""
    lib = _lib.load()
    _need_gpu(w, u, v)
    w = _f32c(w)
    rows, cols = w.shape[0], w.numel() // w.shape[0]
    assert u.is_contiguous() and v.is_contiguous() and u.numel() == rows and v.numel() == cols
    sigma = torch.empty(1, dtype=torch.float32, device=w.device)
    ws = torch.empty(rows + cols, dtype=torch.float32, device=w.device)
    _lib.check(lib.agx_spectral_sigma(_ptr(w), rows, cols, _ptr(u), _ptr(v), power_iterations, eps, _ptr(sigma),
                                      _ptr(ws), _stream()), "agx_spectral_sigma")
    return sigma


def conv_pack_sigma(desc: ConvDesc, w: Tensor, sigma: Tensor) -> Tensor:
    return _pack("agx_conv_packed_floats", "agx_conv_pack_sigma", desc, w, sigma)


def conv_pack_bwd_sigma(desc: ConvDesc, w: Tensor, sigma: Tensor) -> Tensor:
    return _pack("agx_conv_bwd_packed_floats", "agx_conv_pack_bwd_sigma", desc, w, sigma)


def conv_grouped_bwd_data(desc: ConvDesc, dz: Tensor, w: Tensor, sigma: Optional[Tensor] = None,
                          add: Optional[Tensor] = None, mask: Optional[Tensor] = None, slope: float = 0.2) -> Tensor:
    lib = _lib.load()
    _need_gpu(dz, w, sigma, add, mask)
    dz, w = _f32c(dz), _f32c(w)
    add = None if add is None else _f32c(add)
    mask = None if mask is None else _f32c(mask)
    dx = torch.empty(desc.batch, desc.c_in, desc.l_in, dtype=torch.float32, device=dz.device)
    count_macs("conv_bwd_data", _conv_macs(desc), desc)
    _lib.check(lib.agx_conv_grouped_bwd_data(ctypes.byref(desc), _ptr(dz), _ptr(w), _ptr(sigma), _ptr(add), _ptr(mask),
                                             slope, _ptr(dx), _stream()), "agx_conv_grouped_bwd_data")
    return dx


def conv_grouped_bwd_weight(desc: ConvDesc, x: Tensor, dz: Tensor, want_bias: bool = True):
    """Plain (dw, dbias) of a grouped AGX_CONV_PADDED layer; dw has the torch layout (c_out, c_in / groups, K)."""
    lib = _lib.load()
    _need_gpu(x, dz)
    x, dz = _f32c(x), _f32c(dz)
    g = max(desc.groups, 1)
    dw = torch.empty(desc.c_out, desc.c_in // g, desc.kernel, dtype=torch.float32, device=x.device)
    db = torch.empty(desc.c_out, dtype=torch.float32, device=x.device) if want_bias else None
    nbytes = int(lib.agx_conv_grouped_bwd_weight_workspace_bytes(ctypes.byref(desc)))
    ws = _workspace(nbytes, x.device, "agx_conv_grouped_bwd_weight_workspace_bytes")
    count_macs("conv_bwd_weight", _conv_macs(desc), desc)
    _lib.check(lib.agx_conv_grouped_bwd_weight(ctypes.byref(desc), _ptr(x), _ptr(dz), _ptr(dw), _ptr(db), _ptr(ws),
                                               nbytes, _stream()), "agx_conv_grouped_bwd_weight")
    return dw, db


def conv_grouped_bwd_weight_kernel_name(desc: ConvDesc) -> str:
    """What ``conv_grouped_bwd_weight`` runs: "<kernel> op=none slices=.. items=.." (include/agx.h)."""
    return _kernel_name("agx_conv_grouped_bwd_weight_kernel_name", desc, size=128)


def avgpool1d(x: Tensor, kernel: int, stride: int, padding: int) -> Tensor:
    lib = _lib.load()
    _need_gpu(x)
    x = _f32c(x)
    l_in = x.shape[-1]
    l_out = lib.agx_avgpool1d_out_len(l_in, kernel, stride, padding)
    if l_out < 0:
        _lib.check(int(l_out), "agx_avgpool1d_out_len")
    rows = x.numel() // l_in
    y = torch.empty(*x.shape[:-1], int(l_out), dtype=torch.float32, device=x.device)
    _lib.check(lib.agx_avgpool1d(_ptr(x), _ptr(y), rows, l_in, kernel, stride, padding, _stream()), "agx_avgpool1d")
    return y


def conv2d_desc(batch, c_in, c_out, h_in, w_in, kh, kw, stride=(1, 1), padding=(0, 0), epilogue=0, slope=0.2,
                impl=IMPL_AUTO) -> _lib.Conv2dDesc:
    return _lib.Conv2dDesc(batch, c_in, c_out, h_in, w_in, kh, kw, stride[0], stride[1], padding[0], padding[1],
                           epilogue, slope, impl)


def conv2d_pack(desc, w: Tensor, sigma: Optional[Tensor] = None) -> Tensor:
    return _pack("agx_conv2d_packed_floats", "agx_conv2d_pack", desc, w, sigma)


def conv2d_forward(desc, x: Tensor, packed: Tensor, bias: Optional[Tensor]) -> Tensor:
    lib = _lib.load()
    _need_gpu(x, packed, bias)
    x = _f32c(x)
    ho, wo = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(lib.agx_conv2d_out_shape(ctypes.byref(desc), ctypes.byref(ho), ctypes.byref(wo)), "agx_conv2d_out_shape")
    y = torch.empty(desc.batch, desc.c_out, ho.value, wo.value, dtype=torch.float32, device=x.device)
    bias = None if bias is None else _f32c(bias)
    tok = _observer.begin("other", ("conv2d:bf16x3" if desc.impl == _lib.IMPL_MFMA_BF16X3 else "conv2d", 4 * (x.numel() + y.numel()),
                                     _conv2d_macs(desc))) if _observer is not None else None
    _lib.check(lib.agx_conv2d_forward(ctypes.byref(desc), _ptr(x), _ptr(packed), _ptr(bias), _ptr(y), _stream()),
               "agx_conv2d_forward")
    if tok is not None:
        _observer.end(tok)
    return y


def conv2d_pack_bwd(desc, w: Tensor, sigma: Optional[Tensor] = None) -> Tensor:
    return _pack("agx_conv2d_bwd_packed_floats", "agx_conv2d_pack_bwd", desc, w, sigma)


def conv2d_bwd_data(desc, dy: Tensor, packed_bwd: Tensor, mask: Optional[Tensor] = None, slope: float = 0.2,
                    add: Optional[Tensor] = None) -> Tensor:
    """Gradient w.r.t. the input of the Conv2d layer ``desc`` describes (forward descriptor); ``add`` is summed
    in and the LeakyReLU gradient (``mask``) applied in the kernel's epilogue."""
    lib = _lib.load()
    _need_gpu(dy, packed_bwd, mask, add)
    dy = _f32c(dy)
    mask = None if mask is None else _f32c(mask)
    add = None if add is None else _f32c(add)
    dx = torch.empty(desc.batch, desc.c_in, desc.h_in, desc.w_in, dtype=torch.float32, device=dy.device)
    count_macs("conv2d_bwd_data", _conv2d_macs(desc), desc)
    _lib.check(lib.agx_conv2d_bwd_data(ctypes.byref(desc), _ptr(dy), _ptr(packed_bwd), _ptr(add), _ptr(mask), slope,
                                       _ptr(dx), _stream()), "agx_conv2d_bwd_data")
    return dx


def conv2d_bwd_weight(desc, x: Tensor, dy: Tensor, w: Optional[Tensor] = None, sigma: Optional[Tensor] = None,
                      u: Optional[Tensor] = None, v: Optional[Tensor] = None, want_bias: bool = True):
    """(dw, dbias or None); with ``sigma`` the spectral-norm chain rule is applied (dw w.r.t. weight_orig)."""
    lib = _lib.load()
    _need_gpu(x, dy, w, sigma, u, v)
    x, dy = _f32c(x), _f32c(dy)
    dw = torch.empty(desc.c_out, desc.c_in, desc.kh, desc.kw, dtype=torch.float32, device=x.device)
    db = torch.empty(desc.c_out, dtype=torch.float32, device=x.device) if want_bias else None
    nbytes = int(lib.agx_conv2d_bwd_weight_workspace_bytes(ctypes.byref(desc)))
    ws = _workspace(nbytes, x.device, "agx_conv2d_bwd_weight_workspace_bytes")
    w = None if w is None else _f32c(w)
    count_macs("conv2d_bwd_weight", _conv2d_macs(desc), desc)
    _lib.check(lib.agx_conv2d_bwd_weight(ctypes.byref(desc), _ptr(x), _ptr(dy), _ptr(w), _ptr(sigma), _ptr(u), _ptr(v),
                                         _ptr(dw), _ptr(db), _ptr(ws), nbytes, _stream()), "agx_conv2d_bwd_weight")
    return dw, db


def conv2d_bwd_data_fewchannels(desc, dy: Tensor, w: Tensor, sigma: Optional[Tensor] = None,
                                add: Optional[Tensor] = None) -> Tensor:
    """Backward-data of a stride-1 Conv2d with very few input channels (c_in * kw >= 8 rows on the MFMA tiles instead
    of c_in): auxiliary (kh x 1) conv over dy, then a column fold (include/agx.h: agx_conv2d_colsplit_weights)."""
    lib = _lib.load()
    _need_gpu(dy, w, sigma, add)
    dy, w = _f32c(dy), _f32c(w)
    add = None if add is None else _f32c(add)
    wp = torch.empty(desc.c_in * desc.kw, desc.c_out, desc.kh, 1, dtype=torch.float32, device=dy.device)
    _lib.check(lib.agx_conv2d_colsplit_weights(ctypes.byref(desc), _ptr(w), _ptr(sigma), _ptr(wp), _stream()),
               "agx_conv2d_colsplit_weights")
    aux = conv2d_desc(desc.batch, desc.c_out, desc.c_in * desc.kw, dy.shape[2], dy.shape[3], desc.kh, 1, (1, 1),
                      (desc.kh - 1 - desc.pad_h, 0))
    pbuf = conv2d_forward(aux, dy, conv2d_pack(aux, wp), None)
    dx = torch.empty(desc.batch, desc.c_in, desc.h_in, desc.w_in, dtype=torch.float32, device=dy.device)
    _lib.check(lib.agx_conv2d_colsum(ctypes.byref(desc), _ptr(pbuf), _ptr(add), _ptr(dx), _stream()), "agx_conv2d_colsum")
    return dx


def conv2d_kernel_name(desc) -> str:
    return _kernel_name("agx_conv2d_kernel_name", desc)


def conv2d_bwd_data_kernel_name(desc) -> str:
    return _kernel_name("agx_conv2d_bwd_data_kernel_name", desc)


def conv2d_bwd_weight_kernel_name(desc) -> str:
    """What ``conv2d_bwd_weight`` runs: "<kernel> cfg=.. op=.. slices=.. items=.." (include/agx.h)."""
    return _kernel_name("agx_conv2d_bwd_weight_kernel_name", desc, size=128)


_STFT_IMAGES = {}
_DEVICE_CACHES = (_STFT_IMAGES,)     # every module-level cache that keeps device buffers across calls


def _stft_image_and_workspace(backward: bool, b: int, length: int, n_fft: int, normalized: bool, device):
    """The cached weight image of one direction (packed on first use) and a fresh workspace."""
    lib = _lib.load()
    key = (bool(backward), n_fft, bool(normalized), device)
    if key not in _STFT_IMAGES:
        pack, name = (lib.agx_stft_pack_bwd, "agx_stft_pack_bwd") if backward else (lib.agx_stft_pack, "agx_stft_pack")
        img = torch.empty(int(lib.agx_stft_packed_floats(n_fft)), dtype=torch.float32, device=device)
        _lib.check(pack(n_fft, int(normalized), _ptr(img), _stream()), name)
        _STFT_IMAGES[key] = img
    ws = _workspace(lib.agx_stft_workspace_bytes(b, length, n_fft), device, "agx_stft_workspace_bytes")
    return _STFT_IMAGES[key], ws


def stft(x: Tensor, n_fft: int, normalized: bool = True) -> Tensor:
    """(B, L) -> (B, 2, T, n_fft): two-sided rectangular-window STFT, hop n_fft / 4, reflect-centred."""
    lib = _lib.load()
    _need_gpu(x)
    x = _f32c(x)
    b, length = x.shape
    t = lib.agx_stft_frames(length, n_fft)
    if t < 0:
        _lib.check(int(t), "agx_stft_frames")
    img, ws = _stft_image_and_workspace(False, b, length, n_fft, normalized, x.device)
    y = torch.empty(b, 2, int(t), n_fft, dtype=torch.float32, device=x.device)
    tok = _observer.begin("other", ("stft", 4 * (x.numel() + y.numel()), b * 2 * n_fft * n_fft * int(t))) if _observer is not None else None
    _lib.check(lib.agx_stft_forward(_ptr(x), _ptr(img), _ptr(y), _ptr(ws), b, length, n_fft, _stream()), "agx_stft_forward")
    if tok is not None:
        _observer.end(tok)
    return y


def stft_backward(dy: Tensor, length: int, n_fft: int, normalized: bool = True) -> Tensor:
    """Adjoint of ``stft``: (B, 2, T, n_fft) -> (B, L)."""
    lib = _lib.load()
    _need_gpu(dy)
    dy = _f32c(dy)
    b = dy.shape[0]
    img, ws = _stft_image_and_workspace(True, b, length, n_fft, normalized, dy.device)
    dx = torch.empty(b, length, dtype=torch.float32, device=dy.device)
    count_macs("stft_backward", b * 2 * n_fft * n_fft * dy.shape[2])
    _lib.check(lib.agx_stft_backward(_ptr(dy), _ptr(img), _ptr(dx), _ptr(ws), b, length, n_fft, _stream()), "agx_stft_backward")
    return dx


def avgpool1d_backward(dy: Tensor, l_in: int, kernel: int, stride: int, padding: int,
                       add: Optional[Tensor] = None) -> Tensor:
    lib = _lib.load()
    _need_gpu(dy, add)
    dy = _f32c(dy)
    add = None if add is None else _f32c(add)
    rows = dy.numel() // dy.shape[-1]
    dx = torch.empty(*dy.shape[:-1], l_in, dtype=torch.float32, device=dy.device)
    _lib.check(lib.agx_avgpool1d_backward(_ptr(dy), _ptr(add), _ptr(dx), rows, l_in, kernel, stride, padding, _stream()),
               "agx_avgpool1d_backward")
    return dx


def sigmoid_backward(dy: Tensor, s: Tensor) -> Tensor:
    lib = _lib.load()
    _need_gpu(dy, s)
    dy, s = _f32c(dy), _f32c(s)
    dz = torch.empty_like(s)
    _lib.check(lib.agx_sigmoid_backward(_ptr(dy), _ptr(s), _ptr(dz), s.numel(), _stream()), "agx_sigmoid_backward")
    return dz


def spectral_grad_(g: Tensor, w: Tensor, sigma: Tensor, u: Tensor, v: Tensor) -> Tensor:
    """In place: plain weight gradient -> gradient w.r.t. weight_orig of a spectrally normalised layer."""
    lib = _lib.load()
    _need_gpu(g, w, sigma, u, v)
    assert g.is_contiguous() and g.dtype == torch.float32
    rows, cols = g.shape[0], g.numel() // g.shape[0]
    ws = torch.empty(rows, dtype=torch.float32, device=g.device)
    _lib.check(lib.agx_spectral_grad(_ptr(g), _ptr(_f32c(w)), _ptr(sigma), _ptr(u), _ptr(v), rows, cols, _ptr(ws),
                                     _stream()), "agx_spectral_grad")
    return g


REDUCE_MEAN, REDUCE_HINGE_REAL, REDUCE_HINGE_FAKE, REDUCE_L1, REDUCE_ABS_EPS = 0, 1, 2, 3, 4


def reduce_mean(x: Tensor, mode: int, y: Optional[Tensor] = None) -> Tensor:
    """One of the means of ``discriminator_generator_loss`` as a 0-d device tensor."""
    lib = _lib.load()
    _need_gpu(x, y)
    x = _f32c(x)
    y = None if y is None else _f32c(y)
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = torch.empty(1024, dtype=torch.float32, device=x.device)
    _lib.check(lib.agx_reduce_mean(_ptr(x), _ptr(y), x.numel(), mode, _ptr(out), _ptr(ws), _stream()),
               "agx_reduce_mean")
    return out[0]


def reduce_mean_backward(x: Tensor, mode: int, grad: Tensor, y: Optional[Tensor] = None, want_dy: bool = False):
    lib = _lib.load()
    _need_gpu(x, y, grad)
    x = _f32c(x)
    y = None if y is None else _f32c(y)
    grad = _f32c(grad.reshape(1))
    dx = torch.empty_like(x)
    dy = torch.empty_like(x) if want_dy else None
    _lib.check(lib.agx_reduce_mean_backward(_ptr(x), _ptr(y), x.numel(), mode, _ptr(grad), _ptr(dx), _ptr(dy),
                                            _stream()), "agx_reduce_mean_backward")
    return dx, dy


def feature_means(x: Tensor, y: Tensor) -> Tensor:
    """(mean|x - y|, mean|x + 1e-3|) of one feature-matching term in one pass: a 2-element device tensor."""
    lib = _lib.load()
    _need_gpu(x, y)
    x, y = _f32c(x), _f32c(y)
    if x.shape != y.shape:
        raise AgxError(f"feature_means: shapes differ ({tuple(x.shape)} vs {tuple(y.shape)})")
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    ws = torch.empty(2048, dtype=torch.float32, device=x.device)
    _lib.check(lib.agx_feature_means(_ptr(x), _ptr(y), x.numel(), _ptr(out), _ptr(ws), _stream()), "agx_feature_means")
    return out


def feature_means_backward(x: Tensor, y: Tensor, grad: Tensor, want_dx: bool = True, want_dy: bool = True):
    lib = _lib.load()
    _need_gpu(x, y, grad)
    x, y = _f32c(x), _f32c(y)
    grad = _f32c(grad.reshape(2))
    dx = torch.empty_like(x) if want_dx else None
    dy = torch.empty_like(x) if want_dy else None
    if dx is None and dy is None:
        return None, None
    _lib.check(lib.agx_feature_means_backward(_ptr(x), _ptr(y), x.numel(), _ptr(grad), _ptr(dx), _ptr(dy), _stream()),
               "agx_feature_means_backward")
    return dx, dy


def sigmoid(x: Tensor) -> Tensor:
    lib = _lib.load()
    _need_gpu(x)
    x = _f32c(x)
    y = torch.empty_like(x)
    _lib.check(lib.agx_sigmoid(_ptr(x), _ptr(y), x.numel(), _stream()), "agx_sigmoid")
    return y


# ------------------------------------------------------------------ bitstream
def codes_pack(index: Tensor, bits: int) -> Tensor:
    """(..,) int64 codes -> uint8 stream, `bits` bits per code (dense, little-endian)."""
    lib = _lib.load()
    _need_gpu(index)
    idx = index.contiguous().to(torch.int64)
    n = idx.numel()
    nbytes = lib.agx_codes_packed_bytes(n, bits)
    if nbytes < 0 or n == 0:
        raise AgxError(f"codes_pack: bad arguments (n={n}, bits={bits})")
    out = torch.empty(int(nbytes), dtype=torch.uint8, device=idx.device)
    _lib.check(lib.agx_codes_pack(_ptr(idx), n, bits, _ptr(out), _stream()), "agx_codes_pack")
    return out


def codes_unpack(stream: Tensor, n_codes: int, bits: int) -> Tensor:
    lib = _lib.load()
    _need_gpu(stream)
    if stream.dtype != torch.uint8 or stream.numel() < lib.agx_codes_packed_bytes(n_codes, bits):
        raise AgxError("codes_unpack: stream must be uint8 and hold ceil(n_codes*bits/8) bytes")
    out = torch.empty(n_codes, dtype=torch.int64, device=stream.device)
    _lib.check(lib.agx_codes_unpack(_ptr(stream.contiguous()), n_codes, bits, _ptr(out), _stream()), "agx_codes_unpack")
    return out


# ------------------------------------------------------------------ time folding (longform.py)
def _fold_operand(x: Tensor, what: str) -> Tensor:
    _need_gpu(x)
    if x.dtype != torch.float32 or x.dim() != 3 or not x.is_contiguous():
        raise AgxError(f"{what}: expected a contiguous float32 (B, C, L) tensor, got {x.dtype} {tuple(x.shape)}"
                       f"{'' if x.is_contiguous() else ' (not contiguous)'}")
    return x


def time_fold(x: Tensor, windows: int, hop: int, width: int, src_off: int = 0) -> Tensor:
    """(B, C, L) -> (B*windows, C, width): ``out[b*S + s, c, j] = x[b, c, src_off + s*hop + j]`` (overlapping windows)."""
    lib = _lib.load()
    x = _fold_operand(x, "time_fold")
    b, c, length = x.shape
    windows, hop, width, src_off = int(windows), int(hop), int(width), int(src_off)
    if windows < 1 or width < 1 or hop < 0 or src_off < 0 or src_off + (windows - 1) * hop + width > length:
        raise AgxError(f"time_fold: {windows} windows of {width} at hop {hop} from {src_off} leave the source (L = {length})")
    out = torch.empty((b * windows, c, width), dtype=torch.float32, device=x.device)
    _lib.check(lib.agx_time_fold(_ptr(x), _ptr(out), b, c, length, windows, hop, width, src_off, _stream()), "agx_time_fold")
    return out


def time_unfold(src: Tensor, out: Tensor, windows: int, keep: int, src_off: int = 0, dst_off: int = 0,
                n_win: Optional[int] = None) -> Tensor:
    """Crop-and-place into ``out`` (B, C, L'): ``out[b, c, dst_off + s*keep + j] = src[b*S + s, c, src_off + j]`` for
    ``j < keep`` and ``s < n_win`` (default: all ``S = windows``).  Returns ``out``."""
    lib = _lib.load()
    src, out = _fold_operand(src, "time_unfold"), _fold_operand(out, "time_unfold")
    windows, keep, src_off, dst_off = int(windows), int(keep), int(src_off), int(dst_off)
    n_win = windows if n_win is None else int(n_win)
    b, c, length = out.shape
    if windows < 1 or src.shape[0] != b * windows or src.shape[1] != c or src.device != out.device:
        raise AgxError(f"time_unfold: source {tuple(src.shape)} is not {windows} windows per clip of {tuple(out.shape)}")
    width = src.shape[2]
    if not (1 <= n_win <= windows) or keep < 1 or src_off < 0 or dst_off < 0 or src_off + keep > width \
            or dst_off + n_win * keep > length:
        raise AgxError(f"time_unfold: crop [{src_off}, {src_off + keep}) of width {width} x {n_win} windows placed at {dst_off} "
                       f"does not fit (L = {length})")
    _lib.check(lib.agx_time_unfold(_ptr(src), _ptr(out), b, c, windows, width, length, n_win, src_off, dst_off, keep, _stream()),
               "agx_time_unfold")
    return out


# ------------------------------------------------------------------ conditioning (conditioning.py)
FILM_CT, FILM_TC = _lib.FILM_CT, _lib.FILM_TC


def _film_shape(op: str, x: Tensor, gb: Tensor, has_beta: bool, layout: int):
    """(B, C, T) of a FiLM operand in ``layout``; ``gb`` must be the (B, C) or (B, 2 C) tensor that goes with it."""
    if layout not in (FILM_CT, FILM_TC):
        raise AgxError(f"{op}: layout = {layout!r} is neither FILM_CT nor FILM_TC")
    if x.dim() != 3:
        raise AgxError(f"{op}: x is {tuple(x.shape)}, expected three dimensions")
    b, c, t = x.shape if layout == FILM_CT else (x.shape[0], x.shape[2], x.shape[1])
    if tuple(gb.shape) != (b, (2 if has_beta else 1) * c):
        raise AgxError(f"{op}: gb is {tuple(gb.shape)}, expected {(b, (2 if has_beta else 1) * c)}")
    return b, c, t


def _same_out(op: str, x: Tensor, out: Optional[Tensor]) -> Tensor:
    """``out`` of an elementwise op over contiguous ``x``: a new tensor, or the caller's (``x`` itself: in place)."""
    if out is None:
        return torch.empty_like(x)
    if out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise AgxError(f"{op}: out must be a contiguous float32 tensor of x's shape")
    return out


def _elementwise(op: str, lib, symbol: str, x: Tensor, out: Optional[Tensor], traffic: Optional[int], args) -> Tensor:
    """What every elementwise wrapper ends in: ``x`` must be contiguous float32, ``out`` is checked against it (or made), and
    ``symbol(*args(out), stream)`` runs -- under the observer, as ``traffic`` bytes per element, unless ``traffic`` is None."""
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise AgxError(f"{op}: x must be a contiguous float32 tensor")
    out = _same_out(op, x, out)
    tok = _observer.begin("other", (op, traffic * x.numel())) if traffic is not None and _observer is not None else None
    _lib.check(getattr(lib, symbol)(*args(out), _stream()), symbol)
    if tok is not None:
        _observer.end(tok)
    return out


def film_params(cond: Tensor, w: Tensor, bias: Optional[Tensor]) -> Tensor:
    """``gb[b, r] = bias[r] + sum_d cond[b, d] w[r, d]``: cond (B, D), w (R, D), bias (R) or None -> (B, R)."""
    lib = _lib.load()
    _need_gpu(cond, w, bias)
    cond, w = _f32c(cond), _f32c(w)
    if cond.dim() != 2 or w.dim() != 2 or cond.shape[1] != w.shape[1] or (bias is not None and tuple(bias.shape) != (w.shape[0],)):
        raise AgxError(f"film_params: cond {tuple(cond.shape)}, w {tuple(w.shape)}, bias "
                       f"{None if bias is None else tuple(bias.shape)}: expected (B, D), (R, D), (R,)")
    (b, d), r = cond.shape, w.shape[0]
    gb = torch.empty((b, r), dtype=torch.float32, device=cond.device)
    tok = _observer.begin("other", ("film_params", 4 * (cond.numel() + b * w.numel() + gb.numel()))) if _observer is not None else None
    _lib.check(lib.agx_film_params(_ptr(cond), _ptr(w), _ptr(None if bias is None else _f32c(bias)), _ptr(gb), b, d, r,
                                   _stream()), "agx_film_params")
    if tok is not None:
        _observer.end(tok)
    return gb


def film_apply(x: Tensor, gb: Tensor, has_beta: bool, layout: int = FILM_CT, out: Optional[Tensor] = None) -> Tensor:
    """``x * gamma + beta`` per (batch row, channel): x (B, C, T) for FILM_CT or (B, T, C) for FILM_TC, gb (B, 2 C) -- gamma
    then beta -- or (B, C) without beta.  ``out`` may be ``x`` (in place)."""
    lib = _lib.load()
    _need_gpu(x, gb, out)
    b, c, t = _film_shape("film_apply", x, gb, has_beta, layout)
    return _elementwise("film_apply", lib, "agx_film_apply", x, out, 8,
                        lambda out: (_ptr(x), _ptr(_f32c(gb)), _ptr(out), b, c, t, int(bool(has_beta)), int(layout)))


def film_backward(x: Tensor, gb: Tensor, dout: Tensor, has_beta: bool, layout: int = FILM_CT):
    """(dx, dgb) of ``film_apply``: ``dx = dout * gamma``; ``dgb`` has gb's shape, ``sum_t dout * x`` then (with beta)
    ``sum_t dout``.  One pass, no atomics; bitwise the same in both layouts."""
    lib = _lib.load()
    _need_gpu(x, gb, dout)
    b, c, t = _film_shape("film_backward", x, gb, has_beta, layout)
    if dout.shape != x.shape:
        raise AgxError(f"film_backward: dout is {tuple(dout.shape)}, x is {tuple(x.shape)}")
    x, dout = _f32c(x), _f32c(dout)
    dx = torch.empty_like(x)
    dgb = torch.empty((b, gb.shape[1]), dtype=torch.float32, device=x.device)
    _lib.check(lib.agx_film_backward(_ptr(x), _ptr(_f32c(gb)), _ptr(dout), _ptr(dx), _ptr(dgb), b, c, t, int(bool(has_beta)),
                                     int(layout), _stream()), "agx_film_backward")
    return dx, dgb


def film_params_backward(cond: Tensor, w: Tensor, dgb: Tensor, want_dcond: bool = True):
    """(dw (R, D), dbias (R), dcond (B, D) or None) of ``film_params``."""
    lib = _lib.load()
    _need_gpu(cond, w, dgb)
    cond, w, dgb = _f32c(cond), _f32c(w), _f32c(dgb)
    (b, d), r = cond.shape, w.shape[0]
    if tuple(w.shape) != (r, d) or tuple(dgb.shape) != (b, r):
        raise AgxError(f"film_params_backward: cond {tuple(cond.shape)}, w {tuple(w.shape)}, dgb {tuple(dgb.shape)}: expected "
                       "(B, D), (R, D), (B, R)")
    dw = torch.empty_like(w)
    dbias = torch.empty(r, dtype=torch.float32, device=w.device)
    dcond = torch.empty_like(cond) if want_dcond else None
    _lib.check(lib.agx_film_params_backward(_ptr(cond), _ptr(w), _ptr(dgb), _ptr(dw), _ptr(dbias), _ptr(dcond), b, d, r,
                                            _stream()), "agx_film_params_backward")
    return dw, dbias, dcond


def sigmoid_gate(x: Tensor, z: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """``x * sigmoid(z)`` elementwise; ``out`` may be ``x`` (in place)."""
    lib = _lib.load()
    _need_gpu(x, z, out)
    if x.dtype != torch.float32 or not x.is_contiguous() or z.shape != x.shape:
        raise AgxError(f"sigmoid_gate: x must be a contiguous float32 tensor and z of its shape (x {tuple(x.shape)}, z {tuple(z.shape)})")
    return _elementwise("sigmoid_gate", lib, "agx_sigmoid_gate", x, out, 12, lambda out: (_ptr(x), _ptr(_f32c(z)), _ptr(out), x.numel()))


def sigmoid_gate_backward(x: Tensor, z: Tensor, dout: Tensor):
    """(dx, dz) of ``sigmoid_gate``: ``dout * s`` and ``dout * x * s * (1 - s)`` with ``s = sigmoid(z)``, one launch."""
    lib = _lib.load()
    _need_gpu(x, z, dout)
    if z.shape != x.shape or dout.shape != x.shape:
        raise AgxError(f"sigmoid_gate_backward: x {tuple(x.shape)}, z {tuple(z.shape)}, dout {tuple(dout.shape)} differ in shape")
    x, z, dout = _f32c(x), _f32c(z), _f32c(dout)
    dx, dz = torch.empty_like(x), torch.empty_like(x)
    _lib.check(lib.agx_sigmoid_gate_backward(_ptr(x), _ptr(z), _ptr(dout), _ptr(dx), _ptr(dz), x.numel(), _stream()),
               "agx_sigmoid_gate_backward")
    return dx, dz


# ------------------------------------------------------------------ snake activations (utils.py:44-105)
SNAKE_PLAIN, SNAKE_RELU = _lib.SNAKE_PLAIN, _lib.SNAKE_RELU


def _snake_shape(op: str, x: Tensor, alpha: Tensor, variant: int):
    """(rows, channels, n) of a snake operand: x is (B, C, ...), rows = B * C, and ``alpha`` holds C floats or one."""
    if variant not in (SNAKE_PLAIN, SNAKE_RELU):
        raise AgxError(f"{op}: variant = {variant!r} is neither SNAKE_PLAIN nor SNAKE_RELU")
    if x.dim() < 2:
        raise AgxError(f"{op}: x is {tuple(x.shape)}, expected (B, C, ...)")
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise AgxError(f"{op}: x must be a contiguous float32 tensor (x {tuple(x.shape)}, {x.dtype})")
    channels = alpha.numel()
    if channels not in (1, x.shape[1]):
        raise AgxError(f"{op}: x is {tuple(x.shape)} and has {x.shape[1]} channels, alpha {tuple(alpha.shape)} holds {channels}")
    rows = x.shape[0] * x.shape[1]
    return rows, channels, (x.numel() // rows if rows else 0)


def snake_forward(x: Tensor, alpha: Tensor, variant: int, eps: float = 1e-6, out: Optional[Tensor] = None) -> Tensor:
    """``(max(x, 0) if variant else x) + sin(alpha x)^2 / (alpha + eps)`` per channel: x (B, C, ...), alpha of C elements or
    of one (every channel).  ``out`` may be ``x`` (in place).  One launch."""
    lib = _lib.load()
    _need_gpu(x, alpha, out)
    rows, channels, n = _snake_shape("snake_forward", x, alpha, variant)
    return _elementwise("snake_forward", lib, "agx_snake_forward", x, out, 8,
                        lambda out: (_ptr(x), _ptr(_f32c(alpha)), _ptr(out), rows, channels, n, int(variant), float(eps)))


def snake_backward(x: Tensor, alpha: Tensor, dout: Tensor, variant: int, eps: float = 1e-6, want_dx: bool = True,
                   want_dalpha: bool = True):
    """(dx or None, dalpha or None) of ``snake_forward``; ``dalpha`` has C (or one) elements.  Without ``dalpha`` one
    element-wise launch; with it one pass that writes ``dx`` and per-segment partial sums, and a second launch that adds them
    per channel in a fixed order."""
    lib = _lib.load()
    _need_gpu(x, alpha, dout)
    rows, channels, n = _snake_shape("snake_backward", x, alpha, variant)
    if dout.shape != x.shape:
        raise AgxError(f"snake_backward: dout is {tuple(dout.shape)}, x is {tuple(x.shape)}")
    alpha, dout = _f32c(alpha), _f32c(dout)
    dx = torch.empty_like(x) if want_dx else None
    dalpha = ws = None
    nbytes = 0
    if want_dalpha:
        if x.numel() == 0:          # nothing is launched: the empty sum
            return dx, torch.zeros(channels, dtype=torch.float32, device=x.device)
        dalpha = torch.empty(channels, dtype=torch.float32, device=x.device)
        nbytes = int(lib.agx_snake_backward_workspace_bytes(rows, channels, n))
        ws = _workspace(nbytes, x.device, "agx_snake_backward_workspace_bytes")
    _lib.check(lib.agx_snake_backward(_ptr(x), _ptr(alpha), _ptr(dout), _ptr(dx), _ptr(dalpha), _ptr(ws), nbytes, rows, channels, n,
                                      int(variant), float(eps), _stream()), "agx_snake_backward")
    return dx, dalpha


# ------------------------------------------------------------------ Conformer convolution module (transformers.py:281-335)
CONFORMER_MAX_K = _lib.CONFORMER_MAX_K


def _glu_shape(op: str, u: Tensor, w: Tensor):
    """(B, C, T, K) of the fused GLU + depthwise conv: u (B, 2 C, T), w (C, 1, K) or (C, K)."""
    if u.dim() != 3 or u.shape[1] % 2 or u.dtype != torch.float32 or not u.is_contiguous():
        raise AgxError(f"{op}: u must be a contiguous float32 (B, 2 C, T) tensor, got {tuple(u.shape)} {u.dtype}")
    b, c2, t = u.shape
    c = c2 // 2
    if w.dim() not in (2, 3) or w.shape[0] != c or w.numel() != c * w.shape[-1]:
        raise AgxError(f"{op}: w is {tuple(w.shape)}, expected ({c}, 1, K): one filter per channel")
    k = w.shape[-1]
    if not 1 <= k <= CONFORMER_MAX_K:
        raise AgxError(f"{op}: kernel_size = {k} is outside [1, {CONFORMER_MAX_K}]")
    return b, c, t, k


def _bn_vectors(op: str, c: int, *vectors: Tensor):
    for v in vectors:
        if v.numel() != c:
            raise AgxError(f"{op}: a per-channel vector holds {v.numel()} floats, the tensor has {c} channels")
    return tuple(_f32c(v) for v in vectors)


def _bct(op: str, *tensors: Tensor):
    x = tensors[0]
    if x.dim() != 3:
        raise AgxError(f"{op}: expected (B, C, T), got {tuple(x.shape)}")
    for t in tensors:
        if t.shape != x.shape or t.dtype != torch.float32 or not t.is_contiguous():
            raise AgxError(f"{op}: operands must be contiguous float32 tensors of one shape {tuple(x.shape)}, got {tuple(t.shape)} {t.dtype}")
    return x.shape


def _glu_hist(op: str, hist: Optional[Tensor], b: int, c: int, k: int) -> None:
    """A conv state is a contiguous float32 (B, C, K - 1) tensor: it is written in place, so it is never copied."""
    if hist is not None and (tuple(hist.shape) != (b, c, k - 1) or hist.dtype != torch.float32 or not hist.is_contiguous()):
        raise AgxError(f"{op}: hist must be a contiguous float32 {(b, c, k - 1)} tensor (B, C, K - 1), got {tuple(hist.shape)} {hist.dtype}")


def _glu_dwconv_forward(op: str, symbol: str, u: Tensor, w: Tensor, bias: Tensor, bn: Optional[tuple], eps: float, hist: tuple) -> Tensor:
    """``glu_dwconv`` (``hist`` = ()) and ``glu_dwconv_causal`` (``hist`` = (the state or None,), an operand of its symbol)."""
    lib = _lib.load()
    _need_gpu(u, w, bias, *hist, *(bn or ()))
    b, c, t, k = _glu_shape(op, u, w)
    w, (bias,) = _f32c(w), _bn_vectors(op, c, bias)
    bn = (None,) * 4 if bn is None else _bn_vectors(op, c, *bn)
    for h in hist:
        _glu_hist(op, h, b, c, k)
    out = torch.empty((b, c, t), dtype=torch.float32, device=u.device)
    tok = _observer.begin("other", (op, 12 * out.numel())) if _observer is not None else None
    _lib.check(getattr(lib, symbol)(_ptr(u), _ptr(w), _ptr(bias), *(_ptr(v) for v in bn), float(eps), *(_ptr(h) for h in hist), _ptr(out),
                                    b, c, t, k, _stream()), symbol)
    if tok is not None:
        _observer.end(tok)
    return out


def _glu_dwconv_backward(op: str, symbol: str, dz: Tensor, u: Tensor, w: Tensor, want_du: bool, want_params: bool):
    """``glu_dwconv_backward`` and ``glu_dwconv_causal_backward``: ``symbol`` and its ``_workspace_bytes`` query."""
    lib = _lib.load()
    _need_gpu(dz, u, w)
    b, c, t, k = _glu_shape(op, u, w)
    if tuple(dz.shape) != (b, c, t):
        raise AgxError(f"{op}: dz is {tuple(dz.shape)}, expected {(b, c, t)}")
    dz, w = _f32c(dz), _f32c(w)
    du = torch.empty_like(u) if want_du else None
    dw = dbias = ws = None
    nbytes = 0
    if want_params:
        dw, dbias = torch.empty_like(w), torch.empty(c, dtype=torch.float32, device=u.device)
        nbytes = int(getattr(lib, symbol + "_workspace_bytes")(b, c, t, k))
        ws = _workspace(nbytes, u.device, symbol + "_workspace_bytes")
    _lib.check(getattr(lib, symbol)(_ptr(dz), _ptr(u), _ptr(w), _ptr(du), _ptr(dw), _ptr(dbias), _ptr(ws), nbytes, b, c, t, k, _stream()),
               symbol)
    return du, dw, dbias


def glu_dwconv(u: Tensor, w: Tensor, bias: Tensor, bn: Optional[tuple] = None, eps: float = 1e-5) -> Tensor:
    """``z = bias + depthwise_same_conv(u[:, :C] * sigmoid(u[:, C:]), w)``: u (B, 2 C, T) -> (B, C, T), one launch, the GLU
    output never written.  ``bn`` = (gamma, beta, running_mean, running_var): the eval-mode module -- the normalisation on the
    given statistics and SiLU applied in the same launch, ``y`` returned and ``z`` not written."""
    return _glu_dwconv_forward("glu_dwconv", "agx_glu_dwconv_forward", u, w, bias, bn, eps, ())


def glu_dwconv_backward(dz: Tensor, u: Tensor, w: Tensor, want_du: bool = True, want_params: bool = True):
    """(du (B, 2 C, T) or None, dw of w's shape or None, dbias (C) or None) of ``glu_dwconv`` without ``bn``."""
    return _glu_dwconv_backward("glu_dwconv_backward", "agx_glu_dwconv_backward", dz, u, w, want_du, want_params)


CONFORMER_MAX_STEP = _lib.CONFORMER_MAX_STEP


def glu_dwconv_causal(u: Tensor, w: Tensor, bias: Tensor, bn: Optional[tuple] = None, eps: float = 1e-5,
                      hist: Optional[Tensor] = None) -> Tensor:
    """``glu_dwconv`` with the causal conv: an output sees its own frame and the K - 1 before it.  ``hist`` (B, C, K - 1), oldest
    frame first: the post-GLU values of the K - 1 frames before ``u`` (None: zeros, the start of a sequence); read, not written."""
    return _glu_dwconv_forward("glu_dwconv_causal", "agx_glu_dwconv_causal_forward", u, w, bias, bn, eps, (hist,))


def glu_dwconv_causal_backward(dz: Tensor, u: Tensor, w: Tensor, want_du: bool = True, want_params: bool = True):
    """(du (B, 2 C, T) or None, dw of w's shape or None, dbias (C) or None) of ``glu_dwconv_causal`` without ``bn`` and without
    ``hist``: there is no backward through a cached call."""
    return _glu_dwconv_backward("glu_dwconv_causal_backward", "agx_glu_dwconv_causal_backward", dz, u, w, want_du, want_params)


def glu_dwconv_step(u: Tensor, w: Tensor, bias: Tensor, bn: tuple, hist: Optional[Tensor], eps: float = 1e-5,
                    counts: Optional[Tensor] = None) -> Tensor:
    """The streaming step, one launch: ``y`` (B, C, n) of the ``n <= CONFORMER_MAX_STEP`` new frames ``u`` (B, 2 C, n) -- the eval
    form, ``bn`` = (gamma, beta, running_mean, running_var) -- and ``hist`` (B, C, K - 1) rewritten in place with the last K - 1
    post-GLU values of [hist | chunk].  ``hist`` may be None only for K == 1.  ``counts`` (int64 (B,), device): row ``b`` takes
    its first ``c_b = clamp(counts[b], 0, n)`` frames -- ``y`` is exact 0 behind them and the history is that of
    [hist | first c_b frames], untouched where ``c_b == 0``."""
    lib = _lib.load()
    _need_gpu(u, w, bias, hist, *(bn or ()))
    b, c, n, k = _glu_shape("glu_dwconv_step", u, w)
    if not 1 <= n <= CONFORMER_MAX_STEP:
        raise AgxError(f"glu_dwconv_step: n = {n} frames is outside [1, {CONFORMER_MAX_STEP}] (longer chunks: glu_dwconv_causal(hist=) "
                       "+ glu_hist_update)")
    if bn is None or len(bn) != 4 or any(v is None for v in bn):
        raise AgxError("glu_dwconv_step: the step is the eval form: bn = (gamma, beta, running_mean, running_var)")
    if hist is None and k > 1:
        raise AgxError(f"glu_dwconv_step: kernel_size = {k} needs hist (B, C, K - 1)")
    w, (bias,) = _f32c(w), _bn_vectors("glu_dwconv_step", c, bias)
    bn = _bn_vectors("glu_dwconv_step", c, *bn)
    _glu_hist("glu_dwconv_step", hist, b, c, k)
    if counts is not None:
        counts = _checked_counts("glu_dwconv_step", counts, b, u.device)
    out = torch.empty((b, c, n), dtype=torch.float32, device=u.device)
    tok = _observer.begin("other", ("glu_dwconv_step", 12 * out.numel())) if _observer is not None else None
    if counts is not None:
        _lib.check(lib.agx_glu_dwconv_step_counted(_ptr(u), _ptr(w), _ptr(bias), *(_ptr(v) for v in bn), float(eps), _ptr(hist), _ptr(out),
                                                   _ptr(counts), b, c, n, k, _stream()), "agx_glu_dwconv_step_counted")
    else:
        _lib.check(lib.agx_glu_dwconv_step(_ptr(u), _ptr(w), _ptr(bias), *(_ptr(v) for v in bn), float(eps), _ptr(hist), _ptr(out), b, c,
                                           n, k, _stream()), "agx_glu_dwconv_step")
    if tok is not None:
        _observer.end(tok)
    return out


def glu_hist_update(u: Tensor, hist: Tensor) -> Tensor:
    """``hist`` (B, C, K - 1) <- the last K - 1 post-GLU values of [hist | u (B, 2 C, T)], in place, one launch, any T: what
    ``glu_dwconv_step`` does to its state, for cached calls longer than a step.  K == 1: nothing to do.  Returns ``hist``."""
    lib = _lib.load()
    _need_gpu(u, hist)
    if u.dim() != 3 or u.shape[1] % 2 or u.dtype != torch.float32 or not u.is_contiguous():
        raise AgxError(f"glu_hist_update: u must be a contiguous float32 (B, 2 C, T) tensor, got {tuple(u.shape)} {u.dtype}")
    b, c, t = u.shape[0], u.shape[1] // 2, u.shape[2]
    if hist.dim() != 3 or not 1 <= hist.shape[-1] + 1 <= CONFORMER_MAX_K:
        raise AgxError(f"glu_hist_update: hist is {tuple(hist.shape)}, expected (B, C, K - 1) with 1 <= K <= {CONFORMER_MAX_K}")
    k = hist.shape[-1] + 1
    _glu_hist("glu_hist_update", hist, b, c, k)
    _lib.check(lib.agx_glu_hist_update(_ptr(u), _ptr(hist), b, c, t, k, _stream()), "agx_glu_hist_update")
    return hist


def bn_stats(z: Tensor, running_mean: Optional[Tensor] = None, running_var: Optional[Tensor] = None,
             num_batches_tracked: Optional[Tensor] = None, momentum: float = 0.1):
    """(mean, var): the per-channel mean and biased variance of z (B, C, T) over (B, T), by a merge of per-segment (n, mean,
    M2).  The running statistics (unbiased variance) and the int64 counter are updated in place by the finishing launch."""
    lib = _lib.load()
    _need_gpu(z, running_mean, running_var, num_batches_tracked)
    b, c, t = _bct("bn_stats", z)
    if b * t < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(z.shape)}")
    for v in (running_mean, running_var):
        if v is not None and (v.dtype != torch.float32 or not v.is_contiguous() or v.numel() != c):
            raise AgxError(f"bn_stats: a running statistic must be a contiguous float32 tensor of {c} elements")
    if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1):
        raise AgxError("bn_stats: num_batches_tracked must be one int64")
    mean, var = torch.empty(c, dtype=torch.float32, device=z.device), torch.empty(c, dtype=torch.float32, device=z.device)
    nbytes = int(lib.agx_bn_stats_workspace_bytes(b, c, t))
    ws = _workspace(nbytes, z.device, "agx_bn_stats_workspace_bytes")
    _lib.check(lib.agx_bn_stats(_ptr(z), _ptr(mean), _ptr(var), _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked),
                                float(momentum), _ptr(ws), nbytes, b, c, t, _stream()), "agx_bn_stats")
    return mean, var


def bn_silu(z: Tensor, gamma: Tensor, beta: Tensor, mean: Tensor, var: Tensor, eps: float = 1e-5, training: bool = True,
            out: Optional[Tensor] = None) -> Tensor:
    """``silu(a)`` with ``a = (z - mean) rstd gamma + beta`` per channel (``training=False``: ``z scale + shift``, the folded
    form of the fused eval launch, bit for bit).  ``out`` may be ``z``."""
    lib = _lib.load()
    _need_gpu(z, gamma, beta, mean, var, out)
    b, c, t = _bct("bn_silu", z)
    gamma, beta, mean, var = _bn_vectors("bn_silu", c, gamma, beta, mean, var)
    return _elementwise("bn_silu", lib, "agx_bn_silu_forward", z, out, 8,
                        lambda out: (_ptr(z), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(var), float(eps), int(bool(training)), _ptr(out), b, c, t))


def bn_silu_backward(dy: Tensor, z: Tensor, gamma: Tensor, beta: Tensor, mean: Tensor, var: Tensor, eps: float = 1e-5,
                     training: bool = True, want_dz: bool = True, want_params: bool = True, out: Optional[Tensor] = None):
    """(dz or None, dgamma or None, dbeta or None) of ``bn_silu`` -- in training mode through the batch statistics as well.
    ``out`` (for dz) may be ``dy``."""
    lib = _lib.load()
    _need_gpu(dy, z, gamma, beta, mean, var, out)
    b, c, t = _bct("bn_silu_backward", z, dy)
    gamma, beta, mean, var = _bn_vectors("bn_silu_backward", c, gamma, beta, mean, var)
    dz = _same_out("bn_silu_backward", z, out) if want_dz else None
    dgamma = torch.empty(c, dtype=torch.float32, device=z.device) if want_params else None
    dbeta = torch.empty(c, dtype=torch.float32, device=z.device) if want_params else None
    if not want_dz and not want_params:
        return None, None, None
    nbytes = int(lib.agx_bn_silu_backward_workspace_bytes(b, c, t))
    ws = _workspace(nbytes, z.device, "agx_bn_silu_backward_workspace_bytes")
    _lib.check(lib.agx_bn_silu_backward(_ptr(dy), _ptr(z), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(var), float(eps),
                                        int(bool(training)), _ptr(dz), _ptr(dgamma), _ptr(dbeta), _ptr(ws), nbytes, b, c, t,
                                        _stream()), "agx_bn_silu_backward")
    return dz, dgamma, dbeta


def silu(x: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """``x * sigmoid(x)`` elementwise; ``out`` may be ``x`` (in place)."""
    lib = _lib.load()
    _need_gpu(x, out)
    return _elementwise("silu", lib, "agx_silu", x, out, 8, lambda out: (_ptr(x), _ptr(out), x.numel()))


def silu_backward(x: Tensor, dout: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """``dout * silu'(x)`` elementwise; ``out`` may be ``dout`` (in place)."""
    lib = _lib.load()
    _need_gpu(x, dout, out)
    if x.dtype != torch.float32 or not x.is_contiguous() or dout.shape != x.shape or dout.dtype != torch.float32 or not dout.is_contiguous():
        raise AgxError(f"silu_backward: x and dout must be contiguous float32 tensors of one shape (x {tuple(x.shape)}, dout {tuple(dout.shape)})")
    return _elementwise("silu_backward", lib, "agx_silu_backward", x, out, None, lambda out: (_ptr(x), _ptr(dout), _ptr(out), x.numel()))


# ------------------------------------------------------------------ streaming conv stacks (include/agx.h "Streaming conv stacks")
STREAM_LIVE = _lib.STREAM_LIVE


def conv_stream_pack(desc: ConvDesc, v: Tensor, g: Optional[Tensor] = None) -> Tensor:
    """The image ``conv_stream_step`` reads: the standard fp32 image of ``conv_pack`` whatever arithmetic the layer's plain call
    uses (a name of its own, so that ``units.packed_image`` keeps it beside the plain call's image)."""
    if desc.impl != IMPL_AUTO or desc.groups != 1:
        raise AgxError("conv_stream_pack: the streaming step reads the dense fp32 image (impl = IMPL_AUTO, groups = 1)")
    return conv_pack(desc, v, g)


def conv_stream_kernel_name(kind: int, c_in: int, c_out: int, kernel: int, stride: int, dilation: int, n: int, rate_in: int) -> str:
    """The kernel ``conv_stream_step`` runs for this layer and step (host-only); ``AgxError`` with the launcher's refusal."""
    return _kernel_name("agx_conv_stream_kernel_name", kind, c_in, c_out, kernel, stride, dilation, n, rate_in)


def _stream_rates(kind: int, stride: int, rate_in: int, delay_in: int) -> Tuple[int, int]:
    """(rate_out, delay_out) of a layer (include/agx.h); the library refuses what does not divide."""
    if kind == CONV_UPSAMPLE:
        return rate_in * stride, delay_in * stride + stride
    if kind == CONV_CAUSAL:
        return rate_in // stride, delay_in // stride
    return rate_in, delay_in


def conv_stream_step(kind: int, c_in: int, c_out: int, kernel: int, stride: int, dilation: int, packed: Tensor, bias: Optional[Tensor],
                     src: Tensor, dst: Tensor, pos: Tensor, n: int, rate_in: int, delay_in: int, src_ring: bool = True,
                     dst_ring: bool = True, res: Optional[Tensor] = None, end: Optional[Tensor] = None, epilogue: int = 0,
                     slope: float = 0.1, counts: Optional[Tensor] = None) -> Tensor:
    """One chunk of ``n`` frames through one conv layer of a stream (``agx_conv_stream_step``).  ``src``: the layer's input ring
    (B, c_in, cap), or with ``src_ring=False`` a plain (B, c_in, n * rate_in) tensor of the step's own columns (kernel 1 only);
    ``dst``: the consumer's ring (B, c_out, cap') or, ``dst_ring=False``, a plain (B, c_out, n * rate_out) tensor; ``res``: the
    ring the residual is read from, at the output's columns; ``pos`` / ``end``: int64 (B,) device tensors, read by the kernel
    and never written (``end=None``: no validity mask).  Writes the step's n * rate_out columns of ``dst`` and returns it.
    Every refusal -- this wrapper's or the library's -- precedes the launch.

    ``counts`` (int64 (B,), device; ``agx_conv_stream_step_counted``): row ``b`` takes the first ``c_b = clamp(counts[b], 0, n)``
    frames.  Its first ``c_b * rate_out`` output columns are bit for bit those of the uncounted step on these frames; behind them
    a plain ``dst`` holds exact 0 and a ring ``dst`` is not written.  The kernel reads ``counts``; the host never does."""
    return _conv_stream_step(kind, c_in, c_out, kernel, stride, dilation, packed, bias, src, dst, pos, n, rate_in, delay_in, src_ring,
                             dst_ring, res, end, epilogue, slope, counts, None)


def conv_stream_step_affine(c_in: int, c_out: int, kernel: int, dilation: int, packed: Tensor, bias: Optional[Tensor], scale: Tensor,
                            shift: Tensor, src: Tensor, dst: Tensor, pos: Tensor, n: int, rate_in: int, delay_in: int,
                            dst_ring: bool = True, end: Optional[Tensor] = None, epilogue: int = 0, slope: float = 0.1,
                            counts: Optional[Tensor] = None, kind: int = CONV_CAUSAL, stride: int = 1, src_ring: bool = True) -> Tensor:
    """``conv_stream_step`` of a stride-1 causal conv with a per-channel affine in its operand fetch
    (``agx_conv_stream_step_affine``): ``scale`` / ``shift`` are two fp32 (c_in,) vectors, the folded weight and the
    bias of the grouped k = 1 conv in front of a depthwise residual block's dilated conv.  The operand of channel ``c`` at stream
    column ``i`` is ``fmaf(scale[c], x[c, i], shift[c])`` for ``i >= 0`` and exact 0 before the start of the stream: the causal
    zero padding lies behind the affine.  ``kind`` / ``stride`` / ``src_ring`` are there to be refused: the policy is that of a
    stride-1 causal conv reading a ring.  Everything else as in ``conv_stream_step``; every refusal precedes the launch."""
    return _conv_stream_step(kind, c_in, c_out, kernel, stride, dilation, packed, bias, src, dst, pos, n, rate_in, delay_in, src_ring,
                             dst_ring, None, end, epilogue, slope, counts, (scale, shift))


def _conv_stream_step(kind, c_in, c_out, kernel, stride, dilation, packed, bias, src, dst, pos, n, rate_in, delay_in, src_ring, dst_ring,
                      res, end, epilogue, slope, counts, affine) -> Tensor:
    """The one body of ``conv_stream_step`` (``affine=None``) and ``conv_stream_step_affine`` (``affine=(scale, shift)``)."""
    n, rate_in, delay_in = int(n), int(rate_in), int(delay_in)
    if affine is not None:      # shape refusals of the affine form first: they need no device
        if kind != CONV_CAUSAL or int(stride) != 1 or not src_ring:
            raise AgxError("conv_stream_step_affine: the affine is the operand of a stride-1 causal conv reading a ring "
                           f"(kind={kind} stride={stride} src_ring={src_ring})")
        if any(not isinstance(t, Tensor) or t.dtype != torch.float32 or t.dim() != 1 or t.numel() != int(c_in)
                                   or not t.is_contiguous() for t in affine):
            raise AgxError(f"conv_stream_step_affine: scale and shift are two contiguous float32 ({c_in},) vectors")
    lib = _lib.load()
    _need_gpu(packed, bias, src, dst, res, *(affine or ()))
    if n < 1:
        raise AgxError(f"conv_stream_step: a step takes n >= 1 frames, got {n}")
    for name, t in (("src", src), ("dst", dst), ("res", res)):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 3 or not t.is_contiguous()):
            raise AgxError(f"conv_stream_step: {name} must be a contiguous float32 (B, C, columns) tensor")
    b = src.shape[0]
    rate_out, _ = _stream_rates(kind, stride, rate_in, delay_in)
    if src.shape[1] != c_in or (not src_ring and src.shape[2] != n * rate_in):
        raise AgxError(f"conv_stream_step: src is {tuple(src.shape)} for c_in={c_in}"
                       + ("" if src_ring else f" and {n * rate_in} plain columns"))
    if tuple(dst.shape[:2]) != (b, c_out) or (not dst_ring and dst.shape[2] != n * rate_out):
        raise AgxError(f"conv_stream_step: dst is {tuple(dst.shape)} for batch {b}, c_out={c_out}"
                       + ("" if dst_ring else f" and {n * rate_out} plain columns"))
    if bool(epilogue & EPI_RESIDUAL) != (res is not None):
        raise AgxError("conv_stream_step: EPI_RESIDUAL and the residual ring go together")
    if res is not None and tuple(res.shape[:2]) != (b, c_out):
        raise AgxError(f"conv_stream_step: the residual ring is {tuple(res.shape)} for batch {b}, c_out={c_out}")
    if any(t is not None and t.device != src.device for t in (packed, bias, dst, res, *(affine or ()))):
        raise AgxError("conv_stream_step: operands on different devices")
    pos = _checked_pos("conv_stream_step", pos, b, src.device)
    if end is not None:
        end = _checked_pos("conv_stream_step", end, b, src.device)
    if counts is not None:
        counts = _checked_counts("conv_stream_step", counts, b, src.device)
    packed = _f32c(packed)
    need = _lib.load().agx_conv_packed_floats(ctypes.byref(conv_desc(kind, 1, c_in, c_out, 1 << 20, kernel, stride, dilation)))
    if need < 0:
        _lib.check(int(need), "agx_conv_packed_floats")
    if packed.numel() != need:
        raise AgxError(f"conv_stream_step: the packed image has {packed.numel()} floats, the layer's has {need}")
    if bias is not None:
        bias = _f32c(bias)
        if bias.numel() != c_out:
            raise AgxError(f"conv_stream_step: bias has {bias.numel()} entries for c_out={c_out}")
    tok = None
    if _observer is not None:
        tok = _observer.begin("other", ("conv_stream_step", 4 * (packed.numel() + b * c_out * n * rate_out), 0))
    head = (kind, c_in, c_out, kernel, stride, dilation, int(epilogue), float(slope), _ptr(packed), _ptr(bias),
            *(() if affine is None else (_ptr(affine[0]), _ptr(affine[1]))), _ptr(src),
            src.shape[2] if src_ring else 0, _ptr(res), res.shape[2] if res is not None else 0, _ptr(dst),
            dst.shape[2] if dst_ring else 0, _ptr(pos), _ptr(end))
    if affine is not None and counts is not None:
        _lib.check(lib.agx_conv_stream_step_affine_counted(*head, _ptr(counts), b, n, rate_in, delay_in, _stream()),
                   "agx_conv_stream_step_affine_counted")
    elif affine is not None:
        _lib.check(lib.agx_conv_stream_step_affine(*head, b, n, rate_in, delay_in, _stream()), "agx_conv_stream_step_affine")
    elif counts is not None:
        _lib.check(lib.agx_conv_stream_step_counted(*head, _ptr(counts), b, n, rate_in, delay_in, _stream()),
                   "agx_conv_stream_step_counted")
    else:
        _lib.check(lib.agx_conv_stream_step(*head, b, n, rate_in, delay_in, _stream()), "agx_conv_stream_step")
    if tok is not None:
        _observer.end(tok)
    return dst


MULTIRES_STREAM_TILE = 1024          # AGX_MULTIRES_STREAM_TILE
MULTIRES_STREAM_LDS_BYTES = 65536    # AGX_MULTIRES_STREAM_LDS_BYTES


def multires_stream_reach(kernel: int, depth: int) -> int:
    """Input columns the cascade reads before an output's own: ``(K - 1)(2^depth - 1)``."""
    return (int(kernel) - 1) * ((1 << int(depth)) - 1)


def multires_stream_fits(kernel: int, depth: int, cols: int) -> bool:
    """Whether ``multires_stream_step`` holds a step of ``cols`` columns: the two LDS rows of reach + tile floats and the taps of
    one channel row within ``MULTIRES_STREAM_LDS_BYTES`` (the library's own refusal, host-only)."""
    if int(depth) < 0 or int(depth) > 20 or int(kernel) < 1:
        return False
    tile = min(int(cols), MULTIRES_STREAM_TILE)
    return 4 * (2 * (multires_stream_reach(kernel, depth) + tile) + 2 * int(kernel)) <= MULTIRES_STREAM_LDS_BYTES


def multires_stream_step(h0: Tensor, h1: Tensor, w: Tensor, depth: int, src: Tensor, dst: Tensor, pos: Tensor, n: int, rate: int,
                         delay: int, dst_ring: bool = True, end: Optional[Tensor] = None, counts: Optional[Tensor] = None) -> Tensor:
    """One chunk of ``n`` frames through a ``CausalMultiresConv1d`` of a stream (``agx_multires_stream_step``), one
    launch: from the layer's input ring ``src`` (B, C, cap >= (K - 1)(2^depth - 1) + n rate) to the n rate columns
    [pos rate - delay, (pos + n) rate - delay) of ``dst`` -- the consumer's ring (B, C, cap' >= n rate) or, ``dst_ring=False``, a
    plain (B, C, n rate) tensor --, each the cascade and GELU of ``multires_forward``, exact 0 where the index is negative or at
    and behind ``end[b] rate`` (``end=None``: no mask).  ``h0`` / ``h1`` (C, 1, K) and ``w`` (C, depth + 2): the layer's parameters.
    ``counts``: the counted form -- behind a row's count a plain ``dst`` holds exact 0, a ring is not written and no source column
    is read.  Every refusal precedes the launch.  Returns ``dst``."""
    op = "multires_stream_step"
    depth, n, rate, delay = int(depth), int(n), int(rate), int(delay)
    if n < 1:
        raise AgxError(f"{op}: a step takes n >= 1 frames, got {n}")
    if rate < 1 or delay < 0:
        raise AgxError(f"{op}: rate = {rate} / delay = {delay}")
    for name, t in (("src", src), ("dst", dst)):
        if not isinstance(t, Tensor) or t.dtype != torch.float32 or t.dim() != 3 or not t.is_contiguous():
            raise AgxError(f"{op}: {name} must be a contiguous float32 (B, C, columns) tensor")
    b, c, cap = src.shape
    k = h0.shape[-1]
    if depth < 0 or tuple(h0.shape) != (c, 1, k) or tuple(h1.shape) != (c, 1, k) or tuple(w.shape) != (c, depth + 2):
        raise AgxError(f"{op}: parameter shapes do not match (C,1,K) / (C,depth+2) for C={c}, depth={depth}")
    if any(t.dtype != torch.float32 or not t.is_contiguous() for t in (h0, h1, w)):
        raise AgxError(f"{op}: h0, h1 and w must be contiguous float32 tensors")
    reach, cols = multires_stream_reach(k, depth), n * rate
    if not multires_stream_fits(k, depth, cols):
        raise AgxError(f"{op}: reach {reach} + a tile of {min(cols, MULTIRES_STREAM_TILE)} columns does not fit "
                       f"{MULTIRES_STREAM_LDS_BYTES} bytes of LDS")
    if cap < reach + cols:
        raise AgxError(f"{op}: src is {tuple(src.shape)} for a ring of at least {reach + cols} columns (the step's writes would alias "
                       "its history)")
    if tuple(dst.shape[:2]) != (b, c) or (dst.shape[2] < cols if dst_ring else dst.shape[2] != cols):
        raise AgxError(f"{op}: dst is {tuple(dst.shape)} for batch {b}, C={c} and {cols} "
                       + ("new columns of a ring" if dst_ring else "plain columns"))
    if dst.data_ptr() == src.data_ptr():
        raise AgxError(f"{op}: the destination is the source")
    lib = _lib.load()
    _need_gpu(h0, h1, w, src, dst)
    if any(t.device != src.device for t in (h0, h1, w, dst)):
        raise AgxError(f"{op}: operands on different devices")
    pos = _checked_pos(op, pos, b, src.device)
    if end is not None:
        end = _checked_pos(op, end, b, src.device)
    if counts is not None:
        counts = _checked_counts(op, counts, b, src.device)
    tok = None
    if _observer is not None:
        tok = _observer.begin("other", (op, 4 * b * c * (reach + 2 * cols), 0))
    head = (_ptr(h0), _ptr(h1), _ptr(w), _ptr(src), cap, _ptr(dst), dst.shape[2] if dst_ring else 0, _ptr(pos), _ptr(end))
    if counts is not None:
        _lib.check(lib.agx_multires_stream_step_counted(*head, _ptr(counts), b, c, n, k, depth, rate, delay, _stream()),
                   "agx_multires_stream_step_counted")
    else:
        _lib.check(lib.agx_multires_stream_step(*head, b, c, n, k, depth, rate, delay, _stream()), "agx_multires_stream_step")
    if tok is not None:
        _observer.end(tok)
    return dst


def ring_write_rate(buf: Tensor, src: Tensor, pos: Tensor, rate: int, counts: Optional[Tensor] = None) -> None:
    """``buf[b, :, (pos[b] * rate + t) mod cap] = src[b, :, t]`` for src (B, C, n * rate) and the ring buf (B, C, cap): a stack's
    input chunk into its first ring, every row at its own position, one launch.  ``pos`` is not written.  ``counts`` (int64
    (B,), device): only the ``clamp(counts[b], 0, n) * rate`` first columns of row ``b``; the others are neither read nor written."""
    lib = _lib.load()
    _need_gpu(buf, src)
    if any(t.dtype != torch.float32 or t.dim() != 3 or not t.is_contiguous() for t in (buf, src)):
        raise AgxError("ring_write_rate: buf (B, C, cap) and src (B, C, columns) must be contiguous float32 tensors")
    b, c, cols = src.shape
    if tuple(buf.shape[:2]) != (b, c) or src.device != buf.device:
        raise AgxError(f"ring_write_rate: src {tuple(src.shape)} does not match buf {tuple(buf.shape)}")
    if int(rate) < 1 or cols % int(rate):
        raise AgxError(f"ring_write_rate: {cols} columns are not whole frames of {rate}")
    pos = _checked_pos("ring_write_rate", pos, b, buf.device)
    if counts is not None:
        counts = _checked_counts("ring_write_rate", counts, b, buf.device)
        _lib.check(lib.agx_ring_write_rate_counted(_ptr(buf), _ptr(src), _ptr(pos), _ptr(counts), b, c, cols, buf.shape[2], int(rate),
                                                   _stream()), "agx_ring_write_rate_counted")
        return
    _lib.check(lib.agx_ring_write_rate(_ptr(buf), _ptr(src), _ptr(pos), b, c, cols, buf.shape[2], int(rate), _stream()),
               "agx_ring_write_rate")


def stream_mark_end(pos: Tensor, end: Tensor, rows: Optional[Tensor] = None) -> None:
    """``end[r] = pos[r]`` on the device for the row numbers in ``rows`` (an int64 device tensor; default every row)."""
    lib = _lib.load()
    if not isinstance(pos, Tensor) or not isinstance(end, Tensor):
        raise AgxError("stream_mark_end: pos and end must be contiguous int64 device tensors")
    pos = _checked_pos("stream_mark_end", pos, pos.numel(), pos.device)
    end = _checked_pos("stream_mark_end", end, pos.numel(), pos.device)
    if rows is not None:
        rows = _checked_pos("stream_mark_end", rows, rows.numel() if isinstance(rows, Tensor) else 0, pos.device)
    _lib.check(lib.agx_stream_mark_end(_ptr(pos), _ptr(end), _ptr(rows), 0 if rows is None else rows.numel(), pos.numel(), _stream()),
               "agx_stream_mark_end")


# ------------------------------------------------------------------ streaming wavelet blocks (include/agx.h "Streaming wavelet blocks")
def wavelet_fold_table(space: Tensor, sigma: Tensor, channels: int, scale: int) -> Tensor:
    """The per-channel table the wavelet out-step reads (``agx_wavelet_fold_table``): (channels, 3 scale - 1) fp32 =
    [S_hi[0 .. s) | S_lo[0 .. s) | the s - 1 tail taps], formed by the code of ``wavelet_fold``.  ``sigma``: 1 or ``channels``
    entries.  One small launch."""
    channels, scale = int(channels), int(scale)
    p = space.numel()
    if scale < 2 or p % scale:
        raise AgxError(f"wavelet_fold_table: scale = {scale} must be >= 2 and divide n_points = {p}")
    if sigma.numel() not in (1, channels):
        raise AgxError(f"wavelet_fold_table: sigma has {sigma.numel()} entries for {channels} channels (1 or {channels})")
    lib = _lib.load()
    _need_gpu(space, sigma)
    space, sigma = _f32c(space.reshape(-1)), _f32c(sigma.reshape(-1))
    table = torch.empty((channels, 3 * scale - 1), dtype=torch.float32, device=space.device)
    _lib.check(lib.agx_wavelet_fold_table(_ptr(space), _ptr(sigma), sigma.numel(), _ptr(table), channels, p, scale, _stream()),
               "agx_wavelet_fold_table")
    return table


def wavelet_stream_in_kernel_name(c_in: int, hidden: int, kernel: int, n: int, rate_in: int) -> str:
    """The kernel ``wavelet_stream_in_step`` runs for this layer and step (host-only); ``AgxError`` with the launcher's refusal."""
    return _kernel_name("agx_wavelet_stream_in_kernel_name", c_in, hidden, kernel, n, rate_in)


def wavelet_stream_out_kernel_name(hidden: int, c_out: int, kernel: int, scale: int, n: int, rate_h: int) -> str:
    """The kernel ``wavelet_stream_out_step`` runs for this layer and step (host-only); ``AgxError`` with the launcher's refusal."""
    return _kernel_name("agx_wavelet_stream_out_kernel_name", hidden, c_out, kernel, scale, n, rate_h)


def _wavelet_step_operands(op: str, kind_desc, packed: Tensor, bias: Optional[Tensor], src: Tensor, dst: Tensor, pos, end, counts,
                           c_in: int, c_out: int, n: int, src_need: int, dst_cols: int, dst_ring: bool, src_name: str):
    """The checks the two wavelet steps share, in ``conv_stream_step``'s words; shapes first, so that every refusal precedes the
    first use of the device.  Returns (b, packed, bias, pos, end, counts)."""
    if n < 1:
        raise AgxError(f"{op}: a step takes n >= 1 frames, got {n}")
    for name, t in ((src_name, src), ("dst", dst)):
        if not isinstance(t, Tensor) or t.dtype != torch.float32 or t.dim() != 3 or not t.is_contiguous():
            raise AgxError(f"{op}: {name} must be a contiguous float32 (B, C, columns) tensor")
    b = src.shape[0]
    if src.shape[1] != c_in or src.shape[2] < src_need:
        raise AgxError(f"{op}: {src_name} is {tuple(src.shape)} for {c_in} channels and a ring of at least {src_need} columns "
                       "(the step's writes would alias its history)")
    if tuple(dst.shape[:2]) != (b, c_out) or (dst.shape[2] < dst_cols if dst_ring else dst.shape[2] != dst_cols):
        raise AgxError(f"{op}: dst is {tuple(dst.shape)} for batch {b}, c_out={c_out} and {dst_cols} "
                       + ("new columns of a ring" if dst_ring else "plain columns"))
    if dst.data_ptr() == src.data_ptr():
        raise AgxError(f"{op}: the destination is one of the sources")
    if end is None:
        raise AgxError(f"{op}: end is needed (the block's zero padding and its raw tail are decided by the stream's end)")
    lib = _lib.load()
    _need_gpu(packed, bias, src, dst)
    if any(t is not None and t.device != src.device for t in (packed, bias, dst)):
        raise AgxError(f"{op}: operands on different devices")
    pos = _checked_pos(op, pos, b, src.device)
    end = _checked_pos(op, end, b, src.device)
    if counts is not None:
        counts = _checked_counts(op, counts, b, src.device)
    packed = _f32c(packed)
    need = lib.agx_conv_packed_floats(ctypes.byref(kind_desc))
    if need < 0:
        _lib.check(int(need), "agx_conv_packed_floats")
    if packed.numel() != need:
        raise AgxError(f"{op}: the packed image has {packed.numel()} floats, the layer's has {need}")
    if bias is not None:
        bias = _f32c(bias)
        if bias.numel() != c_out:
            raise AgxError(f"{op}: bias has {bias.numel()} entries for c_out={c_out}")
    return b, packed, bias, pos, end, counts


def wavelet_stream_in_step(c_in: int, hidden: int, kernel: int, packed: Tensor, bias: Optional[Tensor], src: Tensor, dst: Tensor,
                           pos: Tensor, end: Tensor, n: int, rate_in: int, delay_in: int, counts: Optional[Tensor] = None) -> Tensor:
    """conv_in of a wavelet block as a stream's step (``agx_wavelet_stream_in_step``): the "same" conv of ``kernel`` (odd) taps
    from the block's input ring ``src`` (B, c_in, cap >= kernel - 1 + n rate_in) into the ring of the hidden activation ``dst``
    (B, hidden, cap' >= n rate_in): the n rate_in columns [pos rate_in - D_h, ...), D_h = delay_in + (kernel - 1) / 2, exact 0
    outside [0, end rate_in).  ``packed``: the ``conv_stream_pack`` image of the layer for ``CONV_SAME``.  ``counts``: the counted
    form -- the ring is not written past a row's count.  Returns ``dst``."""
    op = "wavelet_stream_in_step"
    c_in, hidden, kernel, n, rate_in, delay_in = int(c_in), int(hidden), int(kernel), int(n), int(rate_in), int(delay_in)
    if kernel < 1 or kernel % 2 == 0:
        raise AgxError(f"{op}: a \"same\" conv streams with an odd kernel, got {kernel}")
    if rate_in < 1 or delay_in < 0:
        raise AgxError(f"{op}: rate_in = {rate_in} / delay_in = {delay_in}")
    desc = conv_desc(CONV_SAME, 1, c_in, hidden, 1 << 20, kernel, 1, 1)
    b, packed, bias, pos, end, counts = _wavelet_step_operands(op, desc, packed, bias, src, dst, pos, end, counts, c_in, hidden, n,
                                                               kernel - 1 + n * rate_in, n * rate_in, True, "src")
    lib = _lib.load()
    tok = None
    if _observer is not None:
        tok = _observer.begin("other", (op, 4 * (packed.numel() + b * hidden * n * rate_in), 0))
    head = (c_in, hidden, kernel, _ptr(packed), _ptr(bias), _ptr(src), src.shape[2], _ptr(dst), dst.shape[2], _ptr(pos), _ptr(end))
    if counts is not None:
        _lib.check(lib.agx_wavelet_stream_in_step_counted(*head, _ptr(counts), b, n, rate_in, delay_in, _stream()),
                   "agx_wavelet_stream_in_step_counted")
    else:
        _lib.check(lib.agx_wavelet_stream_in_step(*head, b, n, rate_in, delay_in, _stream()), "agx_wavelet_stream_in_step")
    if tok is not None:
        _observer.end(tok)
    return dst


def wavelet_stream_out_step(hidden: int, c_out: int, kernel: int, scale: int, packed: Tensor, bias: Optional[Tensor], table: Tensor,
                            h: Tensor, dst: Tensor, pos: Tensor, end: Tensor, n: int, rate_h: int, delay_h: int, dst_ring: bool = True,
                            epilogue: int = 0, slope: float = 0.1, counts: Optional[Tensor] = None) -> Tensor:
    """conv_out of a wavelet block with the fold fused into its operand fetch (``agx_wavelet_stream_out_step``): from the ring
    ``h`` (B, hidden, cap >= 1 + ceil((kernel - 1) / scale) + n rate_h) of the in-step (``rate_h`` columns per frame, delay
    ``delay_h``) and ``table`` (``wavelet_fold_table``) to the n rate_h scale columns [pos rate_h scale - D_out, ...), D_out =
    delay_h scale + scale + (kernel - 1) / 2, exact 0 outside [0, end rate_h scale).  ``dst``: the consumer's ring or,
    ``dst_ring=False``, a plain (B, c_out, n rate_h scale) tensor.  ``epilogue``: 0 or ``EPI_LEAKY_PRE``.  ``counts``: the counted
    form.  Returns ``dst``."""
    op = "wavelet_stream_out_step"
    hidden, c_out, kernel, scale, n, rate_h, delay_h = int(hidden), int(c_out), int(kernel), int(scale), int(n), int(rate_h), int(delay_h)
    if kernel < 1 or kernel % 2 == 0:
        raise AgxError(f"{op}: a \"same\" conv streams with an odd kernel, got {kernel}")
    if scale < 2:
        raise AgxError(f"{op}: scale = {scale} < 2")
    if rate_h < 1 or delay_h < 0:
        raise AgxError(f"{op}: rate_h = {rate_h} / delay_h = {delay_h}")
    if int(epilogue) & ~EPI_LEAKY_PRE:
        raise AgxError(f"{op}: epilogue {epilogue} (bias and EPI_LEAKY_PRE are fused)")
    if not isinstance(table, Tensor) or table.dtype != torch.float32 or tuple(table.shape) != (hidden, 3 * scale - 1) \
            or not table.is_contiguous():
        raise AgxError(f"{op}: table must be a contiguous float32 ({hidden}, {3 * scale - 1}) tensor (wavelet_fold_table)")
    desc = conv_desc(CONV_SAME, 1, hidden, c_out, 1 << 20, kernel, 1, 1)
    reach = 1 + -((1 - kernel) // scale)
    b, packed, bias, pos, end, counts = _wavelet_step_operands(op, desc, packed, bias, h, dst, pos, end, counts, hidden, c_out, n,
                                                               reach + n * rate_h, n * rate_h * scale, dst_ring, "h")
    _need_gpu(table)
    if table.device != h.device:
        raise AgxError(f"{op}: operands on different devices")
    lib = _lib.load()
    tok = None
    if _observer is not None:
        tok = _observer.begin("other", (op, 4 * (packed.numel() + b * c_out * n * rate_h * scale), 0))
    head = (hidden, c_out, kernel, scale, int(epilogue), float(slope), _ptr(packed), _ptr(bias), _ptr(table), _ptr(h), h.shape[2],
            _ptr(dst), dst.shape[2] if dst_ring else 0, _ptr(pos), _ptr(end))
    if counts is not None:
        _lib.check(lib.agx_wavelet_stream_out_step_counted(*head, _ptr(counts), b, n, rate_h, delay_h, _stream()),
                   "agx_wavelet_stream_out_step_counted")
    else:
        _lib.check(lib.agx_wavelet_stream_out_step(*head, b, n, rate_h, delay_h, _stream()), "agx_wavelet_stream_out_step")
    if tok is not None:
        _observer.end(tok)
    return dst


# --------------------------------------------------------------------------- code prior
CODES_SAMPLE_MAX_K = _lib.CODES_SAMPLE_MAX_K


def _checked_operand(op: str, what: str, t, dtype, shape: tuple, device=None) -> Tensor:
    """An operand of the code-prior and entropy ops as the kernels read it: a contiguous tensor of ``dtype`` and ``shape`` (an entry of
    ``shape`` that is None is free), on ``device`` when one is given."""
    if not isinstance(t, Tensor) or t.dtype != dtype or t.dim() != len(shape) or \
            any(want is not None and have != want for have, want in zip(t.shape, shape)):
        have = f"{tuple(t.shape)} {t.dtype}" if isinstance(t, Tensor) else type(t).__name__
        raise AgxError(f"{op}: {what} must be a {dtype} tensor of shape {tuple('*' if s is None else s for s in shape)}, got {have}")
    if not t.is_contiguous():
        raise AgxError(f"{op}: {what} is not contiguous (stride {tuple(t.stride())})")
    if device is not None and t.device != device:
        raise AgxError(f"{op}: {what} is on '{t.device}', the operands are on '{device}'")
    return t


def codes_embed(index: Tensor, tables: Tensor, counts: Optional[Tensor] = None) -> Tensor:
    """Gather-sum of one table row per stage (``agx_codes_embed``, one launch): index (B, n, Q) int64, tables (Q, R, D) fp32 ->
    (B, D, n) fp32, channel-major, ``out[b, :, i] = ((0 + tables[0][index[b,i,0]]) + tables[1][index[b,i,1]]) + ...`` in stage
    order.  An index outside [0, R) -- ``-1`` above all -- contributes nothing; ``counts`` (int64 (B,), device): the columns at or
    behind ``clamp(counts[b], 0, n)`` are exact 0."""
    op = "codes_embed"
    _need_gpu(index, tables, counts)
    tables = _checked_operand(op, "tables", tables, torch.float32, (None, None, None))
    n_q, r, d = tables.shape
    index = _checked_operand(op, "index", index, torch.int64, (None, None, n_q), tables.device)
    b, n, _ = index.shape
    _stage_sizes(op, None, n_q, r)
    if b < 1 or n < 1 or r < 1 or d < 1:
        raise AgxError(f"{op}: empty operands: index {tuple(index.shape)}, tables {tuple(tables.shape)}")
    counts, _ = _checked_rows(op, b, tables.device, counts)
    out = torch.empty((b, d, n), dtype=torch.float32, device=tables.device)
    tok = _observer.begin("other", (op, 4 * (b * n * n_q * d + b * d * n) + 8 * b * n * n_q, 0)) if _observer is not None else None
    _lib.check(_lib.load().agx_codes_embed(_ptr(tables), _ptr(index), _ptr(counts), _ptr(out), b, n, n_q, r, d, _stream()),
               "agx_codes_embed")
    if tok is not None:
        _observer.end(tok)
    return out


def codes_embed_backward(dout: Tensor, index: Tensor, rows: int, counts: Optional[Tensor] = None) -> Tensor:
    """Backward of ``codes_embed`` for the tables (``agx_codes_embed_backward``): dout (B, D, n) fp32, index (B, n, Q) -> dtables
    (Q, rows, D), ``dtables[q][r]`` the sum of ``dout[b, :, i]`` over the frames with ``index[b,i,q] == r`` below the row's count,
    taken in frame order on one chain per element: no atomics, two calls agree bit for bit, exact 0 for a row nobody chose."""
    op = "codes_embed_backward"
    _need_gpu(dout, index, counts)
    dout = _checked_operand(op, "dout", dout, torch.float32, (None, None, None))
    b, d, n = dout.shape
    index = _checked_operand(op, "index", index, torch.int64, (b, n, None), dout.device)
    n_q, rows = index.shape[2], int(rows)
    _stage_sizes(op, None, n_q, rows)
    if b < 1 or n < 1 or n_q < 1 or rows < 1 or d < 1:
        raise AgxError(f"{op}: empty operands: dout {tuple(dout.shape)}, index {tuple(index.shape)}, rows = {rows}")
    counts, _ = _checked_rows(op, b, dout.device, counts)
    lib = _lib.load()
    dtables = torch.empty((n_q, rows, d), dtype=torch.float32, device=dout.device)
    nbytes = int(lib.agx_codes_embed_backward_workspace_bytes(b, n, n_q, d))
    ws = _workspace(nbytes, dout.device, "agx_codes_embed_backward_workspace_bytes")
    _lib.check(lib.agx_codes_embed_backward(_ptr(dout), _ptr(index), _ptr(counts), _ptr(dtables), b, n, n_q, rows, d, _ptr(ws), nbytes,
                                            _stream()), "agx_codes_embed_backward")
    return dtables


def _ce_operands(op: str, logits: Tensor, target: Tensor, sizes):
    logits = _checked_operand(op, "logits", logits, torch.float32, (None, None, None))
    b, c, t = logits.shape
    target = _checked_operand(op, "target", target, torch.int64, (b, t, None), logits.device)
    n_q = target.shape[2]
    if b < 1 or t < 1 or n_q < 1 or c < 1 or c % n_q:
        raise AgxError(f"{op}: logits {tuple(logits.shape)} are not (B, Q K, T) for target {tuple(target.shape)} = (B, T, Q)")
    k = c // n_q
    return logits, target, b, t, n_q, k, _stage_sizes(op, sizes, n_q, k)


def codes_cross_entropy(logits: Tensor, target: Tensor, sizes: Optional[Sequence[int]] = None):
    """Cross-entropy of a code prior (``agx_codes_cross_entropy``): logits (B, Q K, T) fp32 -- channel ``q K + k``, the head conv's
    output as it stands --, target (B, T, Q) int64, ``sizes[q] <= K`` the codes of stage q -> (loss 0-d fp32, nll (B, T, Q), lse
    (B, T, Q), n_live 0-d int64).  Entry (b, t, q) is live when ``0 <= target < sizes[q]``; ``lse`` runs over ``k < sizes[q]``;
    ``nll = lse - logit[target]``, exact 0 where dead; ``loss = sum(nll) / n_live`` with the count taken on the device, 0 when
    nothing is live.  The sum runs in a fixed order: two calls agree bit for bit."""
    op = "codes_cross_entropy"
    _need_gpu(logits, target)
    logits, target, b, t, n_q, k, arr = _ce_operands(op, logits, target, sizes)
    lib = _lib.load()
    nll = torch.empty((b, t, n_q), dtype=torch.float32, device=logits.device)
    lse = torch.empty((b, t, n_q), dtype=torch.float32, device=logits.device)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    n_live = torch.empty((), dtype=torch.int64, device=logits.device)
    nbytes = int(lib.agx_codes_cross_entropy_workspace_bytes(b, t, n_q))
    ws = _workspace(nbytes, logits.device, "agx_codes_cross_entropy_workspace_bytes")
    tok = _observer.begin("other", (op, 4 * logits.numel() + 16 * target.numel(), 0)) if _observer is not None else None
    _lib.check(lib.agx_codes_cross_entropy(_ptr(logits), _ptr(target), _arr_ptr(arr), b, t, n_q, k, _ptr(nll), _ptr(lse), _ptr(loss),
                                           _ptr(n_live), _ptr(ws), nbytes, _stream()), "agx_codes_cross_entropy")
    if tok is not None:
        _observer.end(tok)
    return loss, nll, lse, n_live


def codes_cross_entropy_backward(logits: Tensor, target: Tensor, lse: Tensor, n_live: Tensor, g: Tensor,
                                 sizes: Optional[Sequence[int]] = None) -> Tensor:
    """Backward of ``codes_cross_entropy`` from its ``lse`` and ``n_live`` and ``g``, one fp32 on the device (the gradient of the
    loss; never read on the host) -> dlogits (B, Q K, T), ``g (softmax - onehot) / n_live`` at live entries, exact 0 at dead ones
    and at ``k >= sizes[q]``."""
    op = "codes_cross_entropy_backward"
    _need_gpu(logits, target, lse, n_live, g)
    logits, target, b, t, n_q, k, arr = _ce_operands(op, logits, target, sizes)
    lse = _checked_operand(op, "lse", lse, torch.float32, (b, t, n_q), logits.device)
    if not isinstance(n_live, Tensor) or n_live.dtype != torch.int64 or n_live.numel() != 1 or n_live.device != logits.device:
        raise AgxError(f"{op}: n_live must be the one-element int64 device tensor the forward returned")
    if not isinstance(g, Tensor) or g.dtype != torch.float32 or g.numel() != 1 or g.device != logits.device:
        raise AgxError(f"{op}: g must hold one float32 on the operands' device")
    dlogits = torch.empty(logits.shape, dtype=torch.float32, device=logits.device)
    tok = _observer.begin("other", (op, 8 * logits.numel(), 0)) if _observer is not None else None
    _lib.check(_lib.load().agx_codes_cross_entropy_backward(_ptr(logits), _ptr(target), _arr_ptr(arr), _ptr(lse), _ptr(n_live), _ptr(g),
                                                            b, t, n_q, k, _ptr(dlogits), _stream()), "agx_codes_cross_entropy_backward")
    if tok is not None:
        _observer.end(tok)
    return dlogits


def codes_sample(logits: Tensor, n_q: int, seeds: Tensor, frame0: Tensor, temperature: Tensor, top_k: Tensor, top_p: Tensor,
                 sizes: Optional[Sequence[int]] = None, counts: Optional[Tensor] = None, stages: Optional[Tensor] = None,
                 carry: Optional[Tensor] = None) -> Tensor:
    """Temperature / top-k / top-p sampling on the device (``agx_codes_sample``, one launch): logits (B, n_q K, n) fp32 -> codes
    (B, n, n_q) int64, ``K <= CODES_SAMPLE_MAX_K``.  Per row, all on the device: ``seeds`` and ``frame0`` int64 (B,) -- frame i of row
    b draws at Philox counter ``(frame0[b] + i, q)`` under key ``seeds[b]`` --, ``temperature`` fp32 (``<= 0``: the argmax),
    ``top_k`` int64 (``<= 0``: off), ``top_p`` fp32 (``>= 1``: off).  include/agx.h "Code prior" states the contract of a row; a draw
    is a pure function of (seed, frame, stage, logits, settings).  ``counts`` / ``stages``: -1 behind a row's frame count or stage
    count.  ``carry`` (B, n_q) int64, in/out: takes the codes of frame ``c_b - 1`` where ``c_b >= 1``, untouched otherwise."""
    op = "codes_sample"
    _need_gpu(logits, seeds, frame0, temperature, top_k, top_p, counts, stages, carry)
    logits = _checked_operand(op, "logits", logits, torch.float32, (None, None, None))
    b, c, n = logits.shape
    n_q = int(n_q)
    if b < 1 or n < 1 or n_q < 1 or c < 1 or c % n_q:
        raise AgxError(f"{op}: logits {tuple(logits.shape)} are not (B, Q K, n) for Q = {n_q}")
    k = c // n_q
    if k > CODES_SAMPLE_MAX_K:
        raise AgxError(f"{op}: K = {k} codes per stage exceed CODES_SAMPLE_MAX_K = {CODES_SAMPLE_MAX_K}")
    arr = _stage_sizes(op, sizes, n_q, k)
    dev = logits.device
    seeds = _checked_operand(op, "seeds", seeds, torch.int64, (b,), dev)
    frame0 = _checked_operand(op, "frame0", frame0, torch.int64, (b,), dev)
    temperature = _checked_operand(op, "temperature", temperature, torch.float32, (b,), dev)
    top_k = _checked_operand(op, "top_k", top_k, torch.int64, (b,), dev)
    top_p = _checked_operand(op, "top_p", top_p, torch.float32, (b,), dev)
    counts, stages = _checked_rows(op, b, dev, counts, stages)
    if carry is not None:
        carry = _checked_operand(op, "carry", carry, torch.int64, (b, n_q), dev)
    codes = torch.empty((b, n, n_q), dtype=torch.int64, device=dev)
    tok = _observer.begin("other", (op, 4 * logits.numel() + 8 * codes.numel(), 0)) if _observer is not None else None
    _lib.check(_lib.load().agx_codes_sample(_ptr(logits), _arr_ptr(arr), _ptr(seeds), _ptr(frame0), _ptr(temperature), _ptr(top_k),
                                            _ptr(top_p), _ptr(counts), _ptr(stages), _ptr(carry), _ptr(codes), b, n, n_q, k, _stream()),
               "agx_codes_sample")
    if tok is not None:
        _observer.end(tok)
    return codes


# --------------------------------------------------------------------------- entropy coding
RANS_SCALE_BITS = _lib.RANS_SCALE_BITS
RANS_M = 1 << _lib.RANS_SCALE_BITS
RANS_L = _lib.RANS_L
RANS_MAX_SYMBOLS = _lib.RANS_MAX_SYMBOLS
CODES_CUM_MAX_K = _lib.CODES_CUM_MAX_K


def _entropy_limits(op: str, n_q: int, k: int, symbols: Optional[int] = None) -> None:
    """The refusals of include/agx.h "Entropy coding" that need no tensor, made on the host before anything else."""
    if n_q > 64:
        raise AgxError(f"{op}: at most 64 stages, got {n_q}")
    if k > CODES_CUM_MAX_K:
        raise AgxError(f"{op}: K = {k} codes per stage exceed CODES_CUM_MAX_K = {CODES_CUM_MAX_K}")
    if symbols is not None and symbols > RANS_MAX_SYMBOLS:
        raise AgxError(f"{op}: n Q = {symbols} symbols per row exceed RANS_MAX_SYMBOLS = {RANS_MAX_SYMBOLS}")


def _need_gpu_tables(t: Optional[Tensor]) -> None:
    """``_need_gpu`` for the int32 frequency tables, the one operand of this library outside ``_DTYPES``."""
    if t is not None and not t.is_cuda:
        raise AgxError(f"audio_generation_amd runs on the MI355X only: got a tensor on '{t.device}'.  There is no CPU / eager fallback.")


def codes_cum(logits: Tensor, n_q: int, sizes: Optional[Sequence[int]] = None, counts: Optional[Tensor] = None,
              stages: Optional[Tensor] = None, out: Optional[Tensor] = None, frame0: int = 0) -> Tensor:
    """Logits -> exactly normalised integer frequency tables (``agx_codes_cum``, one launch): logits (B, n_q K, n) fp32 -> cum
    int32 (B, n, n_q, K + 1), ``cum[b, i, q]`` the exclusive prefix sums of the frequencies of stage q at frame i: ``cum[0] == 0``,
    strictly increasing below ``sizes[q]``, ``RANS_M`` from there on; include/agx.h "Entropy coding" states the contract of an
    entry.  ``counts`` / ``stages``: the tables behind a row's frame count or stage count are exact 0 and their logits are not
    read.  ``out`` (int32 (B, n_out, n_q, K + 1)) with ``frame0``: the call's frames land at ``out[:, frame0:frame0 + n]`` and
    nothing else of ``out`` is touched -- a hop's tables gathered from one-frame steps.  ``K <= CODES_CUM_MAX_K``."""
    op = "codes_cum"
    logits = _checked_operand(op, "logits", logits, torch.float32, (None, None, None))
    b, c, n = logits.shape
    n_q, frame0 = int(n_q), int(frame0)
    if b < 1 or n < 1 or n_q < 1 or c < 1 or c % n_q:
        raise AgxError(f"{op}: logits {tuple(logits.shape)} are not (B, Q K, n) for Q = {n_q}")
    k = c // n_q
    _entropy_limits(op, n_q, k)
    arr = _stage_sizes(op, sizes, n_q, k)
    if out is not None:
        out = _checked_operand(op, "out", out, torch.int32, (b, None, n_q, k + 1), logits.device)
        if not 0 <= frame0 <= out.shape[1] - n:
            raise AgxError(f"{op}: frames {frame0} .. {frame0 + n - 1} do not lie in a table buffer of {out.shape[1]} frames")
    elif frame0:
        raise AgxError(f"{op}: frame0 = {frame0} without a table buffer")
    _need_gpu(logits, counts, stages)
    _need_gpu_tables(out)
    counts, stages = _checked_rows(op, b, logits.device, counts, stages)
    if out is None:
        out = torch.empty((b, n, n_q, k + 1), dtype=torch.int32, device=logits.device)
    tok = _observer.begin("other", (op, 4 * logits.numel() + 4 * b * n * n_q * (k + 1), 0)) if _observer is not None else None
    _lib.check(_lib.load().agx_codes_cum(_ptr(logits), _arr_ptr(arr), _ptr(counts), _ptr(stages), _ptr(out), b, n, n_q, k, out.shape[1],
                                         frame0, _stream()), "agx_codes_cum")
    if tok is not None:
        _observer.end(tok)
    return out


def _rans_tables(op: str, cum: Tensor):
    if not isinstance(cum, Tensor) or cum.dim() != 4:
        raise AgxError(f"{op}: cum must be an int32 (B, n, Q, K + 1) tensor, got "
                       f"{tuple(cum.shape) if isinstance(cum, Tensor) else type(cum).__name__}")
    cum = _checked_operand(op, "cum", cum, torch.int32, (None, None, None, None))
    b, n, n_q, k1 = cum.shape
    if b < 1 or n < 1 or n_q < 1 or k1 < 2:
        raise AgxError(f"{op}: cum {tuple(cum.shape)} is not (B, n, Q, K + 1)")
    _entropy_limits(op, n_q, k1 - 1, n * n_q)
    return cum, b, n, n_q, k1 - 1


def codes_rans_encode(cum: Tensor, codes: Tensor, sizes: Optional[Sequence[int]] = None, counts: Optional[Tensor] = None,
                      stages: Optional[Tensor] = None):
    """Byte-wise rANS of a hop (``agx_codes_rans_encode``, one launch, one wave per row): cum int32 (B, n, Q, K + 1)
    (``codes_cum``), codes int64 (B, n, Q) -> (packets uint8 (B, 2 n Q + 4), nbytes int64 (B,), status int64 (B,)).  Row b's
    packet is its first ``nbytes[b]`` bytes -- 0 when the row codes nothing -- and every byte behind them is 0; its symbols are
    its live entries (``counts`` / ``stages``) in (frame, stage) order.  ``status``: bit 0 when a live code lay outside its stage
    (it is skipped).  The bytes are pinned by include/agx.h "Entropy coding" (tests/entropy_ref.py mirrors them in Python ints)."""
    op = "codes_rans_encode"
    cum, b, n, n_q, k = _rans_tables(op, cum)
    codes = _checked_operand(op, "codes", codes, torch.int64, (b, n, n_q), cum.device)
    arr = _stage_sizes(op, sizes, n_q, k)
    _need_gpu_tables(cum)
    _need_gpu(codes, counts, stages)
    counts, stages = _checked_rows(op, b, cum.device, counts, stages)
    packets = torch.empty((b, 2 * n * n_q + 4), dtype=torch.uint8, device=cum.device)
    nbytes = torch.empty((b,), dtype=torch.int64, device=cum.device)
    status = torch.empty((b,), dtype=torch.int64, device=cum.device)
    tok = _observer.begin("other", (op, 8 * codes.numel() + 8 * codes.numel() + packets.numel(), 0)) if _observer is not None else None
    _lib.check(_lib.load().agx_codes_rans_encode(_ptr(cum), _ptr(codes), _arr_ptr(arr), _ptr(counts), _ptr(stages), _ptr(packets),
                                                 _ptr(nbytes), _ptr(status), b, n, n_q, k, _stream()), "agx_codes_rans_encode")
    if tok is not None:
        _observer.end(tok)
    return packets, nbytes, status


def codes_rans_decode(cum: Tensor, packets: Tensor, nbytes: Tensor, state: Tensor, status: Tensor, i0: int = 0, n: Optional[int] = None,
                      sizes: Optional[Sequence[int]] = None, counts: Optional[Tensor] = None, stages: Optional[Tensor] = None,
                      carry: Optional[Tensor] = None) -> Tensor:
    """The receiver (``agx_codes_rans_decode``, one launch, one wave per row): frames ``i0 .. i0 + n - 1`` (default: all behind
    ``i0``) of a hop whose tables are cum int32 (B, hop, Q, K + 1) -> codes int64 (B, n, Q), -1 behind a row's frame count
    (``counts``, of the hop) and stage count.  packets uint8 (B, any width), nbytes int64 (B,).  ``state`` int64 (B, 2) and
    ``status`` int64 (B,) are in/out: the coder's state and read cursor, and the row's error bits (1: a live code was skipped by
    the sender -- never set here; 2: a read past the packet; 4: the packet did not end where the coder started); the call with
    ``i0 == 0`` starts them, later ones continue.  ``carry`` int64 (B, Q), in/out: takes the codes of a row's last frame when this
    call decoded it.  One call and ``n`` calls of one frame agree bit for bit."""
    op = "codes_rans_decode"
    cum, b, hop, n_q, k = _rans_tables(op, cum)
    i0 = int(i0)
    n = hop - i0 if n is None else int(n)
    if n < 1 or i0 < 0 or i0 > hop - n:
        raise AgxError(f"{op}: frames {i0} .. {i0 + n - 1} do not lie in a hop of {hop} frames")
    dev = cum.device
    packets = _checked_operand(op, "packets", packets, torch.uint8, (b, None), dev)
    if packets.shape[1] < 1:
        raise AgxError(f"{op}: packets {tuple(packets.shape)} hold no byte")
    nbytes = _checked_operand(op, "nbytes", nbytes, torch.int64, (b,), dev)
    state = _checked_operand(op, "state", state, torch.int64, (b, 2), dev)
    status = _checked_operand(op, "status", status, torch.int64, (b,), dev)
    if carry is not None:
        carry = _checked_operand(op, "carry", carry, torch.int64, (b, n_q), dev)
    arr = _stage_sizes(op, sizes, n_q, k)
    _need_gpu_tables(cum)
    _need_gpu(packets, nbytes, state, status, counts, stages, carry)
    counts, stages = _checked_rows(op, b, dev, counts, stages)
    codes = torch.empty((b, n, n_q), dtype=torch.int64, device=dev)
    tok = _observer.begin("other", (op, 8 * codes.numel() + 8 * codes.numel() + packets.numel(), 0)) if _observer is not None else None
    _lib.check(_lib.load().agx_codes_rans_decode(_ptr(cum), _ptr(packets), _ptr(nbytes), _arr_ptr(arr), _ptr(counts), _ptr(stages),
                                                 _ptr(state), _ptr(codes), _ptr(carry), _ptr(status), b, hop, i0, n, n_q, k,
                                                 packets.shape[1], _stream()), "agx_codes_rans_decode")
    if tok is not None:
        _observer.end(tok)
    return codes
