"""Drop-in ``Alibi`` / ``Attention`` / ``FeedForward`` / ``Transformer`` executed
by libagx, plus the bottleneck adapter the reference never shipped.

Mirrors ``networks/transformers.py:7-279`` (class names, constructor arguments,
``state_dict()`` keys ``layers.{i}.0.norm.*``, ``layers.{i}.0.W_{q,k,v,o}.weight``,
``layers.{i}.1.net.{0,1,4}.*``).  The branches the reference can actually
execute are implemented: ALiBi self-attention, and ALiBi cross-attention
(``context_y=``: queries from ``LN(x)``, keys and values from the un-normalised
second sequence ``y``, transformers.py:159-170 -- it runs in the reference, with
``Alibi.M`` stored transposed, see ``Alibi``).  The learned pos-emb branch raises
in the reference and here.  ``depth > 1`` is build-defined as "every
layer uses ALiBi"; with ``context_y`` layer 0 is the cross-attention layer
(transformers.py:272-273) and the later ones are self-attention over ``context_x``.

Execution is channel-major: the block works on ``(B, C, T)`` tensors (what the
encoder emits), every ``Linear`` is a k=1 convolution on the fp32 MFMA conv
kernel with the activation / residual fused into its epilogue, LayerNorm and
softmax(QK^T + ALiBi)V are the two dedicated kernels of ``csrc/attention.hip``
(cross-attention: ``csrc/attention_cross.hip``, fp32 only).  ``dropout > 0`` acts in
training mode only, on counter-based masks generated inside the kernels of
``csrc/attention_dropout.hip`` (``Transformer._hip_bct``); in eval mode it is the identity.
``causal=True`` (build-defined, default off) makes every self-attention layer one-sided -- keys ``j <= i``, bias
``-slope_h (i - j)`` -- on the kernels of ``csrc/attention_causal.hip``, and lets a ``Transformer`` run incrementally on a
key/value cache (``Transformer.new_cache``).  ``window=W`` (with ``causal=True``) narrows every query to its last ``W`` keys
on the kernels of ``csrc/attention_window.hip``; the cache is then a ring of fixed size and the stream has no end.
``Transformer.new_stream_cache`` keeps the position of every batch row in device memory (``csrc/attention_stream.hip``): a
cached step can be captured and replayed, and a row restarts without the others.
``lengths=`` / ``y_lengths=`` (build-defined, keyword-only, default None) give every batch row of ``x`` / ``y`` its own valid
length for a right-padded ragged batch: the symmetric layers run on the kernels of ``csrc/attention_ragged.hip``, which read
the lengths from device memory, the block's output is exactly 0 at padded positions, and its valid positions and every
gradient are independent of what the padding held, NaN included (``Transformer._hip_bct``).  fp32, no dropout, not on a
causal layer -- whose valid frames never see right padding anyway.
``Transformer.run_packed`` (build-defined) takes the same batch without its padding: the sequences concatenated along the time
axis, ``(1, dim, N)`` with ``N`` the sum of the lengths, and ``cu_seqlens``, the n_seq + 1 starts and ends.  Every op but the
attention is pointwise in time and runs on the packed tensor as it is; the attention runs on the kernels of
``csrc/attention_packed.hip``, which read ``cu_seqlens`` from device memory.  ``pack_padded`` / ``unpack_padded`` convert.
``ConformerConvBlock`` / ``ConformerBlock`` (transformers.py:281-368; build-defined where the reference cannot be constructed, see the
classes) run their GLU, depthwise "same" convolution, BatchNorm1d and SiLU on the kernels of ``csrc/conformer.hip``, training and eval
mode, forward and backward; ``FeedForward(activation=nn.SiLU)`` is their feed-forward half.
The ``nn.LayerNorm`` / ``nn.Linear`` children only hold parameters.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import ops
from ._lib import CONV_CAUSAL, EPI_GELU_PRE, EPI_RESIDUAL, AgxError, needs_grad

Tensor = torch.Tensor


class Alibi(nn.Module):
    """transformers.py:7-93.  ``M`` is a registered (non-persistent) buffer here,
    so it follows ``.to(device)`` -- the reference leaves it on the CPU.
    The attention kernels never read ``M``: they evaluate ``-slope_h * |i - j|`` themselves.

    With ``context_y`` the reference's ``_create_M`` (:45-77) builds ``M`` as ``(H, context_y, context_x)`` in both of its
    branches -- the transpose of the ``(context_x, context_y)`` it is cropped as (:92) -- with every entry
    ``-slope_h * |row - col|``.  The formula is symmetric, so the transposition changes the lengths a call accepts
    (``Attention.run_bct``) and no value; ``M`` is built here with the reference's shape."""

    def __init__(self, context_x, context_y=None, n_heads=8):
        super().__init__()
        self.context_x = context_x
        self.context_y = context_x if context_y is None else context_y
        self.n_heads = n_heads
        n_sequence = torch.arange(start=n_heads, end=0, step=-1)
        self.register_buffer("head_scalars", 2 ** (-8 / n_sequence), persistent=False)  # :38-39
        rows, cols = torch.arange(self.context_y, dtype=torch.float32), torch.arange(context_x, dtype=torch.float32)
        m = -(rows[:, None] - cols[None, :]).abs()
        self.register_buffer("M", m[None, :] * self.head_scalars[:, None, None], persistent=False)
        self.requires_grad_(False)

    def get_M(self, crop=None):
        m = self.M
        if crop is not None:
            if isinstance(crop, int):
                crop = (crop, crop)
            m = m[:, :crop[0], :crop[1]]
        return m.unsqueeze(0)


class _PackedLinear:
    """One or more ``nn.Linear`` stacked along the output dim and run as one k=1 convolution over the channel dim of a
    (B, C, T) tensor; caches the packed image of the stacked weights.  ``scale`` (a power of two: exact in fp32) is folded into
    the image and the bias -- ``scale (W h + b) == (scale W) h + scale b`` bit for bit, short of underflow -- and into the
    parameter gradients ``backward`` returns: the 0.5 of ``ConformerBlock``'s half-step feed-forwards costs no launch."""

    def __init__(self, *linears, scale: float = 1.0):
        self.linears, self.scale = linears, float(scale)
        self.c_out = sum(l.out_features for l in linears)
        self.key = self.packed = self.bias = self.w3d = None

    def get(self):
        key = tuple((l.weight.data_ptr(), l.weight._version,
                     None if l.bias is None else (l.bias.data_ptr(), l.bias._version)) for l in self.linears)
        if key != self.key:
            w = torch.cat([l.weight.detach() for l in self.linears], dim=0)
            if self.scale != 1.0:
                w = w * self.scale
            c_out, c_in = w.shape
            desc = ops.conv_desc(CONV_CAUSAL, 1, c_in, c_out, 1 << 20, 1)
            self.w3d = w.reshape(c_out, c_in, 1).contiguous()      # the native backward reads it
            self.packed = ops.conv_pack(desc, self.w3d)
            if any(l.bias is not None for l in self.linears):
                self.bias = torch.cat([l.bias.detach() if l.bias is not None
                                       else torch.zeros(l.out_features, device=w.device) for l in self.linears])
            else:
                self.bias = None
            if self.bias is not None and self.scale != 1.0:
                self.bias = self.bias * self.scale
            self.key = key
        return self.packed, self.bias

    def forward(self, x: Tensor, epilogue: int = 0, res: Optional[Tensor] = None, slope: float = 0.1) -> Tensor:
        """``slope``: the LeakyReLU slope of an ``EPI_LEAKY_PRE`` epilogue (0.0: ReLU); the descriptor's default otherwise."""
        packed, bias = self.get()
        b, c_in, t = x.shape
        desc = ops.conv_desc(CONV_CAUSAL, b, c_in, self.c_out, t, 1, 1, 1, epilogue, slope)
        return ops.conv_forward(desc, x, packed, bias, res)

    def backward(self, x_in: Tensor, dy: Tensor, pre: Optional[Tensor] = None, want_dx: bool = True,
                 add: Optional[Tensor] = None, mask: Optional[Tensor] = None, slope: float = 0.1):
        """Backward of ``forward`` with epilogue 0, on the image that forward packed: (dx, the gradients of the linears'
        parameters in ``parameters()`` order); with ``pre`` the GELU gradient of the layer BELOW (at its pre-activation)
        is fused into the bwd-data epilogue.  ``want_dx=False`` skips the backward-data conv (dx is None).  Without ``pre``:
        ``add`` is accumulated into dx first and ``mask`` -- the layer input, the LeakyReLU(``slope``) output of the layer
        below -- multiplies it by that activation's gradient (``ops.conv_bwd_data``)."""
        b, c_in, t = x_in.shape
        desc = ops.conv_desc(CONV_CAUSAL, b, c_in, self.c_out, t, 1)
        dw, _, db = ops.conv_bwd_weight(desc, x_in, dy, self.w3d, None, want_bias=self.bias is not None)
        dx = None
        if want_dx:
            pk = ops.conv_pack_bwd(desc, self.w3d)
            dx = ops.conv_bwd_data(desc, dy, pk, add, mask, slope) if pre is None else ops.conv_bwd_data_gelu(desc, dy, pk, pre)
        dw, grads, row = dw.reshape(self.c_out, c_in), [], 0
        if self.scale != 1.0:      # dy reached the scaled layer: the gradients of the unscaled parameters
            dw, db = dw * self.scale, None if db is None else db * self.scale
        for l in self.linears:
            rows = slice(row, row + l.out_features)
            grads += [dw[rows]] if l.bias is None else [dw[rows], db[rows]]
            row = rows.stop
        return dx, grads


def _ln(ln: nn.LayerNorm, x: Tensor) -> Tensor:
    return ops.layernorm_ct(x, ln.weight.detach(), ln.bias.detach(), ln.eps)


def _ln_bwd(ln: nn.LayerNorm, x: Tensor, dy: Tensor, add: Tensor):
    """(dx + add, dweight, dbias): ``add`` is the gradient that reached the residual branch around the sub-block."""
    return ops.layernorm_ct_backward(x, ln.weight.detach(), dy, ln.eps, add=add)


def _active_p(drop: nn.Dropout) -> float:
    """The probability a dropout site applies in this call: 0 in eval mode (the site is the identity and no dropout kernel
    runs).  p = 1 drops everything and has no finite scale 1 / (1 - p): refused at the first training-mode call."""
    if not drop.training or drop.p == 0:
        return 0.0
    if not 0.0 < drop.p < 1.0:
        raise AgxError(f"dropout = {drop.p} in training mode: the kernels take 0 <= p < 1 (agx_dropout_add)")
    return float(drop.p)


def _site(drop: Optional[tuple], module: nn.Module) -> tuple:
    """(seed, layer) of a dropout site: what the enclosing ``Transformer`` drew for this forward, or -- a sub-block called on
    its own -- a fresh seed for layer 0, kept on the module as ``last_dropout_seed``."""
    if drop is None:
        drop = (ops.draw_dropout_seed(), 0)
        module.last_dropout_seed = drop[0]
    return drop


# stream ids of the four dropout sites of layer ``l``: 4 l + site
SITE_PROB, SITE_ATTN_OUT, SITE_FFN_HIDDEN, SITE_FFN_OUT = 0, 1, 2, 3


def _checked_window(window, causal, context_x) -> Optional[int]:
    """The ``window=`` constructor argument of ``Attention`` / ``Transformer``: None, or 1 <= window <= context_x on a causal layer."""
    if window is None:
        return None
    if not causal:
        raise ValueError("window= needs causal=True: the sliding window is a narrowed causal mask")
    if int(window) != window or window < 1:
        raise ValueError(f"window = {window}: a query sees at least itself (window >= 1)")
    if window > context_x:
        raise ValueError(f"window = {window} exceeds context_x = {context_x}: no call is longer than context_x frames, "
                         "so a larger window is causal=True without window")
    return int(window)


def _checked_lengths(what: str, lengths, batch: int, t: int, device) -> Optional[Tensor]:
    """A ``lengths=`` / ``y_lengths=`` argument as the kernels read it: ``batch`` int32 entries on ``device``, or None.
    A Python sequence or a CPU integer tensor is validated here (0 <= length <= t) and copied to the device.  A device
    integer tensor is used as it is, without a sync: the kernels clamp what it holds when they run, so under graph capture
    a replay reads the lengths of the replay."""
    if lengths is None:
        return None
    on_device = isinstance(lengths, Tensor) and lengths.is_cuda
    host = lengths if on_device else torch.as_tensor(lengths)
    if host.dtype.is_floating_point or host.dtype.is_complex or host.dtype == torch.bool:
        raise AgxError(f"{what} must hold integers, got {host.dtype}")
    if host.dim() != 1 or host.numel() != batch:
        raise AgxError(f"{what} has shape {tuple(host.shape)}: one length per batch row is ({batch},)")
    if on_device:
        return host.to(torch.int32).contiguous()
    if batch and (int(host.min()) < 0 or int(host.max()) > t):
        raise AgxError(f"{what} = {host.tolist()}: every length must lie in [0, {t}], the padded length")
    return host.to(torch.int32).to(device)


class _Packed:
    """The checked partition of a packed call (``Transformer._check_packed``): ``cu`` / ``y_cu`` are int32 device tensors of
    n_seq + 1 entries, ``max_len`` / ``y_max_len`` host-known bounds of the sequence lengths, and ``slack`` / ``y_slack`` say
    whether columns behind the last sequence may exist (a device array, or a host array that ends before N): only then does
    the walk mask them (``Transformer._hip_bct``)."""

    def __init__(self, cu, max_len, slack, y_cu=None, y_max_len=None, y_slack=False):
        self.cu, self.max_len, self.slack, self.y_cu, self.y_max_len, self.y_slack = cu, max_len, slack, y_cu, y_max_len, y_slack

    def attn_args(self, cross: bool) -> dict:
        if cross:
            return dict(cu_seqlens=self.cu, max_len=self.max_len, y_cu_seqlens=self.y_cu, y_max_len=self.y_max_len)
        return dict(cu_seqlens=self.cu, max_len=self.max_len)


def _checked_cu(what: str, cu, n: int, max_len, device) -> tuple:
    """A ``cu_seqlens`` argument over ``n`` packed columns -> (int32 device tensor, max_len, slack).  A Python sequence or a CPU
    integer tensor is validated here -- starts at 0, non-decreasing, ends at or before ``n`` -- its longest sequence is
    ``max_len`` (a given ``max_len`` must not be smaller) and ``slack`` says whether it ends before ``n``.  A device integer
    tensor is used as it is, without a sync: ``max_len`` must then be given, the kernels clamp what the array holds when they
    run, and ``slack`` is True because nobody here knows."""
    on_device = isinstance(cu, Tensor) and cu.is_cuda
    host = cu if on_device else torch.as_tensor(cu)
    if host.dtype.is_floating_point or host.dtype.is_complex or host.dtype == torch.bool:
        raise AgxError(f"{what} must hold integers, got {host.dtype}")
    if host.dim() != 1 or host.numel() < 2:
        raise AgxError(f"{what} has shape {tuple(host.shape)}: n_seq + 1 >= 2 entries, the start of every sequence and the end of the last")
    if max_len is not None and (int(max_len) != max_len or max_len < 0):
        raise AgxError(f"max_len = {max_len} for {what}: the bound of the sequence lengths is an integer >= 0")
    if on_device:
        if max_len is None:
            raise AgxError(f"a device {what} needs max_len: the host does not read the array, and the bound sizes the grid")
        return host.to(torch.int32).contiguous(), int(max_len), True
    vals = [int(v) for v in host.tolist()]
    if vals[0] != 0 or any(b < a for a, b in zip(vals, vals[1:])) or vals[-1] > n:
        raise AgxError(f"{what} = {vals}: it must start at 0, never decrease and end at or before N = {n}")
    longest = max(b - a for a, b in zip(vals, vals[1:]))
    if max_len is not None and max_len < longest:
        raise AgxError(f"max_len = {max_len} for {what}, whose longest sequence has {longest} frames")
    return host.to(torch.int32).to(device), (longest if max_len is None else int(max_len)), vals[-1] < n


def pack_padded(x: Tensor, lengths, total: Optional[int] = None) -> tuple:
    """A right-padded channel-major batch ``x`` (B, dim, T) with the valid ``lengths`` of its rows -> ``(xp, cu_seqlens,
    max_len)``, the arguments of ``Transformer.run_packed``: ``xp`` (1, dim, N), ``cu_seqlens`` an int32 device tensor (a device
    ``cumsum`` of the lengths).  Host ``lengths`` (a Python sequence or a CPU integer tensor) are validated, ``N`` is their sum
    and ``max_len`` their maximum.  Device ``lengths`` are not read: the caller passes ``total``, the capacity ``N`` of the
    packed tensor (at least their sum -- what lies behind it is slack, exactly 0), and ``max_len`` is T."""
    if x.dim() != 3:
        raise AgxError(f"pack_padded: x is {tuple(x.shape)}, expected (B, dim, T)")
    b, _, t = x.shape
    dev = _checked_lengths("lengths", lengths, b, t, x.device)
    if dev is None:
        raise AgxError("pack_padded: lengths is required")
    if isinstance(lengths, Tensor) and lengths.is_cuda:
        if total is None:
            raise AgxError("pack_padded: device lengths need total=, the capacity of the packed tensor (the host does not read them)")
        n, max_len = int(total), t
    else:
        host = [int(v) for v in torch.as_tensor(lengths).tolist()]
        n, max_len = sum(host), max(host, default=0)
        if total is not None:
            if total < n:
                raise AgxError(f"pack_padded: total = {total} is less than the sum of the lengths, {n}")
            n = int(total)
    cu = torch.zeros(b + 1, dtype=torch.int32, device=x.device)
    cu[1:] = torch.cumsum(dev, 0)
    return ops.pack_rows(x, cu, n), cu, max_len


def unpack_padded(xp: Tensor, cu_seqlens, t: int) -> Tensor:
    """The inverse of ``pack_padded``: a packed (1, dim, N) tensor -> the right-padded (B, dim, ``t``) batch, exactly 0 at padded
    positions.  ``cu_seqlens`` as ``Transformer.run_packed`` takes it."""
    if xp.dim() != 3 or xp.shape[0] != 1:
        raise AgxError(f"unpack_padded: xp is {tuple(xp.shape)}, expected (1, dim, N)")
    cu, _, _ = _checked_cu("cu_seqlens", cu_seqlens, xp.shape[-1], t, xp.device)
    return ops.unpack_rows(xp, cu, t)


class Attention(nn.Module):
    """transformers.py:95-191 (pre-LN multi-head attention with ALiBi).  ``context_y`` makes it a cross-attention layer:
    ``W_q`` reads ``LN(x)``, ``W_k`` / ``W_v`` (stacked into one projection) read the second sequence ``y`` as given."""

    def __init__(self, dim, dim_head=64, n_heads=8, dropout=0., bias=False, context_x=32, context_y=None,
                 has_pos_emb=True, alibi=True, causal=False, window=None):
        super().__init__()
        if not alibi:
            raise NotImplementedError("only the ALiBi branch is defined in the reference (SURVEY 5.1)")
        if causal and context_y is not None:
            raise ValueError("causal=True with context_y: causal cross-attention is not defined (cross-attention stays symmetric)")
        self.causal = bool(causal)     # build-defined: keys j <= i, bias -slope_h (i - j); parameters and state_dict unchanged
        self.window = _checked_window(window, causal, context_x)     # build-defined: the last ``window`` keys only
        self.dim, self.dim_head, self.n_heads = dim, dim_head, n_heads
        self.inner_dim = dim_head * n_heads
        self.norm = nn.LayerNorm(dim)
        self.W_q = nn.Linear(dim, self.inner_dim, bias=bias)
        self.W_k = nn.Linear(dim, self.inner_dim, bias=bias)
        self.W_v = nn.Linear(dim, self.inner_dim, bias=bias)
        self.W_o = nn.Linear(self.inner_dim, dim, bias=bias)
        self.dropout = nn.Dropout(dropout)
        self.alibi = alibi
        self.has_pos_emb = has_pos_emb
        self.cross_attention = context_y is not None     # :146
        self.context = context_x
        self.alibi_obj = Alibi(context_x, context_y, n_heads=n_heads)
        self._o = _PackedLinear(self.W_o)
        if self.cross_attention:     # two projections: W_q on LN(x), W_k / W_v stacked on y
            self._q, self._kv = _PackedLinear(self.W_q), _PackedLinear(self.W_k, self.W_v)
        else:
            self._qkv = _PackedLinear(self.W_q, self.W_k, self.W_v)
        # arithmetic of the QK^T / PV contractions: "fp32" (exact, the reference's) or "bf16" (bf16 MFMA, fp32 accumulate
        # and softmax -- BASELINE config 3); inference only (run_bct: ``keep``)
        self.attention_dtype = "fp32"
        self.last_dropout_seed = None     # the mask seed of the last training-mode forward with dropout > 0

    def _attn(self) -> dict:
        return dict(slopes=self.alibi_obj.head_scalars, heads=self.n_heads, head_dim=self.dim_head, scale_div=self.dim_head ** 0.5)

    def _check_ragged(self) -> None:
        """The refusals of a call with ``lengths`` / ``y_lengths``, before any op."""
        if self.causal:
            raise AgxError("lengths= on a causal" + (" (windowed)" if self.window is not None else "") + " layer: a causal layer's "
                           "valid frames never see right padding, so the call without lengths is already correct")
        if _active_p(self.dropout) > 0:
            raise AgxError("lengths= with an active dropout site (training mode, dropout > 0): dropout on ragged batches has "
                           "no kernel (eval mode runs)")
        if self.attention_dtype != "fp32":
            raise AgxError(f"lengths=: ragged attention runs in fp32, attention_dtype = {self.attention_dtype!r} has no kernel")

    def _check_packed(self) -> None:
        """The refusals of a packed call that depend on the layer alone, before any op."""
        if self.causal:
            raise AgxError("a packed batch on a causal" + (" (windowed)" if self.window is not None else "") + " layer: packed "
                           "attention is symmetric, causal and windowed packed calls have no kernel")
        if _active_p(self.dropout) > 0:
            raise AgxError("a packed batch with an active dropout site (training mode, dropout > 0): dropout on packed batches "
                           "has no kernel (eval mode runs)")
        if self.attention_dtype != "fp32":
            raise AgxError(f"a packed batch runs in fp32: attention_dtype = {self.attention_dtype!r} has no packed kernel")

    def _run_packed_bct(self, x: Tensor, residual: Optional[Tensor], keep: Optional[dict], y: Optional[Tensor], kv_cache,
                        cu_seqlens, max_len, y_cu_seqlens, y_max_len) -> Tensor:
        """The layer on a packed batch (``run_bct``): every refusal, then the plain walk with ``attention_alibi_packed`` where
        the attention op was."""
        if kv_cache is not None:
            raise AgxError("a packed batch with a key/value cache: a cached call is causal and packed attention is symmetric")
        self._check_packed()
        if x.dim() != 3 or x.shape[0] != 1 or x.shape[1] != self.dim:
            raise AgxError(f"a packed batch is one row: x is {tuple(x.shape)}, expected (1, {self.dim}, N)")
        if cu_seqlens is None or max_len is None:
            raise AgxError("a packed call needs cu_seqlens and max_len (a device array is not read by the host: max_len sizes the grid)")
        if self.cross_attention != (y_cu_seqlens is not None):
            raise AgxError("y_cu_seqlens= on a self-attention layer (built without context_y): there is no second sequence"
                           if y_cu_seqlens is not None else
                           "a cross-attention layer (built with context_y) needs y_cu_seqlens, the partition of its second sequence")
        if keep is not None and self.dim_head > 128:
            raise AgxError("Transformer: the attention backward kernels cover head_dim <= 128 "
                           "(agx_attention_alibi_packed_backward); larger heads have no kernel -- there is no ATen fallback")
        if self.cross_attention:
            if y is None or y.dim() != 3 or y.shape[0] != 1 or y.shape[1] != self.dim:
                raise AgxError(f"packed cross-attention: y is {None if y is None else tuple(y.shape)}, expected (1, {self.dim}, Ny)")
            if y_max_len is None:
                raise AgxError("a packed call needs y_max_len with y_cu_seqlens")
            if y_cu_seqlens.numel() != cu_seqlens.numel():
                raise AgxError(f"x has {cu_seqlens.numel() - 1} sequences and y has {y_cu_seqlens.numel() - 1}: sequence s of x "
                               "attends to sequence s of y")
            cx, cy = self.alibi_obj.context_x, self.alibi_obj.context_y
            if not ((max_len <= cx and y_max_len <= cy) or (max_len <= cy and y_max_len <= cx)):
                raise AgxError(f"sequence lengths up to ({max_len}, {y_max_len}) exceed the ALiBi contexts ({cx}, {cy}) in both orders")
            xn = _ln(self.norm, x)
            q = self._q.forward(xn)
            kv = self._kv.forward(y)
            o = ops.attention_alibi_packed(q, kv, cu_q=cu_seqlens, max_q=max_len, cu_k=y_cu_seqlens, max_k=y_max_len, **self._attn())
            if keep is not None:
                keep.update(h=x, xn1=xn, q=q, y=y, kv=kv, o=o)
            return self._o.forward(o, EPI_RESIDUAL if residual is not None else 0, residual)
        if y is not None:
            raise AgxError("a self-attention layer (built without context_y) takes no second sequence y")
        if max_len > self.context:
            raise AgxError(f"sequence lengths up to max_len = {max_len} exceed the ALiBi context {self.context}")
        xn = _ln(self.norm, x)
        qkv = self._qkv.forward(xn)
        o = ops.attention_alibi_packed(qkv, None, cu_q=cu_seqlens, max_q=max_len, **self._attn())
        if keep is not None:
            keep.update(h=x, xn1=xn, qkv=qkv, o=o)
        return self._o.forward(o, EPI_RESIDUAL if residual is not None else 0, residual)

    def _run_cross_bct(self, x: Tensor, residual: Optional[Tensor], keep: Optional[dict], y: Optional[Tensor],
                       drop: Optional[tuple] = None, lengths: Optional[Tensor] = None,
                       y_lengths: Optional[Tensor] = None) -> Tensor:
        """The cross-attention layer: LN1 -> Q projection, KV projection of ``y`` (no LayerNorm, transformers.py:170) ->
        attention -> W_o (+res).  Lengths: what the reference runs -- its transposed ``M[:, :Tx, :Ty]`` (:92) must broadcast,
        ``Tx <= context_y and Ty <= context_x`` -- and the intended reading ``Tx <= context_x and Ty <= context_y``; the
        bias is the same formula in both."""
        if y is None:
            raise AgxError("Cross attention requires two inputs: this layer was built with context_y and got no y "
                           "(the reference asserts here, transformers.py:166)")
        if y.dim() != 3 or y.shape[0] != x.shape[0] or y.shape[1] != self.dim:
            raise AgxError(f"cross-attention: y is {tuple(y.shape)}, expected ({x.shape[0]}, {self.dim}, Ty)")
        cx, cy = self.alibi_obj.context_x, self.alibi_obj.context_y
        tx, ty = x.shape[-1], y.shape[-1]
        if not ((tx <= cx and ty <= cy) or (tx <= cy and ty <= cx)):
            raise AgxError(f"sequence lengths ({tx}, {ty}) exceed the ALiBi contexts ({cx}, {cy}) in both orders "
                           "(the reference fails here too, transformers.py:88-93)")
        if self.attention_dtype != "fp32":
            raise AgxError(f"cross-attention runs in fp32: attention_dtype = {self.attention_dtype!r} has no kernel")
        if keep is not None and self.dim_head > 128:
            raise AgxError("Transformer: the attention backward kernels cover head_dim <= 128 "
                           "(agx_attention_alibi_cross_backward); larger heads have no kernel -- there is no ATen fallback")
        p = _active_p(self.dropout)
        xn = _ln(self.norm, x)
        q = self._q.forward(xn)
        kv = self._kv.forward(y)
        if p > 0:
            seed, layer = _site(drop, self)
            o = ops.attention_alibi_dropout(q, kv, p=p, seed=seed, stream_id=4 * layer + SITE_PROB, **self._attn())
        elif lengths is not None or y_lengths is not None:
            o = ops.attention_alibi_ragged(q, kv, q_len=lengths, k_len=y_lengths, **self._attn())
        else:
            o = ops.attention_alibi_cross(q, kv, **self._attn())
        if keep is not None:
            keep.update(h=x, xn1=xn, q=q, y=y, kv=kv, o=o)
        if p > 0:
            return self._drop_out(o, residual, keep, p, seed, layer)
        return self._o.forward(o, EPI_RESIDUAL if residual is not None else 0, residual)

    def _drop_out(self, o: Tensor, residual: Optional[Tensor], keep: Optional[dict], p: float, seed: int, layer: int) -> Tensor:
        """The tail of a training-mode walk with dropout: W_o without the fused residual, then dropout (+ residual) in place."""
        if keep is not None:
            keep["drop"] = dict(seed=seed, layer=layer, attn=p)
        ao = self._o.forward(o)
        return ops.dropout_add(ao, residual, p, seed, 4 * layer + SITE_ATTN_OUT, out=ao)

    def _run_causal_bct(self, x: Tensor, residual: Optional[Tensor], keep: Optional[dict], kv_cache: Optional[tuple]) -> Tensor:
        """The causal layer: the walk of the self-attention layer with ``attention_alibi_causal`` in place of
        ``attention_alibi``.  Every refusal comes before the first op.  ``kv_cache`` = (buffer (B, 2*H*Dh, capacity), length):
        the K / V rows of the new frames are copied into columns [length, length + n) of the buffer (a strided device copy) and
        the queries, read in place from qkv, attend to the buffer's first length + n columns from position ``length``.

        With ``window`` the two causal ops are ``attention_alibi_window`` / ``attention_alibi_window_backward`` and the buffer
        is a ring: frame ``length + t`` goes to column ``(length + t) mod capacity`` (one strided copy, two when the chunk
        wraps), ``n + min(window - 1, length) <= capacity`` and ``length`` has no limit.

        ``kv_cache`` = (ring, pos) with ``pos`` an int64 (B,) device tensor (``TransformerStreamCache``): the same walk with
        ``ops.ring_write_pos`` / ``ops.attention_alibi_stream`` in place of ``ops.ring_write`` / ``ops.attention_alibi_window`` --
        both read every row's position from ``pos`` -- and the worst-case bound ``n + window - 1 <= capacity``.

        ``kv_cache`` = (ring, pos, counts): the counted step.  Row ``b``'s K / V rows beyond its first
        ``counts[b]`` frames are not written, and the attention's keys end at the count -- a masked key still meets its V
        as ``0 * v``, so an unwritten ring column must not be live.  What the queries behind the count hold is the caller's to
        mask (``Transformer`` / ``ConformerBlock`` do)."""
        if self.attention_dtype != "fp32":
            raise AgxError(f"causal attention runs in fp32: attention_dtype = {self.attention_dtype!r} has no kernel")
        if _active_p(self.dropout) > 0:
            raise AgxError("causal attention with dropout > 0 in training mode has no kernel (eval mode runs)")
        if keep is not None and kv_cache is not None:
            raise AgxError("there is no backward through a cached call")
        on_device = kv_cache is not None and isinstance(kv_cache[1], Tensor)     # a stream cache: positions in device memory
        if on_device and self.window is None:
            raise AgxError("device-held positions need a windowed layer (window=): the linear cache's limit needs the host to "
                           "know the position")
        if kv_cache is not None and self.window is not None:
            # the cached frames the first new query still sees; the worst case where the host does not know the position
            behind = self.window - 1 if on_device else min(self.window - 1, kv_cache[1])
            if x.shape[-1] + behind > kv_cache[0].shape[-1]:
                raise AgxError(f"cached call: {x.shape[-1]} new frames + the {behind} cached frames their window reaches exceed "
                               f"the ring's {kv_cache[0].shape[-1]} columns")
        elif kv_cache is not None and kv_cache[1] + x.shape[-1] > min(kv_cache[0].shape[-1], self.context):
            raise AgxError(f"cached call: {kv_cache[1]} cached + {x.shape[-1]} new frames exceed the buffer's "
                           f"{kv_cache[0].shape[-1]} columns or the ALiBi context {self.context}")
        xn = _ln(self.norm, x)
        qkv = self._qkv.forward(xn)
        if self.window is not None:
            if kv_cache is None:
                o = ops.attention_alibi_window(qkv, None, window=self.window, **self._attn())
            elif on_device:      # pos (B,) is read by both kernels: one write launch, wrap included
                buf, pos = kv_cache[:2]
                counts = kv_cache[2] if len(kv_cache) > 2 else None
                ops.ring_write_pos(buf, qkv[:, self.inner_dim:, :], pos, buf.shape[-1], counts=counts)
                o = ops.attention_alibi_stream(qkv, buf, pos, window=self.window, ring=buf.shape[-1], counts=counts, **self._attn())
            else:
                buf, length = kv_cache
                n, cap = x.shape[-1], buf.shape[-1]
                col0 = length % cap
                head = min(n, cap - col0)          # the frames that fit before the ring wraps
                ops.ring_write(buf, qkv[:, self.inner_dim:, :head], col0)
                if head < n:
                    ops.ring_write(buf, qkv[:, self.inner_dim:, head:], 0)
                o = ops.attention_alibi_window(qkv, buf, window=self.window, q_pos0=length, ring=cap, **self._attn())
        elif kv_cache is None:
            o = ops.attention_alibi_causal(qkv, None, **self._attn())
        else:
            buf, length = kv_cache
            n = x.shape[-1]
            buf[:, :, length:length + n].copy_(qkv[:, self.inner_dim:, :])
            o = ops.attention_alibi_causal(qkv, buf, q_pos0=length, tk=length + n, **self._attn())
        if keep is not None:
            keep.update(h=x, xn1=xn, qkv=qkv, o=o)
        return self._o.forward(o, EPI_RESIDUAL if residual is not None else 0, residual)

    def run_bct(self, x: Tensor, residual: Optional[Tensor] = None, keep: Optional[dict] = None,
                y: Optional[Tensor] = None, drop: Optional[tuple] = None, kv_cache: Optional[tuple] = None, *,
                lengths=None, y_lengths=None, cu_seqlens=None, max_len=None, y_cu_seqlens=None, y_max_len=None) -> Tensor:
        """(B, dim, T) -> W_o(attn(LN(x))) [+ residual], channel-major; a cross-attention layer also takes ``y``
        (B, dim, Ty).  ``keep`` marks the training forward: the dict
        receives what ``backward_bct`` reads, and the attention arithmetic is fp32 whatever ``attention_dtype`` says
        (the backward kernels recompute P from fp32 scores, and cover head_dim <= 128).

        In training mode (``self.training``; grad mode plays no part, as in torch) with ``dropout > 0`` the probabilities and
        the W_o output are dropped (transformers.py:185, :191): ``attention_alibi_dropout``, then W_o without the fused
        residual and ``dropout_add(., residual)``.  ``drop`` = (seed, layer) from the enclosing ``Transformer``.  fp32,
        head_dim <= 128.  In eval mode, or with ``dropout == 0``, the walk is the one it always was.

        A ``causal`` layer runs ``_run_causal_bct`` (fp32, no dropout in training mode); ``kv_cache`` is its cached call.

        ``lengths`` (``y_lengths``: a cross-attention layer's second sequence) are the valid lengths of the batch rows
        (``_checked_lengths``): the layer's launches are unchanged but for ``attention_alibi_ragged`` where its attention op
        was, with ``q_len = k_len = lengths`` (cross: ``k_len = y_lengths``).  Only the attention mixes positions, so the
        valid positions of the result do not depend on the padding; the padded ones hold whatever the pointwise ops make of
        it -- zeroing them (``ops.mask_tail``) is the caller's part: ``forward`` and ``Transformer`` do it.

        ``cu_seqlens`` / ``max_len`` (``y_cu_seqlens`` / ``y_max_len``: a cross-attention layer's second sequence) make ``x``
        (1, dim, N) a packed batch: int32 device tensors of n_seq + 1 entries and host-known bounds of the sequence lengths, as
        ``ops.attention_alibi_packed`` takes them.  The layer's launches are unchanged but for that op where its attention op
        was.  Not with ``lengths``; fp32, symmetric layers, no active dropout site.  The columns no sequence owns hold what the
        pointwise ops make of them -- ``Transformer.run_packed`` masks them where they can exist.  With all four absent no
        packed op is called."""
        if cu_seqlens is not None or max_len is not None or y_cu_seqlens is not None or y_max_len is not None:
            if lengths is not None or y_lengths is not None:
                raise AgxError("lengths= with cu_seqlens=: a batch is right-padded or packed, not both")
            return self._run_packed_bct(x, residual, keep, y, kv_cache, cu_seqlens, max_len, y_cu_seqlens, y_max_len)
        if lengths is not None or y_lengths is not None:
            if kv_cache is not None:
                raise AgxError("lengths= with a key/value cache: a cached call is causal and takes no lengths")
            self._check_ragged()
            if y_lengths is not None and not self.cross_attention:
                raise AgxError("y_lengths= on a self-attention layer (built without context_y): there is no second sequence")
            lengths = _checked_lengths("lengths", lengths, x.shape[0], x.shape[-1], x.device)
            if y_lengths is not None and y is not None and y.dim() == 3:
                y_lengths = _checked_lengths("y_lengths", y_lengths, y.shape[0], y.shape[-1], y.device)
        if kv_cache is not None and not self.causal:
            raise AgxError("a key/value cache needs a causal self-attention layer (causal=True, no context_y)")
        if self.cross_attention:
            return self._run_cross_bct(x, residual, keep, y, drop, lengths, y_lengths)
        if y is not None:
            raise AgxError("a self-attention layer (built without context_y) takes no second sequence y")
        if x.shape[-1] > self.context:
            raise AgxError(f"sequence length {x.shape[-1]} exceeds the ALiBi context {self.context} "
                           "(the reference fails here too, transformers.py:88-93)")
        if keep is not None and self.dim_head > 128:
            raise AgxError("Transformer: the attention backward kernels cover head_dim <= 128 "
                           "(agx_attention_alibi_backward_ex); larger heads run forward only -- there is no ATen fallback")
        if self.causal:
            return self._run_causal_bct(x, residual, keep, kv_cache)
        p = _active_p(self.dropout)
        if p > 0:
            if self.attention_dtype != "fp32":
                raise AgxError(f"attention with dropout runs in fp32: attention_dtype = {self.attention_dtype!r} has no kernel")
            seed, layer = _site(drop, self)
            xn = _ln(self.norm, x)
            qkv = self._qkv.forward(xn)
            o = ops.attention_alibi_dropout(qkv, None, p=p, seed=seed, stream_id=4 * layer + SITE_PROB, **self._attn())
            if keep is not None:
                keep.update(h=x, xn1=xn, qkv=qkv, o=o)
            return self._drop_out(o, residual, keep, p, seed, layer)
        xn = _ln(self.norm, x)
        qkv = self._qkv.forward(xn)
        bf16 = self.attention_dtype == "bf16" and keep is None
        if lengths is not None:
            o = ops.attention_alibi_ragged(qkv, None, q_len=lengths, k_len=lengths, **self._attn())
        else:
            o = ops.attention_alibi(qkv, precision=ops.ATTN_BF16 if bf16 else ops.ATTN_FP32, **self._attn())
        if keep is not None:
            keep.update(h=x, xn1=xn, qkv=qkv, o=o)
        return self._o.forward(o, EPI_RESIDUAL if residual is not None else 0, residual)

    def backward_bct(self, kept: dict, g: Tensor, want_dy: bool = False, lengths: Optional[Tensor] = None,
                     y_lengths: Optional[Tensor] = None, packed: Optional["_Packed"] = None):
        """``g`` = the gradient of ``run_bct(h, residual=h, keep=kept)`` -> (dh, gradients in ``parameters()`` order, dy).
        ``dy`` is the gradient of a cross-attention layer's second sequence -- the backward-data of the stacked W_k / W_v
        projection, run only when ``want_dy`` -- and None otherwise.  ``lengths`` / ``y_lengths``: the device tensors the
        forward ran with (``attention_alibi_ragged_backward`` in the attention backward's place).  ``packed``: the partition
        of a packed forward (``attention_alibi_packed_backward`` in that place)."""
        d = kept.get("drop")
        d = d if d is not None and d.get("attn") else None      # the forward's (seed, layer, p): its masks are regenerated
        if d is not None:    # the W_o site: the residual branch takes g unmasked (``add=g`` below)
            mask = dict(p=d["attn"], seed=d["seed"], stream_id=4 * d["layer"] + SITE_PROB)
            do, g_o = self._o.backward(kept["o"], ops.dropout_add(g, None, d["attn"], d["seed"], 4 * d["layer"] + SITE_ATTN_OUT))
        else:
            do, g_o = self._o.backward(kept["o"], g)
        if self.cross_attention:
            if d is not None:
                dq, dkv = ops.attention_alibi_dropout_backward(kept["q"], kept["kv"], dout=do, out=kept["o"], **mask, **self._attn())
            elif packed is not None:
                dq, dkv = ops.attention_alibi_packed_backward(kept["q"], kept["kv"], dout=do, out=kept["o"], cu_q=packed.cu,
                                                              max_q=packed.max_len, cu_k=packed.y_cu, max_k=packed.y_max_len,
                                                              **self._attn())
            elif lengths is not None or y_lengths is not None:
                dq, dkv = ops.attention_alibi_ragged_backward(kept["q"], kept["kv"], dout=do, out=kept["o"], q_len=lengths,
                                                              k_len=y_lengths, **self._attn())
            else:
                dq, dkv = ops.attention_alibi_cross_backward(kept["q"], kept["kv"], dout=do, out=kept["o"], **self._attn())
            dxn, g_q = self._q.backward(kept["xn1"], dq)
            dy, g_kv = self._kv.backward(kept["y"], dkv, want_dx=want_dy)
            dh, dweight, dbias = _ln_bwd(self.norm, kept["h"], dxn, add=g)
            return dh, [dweight, dbias] + g_q + g_kv + g_o, dy
        if d is not None:
            dqkv = ops.attention_alibi_dropout_backward(kept["qkv"], None, dout=do, out=kept["o"], **mask, **self._attn())
        elif self.window is not None:
            dqkv = ops.attention_alibi_window_backward(kept["qkv"], out=kept["o"], dout=do, window=self.window, **self._attn())
        elif self.causal:
            dqkv = ops.attention_alibi_causal_backward(kept["qkv"], out=kept["o"], dout=do, **self._attn())
        elif packed is not None:
            dqkv = ops.attention_alibi_packed_backward(kept["qkv"], None, dout=do, out=kept["o"], cu_q=packed.cu,
                                                       max_q=packed.max_len, **self._attn())
        elif lengths is not None:
            dqkv = ops.attention_alibi_ragged_backward(kept["qkv"], None, dout=do, out=kept["o"], q_len=lengths, k_len=lengths,
                                                       **self._attn())
        else:
            dqkv = ops.attention_alibi_backward(kept["qkv"], dout=do, out=kept["o"], **self._attn())
        dxn, g_qkv = self._qkv.backward(kept["xn1"], dqkv)
        dh, dweight, dbias = _ln_bwd(self.norm, kept["h"], dxn, add=g)
        return dh, [dweight, dbias] + g_qkv + g_o, None

    def forward(self, x: Tensor, y=None, *, lengths=None, y_lengths=None) -> Tensor:
        """Reference layout: (B, T, dim) [, (B, Ty, dim)] -> (B, T, dim).  With ``lengths`` / ``y_lengths`` (``run_bct``) the
        padded tails of the inputs are zeroed first and the padded tail of the result after: exactly 0 there."""
        y = None if y is None else y.transpose(1, 2).contiguous()
        x = x.transpose(1, 2).contiguous()
        if lengths is None and y_lengths is None:
            return self.run_bct(x, y=y).transpose(1, 2).contiguous()
        self._check_ragged()
        if y_lengths is not None and (not self.cross_attention or y is None):
            raise AgxError("y_lengths= on a self-attention layer (built without context_y): there is no second sequence")
        lengths = _checked_lengths("lengths", lengths, x.shape[0], x.shape[-1], x.device)
        if y_lengths is not None:
            y_lengths = _checked_lengths("y_lengths", y_lengths, y.shape[0], y.shape[-1], y.device)
            y = ops.mask_tail(y, y_lengths)               # out of place: the caller's tensor is not modified
        if lengths is not None:
            x = ops.mask_tail(x, lengths)
        out = self.run_bct(x, y=y, lengths=lengths, y_lengths=y_lengths)
        if lengths is not None:
            ops.mask_tail(out, lengths, out=out)
        return out.transpose(1, 2).contiguous()


class FeedForward(nn.Module):
    """transformers.py:193-223: LN -> Linear -> activation -> Linear.  ``nn.GELU`` (exact) is fused into the FFN-in conv's epilogue;
    ``nn.SiLU`` -- what ``ConformerBlock`` passes -- runs FFN-in with epilogue 0 and the stand-alone ``agx_silu`` behind it."""

    def __init__(self, dim, hidden_dim, dropout=0., activation=nn.GELU):
        super().__init__()
        if activation is not nn.GELU and activation is not nn.SiLU:
            raise NotImplementedError("only GELU (fused into the FFN kernel epilogue) and SiLU (one element-wise kernel) have kernels")
        self.silu = activation is nn.SiLU
        self.net = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, hidden_dim), activation(), nn.Dropout(dropout),
                                 nn.Linear(hidden_dim, dim), nn.Dropout(dropout))
        self._l1, self._l2 = _PackedLinear(self.net[1]), _PackedLinear(self.net[4])
        self._l2_scaled = {}      # scale -> FFN-out with the scale folded into its image (``run_bct``: ``scale``)
        self.last_dropout_seed = None

    def _out(self, scale: float) -> _PackedLinear:
        if scale == 1.0:
            return self._l2
        if scale not in self._l2_scaled:
            self._l2_scaled[scale] = _PackedLinear(self.net[4], scale=scale)
        return self._l2_scaled[scale]

    def run_bct(self, x: Tensor, residual: Optional[Tensor] = None, keep: Optional[dict] = None,
                drop: Optional[tuple] = None, scale: float = 1.0) -> Tensor:
        """In training mode with ``dropout > 0`` the hidden tensor is dropped in place behind the activation (``net[3]``) and
        the FFN-out result before the residual add (``net[5]``: the conv runs without its fused residual, then
        ``dropout_add(., residual)``); otherwise the two launches it always was (SiLU: three).  ``scale`` (a power of two)
        multiplies the result before the residual add, folded into FFN-out's packed image: no launch."""
        p_hid, p_out = _active_p(self.net[3]), _active_p(self.net[5])
        l2 = self._out(scale)
        xn = _ln(self.net[0], x)
        if self.silu:
            pre = self._l1.forward(xn)
            hid = ops.silu(pre, out=None if keep is not None else pre)      # the backward reads the pre-activation
        else:
            hid = self._l1.forward(xn, EPI_GELU_PRE)
        if p_hid > 0 or p_out > 0:
            seed, layer = _site(drop, self)
            if keep is not None:
                keep.setdefault("drop", dict(seed=seed, layer=layer)).update(hid=p_hid, out=p_out)
        if p_hid > 0:
            ops.dropout_add(hid, None, p_hid, seed, 4 * layer + SITE_FFN_HIDDEN, out=hid)
        if keep is not None:
            keep.update(x1=x, xn2=xn, hid=hid)     # with dropout: the masked hidden tensor, FFN-out's input
            if self.silu:
                keep.update(pre=pre)
        if p_out > 0:
            out = l2.forward(hid)
            return ops.dropout_add(out, residual, p_out, seed, 4 * layer + SITE_FFN_OUT, out=out)
        return l2.forward(hid, EPI_RESIDUAL if residual is not None else 0, residual)

    def backward_bct(self, kept: dict, g: Tensor, scale: float = 1.0):
        """As ``Attention.backward_bct``; the GELU gradient sits in the FFN-out bwd-data epilogue, at the pre-activation,
        which is recomputed with one conv launch: the forward's FFN-in projection with epilogue 0.  SiLU: the plain k = 1
        backward of FFN-out, then ``agx_silu_backward`` in place at the saved pre-activation."""
        d = kept.get("drop") or {}
        g_out = g        # the FFN-out site: the residual branch takes g unmasked (``add=g`` below)
        if d.get("out"):
            g_out = ops.dropout_add(g, None, d["out"], d["seed"], 4 * d["layer"] + SITE_FFN_OUT)
        if self.silu:
            dpre, g2 = self._out(scale).backward(kept["hid"], g_out)
        else:
            pre = self._l1.forward(kept["xn2"])
            dpre, g2 = self._out(scale).backward(kept["hid"], g_out, pre=pre)
        if d.get("hid"):     # d hid~ -> d pre: mask * scale and the activation's gradient commute
            ops.dropout_add(dpre, None, d["hid"], d["seed"], 4 * d["layer"] + SITE_FFN_HIDDEN, out=dpre)
        if self.silu:
            ops.silu_backward(kept["pre"], dpre, out=dpre)
        dxn, g1 = self._l1.backward(kept["xn2"], dpre)
        dx1, dweight, dbias = _ln_bwd(self.net[0], kept["x1"], dxn, add=g)
        return dx1, [dweight, dbias] + g1 + g2

    def forward(self, x: Tensor) -> Tensor:
        return self.run_bct(x.transpose(1, 2).contiguous()).transpose(1, 2).contiguous()


class _TransformerNative(torch.autograd.Function):
    """Transformer forward + hand-written backward on the HIP kernels: k=1 conv backward for every Linear,
    ``agx_attention_alibi_backward`` / ``agx_attention_alibi_cross_backward``, ``agx_layernorm_ct_backward`` (residual
    adds fused as ``add``), the GELU gradient in a bwd-data epilogue; the dropout masks of a training-mode forward are
    regenerated from the seed saved in the context (``agx_attention_alibi_dropout_backward``, ``agx_dropout_add``).
    Every layer, the first included, computes its input gradient; ``y`` (None without cross-attention) is a differentiable
    input too: its gradient is the backward-data of the cross layer's stacked W_k / W_v projection.

    ``lens`` = (lengths, y_lengths), the checked device tensors of a ragged call (``Transformer.run_bct``), or None: they
    travel in the context as non-differentiable values.  The backward masks the incoming gradient's tail first
    (``mask_tail``, out of place), then walks as usual with ``attention_alibi_ragged_backward``: every tensor the forward
    kept is finite at padded positions and every gradient there exactly 0, so the padding contributes exactly 0 to every
    parameter gradient and ``dx`` / ``dy`` come out exactly 0 there.

    ``lens`` may instead be the ``_Packed`` partition of ``Transformer.run_packed``, carried the same way: the backward zeroes
    the slack columns of the incoming gradient once (one ``mask_tail`` of the one packed row at ``cu_seqlens[-1]``, and only
    where slack can exist), then walks as usual with ``attention_alibi_packed_backward``; the same argument keeps the slack
    out of every parameter gradient."""

    @staticmethod
    def forward(ctx, tf, lens, x: Tensor, y: Optional[Tensor], *params: Tensor):
        keep = []
        ctx.packed = lens if isinstance(lens, _Packed) else None
        ctx.lens = lens = None if ctx.packed is not None else lens
        with torch.no_grad():
            out = tf._hip_bct(x.detach(), keep, None if y is None else y.detach(), lens=lens, packed=ctx.packed)
        ctx.drop = [kept.pop("drop", None) for kept in keep]     # per layer: the seed, layer and probabilities of its masks
        ctx.tf, ctx.names = tf, [(li, name) for li, kept in enumerate(keep) for name in kept]
        ctx.save_for_backward(*[t for kept in keep for t in kept.values()])
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        keep = [{"drop": d} for d in ctx.drop]
        for (li, name), t in zip(ctx.names, ctx.saved_tensors):
            keep[li][name] = t
        g, grads, gy = g.contiguous(), [], None
        lengths, y_lengths = ctx.lens if ctx.lens is not None else (None, None)
        if lengths is not None:
            g = ops.mask_tail(g, lengths)                   # the backward of the block's last op
        if ctx.packed is not None and ctx.packed.slack:
            g = ops.mask_tail(g, ctx.packed.cu[-1:])        # likewise: the one packed row ends at cu_seqlens[-1]
        for (attention, ff), kept in zip(reversed(ctx.tf.layers), reversed(keep)):
            g, g_ff = ff.backward_bct(kept, g)              # x2 = x1 + W2 gelu(W1 LN2(x1) + b1) + b2
            # x1 = h + W_o attn(W_qkv LN1(h))  (cross: W_q LN1(h), W_kv y -- dy only when y asks for a gradient)
            if ctx.packed is not None:
                g, g_attention, dy = attention.backward_bct(kept, g, want_dy=ctx.needs_input_grad[3], packed=ctx.packed)
            elif ctx.lens is None:
                g, g_attention, dy = attention.backward_bct(kept, g, want_dy=ctx.needs_input_grad[3])
            else:
                g, g_attention, dy = attention.backward_bct(kept, g, want_dy=ctx.needs_input_grad[3], lengths=lengths,
                                                            y_lengths=y_lengths if attention.cross_attention else None)
            grads = g_attention + g_ff + grads              # the order of Transformer.parameters()
            gy = dy if attention.cross_attention else gy
        return (None, None, g if ctx.needs_input_grad[2] else None, gy, *grads)


def _layer_kv(kv, layer: int) -> Tensor:
    return kv[layer] if isinstance(kv, list) else kv      # a Transformer keeps one buffer per layer, a ConformerBlock its one


class _HostCache:
    """A key/value cache whose ``length`` -- the frames every row holds -- is one host integer.  ``state``: further per-row state
    tensors that ``reset`` zeroes (none for a Transformer, the conv state for a ConformerBlock)."""

    def __init__(self, kv, batch: int, capacity: int, window: Optional[int] = None, state: tuple = ()):
        self.kv, self.batch, self.capacity, self.length, self.window, self._state = kv, batch, capacity, 0, window, state

    def reset(self) -> None:
        self.length = 0
        for t in self._state:
            t.zero_()

    def kv_cache(self, layer: int = 0, counts=None) -> tuple:
        """The ``kv_cache=`` of layer ``layer``'s attention call (``Attention._run_causal_bct``)."""
        return _layer_kv(self.kv, layer), self.length

    def advance(self, n: int, counts=None) -> None:
        self.length += n


class _StreamCache:
    """A ring key/value cache whose positions live in device memory: ``pos``, int64 (B,), one per batch row, read by the kernels
    and advanced by a kernel.  ``state``: as in ``_HostCache``."""

    def __init__(self, kv, pos: Tensor, capacity: int, window: int, max_chunk: int, state: tuple = ()):
        self.kv, self.pos, self.batch, self.capacity, self.window, self.max_chunk = kv, pos, pos.numel(), capacity, window, max_chunk
        self._state = state

    def reset(self, rows=None) -> None:
        """Zero the positions (and the per-row state) of ``rows`` (default: every row) with device fills: those rows start a new
        stream at their next call; what their ring columns hold is never read again.  Call it between steps, outside any
        captured graph."""
        for sel in ops._row_slices("reset", rows, self.batch, "cache"):
            for t in (self.pos, *self._state):
                t[sel].zero_()

    def positions(self) -> list:
        """The positions as a list of ints.  Synchronises: for tests and debugging, never called in the walk."""
        return self.pos.tolist()

    def kv_cache(self, layer: int = 0, counts: Optional[Tensor] = None) -> tuple:
        """The ``kv_cache=`` of layer ``layer``'s attention call (``Attention._run_causal_bct``); ``counts``: the counted step."""
        return _layer_kv(self.kv, layer), self.pos, counts

    def advance(self, n: int, counts: Optional[Tensor] = None) -> None:
        ops.stream_advance(self.pos, n, counts=counts)       # once per call: every layer read the same positions


class TransformerCache(_HostCache):
    """The key/value cache of a causal ``Transformer`` (``Transformer.new_cache``): per layer one fp32
    (B, 2*H*Dh, capacity) buffer, K rows first, then V rows -- the kv layout of ``agx_attention_alibi_causal`` with
    ``kv_row_stride = capacity`` -- and one ``length``, the frames every layer holds.  The buffers come from ``torch.empty``
    and are never cleared: the kernel reads nothing at or beyond column ``length`` of a row.

    On a windowed Transformer (``window`` is its window) every buffer is a ring: frame ``p`` lives in column ``p mod capacity``,
    ``length`` keeps counting (a Python int: no 32-bit limit) and the kernel reads no column outside a workgroup's window."""


class ConformerCache(_HostCache):
    """The cache of a causal ``ConformerBlock`` (``ConformerBlock.new_cache``): ``kv``, the attention's fp32
    (B, 2*H*Dh, capacity) key/value buffer with one ``length`` as ``TransformerCache`` has them -- a ring on a windowed block --,
    and ``conv_state``, the conv block's (B, C, K - 1) post-GLU history (zeros: the start of a stream), which ``reset`` zeroes."""

    def __init__(self, kv: Tensor, batch: int, capacity: int, window: Optional[int], conv_state: Tensor):
        super().__init__(kv, batch, capacity, window, (conv_state,))
        self.conv_state = conv_state


def _checked_counts(what: str, counts, cache, stream_type, host_type) -> Tensor:
    """The refusals of ``counts=`` on a cached call, before any op: the cache's kind here, the tensor in ``ops._checked_counts``."""
    if cache is None:
        raise AgxError(f"{what}: counts= without cache=: a per-row frame count belongs to a cached step on a stream cache "
                       "(new_stream_cache)")
    if isinstance(cache, host_type):
        raise AgxError(f"{what}: counts= with a {host_type.__name__}: its length is one host integer for the whole batch; per-row "
                       f"counts need the device-held positions of a {stream_type.__name__} (new_stream_cache)")
    if not isinstance(cache, stream_type):
        raise AgxError(f"{what}: counts= needs a {stream_type.__name__} (new_stream_cache), got {type(cache).__name__}")
    return ops._checked_counts(what, counts, cache.batch, cache.pos.device, on="the cache on")


class TransformerStreamCache(_StreamCache):
    """The ring key/value cache of a windowed causal ``Transformer`` with the positions in device memory, one per batch row
    (``Transformer.new_stream_cache``): per layer one fp32 (B, 2*H*Dh, capacity) ring from ``torch.empty``, never cleared, and
    ``pos``, an int64 (B,) device tensor of the frames every row has consumed.  The kernels read ``pos`` (``ops.ring_write_pos``,
    ``ops.attention_alibi_stream``) and a kernel advances it (``ops.stream_advance``): a cached step makes no host decision that
    depends on the position, so it can be captured once and replayed for ever, and every row has an age of its own --
    ``reset(rows=[r])`` hands row ``r`` to a new stream while the others go on.

    The host does not know the positions, so a call of ``n`` frames is bounded by the worst case over all of them,
    ``n <= max_chunk = min(capacity - window + 1, context_x)``: stricter than ``TransformerCache`` at the start of a stream, where
    ``n + min(window - 1, length) <= capacity`` lets the first call fill the whole ring."""


class ConformerStreamCache(_StreamCache):
    """The cache of a windowed causal ``ConformerBlock`` with the positions in device memory (``ConformerBlock.new_stream_cache``):
    the ring ``kv`` and the int64 (B,) ``pos`` of ``TransformerStreamCache``, ``max_chunk`` as there, and ``conv_state``
    (B, C, K - 1), whose rows ``reset`` zeroes with the positions.  The conv state holds values, not positions: the step kernel
    shifts it by the call's frames whatever the row's age, so a cached step makes no host decision and every row is a stream of
    its own."""

    def __init__(self, kv: Tensor, pos: Tensor, capacity: int, window: int, max_chunk: int, conv_state: Tensor):
        super().__init__(kv, pos, capacity, window, max_chunk, (conv_state,))
        self.conv_state = conv_state


def _new_kv(what: str, model, inner_dims: list, batch: int, capacity: Optional[int]) -> tuple:
    """The buffers of ``new_cache`` / ``new_stream_cache``: one empty fp32 (B, 2*H*Dh, capacity) per entry of ``inner_dims`` on the
    parameters' device, ``capacity`` (default ``context_x``; a ring holds at least the window), and ``max_chunk``, the frames a
    call on device-held positions may take: the worst case over every position (None without a window)."""
    capacity = model.context_x if capacity is None else int(capacity)
    if batch < 1 or capacity < 1:
        raise AgxError(f"{what}: batch = {batch}, capacity = {capacity}")
    if model.window is not None and capacity < model.window:
        raise AgxError(f"{what}: a ring of capacity = {capacity} cannot hold a window of {model.window} frames")
    device = next(model.parameters()).device
    kv = [torch.empty((batch, 2 * d, capacity), dtype=torch.float32, device=device) for d in inner_dims]
    return kv, capacity, None if model.window is None else min(capacity - model.window + 1, model.context_x)


def _check_cached_call(model, this: str, x: Tensor, cache, on_device: bool, dim: Optional[int] = None) -> None:
    """The refusals a cached call of a ``Transformer`` or a ``ConformerBlock`` (``this``) shares, before any op and without reading
    a position: no gradient, no active dropout, the batch, the window, and the frames the cache can take -- on device-held
    positions ``max_chunk``, the worst case; on a host ring what the first new query still sees; on a linear buffer its end.
    ``dim``: a ConformerBlock's, the strict caller -- it also checks its ``dim``, and on a host cache it refuses ``n < 1`` and a
    window other than its own even where it has none; a Transformer does neither (its attention layer's own check follows,
    still before any op)."""
    strict = dim is not None
    if needs_grad(x, model):
        raise AgxError("there is no backward through a cached call: run it under torch.no_grad()")
    if model._dropout_active():
        raise AgxError("a cached call with an active dropout site (training mode, dropout > 0) has no kernel")
    if x.dim() != 3 or x.shape[0] != cache.batch or (strict and x.shape[1] != dim):
        raise AgxError(f"cached call: x is {tuple(x.shape)}, the cache was made for batch {cache.batch}"
                       + (f" of a block of dim {dim}" if strict else ""))
    if (strict or on_device or model.window is not None) and cache.window != model.window:
        raise AgxError(f"the cache was made for window {cache.window}, {this} has window {model.window}")
    n, least = x.shape[-1], 1 if strict else 0
    if on_device:
        if n < 1 or n > cache.max_chunk:
            raise AgxError(f"stream cache: a call takes 1 <= n <= max_chunk = {cache.max_chunk} frames (min(capacity {cache.capacity} "
                           f"- window {model.window} + 1, context_x {model.context_x}): the worst case over every position), got {n}")
    elif model.window is not None:       # a ring: the new frames must not overwrite what their first query still sees
        behind = min(model.window - 1, cache.length)
        if n < least or n + behind > cache.capacity:
            raise AgxError(f"cached call: {n} new frames + the {behind} cached frames their window reaches exceed the ring's "
                           f"capacity {cache.capacity}")
    elif n < least or cache.length + n > min(cache.capacity, model.context_x):
        raise AgxError(f"cached call: {cache.length} cached + {n} new frames exceed min(capacity {cache.capacity}, context_x "
                       f"{model.context_x}) = {min(cache.capacity, model.context_x)}")


class Transformer(nn.Module):
    """transformers.py:225-279: ``x += attn(x); x += ff(x)`` per layer.  ``causal=True`` (build-defined): every layer is
    causal self-attention, and ``new_cache`` / ``run_bct(x, cache=)`` run the block incrementally.  ``window=W`` (with
    ``causal=True``, 1 <= W <= context_x): every query sees its last W keys, the cache is a ring and a stream has no end."""

    def __init__(self, dim, depth=1, heads=8, head_dim=64, dropout=0., context_x=32, context_y=None,
                 has_pos_emb=True, alibi=True, causal=False, window=None):
        super().__init__()
        if causal and context_y is not None:
            raise ValueError("causal=True with context_y: causal cross-attention is not defined (cross-attention stays symmetric)")
        self.causal, self.context_x = bool(causal), context_x
        self.window = _checked_window(window, causal, context_x)
        self.cross_attention = context_y is not None     # :253-256
        self.layers = nn.ModuleList([
            nn.ModuleList([Attention(dim, n_heads=heads, dim_head=head_dim, dropout=dropout, context_x=context_x,
                                     context_y=context_y if i == 0 else None,     # :272-273: the first layer only
                                     has_pos_emb=has_pos_emb, alibi=alibi, causal=causal, window=window),
                           FeedForward(dim, dim, dropout=dropout)])
            for i in range(depth)])
        self.last_dropout_seed = None     # the mask seed of the last training-mode forward with dropout > 0

    def _dropout_active(self) -> bool:
        return any(m.training and m.p > 0 for a, f in self.layers for m in (a.dropout, f.net[3], f.net[5]))

    def new_cache(self, batch: int, capacity: Optional[int] = None) -> TransformerCache:
        """An empty key/value cache for ``batch`` sequences of up to ``capacity`` frames (default ``context_x``), on the
        parameters' device.  No memset: see ``TransformerCache``.  On a windowed Transformer the cache is a ring of
        ``capacity >= window`` columns: a call of ``n`` frames needs ``n + min(window - 1, cache.length) <= capacity`` -- the
        new frames must not overwrite a cached frame their first query still sees -- and the stream has no end."""
        if not self.causal or self.cross_attention:
            raise AgxError("new_cache: a key/value cache needs a causal self-attention Transformer (causal=True, no context_y)")
        kv, capacity, _ = _new_kv("new_cache", self, [a.inner_dim for a, _ in self.layers], batch, capacity)
        return TransformerCache(kv, batch, capacity, self.window)

    def new_stream_cache(self, batch: int, capacity: Optional[int] = None) -> "TransformerStreamCache":
        """An empty ring cache for ``batch`` live streams with the positions in device memory (``TransformerStreamCache``), on the
        parameters' device: ``capacity`` columns per row (default ``context_x``, at least ``window``), every position 0.  Needs a
        windowed causal self-attention Transformer.  A call takes ``1 <= n <= cache.max_chunk`` frames."""
        if not self.causal or self.cross_attention or self.window is None:
            raise AgxError("new_stream_cache: device-held positions need a windowed causal self-attention Transformer "
                           "(causal=True, window=W, no context_y)")
        kv, capacity, max_chunk = _new_kv("new_stream_cache", self, [a.inner_dim for a, _ in self.layers], batch, capacity)
        pos = torch.zeros(batch, dtype=torch.int64, device=kv[0].device)
        return TransformerStreamCache(kv, pos, capacity, self.window, max_chunk)

    def _check_cache(self, x: Tensor, cache) -> None:
        """The refusals of a cached call, before any op; on a stream cache none of them reads a position."""
        on_device = isinstance(cache, TransformerStreamCache)
        if not self.causal or self.cross_attention or (on_device and self.window is None):
            raise AgxError("a stream cache needs a windowed causal self-attention Transformer (causal=True, window=W, no context_y)"
                           if on_device else "a key/value cache needs a causal self-attention Transformer (causal=True, no context_y)")
        _check_cached_call(self, "this Transformer", x, cache, on_device)
        if on_device:       # on a host cache the attention layer itself refuses it, still before any op
            for attention, _ in self.layers:
                if attention.attention_dtype != "fp32":
                    raise AgxError(f"causal attention runs in fp32: attention_dtype = {attention.attention_dtype!r} has no kernel")
        if len(cache.kv) != len(self.layers):
            raise AgxError(f"the cache holds {len(cache.kv)} layers, this Transformer has {len(self.layers)}")

    def _check_lengths(self, x: Tensor, y: Optional[Tensor], cache, lengths, y_lengths) -> tuple:
        """The refusals of a ragged call, before any op, and its (lengths, y_lengths) as checked device tensors."""
        if cache is not None:
            raise AgxError("lengths= with cache=: a cached call is causal, and a causal layer's valid frames never see right "
                           "padding -- run it without lengths")
        for attention, _ in self.layers:
            attention._check_ragged()
        if self._dropout_active():
            raise AgxError("lengths= with an active dropout site (training mode, dropout > 0): dropout on ragged batches has "
                           "no kernel (eval mode runs)")
        if y_lengths is not None and not self.cross_attention:
            raise AgxError("y_lengths= on a Transformer without a cross-attention layer (built without context_y)")
        if x.dim() != 3:
            raise AgxError(f"lengths=: x is {tuple(x.shape)}, expected (B, dim, T)")
        lengths = _checked_lengths("lengths", lengths, x.shape[0], x.shape[-1], x.device)
        if y_lengths is not None:
            if y is None or y.dim() != 3:
                raise AgxError("y_lengths= without a second sequence y of shape (B, dim, Ty)")
            y_lengths = _checked_lengths("y_lengths", y_lengths, y.shape[0], y.shape[-1], y.device)
        return lengths, y_lengths

    def _hip_bct(self, x: Tensor, keep: Optional[list] = None, y: Optional[Tensor] = None,
                 cache=None, lens: Optional[tuple] = None, packed: Optional[_Packed] = None, counts: Optional[Tensor] = None) -> Tensor:
        """The one forward walk, LN1 -> QKV -> attention -> W_o (+res) -> LN2 -> FFN-in (GELU) -> FFN-out (+res) per layer:
        7 launches, both residual adds fused into the W_o / FFN-out conv epilogues (a cross-attention layer: 8, a Q and a
        KV projection in place of the QKV one).  ``keep``: the training forward
        (``Attention.run_bct``) -- the list receives one dict of named intermediates per layer.

        Training mode with ``dropout > 0``: LN1 -> QKV -> attention with dropout on the probabilities -> W_o -> dropout + res ->
        LN2 -> FFN-in (GELU) -> dropout in place -> FFN-out -> dropout + res: 10 launches (a cross-attention layer: 11).  The
        four masks of layer ``l`` have the stream ids ``4 l + {0: probabilities, 1: attention output, 2: FFN hidden, 3: FFN
        output}`` under one 64-bit seed per call, drawn on the CPU from torch's default generator (``torch.manual_seed``
        reproduces a run) and kept as ``last_dropout_seed``.  The seed travels to the kernels by value: a captured graph
        (``torch.cuda.graph``) replays the one mask it was captured with -- capture-safe seeds are not provided.  In eval mode
        or with ``dropout == 0`` nothing changes: the same 7 (8) launches, no seed is drawn.

        ``causal``: the same 7 launches with ``attention_alibi_causal`` in place of ``attention_alibi``; fp32, and refused in
        training mode with ``dropout > 0``.  With ``cache`` the ``n`` frames of ``x`` continue the cached sequence: per layer
        LN1 -> QKV of the n frames -> their K / V rows copied behind the cached ones -> attention from position
        ``cache.length`` over ``cache.length + n`` keys -> W_o (+res) -> FFN; ``cache.length`` advances after the last layer.

        ``window``: the causal walk with ``attention_alibi_window`` / ``attention_alibi_window_backward`` in place of the causal
        ops and the same refusals; with ``cache`` the K / V rows go into a ring (``Attention._run_causal_bct``).

        A ``TransformerStreamCache`` walks the same steps and differs at three places: the ring write is ``ops.ring_write_pos``,
        the attention op is ``ops.attention_alibi_stream`` (both read every row's position from ``cache.pos``) and the advance is
        ``ops.stream_advance`` -- 8 launches per layer and one advance per call, no host read of a position, no allocation but
        the ops' outputs, one stream: the step can be captured (``torch.cuda.graph``) as a linear chain.

        ``lens`` = (lengths, y_lengths) (``_check_lengths``; either may be None = every row is full), a right-padded ragged
        batch: ``x0 = mask_tail(x, lengths)`` and ``y0 = mask_tail(y, y_lengths)`` out of place (the caller's tensors are not
        modified), then per layer the unchanged launches with ``attention_alibi_ragged`` where the attention op was
        (self-attention: ``q_len = k_len = lengths``; the cross layer: ``q_len = lengths``, ``k_len = y_lengths``), then
        ``mask_tail`` in place on the block's output: two more launches per call (three with ``y_lengths``).  Every other op
        is pointwise in time, so the output at valid positions does not depend on what the padding held (NaN included: the
        masked inputs are finite) and is exactly 0 at padded ones.  ``lens=None``: no new op is called.

        ``packed`` (``_check_packed``): ``x`` (1, dim, N) and ``y`` (1, dim, Ny) hold the sequences back to back.  The walk is
        the plain one, 7 launches per layer (8 for the cross layer), with ``attention_alibi_packed`` where the attention op
        was (``cu_q = cu_k = packed.cu``; the cross layer: ``cu_k = packed.y_cu``): nothing else mixes columns, and a
        partition the host validated to end at N leaves no column without an owner, so there is nothing to mask.  Where
        slack columns can exist -- a device ``cu_seqlens``, which the host does not read, or a host one that ends before N --
        they are masked exactly as the padded tails above: ``mask_tail`` of the one packed row at ``cu[-1]``, out of place on
        ``x`` (and on ``y`` likewise), in place on the output, so the output is exactly 0 there, the kept tensors are finite
        and NaN in the slack changes nothing.  ``packed=None``: no packed op is called.

        ``counts`` (``_checked_counts``; a stream cache only): row ``b`` takes the first ``clamp(counts[b], 0, n)`` frames of
        ``x``.  ``x0 = mask_tail(x, counts=)`` out of place, then per layer the stream-cache launches with the
        counted ring write, the counted advance, and ``mask_tail`` in place on the output: two more launches per call, and the
        contract of the padded tails above -- valid frames bit for bit those of an uncounted call on them, exact 0 behind the
        count, NaN there harmless.  ``counts=None``: no counted op is called."""
        lengths, y_lengths = lens if lens is not None else (None, None)
        if (y is not None) != self.cross_attention:
            raise AgxError("Cross attention requires two inputs: this Transformer was built with context_y and got no y"
                           if y is None else "this Transformer was built without context_y and takes no second sequence y")
        if self.causal and self._dropout_active():
            raise AgxError("a causal Transformer with dropout > 0 in training mode has no kernel (eval mode runs)")
        seed = None
        if self._dropout_active():
            seed = self.last_dropout_seed = ops.draw_dropout_seed()
        if lengths is not None:
            x = ops.mask_tail(x, lengths)
        if y_lengths is not None:
            y = ops.mask_tail(y, y_lengths)
        if counts is not None:
            x = ops.mask_tail(x, None, counts=counts)
        if packed is not None and packed.slack:
            x = ops.mask_tail(x, packed.cu[-1:])
        if packed is not None and packed.y_slack:
            y = ops.mask_tail(y, packed.y_cu[-1:])
        for li, (attention, ff) in enumerate(self.layers):
            kept = None if keep is None else {}
            drop = None if seed is None else (seed, li)
            if cache is not None:
                x = attention.run_bct(x, x, kept, None, drop, kv_cache=cache.kv_cache(li, counts))
            elif packed is not None:
                x = attention.run_bct(x, x, kept, y if attention.cross_attention else None, drop,
                                      **packed.attn_args(attention.cross_attention))
            elif lens is not None:
                x = attention.run_bct(x, x, kept, y if attention.cross_attention else None, drop, lengths=lengths,
                                      y_lengths=y_lengths if attention.cross_attention else None)
            else:
                x = attention.run_bct(x, x, kept, y if attention.cross_attention else None, drop)
            x = ff.run_bct(x, x, kept, drop)
            if keep is not None:
                keep.append(kept)
        if cache is not None:
            cache.advance(x.shape[-1], counts)
        if lengths is not None:
            x = ops.mask_tail(x, lengths, out=x)
        if counts is not None:
            x = ops.mask_tail(x, None, out=x, counts=counts)
        if packed is not None and packed.slack:
            x = ops.mask_tail(x, packed.cu[-1:], out=x)
        return x

    def _check_packed(self, x: Tensor, cu_seqlens, max_len, y: Optional[Tensor], y_cu_seqlens, y_max_len) -> _Packed:
        """The refusals of a packed call, before any op, and its partition as checked device tensors."""
        if self.causal:
            raise AgxError("run_packed on a causal" + (" (windowed)" if self.window is not None else "") + " Transformer: packed "
                           "attention is symmetric, causal and windowed packed calls have no kernel")
        if self._dropout_active():
            raise AgxError("run_packed with an active dropout site (training mode, dropout > 0): dropout on packed batches has "
                           "no kernel (eval mode runs)")
        for attention, _ in self.layers:
            attention._check_packed()
        if y_cu_seqlens is not None and not self.cross_attention:
            raise AgxError("y_cu_seqlens= on a Transformer without a cross-attention layer (built without context_y)")
        if self.cross_attention and (y is None or y_cu_seqlens is None):
            raise AgxError("run_packed on a Transformer with a cross-attention layer (built with context_y) needs y and "
                           "y_cu_seqlens, the packed second sequence and its partition")
        if y is not None and not self.cross_attention:
            raise AgxError("this Transformer was built without context_y and takes no second sequence y")
        dim = self.layers[0][0].dim
        if x.dim() != 3 or x.shape[0] != 1 or x.shape[1] != dim:
            raise AgxError(f"run_packed: x is {tuple(x.shape)}, expected (1, {dim}, N): a packed batch is one row")
        cu, max_len, slack = _checked_cu("cu_seqlens", cu_seqlens, x.shape[-1], max_len, x.device)
        if not self.cross_attention:
            if max_len > self.context_x:
                raise AgxError(f"run_packed: sequences of up to max_len = {max_len} frames exceed context_x = {self.context_x}")
            return _Packed(cu, max_len, slack)
        if y.dim() != 3 or y.shape[0] != 1 or y.shape[1] != dim:
            raise AgxError(f"run_packed: y is {tuple(y.shape)}, expected (1, {dim}, Ny): a packed batch is one row")
        y_cu, y_max_len, y_slack = _checked_cu("y_cu_seqlens", y_cu_seqlens, y.shape[-1], y_max_len, y.device)
        if y_cu.numel() != cu.numel():
            raise AgxError(f"run_packed: x has {cu.numel() - 1} sequences and y has {y_cu.numel() - 1}: sequence s of x attends to "
                           "sequence s of y")
        cx, cy = self.context_x, self.layers[0][0].alibi_obj.context_y
        if not ((max_len <= cx and y_max_len <= cy) or (max_len <= cy and y_max_len <= cx)) or (len(self.layers) > 1 and max_len > cx):
            raise AgxError(f"run_packed: sequences of up to ({max_len}, {y_max_len}) frames exceed the ALiBi contexts ({cx}, {cy}) "
                           "in both orders, or context_x in the self-attention layers")
        return _Packed(cu, max_len, slack, y_cu, y_max_len, y_slack)

    def run_packed(self, x: Tensor, cu_seqlens, max_len: Optional[int] = None, y: Optional[Tensor] = None, y_cu_seqlens=None,
                   y_max_len: Optional[int] = None, cache=None) -> Tensor:
        """A ragged batch without its padding: ``x`` (1, dim, N) holds the sequences back to back, channel-major, and sequence
        ``s`` owns the columns ``[cu_seqlens[s], cu_seqlens[s+1])``; (1, dim, N) comes back, exactly 0 in the columns behind
        ``cu_seqlens[-1]``.  ``y`` (1, dim, Ny) with ``y_cu_seqlens`` is the cross-attention layer's second sequence, packed
        the same way, un-normalised as ever; sequence ``s`` of ``x`` attends to sequence ``s`` of ``y``.  Every sequence
        comes out as ``run_bct`` computes it alone (``_hip_bct``: the walk).  With autograd on, the backward runs on the HIP
        kernels too.

        A Python sequence or a CPU integer tensor is validated on the host -- it starts at 0, never decreases, ends at or
        before N, no sequence exceeds ``context_x`` (with ``y``: the two-order rule of the cross layer) -- and ``max_len`` is
        derived from it.  A device integer tensor is used without a sync and clamped by the kernels -- the form to pass
        under graph capture -- and ``max_len`` (``y_max_len``), a bound of the sequence lengths, is then required.  Refused,
        before any op: a causal or windowed Transformer, ``cache=``, an active dropout site, ``attention_dtype = "bf16"``,
        ``y_cu_seqlens`` without a cross-attention layer or such a layer without it, a device ``cu_seqlens`` without
        ``max_len``, ``x`` not (1, dim, N), a count of sequences that differs between ``x`` and ``y``."""
        if cache is not None:
            raise AgxError("run_packed with cache=: a cached call is causal and packed attention is symmetric")
        packed = self._check_packed(x, cu_seqlens, max_len, y, y_cu_seqlens, y_max_len)
        if needs_grad(x, self) or (y is not None and torch.is_grad_enabled() and y.requires_grad):
            return _TransformerNative.apply(self, packed, x, y, *list(self.parameters()))
        return self._hip_bct(x, None, y, packed=packed)

    def forward_packed(self, x: Tensor, cu_seqlens, max_len: Optional[int] = None, y: Optional[Tensor] = None, y_cu_seqlens=None,
                       y_max_len: Optional[int] = None) -> Tensor:
        """``run_packed`` in the reference layout: (1, N, dim) [, (1, Ny, dim)] -> (1, N, dim)."""
        y = None if y is None else y.transpose(1, 2).contiguous()
        return self.run_packed(x.transpose(1, 2).contiguous(), cu_seqlens, max_len, y, y_cu_seqlens,
                               y_max_len).transpose(1, 2).contiguous()

    def run_bct(self, x: Tensor, y: Optional[Tensor] = None, cache=None, *, lengths=None, y_lengths=None, counts=None) -> Tensor:
        """Channel-major (B, dim, T) in and out; ``y`` (B, dim, Ty) is the cross-attention layer's second sequence.  With
        autograd on, the backward runs on the HIP kernels too (_TransformerNative).  ``cache`` (``new_cache``): ``x`` holds
        the next ``n`` frames of a causal Transformer's sequence; inference only.  A ``TransformerStreamCache``
        (``new_stream_cache``) keeps one position per batch row in device memory: ``1 <= n <= cache.max_chunk``.

        ``lengths`` / ``y_lengths`` (keyword-only): the valid length of every batch row of ``x`` / ``y``, padding on the right
        (``_hip_bct``: the walk and its contract).  A Python sequence or a CPU integer tensor of B entries is validated on the
        host (0 <= length <= T) and copied to the device; a device integer tensor is used without a sync and clamped by the
        kernels -- the form to pass under graph capture.  ``y_lengths`` alone leaves every row of ``x`` full.  Refused, before
        any op: a causal or windowed Transformer, ``cache=``, an active dropout site, ``attention_dtype = "bf16"``,
        ``y_lengths`` without a cross-attention layer, a size other than B.

        ``counts`` (keyword-only; a ``TransformerStreamCache`` only): a contiguous int64 (B,) device tensor; row ``b`` takes the
        first ``clamp(counts[b], 0, n)`` frames and advances by as many (``_hip_bct``).  The kernels read it, the host never
        does.  Refused, before any op: no cache, a ``TransformerCache`` (its ``length`` is a host integer), ``lengths=``, a
        wrong dtype, shape or device, a non-contiguous tensor."""
        if counts is not None:
            if lengths is not None or y_lengths is not None:
                raise AgxError("counts= with lengths=: a counted call is a cached causal step and takes no lengths")
            _checked_counts("Transformer", counts, cache, TransformerStreamCache, TransformerCache)
        if lengths is not None or y_lengths is not None:
            lens = self._check_lengths(x, y, cache, lengths, y_lengths)
            if needs_grad(x, self) or (y is not None and torch.is_grad_enabled() and y.requires_grad):
                return _TransformerNative.apply(self, lens, x, y, *list(self.parameters()))
            return self._hip_bct(x, None, y, lens=lens)
        if cache is not None:
            self._check_cache(x, cache)
            if y is not None:
                raise AgxError("this Transformer was built without context_y and takes no second sequence y")
            return self._hip_bct(x, None, None, cache, counts=counts)
        if needs_grad(x, self) or (y is not None and torch.is_grad_enabled() and y.requires_grad):
            return _TransformerNative.apply(self, None, x, y, *list(self.parameters()))
        return self._hip_bct(x, None, y)

    def forward(self, x: Tensor, y=None, cache=None, *, lengths=None, y_lengths=None, counts=None) -> Tensor:
        y = None if y is None else y.transpose(1, 2).contiguous()
        return self.run_bct(x.transpose(1, 2).contiguous(), y, cache, lengths=lengths, y_lengths=y_lengths,
                            counts=counts).transpose(1, 2).contiguous()


class TransformerBottleneck(nn.Module):
    """Adapter that lets a ``Transformer`` stand where the quantiser does
    (``CausalVQAE.replace_quantizer``, vae.py:347-348; ``Trainer.train_new_quantizer``,
    training.py:502-523).  Honours the quantiser call contract of vae.py:315-318:
    ``(x[b l c], codebook_n, update_codebook=, prioritize_early=) -> (x_out, index, loss)``
    with ``index = None`` and a zero loss (there is nothing to commit to).  The
    reference ships no such adapter; this one is build-defined."""

    def __init__(self, transformer: Transformer, num_quantizers: int = 1):
        super().__init__()
        self.transformer = transformer
        self.num_quantizers = num_quantizers   # training.py:183 reads it
        self.use_som = False                    # utils.py:239

    def quantize_bcl(self, x: Tensor, codebook_n=None, update_codebook=False, prioritize_early=False, cache=None, *,
                     lengths=None):
        """``cache`` (``Transformer.new_cache``; default None: the uncached call) and ``lengths`` (the valid frames of every
        row of a right-padded batch, ``Transformer.run_bct``) are passed on to the transformer."""
        if self.transformer.cross_attention:
            raise AgxError("TransformerBottleneck: the transformer has a cross-attention layer (context_y) and the quantiser call "
                           "contract of CausalVQAE.forward carries no second sequence y -- call Transformer.forward(x, y) directly")
        y = self.transformer.run_bct(x, cache=cache, lengths=lengths)
        return y, None, torch.zeros((), dtype=torch.float32, device=x.device)

    def forward(self, x: Tensor, codebook_n=None, update_codebook=False, prioritize_early=False, cache=None, *, lengths=None):
        y, idx, loss = self.quantize_bcl(x.transpose(1, 2).contiguous(), cache=cache, lengths=lengths)
        return y.transpose(1, 2).contiguous(), idx, loss

    def get_stale_clusters(self):
        return []

    def update_cutoff(self, new_cutoff=None, ratio=None):
        return None


class _Conv1x1:
    """A k = 1 ``nn.Conv1d`` seen as the ``nn.Linear`` ``_PackedLinear`` stacks: ``weight`` (out, in) is a view of the conv's
    (out, in, 1), so its data pointer and version are the parameter's."""

    def __init__(self, conv: nn.Conv1d):
        self.conv, self.out_features = conv, conv.out_channels

    @property
    def weight(self):
        return self.conv.weight[:, :, 0]

    @property
    def bias(self):
        return self.conv.bias


# Stream ids of the dropout sites of a ConformerBlock: its four sub-blocks are "layers" 0..3 of the one seed a call draws, so
# first_ff takes the streams 2, 3, the attention 4, 5, the conv block 8 and second_ff 14, 15 -- seven distinct pairs.
CONFORMER_FF1, CONFORMER_ATTENTION, CONFORMER_CONV, CONFORMER_FF2 = 0, 1, 2, 3
SITE_CONV_OUT = 0


class ConformerConvBlock(nn.Module):
    """transformers.py:281-335, the convolution module of a Conformer block: LayerNorm -> pointwise conv C -> 2 C -> GLU ->
    depthwise conv, ``padding="same"`` -> BatchNorm1d -> SiLU -> pointwise conv -> dropout, with the reference's ``net`` layout
    and ``state_dict()`` keys.  Build-defined, because the reference's class cannot be constructed or run:
    ``out_channels = in_channels`` (the reference reads an attribute it never sets: the conv is depthwise), and the LayerNorm
    acts over channels, before the rearrangement to (b, d, n), as in the Conformer paper (the reference applies it after, to
    the time axis).  ``forward`` takes (B, T, C); ``run_bct`` the channel-major (B, C, T) it computes in.

    Eval mode is four launches: LN, pointwise-in, the fused GLU + depthwise conv + BatchNorm (running statistics) + SiLU kernel
    of ``csrc/conformer.hip``, pointwise-out (+ residual).  Training mode: LN, pointwise-in, GLU + depthwise conv, batch
    statistics (two launches; the running statistics and ``num_batches_tracked`` are updated by the second), normalise + SiLU,
    pointwise-out, and with ``dropout > 0`` ``dropout_add``.  The ``nn`` children only hold parameters and buffers.

    ``causal=True`` (build-defined, keyword-only): ``net[3]`` is the same depthwise ``nn.Conv1d`` without padding, the input is
    padded by K - 1 frames on the left -- an output sees its own frame and the K - 1 before it -- and every launch count above
    holds with the causal ops of ``csrc/conformer.hip`` in place of the "same" ones.  The ``state_dict()`` keys and shapes are
    those of the non-causal block.  A causal block in eval mode also runs incrementally: ``new_conv_state(batch)`` is the
    (B, C, K - 1) history of post-GLU values, and ``run_bct(x, conv_state=state)`` takes the next ``n`` frames -- up to
    ``ops.CONFORMER_MAX_STEP`` in the one launch of ``ops.glu_dwconv_step`` where the fused conv launch was, a longer chunk in
    ``ops.glu_dwconv_causal(hist=)`` + ``ops.glu_hist_update`` -- and rewrites the state in place.  Chunked calls are bit for bit
    the single call."""

    def __init__(self, in_channels, kernel_size=17, dropout=0.1, activation=nn.SiLU, *, causal=False):
        super().__init__()
        if activation is not nn.SiLU:
            raise NotImplementedError("only SiLU is fused behind the BatchNorm (csrc/conformer.hip)")
        if int(kernel_size) != kernel_size or not 1 <= kernel_size <= ops.CONFORMER_MAX_K:
            raise ValueError(f"kernel_size = {kernel_size}: the depthwise kernel takes 1 <= kernel_size <= {ops.CONFORMER_MAX_K}")
        self.in_channels = self.out_channels = in_channels
        self.kernel_size, self.causal = int(kernel_size), bool(causal)
        self.net = nn.Sequential(
            nn.LayerNorm(in_channels),
            nn.Conv1d(in_channels, 2 * in_channels, kernel_size=1),
            nn.GLU(dim=-2),
            nn.Conv1d(in_channels, in_channels, kernel_size=self.kernel_size, groups=in_channels) if self.causal else
            nn.Conv1d(in_channels, in_channels, kernel_size=self.kernel_size, padding="same", groups=in_channels),
            nn.BatchNorm1d(in_channels),
            activation(),
            nn.Conv1d(in_channels, in_channels, kernel_size=1),
            nn.Dropout(dropout) if dropout > 0 else nn.Identity())
        self._in, self._out = _PackedLinear(_Conv1x1(self.net[1])), _PackedLinear(_Conv1x1(self.net[6]))
        self.last_dropout_seed = None

    def _p_out(self) -> float:
        return _active_p(self.net[7]) if isinstance(self.net[7], nn.Dropout) else 0.0

    def new_conv_state(self, batch: int) -> Tensor:
        """The conv state of ``batch`` streams at their start: zeros (B, C, K - 1) on the parameters' device -- the post-GLU values
        of the K - 1 frames before the next call, oldest first.  ``state[rows].zero_()`` hands rows to new streams."""
        if not self.causal:
            raise AgxError("new_conv_state: a conv state needs a causal block (causal=True): the \"same\" conv looks ahead")
        if batch < 1:
            raise AgxError(f"new_conv_state: batch = {batch}")
        return torch.zeros((batch, self.in_channels, self.kernel_size - 1), dtype=torch.float32, device=self.net[3].weight.device)

    def _check_conv_state(self, x: Tensor, keep: Optional[dict], conv_state: Tensor) -> None:
        """The refusals of a call on a conv state, before any op."""
        if not self.causal:
            raise AgxError("a conv state needs a causal block (causal=True): the \"same\" conv looks ahead")
        if self.net[4].training:
            raise AgxError("a conv state with BatchNorm in training mode: batch statistics of a chunk are not those of the sequence "
                           "(a cached call runs in eval mode)")
        if keep is not None or needs_grad(x, self):
            raise AgxError("there is no backward through a cached call: run it under torch.no_grad()")
        if x.dim() != 3 or x.shape[1] != self.in_channels:
            raise AgxError(f"ConformerConvBlock: x is {tuple(x.shape)}, expected (B, {self.in_channels}, T)")
        want = (x.shape[0], self.in_channels, self.kernel_size - 1)
        if not isinstance(conv_state, Tensor) or tuple(conv_state.shape) != want or conv_state.dtype != torch.float32 \
                or not conv_state.is_contiguous():
            got = tuple(conv_state.shape) if isinstance(conv_state, Tensor) else type(conv_state).__name__
            raise AgxError(f"conv state: expected a contiguous float32 {want} tensor (B, C, K - 1) for x {tuple(x.shape)}, got {got}")

    def _check_counts(self, x: Tensor, conv_state: Optional[Tensor], counts) -> None:
        """The refusals of ``counts=``, before any op.  No value is read: the kernel clamps every entry to [0, n]."""
        if conv_state is None:
            raise AgxError("ConformerConvBlock: counts= without a conv state: a per-row frame count belongs to a cached step")
        b, device = (conv_state.shape[0], conv_state.device) if isinstance(conv_state, Tensor) else (0, None)
        ops._checked_counts("ConformerConvBlock", counts, b, device, on="the conv state on")
        if x.dim() == 3 and x.shape[-1] > ops.CONFORMER_MAX_STEP:
            raise AgxError(f"ConformerConvBlock: a counted call takes at most CONFORMER_MAX_STEP = {ops.CONFORMER_MAX_STEP} frames (the "
                           f"one launch of glu_dwconv_step), got {x.shape[-1]}")

    def run_bct(self, x: Tensor, residual: Optional[Tensor] = None, keep: Optional[dict] = None,
                drop: Optional[tuple] = None, conv_state: Optional[Tensor] = None, counts: Optional[Tensor] = None,
                mask_counts: bool = True) -> Tensor:
        """(B, C, T) -> net(x) [+ residual: x itself].  ``keep`` marks a forward whose backward will run (``backward_bct``): z is then
        written in eval mode too.  With autograd on and no ``keep`` the call goes through ``_ConformerNative``.  ``conv_state``
        (``new_conv_state``; a causal block in eval mode, no gradient): ``x`` holds the next T frames of the streams the state
        belongs to, and the state is rewritten in place.

        ``counts`` (with ``conv_state``; int64 (B,), device; T <= ``ops.CONFORMER_MAX_STEP``): row ``b`` takes its first
        ``clamp(counts[b], 0, T)`` frames -- ``ops.glu_dwconv_step(counts=)`` where the step was, so the state is that of those
        frames alone -- and the result is exact 0 behind them (``ops.mask_tail`` in place, one more launch; the enclosing
        ``ConformerBlock`` passes ``mask_counts=False`` and masks its own output instead).  Every other op of the block is
        pointwise in time, so NaN in ``x`` behind a row's count reaches neither a valid frame nor the state."""
        if residual is not None and residual is not x:
            raise AgxError("ConformerConvBlock: the residual is the block's own input (x + net(x)), or None")
        if counts is not None:
            self._check_counts(x, conv_state, counts)
        if conv_state is not None:
            self._check_conv_state(x, keep, conv_state)
        if keep is None and needs_grad(x, self):
            return _ConformerNative.apply(self, residual is not None, drop, x, *list(self.parameters()))
        dw, bn = self.net[3], self.net[4]
        if x.dim() != 3 or x.shape[1] != self.in_channels:
            raise AgxError(f"ConformerConvBlock: x is {tuple(x.shape)}, expected (B, {self.in_channels}, T)")
        if bn.training and x.shape[0] * x.shape[2] < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
        p = self._p_out()
        gamma, beta = bn.weight.detach(), bn.bias.detach()
        conv = ops.glu_dwconv_causal if self.causal else ops.glu_dwconv
        xn = _ln(self.net[0], x)
        u = self._in.forward(xn)
        if conv_state is not None:
            bn_eval = (gamma, beta, bn.running_mean, bn.running_var)
            if counts is not None:
                y = ops.glu_dwconv_step(u, dw.weight.detach(), dw.bias.detach(), bn_eval, conv_state, eps=bn.eps, counts=counts)
            elif x.shape[-1] <= ops.CONFORMER_MAX_STEP:
                y = ops.glu_dwconv_step(u, dw.weight.detach(), dw.bias.detach(), bn_eval, conv_state, eps=bn.eps)
            else:
                y = ops.glu_dwconv_causal(u, dw.weight.detach(), dw.bias.detach(), bn=bn_eval, eps=bn.eps, hist=conv_state)
                ops.glu_hist_update(u, conv_state)
        elif not bn.training and keep is None:
            y = conv(u, dw.weight.detach(), dw.bias.detach(), bn=(gamma, beta, bn.running_mean, bn.running_var), eps=bn.eps)
        else:
            z = conv(u, dw.weight.detach(), dw.bias.detach())
            if bn.training:
                mean, var = ops.bn_stats(z, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum)
            else:       # frozen statistics: a private copy, the backward must see what the forward saw
                mean, var = bn.running_mean.clone(), bn.running_var.clone()
            y = ops.bn_silu(z, gamma, beta, mean, var, bn.eps, training=bn.training)
            if keep is not None:
                keep.update(cx=x, cxn=xn, u=u, z=z, mean=mean, var=var, y=y)
                keep["conv"] = dict(training=bn.training)
        if p > 0:
            seed, layer = _site(drop, self)
            if keep is not None:
                keep["conv"].update(p=p, seed=seed, layer=layer)
            out = self._out.forward(y)
            return ops.dropout_add(out, residual, p, seed, 4 * layer + SITE_CONV_OUT, out=out)
        out = self._out.forward(y, EPI_RESIDUAL if residual is not None else 0, residual)
        if counts is not None and mask_counts:
            ops.mask_tail(out, None, out=out, counts=counts)
        return out

    def backward_bct(self, kept: dict, g: Tensor, residual: bool = True):
        """``g`` = the gradient of ``run_bct(x, residual=x, keep=kept)`` -> (dx, gradients in ``parameters()`` order); without
        ``residual`` the gradient does not reach x around the block."""
        c = kept["conv"]
        dw, bn = self.net[3], self.net[4]
        g_out = g
        if c.get("p"):
            g_out = ops.dropout_add(g, None, c["p"], c["seed"], 4 * c["layer"] + SITE_CONV_OUT)
        dy, g_o = self._out.backward(kept["y"], g_out)
        dz, dgamma, dbeta = ops.bn_silu_backward(dy, kept["z"], bn.weight.detach(), bn.bias.detach(), kept["mean"], kept["var"],
                                                 bn.eps, training=c["training"], out=dy)
        du, d_dw, d_db = (ops.glu_dwconv_causal_backward if self.causal else ops.glu_dwconv_backward)(dz, kept["u"], dw.weight.detach())
        dxn, g_i = self._in.backward(kept["cxn"], du)
        dx, dweight, dbias = _ln_bwd(self.net[0], kept["cx"], dxn, add=g if residual else None)
        return dx, [dweight, dbias, g_i[0].unsqueeze(-1), g_i[1], d_dw, d_db, dgamma, dbeta, g_o[0].unsqueeze(-1), g_o[1]]

    def forward(self, x: Tensor, cache=None, counts=None) -> Tensor:
        """Reference layout (B, T, C).  ``cache`` (a ``ConformerStreamCache``, or a ``ConformerCache`` without ``counts``): the
        block runs on the cache's conv state; it has no position of its own and advances none.  ``counts``: ``run_bct``."""
        if cache is None:
            if counts is not None:
                raise AgxError("ConformerConvBlock: counts= without cache=: a per-row frame count belongs to a cached step on a stream "
                               "cache (new_stream_cache)")
            return self.run_bct(x.transpose(1, 2).contiguous()).transpose(1, 2).contiguous()
        if not isinstance(cache, (ConformerCache, ConformerStreamCache)):
            raise AgxError(f"cache= takes a ConformerCache or a ConformerStreamCache (new_cache / new_stream_cache), got {type(cache).__name__}")
        if counts is not None:
            _checked_counts("ConformerConvBlock", counts, cache, ConformerStreamCache, ConformerCache)
        return self.run_bct(x.transpose(1, 2).contiguous(), conv_state=cache.conv_state, counts=counts).transpose(1, 2).contiguous()


class ConformerBlock(nn.Module):
    """transformers.py:337-368: ``x += 0.5 ff1(x); x += attention(x); x += conv_block(x); LN(x + 0.5 ff2(x))``.  Build-defined
    where the reference cannot be constructed: the stray ``activation`` keyword it passes to ``Attention`` is
    dropped, and ``kernel_size`` / ``context_x`` -- which the reference hard-codes through the defaults of its children -- are
    keyword-only arguments.  Both 0.5 factors are folded into the packed image of the FFN-out projections (``_PackedLinear``):
    no launch, no pass over the tensor.

    An eval-mode call is 4 + 4 + 4 + 4 + 1 = 17 launches: per feed-forward LN, FFN-in, SiLU, FFN-out (+res) -- the SiLU one more
    than a GELU feed-forward --, the attention's LN, QKV, attention, W_o (+res), the conv block's four and the final LN.  A
    training-mode call with ``dropout > 0`` draws one 64-bit seed (``last_dropout_seed``; ``torch.manual_seed`` reproduces it);
    its seven sites take distinct stream ids (``CONFORMER_*``).

    ``causal=True`` (build-defined, keyword-only; ``window=W`` with it): the attention is the causal (windowed) layer of
    ``Attention`` and the conv block the causal one, so no output sees a later frame; parameters and ``state_dict()`` are
    unchanged.  Causal attention has no dropout kernel: a causal block whose attention dropout is active (training mode,
    ``dropout > 0``) is refused.  ``new_cache`` / ``new_stream_cache`` and ``run_bct(x, cache=)`` run the block incrementally, as
    ``Transformer`` does: the attention on its key/value buffer or ring, the conv block on its (B, C, K - 1) state.  A cached
    step is the 17 launches above plus the attention's write into its cache and, on a stream cache, ``ops.stream_advance``:
    the conv state needs no position, so a step on a stream cache makes no host decision and can be captured once and
    replayed (``GraphedForward``)."""

    def __init__(self, dim, hidden_dim_ratio=4, heads=8, dropout=0.1, ff_activation=nn.SiLU, conv_activation=nn.SiLU, *,
                 kernel_size=17, context_x=32, causal=False, window=None):
        super().__init__()
        self.first_ff = FeedForward(dim, dim * hidden_dim_ratio, activation=ff_activation, dropout=dropout)
        self.attention = Attention(dim, n_heads=heads, dim_head=dim // heads, dropout=dropout, context_x=context_x, causal=causal,
                                   window=window)
        self.conv_block = ConformerConvBlock(dim, kernel_size=kernel_size, dropout=dropout, activation=conv_activation, causal=causal)
        self.second_ff = FeedForward(dim, dim * hidden_dim_ratio, activation=ff_activation, dropout=dropout)
        self.layer_norm = nn.LayerNorm(dim)
        self.dim, self.context_x = dim, context_x
        self.causal, self.window = bool(causal), self.attention.window
        self.last_dropout_seed = None

    def new_cache(self, batch: int, capacity: Optional[int] = None) -> "ConformerCache":
        """An empty cache for ``batch`` sequences (``ConformerCache``): the attention's key/value buffer of ``capacity`` columns
        (default ``context_x``; a ring of at least ``window`` columns on a windowed block) as ``Transformer.new_cache`` makes it,
        and the conv state at the start of a stream.  Needs a causal block."""
        if not self.causal:
            raise AgxError("new_cache: a cache needs a causal ConformerBlock (causal=True)")
        (kv,), capacity, _ = _new_kv("new_cache", self, [self.attention.inner_dim], batch, capacity)
        return ConformerCache(kv, batch, capacity, self.window, self.conv_block.new_conv_state(batch))

    def new_stream_cache(self, batch: int, capacity: Optional[int] = None) -> "ConformerStreamCache":
        """An empty cache for ``batch`` live streams with the positions in device memory (``ConformerStreamCache``): the ring of
        ``Transformer.new_stream_cache``, every position 0, and the conv state at the start of a stream.  Needs a windowed causal
        block.  A call takes ``1 <= n <= cache.max_chunk`` frames."""
        if not self.causal or self.window is None:
            raise AgxError("new_stream_cache: device-held positions need a windowed causal ConformerBlock (causal=True, window=W)")
        (kv,), capacity, max_chunk = _new_kv("new_stream_cache", self, [self.attention.inner_dim], batch, capacity)
        pos = torch.zeros(batch, dtype=torch.int64, device=kv.device)
        return ConformerStreamCache(kv, pos, capacity, self.window, max_chunk, self.conv_block.new_conv_state(batch))

    def _check_cache(self, x: Tensor, cache) -> None:
        """The refusals of a cached call, before any op; on a stream cache none of them reads a position."""
        on_device = isinstance(cache, ConformerStreamCache)
        if not isinstance(cache, (ConformerCache, ConformerStreamCache)):
            raise AgxError(f"cache= takes a ConformerCache or a ConformerStreamCache (new_cache / new_stream_cache), got {type(cache).__name__}")
        if not self.causal or (on_device and self.window is None):
            raise AgxError("a stream cache needs a windowed causal ConformerBlock (causal=True, window=W)" if on_device else
                           "a cache needs a causal ConformerBlock (causal=True)")
        _check_cached_call(self, "this block", x, cache, on_device, self.dim)
        if self.conv_block.net[4].training:
            raise AgxError("a cached call with BatchNorm in training mode: batch statistics of a chunk are not those of the sequence "
                           "(a cached call runs in eval mode)")
        if self.attention.attention_dtype != "fp32":
            raise AgxError(f"causal attention runs in fp32: attention_dtype = {self.attention.attention_dtype!r} has no kernel")
        if tuple(cache.kv.shape) != (cache.batch, 2 * self.attention.inner_dim, cache.capacity):
            raise AgxError(f"the cache's key/value buffer is {tuple(cache.kv.shape)}, this block needs "
                           f"{(cache.batch, 2 * self.attention.inner_dim, cache.capacity)}")
        want = (cache.batch, self.dim, self.conv_block.kernel_size - 1)
        if tuple(cache.conv_state.shape) != want:
            raise AgxError(f"the cache's conv state is {tuple(cache.conv_state.shape)}, this block needs {want} (B, C, K - 1)")

    def _dropout_active(self) -> bool:
        sites = [self.attention.dropout, self.conv_block.net[7]] + [f.net[i] for f in (self.first_ff, self.second_ff) for i in (3, 5)]
        return any(isinstance(m, nn.Dropout) and m.training and m.p > 0 for m in sites)

    def _hip_bct(self, x: Tensor, keep: Optional[dict] = None, cache=None, counts: Optional[Tensor] = None) -> Tensor:
        """The one forward walk.  ``keep``: the training forward -- the dict receives one dict of named intermediates per
        sub-block.  ``cache`` (checked by ``_check_cache``): the attention runs on the cache's key/value buffer, the conv block on
        its state, and the cache advances by the call's frames.

        ``counts`` (a stream cache only): ``mask_tail(x, counts=)`` out of place on the way in, the counted ring
        write and the counted conv step where the uncounted ones were, the counted advance, and ``mask_tail`` in place on the
        output -- two more launches than the uncounted step.  ``counts=None``: no counted op is called."""
        if x.dim() != 3 or x.shape[1] != self.dim:
            raise AgxError(f"ConformerBlock: x is {tuple(x.shape)}, expected (B, {self.dim}, T)")
        if x.shape[-1] > self.context_x:
            raise AgxError(f"sequence length {x.shape[-1]} exceeds the ALiBi context {self.context_x}")
        if self.causal and _active_p(self.attention.dropout) > 0:
            raise AgxError("a causal ConformerBlock with attention dropout > 0 in training mode has no kernel (eval mode runs)")
        if cache is not None:
            if counts is not None:
                x = ops.mask_tail(x, None, counts=counts)
            x = self.first_ff.run_bct(x, x, None, None, scale=0.5)
            x = self.attention.run_bct(x, x, None, None, None, kv_cache=cache.kv_cache(0, counts))
            # the conv block's own mask is off on a counted step: the block masks its output once, behind the last LayerNorm
            x = self.conv_block.run_bct(x, x, None, None, conv_state=cache.conv_state, counts=counts, mask_counts=counts is None)
            x = self.second_ff.run_bct(x, x, None, None, scale=0.5)
            cache.advance(x.shape[-1], counts)
            x = _ln(self.layer_norm, x)
            return x if counts is None else ops.mask_tail(x, None, out=x, counts=counts)
        seed = None
        if self._dropout_active():
            seed = self.last_dropout_seed = ops.draw_dropout_seed()
        kept = {name: (None if keep is None else {}) for name in ("ff1", "attention", "conv", "ff2")}
        site = (lambda layer: None) if seed is None else (lambda layer: (seed, layer))
        x = self.first_ff.run_bct(x, x, kept["ff1"], site(CONFORMER_FF1), scale=0.5)
        x = self.attention.run_bct(x, x, kept["attention"], None, site(CONFORMER_ATTENTION))
        x = self.conv_block.run_bct(x, x, kept["conv"], site(CONFORMER_CONV))
        x = self.second_ff.run_bct(x, x, kept["ff2"], site(CONFORMER_FF2), scale=0.5)
        if keep is not None:
            kept["ln"] = dict(x4=x)
            keep.update(kept)
        return _ln(self.layer_norm, x)

    def backward_bct(self, keep: dict, g: Tensor):
        """``g`` = the gradient of ``_hip_bct(x, keep)`` -> (dx, gradients in ``parameters()`` order)."""
        g, dweight, dbias = _ln_bwd(self.layer_norm, keep["ln"]["x4"], g, add=None)
        g, g_ff2 = self.second_ff.backward_bct(keep["ff2"], g, scale=0.5)
        g, g_conv = self.conv_block.backward_bct(keep["conv"], g)
        g, g_attention, _ = self.attention.backward_bct(keep["attention"], g)
        g, g_ff1 = self.first_ff.backward_bct(keep["ff1"], g, scale=0.5)
        return g, g_ff1 + g_attention + g_conv + g_ff2 + [dweight, dbias]

    def run_bct(self, x: Tensor, cache=None, counts=None) -> Tensor:
        """Channel-major (B, dim, T) in and out, T <= context_x.  With autograd on, the backward runs on the HIP kernels too
        (``_ConformerNative``).  ``cache`` (``new_cache`` / ``new_stream_cache``): ``x`` holds the next ``n`` frames of a causal
        block's sequences; inference only, eval mode.  ``counts`` (a ``ConformerStreamCache`` only): a contiguous int64 (B,)
        device tensor; row ``b`` takes the first ``clamp(counts[b], 0, n)`` frames and advances by as many (``_hip_bct``).
        Refused, before any op: no cache, a ``ConformerCache`` (its ``length`` is a host integer), a wrong dtype, shape or
        device, a non-contiguous tensor."""
        if counts is not None:
            _checked_counts("ConformerBlock", counts, cache, ConformerStreamCache, ConformerCache)
        if cache is not None:
            self._check_cache(x, cache)
            return self._hip_bct(x, None, cache, counts)
        if needs_grad(x, self):
            return _ConformerNative.apply(self, False, None, x, *list(self.parameters()))
        return self._hip_bct(x)

    def forward(self, x: Tensor, cache=None, counts=None) -> Tensor:
        return self.run_bct(x.transpose(1, 2).contiguous(), cache, counts).transpose(1, 2).contiguous()


class _ConformerNative(torch.autograd.Function):
    """``ConformerBlock`` or ``ConformerConvBlock`` forward + hand-written backward on the HIP kernels, in the style of
    ``_TransformerNative``: the k = 1 conv backward for every Linear and pointwise conv, the attention and LayerNorm backward
    kernels, ``agx_silu_backward``, and the three backward ops of ``csrc/conformer.hip``; the dropout masks of a training-mode
    forward are regenerated from the seed saved in the context.  No ATen arithmetic touches an activation.  ``residual`` and
    ``drop`` are the conv block's own arguments (a block passes False and None)."""

    @staticmethod
    def forward(ctx, module, residual: bool, drop, x: Tensor, *params: Tensor):
        keep = {}
        x = x.detach()
        with torch.no_grad():
            if isinstance(module, ConformerBlock):
                out = module._hip_bct(x, keep)
            else:
                keep["conv"] = {}
                out = module.run_bct(x, x if residual else None, keep["conv"], drop)
        # tensors go through save_for_backward, everything else (seeds, probabilities, modes) stays in the context
        ctx.meta = {name: {k: v for k, v in kept.items() if not isinstance(v, Tensor)} for name, kept in keep.items()}
        ctx.names = [(name, k) for name, kept in keep.items() for k, v in kept.items() if isinstance(v, Tensor)]
        ctx.save_for_backward(*[keep[name][k] for name, k in ctx.names])
        ctx.module, ctx.residual = module, residual
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g: Tensor):
        keep = {name: dict(meta) for name, meta in ctx.meta.items()}
        for (name, k), t in zip(ctx.names, ctx.saved_tensors):
            keep[name][k] = t
        g = g.contiguous()
        if isinstance(ctx.module, ConformerBlock):
            dx, grads = ctx.module.backward_bct(keep, g)
        else:
            dx, grads = ctx.module.backward_bct(keep["conv"], g, residual=ctx.residual)
        return (None, None, None, dx if ctx.needs_input_grad[3] else None, *grads)
