"""Drop-in ``Alibi`` / ``Attention`` / ``FeedForward`` / ``Transformer`` executed
by libagx, plus the bottleneck adapter the reference never shipped.

Mirrors ``networks/transformers.py:7-279`` (class names, constructor arguments,
``state_dict()`` keys ``layers.{i}.0.norm.*``, ``layers.{i}.0.W_{q,k,v,o}.weight``,
``layers.{i}.1.net.{0,1,4}.*``).  Only the branch the reference can actually
execute is implemented -- self-attention with ALiBi (the learned
pos-emb and cross-attention branches raise in the reference); ``depth > 1`` is
build-defined as "every layer uses ALiBi".

Execution is channel-major: the block works on ``(B, C, T)`` tensors (what the
encoder emits), every ``Linear`` is a k=1 convolution on the fp32 MFMA conv
kernel with the activation / residual fused into its epilogue, LayerNorm and
softmax(QK^T + ALiBi)V are the two dedicated kernels of ``csrc/attention.hip``.
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
    The attention kernel never reads ``M``: it evaluates ``-slope_h * |i - j|`` itself."""

    def __init__(self, context_x, context_y=None, n_heads=8):
        super().__init__()
        if context_y is not None and context_y != context_x:
            raise NotImplementedError("cross-attention ALiBi (context_y != context_x) has no HIP kernel")
        self.context_x = context_x
        self.context_y = context_x if context_y is None else context_y
        self.n_heads = n_heads
        n_sequence = torch.arange(start=n_heads, end=0, step=-1)
        self.register_buffer("head_scalars", 2 ** (-8 / n_sequence), persistent=False)  # :38-39
        idx = torch.arange(context_x, dtype=torch.float32)
        m = -(idx[:, None] - idx[None, :]).abs()
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
    (B, C, T) tensor; caches the packed image of the stacked weights."""

    def __init__(self, *linears):
        self.linears = linears
        self.c_out = sum(l.out_features for l in linears)
        self.key = self.packed = self.bias = self.w3d = None

    def get(self):
        key = tuple((l.weight.data_ptr(), l.weight._version,
                     None if l.bias is None else (l.bias.data_ptr(), l.bias._version)) for l in self.linears)
        if key != self.key:
            w = torch.cat([l.weight.detach() for l in self.linears], dim=0)
            c_out, c_in = w.shape
            desc = ops.conv_desc(CONV_CAUSAL, 1, c_in, c_out, 1 << 20, 1)
            self.w3d = w.reshape(c_out, c_in, 1).contiguous()      # the native backward reads it
            self.packed = ops.conv_pack(desc, self.w3d)
            if any(l.bias is not None for l in self.linears):
                self.bias = torch.cat([l.bias.detach() if l.bias is not None
                                       else torch.zeros(l.out_features, device=w.device) for l in self.linears])
            else:
                self.bias = None
            self.key = key
        return self.packed, self.bias

    def forward(self, x: Tensor, epilogue: int = 0, res: Optional[Tensor] = None) -> Tensor:
        packed, bias = self.get()
        b, c_in, t = x.shape
        desc = ops.conv_desc(CONV_CAUSAL, b, c_in, self.c_out, t, 1, 1, 1, epilogue)
        return ops.conv_forward(desc, x, packed, bias, res)

    def backward(self, x_in: Tensor, dy: Tensor, pre: Optional[Tensor] = None):
        """Backward of ``forward`` with epilogue 0, on the image that forward packed: (dx, the gradients of the linears'
        parameters in ``parameters()`` order); with ``pre`` the GELU gradient of the layer BELOW (at its pre-activation)
        is fused into the bwd-data epilogue."""
        b, c_in, t = x_in.shape
        desc = ops.conv_desc(CONV_CAUSAL, b, c_in, self.c_out, t, 1)
        dw, _, db = ops.conv_bwd_weight(desc, x_in, dy, self.w3d, None, want_bias=self.bias is not None)
        pk = ops.conv_pack_bwd(desc, self.w3d)
        dx = ops.conv_bwd_data(desc, dy, pk) if pre is None else ops.conv_bwd_data_gelu(desc, dy, pk, pre)
        dw, grads, row = dw.reshape(self.c_out, c_in), [], 0
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


class Attention(nn.Module):
    """transformers.py:95-191 (pre-LN multi-head self-attention with ALiBi)."""

    def __init__(self, dim, dim_head=64, n_heads=8, dropout=0., bias=False, context_x=32, context_y=None,
                 has_pos_emb=True, alibi=True):
        super().__init__()
        if not alibi:
            raise NotImplementedError("only the ALiBi branch is defined in the reference (SURVEY 5.1)")
        if context_y is not None:
            raise NotImplementedError("cross-attention has no HIP kernel")
        if dropout != 0.:
            raise NotImplementedError("dropout > 0 is training-only and not on the forward path")
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
        self.cross_attention = False
        self.context = context_x
        self.alibi_obj = Alibi(context_x, None, n_heads=n_heads)
        self._qkv, self._o = _PackedLinear(self.W_q, self.W_k, self.W_v), _PackedLinear(self.W_o)
        # arithmetic of the QK^T / PV contractions: "fp32" (exact, the reference's) or "bf16" (bf16 MFMA, fp32 accumulate
        # and softmax -- BASELINE config 3); inference only (run_bct: ``keep``)
        self.attention_dtype = "fp32"

    def _attn(self) -> dict:
        return dict(slopes=self.alibi_obj.head_scalars, heads=self.n_heads, head_dim=self.dim_head, scale_div=self.dim_head ** 0.5)

    def run_bct(self, x: Tensor, residual: Optional[Tensor] = None, keep: Optional[dict] = None) -> Tensor:
        """(B, dim, T) -> W_o(attn(LN(x))) [+ residual], channel-major.  ``keep`` marks the training forward: the dict
        receives what ``backward_bct`` reads, and the attention arithmetic is fp32 whatever ``attention_dtype`` says
        (the backward kernels recompute P from fp32 scores, and cover head_dim <= 128)."""
        if x.shape[-1] > self.context:
            raise AgxError(f"sequence length {x.shape[-1]} exceeds the ALiBi context {self.context} "
                           "(the reference fails here too, transformers.py:88-93)")
        if keep is not None and self.dim_head > 128:
            raise AgxError("Transformer: the attention backward kernels cover head_dim <= 128 "
                           "(agx_attention_alibi_backward_ex); larger heads run forward only -- there is no ATen fallback")
        xn = _ln(self.norm, x)
        qkv = self._qkv.forward(xn)
        bf16 = self.attention_dtype == "bf16" and keep is None
        o = ops.attention_alibi(qkv, precision=ops.ATTN_BF16 if bf16 else ops.ATTN_FP32, **self._attn())
        if keep is not None:
            keep.update(h=x, xn1=xn, qkv=qkv, o=o)
        return self._o.forward(o, EPI_RESIDUAL if residual is not None else 0, residual)

    def backward_bct(self, kept: dict, g: Tensor):
        """``g`` = the gradient of ``run_bct(h, residual=h, keep=kept)`` -> (dh, gradients in ``parameters()`` order)."""
        do, g_o = self._o.backward(kept["o"], g)
        dqkv = ops.attention_alibi_backward(kept["qkv"], dout=do, out=kept["o"], **self._attn())
        dxn, g_qkv = self._qkv.backward(kept["xn1"], dqkv)
        dh, dweight, dbias = _ln_bwd(self.norm, kept["h"], dxn, add=g)
        return dh, [dweight, dbias] + g_qkv + g_o

    def forward(self, x: Tensor, y=None) -> Tensor:
        """Reference layout: (B, T, dim) -> (B, T, dim)."""
        if y is not None:
            raise NotImplementedError("cross-attention has no HIP kernel")
        return self.run_bct(x.transpose(1, 2).contiguous()).transpose(1, 2).contiguous()


class FeedForward(nn.Module):
    """transformers.py:193-223: LN -> Linear -> exact GELU -> Linear."""

    def __init__(self, dim, hidden_dim, dropout=0., activation=nn.GELU):
        super().__init__()
        if activation is not nn.GELU:
            raise NotImplementedError("only GELU is fused into the FFN kernel epilogue")
        if dropout != 0.:
            raise NotImplementedError("dropout > 0 is training-only and not on the forward path")
        self.net = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, hidden_dim), activation(), nn.Dropout(dropout),
                                 nn.Linear(hidden_dim, dim), nn.Dropout(dropout))
        self._l1, self._l2 = _PackedLinear(self.net[1]), _PackedLinear(self.net[4])

    def run_bct(self, x: Tensor, residual: Optional[Tensor] = None, keep: Optional[dict] = None) -> Tensor:
        xn = _ln(self.net[0], x)
        hid = self._l1.forward(xn, EPI_GELU_PRE)
        if keep is not None:
            keep.update(x1=x, xn2=xn, hid=hid)
        return self._l2.forward(hid, EPI_RESIDUAL if residual is not None else 0, residual)

    def backward_bct(self, kept: dict, g: Tensor):
        """As ``Attention.backward_bct``; the GELU gradient sits in the FFN-out bwd-data epilogue, at the pre-activation,
        which is recomputed with one conv launch: the forward's FFN-in projection with epilogue 0."""
        pre = self._l1.forward(kept["xn2"])
        dpre, g2 = self._l2.backward(kept["hid"], g, pre=pre)
        dxn, g1 = self._l1.backward(kept["xn2"], dpre)
        dx1, dweight, dbias = _ln_bwd(self.net[0], kept["x1"], dxn, add=g)
        return dx1, [dweight, dbias] + g1 + g2

    def forward(self, x: Tensor) -> Tensor:
        return self.run_bct(x.transpose(1, 2).contiguous()).transpose(1, 2).contiguous()


class _TransformerNative(torch.autograd.Function):
    """Transformer forward + hand-written backward on the HIP kernels: k=1 conv backward for every Linear,
    ``agx_attention_alibi_backward``, ``agx_layernorm_ct_backward`` (residual adds fused as ``add``), the GELU
    gradient in a bwd-data epilogue.  Every layer, the first included, computes its input gradient."""

    @staticmethod
    def forward(ctx, tf, x: Tensor, *params: Tensor):
        keep = []
        with torch.no_grad():
            y = tf._hip_bct(x.detach(), keep)
        ctx.tf, ctx.names = tf, [(li, name) for li, kept in enumerate(keep) for name in kept]
        ctx.save_for_backward(*[t for kept in keep for t in kept.values()])
        return y

    @staticmethod
    def backward(ctx, g: Tensor):
        keep = [{} for _ in ctx.tf.layers]
        for (li, name), t in zip(ctx.names, ctx.saved_tensors):
            keep[li][name] = t
        g, grads = g.contiguous(), []
        for (attention, ff), kept in zip(reversed(ctx.tf.layers), reversed(keep)):
            g, g_ff = ff.backward_bct(kept, g)              # x2 = x1 + W2 gelu(W1 LN2(x1) + b1) + b2
            g, g_attention = attention.backward_bct(kept, g)   # x1 = h + W_o attn(W_qkv LN1(h))
            grads = g_attention + g_ff + grads              # the order of Transformer.parameters()
        return (None, g if ctx.needs_input_grad[1] else None, *grads)


class Transformer(nn.Module):
    """transformers.py:225-279: ``x += attn(x); x += ff(x)`` per layer."""

    def __init__(self, dim, depth=1, heads=8, head_dim=64, dropout=0., context_x=32, context_y=None,
                 has_pos_emb=True, alibi=True):
        super().__init__()
        if context_y is not None:
            raise NotImplementedError("cross-attention has no HIP kernel")
        self.cross_attention = False
        self.layers = nn.ModuleList([
            nn.ModuleList([Attention(dim, n_heads=heads, dim_head=head_dim, dropout=dropout, context_x=context_x,
                                     has_pos_emb=has_pos_emb, alibi=alibi),
                           FeedForward(dim, dim, dropout=dropout)])
            for _ in range(depth)])

    def _hip_bct(self, x: Tensor, keep: Optional[list] = None) -> Tensor:
        """The one forward walk, LN1 -> QKV -> attention -> W_o (+res) -> LN2 -> FFN-in (GELU) -> FFN-out (+res) per layer:
        7 launches, both residual adds fused into the W_o / FFN-out conv epilogues.  ``keep``: the training forward
        (``Attention.run_bct``) -- the list receives one dict of named intermediates per layer."""
        for attention, ff in self.layers:
            kept = None if keep is None else {}
            x = attention.run_bct(x, x, kept)
            x = ff.run_bct(x, x, kept)
            if keep is not None:
                keep.append(kept)
        return x

    def run_bct(self, x: Tensor) -> Tensor:
        """Channel-major (B, dim, T) in and out.  With autograd on, the backward runs on the HIP kernels too
        (_TransformerNative)."""
        if needs_grad(x, self):
            return _TransformerNative.apply(self, x, *list(self.parameters()))
        return self._hip_bct(x)

    def forward(self, x: Tensor, y=None) -> Tensor:
        if y is not None:
            raise NotImplementedError("cross-attention has no HIP kernel")
        return self.run_bct(x.transpose(1, 2).contiguous()).transpose(1, 2).contiguous()


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

    def quantize_bcl(self, x: Tensor, codebook_n=None, update_codebook=False, prioritize_early=False):
        y = self.transformer.run_bct(x)
        return y, None, torch.zeros((), dtype=torch.float32, device=x.device)

    def forward(self, x: Tensor, codebook_n=None, update_codebook=False, prioritize_early=False):
        y, idx, loss = self.quantize_bcl(x.transpose(1, 2).contiguous())
        return y.transpose(1, 2).contiguous(), idx, loss

    def get_stale_clusters(self):
        return []

    def update_cutoff(self, new_cutoff=None, ratio=None):
        return None
