"""Drop-in ``FiLM`` / ``SqueezeExcite`` executed by libagx: conditioning on a vector.

Mirrors ``networks/conditioning.py:3-52`` (class names, constructor arguments, attributes, ``state_dict()`` keys
``gamma.*`` / ``beta.*`` and ``squeeze.*`` / ``excite.*``).  Everything is fp32; forward and backward run on the kernels of
``csrc/conditioning.hip`` and, for the two projections of ``SqueezeExcite``, on the k = 1 convolution the transformer block
uses.  No op reads device memory on the host, so a forward can be captured in a graph and replayed.  The ``nn.Linear``
children only hold parameters.

Both modules have two entry points, as the transformer modules have: ``forward`` takes the reference layout (B, L, dim) and
``run_bct`` the channel-major (B, dim, T) that the conv stacks and ``Transformer.run_bct`` work in.  ``FiLM`` is a
memory-bound pass and its kernels take the layout as a flag: nothing is transposed.  ``SqueezeExcite`` is two projections over
the channel dim, which run channel-major: its ``forward`` transposes around ``run_bct`` as ``FeedForward.forward`` does.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import ops
from ._lib import EPI_LEAKY_PRE, FILM_CT, FILM_TC, AgxError, needs_grad
from .transformers import _PackedLinear

Tensor = torch.Tensor


class _StackedLinear:
    """``gamma`` over ``beta`` as one (R, D) weight and one (R,) bias, R = C or 2 C: the image ``ops.film_params`` reads.
    Cached by data pointer and version of the parts, as ``_PackedLinear`` caches its image."""

    def __init__(self, *linears):
        self.linears = linears
        self.key = self.w = self.b = None

    def get(self):
        key = tuple((t.data_ptr(), t._version) for l in self.linears for t in (l.weight, l.bias))
        if key != self.key:
            if len(self.linears) == 1:
                self.w, self.b = self.linears[0].weight.detach(), self.linears[0].bias.detach()
            else:
                self.w = torch.cat([l.weight.detach() for l in self.linears], dim=0)
                self.b = torch.cat([l.bias.detach() for l in self.linears], dim=0)
            self.key = key
        return self.w, self.b


class _FiLMNative(torch.autograd.Function):
    """FiLM forward + backward on the HIP kernels.  Keeps ``x``, ``gb`` and ``condition``; the backward is
    ``film_backward`` (dx and the per-(b, c) sums in one pass over ``x`` and the incoming gradient) and
    ``film_params_backward``, and runs only what ``needs_input_grad`` asks for: ``x`` alone is one ``film_apply`` of the
    incoming gradient with gamma."""

    @staticmethod
    def forward(ctx, film, layout: int, x: Tensor, condition: Tensor, *params: Tensor):
        w, b = film._stacked.get()
        gb = ops.film_params(condition.detach(), w, b)
        out = ops.film_apply(x.detach(), gb, film.bias, layout)
        ctx.film, ctx.layout = film, layout
        ctx.save_for_backward(x, gb, condition)
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        x, gb, condition = ctx.saved_tensors
        film, c = ctx.film, ctx.film.out_dim
        need_x, need_cond, need_p = ctx.needs_input_grad[2], ctx.needs_input_grad[3], ctx.needs_input_grad[4:]
        g = g.contiguous()
        if not (need_cond or any(need_p)):
            gamma = gb[:, :c].contiguous() if film.bias else gb
            return (None, None, ops.film_apply(g, gamma, False, ctx.layout) if need_x else None, None) + (None,) * len(need_p)
        dx, dgb = ops.film_backward(x, gb, g, film.bias, ctx.layout)
        w, _ = film._stacked.get()
        dw, db, dcond = ops.film_params_backward(condition, w, dgb, want_dcond=need_cond)
        grads = [dw[:c], db[:c]] + ([dw[c:], db[c:]] if film.bias else [])      # the order of FiLM.parameters()
        return (None, None, dx if need_x else None, dcond) + tuple(t if need else None for t, need in zip(grads, need_p))


class FiLM(nn.Module):
    """conditioning.py:26-52: ``x * gamma(condition)[:, None, :] + beta(condition)[:, None, :]`` (``bias=False``: no beta).
    ``in_dim`` is the width of the conditioning vector (``self.dim``), ``out_dim`` the channels of ``x``."""

    def __init__(self, in_dim, out_dim=None, bias=True):
        super().__init__()
        self.dim = in_dim
        self.out_dim = out_dim if out_dim is not None else in_dim
        self.gamma = nn.Linear(self.dim, self.out_dim)
        self.bias = bias
        if bias:
            self.beta = nn.Linear(self.dim, self.out_dim)
        self._stacked = _StackedLinear(self.gamma, self.beta) if bias else _StackedLinear(self.gamma)

    def _run(self, x: Tensor, condition: Optional[Tensor], layout: int) -> Tensor:
        if condition is None:
            return x
        if x.dim() != 3:
            raise AgxError(f"FiLM: x is {tuple(x.shape)}, expected " + ("(B, dim, T)" if layout == FILM_CT else "(B, L, dim)"))
        if condition.dim() != 2:
            raise AgxError(f"FiLM: condition is {tuple(condition.shape)}, expected (B, {self.dim}): one vector per batch row")
        channels = x.shape[1] if layout == FILM_CT else x.shape[2]
        if channels != self.out_dim:
            raise AgxError(f"FiLM: x is {tuple(x.shape)} and has {channels} channels, this layer scales {self.out_dim}")
        if condition.shape[0] != x.shape[0] or condition.shape[1] != self.dim:
            raise AgxError(f"FiLM: condition is {tuple(condition.shape)}, expected ({x.shape[0]}, {self.dim})")
        x = x if x.is_contiguous() else x.contiguous()
        if needs_grad(x, self) or (torch.is_grad_enabled() and condition.requires_grad):
            return _FiLMNative.apply(self, layout, x, condition, *self.parameters())
        w, b = self._stacked.get()
        return ops.film_apply(x, ops.film_params(condition, w, b), self.bias, layout)

    def run_bct(self, x: Tensor, condition: Optional[Tensor]) -> Tensor:
        """Channel-major: (B, out_dim, T), (B, in_dim) -> (B, out_dim, T).  ``condition=None`` returns ``x`` itself."""
        return self._run(x, condition, FILM_CT)

    def forward(self, x: Tensor, condition: Optional[Tensor]) -> Tensor:
        """Reference layout: (B, L, out_dim), (B, in_dim) -> (B, L, out_dim), on the same kernels (no transposition)."""
        return self._run(x, condition, FILM_TC)


class _SqueezeExciteNative(torch.autograd.Function):
    """SqueezeExcite forward + hand-written backward: the gate backward, then the k = 1 conv backward of the two
    projections -- the ReLU gradient in the excite layer's bwd-data epilogue (``mask`` = the hidden tensor, slope 0) and the
    gate's direct ``dx`` as ``add`` of the squeeze layer's."""

    @staticmethod
    def forward(ctx, se, x: Tensor, *params: Tensor):
        keep = {}
        out = se._hip_bct(x.detach(), keep)
        ctx.se = se
        ctx.save_for_backward(x, keep["hidden"], keep["z"])
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        x, hidden, z = ctx.saved_tensors
        se = ctx.se
        dx_gate, dz = ops.sigmoid_gate_backward(x, z, g.contiguous())
        dhidden, g_excite = se._excite.backward(hidden, dz, mask=hidden, slope=0.0)
        dx, g_squeeze = se._squeeze.backward(x, dhidden, want_dx=ctx.needs_input_grad[1], add=dx_gate)
        return (None, dx, *g_squeeze, *g_excite)       # the order of SqueezeExcite.parameters()


class SqueezeExcite(nn.Module):
    """conditioning.py:3-24: ``x * sigmoid(excite(relu(squeeze(x))))`` per position, ``hidden_dim = dim // scale_factor``.
    Only the reference's default activations have kernels: ReLU is the squeeze conv's LeakyReLU epilogue at slope 0 and the
    sigmoid lives in the gate kernel."""

    def __init__(self, dim, scale_factor=2, first_activation=nn.ReLU(), second_activation=nn.Sigmoid()):
        super().__init__()
        if type(first_activation) is not nn.ReLU or type(second_activation) is not nn.Sigmoid:
            raise NotImplementedError("only ReLU then Sigmoid (the reference's defaults) are fused into the SqueezeExcite kernels")
        if dim // scale_factor == 0:
            raise ValueError(f"dim = {dim} with scale_factor = {scale_factor} leaves no hidden channel (dim // scale_factor == 0)")
        self.scale_factor = scale_factor
        self.dim = dim
        self.hidden_dim = dim // scale_factor
        self.squeeze = nn.Linear(dim, self.hidden_dim)
        self.excite = nn.Linear(self.hidden_dim, dim)
        self.first_activation = first_activation
        self.second_activation = second_activation
        self._squeeze, self._excite = _PackedLinear(self.squeeze), _PackedLinear(self.excite)

    def _hip_bct(self, x: Tensor, keep: Optional[dict] = None) -> Tensor:
        """The three launches: squeeze conv with the ReLU epilogue, excite conv, gate.  ``keep`` receives what the backward reads."""
        hidden = self._squeeze.forward(x, EPI_LEAKY_PRE, slope=0.0)
        z = self._excite.forward(hidden)
        if keep is not None:
            keep.update(hidden=hidden, z=z)
        return ops.sigmoid_gate(x, z)

    def run_bct(self, x: Tensor) -> Tensor:
        """Channel-major: (B, dim, T) -> (B, dim, T)."""
        if x.dim() != 3 or x.shape[1] != self.dim:
            raise AgxError(f"SqueezeExcite: x is {tuple(x.shape)}, expected (B, {self.dim}, T)")
        x = x if x.is_contiguous() else x.contiguous()
        if needs_grad(x, self):
            return _SqueezeExciteNative.apply(self, x, *self.parameters())
        return self._hip_bct(x)

    def forward(self, x: Tensor) -> Tensor:
        """Reference layout: (B, L, dim) -> (B, L, dim)."""
        if x.dim() != 3 or x.shape[2] != self.dim:
            raise AgxError(f"SqueezeExcite: x is {tuple(x.shape)}, expected (B, L, {self.dim})")
        return self.run_bct(x.transpose(1, 2).contiguous()).transpose(1, 2).contiguous()
