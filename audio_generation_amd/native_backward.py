"""Native backward of the conv stacks on the HIP kernels.

A stack (``model.encoders`` / ``model.decoders``) is a list of *units* (``units.py``; ``CausalVQAE._units``):

* conv unit      ``y = act(conv(x) + b)``             (act optional)
* residual unit  ``y = act(x + conv2(act(conv1(x) + b1)) + b2)``
* depthwise residual unit  ``y = act(x + conv2(act(conv1(dw(x)) + b1)) + b2)`` with ``dw`` the per-channel k = 1 conv
  of ``vae.py:103-105`` (grouped-conv backward kernels of ``conv_grouped_bwd.hip``)
* wavelet unit   ``y = act(conv_out(fold(conv_in(x))))``  (``WaveletLayer.backward_native``)
* multires unit  the cascade of ``CausalMultiresConv1d`` (``agx_multires_backward``)

Forward runs the usual fused kernels and keeps every unit's input.  Backward walks the
units in reverse with three C-ABI ops per conv:

* ``agx_conv_bwd_data``   -- gradient w.r.t. the unit input; the residual branch is added and
  the LeakyReLU gradient of the *producing* unit is applied in the same kernel's epilogue
  (mask = the saved activation), so the gradient that travels between units is always the
  one w.r.t. the pre-activation;
* ``agx_conv_bwd_weight`` -- dv / dg / dbias (weight-norm chain rule included);
* (``SAVE_HIDDEN = False`` only) one ``agx_conv_forward`` per residual unit to re-materialise the hidden activation the
  fused forward kernel never wrote.

A stack containing a unit without backward kernels (``Unit.no_backward``: an activation the kernels do not fuse) raises
``AgxError`` when a gradient is asked for: there is no ATen fallback.
"""
from __future__ import annotations

from typing import List

import torch

from . import ops
from ._lib import CONV_CAUSAL, EPI_LEAKY_PRE, IMPL_AUTO, AgxError
from .units import Unit, detached

# Training forward of a residual unit: True = conv1 and conv2 as two launches that leave the hidden activation in
# HBM for the backward (one C x L tensor per block: +3.5 GB at config S, batch 32); False = the fused inference
# kernel, and the backward re-materialises the hidden activation with one more conv launch (6 % slower step).
SAVE_HIDDEN = True

Tensor = torch.Tensor


def _vg(conv):
    v, g = conv.conv.weights()
    return v.detach(), detached(g)


def _grads_of(conv, x: Tensor, dz: Tensor) -> List[Tensor]:
    """[dv, dg, dbias] / [dweight, dbias] in the order of ``_Unit.params``."""
    v, g = _vg(conv)
    dv, dg, db = ops.conv_bwd_weight(conv.desc(x.shape), x, dz, v, g, want_bias=conv.conv.bias is not None)
    out = [dv] if g is None else [dv, dg]
    if db is not None:
        out.append(db)
    return out


def _dw_weight(conv) -> Tensor:
    """Effective (C, 1, 1) weight of the weight-normed per-channel conv: g v / |v| (a C-element parameter fold)."""
    v, g = _vg(conv)
    return v if g is None else v * (g / v.abs().clamp_min(1e-30))


def _dw_desc(conv, x: Tensor):
    return conv.desc(x.shape, impl=IMPL_AUTO)      # whatever family the layer's forward is pinned to


def _dw_grads(conv, x: Tensor, du: Tensor) -> List[Tensor]:
    """[dv, dg, dbias] / [dweight, dbias] of the per-channel conv: ``agx_conv_grouped_bwd_weight`` + the weight-norm chain
    rule on the C-element parameter vectors (for a 1-element direction v: dg = dw sign(v), dv = 0 up to rounding)."""
    v, g = _vg(conv)
    dw, db = ops.conv_grouped_bwd_weight(_dw_desc(conv, x), x, du, want_bias=conv.conv.bias is not None)
    if g is None:
        out = [dw]
    else:
        n = v.abs().clamp_min(1e-30)
        dot = dw * v
        out = [(g / n) * (dw - v * dot / (n * n)), dot / n]
    if db is not None:
        out.append(db)
    return out


class _NativeStack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, units: List[Unit], x: Tensor, *params: Tensor):
        ctx.units = units
        inputs, hidden = [], []
        with torch.no_grad():
            for u in units:
                inputs.append(x)
                if u.kind == "res" and SAVE_HIDDEN:
                    # conv1 and conv2 as two launches: the hidden activation the backward needs is written once
                    # here instead of being re-materialised there (the fused inference kernel never writes it)
                    c1, c2 = u.convs
                    h = c1.run(x, EPI_LEAKY_PRE, u.inner_slope)
                    epi = ops.EPI_RESIDUAL | (ops.EPI_LEAKY_POST if u.slope is not None else 0)
                    x = c2.run(h, epi, u.slope or 0.0, res=x)
                    hidden.append(h)
                else:
                    x = u.forward(x)
        ctx.n_inputs = len(inputs)
        ctx.save_for_backward(*inputs, *hidden)
        ctx.mark_non_differentiable()
        return x

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        units, inputs = ctx.units, ctx.saved_tensors[:ctx.n_inputs]
        hidden = list(ctx.saved_tensors[ctx.n_inputs:])
        if units[-1].slope is not None:
            raise NotImplementedError("a stack ending in an activation needs its output saved for the mask")
        dz = grad_out.contiguous()                    # gradient w.r.t. the last unit's linear output
        grads: List[List[Tensor]] = [None] * len(units)
        for i in range(len(units) - 1, -1, -1):
            u, x = units[i], inputs[i]
            # the unit that produced x (if any) applied an activation: fold its gradient into dx
            prev_slope = units[i - 1].slope if i > 0 else None
            mask = x if prev_slope is not None else None
            if u.kind == "wavelet":
                dz, grads[i] = u.layer.backward_native(x, dz, mask, prev_slope or 0.0)
            elif u.kind == "multires":
                if mask is not None:
                    raise AgxError("a multires unit behind an activation has no fused mask (the blocks place it behind a linear conv)")
                m = u.layer
                dz, dh0, dh1, dw = ops.multires_backward(x, dz, m.h0.detach(), m.h1.detach(), m.w.detach(), m.depth)
                grads[i] = [dh0, dh1, dw]
            elif u.kind == "conv":
                conv = u.layer
                grads[i] = _grads_of(conv, x, dz)
                dz = ops.conv_bwd_data(conv.desc(x.shape), dz, conv.conv.packed_bwd(conv.kind), None, mask,
                                       prev_slope or 0.0)
            elif u.kind == "resdw":
                dwc, c1, c2 = u.convs
                ux = dwc.run(x)                                           # re-materialised: one bandwidth-bound launch
                h = c1.run(ux, EPI_LEAKY_PRE, u.inner_slope)
                g2 = _grads_of(c2, h, dz)
                dh = ops.conv_bwd_data(c2.desc(h.shape), dz, c2.conv.packed_bwd(CONV_CAUSAL), None, h, u.inner_slope)
                g1 = _grads_of(c1, ux, dh)
                du = ops.conv_bwd_data(c1.desc(ux.shape), dh, c1.conv.packed_bwd(CONV_CAUSAL))
                g0 = _dw_grads(dwc, x, du)
                dz = ops.conv_grouped_bwd_data(_dw_desc(dwc, x), du, _dw_weight(dwc), None, dz, mask, prev_slope or 0.0)
                grads[i] = g0 + g1 + g2
            else:
                c1, c2 = u.convs
                # the hidden activation: saved by the forward, or re-materialised with one conv launch
                h = hidden.pop() if hidden else c1.run(x, EPI_LEAKY_PRE, u.inner_slope)
                g2 = _grads_of(c2, h, dz)
                dh = ops.conv_bwd_data(c2.desc(h.shape), dz, c2.conv.packed_bwd(CONV_CAUSAL), None, h, u.inner_slope)
                g1 = _grads_of(c1, x, dh)
                dz = ops.conv_bwd_data(c1.desc(x.shape), dh, c1.conv.packed_bwd(CONV_CAUSAL), dz, mask,
                                       prev_slope or 0.0)
                grads[i] = g1 + g2
        flat = [g for gl in grads for g in gl]
        return (None, dz, *flat)


def run_stack(units: List[Unit], x: Tensor) -> Tensor:
    for u in units:
        if u.no_backward:
            raise AgxError(f"no backward kernels for {u.no_backward} (activation or layer type the HIP kernels do not "
                           "cover); there is no ATen fallback")
    params = [p for u in units for p in u.params()]
    return _NativeStack.apply(units, x, *params)
