"""The unit of a conv stack, and the plumbing the conv layers of ``vae.py`` and ``wavelets.py`` share.

A stack (``model.encoders`` / ``model.decoders``) is a list of *units*, each one fused forward call.  Every layer type says which
units it is (its ``units(act)`` method, ``act`` = the activation that follows it in the enclosing ``Sequential``);
``CausalVQAE._units`` concatenates them.  That list is the single description of a stack: inference walks it, the native backward
(``native_backward.py``) walks it in reverse, the long-form planner (``longform.py``) reads its ``primitives()``.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
from torch import nn

from . import ops
from ._lib import IMPL_AUTO

Tensor = torch.Tensor


def leaky_slope(act: Optional[nn.Module]) -> Optional[float]:
    """Negative slope if ``act`` is an activation the kernels fuse."""
    if act is None or isinstance(act, nn.Identity):
        return None
    if isinstance(act, nn.LeakyReLU):
        return float(act.negative_slope)
    if isinstance(act, nn.ReLU):
        return 0.0
    raise NotImplementedError(
        f"activation {type(act).__name__} has no HIP kernel (LeakyReLU / ReLU are fused into the convs)")


def refuse_training_dropout(layer: nn.Module, drop: nn.Dropout) -> None:
    """The conv stacks have no dropout kernel: a layer built with ``dropout > 0`` runs in eval mode (dropout is the identity
    there, the path is the one of ``dropout = 0``) and refuses a training-mode call."""
    if drop.p > 0 and drop.training:
        raise ops.AgxError(f"{type(layer).__name__}: dropout = {drop.p} in training mode has no kernel (it runs in eval mode, "
                           "where dropout is the identity) -- there is no ATen fallback")


def detached(t: Optional[Tensor]) -> Optional[Tensor]:
    """A parameter as the kernels take it (an absent bias stays ``None``)."""
    return None if t is None else t.detach()


def packed_image(holder: nn.Module, op: str, kind: int, **desc) -> Tensor:
    """Packed image of ``holder``'s weights for ``ops.conv_pack`` / ``ops.conv_pack_bwd`` (``op``), one per direction, rebuilt
    when the layer kind, the arithmetic (``impl``) or ``data_ptr`` / ``_version`` of the source tensors change (optimizer step,
    ``load_state_dict``, ``.to(device)``).  ``holder`` has ``weights()`` and the conv attributes; ``desc``: the trailing fields of
    the nominal descriptor the image is packed with."""
    v, g = holder.weights()
    key = (kind, desc.get("impl", IMPL_AUTO)) + tuple(k for t in (v, g) if t is not None for k in (t.data_ptr(), t._version))
    slot = holder.__dict__.setdefault("_images", {})
    if op not in slot or slot[op][0] != key:
        nominal = ops.conv_desc(kind, 1, holder.in_channels, holder.out_channels, 1 << 20, holder.kernel_size[0],
                                holder.stride[0], holder.dilation[0], **desc)
        slot[op] = (key, getattr(ops, op)(nominal, v.detach(), detached(g)))
    return slot[op][1]


class Unit:
    """One fused forward call of a stack.  Frozen when the list is built: order, kind and the two slopes.  Read when it runs:
    the layers' ``impl``, parameters and biases, ``CausalResidualBlock1d.split_launches``."""

    def __init__(self, kind: str, layer: nn.Module, convs: Sequence[nn.Module], slope: Optional[float],
                 inner_slope: Optional[float] = None, no_backward: Optional[str] = None, bare: bool = False):
        self.kind = kind                # "conv" | "res" | "resdw" | "wavelet" | "multires"
        self.layer = layer              # the module that runs the unit: the conv, the residual block, the wavelet / multires layer
        self.convs = list(convs)        # [layer], [conv1, conv2] or [depthwise, conv1, conv2]: what the backward walks
        self.slope = slope              # activation after the unit (None = linear output)
        self.inner_slope = inner_slope  # activation inside a residual unit
        self.no_backward = no_backward  # None, or why the backward kernels do not cover the unit (it still runs at inference)
        self.bare = bare                # a conv that is a stack member of its own: inference runs it as its plain forward()

    def forward(self, x: Tensor) -> Tensor:
        return self.layer.run_fused(x, self.slope)

    def params(self) -> List[Tensor]:
        return [p for c in self.convs for p in c.params()]

    def primitives(self) -> List[tuple]:
        """The layers that move information along time, in execution order: ``("causal", k, stride, dilation)`` /
        ``("convt", k, stride)`` / ``("up", k, stride)`` / ``("wavelet", k_in, scale, n_points, k_out)`` / ``("multires", k, depth)``."""
        return [p for c in self.convs for p in c.primitives()]
