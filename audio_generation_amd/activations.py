"""Drop-in ``Snek`` / ``SnekReLU`` executed by libagx: the snake activations with one learnable alpha per channel.

Mirrors ``networks/utils.py:44-105`` (class names, constructor arguments, the parameter ``alphas`` and its ``state_dict()``
key, the two functions and their signatures).  Everything is fp32; forward and backward run on the kernels of
``csrc/snake.hip``.  ``x`` is (B, C, T) for ``dim=1`` and (B, C, H, W) for ``dim=2`` -- the channel-major layout the conv
stacks and ``Transformer.run_bct`` work in, so there is one entry point and nothing is transposed.  No op reads device memory
on the host and the backward's workspace comes from the torch allocator: forward and backward can be captured in a graph.
"""
from __future__ import annotations

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import ops
from ._lib import SNAKE_PLAIN, SNAKE_RELU, AgxError

Tensor = torch.Tensor


class _SnakeNative(torch.autograd.Function):
    """Forward and backward on the HIP kernels.  Keeps ``x`` and ``alpha``; the backward is one ``ops.snake_backward`` that is
    asked only for what ``needs_input_grad`` wants: frozen alphas give the element-wise ``dx`` kernel with no reduction, an
    input without a gradient gives the sums alone."""

    @staticmethod
    def forward(ctx, x: Tensor, alpha: Tensor, variant: int, eps: float):
        ctx.variant, ctx.eps = variant, eps
        ctx.save_for_backward(x, alpha)
        return ops.snake_forward(x.detach(), alpha.detach(), variant, eps)

    @staticmethod
    @once_differentiable
    def backward(ctx, g: Tensor):
        x, alpha = ctx.saved_tensors
        need_x, need_alpha = ctx.needs_input_grad[:2]
        dx, dalpha = ops.snake_backward(x, alpha.detach(), g.contiguous(), ctx.variant, ctx.eps, want_dx=need_x,
                                        want_dalpha=need_alpha)
        return dx, None if dalpha is None else dalpha.view(alpha.shape), None, None


def _snake(name: str, x: Tensor, alpha: Tensor, variant: int, eps: float) -> Tensor:
    if x.dim() < 3 or alpha.numel() not in (1, x.shape[1]) or alpha.dim() not in (0, x.dim()) or \
            (alpha.dim() and alpha.shape[1] != alpha.numel()):
        raise AgxError(f"{name}: x is {tuple(x.shape)} and alpha {tuple(alpha.shape)}: expected x (B, C, T) or (B, C, H, W) and "
                       "one alpha per channel, (1, C, 1) or (1, C, 1, 1), or a single alpha")
    x = x if x.is_contiguous() else x.contiguous()
    if torch.is_grad_enabled() and (x.requires_grad or alpha.requires_grad):
        return _SnakeNative.apply(x, alpha, variant, eps)
    return ops.snake_forward(x, alpha, variant, eps)


def snake_activation(x: Tensor, alpha: Tensor, eps: float = 1e-6) -> Tensor:
    """utils.py:44-59: ``x + sin(alpha x)^2 / (alpha + eps)``; ``alpha`` broadcasts over batch and positions."""
    return _snake("snake_activation", x, alpha, SNAKE_PLAIN, eps)


def snake_relu_activation(x: Tensor, alpha: Tensor, eps: float = 1e-6) -> Tensor:
    """utils.py:61-73: ``clamp(x, 0) + sin(alpha x)^2 / (alpha + eps)``; the gradient of the clamp at 0 is 1, as torch's."""
    return _snake("snake_relu_activation", x, alpha, SNAKE_RELU, eps)


class Snek(nn.Module):
    """utils.py:75-89: the snake activation with a learnable alpha per channel, initialised to ones.  ``dim=1``: x is
    (B, C, T), ``dim=2``: (B, C, H, W).  ``in_channels=1`` is one alpha for every channel, as the reference's broadcast."""

    _activation = staticmethod(snake_activation)

    def __init__(self, in_channels, dim=1):
        super().__init__()
        if dim == 1:
            self.alphas = nn.Parameter(torch.ones(1, in_channels, 1))
        elif dim == 2:
            self.alphas = nn.Parameter(torch.ones(1, in_channels, 1, 1))
        else:
            raise ValueError("Snek cannot handle such dims")

    def forward(self, x: Tensor) -> Tensor:
        name, c = type(self).__name__, self.alphas.shape[1]
        if x.dim() != self.alphas.dim():
            raise AgxError(f"{name}: x is {tuple(x.shape)}, expected " + ("(B, C, T)" if self.alphas.dim() == 3 else "(B, C, H, W)"))
        if c != 1 and x.shape[1] != c:
            raise AgxError(f"{name}: x is {tuple(x.shape)} and has {x.shape[1]} channels, this layer holds {c} alphas")
        return self._activation(x, self.alphas)


class SnekReLU(Snek):
    """utils.py:91-105: as ``Snek`` on ``clamp(x, 0)``."""

    _activation = staticmethod(snake_relu_activation)
