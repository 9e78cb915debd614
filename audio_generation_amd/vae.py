"""Drop-in ``CausalVQAE`` and its causal conv modules, executed by libagx.

Same class names, constructor arguments, attribute names, forward signatures
and ``state_dict()`` keys as the reference's ``networks/vae.py`` (cited per
class), so the reference's training / sampling callers (``training.py:325-328,
488-500, 502-516``; ``utils.py:238-259``) keep working -- but no ATen conv is
called: every layer runs as a hand-written HIP kernel behind the C ABI of
``include/agx.h``.  The module tree exists for parameters and checkpoints;
``forward`` walks it and issues fused launches (residual block = one call,
activation / padding / crop / upsample folded into the conv kernels).

Differentiation: forward AND backward run on libagx (``native_backward.py``: conv
backward-data / weight-gradient kernels incl. the ``depthwise=True`` block variant, the RVQ
straight-through pass).  No ATen arithmetic op is differentiated anywhere: a configuration
without backward kernels (an activation the kernels do not fuse, ``norm != Identity``)
raises ``AgxError`` / ``NotImplementedError`` instead of falling back.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch
from torch import nn

from . import ops
from ._lib import (CONV_CAUSAL, CONV_PADDED, CONV_TRANSPOSED, CONV_UPSAMPLE, EPI_LEAKY_POST, EPI_LEAKY_PRE,
                   IMPL_AUTO, IMPL_MFMA_BF16X3, AgxError, needs_grad)
from .native_backward import run_stack
from .units import Unit, detached, leaky_slope, packed_image, refuse_training_dropout

Tensor = torch.Tensor


def tuple_checker(item, length):
    """Same contract as the reference helper (networks/utils.py:212-220; also
    re-exported by the external quantiser module, vae.py:6)."""
    if isinstance(item, (int, float, str)):
        item = [item] * length
    elif isinstance(item, (tuple, list)):
        assert len(item) == length, f"Expected tuple of length {length}, got {len(item)}"
    return item


class _ConvParams(nn.Module):
    """Parameter holder standing where the reference has a weight-normed
    ``torch.nn.Conv1d`` / ``ConvTranspose1d`` (``add_util_norm``, utils.py:34-42):
    parameters ``weight_g`` (dim0,1,1), ``weight_v`` and ``bias`` under the same
    names, initialised the way torch initialises a conv + ``weight_norm``.
    With ``norm != "weight"`` it holds a plain ``weight``.
    """

    def __init__(self, c_in: int, c_out: int, kernel: int, stride: int, dilation: int, bias: bool,
                 transposed: bool, norm: str = "weight", groups: int = 1):
        super().__init__()
        self.in_channels, self.out_channels = c_in, c_out
        self.kernel_size, self.stride, self.dilation = (kernel,), (stride,), (dilation,)
        self.transposed = transposed
        self.groups = groups
        shape = (c_in, c_out, kernel) if transposed else (c_out, c_in // groups, kernel)
        w = torch.empty(shape)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        fan_in = shape[1] * kernel
        bias_p = None
        if bias:
            bound = 1.0 / math.sqrt(fan_in)
            bias_p = nn.Parameter(torch.empty(c_out).uniform_(-bound, bound))
        if norm == "weight":
            # registration order of torch's weight_norm(Conv1d): bias, weight_g, weight_v -- ``parameters()`` order is
            # what an index-based optimizer state of the reference (trainer_state.pkl, training.py:225-242) refers to
            self.register_parameter("bias", bias_p)
            self.weight_g = nn.Parameter(w.reshape(shape[0], -1).norm(dim=1).reshape(-1, 1, 1))
            self.weight_v = nn.Parameter(w)
        elif norm == "spectral":
            raise NotImplementedError("spectral norm is only used by the discriminators (out of scope)")
        else:
            self.weight = nn.Parameter(w)
            self.register_parameter("bias", bias_p)

    def weights(self):
        """(direction, gain) of the weight-normed layer, (weight, None) of a plain one."""
        return (self.weight_v, self.weight_g) if hasattr(self, "weight_v") else (self.weight, None)

    def packed_bwd(self, kind: int) -> Tensor:
        """Packed image of the layer's backward-data op (same invalidation rule as ``packed``)."""
        return packed_image(self, "conv_pack_bwd", kind)

    def packed(self, kind: int, impl: int = IMPL_AUTO) -> Tensor:
        """Packed (weight-norm folded) image, rebuilt when the parameters change.  The bf16x3 kernels have their own image."""
        return packed_image(self, "conv_pack", kind, impl=IMPL_MFMA_BF16X3 if impl == IMPL_MFMA_BF16X3 else IMPL_AUTO,
                            groups=self.groups)


class _ConvBase(nn.Module):
    kind = CONV_CAUSAL
    impl = IMPL_AUTO  # tests override to pin a kernel family
    _primitive = {CONV_CAUSAL: "causal", CONV_TRANSPOSED: "convt", CONV_UPSAMPLE: "up"}

    def desc(self, shape, epilogue: int = 0, slope: float = 0.1, impl: Optional[int] = None):
        """The layer's descriptor for an input of ``shape`` (B, C, L); ``impl`` overrides the layer's own (the nominal
        bf16x3 query of ``set_conv_arithmetic``, the grouped k = 1 layer's backward, which is always ``IMPL_AUTO``)."""
        c = self.conv
        return ops.conv_desc(self.kind, shape[0], c.in_channels, c.out_channels, shape[2], c.kernel_size[0], c.stride[0],
                             c.dilation[0], epilogue, slope, self.impl if impl is None else impl, groups=c.groups)

    def run(self, x: Tensor, epilogue: int = 0, slope: float = 0.1, res: Optional[Tensor] = None) -> Tensor:
        c = self.conv
        if x.dim() != 3 or x.shape[1] != c.in_channels:
            raise AgxError(f"{type(self).__name__}: expected (B,{c.in_channels},L), got {tuple(x.shape)}")
        return ops.conv_forward(self.desc(x.shape, epilogue, slope), x, c.packed(self.kind, self.impl), detached(c.bias), res)

    def run_fused(self, x: Tensor, post_slope: Optional[float] = None) -> Tensor:
        """``act(conv(x))`` with the activation folded into the kernel."""
        return self.run(x, EPI_LEAKY_PRE if post_slope is not None else 0, post_slope or 0.0)

    def forward(self, x: Tensor) -> Tensor:
        return self.run(x)

    def units(self, act: Optional[nn.Module] = None) -> List[Unit]:
        return [Unit("conv", self, [self], leaky_slope(act), bare=act is None)]

    def params(self) -> List[Tensor]:
        """[weight_v, weight_g, bias] / [weight, bias]: the order of the gradients ``native_backward`` returns."""
        return [p for p in (*self.conv.weights(), self.conv.bias) if p is not None]

    def primitives(self) -> List[tuple]:
        c = self.conv
        k, s, d = c.kernel_size[0], c.stride[0], c.dilation[0]
        if self.kind == CONV_PADDED:       # the grouped k = 1 conv moves nothing along time
            if k != 1 or s != 1:
                raise NotImplementedError("receptive_field: grouped conv with kernel > 1")
            return []
        if self.kind not in self._primitive:
            raise NotImplementedError(f"receptive_field: conv kind {self.kind}")
        return [(self._primitive[self.kind], k, s) + ((d,) if self.kind == CONV_CAUSAL else ())]


class CausalConv1d(_ConvBase):
    """networks/vae.py:14-43."""
    kind = CONV_CAUSAL

    def __init__(self, in_channels, out_channels, kernel_size, dilation=1, stride=1, bias=True,
                 groups=1, norm="weight"):
        super().__init__()
        if groups != 1:
            # the one grouped use in the reference: the k = 1 depthwise conv of vae.py:103 -- no padding at all,
            # so it is the grouped AGX_CONV_PADDED layer (direct kernel)
            if kernel_size != 1 or stride != 1 or dilation != 1:
                raise NotImplementedError("grouped causal convs are wired for kernel 1 / stride 1 only (vae.py:103)")
            self.kind = CONV_PADDED
        self.conv = _ConvParams(in_channels, out_channels, kernel_size, stride, dilation, bias, False, norm, groups)
        self.dilation = dilation
        self.pad = dilation * (kernel_size - 1) - stride + 1  # vae.py:32


class CausalConvT1d(_ConvBase):
    """networks/vae.py:45-64."""
    kind = CONV_TRANSPOSED

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, bias=True, norm="weight"):
        super().__init__()
        self.conv = _ConvParams(in_channels, out_channels, kernel_size, stride, 1, bias, True, norm)
        self.right_pad = kernel_size - stride


class CausalUpsampleConv1d(_ConvBase):
    """networks/vae.py:66-89 (nearest upsample + ``padding="same"`` conv; not
    causal in the reference either).  Runs as ``stride`` polyphase 3-tap filters
    on the low-rate signal -- the upsampled tensor is never materialised."""
    kind = CONV_UPSAMPLE

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, bias=True, norm="weight"):
        super().__init__()
        self.scale_factor = stride
        self.conv = _ConvParams(in_channels, out_channels, kernel_size, stride, 1, bias, False, norm)


class CausalResidualBlock1d(nn.Module):
    """networks/vae.py:91-117: ``x + conv_k1(act(conv_k7,dil(x)))``."""
    # profiling aid: issue the two convs as separate C-ABI calls (same kernels) so a
    # launch observer can time them one by one
    split_launches = False

    def __init__(self, in_channels, out_channels, kernel_size=7, dilation=1, bias=True,
                 activation=None, dropout=0.0, depthwise=False):
        super().__init__()
        if in_channels != out_channels:
            raise AgxError("residual block needs in_channels == out_channels (as the reference's add does)")
        self.depthwise = depthwise
        if depthwise:   # vae.py:103-105: a per-channel k = 1 conv in front of the dilated conv (three launches, unfused)
            self.conv1 = nn.Sequential(CausalConv1d(in_channels, in_channels, 1, bias=bias, groups=in_channels),
                                       CausalConv1d(in_channels, out_channels, kernel_size, dilation=dilation, bias=bias))
        else:
            self.conv1 = CausalConv1d(in_channels, out_channels, kernel_size, dilation=dilation, bias=bias)
        self.conv2 = CausalConv1d(out_channels, out_channels, 1, bias=bias)
        self.activation = nn.LeakyReLU(0.1) if activation is None else activation
        self.dropout = nn.Dropout(dropout)

    def run(self, x: Tensor, post_slope: Optional[float] = None) -> Tensor:
        """Whole block (+ the activation that follows it in the enclosing
        ``Sequential`` when ``post_slope`` is given) through ``agx_resblock_forward``."""
        refuse_training_dropout(self, self.dropout)
        slope = leaky_slope(self.activation)
        if self.depthwise:
            h = self.conv1[1].run(self.conv1[0].run(x), EPI_LEAKY_PRE if slope is not None else 0, slope or 0.0)
            if slope is None:
                h = self.activation(h)
            epi = ops.EPI_RESIDUAL | (EPI_LEAKY_POST if post_slope is not None else 0)
            return self.conv2.run(h, epi, post_slope or 0.0, res=x)
        if self.split_launches or slope is None or (post_slope is not None and post_slope != slope):
            # exotic activation mix: two convs with separate epilogues
            h = self.conv1.run(x, EPI_LEAKY_PRE if slope is not None else 0, slope or 0.0)
            epi = ops.EPI_RESIDUAL | (EPI_LEAKY_POST if post_slope is not None else 0)
            return self.conv2.run(h, epi, post_slope or 0.0, res=x)
        c1, c2, impl = self.conv1.conv, self.conv2.conv, self.conv1.impl
        return ops.resblock_forward(self.conv1.desc(x.shape, 0, slope), x, c1.packed(CONV_CAUSAL, impl), detached(c1.bias),
                                    c2.packed(CONV_CAUSAL, impl), detached(c2.bias), post_act=post_slope is not None)

    run_fused = run

    def takes_quads(self, shape, post_slope: Optional[float]) -> bool:
        """``run`` on a ``shape`` = (B, C, L) input would be ONE ``ops.resblock_forward`` call, and the library has the
        channel-quad variants of its kernel (``agx_resblock_q4_supported``)."""
        slope = leaky_slope(self.activation)
        if self.depthwise or self.split_launches or slope is None or (post_slope is not None and post_slope != slope):
            return False
        return ops.resblock_q4_supported(self.conv1.desc(shape, 0, slope))

    def run_quads(self, x: Tensor, post_slope: Optional[float], x_is_q4: bool, y_is_q4: bool) -> Tensor:
        """``run`` of a block that ``takes_quads``, its input and / or output in channel quads ``(B, C / 4, L, 4)``."""
        refuse_training_dropout(self, self.dropout)
        c1, c2, impl = self.conv1.conv, self.conv2.conv, self.conv1.impl
        shape = (x.shape[0], x.shape[1] * 4, x.shape[2]) if x_is_q4 else x.shape
        return ops.resblock_forward_q4(self.conv1.desc(shape, 0, leaky_slope(self.activation)), x, c1.packed(CONV_CAUSAL, impl),
                                       detached(c1.bias), c2.packed(CONV_CAUSAL, impl), detached(c2.bias),
                                       post_act=post_slope is not None, x_is_q4=x_is_q4, y_is_q4=y_is_q4)

    def forward(self, x: Tensor) -> Tensor:
        return self.run(x, None)

    def units(self, act: Optional[nn.Module] = None) -> List[Unit]:
        """One unit; a block whose own activation the kernels do not fuse (``nn.Identity``) runs, and has no backward."""
        refuse_training_dropout(self, self.dropout)
        inner = leaky_slope(self.activation)
        convs = [*self.conv1, self.conv2] if self.depthwise else [self.conv1, self.conv2]
        return [Unit("resdw" if self.depthwise else "res", self, convs, leaky_slope(act), inner,
                     None if inner is not None else f"a residual block around {type(self.activation).__name__}")]


def _default_act():
    return nn.LeakyReLU(0.1)


class CausalEncoderBlock(nn.Module):
    """networks/vae.py:119-148."""

    def __init__(self, in_channels, out_channels, stride, n_layers=4, activation=None, depthwise=False, multires=None):
        super().__init__()
        activation = _default_act() if activation is None else activation
        layers = [nn.Sequential(CausalResidualBlock1d(in_channels, in_channels, dilation=3 ** i,
                                                      depthwise=depthwise), activation)
                  for i in range(n_layers - 1)]
        # multires = (kernel_size, depth): BUILD-DEFINED placement of CausalMultiresConv1d (the reference imports it at vae.py:7
        # and never wires it) -- right behind the strided conv, its GELU in place of the block's activation there
        layers.append(nn.Sequential(CausalConv1d(in_channels, out_channels, 2 * stride + 1, stride=stride),
                                    nn.Identity() if multires else activation))
        self.layers = nn.ModuleList(layers)
        if multires:
            from .wavelets import CausalMultiresConv1d
            self.multires = CausalMultiresConv1d(out_channels, multires[0], multires[1])

    def units(self, act: Optional[nn.Module] = None) -> List[Unit]:
        return [u for m, a in (*self.layers, *_multires_pair(self)) for u in m.units(a)]

    def forward(self, x: Tensor) -> Tensor:
        return _run_units(self.units(), x)


class CausalDecoderBlock(nn.Module):
    """networks/vae.py:150-202."""

    def __init__(self, in_channels, out_channels, stride, n_layers=4, activation=None, depthwise=False,
                 upsample=True, wavelet=False, wavelet_hidden_ratio=4, channelwise=True, multires=None):
        super().__init__()
        activation = _default_act() if activation is None else activation
        self.wavelet = wavelet
        if wavelet:
            from .wavelets import WaveletLayer
            conv_layer = WaveletLayer(in_channels, out_channels * wavelet_hidden_ratio,
                                      out_channels=out_channels, scale_factor=stride,
                                      wavelet_kernel_size=2 * stride + 1,
                                      n_points=2 * stride * wavelet_hidden_ratio,
                                      channelwise_scale=channelwise)
        elif upsample:
            conv_layer = CausalUpsampleConv1d(in_channels, out_channels, 2 * stride + 1, stride=stride)
        else:
            conv_layer = CausalConvT1d(in_channels, out_channels, 2 * stride + 1, stride=stride)
        self.in_conv = nn.Sequential(conv_layer, nn.Identity() if multires else activation)
        if multires:   # build-defined placement, as in CausalEncoderBlock: behind the resampling layer, GELU instead of the activation
            from .wavelets import CausalMultiresConv1d
            self.multires = CausalMultiresConv1d(out_channels, multires[0], multires[1])
        self.layers = nn.ModuleList([
            nn.Sequential(CausalResidualBlock1d(out_channels, out_channels, dilation=3 ** i,
                                                depthwise=depthwise), activation)
            for i in range(n_layers - 1)])

    def units(self, act: Optional[nn.Module] = None) -> List[Unit]:
        return [u for m, a in (self.in_conv, *_multires_pair(self), *self.layers) for u in m.units(a)]

    def forward(self, x: Tensor) -> Tensor:
        return _run_units(self.units(), x)


def _multires_pair(block: nn.Module):
    """The block's build-defined multires layer as a (layer, activation) pair like the block's ``Sequential``s, if it has one."""
    return [(block.multires, None)] if hasattr(block, "multires") else []


def _run_units(units: Sequence[Unit], x: Tensor, quads: bool = True) -> Tensor:
    """Inference walk.  A bare conv runs as its ``forward()``, a conv behind ``nn.Identity`` as ``run_fused(x, None)``: the same
    launch, but the descriptor's slope field (unread without an epilogue) is 0.1 in the one and 0.0 in the other, and 0.0 in
    the training forward of both -- kept as recorded in tests/golden/stack_launch_trace.json.

    ``quads``: a run of two or more consecutive residual blocks that all have the channel-quad variants of the fp32 ring kernel
    (include/agx.h; ``takes_quads``) passes its activation from block to block in quads -- the first block writes them, the
    last one reads them; same values bit for bit.  Device tensors without autograd only: everything else (and ``quads=False``:
    long-form) makes the plain calls."""
    i, n = 0, len(units)
    quads = quads and x.is_cuda and x.dim() == 3 and not torch.is_grad_enabled()
    while i < n:
        u = units[i]
        j = i
        if quads and u.kind == "res":   # a run of residual blocks that all have the channel-quad variants
            while j < n and units[j].kind == "res" and units[j].layer.takes_quads(x.shape, units[j].slope):
                j += 1
        if j - i >= 2:   # the activation BETWEEN the blocks travels in channel quads (include/agx.h): same kernels' arithmetic
            for k in range(i, j):
                x = units[k].layer.run_quads(x, units[k].slope, x_is_q4=k > i, y_is_q4=k < j - 1)
            i = j
        else:
            x = u.layer(x) if u.bare else u.forward(x)
            i += 1
    return x


class CausalVQAE(nn.Module):
    """networks/vae.py:204-351 -- same constructor, attributes and methods."""

    def __init__(self, in_channels=1, n_blocks=5, n_layers_per_block=4, first_block_channels=32,
                 num_quantizers=8, codebook_size=1024, codebook_dim=512, vq_cutoff_freq=1,
                 vq_type="ema", strides=(2, 3, 4, 4, 5), input_format="b l c", channel_multiplier=2,
                 norm=nn.Identity, depthwise=False, use_som=True, som_kernel_type="hard",
                 wavelet_decoders=(False, True, False, False, False),
                 multires_encoders=False, multires_decoders=False, multires_kernel_size=2, multires_depth=3):
        """The last four arguments are BUILD-DEFINED (default off: the reference's model): block i gets a
        ``CausalMultiresConv1d(channels, multires_kernel_size, multires_depth)`` (wavelets.py:38-96 -- imported by the
        reference at vae.py:7 and never wired) right behind its strided / upsampling conv, whose GELU takes the place of the block
        activation there; lists are in encoder order resp. decoder order.  BASELINE config 4 ("multiresolution / wavelet layers in
        encoder + decoder") at model level; oracle: oracle/codec.py CodecSpec."""
        super().__init__()
        from .quantizer import ResidualQuantizer

        self.in_channels = in_channels
        self.n_blocks = n_blocks
        self.n_layers_per_block = n_layers_per_block
        self.num_quantizers = num_quantizers
        self.vq_cutoff_freq = vq_cutoff_freq
        self.codebook_dim = codebook_dim
        self.codebook_size = tuple_checker(codebook_size, num_quantizers)
        self.strides = tuple_checker(strides, n_blocks)
        self.scale_factor = int(math.prod(int(s) for s in self.strides))
        self.input_format = input_format

        if isinstance(wavelet_decoders, (list, tuple)):
            assert len(wavelet_decoders) == n_blocks, "Number of wavelet decoders must match number of blocks."
            self.wavelet_decoders = list(wavelet_decoders)[::-1]  # vae.py:240: iterated backwards
        else:
            self.wavelet_decoders = [wavelet_decoders] * n_blocks

        self.quantizer = ResidualQuantizer(num_quantizers=num_quantizers, dim=codebook_dim,
                                           quantizer_class=vq_type, codebook_sizes=codebook_size,
                                           vq_cutoff_freq=vq_cutoff_freq, use_som=use_som,
                                           som_kernel_type=som_kernel_type)

        self.multires_encoders = list(tuple_checker(multires_encoders, n_blocks))
        self.multires_decoders = list(tuple_checker(multires_decoders, n_blocks))
        mr = (multires_kernel_size, multires_depth)
        ch = [first_block_channels * channel_multiplier ** i for i in range(n_blocks + 1)]
        encoders: List[nn.Module] = [nn.Sequential(norm(), CausalConv1d(in_channels, first_block_channels, 7))]
        for i in range(n_blocks):
            encoders.append(CausalEncoderBlock(ch[i], ch[i + 1], self.strides[i], n_layers_per_block,
                                               depthwise=depthwise, multires=mr if self.multires_encoders[i] else None))
        encoders.append(CausalConv1d(ch[-1], codebook_dim, 3))

        decoders: List[nn.Module] = [CausalConvT1d(codebook_dim, ch[-1], 7)]
        for i in range(n_blocks, 0, -1):
            decoders.append(CausalDecoderBlock(ch[i], ch[i - 1], self.strides[i - 1],
                                               n_layers=n_layers_per_block, depthwise=depthwise,
                                               wavelet=self.wavelet_decoders[i - 1],
                                               multires=mr if self.multires_decoders[n_blocks - i] else None))
        decoders.append(CausalConv1d(first_block_channels, in_channels, 7))

        self.encoders = nn.ModuleList(encoders)
        self.decoders = nn.ModuleList(decoders)

    # -- arithmetic of the conv stacks (build-defined; the reference has fp32 only) ------------------
    def set_conv_arithmetic(self, decoders: str = "fp32", encoders: str = "fp32") -> "CausalVQAE":
        """``"fp32"``: the fp32-input MFMA kernels (bitwise an fp32 FMA chain).  ``"bf16x3"``: operands split into three
        bf16 pieces on the bf16 MFMA -- the same error against fp64 as fp32 (tools/bf16x3_accuracy.py), 1.3-1.5x
        faster, but not the bitwise fp32 chain.  The default keeps the ENCODER exact (it decides the RVQ indices)
        and is what every parity statement refers to; ``bench.py`` reports which setting it ran."""
        for stack, mode in ((self.decoders, decoders), (self.encoders, encoders)):
            if mode not in ("fp32", "bf16x3"):
                raise ValueError(f"unknown arithmetic {mode!r}")
            in_block = {id(c_) for blk in stack.modules() if isinstance(blk, CausalResidualBlock1d)
                        for c_ in blk.modules() if isinstance(c_, _ConvBase)}
            for m in stack.modules():
                if isinstance(m, _ConvBase):
                    c = m.conv
                    q = c.stride[0] if m.kind in (CONV_TRANSPOSED, CONV_UPSAMPLE) else 1
                    ok = mode == "bf16x3" and c.in_channels % 16 == 0 and q * c.out_channels >= 32 and c.groups == 1
                    # resampling convs: bf16x3 where the layer has the ring form (conv_b3.hip: the decoder's up-convs and
                    # the k = 7 transposed conv) or where the first-round bf16x3 kernel beats the fp32 ring kernel (the
                    # stride-4 down-conv; tools/layer_times.py bf16x3); the others stay on the fp32 ring, which is at least as exact
                    if ok and id(m) not in in_block:
                        nominal = m.desc((1, c.in_channels, 4096), EPI_LEAKY_PRE, 0.1, IMPL_MFMA_BF16X3)
                        ok = ops.conv_kernel_name(nominal).startswith("conv_b3") or (m.kind == CONV_CAUSAL and c.stride[0] == 4)
                    m.impl = IMPL_MFMA_BF16X3 if ok else IMPL_AUTO
        self.__dict__.pop("_unit_cache", None)
        return self

    # -- layout helpers (vae.py:283-288) ------------------------------------------------
    def rearrange_in(self, x: Tensor) -> Tensor:
        return x.transpose(1, 2).contiguous() if self.input_format == "b l c" else x

    def rearrange_out(self, x: Tensor) -> Tensor:
        return x.transpose(1, 2).contiguous() if self.input_format == "b l c" else x

    def _encoders_hip(self, x: Tensor, quads: bool = True) -> Tensor:
        return _run_units(self._units("encoders"), x, quads)

    def _decoders_hip(self, x: Tensor, quads: bool = True) -> Tensor:
        x, units = self._decoder_head_on_planes(x, self._units("decoders"))
        return _run_units(units, x, quads)

    def _decoder_head_on_planes(self, x: Tensor, decs):
        """bf16x3 decoders, inference: the k = 7 transposed conv (vae.py:269) writes its output as ACTIVATION PLANES
        (include/agx.h: the three bf16 pieces of every element, split once in the producer's epilogue) and the first
        block's polyphase up-conv (vae.py:176-179; M = 8 x 256 rows = 16 row blocks that each re-split the same input
        tile otherwise) stages them by LDS-DMA.  Bit-identical to the fp32-activation path (same pieces, same products,
        same order: tests/test_gpu_conv_b3.py, test_gpu_fullsize.py); any other configuration takes the plain path.
        ``decs``: the decoder units; returns the activation and the units still to run."""
        if torch.is_grad_enabled() or len(decs) < 2 or x.dim() != 3 or decs[0].kind != "conv" or decs[1].kind != "conv":
            return x, decs
        head, up, slope = decs[0].layer, decs[1].layer, decs[1].slope
        if not (head.kind == CONV_TRANSPOSED and up.kind == CONV_UPSAMPLE and head.impl == up.impl == IMPL_MFMA_BF16X3
                and decs[0].slope is None and x.shape[1] % 8 == 0 and (len(decs) < 3 or decs[2].kind != "multires")):
            return x, decs
        d0 = head.desc(x.shape)
        if head.conv.stride[0] != 1 or ops.conv_planes_supported(d0) != 2:
            return x, decs
        d1 = up.desc((x.shape[0], None, ops.conv_out_len(d0)), EPI_LEAKY_PRE if slope is not None else 0, slope or 0.0)
        if ops.conv_planes_supported(d1) < 1:
            return x, decs
        xp = ops.planes_split(x)                                             # the RVQ's output: 15 MB at config S
        yp = ops.conv_forward_planes(d0, xp, head.conv.packed(head.kind, head.impl), detached(head.conv.bias), out_planes=True)
        return ops.conv_forward_planes(d1, yp, up.conv.packed(up.kind, up.impl), detached(up.conv.bias)), decs[2:]

    def _run_encoders(self, x: Tensor) -> Tensor:
        """Encoder stack; when a gradient is needed, forward + backward on the HIP kernels (native_backward.py)."""
        return run_stack(self._units("encoders"), x) if needs_grad(x, self.encoders) else self._encoders_hip(x)

    def _run_decoders(self, x: Tensor) -> Tensor:
        return run_stack(self._units("decoders"), x) if needs_grad(x, self.decoders) else self._decoders_hip(x)

    def _units(self, which: str) -> List[Unit]:
        """Unit list of ``self.encoders`` / ``self.decoders``: the ONE description of a stack.  Inference, the native backward
        and ``longform.receptive_field`` all read it.  Built by the first call that reaches the stack and cached; what is
        frozen then is the order of the units, their kinds and their slopes -- ``set_conv_arithmetic`` drops the cache, and so
        must whoever rewires a stack by hand.  A layer's ``impl``, parameters and biases, ``split_launches`` and
        ``torch.is_grad_enabled()`` (the planes head) are read by every call.  A unit without backward kernels is listed
        (inference runs it); ``run_stack`` raises for it when a gradient is asked for."""
        cache = self.__dict__.setdefault("_unit_cache", {})
        if which not in cache:
            units: List[Unit] = []
            for m in getattr(self, which):
                if isinstance(m, nn.Sequential):      # encoders[0]: Sequential(norm(), conv)
                    if len(m) != 2 or not isinstance(m[0], nn.Identity):
                        raise NotImplementedError("only norm=Identity (the reference default) has HIP kernels")
                    m = m[1]
                if not hasattr(m, "units"):
                    raise NotImplementedError(f"no HIP path for {type(m).__name__}")
                units += m.units()
            cache[which] = units
        return cache[which]

    def encode(self, x, update_codebook=False, codebook_n=None, prioritize_early=False, *, stages=None):
        """vae.py:307-322 -> (x_q (B,C,T), commit_loss, index (B,T,Q)).  ``stages`` (build-defined): an int64 (B,)
        device tensor, one stage count per batch row -- quantiser dropout in training (``quantizer.dropout_stages``), a per-row
        bitrate in eval; index is -1 at the stages a row does not use."""
        z = self._run_encoders(self.rearrange_in(x))  # (B, D, T)
        q = self.quantizer
        if hasattr(q, "quantize_bcl"):
            # native quantiser: reads and writes the (B,D,T) layout directly, no transposes
            staged = {} if stages is None else {"stages": stages}
            zq, index, commit = q.quantize_bcl(z, codebook_n, update_codebook=update_codebook,
                                               prioritize_early=prioritize_early, **staged)
        elif stages is not None:
            raise NotImplementedError(f"stages= needs the native quantiser: {type(q).__name__} has no quantize_bcl, and the "
                                      "reference call contract (vae.py:315-318) has no per-row stage count")
        else:
            # any replacement bottleneck honouring the reference call contract (vae.py:315-318)
            zq, index, commit = q(z.transpose(1, 2), codebook_n, update_codebook=update_codebook,
                                  prioritize_early=prioritize_early)
            zq = zq.transpose(1, 2).contiguous()
        return zq, commit, index

    def forward(self, x, update_codebook=False, codebook_n=None, prioritize_early=False, *, stages=None):
        """vae.py:293-305 -> (y, commit_loss, index).  ``stages``: as ``encode``."""
        zq, commit, index = self.encode(x, update_codebook, codebook_n, prioritize_early, stages=stages)
        y = self.rearrange_out(self._run_decoders(zq))
        return y, commit, index

    def decode(self, zq: Tensor) -> Tensor:
        """Decoder half of ``forward`` on (B, D, T) quantised latents."""
        return self.rearrange_out(self._run_decoders(zq))

    # -- time-folded long-clip inference (build-defined; longform.py) ----------------------------
    def encode_long(self, x, segment_frames=None, codebook_n=None):
        """``encode`` of long clips with the time axis folded into the batch: overlapping windows of ``segment_frames``
        kept latent frames (plus the receptive-field halos) run as one batch through the encoder kernels, the RVQ
        runs once on the stitched latents.  Same return contract as ``encode``; inference only.  A hop that leaves one
        window IS the plain call, and so is ``None`` (folding bounds memory, it was measured not to be faster)."""
        from . import longform
        return longform.encode_long(self, x, segment_frames, codebook_n)

    def decode_long(self, zq: Tensor, segment_frames=None) -> Tensor:
        """``decode`` on (B, D, T) quantised latents, folded the same way with the decoder's halos."""
        from . import longform
        return longform.decode_long(self, zq, segment_frames)

    def forward_long(self, x, segment_frames=None, codebook_n=None):
        """``forward`` in eval mode through ``encode_long`` / ``decode_long`` -> (y, commit_loss, index)."""
        from . import longform
        return longform.forward_long(self, x, segment_frames, codebook_n)

    # -- streaming on per-layer conv state rings (build-defined; streaming.py) -------------------
    def new_stream(self, batch: int, max_chunk: int = 4, device=None, wavelet_blocks: bool = False, multires_layers: bool = False,
                   depthwise_blocks: bool = False):
        """A ``CodecStream`` for ``batch`` live streams that advance by 1 .. ``max_chunk`` latent frames per call.
        ``wavelet_blocks=True``: wavelet decoder blocks stream too; without it such a model is refused.
        ``multires_layers=True`` / ``depthwise_blocks=True``: likewise the multires layers and the residual blocks built with
        ``depthwise=True``."""
        from . import streaming
        return streaming.CodecStream(self, batch, max_chunk, device, wavelet_blocks, multires_layers, depthwise_blocks)

    def encode_stream(self, x_chunk, stream, codebook_n=None, counts=None):
        """``encode`` of the next ``n`` whole frames of every row -> (zq (B, D, n), commit_loss, index (B, n, Q)); the conv state
        is carried in ``stream``, the quantiser is stateless per frame.  Inference only.  ``counts`` (int64 (B,), device): row
        ``b`` takes the first ``clamp(counts[b], 0, n)`` frames of the chunk (``streaming``: per-row frame counts)."""
        from . import streaming
        return streaming.encode_stream(self, x_chunk, stream, codebook_n, counts)

    def decode_stream(self, zq_chunk: Tensor, stream, counts=None) -> Tensor:
        """Decoder on the next ``n`` frames of (B, D, n) quantised latents -> ``n * scale_factor`` samples per row in the model's
        output format: the block that lags the input by ``stream.decoder_delay`` samples, zeros before the stream's start.
        ``counts``: as in ``encode_stream``; the samples behind a row's count are exact 0."""
        from . import streaming
        return streaming.decode_stream(self, zq_chunk, stream, counts)

    def forward_stream(self, x_chunk, stream, codebook_n=None, counts=None):
        """``encode_stream`` then ``decode_stream`` -> (y, commit_loss, index)."""
        from . import streaming
        return streaming.forward_stream(self, x_chunk, stream, codebook_n, counts)

    def decode_flush(self, stream, rows=None) -> Tensor:
        """After ``stream.finish()``: the zero-frame steps that bring the decoder's delayed tail out.  ``rows``: only those rows
        receive the flush frames; the others stay where they are."""
        from . import streaming
        return streaming.decode_flush(self, stream, rows)

    def sample(self, length=225, device="cuda", normal_var=5e3, n_iters=12):
        """vae.py:324-345: random codes -> dequantise -> decode."""
        self.to(device)
        self.eval()
        with torch.no_grad():
            x = None
            for i in range(self.num_quantizers):
                idx = torch.randint(0, self.codebook_size[0], (1, length), device=device)
                x_i = self.quantizer.quantizers[i].dequantize(idx)
                x = x_i if x is None else x + x_i
            y = self.rearrange_out(self._run_decoders(x.transpose(1, 2).contiguous()))
        self.train(True)  # the reference unconditionally returns to train mode (vae.py:344)
        return y

    # -- codec wire format (bit budget of utils.py:137-147) ---------------------
    @property
    def _code_bits(self) -> int:
        """Bits per code on the wire: every stage at the widest stage's width."""
        return max(1, (max(int(k) for k in self.codebook_size) - 1).bit_length())

    def compress(self, x, codebook_n=None):
        """Waveform -> (uint8 bitstream, (B, T, Q)).  ceil(log2(K)) bits per code, dense."""
        with torch.no_grad():
            _, _, index = self.encode(x, codebook_n=codebook_n)
        return ops.codes_pack(index, self._code_bits), tuple(index.shape)

    def decompress(self, stream, shape):
        """Inverse of ``compress``: bitstream -> codes -> sum of codewords -> decoder."""
        b, t, q = shape
        index = ops.codes_unpack(stream, b * t * q, self._code_bits).reshape(b, t, q)
        with torch.no_grad():
            zq = None
            for i in range(q):
                zq = ops.rvq_dequantize(self.quantizer.codebooks.detach()[i], index[..., i], out=zq,
                                        accumulate=zq is not None)
            return self.decode(zq.transpose(1, 2).contiguous()), index

    def decode_codes(self, index: Tensor) -> Tensor:
        """Codes -> waveform: index (B, T, q) int64, q <= Q -> ``decode`` of the sum of the codewords of the first q stages, which
        ``ops.codes_embed`` forms in ONE launch (``decompress`` takes one per stage) and in the same stage order.  A ``-1`` -- a
        stage a row does not use (``compress_stream(stages=)``, ``CodePrior.step(stages=)``) -- contributes nothing."""
        cb = self.quantizer.codebooks.detach()
        if not isinstance(index, Tensor) or index.dim() != 3 or not 1 <= index.shape[2] <= cb.shape[0]:
            raise AgxError(f"decode_codes: index must be (B, T, q) with 1 <= q <= {cb.shape[0]}, got "
                           f"{tuple(index.shape) if isinstance(index, Tensor) else type(index).__name__}")
        with torch.no_grad():
            return self.decode(ops.codes_embed(index.contiguous(), cb[:index.shape[2]]))

    def compress_stream(self, x_chunk, stream, codebook_n=None, counts=None, stages=None):
        """The sender's step of a live stream: the next ``n`` whole frames of every row -> (packets (B, P) uint8, index (B, n, Q)),
        ``P = ceil(n Q bits / 8)``.  Row ``b``'s first ``ceil(c_b Q bits / 8)`` bytes are its packet -- ``ops.codes_pack`` of its
        ``c_b = clamp(counts[b], 0, n)`` frames' codes -- and every byte behind them is 0; ``index`` behind the count is -1.  Uses
        only the encoder rings of ``stream``.

        ``stages`` (int64 (B,), device): one bitrate per row.  Row ``b`` sends its first ``q_b = clamp(stages[b], 0, Q)`` stages
        (``stages_for_bitrate``): its packet is ``ceil(c_b q_b bits / 8)`` bytes, dense over its own ``q_b``, ``index`` is -1 at
        the stages it does not send, and ``P`` stays what it is -- one captured step serves any mix of bitrates."""
        from . import streaming
        _, index, packets = streaming.encode_codes_stream(self, x_chunk, stream, codebook_n, counts, stages)
        return packets, index

    def decompress_stream(self, packets, stream, frames, codebook_n=None, counts=None, stages=None):
        """The receiver's step: packet rows of ``frames`` frames (``compress_stream``) -> (y, index), ``y`` as ``decode_stream``
        returns it.  The bytes behind a row's count are not read.  Uses only the decoder rings of ``stream``; ``finish``,
        ``decode_flush`` and ``reset`` are those of any stream.

        ``stages``: the tensor the packets were written with (``compress_stream``, or the one ``restage_packets`` returned).  A
        row with ``c_b > 0`` and ``q_b == 0`` pushes ``c_b`` frames of the zero latent through the decoder and advances."""
        from . import streaming
        return streaming.decode_codes_stream(self, packets, stream, frames, codebook_n, counts, stages)

    def compress_stream_coded(self, x_chunk, stream, coder, coder_state, counts=None, stages=None):
        """``compress_stream`` with the packets entropy-coded under a code prior (``entropy.PriorCoder``) ->
        (packets (B, 2 n Q + 4) uint8, nbytes (B,) int64, index (B, n, Q)).  Row ``b``'s packet is its first ``nbytes[b]`` bytes, 0
        behind them; ``index`` is that of ``compress_stream``.  ``coder_state`` is the sender's ``coder.new_state(...)``; the
        prior's stage count and codebook sizes must be the quantiser's."""
        from . import streaming
        return streaming.encode_coded_stream(self, x_chunk, stream, coder, coder_state, counts, stages)

    def decompress_stream_coded(self, packets, nbytes, stream, coder, coder_state, frames, counts=None, stages=None):
        """The receiver of ``compress_stream_coded``: coded packet rows of ``frames`` frames -> (y, index) as ``decompress_stream``
        returns them, with ``counts`` / ``stages`` the sender's.  ``coder_state`` is the receiver's own ``coder.new_state(...)``;
        ``coder_state.status`` is 0 for every row whose packet decoded cleanly.  Lossless against the dense wire: ``index`` is the
        sender's ``index``."""
        from . import streaming
        return streaming.decode_coded_stream(self, packets, nbytes, stream, coder, coder_state, frames, counts, stages)

    def restage_packets(self, packets, frames, stages, stages_from=None, codebook_n=None, counts=None):
        """A relay's step: packet rows of ``frames`` frames written with ``stages_from`` (None: every stage) -> (packets, stages)
        with row ``b`` at ``min(q_in, clamp(stages[b], 0, Q))`` stages, byte for byte what ``compress_stream`` writes at that
        count.  One launch, no codebooks, no decoding; the returned ``stages`` is written on the device.  Never upward."""
        from . import streaming
        return streaming.restage_packets(self, packets, frames, stages, stages_from, codebook_n, counts)

    def stages_for_bitrate(self, bitrate, sample_rate) -> int:
        """The stages a link of ``bitrate`` bits per second carries at ``sample_rate``: the largest ``q <= num_quantizers`` with
        ``q * _code_bits * sample_rate / scale_factor <= bitrate`` -- ``utils.bitrate_calculator`` solved for the stage count,
        at the width a code has on the wire.  0 when even one stage does not fit.  Host arithmetic."""
        q = 0
        while q < self.num_quantizers and (q + 1) * self._code_bits * sample_rate / self.scale_factor <= bitrate:
            q += 1
        return q

    def replace_quantizer(self, new_quantizer):
        self.quantizer = new_quantizer

    def update_cutoff(self, new_cutoff=None, ratio=None):
        self.quantizer.update_cutoff(new_cutoff=new_cutoff, ratio=ratio)
