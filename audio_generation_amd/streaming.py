"""Streaming codec: chunked encode / decode on per-layer conv state rings.

The conv stacks are causal up to a bounded look-ahead, so a live stream does not have to re-run the receptive field on every hop:
every unit of a stack keeps a ring of its own INPUT, a step of ``n`` latent frames pushes the new columns through the stack with
``ops.conv_stream_step`` (one tap-gather launch per conv, the producer writing straight into the consumer's ring), and the positions
live in device memory, so a step makes no host decision and replays from a captured graph.

* ``plan(model, max_chunk)`` walks ``model._units("encoders" | "decoders")`` -- the list inference, training and ``longform`` read --
  and gives every unit its rate ``r`` (columns per latent frame), left reach ``H``, cumulative delay ``D`` and ring capacity;
  nothing is hard-coded per configuration.
* ``CodecStream`` holds the rings, ``enc_pos`` / ``dec_pos`` / ``end`` (int64 (B,), device), ``max_chunk`` and ``decoder_delay``.

What a stream computes.  A unit's step produces exactly ``n r_out`` columns, the stream indices ``[pos r_out - D_out,
(pos + n) r_out - D_out)``; a column ``j`` is stored as exact 0 unless ``0 <= j < end[b] r_out`` -- the layer's own zero padding in
the plain call, before the start and after the end.  The encoder has no delay (a strided conv looks ``s - 1`` samples ahead, inside
the frame's own samples) and needs no mask.  The decoder's upsampling convs are not causal (``vae.py:66-89``), so its output lags
the input by ``decoder_delay`` samples: ``decode_stream`` returns the raw block of that index rule, zeros where the index is
negative, and ``decode_flush`` pushes the ``ceil(decoder_delay / scale_factor)`` zero frames that bring the tail out.  With the
delay removed, the stream equals the plain call on the whole clip.  Ragged last frames are the caller's: pad the last hop to a
whole frame; the plain call pads every layer instead, so that frame differs.

Per-row frame counts.  Every step takes ``counts=``, a contiguous int64 (B,) device tensor: row ``b`` takes the first
``c_b = clamp(counts[b], 0, n)`` frames of the chunk and advances by ``c_b``; with ``c_b = 0`` nothing of the row changes.  The
kernels read it -- the host never does, so a captured step replays with whatever the tensor holds.  The first ``c_b`` frames of
a row's latents, ``zq`` and waveform are bit for bit those of an uncounted stream fed the same frames; every floating-point output
behind them is exact 0 (NaN in the chunk there reaches no result and no ring).  ``index`` behind the count is the code of the
zero latent and means nothing -- slice by ``counts`` -- and ``commit`` is computed over the whole chunk, zero latents included:
it is not meaningful on a counted call.  ``counts=None`` is the uncounted call, launch for launch.

Packets.  ``encode_codes_stream`` / ``decode_codes_stream`` are the two ends of a wire: the sender's step gives one
packet row per stream, the receiver's step turns packet rows into audio.  Their quantiser is ``ops.rvq_step_encode`` /
``ops.rvq_step_decode``, which read ``counts``: ``index`` behind a row's count is -1 and the packet bytes there are 0.

Wavelet decoder blocks.  ``plan(..., wavelet_blocks=True)`` / ``model.new_stream(..., wavelet_blocks=True)`` stream a
``WaveletLayer`` block as two launches: ``ops.wavelet_stream_in_step`` (``conv_in``, a "same" conv, into a ring of the hidden
activation, ``CodecStream.dec_hidden``) and ``ops.wavelet_stream_out_step`` (``conv_out`` with the fold formed in its operand fetch
from that ring, a per-channel table and the stream's ``end``, which decides the reference's raw tail).  Without the keyword such a
model is refused as before.

Multires layers and depthwise residual blocks.  ``multires_layers=True`` streams a ``CausalMultiresConv1d`` as one
launch (``ops.multires_stream_step``: the whole cascade on the ring of the layer's input); ``depthwise_blocks=True`` streams a
residual block built with ``depthwise=True`` as the two launches of a plain one, the per-channel k = 1 conv formed in the dilated
conv's operand fetch (``ops.conv_stream_step_affine``).  Both are causal: no ring of their own, no delay.  Without the
keywords such models are refused as before.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch

from . import ops
from ._lib import (CONV_CAUSAL, CONV_SAME, CONV_TRANSPOSED, CONV_UPSAMPLE, EPI_LEAKY_POST, EPI_LEAKY_PRE, EPI_RESIDUAL, STREAM_LIVE, AgxError,
                   needs_grad)
from .units import Unit, detached, packed_image

Tensor = torch.Tensor


def _ceil_div(a: int, b: int) -> int:
    return -((-a) // b)


@dataclass(frozen=True)
class UnitPlan:
    """One unit of a stack as a stream runs it.  ``kind``: "causal" | "convt" | "up" | "res" | "resdw" | "wavelet" | "multires";
    ``k, s, d`` of its conv (of the dilated conv of a residual unit; of ``conv_in`` and the fold's scale for a wavelet unit; the
    taps of a multires unit, whose cascade has ``depth`` levels and ``reach = (k - 1)(2^depth - 1)``); ``rate_in`` / ``delay_in`` and
    ``rate_out`` / ``delay_out`` in columns; ``reach``: input columns it reads before the chunk's first new one; ``cap = reach +
    max_chunk * rate_in``: its ring, so that a step's writes never alias the history the step reads.  A wavelet unit (DESIGN
    4.23) has a second ring, of its hidden activation ``h``: ``hidden`` channels at ``rate_in`` columns per frame, lagging by
    ``delay_h``, ``reach_h`` columns of history, capacity ``cap_h``; ``k_out``: the taps of ``conv_out``."""
    kind: str
    c_in: int
    c_out: int
    k: int
    s: int
    d: int
    rate_in: int
    delay_in: int
    rate_out: int
    delay_out: int
    reach: int
    cap: int
    hidden: int = 0
    k_out: int = 0
    delay_h: int = 0
    reach_h: int = 0
    cap_h: int = 0
    depth: int = 0


@dataclass(frozen=True)
class StreamPlan:
    scale_factor: int
    max_chunk: int
    encoders: tuple
    decoders: tuple

    @property
    def decoder_delay(self) -> int:
        """Samples by which the decoder's output lags its input."""
        return self.decoders[-1].delay_out

    @property
    def flush_frames(self) -> int:
        return _ceil_div(self.decoder_delay, self.scale_factor)

    @property
    def enc_left(self) -> int:
        """Input samples before a frame's first that the encoder reads: ``longform.receptive_field(model).enc_left``."""
        return sum(u.reach * (self.scale_factor // u.rate_in) for u in self.encoders)


_REFUSED_UNITS = {
    "wavelet": "a wavelet decoder block streams only when asked for: new_stream(..., wavelet_blocks=True)",
    "multires": "a multiresolution layer has no streaming step",
    "resdw": "a depthwise residual block (depthwise=True) has no streaming step",
}


def _wavelet_plan(u: Unit, rate: int, delay: int, max_chunk: int) -> UnitPlan:
    """include/agx.h "Streaming wavelet blocks": D_h = D + p_in, D_out = D_h s + s + p_out; reach k_in - 1 in the input ring and
    1 + ceil(2 p_out / s) in the ring of h."""
    w = u.layer
    k_in, k_out, s = w.wavelet_kernel_size, w.out_conv_kernel_size, w.scale_factor
    if k_in % 2 == 0 or k_out % 2 == 0:
        raise NotImplementedError(f"streaming: a wavelet block with even conv kernels ({k_in}, {k_out}) pads unevenly and has no step")
    if s < 2:
        raise NotImplementedError(f"streaming: a wavelet block with scale_factor {s} < 2 has no step")
    delay_h = delay + (k_in - 1) // 2
    reach_h = 1 + _ceil_div(k_out - 1, s)
    return UnitPlan("wavelet", w.in_channels, w.out_channels, k_in, s, 1, rate, delay, rate * s, delay_h * s + s + (k_out - 1) // 2,
                    k_in - 1, k_in - 1 + max_chunk * rate, w.hidden_channels, k_out, delay_h, reach_h, reach_h + max_chunk * rate)


def _multires_plan(u: Unit, rate: int, delay: int, max_chunk: int) -> UnitPlan:
    """include/agx.h "Streaming multires layers and depthwise residual blocks": causal, per channel, rate and delay unchanged;
    reach (K - 1)(2^depth - 1) in the ring of its input."""
    m = u.layer
    if u.slope is not None:
        raise NotImplementedError("streaming: a multires layer with an activation behind its GELU has no step")
    reach = ops.multires_stream_reach(m.kernel_size, m.depth)
    if not ops.multires_stream_fits(m.kernel_size, m.depth, max_chunk * rate):
        raise NotImplementedError(f"streaming: a multires layer with reach {reach} (kernel {m.kernel_size}, depth {m.depth}) at "
                                  f"{max_chunk * rate} columns per step does not fit the step kernel's "
                                  f"{ops.MULTIRES_STREAM_LDS_BYTES} bytes of LDS")
    return UnitPlan("multires", m.channels, m.channels, m.kernel_size, 1, 1, rate, delay, rate, delay, reach, reach + max_chunk * rate,
                    depth=m.depth)


def _unit_plan(u: Unit, rate: int, delay: int, max_chunk: int, wavelet_blocks: bool = False, multires_layers: bool = False,
               depthwise_blocks: bool = False) -> UnitPlan:
    if u.kind == "wavelet" and wavelet_blocks:
        return _wavelet_plan(u, rate, delay, max_chunk)
    if u.kind == "multires" and multires_layers:
        return _multires_plan(u, rate, delay, max_chunk)
    resdw = u.kind == "resdw" and depthwise_blocks
    if u.kind in _REFUSED_UNITS and not resdw:
        raise NotImplementedError(f"streaming: {_REFUSED_UNITS[u.kind]}; use the plain or the *_long calls")
    if u.kind not in ("conv", "res") and not resdw:
        raise NotImplementedError(f"streaming: no step for a unit of kind {u.kind!r}")
    main = u.convs[1 if resdw else 0]          # a depthwise block's convs: [per-channel k = 1, dilated, k = 1]
    c = main.conv
    k, s, d = c.kernel_size[0], c.stride[0], c.dilation[0]
    layer_kind = main.kind
    if resdw:
        dw = u.convs[0].conv
        if dw.groups != dw.in_channels or dw.in_channels != dw.out_channels or dw.kernel_size[0] != 1 or dw.stride[0] != 1:
            raise NotImplementedError("streaming: the first conv of a depthwise residual block is a per-channel k = 1 conv")
    if u.kind == "res" or resdw:
        c2 = u.convs[-1].conv
        if u.inner_slope is None:
            raise NotImplementedError("streaming: a residual block around an activation the kernels do not fuse")
        if layer_kind != CONV_CAUSAL or s != 1 or c2.kernel_size[0] != 1 or c2.stride[0] != 1:
            raise NotImplementedError("streaming: a residual block is a stride-1 causal conv and a k = 1 conv")
        kind, reach, rate_out, delay_out = u.kind, d * (k - 1), rate, delay
    elif layer_kind == CONV_CAUSAL:
        reach = d * (k - 1) - s + 1
        if rate % s or delay % s:
            raise NotImplementedError(f"streaming: a stride-{s} conv at {rate} columns per frame and delay {delay} leaves no whole columns")
        if reach < 0:
            raise NotImplementedError(f"streaming: a causal conv with stride {s} > dilation (k - 1) + 1")
        kind, rate_out, delay_out = "causal", rate // s, delay // s
    elif layer_kind == CONV_TRANSPOSED:
        if s != 1:
            raise NotImplementedError(f"streaming: a transposed conv with stride {s} > 1 has no streaming step (the decoder blocks "
                                      "upsample with CausalUpsampleConv1d)")
        kind, reach, rate_out, delay_out = "convt", k - 1, rate, delay
    elif layer_kind == CONV_UPSAMPLE:
        if k != 2 * s + 1:
            raise NotImplementedError(f"streaming: an upsampling conv with kernel {k} != 2 * stride + 1")
        kind, reach, rate_out, delay_out = "up", 2, rate * s, delay * s + s
    else:
        raise NotImplementedError(f"streaming: conv kind {layer_kind} has no streaming step")
    return UnitPlan(kind, c.in_channels, u.convs[-1].conv.out_channels, k, s, d, rate, delay, rate_out, delay_out, reach,
                    reach + max_chunk * rate)


def plan(model, max_chunk: int, wavelet_blocks: bool = False, multires_layers: bool = False,
         depthwise_blocks: bool = False) -> StreamPlan:
    """Derived from the model's unit lists as they are wired; raises ``NotImplementedError`` for what a stream does not cover.
    ``wavelet_blocks``: plan the wavelet decoder blocks instead of refusing them; ``multires_layers`` /
    ``depthwise_blocks``: likewise the multires layers and the depthwise residual blocks."""
    from .quantizer import ResidualQuantizer
    max_chunk = int(max_chunk)
    if max_chunk < 1:
        raise AgxError(f"streaming: max_chunk = {max_chunk} < 1")
    if not isinstance(model.quantizer, ResidualQuantizer):
        raise NotImplementedError(f"streaming: the bottleneck {type(model.quantizer).__name__} is not a ResidualQuantizer (the "
                                  "quantiser is stateless per frame; an attention bottleneck needs its own cache wired in)")
    sf = int(model.scale_factor)
    stacks = []
    for which, rate in (("encoders", sf), ("decoders", 1)):
        delay, out = 0, []
        for u in model._units(which):
            p = _unit_plan(u, rate, delay, max_chunk, wavelet_blocks, multires_layers, depthwise_blocks)
            out.append(p)
            rate, delay = p.rate_out, p.delay_out
        if rate != (1 if which == "encoders" else sf):
            raise NotImplementedError(f"streaming: the {which} leave {rate} columns per frame, scale_factor is {sf}")
        stacks.append(tuple(out))
    if stacks[0][-1].delay_out != 0:
        raise NotImplementedError("streaming: an encoder with a delay")
    return StreamPlan(sf, max_chunk, stacks[0], stacks[1])


class CodecStream:
    """The state of ``batch`` live streams through one ``CausalVQAE`` (``model.new_stream``): per unit one fp32 ring
    (B, c_in, cap) of its input, zero-filled; ``enc_pos`` / ``dec_pos``: the frames every row's encoder / decoder has received;
    ``end``: the frame at which a row's stream ended, ``ops.STREAM_LIVE`` while it is live.  All int64 (B,) on the device, read by
    the kernels and advanced by a kernel.  ``decoder_delay``: samples by which ``decode_stream``'s output lags.
    ``wavelet_blocks=True``: the wavelet decoder blocks stream too; ``dec_hidden[i]`` is the ring (B, hidden, cap_h)
    of unit ``i``'s hidden activation, None for every other unit -- ``dec_rings`` stays one ring per unit.
    ``multires_layers=True`` / ``depthwise_blocks=True``: those units stream too, on the ring of their input alone."""

    def __init__(self, model, batch: int, max_chunk: int, device=None, wavelet_blocks: bool = False, multires_layers: bool = False,
                 depthwise_blocks: bool = False):
        batch = int(batch)
        if batch < 1:
            raise AgxError(f"new_stream: batch = {batch} < 1")
        self.plan = plan(model, max_chunk, wavelet_blocks, multires_layers, depthwise_blocks)
        self.model_id = id(model)
        self.batch, self.max_chunk = batch, self.plan.max_chunk
        self.scale_factor, self.decoder_delay = self.plan.scale_factor, self.plan.decoder_delay
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        self.enc_rings = [torch.zeros((batch, u.c_in, u.cap), dtype=torch.float32, device=self.device) for u in self.plan.encoders]
        self.dec_rings = [torch.zeros((batch, u.c_in, u.cap), dtype=torch.float32, device=self.device) for u in self.plan.decoders]
        self.dec_hidden = [torch.zeros((batch, u.hidden, u.cap_h), dtype=torch.float32, device=self.device) if u.kind == "wavelet"
                           else None for u in self.plan.decoders]
        self.enc_pos = torch.zeros(batch, dtype=torch.int64, device=self.device)
        self.dec_pos = torch.zeros(batch, dtype=torch.int64, device=self.device)
        self.end = torch.full((batch,), STREAM_LIVE, dtype=torch.int64, device=self.device)

    def _rows(self, rows, what: str) -> Optional[List[int]]:
        """``rows`` as checked ints (None: every row)."""
        return None if rows is None else [sel.start for sel in ops._row_slices(what, rows, self.batch, "stream")]

    def finish(self, rows=None) -> None:
        """The streams of ``rows`` (default: every row) end at the frames their decoders have received: ``end[r] = dec_pos[r]``,
        on the device.  What the decoder produces past that frame is the plain call's zero padding; ``decode_flush`` brings the
        delayed tail out."""
        rows = self._rows(rows, "finish")
        ops.stream_mark_end(self.dec_pos, self.end,
                            None if rows is None else torch.tensor(rows, dtype=torch.int64).to(self.device))

    def reset(self, rows=None) -> None:
        """``rows`` (default: every row) start a new stream at their next call: positions to 0, ``end`` to live and those rows of
        every ring to zero, all device fills.  Call it between steps, outside any captured graph."""
        for sel in ops._row_slices("reset", rows, self.batch, "stream"):
            self.enc_pos[sel].zero_()
            self.dec_pos[sel].zero_()
            self.end[sel].fill_(STREAM_LIVE)
            for ring in (*self.enc_rings, *self.dec_rings, *self.dec_hidden):
                if ring is not None:
                    ring[sel].zero_()

    def positions(self) -> dict:
        """The positions as lists of ints.  Synchronises: for tests and debugging, never called in a step."""
        return {"enc_pos": self.enc_pos.tolist(), "dec_pos": self.dec_pos.tolist(), "end": self.end.tolist()}


# --------------------------------------------------------------------------- the step
def _image(layer) -> Tensor:
    return packed_image(layer.conv, "conv_stream_pack", layer.kind)


def _run_stack(units: List[Unit], plans, rings: List[Tensor], x: Tensor, pos: Tensor, end: Optional[Tensor], n: int,
               counts: Optional[Tensor] = None, hidden: Optional[List[Optional[Tensor]]] = None) -> Tensor:
    """``n`` frames through a stack: the chunk into the first ring, one or two step launches per unit, the last unit into a plain
    tensor, then the advance of ``pos``.  ``counts``: the same launches in their counted forms (None: the uncounted ones).
    ``hidden``: per unit the ring of a wavelet unit's hidden activation (None: the stack has no such unit)."""
    b = x.shape[0]
    ops.ring_write_rate(rings[0], x, pos, plans[0].rate_in, counts=counts)
    out = None
    for i, (u, p) in enumerate(zip(units, plans)):
        last = i + 1 == len(units)
        dst = torch.empty((b, p.c_out, n * p.rate_out), dtype=torch.float32, device=x.device) if last else rings[i + 1]
        if p.kind == "wavelet":
            out = run_unit(u, p, rings[i], dst, not last, pos, end, n, counts, hidden=hidden[i])
        else:
            out = run_unit(u, p, rings[i], dst, not last, pos, end, n, counts)
    ops.stream_advance(pos, n, counts=counts)
    return out


def fold_table(layer) -> Tensor:
    """The out-step's per-channel table of a ``WaveletLayer`` (``ops.wavelet_fold_table``), kept on the layer and rebuilt when
    ``data_ptr`` / ``_version`` of ``wavelet_scale`` change -- the rule of ``units.packed_image``."""
    sig = layer.wavelet_scale
    key = (sig.data_ptr(), sig._version, layer.space.data_ptr())
    slot = layer.__dict__.get("_fold_table")
    if slot is None or slot[0] != key:
        slot = (key, ops.wavelet_fold_table(layer.space, sig.detach(), layer.hidden_channels, layer.scale_factor))
        layer.__dict__["_fold_table"] = slot
    return slot[1]


def depthwise_affine(layer) -> tuple:
    """(scale, shift) of a depthwise residual block's per-channel k = 1 conv ``layer`` for ``ops.conv_stream_step_affine``: the
    weight-norm folded weights as the plain call's image holds them (row ``c`` of the grouped image, ``ops.conv_pack``) and the
    bias (zeros without one).  Kept on the layer and rebuilt when ``data_ptr`` / ``_version`` of its parameters change -- the rule
    of ``units.packed_image`` -- so that a changed weight is seen and a captured step keeps its pointers."""
    c = layer.conv
    v, g = c.weights()
    key = tuple(k for t in (v, g, c.bias) if t is not None for k in (t.data_ptr(), t._version))
    slot = layer.__dict__.get("_stream_affine")
    if slot is None or slot[0] != key:
        n = c.in_channels
        image = c.packed(layer.kind)                         # ((g J + j) M + m) x 16 with one channel per group: row m, column 0
        scale = image[:n * 16].reshape(n, 16)[:, 0].contiguous()
        shift = c.bias.detach() if c.bias is not None else torch.zeros_like(scale)
        slot = (key, (scale, shift))
        layer.__dict__["_stream_affine"] = slot
    return slot[1]


def run_unit(u: Unit, p: UnitPlan, ring: Tensor, dst: Tensor, dst_ring: bool, pos: Tensor, end: Optional[Tensor], n: int,
             counts: Optional[Tensor] = None, hidden: Optional[Tensor] = None) -> Tensor:
    """One unit's step: ``ring`` -> ``dst``.  A conv is one launch; a residual unit is two, its hidden activation (which only the
    k = 1 conv at the same column reads, so it needs no mask and no history) in a plain scratch tensor.  ``counts``: the counted
    launches (the hidden activation is exact 0 behind a row's count).  A wavelet unit is two: the in-step into ``hidden``, the
    ring of its hidden activation, and the out-step, which folds on the fly.  A multires unit is one launch; a
    depthwise residual unit is the two of a plain one, the first with the per-channel affine in its operand fetch."""
    post = u.slope
    if p.kind == "wavelet":
        w = u.layer
        if hidden is None:
            raise AgxError("streaming: a wavelet unit needs the ring of its hidden activation (CodecStream.dec_hidden)")
        ops.wavelet_stream_in_step(p.c_in, p.hidden, p.k, packed_image(w.conv_in, "conv_stream_pack", CONV_SAME), detached(w.conv_in.bias),
                                   ring, hidden, pos, end, n, p.rate_in, p.delay_in, counts=counts)
        return ops.wavelet_stream_out_step(p.hidden, p.c_out, p.k_out, p.s, packed_image(w.conv_out, "conv_stream_pack", CONV_SAME),
                                           detached(w.conv_out.bias), fold_table(w), hidden, dst, pos, end, n, p.rate_in, p.delay_h,
                                           dst_ring=dst_ring, epilogue=EPI_LEAKY_PRE if post is not None else 0, slope=post or 0.0,
                                           counts=counts)
    if p.kind == "multires":
        m = u.layer
        return ops.multires_stream_step(m.h0.detach(), m.h1.detach(), m.w.detach(), p.depth, ring, dst, pos, n, p.rate_in, p.delay_in,
                                        dst_ring=dst_ring, end=end, counts=counts)
    if p.kind in ("res", "resdw"):
        c1, c2 = u.convs[-2], u.convs[-1]
        hid = torch.empty((ring.shape[0], c1.conv.out_channels, n * p.rate_in), dtype=torch.float32, device=ring.device)
        if p.kind == "resdw":
            scale, shift = depthwise_affine(u.convs[0])
            ops.conv_stream_step_affine(p.c_in, c1.conv.out_channels, p.k, p.d, _image(c1), detached(c1.conv.bias), scale, shift, ring, hid,
                                        pos, n, p.rate_in, p.delay_in, dst_ring=False, epilogue=EPI_LEAKY_PRE, slope=u.inner_slope,
                                        counts=counts)
        else:
            ops.conv_stream_step(CONV_CAUSAL, p.c_in, c1.conv.out_channels, p.k, 1, p.d, _image(c1), detached(c1.conv.bias), ring, hid,
                                 pos, n, p.rate_in, p.delay_in, dst_ring=False, epilogue=EPI_LEAKY_PRE, slope=u.inner_slope,
                                 counts=counts)
        return ops.conv_stream_step(CONV_CAUSAL, c1.conv.out_channels, p.c_out, 1, 1, 1, _image(c2), detached(c2.conv.bias), hid, dst, pos,
                                    n, p.rate_in, p.delay_in, src_ring=False, dst_ring=dst_ring, res=ring, end=end,
                                    epilogue=EPI_RESIDUAL | (EPI_LEAKY_POST if post is not None else 0), slope=post or 0.0,
                                    counts=counts)
    layer = u.convs[0]
    return ops.conv_stream_step(layer.kind, p.c_in, p.c_out, p.k, p.s, p.d, _image(layer), detached(layer.conv.bias), ring, dst, pos, n,
                                p.rate_in, p.delay_in, dst_ring=dst_ring, end=end, epilogue=EPI_LEAKY_PRE if post is not None else 0,
                                slope=post or 0.0, counts=counts)


def _own_stream(model, stream, what: str, training_ok: bool = False) -> None:
    """The two refusals every step starts with: a stream of another model, a model in training mode."""
    if not isinstance(stream, CodecStream) or stream.model_id != id(model):
        raise AgxError(f"{what}: the stream belongs to another model (model.new_stream makes one for this model)")
    if model.training and not training_ok:
        raise NotImplementedError(f"{what}: a stream is inference only: call model.eval() (there is no backward through a stream)")


def _check(model, stream: CodecStream, x: Tensor, what: str, per_frame: int, channels: int, counts=None) -> int:
    """Every refusal of a step, before the first launch; returns the chunk's frames."""
    _own_stream(model, stream, what)
    if needs_grad(x, model):
        raise NotImplementedError(f"{what}: a stream is inference only: call it under torch.no_grad()")
    if x.dim() != 3 or x.shape[1] != channels:
        raise AgxError(f"{what}: expected (B, {channels}, columns) after rearrange_in, got {tuple(x.shape)}")
    if x.shape[0] != stream.batch:
        raise AgxError(f"{what}: the chunk has batch {x.shape[0]}, the stream has {stream.batch}")
    if x.device != stream.device:
        raise AgxError(f"{what}: the chunk is on '{x.device}', the stream on '{stream.device}'")
    n, rest = divmod(x.shape[2], per_frame)
    if rest or n < 1:
        raise AgxError(f"{what}: a chunk is n >= 1 whole frames of {per_frame} columns, got {x.shape[2]} (pad the last hop)")
    if n > stream.max_chunk:
        raise AgxError(f"{what}: a chunk of {n} frames exceeds the stream's max_chunk = {stream.max_chunk}")
    if x.dtype != torch.float32:
        raise AgxError(f"{what}: expected float32, got {x.dtype}")
    if counts is not None:
        ops._checked_counts(what, counts, stream.batch, stream.device, on="the stream on")
    return n


def encode_latents_stream(model, x: Tensor, stream: CodecStream, counts: Optional[Tensor] = None) -> Tensor:
    """Encoder stack on a chunk in the model's input format -> (B, D, n) latents of the chunk's ``n`` frames.  ``counts`` (module
    docstring): row ``b`` takes its first ``c_b`` frames, and its latents behind them are exact 0."""
    xin = model.rearrange_in(x)
    n = _check(model, stream, xin, "encode_stream", stream.scale_factor, model.in_channels, counts)
    return _run_stack(model._units("encoders"), stream.plan.encoders, stream.enc_rings, xin.contiguous(), stream.enc_pos, None, n, counts)


def encode_stream(model, x: Tensor, stream: CodecStream, codebook_n: Optional[int] = None, counts: Optional[Tensor] = None):
    """-> (zq, commit, index) of the chunk.  With ``counts``, ``zq`` is masked to exact 0 behind a row's count; ``index`` there is
    the code of the zero latent and ``commit`` covers the whole chunk (module docstring)."""
    z = encode_latents_stream(model, x, stream, counts)
    zq, index, commit = model.quantizer.quantize_bcl(z, codebook_n, update_codebook=False, prioritize_early=False)
    if counts is not None:
        zq = ops.mask_tail(zq, None, counts=counts)
    return zq, commit, index


def decode_stream(model, zq: Tensor, stream: CodecStream, counts: Optional[Tensor] = None) -> Tensor:
    n = _check(model, stream, zq, "decode_stream", 1, stream.plan.decoders[0].c_in, counts)
    y = _run_stack(model._units("decoders"), stream.plan.decoders, stream.dec_rings, zq.contiguous(), stream.dec_pos, stream.end, n,
                   counts, stream.dec_hidden)
    return model.rearrange_out(y)


def forward_stream(model, x: Tensor, stream: CodecStream, codebook_n: Optional[int] = None, counts: Optional[Tensor] = None):
    zq, commit, index = encode_stream(model, x, stream, codebook_n, counts)
    return decode_stream(model, zq, stream, counts), commit, index


# --------------------------------------------------------------------------- packets
def _step_quantizer(model, what: str, codebook_n):
    """-> (codebooks (Q, K, D), q_used, sizes or None, bits) of the model's ``ResidualQuantizer`` for the step kernels."""
    from .quantizer import ResidualQuantizer
    q = model.quantizer
    if not isinstance(q, ResidualQuantizer):
        raise NotImplementedError(f"{what}: the bottleneck {type(q).__name__} is not a ResidualQuantizer")
    uniform = min(q.codebook_sizes) == q.codebook_size
    return q.codebooks.detach(), q._q_used(codebook_n), None if uniform else q.codebook_sizes, model._code_bits


def _step_frames(what: str, frames, stream, extra_limit: Optional[int] = None) -> int:
    """``frames`` of a packet step as an int, refused outside 1 .. the stream's ``max_chunk`` (and ``extra_limit``, the coder
    state's ``max_frames``) or above the frames of a quantiser step; a relay has no stream (None) and only the latter bound."""
    frames, step = int(frames), f"the {ops.RVQ_STEP_MAX_N} frames a quantiser step takes"
    if stream is None:
        top, limit = ops.RVQ_STEP_MAX_N, step
    elif extra_limit is None:
        top, limit = stream.max_chunk, f"the stream's max_chunk = {stream.max_chunk}"
    else:
        top = min(stream.max_chunk, extra_limit)
        limit = f"min(the stream's max_chunk = {stream.max_chunk}, the coder state's max_frames = {extra_limit})"
    if not 1 <= frames <= top:
        raise AgxError(f"{what}: frames = {frames} outside 1 .. {limit}")
    if frames > ops.RVQ_STEP_MAX_N:
        raise AgxError(f"{what}: frames = {frames} exceeds {step}")
    return frames


def _checked_packet_rows(what: str, packets, frames: int, q_used: int, bits: int) -> None:
    """Dense packets of ``frames`` frames: uint8 rows of ``ceil(frames q_used bits / 8)`` bytes."""
    width = -((-frames * q_used * bits) // 8)
    if not isinstance(packets, Tensor) or packets.dtype != torch.uint8 or packets.dim() != 2 or packets.shape[1] != width:
        got = f"{packets.dtype} {tuple(packets.shape)}" if isinstance(packets, Tensor) else type(packets).__name__
        raise AgxError(f"{what}: packets of {frames} frames x {q_used} codes x {bits} bits are uint8 (B, {width}), got {got}")


def encode_codes_stream(model, x: Tensor, stream: CodecStream, codebook_n: Optional[int] = None, counts: Optional[Tensor] = None,
                        stages: Optional[Tensor] = None):
    """The sender's step -> (zq (B, D, n), index (B, n, Q), packets (B, P) uint8): ``encode_latents_stream``, then the RVQ step
    (``ops.rvq_step_encode``: the full defining search of every frame below its row's count).  Behind a row's count ``zq`` is exact
    0, ``index`` is -1 and the packet bytes are 0; row ``b``'s first ``ceil(c_b Q bits / 8)`` bytes are its packet, ``bits =
    model._code_bits``.  Only the encoder rings of ``stream`` are used.

    ``stages`` (int64 (B,), device): row ``b`` sends its first ``q_b = clamp(stages[b], 0, Q)`` stages -- its packet
    is ``ceil(c_b q_b bits / 8)`` bytes dense over its own ``q_b``, ``zq`` is the sum of those stages and ``index`` is -1 at the
    others.  ``P`` does not depend on it, and the encoder rings advance by ``c_b`` whatever ``q_b`` is."""
    cbs, q_used, sizes, bits = _step_quantizer(model, "encode_codes_stream", codebook_n)      # refusals precede the first launch
    if isinstance(stream, CodecStream):                      # (what is not one is refused by the encoder step, in its own words)
        ops._checked_rows("encode_codes_stream", stream.batch, stream.device, stages=stages, on="the stream on")
        if stream.max_chunk > ops.RVQ_STEP_MAX_N:
            frames = model.rearrange_in(x).shape[-1] // stream.scale_factor
            if frames > ops.RVQ_STEP_MAX_N:
                raise AgxError(f"encode_codes_stream: a chunk of {frames} frames exceeds the {ops.RVQ_STEP_MAX_N} frames a quantiser step "
                               "takes")
    z = encode_latents_stream(model, x, stream, counts)
    return ops.rvq_step_encode(z, cbs, q_used, sizes, counts, bits, stages=stages)


def _packet_step(model, what: str, packets, stream, frames, codebook_n, counts, stages):
    """Every refusal of the receiver's step, before the first launch -> (codebooks, q_used, sizes, bits, frames)."""
    cbs, q_used, sizes, bits = _step_quantizer(model, what, codebook_n)
    _own_stream(model, stream, what)
    frames = _step_frames(what, frames, stream)
    _checked_packet_rows(what, packets, frames, q_used, bits)
    if packets.shape[0] != stream.batch:
        raise AgxError(f"{what}: the packets have batch {packets.shape[0]}, the stream has {stream.batch}")
    if packets.device != stream.device:
        raise AgxError(f"{what}: the packets are on '{packets.device}', the stream on '{stream.device}'")
    ops._checked_rows(what, stream.batch, stream.device, counts, stages, on="the stream on")
    return cbs, q_used, sizes, bits, frames


def decode_codes_stream(model, packets: Tensor, stream: CodecStream, frames: int, codebook_n: Optional[int] = None,
                        counts: Optional[Tensor] = None, stages: Optional[Tensor] = None):
    """The receiver's step -> (y, index (B, frames, Q)): the packets of ``frames`` frames per row (``encode_codes_stream``; the bytes
    behind a row's count are not read) through ``ops.rvq_step_decode`` and the decoder stack step.  Only the decoder rings of
    ``stream`` are used.

    ``stages``: the tensor the sender, or the last ``restage_packets`` on the way, used.  Row ``b``'s frames are the sum of its
    ``q_b`` stages and ``index`` is -1 at the others.  A row with ``c_b > 0`` and ``q_b == 0`` pushes ``c_b`` frames of the zero
    latent through the decoder and advances by ``c_b``: sending no stage is silence of the quantiser, not a pause (``counts``
    pauses a row)."""
    what = "decode_codes_stream"
    cbs, q_used, sizes, bits, frames = _packet_step(model, what, packets, stream, frames, codebook_n, counts, stages)
    zq, index = ops.rvq_step_decode(packets.contiguous(), frames, cbs, q_used, bits, sizes, counts, want_index=True, stages=stages)
    return decode_stream(model, zq, stream, counts), index


# --------------------------------------------------------------------------- coded packets
def _coded_step(model, what: str, stream, coder, coder_state, frames, counts, stages):
    """Every refusal of a coded step, before the first launch: those of ``_packet_step`` without the fixed packet width, and a
    coder whose prior does not model this quantiser's codes -> (codebooks, q_used, sizes, bits, frames)."""
    from .entropy import PriorCoder, PriorCoderState
    cbs, q_used, sizes, bits = _step_quantizer(model, what, None)
    _own_stream(model, stream, what)
    if not isinstance(coder, PriorCoder) or not isinstance(coder_state, PriorCoderState):
        raise AgxError(f"{what}: coder must be a PriorCoder and coder_state the PriorCoderState of its new_state()")
    q = model.quantizer
    if coder.num_quantizers != q_used or tuple(coder.codebook_sizes) != tuple(int(v) for v in q.codebook_sizes):
        raise AgxError(f"{what}: the prior models {coder.num_quantizers} stages of {tuple(coder.codebook_sizes)} codes, the quantiser has "
                       f"{q_used} of {tuple(q.codebook_sizes)}")
    frames = _step_frames(what, frames, stream, coder_state.max_frames)
    if coder_state.batch != stream.batch or coder_state.rans.device != stream.device:
        raise AgxError(f"{what}: the coder state has batch {coder_state.batch} on '{coder_state.rans.device}', the stream {stream.batch} "
                       f"on '{stream.device}'")
    ops._checked_rows(what, stream.batch, stream.device, counts, stages, on="the stream on")
    return cbs, q_used, sizes, bits, frames


def encode_coded_stream(model, x: Tensor, stream: CodecStream, coder, coder_state, counts: Optional[Tensor] = None,
                        stages: Optional[Tensor] = None):
    """The sender's coded step -> (packets (B, 2 n Q + 4) uint8, nbytes (B,) int64, index (B, n, Q)): the ``index`` of
    ``encode_codes_stream`` -- the same encoder step and the same quantiser step, which is not asked for ``zq`` here -- put through
    ``coder.encode``.  Row ``b``'s packet is its first ``nbytes[b]`` bytes.  The quantiser step kernel writes its dense packet bytes
    next to the codes as it always does; they are dropped."""
    what = "compress_stream_coded"
    if not isinstance(x, Tensor):
        raise AgxError(f"{what}: x_chunk must be a tensor, got {type(x).__name__}")
    _own_stream(model, stream, what, training_ok=True)       # (that refusal keeps its place: behind the quantiser's, in _coded_step)
    frames = model.rearrange_in(x).shape[-1] // stream.scale_factor
    cbs, q_used, sizes, bits, _ = _coded_step(model, what, stream, coder, coder_state, frames, counts, stages)
    z = encode_latents_stream(model, x, stream, counts)
    _, index, _ = ops.rvq_step_encode(z, cbs, q_used, sizes, counts, bits, want_zq=False, stages=stages)
    packets, nbytes = coder.encode(coder_state, index, counts, stages)
    return packets, nbytes, index


def decode_coded_stream(model, packets: Tensor, nbytes: Tensor, stream: CodecStream, coder, coder_state, frames: int,
                        counts: Optional[Tensor] = None, stages: Optional[Tensor] = None):
    """The receiver's coded step -> (y, index (B, frames, Q)): ``coder.decode``, then ``decode_stream`` of ``ops.codes_embed(index,
    codebooks, counts)`` -- one launch for the sum of a frame's codewords, in stage order, a -1 contributing nothing.  As on the
    dense path a row with ``c_b > 0`` and ``q_b == 0`` pushes ``c_b`` frames of the zero latent through the decoder."""
    what = "decompress_stream_coded"
    cbs, q_used, _, _, frames = _coded_step(model, what, stream, coder, coder_state, frames, counts, stages)
    index = coder.decode(coder_state, packets, nbytes, frames, counts, stages)
    zq = ops.codes_embed(index, cbs[:q_used].contiguous(), counts)
    return decode_stream(model, zq, stream, counts), index


def restage_packets(model, packets: Tensor, frames: int, stages: Tensor, stages_from: Optional[Tensor] = None,
                    codebook_n: Optional[int] = None, counts: Optional[Tensor] = None):
    """A relay's step -> (packets (B, P), stages (B,) int64): packet rows of ``frames`` frames, sent with ``stages_from`` (None:
    all ``Q`` stages), re-packed to ``min(q_in, clamp(stages[b], 0, Q))`` stages per row (``ops.rvq_packets_restage``: one launch,
    no codebooks, no decoding, no stream).  The packets are byte for byte what the sender would have written at that stage count,
    and the returned ``stages`` -- written on the device -- is what the receiver or the next relay takes."""
    what = "restage_packets"
    _, q_used, _, bits = _step_quantizer(model, what, codebook_n)
    frames = _step_frames(what, frames, None)
    _checked_packet_rows(what, packets, frames, q_used, bits)
    return ops.rvq_packets_restage(packets.contiguous(), frames, q_used, bits, stages, stages_from, counts)


def flush_counts(stream: CodecStream, rows, n: int) -> Tensor:
    """The counts of one flush step of ``n`` frames that only ``rows`` receive: ``n`` for them, 0 for every other row, as an int64
    (B,) tensor on the stream's device.  Built on the host: between steps, outside any captured graph."""
    rows = stream._rows(rows, "decode_flush")
    counts = [0] * stream.batch
    for r in rows:
        counts[r] = int(n)
    return torch.tensor(counts, dtype=torch.int64).to(stream.device)


def decode_flush(model, stream: CodecStream, rows=None) -> Tensor:
    """The ``ceil(decoder_delay / scale_factor)`` zero-frame steps that bring the delayed tail out, in chunks of at most
    ``max_chunk`` frames -> (B, C, frames * scale_factor) in the model's output format.  ``rows``: only those rows receive the
    flush frames (counted steps, ``flush_counts``) -- one stream's tail comes out while the others stay put, their part of the
    result exact 0.  Call it between steps, outside any captured graph."""
    left, parts = stream.plan.flush_frames, []
    c = stream.plan.decoders[0].c_in
    if rows is not None:
        stream._rows(rows, "decode_flush")      # the refusal precedes the first launch
    while left > 0:
        n = min(left, stream.max_chunk)
        counts = None if rows is None else flush_counts(stream, rows, n)
        parts.append(decode_stream(model, torch.zeros((stream.batch, c, n), dtype=torch.float32, device=stream.device), stream, counts))
        left -= n
    if not parts:
        return model.rearrange_out(torch.zeros((stream.batch, model.in_channels, 0), dtype=torch.float32, device=stream.device))
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1 if model.input_format == "b l c" else 2)
