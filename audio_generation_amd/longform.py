"""Time-folded long-clip inference: receptive field, window plan and the folded encode / decode.

The conv stacks are fully convolutional with a finite receptive field, so one long clip can be cut into overlapping
windows, the windows run AS A BATCH on the kernels that are tuned for batches, and the valid part of every window's
result stitched back -- the plain forward's result from a batch of bounded windows.  Stateless (nothing is carried
between calls), inference only.  Measured: this bounds activation memory, it does not make a clip faster.

* ``receptive_field(model)`` walks the model's unit lists (``CausalVQAE._units``) and accumulates, layer by layer, which input positions one output
  frame reads (pad rules of ``vae.py`` / ``wavelets.py``; nothing is hard-coded per configuration);
* ``plan(...)`` is the window table: no window hangs over either end of the clip, because zero-filling a halo is not
  what the kernels' own padding does (every LAYER pads its own input with zeros; a zero-filled waveform halo comes out
  of the first conv as the bias);
* ``encode_long`` / ``decode_long`` / ``forward_long`` fold with ``agx_time_fold``, run the existing stacks, crop and
  place with ``agx_time_unfold``.  The quantiser runs once, on the stitched latents, so halo frames never reach it.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch
from . import ops
from ._lib import needs_grad

Tensor = torch.Tensor


def _ceil_div(a: int, b: int) -> int:
    return -((-a) // b)


# --------------------------------------------------------------------------- layer rules
def _primitives(model, which: str) -> List[tuple]:
    """The layers of a stack that move information along time, in execution order (``Unit.primitives``)."""
    return [p for u in model._units(which) for p in u.primitives()]


def _same_pads(k: int) -> Tuple[int, int]:
    left = (k - 1) // 2                                             # torch padding="same": total k - 1, the odd one on the right
    return left, k - 1 - left


def _back(layer: tuple, lo: int, hi: int) -> Tuple[int, int]:
    """Input index interval that the output interval [lo, hi] of ``layer`` reads (interior of the signal)."""
    kind = layer[0]
    if kind == "causal":      # vae.py:32: left pad d (k - 1) - s + 1, so output i reads i s - pad ... i s + s - 1
        _, k, s, d = layer
        return lo * s - (d * (k - 1) - s + 1), hi * s + s - 1
    if kind == "convt":       # vae.py:58-64: y[j] = sum_{i s + t = j} x[i] w[t], 0 <= t < k (the crop only drops the tail)
        _, k, s = layer
        return _ceil_div(lo - k + 1, s), hi // s
    if kind == "up":          # vae.py:81-89: nearest upsample, then a "same" conv on the upsampled signal
        _, k, s = layer
        left, right = _same_pads(k)
        return (lo - left) // s, (hi + right) // s
    if kind == "multires":    # wavelets.py:79-96: `depth` causal depthwise convs in cascade, dilation doubling
        _, k, depth = layer
        return lo - (k - 1) * (2 ** depth - 1), hi
    raise AssertionError(kind)


def _back_wavelet(layer: tuple, lo: int, hi: int):
    """WaveletLayer (wavelets.py:213-234): "same" conv -> fold -> "same" conv.  Output o of the fold sums the flat signal
    over [o fold, o fold + n_points) with n_points flat samples per input step, i.e. it reads inputs o // scale and (unless
    scale divides o) the next one.  Also returns the interval AT THE FOLD'S OUTPUT, which the end-of-signal quirk needs."""
    _, k_in, scale, n_points, k_out = layer
    fold = n_points // scale
    left, right = _same_pads(k_out)
    lo, hi = lo - left, hi + right
    fold_lo, fold_hi = lo, hi
    lo, hi = (lo * fold) // n_points, (hi * fold + n_points - 1) // n_points
    left, right = _same_pads(k_in)
    return lo - left, hi + right, fold_lo, fold_hi


def _rate(layer: tuple) -> Tuple[int, int]:
    """(down, up) resampling factors of a layer."""
    if layer[0] == "causal":
        return layer[2], 1
    if layer[0] in ("convt", "up", "wavelet"):
        return 1, layer[2]
    return 1, 1


@dataclass(frozen=True)
class ReceptiveField:
    """Reach of one latent frame (encoder, in input samples) and of one frame of output samples (decoder, in latent
    frames), and the halos (whole latent frames) a folded window needs for its kept frames to equal the plain call's.

    Encoder: latent frame ``f`` reads samples ``f * scale_factor - enc_left ... f * scale_factor + enc_right``.
    Decoder: output samples ``[f, f + 1) * scale_factor`` read latent frames ``f - dec_left ... f + dec_right``."""
    scale_factor: int
    enc_left: int
    enc_right: int
    dec_left: int
    dec_right: int
    enc_halo_left: int
    enc_halo_right: int
    dec_halo_left: int
    dec_halo_right: int


def stack_reach(layers: List[tuple]):
    """(down, up, left, right, quirk_right) of a stack: one output "frame" is ``up`` consecutive outputs starting at a
    multiple of ``up`` and corresponds to ``down`` inputs; it reads the inputs ``frame * down - left ... frame * down + right``.
    ``quirk_right``: whole frames at the right end of a tensor that the wavelet fold's end-of-signal rule taints (the
    last ``scale - 1`` fold outputs are raw samples, not window sums: wavelets.py:228-231) -- 0 without a wavelet layer."""
    down = up = 1
    for layer in layers:
        d, u = _rate(layer)
        down, up = down * d, up * u
    if down != 1 and up != 1:
        raise NotImplementedError("receptive_field: a stack that both down- and upsamples")
    lo, hi = 0, up - 1                      # output frame 0 (negative positions stand for "earlier": the rules are shift-invariant)
    per_frame = up                          # outputs per frame at the current layer's output
    quirk = 0
    for layer in reversed(layers):
        if layer[0] == "wavelet":
            scale = layer[2]
            lo, hi, _, fold_hi = _back_wavelet(layer, lo, hi)
            # frame j reads the fold's output up to j * per_frame + fold_hi; in a window of W frames the positions from
            # W * per_frame - (scale - 1) on are tainted, so frames j <= W - 1 - h are clean iff fold_hi + scale <= (1 + h) * per_frame
            quirk = max(quirk, _ceil_div(fold_hi + scale, per_frame) - 1)
        else:
            lo, hi = _back(layer, lo, hi)
        d, u = _rate(layer)
        per_frame = per_frame * d // u
    return down, up, -lo, hi, quirk


def receptive_field(model) -> ReceptiveField:
    """Derived from ``model.encoders`` / ``model.decoders`` as they are wired (see the module docstring)."""
    _require_foldable(model)
    enc, dec = _primitives(model, "encoders"), _primitives(model, "decoders")
    e_down, e_up, e_left, e_right, _ = stack_reach(enc)
    d_down, d_up, d_left, d_right, d_quirk = stack_reach(dec)
    sf = int(model.scale_factor)
    if (e_down, e_up) != (sf, 1) or (d_down, d_up) != (1, sf):
        raise NotImplementedError(f"receptive_field: stacks resample by {e_down}/{e_up} and {d_down}/{d_up}, scale_factor is {sf}")
    # a window of whole frames [a, b) holds the samples [a sf, b sf): frame j is exact when a sf <= j sf - left (or a is the
    # true start) and j sf + right <= b sf - 1.  The strided convs look s - 1 samples ahead, which adds up to at most sf - 1
    # samples: inside frame j itself, so the encoder's right halo is 0 whole frames unless a layer reaches further.
    return ReceptiveField(scale_factor=sf, enc_left=e_left, enc_right=e_right, dec_left=d_left, dec_right=d_right,
                          enc_halo_left=_ceil_div(e_left, sf), enc_halo_right=max(0, _ceil_div(e_right + 1, sf) - 1),
                          dec_halo_left=d_left, dec_halo_right=max(d_right, d_quirk))


# --------------------------------------------------------------------------- window plan
@dataclass(frozen=True)
class Plan:
    """``windows`` equal windows of ``width`` frames at ``hop`` (window s = frames ``[s hop, s hop + width)``) plus, when
    ``tail_start`` is not None, one call on ``[tail_start, n_frames)``.  ``windows == 0`` means: one plain call."""
    n_frames: int
    hop: int
    halo_left: int
    halo_right: int
    width: int
    windows: int
    tail_start: Optional[int]

    @property
    def covered(self) -> int:
        """Output frames the batched windows produce: ``[0, covered)``."""
        return self.windows * self.hop + self.halo_left if self.windows else 0

    @property
    def single(self) -> bool:
        return self.windows == 0 or (self.windows == 1 and self.tail_start is None)

    def segments(self) -> List[Tuple[int, int, int, int]]:
        """(window start, window end, first output, end of outputs) per call, in frames, in output order."""
        if self.windows == 0:
            return [(0, self.n_frames, 0, self.n_frames)]
        segs = [(s * self.hop, s * self.hop + self.width, 0 if s == 0 else s * self.hop + self.halo_left,
                 (s + 1) * self.hop + self.halo_left) for s in range(self.windows)]
        if self.tail_start is not None:
            segs.append((self.tail_start, self.n_frames, self.covered, self.n_frames))
        return segs


def plan(n_frames: int, hop_frames: int, halo_left: int, halo_right: int, whole_frames: Optional[int] = None) -> Plan:
    """Window table for ``n_frames`` output frames.  ``whole_frames`` (default ``n_frames``): frames that lie wholly inside
    the clip -- one less than ``n_frames`` when the clip length is not a multiple of ``scale_factor``; the ragged last frame
    belongs to the tail call, which ends at the true end as the plain call does."""
    n_frames, hop, hl, hr = int(n_frames), int(hop_frames), int(halo_left), int(halo_right)
    whole = n_frames if whole_frames is None else int(whole_frames)
    if n_frames < 1 or hop < 1 or hl < 0 or hr < 0 or not (0 <= whole <= n_frames):
        raise ValueError(f"plan: n_frames={n_frames} hop={hop} halos=({hl}, {hr}) whole_frames={whole}")
    width = hl + hop + hr
    windows = max(0, (whole - width) // hop + 1)            # the largest S with (S - 1) hop + width <= whole
    if windows == 0:
        return Plan(n_frames, hop, hl, hr, width, 0, None)
    covered = windows * hop + hl
    return Plan(n_frames, hop, hl, hr, width, windows, windows * hop if covered < n_frames else None)


# --------------------------------------------------------------------------- folded calls
def _require_foldable(model) -> None:
    from .quantizer import ResidualQuantizer
    if not isinstance(model.quantizer, ResidualQuantizer):
        raise NotImplementedError(
            f"time folding needs a bottleneck with a finite receptive field; {type(model.quantizer).__name__} "
            "(e.g. global attention) has none.  Use the plain encode / forward.")


def _require_inference(model, x: Tensor) -> None:
    if needs_grad(x, model):
        raise NotImplementedError("the *_long entries are inference only (like compress): call them under torch.no_grad(), "
                                  "or use the plain forward for training")


def _rf(model) -> ReceptiveField:
    """``receptive_field(model)``, kept for as long as the unit lists it was derived from are the model's."""
    key = model._units("encoders"), model._units("decoders")
    cached = model.__dict__.get("_longform_rf")
    if cached is None or cached[0][0] is not key[0] or cached[0][1] is not key[1]:
        cached = (key, receptive_field(model))
        model.__dict__["_longform_rf"] = cached
    return cached[1]


def default_segment_frames(batch: int, n_frames: int, halo_left: int, halo_right: int) -> int:
    """The ``segment_frames=None`` rule, a function of the shape alone (so a captured graph stays valid): ONE window, i.e.
    the plain call.  Measured (profiles/longform_times.txt): at 1 x 360 000, 1 x 72 000 and 4 x 72 000 every
    folded row is slower than the plain forward -- a single clip is bound by its chain of dependent launches, not by CU
    fill -- so folding is what an explicit ``segment_frames`` asks for (bounded activation memory, same result)."""
    return max(1, n_frames)


def _fold_run_unfold(x: Tensor, p: Plan, in_unit: int, out_unit: int, run) -> Tensor:
    """``x`` (B, C, L) with ``in_unit`` positions per frame -> stitched output with ``out_unit`` positions per frame."""
    b, _, length = x.shape
    s, hop, hl = p.windows, p.hop, p.halo_left
    yw = run(ops.time_fold(x, s, hop * in_unit, p.width * in_unit))          # (B*S, C', width * out_unit)
    if yw.shape[0] != b * s or yw.shape[2] != p.width * out_unit:
        raise ops.AgxError(f"folded stack returned {tuple(yw.shape)} for {s} windows of {p.width} frames")
    out = torch.empty((b, yw.shape[1], p.n_frames * out_unit), dtype=torch.float32, device=x.device)
    if hl:
        ops.time_unfold(yw, out, s, hl * out_unit, 0, 0, n_win=1)            # window 0 starts at the true start
    ops.time_unfold(yw, out, s, hop * out_unit, hl * out_unit, hl * out_unit)
    if p.tail_start is not None:
        start = p.tail_start * in_unit
        yt = run(ops.time_fold(x, 1, 0, length - start, start))              # ends at the true end, ragged frame included
        keep = (p.n_frames - p.covered) * out_unit
        if yt.shape[2] != (p.n_frames - p.tail_start) * out_unit:
            raise ops.AgxError(f"tail call returned {tuple(yt.shape)} for {p.n_frames - p.tail_start} frames")
        ops.time_unfold(yt, out, 1, keep, (p.covered - p.tail_start) * out_unit, p.covered * out_unit)
    return out


def encode_latents_long(model, x: Tensor, segment_frames: Optional[int] = None) -> Optional[Tensor]:
    """Folded encoder stack on (B, C, L) -> (B, D, T) latents, or None when the plan is a single window."""
    rf = _rf(model)
    sf = rf.scale_factor
    length = x.shape[2]
    n_frames = _ceil_div(length, sf)
    hop = segment_frames if segment_frames is not None else default_segment_frames(x.shape[0], n_frames, rf.enc_halo_left,
                                                                                   rf.enc_halo_right)
    p = plan(n_frames, hop, rf.enc_halo_left, rf.enc_halo_right, whole_frames=length // sf)
    if p.single:
        return None
    return _fold_run_unfold(x, p, sf, 1, lambda t: model._encoders_hip(t, quads=False))


def encode_long(model, x: Tensor, segment_frames: Optional[int] = None, codebook_n: Optional[int] = None):
    _require_foldable(model)
    _require_inference(model, x)
    xin = model.rearrange_in(x)
    z = encode_latents_long(model, ops._fold_operand(ops._f32c(xin), "encode_long"), segment_frames) if xin.dim() == 3 else None
    if z is None:
        return model.encode(x, codebook_n=codebook_n)
    zq, index, commit = model.quantizer.quantize_bcl(z, codebook_n, update_codebook=False, prioritize_early=False)
    return zq, commit, index


def decode_long(model, zq: Tensor, segment_frames: Optional[int] = None) -> Tensor:
    _require_foldable(model)
    _require_inference(model, zq)
    rf = _rf(model)
    if zq.dim() != 3:
        return model.decode(zq)
    zq = ops._fold_operand(zq, "decode_long")
    n_frames = zq.shape[2]
    hop = segment_frames if segment_frames is not None else default_segment_frames(zq.shape[0], n_frames, rf.dec_halo_left,
                                                                                   rf.dec_halo_right)
    p = plan(n_frames, hop, rf.dec_halo_left, rf.dec_halo_right)
    if p.single:
        return model.decode(zq)
    return model.rearrange_out(_fold_run_unfold(zq, p, 1, rf.scale_factor, lambda t: model._decoders_hip(t, quads=False)))


def forward_long(model, x: Tensor, segment_frames: Optional[int] = None, codebook_n: Optional[int] = None):
    zq, commit, index = encode_long(model, x, segment_frames, codebook_n)
    return decode_long(model, zq, segment_frames), commit, index
