"""Entropy coding of the stream packets with the code prior (build-defined).

A prior that predicts the next frame's codes is the probability model of an entropy coder.  ``PriorCoder`` joins ``CodePrior``'s
cached step to a byte-wise rANS coder on the device: the sender codes every frame's codes under the distribution the prior gives
for that frame, the receiver runs the same cached step, decodes the frame, and the decoded frame becomes the step's ``carry``.  The
coded path is lossless against the dense wire (``compress_stream``): the codes that come out are the codes that went in.

Sender and receiver execute the IDENTICAL launch sequence on identical inputs -- one cached walk at n = 1 per frame from
``carry``, then ``ops.codes_cum`` -- so their integer tables agree bit for bit, which is all an entropy coder needs.  (Feeding the
sender a whole hop through ``prime`` in one chunk is out of scope: its logits equal the stepped ones within 2e-5, not bit for
bit.)  The per-frame count arithmetic and the forced ``carry`` are integer device ops ("index plumbing"); the host
makes no decision, so a hop is captured once (``GraphedForward``) and replayed for any mix of paused rows and bitrates.

The coder is flushed per hop: a packet row is self-contained (4 bytes of final state per row and hop), rows pause, reset and
change bitrate alone, and a lost packet costs its hop only -- the prior's cache aside, which the caller resets as it would for
any stream.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import ops
from ._lib import AgxError
from .prior import CodePrior, CodePriorState

Tensor = torch.Tensor

__all__ = ["PriorCoder", "PriorCoderState"]


class PriorCoderState:
    """What one side of a coded link carries between hops (``PriorCoder.new_state``), all of it in device memory: ``prior``, the
    ``CodePriorState`` (cache positions and ``carry``); the hop's table buffer, ``max_frames`` frames of int32 (B, Q, K + 1)
    tables; ``rans`` (B, 2) int64, the receiver's coder state and read cursor; ``status`` (B,) int64, the error bits of the last
    hop (``ops.codes_rans_decode``)."""

    def __init__(self, prior_state: CodePriorState, max_frames: int, num_quantizers: int, k: int):
        dev, b = prior_state.carry.device, prior_state.batch
        self.prior, self.batch, self.max_frames = prior_state, b, int(max_frames)
        self._q, self._k1 = num_quantizers, k + 1
        self._tables = torch.zeros(b * self.max_frames * num_quantizers * (k + 1), dtype=torch.int32, device=dev)
        self.rans = torch.zeros((b, 2), dtype=torch.int64, device=dev)
        self.status = torch.zeros((b,), dtype=torch.int64, device=dev)

    def tables(self, frames: int) -> Tensor:
        """The table buffer of a hop of ``frames`` frames: int32 (B, frames, Q, K + 1), a view of the state's one buffer."""
        return self._tables[:self.batch * frames * self._q * self._k1].view(self.batch, frames, self._q, self._k1)

    def reset(self, rows=None) -> None:
        """Hand ``rows`` (default: all) to a new sequence with device fills: the prior's positions 0 and ``carry`` the start row,
        coder state and status 0.  Call it between hops, outside any captured graph, on both sides of the link."""
        self.prior.reset(rows)
        for sel in ops._row_slices("reset", rows, self.batch, "state"):
            self.rans[sel].fill_(0)
            self.status[sel].fill_(0)


class PriorCoder(nn.Module):
    """``PriorCoder(prior)``: an eval-mode ``CodePrior`` as the model of a per-hop rANS coder.  Adds no parameters."""

    def __init__(self, prior: CodePrior):
        super().__init__()
        if not isinstance(prior, CodePrior):
            raise AgxError(f"PriorCoder: prior must be a CodePrior, got {type(prior).__name__}")
        if prior.training:
            raise AgxError("PriorCoder: the prior must be in eval mode (prior.eval()): both sides of a link run the same inference step")
        self.prior = prior
        self.num_quantizers, self.codebook_sizes, self.k = prior.num_quantizers, prior.codebook_sizes, prior.k

    def new_state(self, batch: int, max_frames: int, capacity: Optional[int] = None) -> PriorCoderState:
        """A ``PriorCoderState`` for ``batch`` rows at position 0 whose hops hold up to ``max_frames`` frames."""
        max_frames = int(max_frames)
        if max_frames < 1 or max_frames * self.num_quantizers > ops.RANS_MAX_SYMBOLS:
            raise AgxError(f"PriorCoder.new_state: max_frames = {max_frames} outside 1 .. {ops.RANS_MAX_SYMBOLS // self.num_quantizers} "
                           f"(a row codes at most {ops.RANS_MAX_SYMBOLS} symbols per hop)")
        return PriorCoderState(self.prior.new_state(batch, seed=0, capacity=capacity), max_frames, self.num_quantizers, self.k)

    # ------------------------------------------------------------------ checks, all before the first launch
    def _checked(self, what: str, state, batch: int, frames: int, counts, stages):
        if not isinstance(state, PriorCoderState):
            raise AgxError(f"{what}: state must be the PriorCoderState of this coder's new_state()")
        self.prior._check_state(what, state.prior)
        if self.prior.training:
            raise AgxError(f"{what}: the prior must be in eval mode")
        if batch != state.batch:
            raise AgxError(f"{what}: the operands have batch {batch}, the state {state.batch}")
        if not 1 <= frames <= state.max_frames:
            raise AgxError(f"{what}: a hop of {frames} frames outside 1 .. the state's max_frames = {state.max_frames}")
        dev = state.rans.device
        return ops._checked_rows(what, batch, dev, counts, stages, on="the state is on")

    def _frame_tables(self, state: PriorCoderState, tables: Tensor, i: int, counts, stages):
        """Frame ``i`` of the hop on either side: the prior's cached walk at n = 1 from ``carry`` and that frame's tables ->
        the per-frame count (``clamp(counts - i, 0, 1)``, an integer device op; None without counts)."""
        q = self.num_quantizers
        c_i = None if counts is None else (counts - i).clamp_(0, 1)
        logits = self.prior._logits(state.prior, state.prior.carry.view(state.batch, 1, q), c_i)
        ops.codes_cum(logits, q, self.codebook_sizes, c_i, stages, out=tables, frame0=i)
        return c_i

    # ------------------------------------------------------------------ the two sides
    def encode(self, state: PriorCoderState, codes: Tensor, counts: Optional[Tensor] = None, stages: Optional[Tensor] = None):
        """The sender's hop: codes (B, n, Q) int64 -> (packets (B, 2 n Q + 4) uint8, nbytes (B,) int64).  Row b codes its first
        ``clamp(counts[b], 0, n)`` frames and, of each, its first ``clamp(stages[b], 0, Q)`` stages; its packet is its first
        ``nbytes[b]`` bytes and everything behind them is 0.  ``state.status`` takes the coder's status (bit 0: a live code lay
        outside its stage and was skipped -- the receiver cannot decode that hop).  No host decision."""
        what = "PriorCoder.encode"
        codes = self.prior._checked_codes(what, codes)
        counts, stages = self._checked(what, state, codes.shape[0], codes.shape[1], counts, stages)
        n = codes.shape[1]
        with torch.no_grad():
            staged = self.prior._staged(codes, stages)
            tables, carry = state.tables(n), state.prior.carry
            for i in range(n):
                c_i = self._frame_tables(state, tables, i, counts, stages)
                if c_i is None:
                    carry.copy_(staged[:, i])
                else:               # the rows that took the frame carry its codes, the others what they carried
                    carry.copy_(torch.where((c_i > 0)[:, None], staged[:, i], carry))
            packets, nbytes, status = ops.codes_rans_encode(tables, codes, self.codebook_sizes, counts, stages)
            state.status.copy_(status)
        return packets, nbytes

    def decode(self, state: PriorCoderState, packets: Tensor, nbytes: Tensor, frames: int, counts: Optional[Tensor] = None,
               stages: Optional[Tensor] = None) -> Tensor:
        """The receiver's hop: the packet rows of ``frames`` frames -> codes (B, frames, Q) int64, -1 behind a row's frame and
        stage counts (the sender's ``counts`` and ``stages``).  Per frame: the same walk and tables as the sender's, then
        ``ops.codes_rans_decode`` of that one frame, which writes ``carry``.  ``state.status`` is 0 for every row whose packet
        decoded cleanly.  No host decision."""
        what = "PriorCoder.decode"
        frames = int(frames)
        if not isinstance(packets, Tensor) or packets.dtype != torch.uint8 or packets.dim() != 2 or packets.shape[1] < 1:
            got = f"{packets.dtype} {tuple(packets.shape)}" if isinstance(packets, Tensor) else type(packets).__name__
            raise AgxError(f"{what}: packets must be uint8 (B, P), got {got}")
        counts, stages = self._checked(what, state, packets.shape[0], frames, counts, stages)
        if not isinstance(nbytes, Tensor) or nbytes.dtype != torch.int64 or tuple(nbytes.shape) != (state.batch,) \
                or nbytes.device != state.rans.device or packets.device != state.rans.device:
            raise AgxError(f"{what}: nbytes must be an int64 ({state.batch},) tensor on the state's device, next to the packets")
        out = []
        with torch.no_grad():
            tables, packets = state.tables(frames), packets.contiguous()
            for i in range(frames):
                self._frame_tables(state, tables, i, counts, stages)
                out.append(ops.codes_rans_decode(tables, packets, nbytes, state.rans, state.status, i, 1, self.codebook_sizes, counts,
                                                 stages, state.prior.carry))
        return out[0] if frames == 1 else torch.cat(out, dim=1)
