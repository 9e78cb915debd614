"""A code prior (build-defined): an autoregressive model over the quantiser's codes on the cached Transformer.

The reference calls itself "a repo for audio generation models" and generates by decoding uniformly random codes
(``CausalVQAE.sample``).  ``CodePrior`` is the model that is missing between the two: a causal, windowed ALiBi ``Transformer``
whose input at frame ``t`` is the sum of one embedding row per residual stage of frame ``t - 1`` (frame 0 takes the start row,
row ``K`` of every stage's table) and whose head predicts all ``Q`` stages of frame ``t`` in parallel from one hidden state.
That pattern is a build-defined decision: a delay or interleaved pattern is out of scope.

Training is teacher-forced cross-entropy (``forward``); forward and backward run on the native kernels (``ops.codes_embed``,
the Transformer's walk, ``layernorm_ct``, the k = 1 conv of the head, ``ops.codes_cross_entropy``).  Generation is a cached step
(``new_state`` / ``step`` / ``prime`` / ``generate``) that makes no host decision: positions, the last frame's codes, seeds and the
per-row sampling settings all live in device memory, so one step is captured once (``GraphedForward``) and replayed for any mix
of rows -- paused rows (``counts``), rows at different bitrates (``stages``), rows with different temperatures.

The conventions are the quantiser's: ``-1`` is a stage a row does not use, ignored by the embedding and by the loss.
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import torch
from torch import nn

from . import ops
from ._lib import AgxError, needs_grad
from .transformers import Transformer, _ln, _PackedLinear

Tensor = torch.Tensor

__all__ = ["CodePrior", "CodePriorState"]


class _EmbedNative(torch.autograd.Function):
    """``ops.codes_embed`` with ``ops.codes_embed_backward`` for the tables."""

    @staticmethod
    def forward(ctx, tables: Tensor, index: Tensor):
        ctx.save_for_backward(index)
        ctx.rows = tables.shape[1]
        return ops.codes_embed(index, tables.detach())

    @staticmethod
    def backward(ctx, g: Tensor):
        (index,) = ctx.saved_tensors
        return ops.codes_embed_backward(g.contiguous(), index, ctx.rows), None


class _HeadLossNative(torch.autograd.Function):
    """Final LayerNorm -> head -> cross-entropy and their backward on the HIP kernels -> (loss, logits); the logits are returned
    for inspection and carry no gradient."""

    @staticmethod
    def forward(ctx, prior, target: Tensor, h: Tensor, *params: Tensor):
        with torch.no_grad():
            h = h.detach()
            y = _ln(prior.norm, h)
            logits = prior._head.forward(y)
            loss, _, lse, n_live = ops.codes_cross_entropy(logits, target, prior.codebook_sizes)
        ctx.prior = prior
        ctx.save_for_backward(h, y, logits, target, lse, n_live)
        ctx.mark_non_differentiable(logits)
        return loss, logits

    @staticmethod
    def backward(ctx, g_loss: Tensor, _g_logits):
        h, y, logits, target, lse, n_live = ctx.saved_tensors
        prior = ctx.prior
        dlogits = ops.codes_cross_entropy_backward(logits, target, lse, n_live, g_loss.contiguous(), prior.codebook_sizes)
        dy, g_head = prior._head.backward(y, dlogits)
        dh, dw, db = ops.layernorm_ct_backward(h, prior.norm.weight.detach(), dy, prior.norm.eps)
        return (None, None, dh, dw, db, *g_head)


class CodePriorState:
    """What a generating batch carries between steps (``CodePrior.new_state``), all of it in device memory: ``cache``, the
    Transformer's ``TransformerStreamCache``; ``carry`` (B, Q) int64, the codes of every row's last frame (the start row before
    the first); ``seeds`` and ``frame0`` (B,) int64; and the per-row sampling settings ``temperature`` (fp32), ``top_k`` (int64,
    ``<= 0`` off) and ``top_p`` (fp32, ``>= 1`` off).  The settings are plain tensors: fill them between steps (``set_sampling``)."""

    def __init__(self, cache, start: int, num_quantizers: int, seeds: Tensor):
        dev, b = cache.pos.device, cache.batch
        self.cache, self.start, self.batch = cache, int(start), b
        self.carry = torch.full((b, num_quantizers), self.start, dtype=torch.int64, device=dev)
        self.seeds = seeds
        self.frame0 = torch.zeros(b, dtype=torch.int64, device=dev)
        self.temperature = torch.ones(b, dtype=torch.float32, device=dev)
        self.top_k = torch.zeros(b, dtype=torch.int64, device=dev)
        self.top_p = torch.ones(b, dtype=torch.float32, device=dev)

    def reset(self, rows=None) -> None:
        """Hand ``rows`` (default: all) to a new sequence with device fills: positions 0, ``carry`` the start row.  Seeds and
        settings stay.  Call it between steps, outside any captured graph."""
        self.cache.reset(rows)
        for sel in ops._row_slices("reset", rows, self.batch, "state"):
            self.carry[sel].fill_(self.start)

    def set_sampling(self, temperature: Optional[float] = None, top_k: Optional[int] = None, top_p: Optional[float] = None,
                     rows=None) -> None:
        """Fill the settings of ``rows`` (default: all); None leaves a setting as it is."""
        for sel in ops._row_slices("set_sampling", rows, self.batch, "state"):
            for t, v in ((self.temperature, temperature), (self.top_k, top_k), (self.top_p, top_p)):
                if v is not None:
                    t[sel].fill_(v)


class CodePrior(nn.Module):
    """``CodePrior(num_quantizers, codebook_size, dim, depth, heads, head_dim, window, context_x)``: ``embed`` (Q, K + 1, dim) --
    row K is the start token, which the sampler can never emit --, a causal windowed ``Transformer``, a final ``LayerNorm(dim)``
    and a head ``Linear(dim, Q K)``.  ``codebook_size``: one int, or one per stage (``K`` is the largest; a shorter stage's
    surplus logits take no part in the loss or the sampling)."""

    def __init__(self, num_quantizers: int, codebook_size: Union[int, Sequence[int]], dim: int, depth: int, heads: int,
                 head_dim: int, window: int, context_x: int):
        super().__init__()
        q = int(num_quantizers)
        sizes = [int(codebook_size)] * q if isinstance(codebook_size, int) else [int(v) for v in codebook_size]
        if not 1 <= q <= 64 or len(sizes) != q or min(sizes) < 1:
            raise ValueError(f"CodePrior: num_quantizers = {num_quantizers} (1 .. 64) with codebook_size = {codebook_size}")
        self.num_quantizers, self.codebook_sizes, self.k, self.dim = q, tuple(sizes), max(sizes), int(dim)
        if self.k > ops.CODES_SAMPLE_MAX_K:
            raise ValueError(f"CodePrior: {self.k} codes per stage exceed the sampler's {ops.CODES_SAMPLE_MAX_K}")
        self.embed = nn.Parameter(torch.randn(q, self.k + 1, dim) * dim ** -0.5)
        self.transformer = Transformer(dim, depth=depth, heads=heads, head_dim=head_dim, causal=True, window=window,
                                       context_x=context_x)
        self.norm = nn.LayerNorm(dim)
        self.head = nn.Linear(dim, q * self.k)
        self._head = _PackedLinear(self.head)

    # ------------------------------------------------------------------ training
    def _checked_codes(self, what: str, codes, n_last: Optional[int] = None) -> Tensor:
        if not isinstance(codes, Tensor) or codes.dtype != torch.int64 or codes.dim() != 3 or codes.shape[2] != self.num_quantizers \
                or codes.shape[1] < 1:
            have = f"{tuple(codes.shape)} {codes.dtype}" if isinstance(codes, Tensor) else type(codes).__name__
            raise AgxError(f"{what}: codes must be an int64 (B, T, {self.num_quantizers}) tensor, got {have}")
        if codes.device != self.embed.device:
            raise AgxError(f"{what}: codes are on '{codes.device}', the model is on '{self.embed.device}'")
        return codes.contiguous()

    def _staged(self, codes: Tensor, stages: Optional[Tensor]) -> Tensor:
        """``codes`` with -1 at the stages a row does not use (index plumbing on the device; the host reads nothing)."""
        if stages is None:
            return codes
        stages = ops._checked_stages("CodePrior", stages, codes.shape[0], codes.device, on="the codes are on")
        live = torch.arange(self.num_quantizers, device=codes.device)[None, None, :] < stages[:, None, None]
        return torch.where(live, codes, torch.full_like(codes, -1))

    def forward(self, codes: Tensor, stages: Optional[Tensor] = None):
        """Teacher-forced: codes (B, T, Q) int64 -> (loss, logits (B, Q K, T)).  The input of frame t is the embedding of frame
        t - 1's codes, frame 0 takes the start row; ``loss`` is the mean cross-entropy over the live entries (``0 <= code <
        sizes[q]``): a ``-1`` is ignored by the embedding and by the loss.  ``stages`` (int64 (B,), device): row b uses its first
        ``clamp(stages[b], 0, Q)`` stages, the others count as -1.  T <= context_x."""
        codes = self._staged(self._checked_codes("CodePrior.forward", codes), stages)
        b, t, q = codes.shape
        start = torch.full((b, 1, q), self.k, dtype=torch.int64, device=codes.device)
        index = torch.cat([start, codes[:, :-1]], dim=1).contiguous()
        params = [self.norm.weight, self.norm.bias, self.head.weight, self.head.bias]
        if needs_grad(self.embed, self):
            x = _EmbedNative.apply(self.embed, index)
            h = self.transformer.run_bct(x)
            return _HeadLossNative.apply(self, codes, h, *params)
        x = ops.codes_embed(index, self.embed.detach())
        logits = self._head.forward(_ln(self.norm, self.transformer.run_bct(x)))
        return ops.codes_cross_entropy(logits, codes, self.codebook_sizes)[0], logits

    # ------------------------------------------------------------------ generation
    def new_state(self, batch: int, seed=None, capacity: Optional[int] = None) -> CodePriorState:
        """A ``CodePriorState`` for ``batch`` rows at position 0.  ``seed``: None draws one from torch's default generator
        (``torch.manual_seed`` reproduces a run); an int gives every row a seed of its own derived from it; a sequence or tensor
        of ``batch`` ints is taken as the rows' seeds.  A row's codes are a function of its own seed, not of its batch slot."""
        cache = self.transformer.new_stream_cache(batch, capacity)
        dev = cache.pos.device
        if seed is None:
            seed = ops.draw_dropout_seed()
        if isinstance(seed, int):
            gen = torch.Generator().manual_seed(seed & ((1 << 63) - 1))
            seeds = torch.randint(0, (1 << 63) - 1, (batch,), dtype=torch.int64, generator=gen)
        else:
            seeds = torch.as_tensor(seed, dtype=torch.int64).reshape(-1).clone()
            if seeds.numel() != batch:
                raise AgxError(f"new_state: {seeds.numel()} seeds for a batch of {batch}")
        return CodePriorState(cache, self.k, self.num_quantizers, seeds.to(dev))

    def _check_state(self, what: str, state) -> None:
        if not isinstance(state, CodePriorState) or state.carry.shape[1] != self.num_quantizers or state.start != self.k:
            raise AgxError(f"{what}: state must be the CodePriorState of this model's new_state()")

    def _logits(self, state: CodePriorState, index: Tensor, counts: Optional[Tensor]) -> Tensor:
        """The cached walk on the frames whose inputs are ``index`` (B, n, Q): embedding -> Transformer on the cache -> LayerNorm
        -> head -> logits (B, Q K, n).  No host decision."""
        x = ops.codes_embed(index, self.embed.detach(), counts)
        h = self.transformer.run_bct(x, cache=state.cache, counts=counts)
        return self._head.forward(_ln(self.norm, h))

    def step(self, state: CodePriorState, counts: Optional[Tensor] = None, stages: Optional[Tensor] = None) -> Tensor:
        """One cached step -> codes (B, 1, Q): snapshot ``frame0 <- cache.pos``, embed ``carry``, the Transformer on the cache,
        LayerNorm, head, ``ops.codes_sample`` (which also writes the new ``carry``).  ``counts`` (int64 (B,), device): a row with
        count 0 pauses -- its position, ring and ``carry`` are untouched, its codes are -1.  ``stages``: row b samples its first
        ``clamp(stages[b], 0, Q)`` stages, -1 elsewhere.  No host decision: capture it with ``GraphedForward`` and replay."""
        self._check_state("CodePrior.step", state)
        with torch.no_grad():
            state.frame0.copy_(state.cache.pos)
            logits = self._logits(state, state.carry.view(state.batch, 1, self.num_quantizers), counts)
            return ops.codes_sample(logits, self.num_quantizers, state.seeds, state.frame0, state.temperature, state.top_k,
                                    state.top_p, self.codebook_sizes, counts, stages, state.carry)

    def prime(self, state: CodePriorState, codes: Tensor, counts: Optional[Tensor] = None) -> Tensor:
        """Feed a prompt through the cache: codes (B, n, Q), in chunks of up to ``state.cache.max_chunk`` frames -> the logits
        (B, Q K, n) that predicted the prompt's frames (teacher-forced ones, computed incrementally).  Afterwards ``carry`` holds
        every row's last prompt frame and the next ``step`` samples frame n.  ``counts`` (int64 (B,), device): row b's prompt is
        its first ``clamp(counts[b], 0, n)`` frames."""
        self._check_state("CodePrior.prime", state)
        codes = self._checked_codes("CodePrior.prime", codes)
        b, n, q = codes.shape
        if b != state.batch:
            raise AgxError(f"CodePrior.prime: codes have batch {b}, the state {state.batch}")
        if counts is not None:
            counts = ops._checked_counts("CodePrior.prime", counts, b, codes.device, on="the codes are on")
        out, step = [], state.cache.max_chunk
        with torch.no_grad():
            for i0 in range(0, n, step):
                chunk = codes[:, i0:i0 + step]
                m = chunk.shape[1]
                c = None if counts is None else (counts - i0).clamp_(0, m)
                index = torch.cat([state.carry[:, None, :], chunk[:, :-1]], dim=1).contiguous()
                out.append(self._logits(state, index, c))
                if c is None:
                    state.carry.copy_(chunk[:, -1])
                else:       # the row's last taken frame, or what it carried: a gather and a select on the device
                    last = chunk.gather(1, (c - 1).clamp_(min=0)[:, None, None].expand(b, 1, q))[:, 0]
                    state.carry.copy_(torch.where((c > 0)[:, None], last, state.carry))
        return out[0] if len(out) == 1 else torch.cat(out, dim=2)

    def generate(self, state: CodePriorState, n_frames: int, counts: Optional[Tensor] = None,
                 stages: Optional[Tensor] = None) -> Tensor:
        """``n_frames`` steps -> codes (B, n_frames, Q); ``counts`` / ``stages`` as in ``step``, the same for every step."""
        if int(n_frames) < 1:
            raise AgxError(f"CodePrior.generate: n_frames = {n_frames}")
        return torch.cat([self.step(state, counts, stages) for _ in range(int(n_frames))], dim=1)
