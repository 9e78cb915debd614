"""Value-conditioned inputs, references and the shape list for the attention and LayerNorm kernels (TEST INFRASTRUCTURE).

Random ``0.7 * randn`` operands keep every logit within a few units of zero: the softmax is nearly flat, the running maximum of
the online-softmax kernels barely moves and no key dominates a row.  The families below put structure into the values instead
(``tests/test_attention_cases_cpu.py`` proves each stated property in float64, so the GPU tests cannot pass vacuously):

=========== ===================================================================================================================
``ramp_up``   logit(i, j) ~ ``RAMP_STEP * j + RAMP_JUMP * (j // 32)``: in every row the maximum over each 32- and 64-key block grows with the block index
              by at least 5 -- every block rescales by ``alpha``, the last (partial) block holds the row maximum
``ramp_down`` the mirror image: the maximum sits in block 0, later blocks add terms near underflow (``alpha == 1``)
``spike``     each query i has ONE key j*(i) (cycling through 0, 31, 32, 63, 64, tk - 1) whose logit exceeds all others by >= 40:
              the output is ``v[:, j*]``, gradients vanish except through v
``offset``    one extra constant component in q and k: every logit lies in (89, 130) -- ``expf`` overflows fp32 above 88.7, so
              the result is wrong wherever a maximum is not subtracted
``local``     identical keys, slopes {0, 8, 0.5}: p(i, j) = exp(-slope |i - j|) / Z in closed form; slope 8 leaves |i - j| <= 2,
              v carries j in channel 0, so an index error at a tile or block edge is an O(1) error
``gauss``     the suite's usual ``0.7 * randn`` (control)
=========== ===================================================================================================================

References are the float64 definitions (``self_core`` is ``_core`` of ``tests/test_gpu_attention_flash.py`` with the slopes as
an argument; cross-attention is ``tests/cross_attention_ref.cross_core``; LayerNorm is ``F.layer_norm`` on the transposed
tensor; gradients by autograd).  The YARDSTICK is the same definition evaluated in float32 on the CPU: ``err32 = max|fp32 -
fp64|`` (and the RMS figure) measures how ill-conditioned an input is, so that a kernel is not charged for it.  A kernel passes
when ``max|gpu - fp64| <= M * err32 + floor`` with ``floor = 4 * 2**-23 * max(1, max|want|)`` (four ulp at the output scale:
``spike`` and ``local`` make the fp32 CPU result exact), and the same for the RMS.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import attention as oattn
from tests.cross_attention_ref import cross_core

Tensor = torch.Tensor

RAMP_STEP = 0.8          # logit units per key; larger than every default slope (2^(-8/H) <= 0.5), so the ramp survives the ALiBi bias
RAMP_JUMP = 6.0          # and per 32-key block on top of that
SPIKE_MARGIN = 48.0      # logit of the chosen key above the ALiBi penalty it can carry (the property proved is a margin >= 40)
SPIKE_KEYS = (0, 31, 32, 63, 64)   # and tk - 1: both sides of the 32-key accumulator tiles and of the 64-key block
OFFSET_LOGIT = 110.0     # centre of the offset family's logits
OFFSET_ALIBI = 8.0       # the largest ALiBi penalty the offset family carries (its slopes are scaled to it)
LOCAL_SLOPES = (0.0, 8.0, 0.5)
EXPF_OVERFLOW = 89.0     # expf(x) is inf in fp32 for x > 88.73


@dataclass
class AttnCase:
    """One input: q (B, H*Dh, Tq), kv (B, 2*H*Dh, Tk: K rows, then V rows), slopes (H,); all float32 on the CPU."""
    q: Tensor
    kv: Tensor
    slopes: Tensor
    heads: int
    dh: int

    @property
    def qkv(self) -> Tensor:
        """(B, 3*H*Dh, T) for the self-attention kernels (Tq == Tk)."""
        assert self.q.shape[-1] == self.kv.shape[-1]
        return torch.cat([self.q, self.kv], dim=1).contiguous()

    @property
    def scale_div(self) -> float:
        return self.dh ** 0.5


def _pack(q: Tensor, k: Tensor, v: Tensor, slopes: Tensor) -> AttnCase:
    b, h, dh, tq = q.shape
    tk = k.shape[-1]
    return AttnCase(q.reshape(b, h * dh, tq).float().contiguous(),
                    torch.cat([k.reshape(b, h * dh, tk), v.reshape(b, h * dh, tk)], dim=1).float().contiguous(),
                    slopes.float(), h, dh)


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _ramp(b, heads, dh, tq, tk, seed, up: bool) -> AttnCase:
    g = _gen(seed)
    u = torch.randn(b, heads, dh, 1, generator=g)
    u = u / u.norm(dim=2, keepdim=True)
    amp, a = dh ** 0.25, 4.0     # |q| = a amp, |k_j| = amp level_j / a:  q . k_j / sqrt(dh) = level_j
    j = torch.arange(tk)
    blk = j // 32                # RAMP_JUMP more at every 32-key boundary: a last block of ONE key still moves the maximum by 5
    level = RAMP_STEP * j + RAMP_JUMP * blk if up else RAMP_STEP * (tk - 1 - j) + RAMP_JUMP * ((tk - 1) // 32 - blk)
    q = u * (amp * a) + 0.05 * torch.randn(b, heads, dh, tq, generator=g)
    k = u * (amp / a) * level.float() + 0.05 * torch.randn(b, heads, dh, tk, generator=g)
    v = torch.randn(b, heads, dh, tk, generator=g)
    return _pack(q, k, v, oattn.alibi_slopes(heads))


def ramp_up(b, heads, dh, tq, tk, seed) -> AttnCase:
    return _ramp(b, heads, dh, tq, tk, seed, True)


def ramp_down(b, heads, dh, tq, tk, seed) -> AttnCase:
    return _ramp(b, heads, dh, tq, tk, seed, False)


def spike_targets(tk: int) -> List[int]:
    return sorted({min(j, tk - 1) for j in SPIKE_KEYS + (tk - 1,)})


def spike_key_of_query(tq: int, tk: int) -> Tensor:
    """j*(i): the key query i attends to."""
    tg = torch.tensor(spike_targets(tk))
    return tg[torch.arange(tq) % len(tg)]


def spike(b, heads, dh, tq, tk, seed) -> AttnCase:
    g = _gen(seed)
    tg = spike_targets(tk)
    n = len(tg)
    assert dh > n, "spike needs one head dim per target key and one for the noise"
    slopes = oattn.alibi_slopes(heads)
    peak = SPIKE_MARGIN + float(slopes.max()) * (max(tq, tk) - 1)
    beta = (peak * dh ** 0.5) ** 0.5                       # beta^2 / sqrt(dh) = peak
    q = 0.3 * torch.randn(b, heads, dh, tq, generator=g)
    k = 0.3 * torch.randn(b, heads, dh, tk, generator=g)
    q[:, :, :n] = 0.0                                      # the first n head dims carry the spikes alone
    k[:, :, :n] = 0.0
    for m, j in enumerate(tg):
        k[:, :, m, j] = beta
    q[:, :, torch.arange(tq) % n, torch.arange(tq)] = beta
    v = torch.randn(b, heads, dh, tk, generator=g)
    return _pack(q, k, v, slopes)


def offset(b, heads, dh, tq, tk, seed) -> AttnCase:
    g = _gen(seed)
    alpha = (dh / (dh - 1.0)) ** 0.25                      # the dh - 1 random components give a logit of unit variance
    big = (OFFSET_LOGIT * dh ** 0.5) ** 0.5                # big^2 / sqrt(dh) = OFFSET_LOGIT
    q = alpha * torch.randn(b, heads, dh, tq, generator=g)
    k = alpha * torch.randn(b, heads, dh, tk, generator=g)
    q[:, :, -1] = big
    k[:, :, -1] = big
    v = torch.randn(b, heads, dh, tk, generator=g)
    slopes = oattn.alibi_slopes(heads)
    slopes = slopes * (OFFSET_ALIBI / (float(slopes.max()) * max(1, max(tq, tk) - 1)))
    return _pack(q, k, v, slopes)


def local(b, heads, dh, tq, tk, seed) -> AttnCase:
    g = _gen(seed)
    q = 0.7 * torch.randn(b, heads, dh, tq, generator=g)
    k = (0.7 * torch.randn(b, heads, dh, 1, generator=g)).expand(b, heads, dh, tk).clone()
    v = torch.randn(b, heads, dh, tk, generator=g)
    v[:, :, 0] = torch.arange(tk, dtype=torch.float32)
    slopes = torch.tensor([LOCAL_SLOPES[h % len(LOCAL_SLOPES)] for h in range(heads)])
    return _pack(q, k, v, slopes)


def gauss(b, heads, dh, tq, tk, seed) -> AttnCase:
    g = _gen(seed)
    q = 0.7 * torch.randn(b, heads, dh, tq, generator=g)
    k = 0.7 * torch.randn(b, heads, dh, tk, generator=g)
    v = 0.7 * torch.randn(b, heads, dh, tk, generator=g)
    return _pack(q, k, v, oattn.alibi_slopes(heads))


FAMILIES: Dict[str, Callable[..., AttnCase]] = {"ramp_up": ramp_up, "ramp_down": ramp_down, "spike": spike, "offset": offset,
                                                "local": local, "gauss": gauss}
BF16_FAMILIES = ("ramp_up", "ramp_down", "spike", "local", "gauss")   # bf16 operands cannot hold logits of 110 to +-0.4


def seed_of(family: str, dh: int, tq: int, tk: int) -> int:
    return 1000 * list(FAMILIES).index(family) + 7 * dh + 31 * tq + tk


# ---------------------------------------------------------------------------------------------------------------- references
def alibi(slopes: Tensor, tq: int, tk: int, dtype) -> Tensor:
    """(H, tq, tk): ``-slope_h |i - j|`` (``oracle.attention.alibi_bias`` with the slopes as an argument)."""
    i = torch.arange(tq, dtype=dtype).reshape(-1, 1)
    j = torch.arange(tk, dtype=dtype).reshape(1, -1)
    return -(i - j).abs().unsqueeze(0) * slopes.to(dtype).reshape(-1, 1, 1)


def logits(q: Tensor, kv: Tensor, slopes: Tensor, heads: int, dh: int) -> Tensor:
    """(B, H, Tq, Tk) in the dtype of ``q``."""
    b, _, tq = q.shape
    tk = kv.shape[-1]
    qh = q.reshape(b, heads, dh, tq)
    kh = kv[:, :heads * dh].reshape(b, heads, dh, tk)
    return torch.einsum("bhdi,bhdj->bhij", qh, kh) / dh ** 0.5 + alibi(slopes, tq, tk, q.dtype)


def self_core(qkv: Tensor, slopes: Tensor, heads: int, dh: int) -> Tensor:
    """``_core`` of tests/test_gpu_attention_flash.py in the dtype of ``qkv`` (differentiable), slopes as an argument."""
    b, _, t = qkv.shape
    q, k, v = (z.reshape(b, heads, dh, t) for z in qkv.chunk(3, dim=1))
    s = torch.einsum("bhdi,bhdj->bhij", q, k) / dh ** 0.5 + alibi(slopes, t, t, qkv.dtype)
    return torch.einsum("bhij,bhdj->bhdi", s.softmax(-1), v).reshape(b, heads * dh, t)


def _bf16(x: Tensor) -> Tensor:
    return x.float().bfloat16().to(x.dtype)


def self_core_bf16(qkv: Tensor, slopes: Tensor, heads: int, dh: int, key_block: int = 64) -> Tensor:
    """The float64 definition on operands rounded to bf16 as csrc/attention_flash.hip rounds them (PREC 1 and
    ``attention_bf16_lds``): q, k and v on load; the UNNORMALISED probabilities ``exp(s - m)`` of each 64-key block, relative
    to the running maximum ``m`` at that block, as the B operand of V P^T.  The row sum ``l`` takes the unrounded ones, the
    logits, the softmax statistics and both accumulations are exact (fp32 in the kernel)."""
    b, _, t = qkv.shape
    q, k, v = (_bf16(z).reshape(b, heads, dh, t) for z in qkv.double().chunk(3, dim=1))
    s = torch.einsum("bhdi,bhdj->bhij", q, k) / dh ** 0.5 + alibi(slopes, t, t, torch.float64)
    m = torch.full((b, heads, t), -float("inf"), dtype=torch.float64)
    l = torch.zeros(b, heads, t, dtype=torch.float64)
    o = torch.zeros(b, heads, dh, t, dtype=torch.float64)
    for j0 in range(0, t, key_block):
        sb = s[..., j0:j0 + key_block]
        mn = torch.maximum(m, sb.max(-1).values)
        a = (m - mn).exp()
        pe = (sb - mn.unsqueeze(-1)).exp()
        l = l * a + pe.sum(-1)
        o = o * a.unsqueeze(2) + torch.einsum("bhij,bhdj->bhdi", _bf16(pe), v[..., j0:j0 + key_block])
        m = mn
    return (o / l.unsqueeze(2)).reshape(b, heads * dh, t)


@dataclass
class Ref:
    """fp64 result(s) and the fp32-CPU yardstick of one case; ``want`` / ``err_max`` / ``err_rms`` are keyed by output name."""
    want: Dict[str, Tensor]
    err_max: Dict[str, float]
    err_rms: Dict[str, float]


def _ref(fn: Callable[[torch.dtype], Dict[str, Tensor]]) -> Ref:
    w64, w32 = fn(torch.float64), fn(torch.float32)
    err_max = {n: float((w32[n].double() - w64[n]).abs().max()) for n in w64}
    err_rms = {n: float((w32[n].double() - w64[n]).pow(2).mean().sqrt()) for n in w64}
    return Ref(w64, err_max, err_rms)


def self_reference(case: AttnCase, dout: Optional[Tensor] = None) -> Ref:
    """``out`` (and with ``dout`` the gradient ``dqkv``) of self-attention: fp64, and their fp32-CPU error."""
    def run(dtype):
        x = case.qkv.detach().to(dtype).clone().requires_grad_(dout is not None)
        o = self_core(x, case.slopes, case.heads, case.dh)
        res = {"out": o.detach()}
        if dout is not None:
            o.backward(dout.to(dtype))
            res["dqkv"] = x.grad
        return res
    return _ref(run)


def cross_reference(case: AttnCase, dout: Optional[Tensor] = None) -> Ref:
    """``out`` (and with ``dout`` the gradient, ``dq`` and ``dkv`` concatenated along the channels like the self kernels'
    ``dqkv`` when Tq == Tk, else flattened one after the other) of cross-attention."""
    def run(dtype):
        q = case.q.detach().to(dtype).clone().requires_grad_(dout is not None)
        kv = case.kv.detach().to(dtype).clone().requires_grad_(dout is not None)
        o = cross_core(q, kv, case.slopes, case.heads, case.dh, case.scale_div)
        res = {"out": o.detach()}
        if dout is not None:
            o.backward(dout.to(dtype))
            res["dq"], res["dkv"] = q.grad, kv.grad
            res["grad"] = torch.cat([q.grad.flatten(), kv.grad.flatten()])
        return res
    return _ref(run)


def floor_of(want: Tensor) -> float:
    """Four ulp (fp32) at the output scale."""
    return 4 * 2.0 ** -23 * max(1.0, float(want.abs().max()))


def measure(got: Tensor, ref: Ref, name: str) -> Tuple[float, float, float, float, float]:
    """(err_gpu max, err_gpu rms, err32 max, err32 rms, floor) of ``got`` against ``ref.want[name]``."""
    want = ref.want[name]
    d = got.detach().cpu().double().reshape(want.shape) - want
    return float(d.abs().max()), float(d.pow(2).mean().sqrt()), ref.err_max[name], ref.err_rms[name], floor_of(want)


def needed(e_gpu: float, e32: float, floor: float) -> float:
    """The smallest M with ``e_gpu <= M * e32 + floor`` (0 inside the floor, inf where only the floor could cover it)."""
    if e_gpu <= floor:
        return 0.0
    return (e_gpu - floor) / e32 if e32 > 0 else float("inf")


def check(label: str, got: Tensor, ref: Ref, name: str, m: float, slack: float = 1.0) -> None:
    """Print the figures, then assert ``err_gpu <= slack * (m * err32 + floor)`` for the maximum and for the RMS."""
    assert torch.isfinite(got).all(), f"{label}: non-finite values"
    g_max, g_rms, e_max, e_rms, floor = measure(got, ref, name)
    print(f"YARDSTICK {label} {name}: gpu max {g_max:.3e} rms {g_rms:.3e} | fp32 max {e_max:.3e} rms {e_rms:.3e} | floor {floor:.3e} "
          f"| M needed max {needed(g_max, e_max, floor):.2f} rms {needed(g_rms, e_rms, floor):.2f}")
    assert g_max <= slack * (m * e_max + floor), (label, name, "max", g_max, e_max, floor)
    assert g_rms <= slack * (m * e_rms + floor), (label, name, "rms", g_rms, e_rms, floor)


# ---------------------------------------------------------------------------------------------------------------- shape list
B, HEADS = 2, 3
# forward, fp32: (head_dim, t, flash) -- one or two t per attention_alibi<NJ,DVT> row, then the online-softmax rows
SINGLE_PASS_SHAPES = [(8, 1), (8, 33), (33, 31), (65, 64),            # NJ 2 (t <= 64):   DVT 1, 1, 2, 4
                      (8, 65), (64, 128), (128, 65),                  # NJ 4 (t <= 128):  DVT 1, 2, 4
                      (8, 255), (33, 129), (64, 256), (128, 129), (65, 256)]   # NJ 8: DVT 1, 2, 2, 4, 4
FLASH_SHAPES = [(8, 321, False), (33, 130, True), (64, 257, False), (65, 130, True), (128, 321, False)]
# forward, bf16: (head_dim, t).  K and V fit the LDS up to t = 1024 / 512 / 256 for DVT 1 / 2 / 4, so the streamed rows
# attention_flash<1,1> and <2,1> start at t = 1025 and 513: no smaller shape reaches them
BF16_SHAPES = [(8, 129), (33, 31), (64, 255), (128, 256), (8, 1025), (33, 513), (65, 257)]
# cross-attention: (head_dim, tq, tk)
CROSS_LENGTHS = [(1, 257), (257, 1), (65, 130), (130, 65), (128, 128)]
CROSS_FORWARD_SHAPES = [(dh, tq, tk) for dh in (16, 128) for tq, tk in CROSS_LENGTHS] + [(33, 65, 130), (33, 130, 65)]
CROSS_BACKWARD_SHAPES = [(dh, tq, tk) for dh in (16, 128) for tq, tk in CROSS_LENGTHS]
# backward: (head_dim, t, split)
BACKWARD_SHAPES = [(64, 225, False), (64, 256, False), (16, 40, False), (128, 130, True), (33, 257, True)]

ALL_SINGLE_PASS_ROWS = {f"attention_alibi<{nj},{dvt}>" for nj in (2, 4, 8) for dvt in (1, 2, 4)}
ALL_FLASH_ROWS = {f"attention_flash<{dvt},{prec}>" for dvt in (1, 2, 4) for prec in (0, 1)}
ALL_BF16_LDS_ROWS = {f"attention_bf16_lds<{dvt}>" for dvt in (1, 2, 4)}
ALL_CROSS_ROWS = {f"attention_cross<{dvt}>" for dvt in (1, 2, 4)}
ALL_BACKWARD_ROWS = {"attention_alibi_bwd<16>", "attention_alibi_bwd<8>", "attn_bwd_stats+attn_bwd_dq+attn_bwd_dkv"}


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
LN_EPS = 1e-5
LN_CONSTANTS = (2.5, -1.25, 0.0, 1024.0)    # C of each (C <= 2100) is exact in fp32, so a constant column's mean is exact


def ln_constant_columns(t: int) -> Tensor:
    """Which of the ``t`` columns the ``constant`` family makes constant (every third, starting with column 0)."""
    return torch.arange(t) % 3 == 0


def ln_input(family: str, b: int, c: int, t: int, seed: int) -> Tensor:
    g = _gen(seed)
    x = torch.randn(b, c, t, generator=g)
    if family == "gauss":
        return x
    if family == "offset":
        return 1e3 + x
    if family == "constant":
        cols = ln_constant_columns(t).nonzero().flatten()
        for n, col in enumerate(cols.tolist()):
            x[:, :, col] = LN_CONSTANTS[n % len(LN_CONSTANTS)]
        return x
    if family == "outlier":
        x[:, (3 * c) // 7] = 1e4
        return x
    raise KeyError(family)


LN_FAMILIES = ("gauss", "offset", "constant", "outlier")
LN_CHANNELS = (63, 65, 129, 256, 257, 500, 513, 1000, 1024, 1025, 2048, 2049, 2100)
LN_LENGTHS = (1, 17, 65)
LN_BATCH = 2


def ln_params(c: int, seed: int) -> Tuple[Tensor, Tensor]:
    g = _gen(seed + 1)
    return 1.0 + 0.5 * torch.randn(c, generator=g), 0.5 * torch.randn(c, generator=g)


def ln_reference(x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], dy: Optional[Tensor] = None,
                 add: Optional[Tensor] = None) -> Ref:
    """``y`` of LayerNorm over the channels of (B, C, T) (``F.layer_norm`` on the transposed tensor), with ``dy`` also ``dx``
    (+ ``add``), ``dweight`` and ``dbias`` by autograd: fp64 and the fp32-CPU error."""
    c = x.shape[1]

    def run(dtype):
        xx = x.detach().to(dtype).clone().requires_grad_(dy is not None)
        w = torch.ones(c, dtype=dtype) if weight is None else weight.detach().to(dtype).clone()
        bb = torch.zeros(c, dtype=dtype) if bias is None else bias.detach().to(dtype).clone()
        w, bb = w.requires_grad_(dy is not None), bb.requires_grad_(dy is not None)
        y = F.layer_norm(xx.transpose(1, 2), (c,), w, bb, LN_EPS).transpose(1, 2)
        res = {"y": y.detach()}
        if dy is not None:
            y.backward(dy.to(dtype))
            res["dx"] = xx.grad if add is None else xx.grad + add.to(dtype)
            res["dweight"], res["dbias"] = w.grad, bb.grad
        return res
    return _ref(run)
