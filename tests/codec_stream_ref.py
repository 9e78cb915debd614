"""Float64 restatement of what a codec stream computes, and the derived error bound of one step.

Everything is on the channel-major tensor.  A stream advances in whole latent frames; ``pos[b]`` counts the frames row ``b`` has
received.  A layer has a rate ``r`` (columns per frame), a left reach ``H`` (input columns before the newest chunk that it reads)
and a cumulative delay ``D`` (in its output columns):

    causal(k, s, d)   output j reads  j s - (d (k - 1) - s + 1) ... j s + s - 1      H = d (k - 1) - s + 1   r / s, D / s
    convt(k, 1)       output j reads  j - (k - 1) ... j                              H = k - 1               r, D
    up(2 s + 1, s)    output j reads  (j - s) // s ... (j + s) // s                  H = 2                   r s, D s + s
    res(d)            leaky(x + conv_1(leaky(conv_7,d(x) + b1)) + b2), reads j - 6 d ... j                    r, D

A step of ``n`` frames produces the ``n r_out`` columns ``[pos r_out - D_out, (pos + n) r_out - D_out)``; column ``j`` is stored as
exact 0 unless ``0 <= j < end[b] r_out``.  State is a ring of the layer's INPUT of capacity ``H + max_chunk r_in``, column ``i`` at
``i mod cap`` (floor mod).  Written with index gathers, not with ``F.conv1d``: the index rule IS the statement.

Bound of one op on fp32 operands (``U`` as in tests/conformer_ref.py): ``(c_in K + 2) U (sum |w| |x| + |bias|)`` -- c_in K fused
multiply-adds in any order, the bias add and the activation's multiply; the polyphase weights of ``up`` are sums of at most
``ceil(K / 3)`` taps formed in fp32, which the factor covers because ``c_in K >= 3 c_in + K / 3 + 1``.  The residual add rounds
once more: ``+ U (|res| + |conv|)``, and so does the activation behind it.  A residual unit runs as two ops with the hidden
activation in fp32: conv1's bound (plus one ``U |h|`` for storing h) is carried through ``|w2|`` (LeakyReLU is 1-Lipschitz) and
conv2's own is added.
"""
import torch

from tests.conformer_ref import U

LIVE = (1 << 63) - 1
SLOPE = 0.1


def leaky(v, slope=SLOPE):
    return torch.where(v > 0, v, v * slope)


class Op:
    """One conv of a stream.  ``w`` in torch's layout for the kind -- (c_out, c_in, k), for "convt" (c_in, c_out, k) -- already
    folded; ``pre`` / ``post``: LeakyReLU slopes before / after the residual add (None = none)."""

    def __init__(self, kind, w, bias, s=1, d=1, pre=None, post=None, residual=False):
        assert kind in ("causal", "convt", "up")
        self.kind, self.s, self.d, self.pre, self.post, self.residual = kind, int(s), int(d), pre, post, residual
        self.w = (w.transpose(0, 1) if kind == "convt" else w).double().contiguous()     # (c_out, c_in, k)
        self.bias = None if bias is None else bias.double()
        self.c_out, self.c_in, self.k = self.w.shape
        assert kind != "convt" or self.s == 1
        assert kind != "up" or self.k == 2 * self.s + 1

    @property
    def reach(self):
        return {"causal": self.d * (self.k - 1) - self.s + 1, "convt": self.k - 1, "up": 2}[self.kind]

    def rates(self, rate_in, delay_in):
        if self.kind == "causal":
            assert rate_in % self.s == 0 and delay_in % self.s == 0
            return rate_in // self.s, delay_in // self.s
        if self.kind == "up":
            return rate_in * self.s, delay_in * self.s + self.s
        return rate_in, delay_in

    def reads(self, j):
        """(len(j), k) input columns that the output columns ``j`` read, tap by tap."""
        t = torch.arange(self.k, dtype=torch.int64)
        j = j.reshape(-1, 1)
        if self.kind == "causal":
            return j * self.s - (self.d * (self.k - 1) - self.s + 1) + t * self.d
        if self.kind == "convt":
            return j - t
        return torch.div(j + t - (self.k - 1) // 2, self.s, rounding_mode="floor")


def _valid(j, end_r, rate_out, mask_start=True, mask_end=True):
    """Column ``j`` is the signal's own iff ``0 <= j < end rate_out``."""
    valid = torch.ones_like(j, dtype=torch.bool)
    if mask_start:
        valid &= j >= 0
    if mask_end and end_r != LIVE:
        valid &= j < end_r * rate_out
    return valid


def step(op, src, dst, pos, end, n, rate_in, delay_in, src_ring=True, dst_ring=True, res=None, mask_start=True, mask_end=True):
    """One step of ``op`` for every row, float64, in place on ``dst``; returns (produced block (B, c_out, n r_out), its bound).
    ``src`` / ``dst`` / ``res``: rings (B, C, cap) -- or plain tensors of the step's own columns with ``*_ring=False``;
    ``pos`` / ``end``: lists of ints (``end=None``: no mask).  ``mask_start`` / ``mask_end`` switch the two sides of the validity
    mask off: tests use that to show the reference needs them."""
    b = src.shape[0]
    rate_out, delay_out = op.rates(rate_in, delay_in)
    out = torch.zeros(b, op.c_out, n * rate_out, dtype=torch.float64)
    bound = torch.zeros_like(out)
    wabs = op.w.abs()
    for r in range(b):
        j = torch.arange(pos[r] * rate_out - delay_out, (pos[r] + n) * rate_out - delay_out, dtype=torch.int64)
        idx = op.reads(j)                                                    # (n_out, k)
        first_new = pos[r] * rate_in - delay_in
        assert int(idx.max()) < first_new + n * rate_in, "a layer reads a column that has not been produced"
        if src_ring:
            cap = src.shape[2]
            assert int(idx.min()) >= first_new + n * rate_in - cap, "a layer reads behind its ring"
            xg = src[r][:, torch.remainder(idx, cap)]                        # (c_in, n_out, k)
        else:
            local = idx - first_new
            ok = (local >= 0) & (local < n * rate_in)
            xg = src[r][:, local.clamp(0, n * rate_in - 1)] * ok
        v = torch.einsum("oik,ijk->oj", op.w, xg)
        mag = torch.einsum("oik,ijk->oj", wabs, xg.abs())
        if op.bias is not None:
            v = v + op.bias[:, None]
            mag = mag + op.bias.abs()[:, None]
        bd = (op.c_in * op.k + 2) * U * mag
        if op.pre is not None:
            v = leaky(v, op.pre)
        if op.residual:
            rr = res[r][:, torch.remainder(j, res.shape[2])]
            bd = bd + U * (rr.abs() + v.abs())
            v = v + rr
        if op.post is not None:
            bd = bd + U * v.abs()
            v = leaky(v, op.post)
        if end is not None:
            valid = _valid(j, end[r], rate_out, mask_start, mask_end)
            v, bd = v * valid, bd * valid
        out[r], bound[r] = v, bd
        if dst_ring:
            dst[r][:, torch.remainder(j, dst.shape[2])] = v
        else:
            dst[r] = v
    return out, bound


def ring_write(ring, x, pos, rate):
    """The stack's input chunk (B, C, n rate) into its first ring."""
    for r in range(x.shape[0]):
        j = torch.arange(pos[r] * rate, pos[r] * rate + x.shape[2], dtype=torch.int64)
        ring[r][:, torch.remainder(j, ring.shape[2])] = x[r].double()


def res_unit_step(op1, op2, ring, dst, pos, end, n, rate, delay, dst_ring=True, **mask):
    """A residual unit as the two ops a stream runs: ``op1`` (k = 7 dilated, LeakyReLU) into a plain hidden tensor, ``op2`` (k = 1,
    residual from ``ring``, LeakyReLU, mask).  Returns (block, bound)."""
    b = ring.shape[0]
    h = torch.zeros(b, op1.c_out, n * rate, dtype=torch.float64)
    _, b1 = step(op1, ring, h, pos, None, n, rate, delay, dst_ring=False)
    out, b2 = step(op2, h, dst, pos, end, n, rate, delay, src_ring=False, dst_ring=dst_ring, res=ring, **mask)
    carried = torch.einsum("oi,bij->boj", op2.w[:, :, 0].abs(), b1 + U * h.abs())
    if end is not None:                                                      # masked columns are exact zeros
        for r in range(b):
            j = torch.arange(pos[r] * rate - delay, (pos[r] + n) * rate - delay, dtype=torch.int64)
            carried[r] = carried[r] * _valid(j, end[r], rate, **mask)
    return out, b2 + carried


# --------------------------------------------------------------------------- a whole stack, from the oracle's state dict
class Unit:
    def __init__(self, ops):
        self.ops = ops              # [op] or [op1, op2] of a residual unit


def stack_units(sd, spec, which):
    """The units of ``oracle.codec``'s encoder / decoder (``encoder_stages`` / ``decoder_stages``) as stream ops, from a state
    dict in the reference's layout.  No wavelet / multires blocks."""
    from oracle import codec
    nd = len(spec.dilations)

    def res(prefix, d):
        w1, b1 = codec.conv_params(sd, prefix + "conv1.conv.")
        w2, b2 = codec.conv_params(sd, prefix + "conv2.conv.")
        return Unit([Op("causal", w1, b1, d=d, pre=SLOPE), Op("causal", w2, b2, residual=True, post=SLOPE)])

    units = []
    if which == "encoders":
        units.append(Unit([Op("causal", *codec.conv_params(sd, "encoders.0.1.conv."))]))
        for i in range(spec.n_blocks):
            p = f"encoders.{i + 1}.layers."
            units += [res(f"{p}{j}.0.", d) for j, d in enumerate(spec.dilations)]
            units.append(Unit([Op("causal", *codec.conv_params(sd, f"{p}{nd}.0.conv."), s=int(spec.strides[i]), pre=SLOPE)]))
        units.append(Unit([Op("causal", *codec.conv_params(sd, f"encoders.{spec.n_blocks + 1}.conv."))]))
    else:
        units.append(Unit([Op("convt", *codec.conv_params(sd, "decoders.0.conv."))]))
        for n in range(1, spec.n_blocks + 1):
            s = int(spec.strides[spec.n_blocks - n])
            p = f"decoders.{n}."
            units.append(Unit([Op("up", *codec.conv_params(sd, p + "in_conv.0.conv."), s=s, pre=SLOPE)]))
            units += [res(f"{p}layers.{j}.0.", d) for j, d in enumerate(spec.dilations)]
        units.append(Unit([Op("causal", *codec.conv_params(sd, f"decoders.{spec.n_blocks + 1}.conv."))]))
    return units


class StackStream:
    """A stack on tight rings: plan (rate, delay, reach, cap per unit) derived here, independently of the package's."""

    def __init__(self, units, rate0, batch, max_chunk, masked, mask_start=True, mask_end=True):
        self.units, self.batch, self.max_chunk, self.masked = units, batch, max_chunk, masked
        self.mask = dict(mask_start=mask_start, mask_end=mask_end)
        self.plan, rate, delay = [], rate0, 0
        for u in units:
            op = u.ops[0]
            reach = op.d * (op.k - 1) if len(u.ops) == 2 else op.reach
            rate_out, delay_out = op.rates(rate, delay)
            self.plan.append((rate, delay, reach, reach + max_chunk * rate))
            rate, delay = rate_out, delay_out
        self.rate_out, self.delay_out = rate, delay
        self.rings = [torch.zeros(batch, u.ops[0].c_in, p[3], dtype=torch.float64) for u, p in zip(units, self.plan)]
        self.pos = [0] * batch
        self.end = [LIVE] * batch

    def finish(self):
        self.end = list(self.pos)

    def run(self, x):
        n, rest = divmod(x.shape[2], self.plan[0][0])
        assert rest == 0 and 1 <= n <= self.max_chunk
        ring_write(self.rings[0], x, self.pos, self.plan[0][0])
        end = self.end if self.masked else None
        out = None
        for i, (u, (rate, delay, _, _)) in enumerate(zip(self.units, self.plan)):
            last = i + 1 == len(self.units)
            c_out = u.ops[-1].c_out
            dst = torch.zeros(self.batch, c_out, n * u.ops[0].rates(rate, delay)[0], dtype=torch.float64) if last else self.rings[i + 1]
            if len(u.ops) == 2:
                out, _ = res_unit_step(u.ops[0], u.ops[1], self.rings[i], dst, self.pos, end, n, rate, delay, dst_ring=not last,
                                       **self.mask)
            else:
                out, _ = step(u.ops[0], self.rings[i], dst, self.pos, end, n, rate, delay, dst_ring=not last, **self.mask)
        self.pos = [p + n for p in self.pos]
        return out
