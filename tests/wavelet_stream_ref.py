"""Float64 restatement of a wavelet decoder block inside a codec stream, and the derived error bound of its steps.

In the terms of tests/codec_stream_ref.py.  The block sits at rate ``r`` (columns per frame) with delay ``D``; ``conv_in`` is a "same"
conv of ``k_in`` taps (``p_in = (k_in - 1) / 2``), the fold has scale ``s`` over ``P`` points, ``conv_out`` is a "same" conv of
``k_out`` taps (``p_out``).  ``L = end r`` is the signal's length at the block's input, infinite while the row is live.

    in-step    h columns [pos r - D_h, (pos + n) r - D_h), D_h = D + p_in:  h[l] = b + sum_j W[j] x[l + j - p_in], exact 0 unless
               0 <= l < L; reads k_in - 1 columns behind the chunk's first new one.
    out-step   columns [pos r s - D_out, (pos + n) r s - D_out), D_out = D_h s + s + p_out:
               out[u] = act(b + sum_{c, j} Wo[o, c, j] y[c, u + j - p_out]), exact 0 unless 0 <= u < L s, with l0 = v // s, ph = v - l0 s,
                   y[c, v] = 0                                                      v < 0 or v >= L s
                   y[c, v] = h[c, l0] S_hi[c, ph] (+ h[c, l0 + 1] S_lo[c, ph], ph > 0)   v < (L - 1) s + 1
                   y[c, v] = tail[c, v - ((L - 1) s + 1)] h[c, L - 1]                the reference's raw tail
               reads 1 + ceil(2 p_out / s) columns of h behind the step's first new one.

Index gathers and ``torch.where`` selects only: the index rule IS the statement.  Both steps assert that they read no column that has
not been produced and none behind the ring, the stream that every tail column is computed after ``finish``.

Bound of the out-step on fp32 operands (the h ring and the table as the device holds them): the conv bound of codec_stream_ref,
``(hidden k_out + 2) U (sum |Wo| |y| + |b|)``, plus the two roundings of y -- the product h0 S_hi and the fused multiply-add -- carried
through ``|Wo|``: ``sum |Wo| U (2 |h0 S_hi| + |h1 S_lo|)`` (one rounding, ``U |y|``, in the tail).  A whole unit adds the in-step's bound
and one ``U |h|`` for storing h, carried through ``|S_hi| + |S_lo|`` and ``|Wo|``.
"""
import torch

from tests.codec_stream_ref import LIVE, SLOPE, Op, U, Unit, leaky, res_unit_step, ring_write, step

__all__ = ["LIVE", "SLOPE", "U", "leaky", "ring_write", "WaveletUnit", "kern64", "fold_table64", "in_step", "out_step", "unit_step",
           "stack_units", "StackStream"]


def kern64(space, sigma, channels):
    """(channels, P) float64: cos(t) exp(-t^2 / sigma_c)."""
    t = space.reshape(1, -1).double()
    sg = sigma.reshape(-1, 1).double().expand(channels, 1) if sigma.numel() == 1 else sigma.reshape(channels, 1).double()
    return torch.cos(t) * torch.exp(-(t * t) / sg)


def fold_table64(space, sigma, channels, s):
    """(channels, 3 s - 1) float64 = [S_hi | S_lo | tail]: S_hi[ph] = sum_{p >= ph fold} kern[p], S_lo[ph] = sum_{p < ph fold} kern[p],
    tail = kern[P - (s - 1):]."""
    k = kern64(space, sigma, channels)
    p = k.shape[1]
    assert s >= 2 and p % s == 0
    fold = p // s
    hi = torch.stack([k[:, ph * fold:].sum(1) for ph in range(s)], 1)
    lo = torch.stack([k[:, :ph * fold].sum(1) for ph in range(s)], 1)
    return torch.cat([hi, lo, k[:, p - (s - 1):]], 1)


class WaveletUnit:
    """``w_in`` (hidden, c_in, k_in), ``w_out`` (c_out, hidden, k_out) in torch's layout; ``table`` (hidden, 3 s - 1); ``post``: the
    LeakyReLU slope behind the block (None = none)."""

    def __init__(self, w_in, b_in, w_out, b_out, table, s, post=None):
        self.w_in, self.w_out = w_in.double().contiguous(), w_out.double().contiguous()
        self.b_in = None if b_in is None else b_in.double()
        self.b_out = None if b_out is None else b_out.double()
        self.table, self.s, self.post = table.double(), int(s), post
        self.hidden, self.c_in, self.k_in = self.w_in.shape
        self.c_out, hid, self.k_out = self.w_out.shape
        assert hid == self.hidden and self.k_in % 2 == 1 and self.k_out % 2 == 1 and self.s >= 2
        assert tuple(self.table.shape) == (self.hidden, 3 * self.s - 1)
        self.p_in, self.p_out = (self.k_in - 1) // 2, (self.k_out - 1) // 2

    @property
    def reach(self):
        return self.k_in - 1

    @property
    def reach_h(self):
        return 1 + -((-2 * self.p_out) // self.s)

    def delay_h(self, delay_in):
        return delay_in + self.p_in

    def rates(self, rate_in, delay_in):
        return rate_in * self.s, self.delay_h(delay_in) * self.s + self.s + self.p_out


def _signal_len(end_r, rate):
    return None if end_r == LIVE else end_r * rate


def in_step(unit, src, hring, pos, end, n, rate, delay, mask_start=True, mask_end=True):
    """The in-step for every row, float64, in place on the ring ``hring``; returns (block (B, hidden, n rate), its bound)."""
    b, cap = src.shape[0], src.shape[2]
    d_h = unit.delay_h(delay)
    out = torch.zeros(b, unit.hidden, n * rate, dtype=torch.float64)
    bound = torch.zeros_like(out)
    t = torch.arange(unit.k_in, dtype=torch.int64)
    for r in range(b):
        l = torch.arange(pos[r] * rate - d_h, (pos[r] + n) * rate - d_h, dtype=torch.int64)
        idx = l.reshape(-1, 1) + t - unit.p_in
        first_new = pos[r] * rate - delay
        assert int(idx.max()) < first_new + n * rate, "the in-step reads a column that has not been produced"
        assert int(idx.min()) >= first_new + n * rate - cap, "the in-step reads behind its ring"
        xg = src[r][:, torch.remainder(idx, cap)]                              # (c_in, n_out, k)
        v = torch.einsum("oik,ijk->oj", unit.w_in, xg)
        mag = torch.einsum("oik,ijk->oj", unit.w_in.abs(), xg.abs())
        if unit.b_in is not None:
            v, mag = v + unit.b_in[:, None], mag + unit.b_in.abs()[:, None]
        bd = (unit.c_in * unit.k_in + 2) * U * mag
        length = _signal_len(end[r], rate)
        valid = torch.ones_like(l, dtype=torch.bool)
        if mask_start:
            valid &= l >= 0
        if mask_end and length is not None:
            valid &= l < length
        zero = torch.zeros((), dtype=torch.float64)
        v, bd = torch.where(valid, v, zero), torch.where(valid, bd, zero)
        out[r], bound[r] = v, bd
        hring[r][:, torch.remainder(l, hring.shape[2])] = v
    return out, bound


def fold_operand(unit, hrow, v, length, first_new, n_new, tail=True, mask_end=True):
    """y[c, v] for the index array ``v`` of any shape from one row's ring ``hrow`` (hidden, cap) -> (y, its rounding bound, the
    sensitivity |dy / dh| summed over the two taps).  ``length``: L or None while live; ``first_new`` / ``n_new``: the first column
    of h the running step produced and how many -- for the two assertions."""
    s, cap, tab = unit.s, hrow.shape[1], unit.table
    l0 = torch.div(v, s, rounding_mode="floor")
    ph = v - l0 * s
    inside = v >= 0
    is_tail = torch.zeros_like(inside)
    if length is not None:
        if mask_end:
            inside &= v < length * s
        if tail:
            is_tail = inside & (v >= (length - 1) * s + 1) & (v < length * s)
    two = inside & ~is_tail
    second = two & (ph > 0)
    read = torch.cat([l0[two], (l0 + 1)[second]] + ([torch.tensor([length - 1])] if bool(is_tail.any()) else []))
    if read.numel():
        assert int(read.max()) < first_new + n_new, "the out-step reads a column of h that has not been produced"
        assert int(read.min()) >= first_new + n_new - cap, "the out-step reads behind the ring of h"
    zero = torch.zeros((), dtype=torch.float64)
    h0 = hrow[:, torch.remainder(l0, cap)]
    h1 = hrow[:, torch.remainder(l0 + 1, cap)]
    a = h0 * tab[:, ph]                                                        # tab[:, ph]: (hidden, *v.shape)
    bq = h1 * tab[:, s + ph]
    y = torch.where(second, a + bq, a)                                         # a select: h1 behind ph == 0 may be stale
    ybd = U * torch.where(second, 2 * a.abs() + bq.abs(), a.abs())
    sens = torch.where(second, tab[:, ph].abs() + tab[:, s + ph].abs(), tab[:, ph].abs())
    if bool(is_tail.any()):
        e = (v - ((length - 1) * s + 1)).clamp(0, s - 2)
        tt = tab[:, 2 * s + e]
        yt = tt * hrow[:, (length - 1) % cap][:, None].reshape([-1] + [1] * v.dim())
        y = torch.where(is_tail, yt, y)
        ybd = torch.where(is_tail, U * yt.abs(), ybd)
        sens = torch.where(is_tail, tt.abs(), sens)
    return torch.where(inside, y, zero), torch.where(inside, ybd, zero), torch.where(inside, sens, zero)


def out_step(unit, hring, dst, pos, end, n, rate, delay_h, dst_ring=True, tail=True, mask_start=True, mask_end=True, h_bound=None):
    """The out-step for every row, float64, in place on ``dst``; returns (block (B, c_out, n rate s), its bound).  ``hring``: the ring
    of h, rate ``rate``, delay ``delay_h``.  ``h_bound`` (B, hidden, cap), optional: a bound on the error of the ring's content, carried
    into the result's.  ``tail`` / ``mask_*``: switches that tests use to show the statement needs them."""
    b, s = hring.shape[0], unit.s
    rate_out, d_out = rate * s, delay_h * s + s + unit.p_out
    out = torch.zeros(b, unit.c_out, n * rate_out, dtype=torch.float64)
    bound = torch.zeros_like(out)
    t = torch.arange(unit.k_out, dtype=torch.int64)
    wabs = unit.w_out.abs()
    for r in range(b):
        u = torch.arange(pos[r] * rate_out - d_out, (pos[r] + n) * rate_out - d_out, dtype=torch.int64)
        v = u.reshape(-1, 1) + t - unit.p_out                                  # (n_out, k)
        length = _signal_len(end[r], rate)
        y, ybd, sens = fold_operand(unit, hring[r], v, length, pos[r] * rate - delay_h, n * rate, tail, mask_end)
        if h_bound is not None:
            cap = hring.shape[2]
            l0 = torch.div(v, s, rounding_mode="floor")
            hb = torch.maximum(h_bound[r][:, torch.remainder(l0, cap)], h_bound[r][:, torch.remainder(l0 + 1, cap)])
            ybd = ybd + sens * torch.where(sens > 0, hb, torch.zeros((), dtype=torch.float64))
        val = torch.einsum("oik,ijk->oj", unit.w_out, y)
        mag = torch.einsum("oik,ijk->oj", wabs, y.abs())
        if unit.b_out is not None:
            val, mag = val + unit.b_out[:, None], mag + unit.b_out.abs()[:, None]
        bd = (unit.hidden * unit.k_out + 2) * U * mag + torch.einsum("oik,ijk->oj", wabs, ybd)
        if unit.post is not None:
            val = leaky(val, unit.post)
        valid = torch.ones_like(u, dtype=torch.bool)
        if mask_start:
            valid &= u >= 0
        if mask_end and length is not None:
            valid &= u < length * s
        zero = torch.zeros((), dtype=torch.float64)
        val, bd = torch.where(valid, val, zero), torch.where(valid, bd, zero)
        out[r], bound[r] = val, bd
        if dst_ring:
            dst[r][:, torch.remainder(u, dst.shape[2])] = val
        else:
            dst[r] = val
    return out, bound


def unit_step(unit, ring, hring, dst, pos, end, n, rate, delay, dst_ring=True, tail=True, **mask):
    """A wavelet unit as the two steps a stream runs.  Returns (block, bound): the out-step's own bound plus the in-step's (and one
    ``U |h|`` for storing h) carried through the fold and ``|Wo|`` -- for the columns of h this step produced; older ones carry the
    same kind of error, which the caller's factor on the bound covers as it does for a stack."""
    h, hb = in_step(unit, ring, hring, pos, end, n, rate, delay, **mask)
    carried = torch.zeros_like(hring)
    d_h = unit.delay_h(delay)
    for r in range(ring.shape[0]):
        l = torch.arange(pos[r] * rate - d_h, (pos[r] + n) * rate - d_h, dtype=torch.int64)
        carried[r][:, torch.remainder(l, hring.shape[2])] = hb[r] + U * h[r].abs()
    return out_step(unit, hring, dst, pos, end, n, rate, d_h, dst_ring=dst_ring, tail=tail, h_bound=carried, **mask)


# --------------------------------------------------------------------------- a whole decoder stack, from the oracle's state dict
def stack_units(sd, spec):
    """The decoder units of ``oracle.codec.decoder_stages`` as stream units, wavelet blocks included."""
    from oracle import codec

    def res(prefix, d):
        w1, b1 = codec.conv_params(sd, prefix + "conv1.conv.")
        w2, b2 = codec.conv_params(sd, prefix + "conv2.conv.")
        return Unit([Op("causal", w1, b1, d=d, pre=SLOPE), Op("causal", w2, b2, residual=True, post=SLOPE)])

    units = [Unit([Op("convt", *codec.conv_params(sd, "decoders.0.conv."))])]
    for n in range(1, spec.n_blocks + 1):
        s = int(spec.strides[spec.n_blocks - n])
        p = f"decoders.{n}."
        if spec.decoder_is_wavelet(n):
            q = p + "in_conv.0."
            hidden = sd[q + "conv_in.weight"].shape[0]
            table = fold_table64(sd[q + "space"], sd[q + "wavelet_scale"], hidden, s)
            units.append(WaveletUnit(sd[q + "conv_in.weight"], sd.get(q + "conv_in.bias"), sd[q + "conv_out.weight"],
                                     sd.get(q + "conv_out.bias"), table, s, post=SLOPE))
        else:
            units.append(Unit([Op("up", *codec.conv_params(sd, p + "in_conv.0.conv."), s=s, pre=SLOPE)]))
        units += [res(f"{p}layers.{j}.0.", d) for j, d in enumerate(spec.dilations)]
    units.append(Unit([Op("causal", *codec.conv_params(sd, f"decoders.{spec.n_blocks + 1}.conv."))]))
    return units


class StackStream:
    """``codec_stream_ref.StackStream`` with wavelet units: tight rings, one more (of h) per wavelet unit, the plan derived here,
    independently of the package's.  ``tail`` / ``mask_*``: switches of the statement."""

    def __init__(self, units, rate0, batch, max_chunk, tail=True, mask_start=True, mask_end=True):
        self.units, self.batch, self.max_chunk, self.tail = units, batch, max_chunk, tail
        self.mask = dict(mask_start=mask_start, mask_end=mask_end)
        self.plan, self.hidden, rate, delay = [], [], rate0, 0
        for u in units:
            if isinstance(u, WaveletUnit):
                reach, (rate_out, delay_out) = u.reach, u.rates(rate, delay)
                self.hidden.append(torch.zeros(batch, u.hidden, u.reach_h + max_chunk * rate, dtype=torch.float64))
            else:
                op = u.ops[0]
                reach = op.d * (op.k - 1) if len(u.ops) == 2 else op.reach
                rate_out, delay_out = op.rates(rate, delay)
                self.hidden.append(None)
            self.plan.append((rate, delay, reach, reach + max_chunk * rate))
            rate, delay = rate_out, delay_out
        self.rate_out, self.delay_out = rate, delay
        self.rings = [torch.zeros(batch, u.c_in if isinstance(u, WaveletUnit) else u.ops[0].c_in, p[3], dtype=torch.float64)
                      for u, p in zip(units, self.plan)]
        self.pos = [0] * batch
        self.end = [LIVE] * batch

    def finish(self):
        for u, (rate, delay, _, _) in zip(self.units, self.plan):
            if isinstance(u, WaveletUnit):               # no tail column has been produced yet: D_out > s - 1
                rate_out, d_out = u.rates(rate, delay)
                assert all(p * rate_out - d_out <= (p * rate - 1) * u.s + 1 for p in self.pos), "a tail column precedes finish()"
        self.end = list(self.pos)

    def run(self, x):
        n, rest = divmod(x.shape[2], self.plan[0][0])
        assert rest == 0 and 1 <= n <= self.max_chunk
        ring_write(self.rings[0], x, self.pos, self.plan[0][0])
        out = None
        for i, (u, (rate, delay, _, _)) in enumerate(zip(self.units, self.plan)):
            last = i + 1 == len(self.units)
            if isinstance(u, WaveletUnit):
                dst = torch.zeros(self.batch, u.c_out, n * rate * u.s, dtype=torch.float64) if last else self.rings[i + 1]
                out, _ = unit_step(u, self.rings[i], self.hidden[i], dst, self.pos, self.end, n, rate, delay, dst_ring=not last,
                                   tail=self.tail, **self.mask)
                continue
            c_out = u.ops[-1].c_out
            dst = torch.zeros(self.batch, c_out, n * u.ops[0].rates(rate, delay)[0], dtype=torch.float64) if last else self.rings[i + 1]
            if len(u.ops) == 2:
                out, _ = res_unit_step(u.ops[0], u.ops[1], self.rings[i], dst, self.pos, self.end, n, rate, delay, dst_ring=not last,
                                       **self.mask)
            else:
                out, _ = step(u.ops[0], self.rings[i], dst, self.pos, self.end, n, rate, delay, dst_ring=not last, **self.mask)
        self.pos = [p + n for p in self.pos]
        return out
