"""``ops.multires_stream_step`` and ``ops.conv_stream_step_affine`` on the GPU, by the criteria of
tests/test_gpu_conv_stream.py: every step against its reference, the schedules bit for bit, a row of a batch against the row alone,
the ring phase, NaN containment and the counted forms.

Rings have the tight capacity ``reach + max_chunk * rate`` (never a power of two here), so the ring phase moves with every step.
A case with ``lag = 1`` sits behind a producer that lags one frame: its input enters the ring at negative indices, its own output
crosses the start mask, and it is flushed past its end.

Multires steps are compared with the whole-signal calls -- ``oracle.wavelets.multires_conv`` and the package's plain
``ops.multires_forward`` -- at the tolerance the suite holds that kernel to on ``randn`` input (1e-5 max abs,
tests/test_gpu_blocks.py) -- and, beside that flat tolerance, both the step and the plain call are within 2 x the derived bound
of the float64 restatement of the whole signal (tests/wavelet_ref.py).  Depthwise steps are within 2 x the derived bound of the
float64 restatement (tests/multires_stream_ref.py) on their own operands: the reference reads a float64 copy of the ring the kernel read.
"""
import pytest
import torch

from audio_generation_amd import ops
from audio_generation_amd._lib import CONV_CAUSAL, EPI_LEAKY_POST, EPI_LEAKY_PRE, EPI_RESIDUAL, AgxError
from oracle import wavelets as owv
from tests import codec_stream_ref as cref
from tests import multires_stream_ref as ref
from tests import wavelet_ref
from tests.test_gpu_conformer import _within
from tests.test_gpu_conv_stream import MAX_CHUNK, SCHEDULES, T, _block

pytestmark = pytest.mark.gpu
DEV = "cuda"
MULTIRES_TOL = 1e-5


class Multires:
    """A multires layer with seeded parameters at ``rate`` columns per frame behind a producer lagging ``lag`` frames."""
    kind = "multires"

    def __init__(self, c, k, depth, rate, lag=0):
        g = torch.Generator().manual_seed(7 * c + 11 * k + 13 * depth)
        self.c, self.k, self.depth, self.rate, self.lag = c, k, depth, rate, lag
        self.c_out, self.reach, self.delay = c, ref.reach(k, depth), lag * rate
        scalar = 2.0 ** 0.5 / (2 * k)
        self.h0 = (torch.rand(c, 1, k, generator=g) * 2 - 1) * scalar
        self.h1 = (torch.rand(c, 1, k, generator=g) * 2 - 1) * scalar
        self.w = (torch.rand(c, depth + 2, generator=g) * 2 - 1) * (2.0 / (2 * depth + 4)) ** 0.5
        self.dev = [t.to(DEV) for t in (self.h0, self.h1, self.w)]

    def launch(self, src, dst, pos, end, n, dst_ring=True, counts=None):
        return ops.multires_stream_step(*self.dev, self.depth, src, dst, pos, n, self.rate, self.delay, dst_ring=dst_ring, end=end,
                                        counts=counts)

    def whole(self, x):
        """The references of the whole signal: the oracle, the package's plain call, and the float64 restatement with its bound --
        which the plain call is held to here, once."""
        want = owv.multires_conv(x, self.h0, self.h1, self.w, self.depth)
        plain = ops.multires_forward(x.to(DEV), *self.dev, self.depth).cpu()
        exact, _, bound = wavelet_ref.multires(x, self.h0, self.h1, self.w, self.depth)
        _within(plain, exact, bound, f"plain multires call C={self.c} K={self.k} depth={self.depth}")
        return want, plain, exact, bound


class Depthwise:
    """A depthwise residual unit: the affine (scale, shift of magnitude 0.5 .. 1), the dilated conv, the k = 1 conv."""
    kind = "resdw"

    def __init__(self, c, k, d, rate, lag=0):
        g = torch.Generator().manual_seed(5 * c + 3 * k + d)
        self.c, self.k, self.d, self.rate, self.lag = c, k, d, rate, lag
        self.c_out, self.reach, self.delay = c, d * (k - 1), lag * rate
        sign = torch.where(torch.randn(c, generator=g) > 0, 1.0, -1.0)
        self.scale = 1.0 + 0.5 * torch.randn(c, generator=g)
        self.shift = sign * (0.5 + 0.5 * torch.rand(c, generator=g))
        w1, b1 = torch.randn(c, c, k, generator=g) / (c * k) ** 0.5, torch.randn(c, generator=g)
        w2, b2 = torch.randn(c, c, 1, generator=g) / c ** 0.5, torch.randn(c, generator=g)
        self.op1 = cref.Op("causal", w1, b1, d=d, pre=cref.SLOPE)
        self.op2 = cref.Op("causal", w2, b2, residual=True, post=cref.SLOPE)
        self.img1 = ops.conv_stream_pack(ops.conv_desc(CONV_CAUSAL, 1, c, c, 1 << 20, k, 1, d), w1.to(DEV))
        self.img2 = ops.conv_stream_pack(ops.conv_desc(CONV_CAUSAL, 1, c, c, 1 << 20, 1, 1, 1), w2.to(DEV))
        self.b1, self.b2, self.sc, self.sh = b1.to(DEV), b2.to(DEV), self.scale.to(DEV), self.shift.to(DEV)

    def launch(self, src, dst, pos, end, n, dst_ring=True, counts=None, hid=None):
        hid = torch.empty(src.shape[0], self.c, n * self.rate, device=DEV) if hid is None else hid
        ops.conv_stream_step_affine(self.c, self.c, self.k, self.d, self.img1, self.b1, self.sc, self.sh, src, hid, pos, n, self.rate,
                                    self.delay, dst_ring=False, epilogue=EPI_LEAKY_PRE, slope=cref.SLOPE, counts=counts)
        self.hid = hid
        return ops.conv_stream_step(CONV_CAUSAL, self.c, self.c, 1, 1, 1, self.img2, self.b2, hid, dst, pos, n, self.rate, self.delay,
                                    src_ring=False, dst_ring=dst_ring, res=src, end=end, epilogue=EPI_RESIDUAL | EPI_LEAKY_POST,
                                    slope=cref.SLOPE, counts=counts)


CASES = {
    "mr6": lambda: Multires(6, 2, 3, 1),                # the reach of 7 is longer than a one-column step
    "mr20lag": lambda: Multires(20, 3, 4, 6, lag=1),    # negative ring indices, the start mask, a reach of 30 over several frames
    "mr33wide": lambda: Multires(33, 4, 1, 40),         # a wide step; 33 channels fill no packing evenly
    "mr3tiles": lambda: Multires(3, 2, 2, 190),         # max_chunk * rate = 1140: one full tile of 1024 columns and a ragged one
    "dw33": lambda: Depthwise(33, 7, 1, 2),             # three channel groups, the last holding one channel
    "dw16": lambda: Depthwise(16, 7, 9, 1),             # reach 54
    "dw8lag": lambda: Depthwise(8, 3, 3, 3, lag=1),     # crosses the start mask
}
_BUILT = {}


def _case(name):
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


def _signal(k, batch, frames=T, seed=5):
    return torch.randn(batch, k.c, frames * k.rate, generator=torch.Generator().manual_seed(seed))


def _feed(k, x, flush_frames=0):
    """The columns as they enter the case's ring, frame by frame: behind a producer that lags, ``delay`` exact zeros (what the
    producer stores at negative indices), the signal, and zeros again past its end."""
    b, c, _ = x.shape
    return torch.cat([torch.zeros(b, c, k.delay), x, torch.zeros(b, c, flush_frames * k.rate)], dim=2)


_WHOLE = {}


def _whole(name, batch):
    """The whole-signal references of a multires case, computed once and never modified."""
    if (name, batch) not in _WHOLE:
        _WHOLE[name, batch] = _case(name).whole(_signal(_case(name), batch))
    return _WHOLE[name, batch]


def run_case(name, batch, feed, schedule, flush=(), check=True, start=None):
    """Stream ``feed`` (``_feed``: B, C, at least frames * rate columns) through the case on tight rings; returns (outputs of all steps, final destination ring,
    final source ring, final positions).  ``flush``: further chunks, after ``stream_mark_end``.  ``start = (src ring, pos)``:
    go on from that state instead of an empty stream at 0."""
    k = _case(name)
    masked = k.lag > 0
    cap, cap_out = k.reach + MAX_CHUNK * k.rate, MAX_CHUNK * k.rate + 3
    assert cap & (cap - 1) and cap_out & (cap_out - 1), "a power-of-two ring would hide a wrong modulus"
    src = torch.zeros(batch, k.c, cap, device=DEV) if start is None else start[0].clone()
    host_pos = [0] * batch if start is None else list(start[1])
    dst = torch.zeros(batch, k.c, cap_out, device=DEV)
    pos = torch.tensor(host_pos, dtype=torch.int64, device=DEV)
    end = torch.full((batch,), ops.STREAM_LIVE, dtype=torch.int64, device=DEV) if masked else None
    host_end = [cref.LIVE] * batch
    refs = _whole(name, batch) if check and k.kind == "multires" else None
    outs, at = [], 0
    for step_no, (n, flushing) in enumerate([(n, False) for n in schedule] + [(n, True) for n in flush]):
        if flushing and host_end[0] == cref.LIVE:
            ops.stream_mark_end(pos, end)
            host_end = list(host_pos)
        chunk = feed[:, :, at * k.rate:(at + n) * k.rate]
        assert chunk.shape[2] == n * k.rate
        at += n
        ops.ring_write_rate(src, chunk.contiguous().to(DEV), pos - k.lag, k.rate)          # columns pos r - delay ...
        src64, before = src.cpu().double(), dst.clone()
        k.launch(src, dst, pos, end, n)
        got = _block(dst, host_pos, n * k.rate, k.rate, k.delay)
        outs.append(got)
        if check:
            what = f"{name} B={batch} step {step_no} n={n}"
            e = host_end if masked else None
            if k.kind == "multires":
                for r, p in enumerate(host_pos):
                    j = torch.arange(p * k.rate - k.delay, (p + n) * k.rate - k.delay)
                    live = (j >= 0) & (j < (host_end[r] if masked and host_end[r] != cref.LIVE else 1 << 40) * k.rate)
                    assert not bool(live.any()) or int(j[live].max()) < refs[0].shape[2]
                    for label, whole in zip(("oracle", "plain call"), refs[:2]):
                        err = float((got[r].cpu()[:, live] - whole[r][:, j[live]]).abs().max()) if bool(live.any()) else 0.0
                        print(f"{what} row {r} vs the {label}: max abs {err:.3e}")
                        assert err < MULTIRES_TOL, (what, label, err)
                    if bool(live.any()):
                        _within(got[r][:, live], refs[2][r][:, j[live]], refs[3][r][:, j[live]], f"{what} row {r} vs the restatement")
                    assert bool((got[r].cpu()[:, ~live] == 0).all()), what                # masked columns are exact zeros
            else:
                scratch = torch.zeros(batch, k.c, cap_out, dtype=torch.float64)
                hid64 = torch.zeros(batch, k.c, n * k.rate, dtype=torch.float64)
                want_h, bound_h = ref.affine_step(k.op1, k.scale, k.shift, src64, hid64, host_pos, n, k.rate, k.delay)
                _within(k.hid, want_h, bound_h, what + " affine conv")
                want, bound = ref.resdw_unit_step(k.op1, k.op2, k.scale, k.shift, src64, scratch, host_pos, e, n, k.rate, k.delay)
                _within(got, want, bound, what)
                if masked:
                    assert bool((got.cpu()[want == 0] == 0).all())
            touched = torch.zeros(batch, cap_out, dtype=torch.bool)
            for r, p in enumerate(host_pos):
                touched[r, torch.remainder(torch.arange(p * k.rate - k.delay, (p + n) * k.rate - k.delay), cap_out)] = True
            keep = ~touched[:, None, :].expand(-1, k.c, -1)
            assert torch.equal(dst.cpu()[keep], before.cpu()[keep]), "a column outside the step's block was written"
        ops.stream_advance(pos, n)
        host_pos = [p + n for p in host_pos]
    assert pos.tolist() == host_pos
    return torch.cat(outs, dim=2), dst, src, host_pos


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_step_against_its_references_and_schedule_invariance(name, batch):
    k = _case(name)
    x = _signal(k, batch)
    flush = (1, 2) if k.lag else ()
    results = [run_case(name, batch, _feed(k, x, sum(flush)), sched, flush=flush) for sched in SCHEDULES]
    out0, ring0 = results[0][:2]
    for sched, (out, ring, _, _) in zip(SCHEDULES[1:], results[1:]):
        assert torch.equal(out, out0), (name, sched)
        assert torch.equal(ring, ring0), (name, sched)
    if k.lag:
        assert float(out0[:, :, :k.delay].abs().max()) == 0.0                          # before the start
        assert float(out0[:, :, k.delay + T * k.rate:].abs().max()) == 0.0             # after the end
        assert float(out0[:, :, k.delay:k.delay + T * k.rate].abs().max()) > 0.0


@pytest.mark.parametrize("name", list(CASES))
def test_a_row_of_a_batch_equals_the_row_alone(name):
    x = _feed(_case(name), _signal(_case(name), 3))
    together = run_case(name, 3, x, [2, 1, 3], check=False)[0]
    alone = run_case(name, 1, x[1:2].contiguous(), [2, 1, 3], check=False)[0]
    assert torch.equal(together[1:2], alone)


def _rotated(k, src, host_pos, shift):
    """The ring of a stream that is ``shift`` frames further along and holds the same history: stream column i sits at
    (i + shift rate) mod cap."""
    cap = src.shape[2]
    out = torch.zeros_like(src)
    for r, p in enumerate(host_pos):
        i = torch.arange(p * k.rate - k.delay - k.reach, p * k.rate - k.delay)
        out[r][:, torch.remainder(i + shift * k.rate, cap).to(DEV)] = src[r][:, torch.remainder(i, cap).to(DEV)]
    return out


@pytest.mark.parametrize("name", ["mr6", "mr20lag", "mr33wide", "dw33", "dw16", "dw8lag"])
def test_the_starting_ring_phase_changes_no_bit(name):
    """The same history and the same chunks at pos and at pos + 2^33, the ring pre-rotated to the new phase.  The history is 60
    frames long, so every column the depthwise operand reads has a stream index >= 0 in both runs."""
    k = _case(name)
    head, tail = [2, 1, 3] * 10, [2, 1, 3]
    x = _feed(k, _signal(k, 2, frames=sum(head) + sum(tail), seed=11))
    assert sum(head) * k.rate - k.delay - k.reach >= 0
    _, _, src, host_pos = run_case(name, 2, x, head, check=False)
    rest = x[:, :, sum(head) * k.rate:].contiguous()
    a = run_case(name, 2, rest, tail, check=False, start=(src, host_pos))[0]
    for shift in (7, 1 << 33):
        b = run_case(name, 2, rest, tail, check=False, start=(_rotated(k, src, host_pos, shift), [p + shift for p in host_pos]))[0]
        assert torch.equal(a, b), (name, shift)
    whole = run_case(name, 2, x, head + tail, check=False)[0]
    assert torch.equal(whole[:, :, sum(head) * k.rate:], a)


@pytest.mark.parametrize("name", ["mr6", "mr20lag", "dw33", "dw16"])
def test_a_nan_leaves_the_outputs_after_the_reach(name):
    """60 frames in chunks of 2, 1, 3: the ring wraps many times after the NaN went in, and it never comes back."""
    k = _case(name)
    schedule = [2, 1, 3] * 10
    x = _signal(k, 1, frames=sum(schedule), seed=9)
    at = 4
    x[0, 1, at] = float("nan")
    out = run_case(name, 1, _feed(k, x), schedule, check=False)[0]
    bad = torch.isnan(out).any(dim=1)[0].nonzero().flatten()
    assert bad.numel() > 0 and int(bad.min()) == at + k.delay and int(bad.max()) == at + k.delay + k.reach, (bad.min(), bad.max(), k.reach)
    clean = run_case(name, 1, _feed(k, torch.nan_to_num(x, nan=0.25)), schedule, check=False)[0]
    assert torch.equal(out[:, :, at + k.delay + k.reach + 1:], clean[:, :, at + k.delay + k.reach + 1:])


@pytest.mark.parametrize("name", list(CASES))
def test_counted_steps_take_the_first_frames_and_leave_a_paused_row_alone(name):
    """counts = [0, n, 1] after three warm-up frames: row 0 changes nowhere, the taken part is the uncounted step bit for bit, a
    plain destination holds exact 0 behind the count -- and the chunk behind a row's count is NaN."""
    k = _case(name)
    n = 3
    x = _signal(k, 3, frames=3 + n, seed=13)
    _, _, src0, host_pos = run_case(name, 3, _feed(k, x[:, :, :3 * k.rate]), [2, 1], check=False)
    chunk = x[:, :, 3 * k.rate:].contiguous().to(DEV)
    cap_out = MAX_CHUNK * k.rate + 3
    end = torch.full((3,), ops.STREAM_LIVE, dtype=torch.int64, device=DEV) if k.lag else None

    def state():
        return (src0.clone(), torch.full((3, k.c, cap_out), 7.0, device=DEV), torch.tensor(host_pos, dtype=torch.int64, device=DEV))

    src, dst, pos = state()
    ops.ring_write_rate(src, chunk, pos - k.lag, k.rate)
    k.launch(src, dst, pos, end, n)
    want = _block(dst, host_pos, n * k.rate, k.rate, k.delay)

    counts_host = [0, n, 1]
    counts = torch.tensor(counts_host, dtype=torch.int64, device=DEV)
    dirty = chunk.clone()
    for r, cnt in enumerate(counts_host):
        dirty[r, :, cnt * k.rate:] = float("nan")
    for dst_ring in (True, False):
        src, dst, pos = state()
        ops.ring_write_rate(src, dirty, pos - k.lag, k.rate, counts=counts)
        assert not bool(torch.isnan(src).any())
        if not dst_ring:
            dst = torch.full((3, k.c, n * k.rate), 7.0, device=DEV)
        before = dst.clone()
        out = k.launch(src, dst, pos, end, n, dst_ring=dst_ring, counts=counts)
        assert torch.equal(src[0], src0[0]) and pos.tolist() == host_pos
        got = _block(dst, host_pos, n * k.rate, k.rate, k.delay) if dst_ring else out
        assert torch.equal(got[1], want[1]) and torch.equal(got[2, :, :k.rate], want[2, :, :k.rate]), (name, dst_ring)
        if dst_ring:
            assert torch.equal(dst[0], before[0])                                          # the paused row: not one column written
            cols = torch.remainder(torch.arange((host_pos[2] + 1) * k.rate - k.delay, (host_pos[2] + n) * k.rate - k.delay), cap_out)
            assert float((dst[2][:, cols.to(DEV)] - 7.0).abs().max()) == 0.0                # not written behind the count
        else:
            assert float(out[0].abs().max()) == 0.0 and float(out[2, :, k.rate:].abs().max()) == 0.0
        ops.stream_advance(pos, n, counts=counts)
        assert pos.tolist() == [host_pos[0], host_pos[1] + n, host_pos[2] + 1]


def test_wrapper_refusals_precede_the_launch():
    k, d = _case("mr6"), _case("dw33")
    src, dst = torch.zeros(2, 6, 7 + 4, device=DEV), torch.full((2, 6, 9), 7.0, device=DEV)
    pos = torch.zeros(2, dtype=torch.int64, device=DEV)
    ok = dict(src=src, dst=dst, pos=pos, end=None, n=4)
    for kw in (dict(n=0), dict(n=5), dict(src=src[:, :5].contiguous()), dict(dst=dst[:1].contiguous()), dict(pos=pos[:1]),
               dict(pos=pos.int()), dict(end=pos.cpu()), dict(dst=src), dict(src=src.double()), dict(dst=dst[:, :, :3].contiguous()),
               dict(counts=pos.cpu()), dict(counts=pos[:1])):
        with pytest.raises(AgxError):
            k.launch(**{**ok, **kw})
    src2, hid = torch.zeros(2, 33, 6 + 8, device=DEV), torch.full((2, 33, 8), 7.0, device=DEV)
    base = dict(c_in=33, c_out=33, kernel=7, dilation=1, packed=d.img1, bias=d.b1, scale=d.sc, shift=d.sh, src=src2, dst=hid, pos=pos, n=4,
                rate_in=2, delay_in=0, dst_ring=False)
    for kw in (dict(stride=2), dict(src_ring=False), dict(scale=d.sc[:32].contiguous()), dict(shift=d.sh.cpu()), dict(n=5),
               dict(src=src2[:, :, :13].contiguous()), dict(dst=src2), dict(packed=d.img2)):
        with pytest.raises(AgxError):
            ops.conv_stream_step_affine(**{**base, **kw})
    torch.cuda.synchronize()
    assert float((dst - 7.0).abs().max()) == 0.0 and float((hid - 7.0).abs().max()) == 0.0 and pos.tolist() == [0, 0]
