"""The causal ops of ``csrc/conformer.hip`` on the device: against the float64 restatement of ``tests/causal_conformer_ref.py``
under its derived bounds (a check allows 2 x the bound, the criterion of ``tests/test_gpu_conformer.py``; nothing here is
measured), and the streaming contract -- chunked calls are bit for bit the single call, a non-finite value leaves the stream
K - 1 frames after it entered, a reset row starts over while the others go on.

Shapes (B, C, T, K): (2, 5, 37, 17) misaligned rows; (1, 3, 1025, 4) one position more than the time tile; (3, 130, 3, 31)
T < K - 1: the history reaches every output; K = 1 (no history at all), K = 2 (one float) and K = 64 (the largest).  Each with
and without a random history.  An op's inputs are exact: a history is given, not produced.
The chunk schedules run at 1, 7 and 390 rows, where the step kernel gives every row a workgroup of its own, and (``PACKED``) at more
than 1024 rows, where it packs several rows into one and the last workgroup is partly empty.
"""
import pytest
import torch

from audio_generation_amd import ops
from audio_generation_amd.transformers import ConformerBlock
from tests import causal_conformer_ref as cref
from tests import conformer_ref as ref
from tests.test_gpu_conformer import _dev, _inputs, _off, _within

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
MAX_STEP = ops.CONFORMER_MAX_STEP
CASES = [(2, 5, 37, 17), (1, 3, ref.TILE + 1, 4), (3, 130, 3, 31), (2, 5, 37, 1), (2, 5, 37, 2), (2, 5, 37, 64)]


def _hist(case, seed=0):
    b, c, _, k = case
    return torch.randn(b, c, k - 1, generator=torch.Generator().manual_seed(seed + sum(case)))


def _bn(d):
    return d["gamma"], d["beta"], d["r_mean"], d["r_var"]


@pytest.mark.parametrize("with_hist", [False, True], ids=["start", "hist"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_ops_against_the_restatement(case, with_hist):
    b, c, t, k = case
    cpu = _inputs(case)
    d = _dev(cpu)
    u64, w64, bias64, gamma64, beta64, rm64, rv64, dy64 = ref.f64(*(cpu[x] for x in ("u", "w", "bias", "gamma", "beta", "r_mean", "r_var", "dy")))
    hist = _hist(case) if with_hist else None
    hist_d, hist64 = (hist.to(DEV), hist.double()) if with_hist else (None, None)

    # forward: z, and the eval-mode fused form
    z = ops.glu_dwconv_causal(d["u"], d["w"], d["bias"], hist=hist_d)
    z64, bz = cref.glu_dwconv(u64, w64, bias64, hist64), cref.bound_z(u64, w64, bias64, hist64)
    _within(z, z64, bz, "z")
    y = ops.glu_dwconv_causal(d["u"], d["w"], d["bias"], bn=_bn(d), eps=EPS, hist=hist_d)
    p = ref.bn_parts(z64, gamma64, beta64, rm64, rv64, EPS)
    _within(y, ref.silu(p["a"]), ref.bound_y(z64, gamma64, beta64, rm64, rv64, EPS, training=False)
            + 1.1 * p["scale"].abs().reshape(1, -1, 1) * bz, "y (eval, fused)")
    assert torch.equal(ops.bn_silu(z, *_bn(d), eps=EPS, training=False), y), "the fused launch and bn_silu(training=False) of z differ"
    if with_hist:
        assert torch.equal(hist_d.cpu(), hist), "the forward wrote its history"
    else:       # no history is a history of zeros
        zeros = torch.zeros(b, c, k - 1, device=DEV)
        assert torch.equal(ops.glu_dwconv_causal(d["u"], d["w"], d["bias"], hist=zeros), z)
    assert torch.equal(ops.glu_dwconv_causal(_off(d["u"]), _off(d["w"]), d["bias"], hist=hist_d), z), "operands off a 16-byte boundary change bits"

    # the step on the same operands: the same bits, and the history moves on
    if t <= MAX_STEP:
        state = hist_d.clone() if with_hist else torch.zeros(b, c, k - 1, device=DEV)
        assert torch.equal(ops.glu_dwconv_step(d["u"], d["w"], d["bias"], _bn(d), state, eps=EPS), y)
        want = cref.next_hist(u64, k, hist64)               # what came from the old history is copied: exact
        d_g = torch.cat([torch.zeros(b, c, k - 1, dtype=torch.float64), ref.d_gate(u64[:, :c], ref.glu(u64))], dim=-1)[..., t:]
        _within(state, want, d_g, "hist after the step")

    # backward (no history: there is no backward through a cached call)
    if not with_hist:
        du, dw, dbias = ops.glu_dwconv_causal_backward(d["dy"], d["u"], d["w"])
        assert dw.shape == d["w"].shape
        want = cref.glu_dwconv_backward(dy64, u64, w64)
        bound = cref.bound_conv_backward(dy64, u64, w64)
        _within(du, want[0], bound[0], "du")
        _within(dw.reshape(c, k), want[1], bound[1], "dw")
        _within(dbias, want[2], bound[2], "dbias")
        again = ops.glu_dwconv_causal_backward(d["dy"], d["u"], d["w"])
        assert all(torch.equal(a, g) for a, g in zip(again, (du, dw, dbias))), "two calls differ"
        du_only, n1, n2 = ops.glu_dwconv_causal_backward(d["dy"], d["u"], d["w"], want_params=False)
        n3, dw_only, dbias_only = ops.glu_dwconv_causal_backward(d["dy"], d["u"], d["w"], want_du=False)
        assert n1 is None and n2 is None and n3 is None
        assert torch.equal(du_only, du) and torch.equal(dw_only, dw) and torch.equal(dbias_only, dbias)
        off = ops.glu_dwconv_causal_backward(_off(d["dy"]), _off(d["u"]), _off(d["w"]))
        assert all(torch.equal(a, g) for a, g in zip(off, (du, dw, dbias))), "operands off a 16-byte boundary change bits"


# ------------------------------------------------------------------------------------------------- chunked = whole
def _feed(u, w, bias, bn, state, chunks):
    """The chunks of u through the state: the step up to MAX_STEP frames, the forward + glu_hist_update beyond."""
    outs, at = [], 0
    for n in chunks:
        uc = u[..., at:at + n].contiguous()
        if n <= MAX_STEP:
            outs.append(ops.glu_dwconv_step(uc, w, bias, bn, state, eps=EPS))
        else:
            outs.append(ops.glu_dwconv_causal(uc, w, bias, bn=bn, eps=EPS, hist=state))
            assert ops.glu_hist_update(uc, state) is state
        at += n
    assert at == u.shape[-1]
    return torch.cat(outs, dim=-1)


def _g(u):
    """The post-GLU values as the kernels compute them: the K = 1 conv with tap 1 and bias 0 is fma(1, g, 0)."""
    c = u.shape[1] // 2
    return ops.glu_dwconv_causal(u, torch.ones(c, 1, 1, device=DEV), torch.zeros(c, device=DEV))


def _schedules(k):
    return {"ones": [1] * (k + 3), "mixed": [3, max(k - 1, 1), k, 1, 40], "short": [max(1, (k - 1) // 3)] * 4 + [1, max(1, (k - 1) // 2)],
            "max_step": [MAX_STEP, 3], "beyond_a_step": [MAX_STEP + 1, 2, MAX_STEP + 1], "across_a_tile": [1000, 20, 3, 1, 1, 5]}


# every schedule at K = 17; K = 2 and K = 64 on the two schedules that move old history
RUNS = [(17, s) for s in ("ones", "mixed", "short", "max_step", "beyond_a_step", "across_a_tile")] + [(k, s) for k in (2, 64) for s in ("mixed", "short")]


@pytest.mark.parametrize("b,c", [(1, 1), (1, 7), (3, 130)], ids=["1row", "7rows", "390rows"])
@pytest.mark.parametrize("k,schedule", RUNS, ids=lambda v: str(v))
def test_chunked_is_the_whole_call_bit_for_bit(k, schedule, b, c):
    chunks = _schedules(k)[schedule]
    t = sum(chunks)
    d = _dev(_inputs((b, c, t, k), seed=len(schedule)))
    bn = _bn(d)
    whole = ops.glu_dwconv_causal(d["u"], d["w"], d["bias"], bn=bn, eps=EPS)
    state = torch.zeros(b, c, k - 1, device=DEV)
    got = _feed(d["u"], d["w"], d["bias"], bn, state, chunks)
    assert torch.equal(got, whole), f"chunks {chunks} differ from the single call"
    g = _g(d["u"])
    want = torch.cat([torch.zeros(b, c, k - 1, device=DEV), g], dim=-1)[..., t:]
    assert torch.equal(state, want), "the final history is not the last K - 1 values of g"


# More than one row per workgroup.  The step kernel gives a workgroup R = min(256 / n, LDS, ceil(B C / 1024)) whole rows, so R > 1
# needs more than 1024 rows; B C is no multiple of R, so the last workgroup is partly empty.  (B, C, K) -> R at n = 1 / 4 / 64:
#   (5, 521, 17)     2605 rows    3 / 3 / 3       the grid term binds, 2605 = 868 * 3 + 1
#   (3, 6667, 17)   20001 rows   20 / 20 / 4      the grid term, then the 256 threads
#   (7, 14287, 64) 100009 rows   94 / 64 / 4      K = 64: the LDS term binds at n = 1 (12288 / 130), the threads at n = 4 and 64
PACKED = [(5, 521, 17, [1, 4, 64, 3, 1]), (3, 6667, 17, [1, 4, 1, 64, 2]), (7, 14287, 64, [1, 4, 64, 1])]


@pytest.mark.parametrize("b,c,k,chunks", PACKED, ids=lambda v: str(v))
def test_packed_rows_are_the_whole_call_bit_for_bit(b, c, k, chunks):
    t = sum(chunks)
    gen = torch.Generator().manual_seed(b + c + k)
    u = (2.0 * torch.randn(b, 2 * c, t, generator=gen)).to(DEV)
    w, bias = (torch.randn(c, 1, k, generator=gen) / k ** 0.5).to(DEV), torch.randn(c, generator=gen).to(DEV)
    bn = tuple(v.to(DEV) for v in (1.0 + 0.3 * torch.randn(c, generator=gen), 0.3 * torch.randn(c, generator=gen),
                                   0.2 * torch.randn(c, generator=gen), 0.5 + torch.rand(c, generator=gen)))
    whole = ops.glu_dwconv_causal(u, w, bias, bn=bn, eps=EPS)
    state = torch.zeros(b, c, k - 1, device=DEV)
    got = _feed(u, w, bias, bn, state, chunks)
    assert torch.equal(got, whole), f"chunks {chunks} differ from the single call"
    want = torch.cat([torch.zeros(b, c, k - 1, device=DEV), _g(u)], dim=-1)[..., t:]
    assert torch.equal(state, want), "the final history is not the last K - 1 values of g"
    # and from a history that is not zeros: every row's own, so a row read at another row's offset shows
    hist = torch.randn(b, c, k - 1, generator=gen).to(DEV)
    for n in (1, 4, MAX_STEP):
        state, uc = hist.clone(), u[..., :n].contiguous()
        assert torch.equal(ops.glu_dwconv_step(uc, w, bias, bn, state, eps=EPS), ops.glu_dwconv_causal(uc, w, bias, bn=bn, eps=EPS, hist=hist)), n
        assert torch.equal(state, torch.cat([hist, _g(uc)], dim=-1)[..., n:]), n


def test_a_non_finite_value_leaves_the_stream_after_k_minus_1_frames():
    case = (2, 5, 60, 17)
    b, c, t, k = case
    t0 = 10
    clean = _dev(_inputs(case))
    chunks = [4, 7, 1, 9, 3, 16, 20]          # the NaN enters in the second chunk and is carried across four boundaries
    bn = _bn(clean)
    s_clean = torch.zeros(b, c, k - 1, device=DEV)
    want = _feed(clean["u"], clean["w"], clean["bias"], bn, s_clean, chunks)
    others = [ch for ch in range(c) if ch != 2]
    for half in (0, 1):
        u = clean["u"].clone()
        u[1, half * c + 2, t0] = float("nan")
        state = torch.zeros(b, c, k - 1, device=DEV)
        got = _feed(u, clean["w"], clean["bias"], bn, state, chunks)
        assert torch.equal(got[:, others], want[:, others]) and torch.equal(got[0], want[0]), "the NaN left its channel"
        assert not torch.isfinite(got[1, 2, t0:t0 + k]).any(), "the NaN must show in the K outputs that see it"
        assert torch.equal(got[1, 2, :t0], want[1, 2, :t0]) and torch.equal(got[1, 2, t0 + k:], want[1, 2, t0 + k:])
        assert torch.equal(state, s_clean), "the NaN is still in the history K - 1 frames after it entered"
        whole = ops.glu_dwconv_causal(u, clean["w"], clean["bias"], bn=bn, eps=EPS)        # NaN != NaN: compare where both are finite
        assert torch.equal(torch.isfinite(whole), torch.isfinite(got)) and torch.equal(whole.nan_to_num(0.0, 0.0, 0.0), got.nan_to_num(0.0, 0.0, 0.0))


@pytest.mark.parametrize("case", [(3, 5, 37, 17), (1, 5, ref.TILE + 8, 4)], ids=lambda c: "x".join(map(str, c)))
def test_zero_taps_give_the_bias_exactly(case):
    b, c, t, k = case
    d = _dev(_inputs(case))
    d["w"][1] = 0.0
    hist = _hist(case).to(DEV)
    z = ops.glu_dwconv_causal(d["u"], d["w"], d["bias"], hist=hist)
    assert torch.equal(z[:, 1], d["bias"][1].expand(b, t))
    du, dw, dbias = ops.glu_dwconv_causal_backward(d["dy"], d["u"], d["w"])
    assert not du[:, 1].any() and not du[:, c + 1].any(), "zero taps pass no gradient to u"
    n = min(t, MAX_STEP)
    y = ops.glu_dwconv_step(d["u"][..., :n].contiguous(), d["w"], d["bias"], _bn(d), hist.clone(), eps=EPS)
    flat = ops.bn_silu(d["bias"].reshape(1, c, 1).expand(b, c, n).contiguous(), *_bn(d), eps=EPS, training=False)
    assert torch.equal(y[:, 1], flat[:, 1])


def test_a_reset_row_starts_over_while_the_others_go_on():
    torch.manual_seed(5)
    block = ConformerBlock(64, heads=2, dropout=0.0, kernel_size=17, context_x=48, causal=True, window=16).to(DEV).eval()
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(3, 64, 40, generator=gen).to(DEV)
    chunks = [1, 5, 1, 13]          # 20 frames, then again after the reset
    with torch.no_grad():
        cache = block.new_stream_cache(3)
        first, at = [], 0
        for n in chunks:
            first.append(block.run_bct(x[..., at:at + n].contiguous(), cache=cache))
            at += n
        cache.reset(rows=[1])
        assert cache.positions() == [20, 0, 20] and not cache.conv_state[1].any() and bool(cache.conv_state[[0, 2]].any())
        feed = x[..., 20:].clone()
        feed[1] = x[1, :, :20]      # row 1 hears its first 20 frames again
        second, at = [], 0
        for n in chunks:
            second.append(block.run_bct(feed[..., at:at + n].contiguous(), cache=cache))
            at += n
        first, second = torch.cat(first, -1), torch.cat(second, -1)
        assert torch.equal(second[1], first[1]), "a reset row must repeat its start-of-stream outputs"
        ref_cache = block.new_stream_cache(3)
        at, straight = 0, []
        for n in chunks + chunks:
            straight.append(block.run_bct(x[..., at:at + n].contiguous(), cache=ref_cache))
            at += n
        straight = torch.cat(straight, -1)
        assert torch.equal(second[[0, 2]], straight[[0, 2], :, 20:]), "the other rows must go on"
        assert cache.positions() == [40, 20, 40]


def test_bad_operands_raise_before_a_launch():
    d = _dev(_inputs((1, 2, 8, 3)))
    state = torch.zeros(1, 2, 2, device=DEV)
    with pytest.raises(ops.AgxError):
        ops.glu_dwconv_step(torch.zeros(1, 4, MAX_STEP + 1, device=DEV), d["w"], d["bias"], _bn(d), state)
    with pytest.raises(ops.AgxError):
        ops.glu_dwconv_step(d["u"], d["w"], d["bias"], _bn(d), None)
    with pytest.raises(ops.AgxError):
        ops.glu_dwconv_step(d["u"], d["w"], d["bias"], _bn(d), torch.zeros(1, 2, 3, device=DEV))
    with pytest.raises(ops.AgxError):
        ops.glu_dwconv_causal(d["u"], d["w"], d["bias"], hist=torch.zeros(2, 2, 2, device=DEV))
    with pytest.raises(ops.AgxError):
        ops.glu_hist_update(d["u"], torch.zeros(1, 3, 2, device=DEV))
    assert not state.any()
