"""Ragged batches on the GPU (csrc/attention_ragged.hip): ``ops.attention_alibi_ragged`` / ``_backward`` against the float64
checker of ``tests/ragged_attention_ref.py`` (the frozen definition on every cropped row), ``ops.mask_tail``, and the
``lengths=`` / ``y_lengths=`` surface of the modules.

Besides the value checks, three properties the feature exists for: what lies beyond a row's length may hold anything (NaN,
3.4e38 and 0 give bitwise the same finite results), a row of a ragged batch is bitwise the row cropped and run alone, and every
result is exactly 0 at padded positions.

Tolerances are the ones the suite states for the same arithmetic: 3e-5 of max(1, max|o|) for the fp32 flash forward, 5e-5 / 1e-5
(max / rms, times max(1, scale of the reference quantity)) for the split backward (tests/test_gpu_cross_attention.py), 1e-4 for
a depth-2 block against float64 and 2e-4 / 5e-4 for its input / parameter gradients (tests/test_gpu_cross_attention.py,
tests/test_gpu_training.py), 2e-5 for a block against itself on another batch layout (tests/test_gpu_blocks.py).  Every measured
error is printed."""
import pytest
import torch

from audio_generation_amd import ops
from audio_generation_amd._lib import AgxError
from audio_generation_amd.transformers import Transformer, TransformerBottleneck
from oracle import attention as oattn
from tests.helpers import max_abs, rms
from tests.ragged_attention_ref import CASE_IDS, CASES, case_inputs, pad_mask, ragged_core, ragged_transformer

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, HUGE = float("nan"), 3.4e38
_REF, _RUNS = {}, {}


def _ref(n):
    """Inputs and the float64 results of case ``n``, computed once."""
    if n not in _REF:
        _, b, heads, dh, tq, tk, q_len, k_len = CASES[n]
        q, kv, dout, slopes = case_inputs(b, heads, dh, tq, tk)
        q64, kv64 = q.double().requires_grad_(), kv.double().requires_grad_()
        out = ragged_core(q64, kv64, slopes, heads, dh, dh ** 0.5, q_len, k_len)
        out.backward(dout.double())
        _REF[n] = dict(q=q, kv=kv, dout=dout, slopes=slopes, out=out.detach(), dq=q64.grad, dkv=kv64.grad)
    return _REF[n]


def _lens(lengths):
    return torch.tensor(lengths, dtype=torch.int32, device=DEV)


def _call(kind, q, kv, dout, slopes, heads, dh, q_len=None, k_len=None, backward=True):
    """(out, dq, dkv) of one forward and one backward on device tensors; a "self" case goes through one qkv tensor."""
    args = (slopes, heads, dh, dh ** 0.5)
    if kind == "self":
        qkv = torch.cat([q, kv], dim=1)
        out = ops.attention_alibi_ragged(qkv, None, *args, q_len=q_len, k_len=k_len)
        if not backward:
            return out, None, None
        dqkv = ops.attention_alibi_ragged_backward(qkv, None, slopes, out, dout, heads, dh, dh ** 0.5, q_len=q_len, k_len=k_len)
        assert dqkv.shape == qkv.shape
        hd = heads * dh
        return out, dqkv[:, :hd], dqkv[:, hd:]
    out = ops.attention_alibi_ragged(q, kv, *args, q_len=q_len, k_len=k_len)
    if not backward:
        return out, None, None
    dq, dkv = ops.attention_alibi_ragged_backward(q, kv, slopes, out, dout, heads, dh, dh ** 0.5, q_len=q_len, k_len=k_len)
    return out, dq, dkv


def _run(n, fill=None):
    """Case ``n`` with the padding of q, kv and dout set to ``fill`` (None: as generated), once per fill."""
    if (n, fill) not in _RUNS:
        kind, b, heads, dh, tq, tk, q_len, k_len = CASES[n]
        c = _ref(n)
        q, kv, dout = c["q"].clone(), c["kv"].clone(), c["dout"].clone()
        if fill is not None:
            q.masked_fill_(pad_mask(q_len, tq), fill)
            dout.masked_fill_(pad_mask(q_len, tq), fill)
            kv.masked_fill_(pad_mask(k_len, tk), fill)
        _RUNS[n, fill] = _call(kind, q.to(DEV), kv.to(DEV), dout.to(DEV), c["slopes"].to(DEV), heads, dh, _lens(q_len), _lens(k_len))
    return _RUNS[n, fill]


@pytest.mark.parametrize("n", range(len(CASES)), ids=CASE_IDS)
def test_ragged_forward_against_the_definition(n):
    _, b, heads, dh, tq, tk, q_len, k_len = CASES[n]
    want = _ref(n)["out"]
    got = _run(n)[0]
    assert tuple(got.shape) == (b, heads * dh, tq)
    err, scale = max_abs(got.cpu(), want), float(want.abs().max())
    print(f"ragged forward {CASE_IDS[n]}: max err {err:.3e}, max|o| {scale:.3e}")
    assert err < 3e-5 * max(1.0, scale)
    pads = pad_mask(q_len, tq).expand_as(want).clone()
    for r in range(b):
        if k_len[r] == 0:
            pads[r] = True
    assert bool((got.cpu()[pads] == 0).all())                      # exactly 0, not merely small


@pytest.mark.parametrize("n", range(len(CASES)), ids=CASE_IDS)
def test_ragged_backward_against_float64_autograd(n):
    kind, b, heads, dh, tq, tk, q_len, k_len = CASES[n]
    c = _ref(n)
    _, dq, dkv = _run(n)
    assert dq.shape == c["q"].shape and dkv.shape == c["kv"].shape
    for name, got, want in (("dq", dq, c["dq"]), ("dkv", dkv, c["dkv"])):
        e_max, e_rms = max_abs(got.cpu(), want), rms(got.cpu(), want)
        s_max, s_rms = float(want.abs().max()), float(want.pow(2).mean().sqrt())
        print(f"ragged backward {CASE_IDS[n]} {name}: max err {e_max:.3e} (max {s_max:.3e}), rms err {e_rms:.3e} (rms {s_rms:.3e})")
        assert e_max < 5e-5 * max(1.0, s_max) and e_rms < 1e-5 * max(1.0, s_rms), name
    dead = torch.tensor([q_len[r] == 0 or k_len[r] == 0 for r in range(b)]).reshape(-1, 1, 1)
    assert bool((dq.cpu()[(pad_mask(q_len, tq) | dead).expand_as(dq)] == 0).all())
    assert bool((dkv.cpu()[(pad_mask(k_len, tk) | dead).expand_as(dkv)] == 0).all())
    q, kv, dout = (c[k].to(DEV) for k in ("q", "kv", "dout"))
    again = _call(kind, q, kv, dout, c["slopes"].to(DEV), heads, dh, _lens(q_len), _lens(k_len))
    for a, g in zip(again, _run(n)):
        assert torch.equal(a, g)                                    # deterministic: no atomics


@pytest.mark.parametrize("n", range(len(CASES)), ids=CASE_IDS)
def test_the_padding_may_hold_anything(n):
    base = _run(n)
    for fill in (NAN, HUGE, 0.0):
        for name, a, g in zip(("out", "dq", "dkv"), _run(n, fill), base):
            assert bool(torch.isfinite(a).all()), (fill, name)
            assert torch.equal(a, g), (fill, name)


@pytest.mark.parametrize("n", range(len(CASES)), ids=CASE_IDS)
def test_a_row_is_the_row_cropped_and_run_alone(n):
    kind, b, heads, dh, tq, tk, q_len, k_len = CASES[n]
    c = _ref(n)
    out, dq, dkv = _run(n)
    checked = 0
    for r in range(b):
        ql, kl = q_len[r], k_len[r]
        if ql == 0 or kl == 0:
            continue
        q, kv, dout = (c[k][r:r + 1, :, :ln].contiguous().to(DEV) for k, ln in (("q", ql), ("kv", kl), ("dout", ql)))
        o1, dq1, dkv1 = _call(kind, q, kv, dout, c["slopes"].to(DEV), heads, dh)        # batch 1, lengths NULL
        assert torch.equal(o1[0], out[r, :, :ql]) and torch.equal(dq1[0], dq[r, :, :ql]) and torch.equal(dkv1[0], dkv[r, :, :kl]), r
        checked += 1
    assert checked >= b - 1


@pytest.mark.parametrize("n", range(len(CASES)), ids=CASE_IDS)
def test_full_lengths_are_the_cross_attention_op(n):
    kind, b, heads, dh, tq, tk, _, _ = CASES[n]
    c = _ref(n)
    q, kv, slopes = c["q"].to(DEV), c["kv"].to(DEV), c["slopes"].to(DEV)
    want = ops.attention_alibi_cross(q, kv, slopes, heads, dh, dh ** 0.5)
    full = _call(kind, q, kv, None, slopes, heads, dh, _lens([tq] * b), _lens([tk] * b), backward=False)[0]
    null = _call(kind, q, kv, None, slopes, heads, dh, backward=False)[0]
    over = _call(kind, q, kv, None, slopes, heads, dh, _lens([tq + 1000] * b), _lens([2 ** 31 - 1] * b), backward=False)[0]   # clamped
    err = max_abs(full, want)
    print(f"ragged forward, full lengths, {CASE_IDS[n]}: {err:.3e} from attention_alibi_cross")
    assert err < 3e-5 * max(1.0, float(want.abs().max()))
    assert torch.equal(null, full) and torch.equal(over, full)


@pytest.mark.parametrize("shape,lengths", [((3, 5, 37), [37, 0, 20]), ((2, 3, 5), [5, 2]), ((4, 7, 3), [0, 1, 2, 3]), ((5, 2, 1), [1, 0, 1, 0, 1]),
                                           ((2, 64, 225), [225, 100]), ((2, 3, 6), [-4, 1000])])
def test_mask_tail_is_an_exact_select(shape, lengths):
    b, c, t = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=gen)
    clamped = [min(max(v, 0), t) for v in lengths]
    want = x.masked_fill(pad_mask(clamped, t), 0.0)
    x.masked_fill_(pad_mask(clamped, t), NAN)                      # a NaN tail: a multiply by 0 would keep it
    xd, ld = x.to(DEV), _lens(lengths)
    out = ops.mask_tail(xd, ld)
    assert torch.equal(out.cpu(), want)
    assert torch.equal(xd.cpu().nan_to_num(nan=7.0), x.nan_to_num(nan=7.0))           # out of place: x is untouched
    odd = torch.empty(x.numel() + 1, device=DEV)[1:].view(shape)   # 4 bytes off a 16-byte boundary: the scalar path
    odd.copy_(xd)
    assert ops.mask_tail(odd, ld, out=odd) is odd and torch.equal(odd.cpu(), want)     # in place
    assert ops.mask_tail(xd, ld, out=xd) is xd and torch.equal(xd.cpu(), want)
    assert torch.equal(ops.mask_tail(out, None).cpu(), want)       # no lengths: a copy


# ------------------------------------------------------------------------------------------------- modules
DIM, HEADS, DH, TX, TY = 64, 4, 16, 70, 110
LENGTHS, Y_LENGTHS = [70, 23, 1], [110, 40, 1]       # one full row, one short row, one row of length 1
_MOD = {}


def _module(cross):
    """(module on the device, float64 state dict with gradients, inputs, float64 output) of the self / cross block."""
    if cross not in _MOD:
        sd = oattn.init_state_dict(DIM, HEADS, DH, depth=2, seed=91)
        tf = Transformer(DIM, depth=2, heads=HEADS, head_dim=DH, context_x=80, **(dict(context_y=120) if cross else {}))
        tf.load_state_dict(sd)
        gen = torch.Generator().manual_seed(93)
        x, y, w = torch.randn(3, DIM, TX, generator=gen), torch.randn(3, DIM, TY, generator=gen), torch.randn(3, DIM, TX, generator=gen)
        sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
        x64, y64 = x.double().requires_grad_(), y.double().requires_grad_()
        want = ragged_transformer(x64.transpose(1, 2), y64.transpose(1, 2) if cross else None, sd64, HEADS, 2, LENGTHS,
                                  Y_LENGTHS if cross else None).transpose(1, 2)
        (want * w.double()).sum().backward()
        _MOD[cross] = dict(tf=tf.to(DEV), sd=sd, sd64=sd64, x=x, y=y if cross else None, w=w, x64=x64, y64=y64 if cross else None,
                           want=want.detach())
    return _MOD[cross]


def _padded(m, fill):
    """(x, y) on the device with their padding set to ``fill``."""
    x = m["x"].masked_fill(pad_mask(LENGTHS, TX), fill).to(DEV)
    y = None if m["y"] is None else m["y"].masked_fill(pad_mask(Y_LENGTHS, TY), fill).to(DEV)
    return x, y


@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
def test_modules_eval(cross):
    m = _module(cross)
    tf = m["tf"].eval()
    kw = dict(lengths=LENGTHS, **(dict(y_lengths=Y_LENGTHS) if cross else {}))
    x, y = m["x"].to(DEV), None if not cross else m["y"].to(DEV)
    with torch.no_grad():
        out = tf.run_bct(x, y, **kw)
        err = max_abs(out.cpu(), m["want"])
        print(f"ragged block ({'cross' if cross else 'self'}) eval: {err:.3e} from float64")
        assert err < 1e-4
        assert bool((out.cpu()[pad_mask(LENGTHS, TX).expand_as(out)] == 0).all())
        for r, n in enumerate(LENGTHS):                           # the same module on the cropped row, without lengths
            alone = tf.run_bct(x[r:r + 1, :, :n].contiguous(), None if not cross else y[r:r + 1, :, :Y_LENGTHS[r]].contiguous())
            e = max_abs(out[r:r + 1, :, :n], alone)
            print(f"ragged block ({'cross' if cross else 'self'}) eval, row {r} alone: {e:.3e}")
            assert e < 2e-5
        xn, yn = _padded(m, NAN)
        before = xn.clone()
        assert torch.equal(tf.run_bct(xn, yn, **kw), out)          # NaN padding: bitwise the same
        assert torch.equal(xn.isnan(), before.isnan())             # and the caller's tensor keeps it
        dev = dict(lengths=torch.tensor(LENGTHS, device=DEV), **(dict(y_lengths=_lens(Y_LENGTHS)) if cross else {}))
        assert torch.equal(tf.run_bct(xn, yn, **dev), out)         # device tensors (int64, int32): no host check, no sync
        assert torch.equal(tf(xn.transpose(1, 2), None if yn is None else yn.transpose(1, 2), **kw), out.transpose(1, 2))


@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
def test_modules_training(cross):
    m = _module(cross)
    tf = m["tf"].train()
    kw = dict(lengths=LENGTHS, **(dict(y_lengths=Y_LENGTHS) if cross else {}))

    def step(fill, w):
        for p in tf.parameters():
            p.grad = None
        x, y = _padded(m, fill)
        x.requires_grad_()
        if y is not None:
            y.requires_grad_()
        out = tf.run_bct(x, y, **kw)
        out.backward(w.to(DEV))                                    # an unmasked upstream gradient
        return out.detach(), x.grad, None if y is None else y.grad, {k: p.grad.clone() for k, p in tf.named_parameters()}

    out, dx, dy, grads = step(NAN, m["w"])
    assert max_abs(out.cpu(), m["want"]) < 1e-4
    for name, got, ref, lens, t in (("dx", dx, m["x64"].grad, LENGTHS, TX),) + ((("dy", dy, m["y64"].grad, Y_LENGTHS, TY),) if cross else ()):
        err, scale = max_abs(got.cpu(), ref), float(ref.abs().max())
        print(f"ragged training ({'cross' if cross else 'self'}) {name}: err {err:.3e}, max|ref| {scale:.3e}")
        assert err < 2e-4 * max(1.0, scale), name
        assert bool((got.cpu()[pad_mask(lens, t).expand_as(got)] == 0).all()), name       # exactly 0 at pads
    assert list(grads) == list(m["sd"])
    for name, g in grads.items():
        ref = m["sd64"][name].grad
        err, scale = max_abs(g.cpu(), ref), float(ref.abs().max())
        print(f"ragged training ({'cross' if cross else 'self'}) {name}: err {err:.3e}, max|ref| {scale:.3e}")
        assert err < 5e-4 * max(1.0, scale), name
    # pads contribute nothing: other padding in x / y, NaN in the upstream gradient's padding -- bitwise the same gradients
    out2, dx2, dy2, grads2 = step(HUGE, m["w"].masked_fill(pad_mask(LENGTHS, TX), NAN))
    assert torch.equal(out2, out) and torch.equal(dx2, dx) and (dy is None or torch.equal(dy2, dy))
    for name in grads:
        assert torch.equal(grads2[name], grads[name]), name


def test_other_surfaces_and_refusals_on_the_gpu():
    m = _module(False)
    tf = m["tf"].eval()
    x = m["x"].to(DEV)
    with torch.no_grad():
        want = tf.run_bct(x, lengths=LENGTHS)
        got, idx, loss = TransformerBottleneck(tf)(x.transpose(1, 2), lengths=LENGTHS)
        assert torch.equal(got, want.transpose(1, 2)) and idx is None and float(loss) == 0.0
        att = tf.layers[0][0]
        sub = att(x.transpose(1, 2), lengths=LENGTHS)
        assert bool(torch.isfinite(sub).all()) and bool((sub.transpose(1, 2)[pad_mask(LENGTHS, TX).to(DEV).expand_as(x)] == 0).all())
        alone = att(x[1:2, :, :LENGTHS[1]].transpose(1, 2))
        assert max_abs(sub[1:2, :LENGTHS[1]], alone) < 2e-5
        with pytest.raises(AgxError, match="y_lengths= on a Transformer without a cross-attention layer"):
            tf.run_bct(x, lengths=LENGTHS, y_lengths=LENGTHS)
        for bad in ([70, 23], torch.tensor([70, 23], device=DEV)):
            with pytest.raises(AgxError, match=r"one length per batch row is \(3,\)"):
                tf.run_bct(x, lengths=bad)
        with pytest.raises(AgxError, match=r"every length must lie in \[0, 70\]"):
            tf.run_bct(x, lengths=[71, 23, 1])
        assert torch.equal(tf.run_bct(x, lengths=torch.tensor([71, 23, 1], device=DEV)), want)     # on the device: clamped
        att.attention_dtype = "bf16"
        try:
            with pytest.raises(AgxError, match="ragged attention runs in fp32"):
                tf.run_bct(x, lengths=LENGTHS)
        finally:
            att.attention_dtype = "fp32"
        causal = Transformer(DIM, depth=1, heads=HEADS, head_dim=DH, context_x=80, causal=True).to(DEV).eval()
        with pytest.raises(AgxError, match="valid frames never see right padding"):
            causal.run_bct(x, lengths=LENGTHS)
        with pytest.raises(AgxError, match="lengths= with cache="):
            causal.run_bct(x[..., :5], cache=causal.new_cache(3), lengths=[5, 5, 5])
    drop = Transformer(DIM, depth=1, heads=HEADS, head_dim=DH, dropout=0.1, context_x=80).to(DEV).train()
    with pytest.raises(AgxError, match="lengths= with an active dropout site"):
        drop.run_bct(x, lengths=LENGTHS)
    assert drop.last_dropout_seed is None
