"""Packed variable-length batches on the GPU (csrc/attention_packed.hip): ``ops.attention_alibi_packed`` / ``_backward`` against
the float64 checker of ``tests/packed_attention_ref.py`` (the frozen definition on every cropped sequence), the two layout ops,
and ``Transformer.run_packed``.

Besides the value checks, the properties the feature exists for: a sequence of a packed batch is bitwise the ragged op on the
sequence cropped and run alone, what its neighbours and the slack hold never reaches it (NaN, 3.4e38 and 0 give bitwise the
same finite results), every result is exactly 0 in the columns no sequence owns, and a captured graph replays with the
partition its device array holds at replay time.

Tolerances are the ones the suite states for the same arithmetic: 3e-5 of max(1, max|o|) for the fp32 flash forward, 5e-5 / 1e-5
(max / rms, times max(1, scale of the reference quantity)) for the split backward (tests/test_gpu_ragged_attention.py), 1e-4 for
a depth-2 block against float64 and 2e-4 / 5e-4 for its input / parameter gradients, 2e-5 for a block against itself on another
batch layout (tests/test_gpu_blocks.py).  Every measured error is printed."""
import pytest
import torch

from audio_generation_amd import ops
from audio_generation_amd._lib import AgxError
from audio_generation_amd.transformers import Transformer, pack_padded, unpack_padded
from oracle import attention as oattn
from tests.helpers import max_abs, rms
from tests.packed_attention_ref import (CASE_IDS, CASES, case_inputs, case_shape, cu_of, pack_ref, packed_core, packed_transformer,
                                        unpack_ref)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, HUGE = float("nan"), 3.4e38
_REF, _RUNS = {}, {}


def _ref(n):
    """Inputs and the float64 results of case ``n``, computed once."""
    if n not in _REF:
        kind, heads, dh, ql, kl, nq, nk, max_q, max_k = case_shape(CASES[n])
        q, kv, dout, slopes = case_inputs(heads, dh, nq, nk)
        q64, kv64 = q.double().requires_grad_(), kv.double().requires_grad_()
        out = packed_core(q64, kv64, slopes, heads, dh, dh ** 0.5, cu_of(ql), cu_of(kl))
        out.backward(dout.double())
        _REF[n] = dict(q=q, kv=kv, dout=dout, slopes=slopes, out=out.detach(), dq=q64.grad, dkv=kv64.grad)
    return _REF[n]


def _cu(lengths):
    return torch.tensor(cu_of(lengths), dtype=torch.int32, device=DEV)


def _call(kind, q, kv, dout, slopes, heads, dh, cu_q, cu_k, max_q, max_k):
    """(out, dq, dkv) of one forward and one backward on device tensors; a "self" case goes through one qkv tensor."""
    if kind == "self":
        qkv = torch.cat([q, kv], dim=1)
        out = ops.attention_alibi_packed(qkv, None, slopes, heads, dh, dh ** 0.5, cu_q=cu_q, max_q=max_q)
        dqkv = ops.attention_alibi_packed_backward(qkv, None, slopes, out, dout, heads, dh, dh ** 0.5, cu_q=cu_q, max_q=max_q)
        assert dqkv.shape == qkv.shape
        hd = heads * dh
        return out, dqkv[:, :hd], dqkv[:, hd:]
    out = ops.attention_alibi_packed(q, kv, slopes, heads, dh, dh ** 0.5, cu_q=cu_q, max_q=max_q, cu_k=cu_k, max_k=max_k)
    dq, dkv = ops.attention_alibi_packed_backward(q, kv, slopes, out, dout, heads, dh, dh ** 0.5, cu_q=cu_q, max_q=max_q, cu_k=cu_k,
                                                  max_k=max_k)
    return out, dq, dkv


def _outside(lengths, n, keep):
    """(1, 1, n) bool: True at every column that sequence ``keep`` does not own (the other sequences and the slack)."""
    cu = cu_of(lengths)
    m = torch.ones(1, 1, n, dtype=torch.bool)
    m[..., cu[keep]:cu[keep + 1]] = False
    return m


def _run(n, keep=None, fill=None):
    """Case ``n``; with ``keep`` everything outside sequence ``keep`` in q, kv and dout is set to ``fill``.  Once per variant."""
    if (n, keep, fill) not in _RUNS:
        kind, heads, dh, ql, kl, nq, nk, max_q, max_k = case_shape(CASES[n])
        c = _ref(n)
        q, kv, dout = c["q"].clone(), c["kv"].clone(), c["dout"].clone()
        if keep is not None:
            q.masked_fill_(_outside(ql, nq, keep), fill)
            dout.masked_fill_(_outside(ql, nq, keep), fill)
            kv.masked_fill_(_outside(kl, nk, keep), fill)
        _RUNS[n, keep, fill] = _call(kind, q.to(DEV), kv.to(DEV), dout.to(DEV), c["slopes"].to(DEV), heads, dh, _cu(ql), _cu(kl), max_q,
                                     max_k)
    return _RUNS[n, keep, fill]


def _dead(ql, kl, n, which):
    """(1, 1, n) bool over the columns of ``which`` ("q" / "k"): the slack, and the sequences whose result is 0 by definition."""
    own = ql if which == "q" else kl
    cu = cu_of(own)
    m = torch.zeros(1, 1, n, dtype=torch.bool)
    m[..., cu[-1]:] = True
    for s in range(len(own)):
        if ql[s] == 0 or kl[s] == 0:
            m[..., cu[s]:cu[s + 1]] = True
    return m


@pytest.mark.parametrize("n", range(len(CASES)), ids=CASE_IDS)
def test_packed_forward_against_the_definition(n):
    _, heads, dh, ql, kl, nq, nk, _, _ = case_shape(CASES[n])
    want = _ref(n)["out"]
    got = _run(n)[0]
    assert tuple(got.shape) == (1, heads * dh, nq)
    err, scale = max_abs(got.cpu(), want), float(want.abs().max())
    print(f"packed forward {CASE_IDS[n]}: max err {err:.3e}, max|o| {scale:.3e}")
    assert err < 3e-5 * max(1.0, scale)
    assert bool((got.cpu()[_dead(ql, kl, nq, "q").expand_as(want)] == 0).all())     # exactly 0, not merely small


@pytest.mark.parametrize("n", range(len(CASES)), ids=CASE_IDS)
def test_packed_backward_against_float64_autograd(n):
    kind, heads, dh, ql, kl, nq, nk, max_q, max_k = case_shape(CASES[n])
    c = _ref(n)
    _, dq, dkv = _run(n)
    assert dq.shape == c["q"].shape and dkv.shape == c["kv"].shape
    for name, got, want in (("dq", dq, c["dq"]), ("dkv", dkv, c["dkv"])):
        e_max, e_rms = max_abs(got.cpu(), want), rms(got.cpu(), want)
        s_max, s_rms = float(want.abs().max()), float(want.pow(2).mean().sqrt())
        print(f"packed backward {CASE_IDS[n]} {name}: max err {e_max:.3e} (max {s_max:.3e}), rms err {e_rms:.3e} (rms {s_rms:.3e})")
        assert e_max < 5e-5 * max(1.0, s_max) and e_rms < 1e-5 * max(1.0, s_rms), name
    assert bool((dq.cpu()[_dead(ql, kl, nq, "q").expand_as(dq)] == 0).all())
    assert bool((dkv.cpu()[_dead(ql, kl, nk, "k").expand_as(dkv)] == 0).all())
    q, kv, dout = (c[k].to(DEV) for k in ("q", "kv", "dout"))
    again = _call(kind, q, kv, dout, c["slopes"].to(DEV), heads, dh, _cu(ql), _cu(kl), max_q, max_k)
    for a, g in zip(again, _run(n)):
        assert torch.equal(a, g)                                    # deterministic: no atomics


@pytest.mark.parametrize("n", range(len(CASES)), ids=CASE_IDS)
def test_a_sequence_is_the_ragged_op_on_its_crop(n):
    kind, heads, dh, ql, kl, nq, nk, _, _ = case_shape(CASES[n])
    c = _ref(n)
    out, dq, dkv = _run(n)
    cq, ck = cu_of(ql), cu_of(kl)
    slopes, args = c["slopes"].to(DEV), (heads, dh, dh ** 0.5)
    checked = 0
    for s in range(len(ql)):
        if ql[s] == 0 or kl[s] == 0:
            continue
        qs, ks = slice(cq[s], cq[s + 1]), slice(ck[s], ck[s + 1])
        q, kv, dout = c["q"][:, :, qs].contiguous().to(DEV), c["kv"][:, :, ks].contiguous().to(DEV), c["dout"][:, :, qs].contiguous().to(DEV)
        if kind == "self":                                          # batch 1, no lengths
            qkv = torch.cat([q, kv], dim=1)
            o1 = ops.attention_alibi_ragged(qkv, None, slopes, *args)
            d = ops.attention_alibi_ragged_backward(qkv, None, slopes, o1, dout, *args)
            dq1, dkv1 = d[:, :heads * dh], d[:, heads * dh:]
        else:
            o1 = ops.attention_alibi_ragged(q, kv, slopes, *args)
            dq1, dkv1 = ops.attention_alibi_ragged_backward(q, kv, slopes, o1, dout, *args)
        assert torch.equal(o1, out[:, :, qs]) and torch.equal(dq1, dq[:, :, qs]) and torch.equal(dkv1, dkv[:, :, ks]), s
        checked += 1
    assert checked >= len(ql) - 1


@pytest.mark.parametrize("n", range(len(CASES)), ids=CASE_IDS)
def test_the_neighbours_and_the_slack_may_hold_anything(n):
    _, heads, dh, ql, kl, nq, nk, _, _ = case_shape(CASES[n])
    base = _run(n)
    cq, ck = cu_of(ql), cu_of(kl)
    for s in range(len(ql)):
        if ql[s] == 0 and kl[s] == 0:
            continue
        for fill in (NAN, HUGE, 0.0):
            got = _run(n, s, fill)
            for name, a, g, cu in (("out", got[0], base[0], cq), ("dq", got[1], base[1], cq), ("dkv", got[2], base[2], ck)):
                a, g = a[:, :, cu[s]:cu[s + 1]], g[:, :, cu[s]:cu[s + 1]]
                assert bool(torch.isfinite(a).all()), (s, fill, name)
                assert torch.equal(a, g), (s, fill, name)
            assert bool((got[0][:, :, cq[-1]:] == 0).all())         # the slack of out stays exactly 0


# ------------------------------------------------------------------------------------------------- the layout ops
LAYOUTS = [((3, 5, 37), [37, 0, 20], None), ((2, 3, 5), [5, 2], 9), ((4, 7, 3), [0, 1, 2, 3], None), ((2, 64, 225), [225, 100], 400),
           ((1, 9, 300), [257], 257)]


@pytest.mark.parametrize("shape,lengths,total", LAYOUTS)
def test_pack_and_unpack_are_exact_selects_and_each_other_s_inverse(shape, lengths, total):
    b, c, t = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=gen)
    pads = torch.arange(t).reshape(1, 1, t) >= torch.tensor(lengths).reshape(-1, 1, 1)
    zeroed = x.masked_fill(pads, 0.0)
    n = sum(lengths) if total is None else total
    cu = _cu(lengths)
    xp = ops.pack_rows(x.masked_fill(pads, NAN).to(DEV), cu, n)     # NaN padding never reaches the packed tensor
    assert tuple(xp.shape) == (1, c, n) and torch.equal(xp.cpu(), pack_ref(x, lengths, n))
    back = ops.unpack_rows(xp, cu, t)
    assert torch.equal(back.cpu(), zeroed)                          # x with its padding zeroed, bitwise
    noisy = xp.clone()
    noisy[:, :, sum(lengths):] = NAN                                # NaN slack never reaches the padded tensor
    assert torch.equal(ops.unpack_rows(noisy, cu, t).cpu(), zeroed)
    assert torch.equal(ops.pack_rows(ops.unpack_rows(noisy, cu, t), cu, n), xp)       # xp with zero slack
    assert torch.equal(unpack_ref(xp.cpu(), cu_of(lengths), t), zeroed)
    # the adjoint identity <pack(x), g> == <x, unpack(g)> on small integers: exact in fp32, compared in float64
    xi = torch.randint(-8, 9, shape, generator=gen).float()
    gi = torch.randint(-8, 9, (1, c, n), generator=gen).float()
    lhs = (ops.pack_rows(xi.to(DEV), cu, n).double() * gi.to(DEV).double()).sum()
    rhs = (xi.to(DEV).double() * ops.unpack_rows(gi.to(DEV), cu, t).double()).sum()
    assert float(lhs) == float(rhs)


def test_layout_ops_clamp_what_the_device_array_holds():
    x = torch.randn(2, 3, 6, generator=torch.Generator().manual_seed(5)).to(DEV)
    for bad in ([0, 1000, 2000], [-5, 4, 3], [0, 9, 10], [7, 7, 7]):
        cu = torch.tensor(bad, dtype=torch.int32, device=DEV)
        xp = ops.pack_rows(x, cu, 10)
        assert bool(torch.isfinite(xp).all()) and bool(torch.isfinite(ops.unpack_rows(xp, cu, 6)).all())
    assert float(ops.unpack_rows(torch.empty(1, 3, 0, device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV), 6).abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------- modules
DIM, HEADS, DH = 64, 2, 32
LENGTHS, Y_LENGTHS = [80, 1, 33, 64], [65, 7, 128, 1]
N, NY, SLACK = sum(LENGTHS), sum(Y_LENGTHS), 6
TX, TY = max(LENGTHS), max(Y_LENGTHS)
_MOD = {}


def _module(cross):
    """(module on the device, float64 state dict with gradients, packed inputs with SLACK slack columns, float64 output)."""
    if cross not in _MOD:
        sd = oattn.init_state_dict(DIM, HEADS, DH, depth=2, seed=91)
        tf = Transformer(DIM, depth=2, heads=HEADS, head_dim=DH, context_x=96, **(dict(context_y=128) if cross else {}))
        tf.load_state_dict(sd)
        gen = torch.Generator().manual_seed(93)
        x, y, w = (torch.randn(1, DIM, N + SLACK, generator=gen), torch.randn(1, DIM, NY + SLACK, generator=gen),
                   torch.randn(1, DIM, N + SLACK, generator=gen))
        sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
        x64, y64 = x.double().requires_grad_(), y.double().requires_grad_()
        want = packed_transformer(x64.transpose(1, 2), y64.transpose(1, 2) if cross else None, sd64, HEADS, 2, cu_of(LENGTHS),
                                  cu_of(Y_LENGTHS) if cross else None).transpose(1, 2)
        (want * w.double()).sum().backward()
        _MOD[cross] = dict(tf=tf.to(DEV), sd=sd, sd64=sd64, x=x, y=y if cross else None, w=w, x64=x64, y64=y64 if cross else None,
                           want=want.detach())
    return _MOD[cross]


def _kw(cross, device=False):
    cu, ycu = cu_of(LENGTHS), cu_of(Y_LENGTHS)
    if device:
        return dict(cu_seqlens=_cu(LENGTHS), max_len=TX, **(dict(y_cu_seqlens=_cu(Y_LENGTHS), y_max_len=TY) if cross else {}))
    return dict(cu_seqlens=cu, **(dict(y_cu_seqlens=ycu) if cross else {}))


def _slacked(m, fill):
    """(x, y) on the device with their slack columns set to ``fill``."""
    x = m["x"].clone()
    x[:, :, N:] = fill
    y = None
    if m["y"] is not None:
        y = m["y"].clone()
        y[:, :, NY:] = fill
        y = y.to(DEV)
    return x.to(DEV), y


@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
def test_modules_eval(cross):
    m = _module(cross)
    tf = m["tf"].eval()
    tag = "cross" if cross else "self"
    x, y = m["x"].to(DEV), None if not cross else m["y"].to(DEV)
    with torch.no_grad():
        out = tf.run_packed(x, y=y, **_kw(cross))
        err = max_abs(out.cpu(), m["want"])
        print(f"packed block ({tag}) eval: {err:.3e} from float64")
        assert tuple(out.shape) == (1, DIM, N + SLACK) and err < 1e-4
        assert bool((out[:, :, N:] == 0).all())                     # exactly 0 in slack
        # the padded equivalent through lengths=: the block against itself on another batch layout
        cu, ycu = _cu(LENGTHS), _cu(Y_LENGTHS)
        xpad = ops.unpack_rows(x, cu, TX)
        ypad = None if not cross else ops.unpack_rows(y, ycu, TY)
        padded = tf.run_bct(xpad, ypad, lengths=LENGTHS, **(dict(y_lengths=Y_LENGTHS) if cross else {}))
        e = max_abs(ops.pack_rows(padded, cu, N + SLACK), out)
        print(f"packed block ({tag}) eval against run_bct(lengths=) on the padded batch: {e:.3e}")
        assert e < 2e-5
        xn, yn = _slacked(m, NAN)
        before = xn.clone()
        assert torch.equal(tf.run_packed(xn, y=yn, **_kw(cross)), out)              # NaN slack: bitwise the same
        assert torch.equal(xn.isnan(), before.isnan())                             # and the caller's tensor keeps it
        assert torch.equal(tf.run_packed(xn, y=yn, **_kw(cross, device=True)), out)   # device arrays: no host check, no sync
        assert torch.equal(tf.forward_packed(xn.transpose(1, 2), y=None if yn is None else yn.transpose(1, 2), **_kw(cross)),
                           out.transpose(1, 2))
        # without slack the walk masks nothing; the same sequences come out
        tight = tf.run_packed(x[:, :, :N].contiguous(), y=None if not cross else y[:, :, :NY].contiguous(), **_kw(cross))
        e = max_abs(tight, out[:, :, :N])
        print(f"packed block ({tag}) eval, no slack: {e:.3e} from the call with slack")
        assert e < 2e-5 and max_abs(tight.cpu(), m["want"][:, :, :N]) < 1e-4
        # pack_padded / unpack_padded round the same trip
        xp, cu2, max_len = pack_padded(xpad, LENGTHS)
        assert torch.equal(cu2, cu) and max_len == TX and torch.equal(xp, x[:, :, :N])
        xp, cu3, max_len = pack_padded(xpad, torch.tensor(LENGTHS, device=DEV), total=N + SLACK)
        assert torch.equal(cu3, cu) and max_len == TX and torch.equal(xp[:, :, :N], x[:, :, :N]) and bool((xp[:, :, N:] == 0).all())
        assert torch.equal(unpack_padded(out, cu_of(LENGTHS), TX), ops.unpack_rows(out, cu, TX))


@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
def test_modules_training(cross):
    m = _module(cross)
    tf = m["tf"].train()
    tag = "cross" if cross else "self"

    def step(fill, w, device):
        for p in tf.parameters():
            p.grad = None
        x, y = _slacked(m, fill)
        x.requires_grad_()
        if y is not None:
            y.requires_grad_()
        out = tf.run_packed(x, y=y, **_kw(cross, device))
        out.backward(w.to(DEV))                                    # an unmasked upstream gradient
        return out.detach(), x.grad, None if y is None else y.grad, {k: p.grad.clone() for k, p in tf.named_parameters()}

    out, dx, dy, grads = step(NAN, m["w"], False)
    assert max_abs(out.cpu(), m["want"]) < 1e-4
    for name, got, ref, n in (("dx", dx, m["x64"].grad, N),) + ((("dy", dy, m["y64"].grad, NY),) if cross else ()):
        err, scale = max_abs(got.cpu(), ref), float(ref.abs().max())
        print(f"packed training ({tag}) {name}: err {err:.3e}, max|ref| {scale:.3e}")
        assert err < 2e-4 * max(1.0, scale), name
        assert bool((got[:, :, n:] == 0).all()), name              # exactly 0 in slack
    assert list(grads) == list(m["sd"])
    for name, g in grads.items():
        ref = m["sd64"][name].grad
        err, scale = max_abs(g.cpu(), ref), float(ref.abs().max())
        print(f"packed training ({tag}) {name}: err {err:.3e}, max|ref| {scale:.3e}")
        assert err < 5e-4 * max(1.0, scale), name
    # the slack contributes nothing: other slack in x / y, NaN in the upstream gradient's slack, device arrays -- bitwise the same
    w2 = m["w"].clone()
    w2[:, :, N:] = NAN
    out2, dx2, dy2, grads2 = step(HUGE, w2, True)
    assert torch.equal(out2, out) and torch.equal(dx2, dx) and (dy is None or torch.equal(dy2, dy))
    for name in grads:
        assert torch.equal(grads2[name], grads[name]), name


def test_a_captured_graph_replays_with_the_partition_of_the_replay(monkeypatch):
    m = _module(False)
    tf = m["tf"].eval()
    x = m["x"].to(DEV)
    other = [33, 80, 64, 1]                                         # another partition of the same N and max_len
    assert sum(other) == N and max(other) == TX
    cu = _cu(LENGTHS)
    with torch.no_grad():
        want_first = tf.run_packed(x, cu, max_len=TX)
        want_other = tf.run_packed(x, _cu(other), max_len=TX)
    assert not torch.equal(want_first, want_other)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            tf.run_packed(x, cu, max_len=TX)
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    real_stream = ops._stream

    def spy():
        seen.append(torch.cuda.current_stream().cuda_stream)
        return real_stream()
    monkeypatch.setattr(ops, "_stream", spy)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        capture_stream = torch.cuda.current_stream().cuda_stream
        static_out = tf.run_packed(x, cu, max_len=TX)
    monkeypatch.undo()
    assert len(seen) == 2 * 7 + 2 and set(seen) == {capture_stream}     # 7 launches per layer + the two slack masks: a linear chain
    graph.replay()
    assert torch.equal(static_out, want_first)
    cu.copy_(_cu(other))
    graph.replay()
    assert torch.equal(static_out, want_other)


def test_refusals_on_the_gpu():
    m = _module(False)
    tf = m["tf"].eval()
    x = m["x"].to(DEV)
    cu = cu_of(LENGTHS)
    with torch.no_grad():
        with pytest.raises(AgxError, match="a device cu_seqlens needs max_len"):
            tf.run_packed(x, _cu(LENGTHS))
        with pytest.raises(AgxError, match=r"run_packed: x is \(2, 64, \d+\), expected \(1, 64, N\)"):
            tf.run_packed(torch.cat([x, x]), cu)
        with pytest.raises(AgxError, match="y_cu_seqlens= on a Transformer without a cross-attention layer"):
            tf.run_packed(x, cu, y_cu_seqlens=cu)
        with pytest.raises(AgxError, match="it must start at 0, never decrease and end at or before N"):
            tf.run_packed(x, [0, 50, 40, N])
        with pytest.raises(AgxError, match="exceed context_x = 96"):
            tf.run_packed(x, [0, 97, N])
        with pytest.raises(AgxError, match="run_packed with cache="):
            tf.run_packed(x, cu, cache=object())
        att = tf.layers[0][0]
        att.attention_dtype = "bf16"
        try:
            with pytest.raises(AgxError, match="a packed batch runs in fp32"):
                tf.run_packed(x, cu)
        finally:
            att.attention_dtype = "fp32"
        for kw in (dict(causal=True), dict(causal=True, window=8)):
            causal = Transformer(DIM, depth=1, heads=HEADS, head_dim=DH, context_x=96, **kw).to(DEV).eval()
            with pytest.raises(AgxError, match="run_packed on a causal"):
                causal.run_packed(x, cu)
        cross = _module(True)["tf"].eval()
        y = _module(True)["y"].to(DEV)
        with pytest.raises(AgxError, match="needs y and y_cu_seqlens"):
            cross.run_packed(x, cu)
        with pytest.raises(AgxError, match="x has 4 sequences and y has 3"):
            cross.run_packed(x, cu, y=y, y_cu_seqlens=[0, 65, 72, NY])
    drop = Transformer(DIM, depth=1, heads=HEADS, head_dim=DH, dropout=0.1, context_x=96).to(DEV).train()
    with pytest.raises(AgxError, match="run_packed with an active dropout site"):
        drop.run_packed(x, cu)
    assert drop.last_dropout_seed is None
