"""Quantiser dropout without a GPU: the CPU statement of the staged training call (tests/rvq_dropout_ref.py)
against autograd of ``oracle.rvq.residual_quantize_train`` where every row runs every stage, the clamp of the stage counts,
``ResidualQuantizer.dropout_stages``, the two new entry points in header, binding and library, and the refusals of ops, module
and model, which precede every launch."""
import os

import pytest
import torch

from audio_generation_amd import _lib, ops
from audio_generation_amd._lib import AgxError
from audio_generation_amd.quantizer import ResidualQuantizer
from oracle import rvq
from tests import rvq_dropout_ref as ref
from tests.test_codec_stream_cpu import _model

SYMBOLS = ("agx_rvq_forward_staged", "agx_rvq_backward_staged")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "agx.h")


def test_entry_points_in_header_binding_and_library():
    lib = _lib.load()
    header = open(HEADER).read()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "DESIGN 4.26" in header
    sig = _lib.SIGNATURES
    assert len(sig["agx_rvq_forward_ex"][1]) == 21 and len(sig["agx_rvq_backward"][1]) == 25         # the old ones as they were
    assert len(sig["agx_rvq_forward_staged"][1]) == 22 and len(sig["agx_rvq_backward_staged"][1]) == 26


def test_taken_stages_clamps_at_both_ends():
    assert ref.taken([4, 1, 2, 0, 2, -7], 6, 3) == [3, 1, 2, 0, 2, 0]
    assert ref.taken(torch.tensor([0, 9, -3, 1]), 4, 2) == [0, 2, 0, 1]
    assert ref.taken(None, 4, 8) == [8] * 4
    assert ref.live_mask([0, 9, -3, 1], 4, 2).tolist() == [[False, False], [True, True], [False, False], [True, False]]


def _case(seed=3, b=3, t=7, d=8, k=16, q=3):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(b, t, d, generator=gen), torch.randn(q, k, d, generator=gen), torch.randn(b, t, d, generator=gen),
            0.5 + float(torch.rand((), generator=gen)))


def test_every_row_at_q_is_the_unstaged_training_call():
    """With every q_b = Q the reference's loss and gradients are autograd of ``oracle.rvq.residual_quantize_train``.  That
    oracle is run in float64 on the same fp32 values, so the two differ by the roundings of the reference's fp32 residual
    chain only -- which is what the reference's own bound ``2 (m + 2) 2^-24 sum|addends|`` covers."""
    x, cbs, g_xq, g_l = _case()
    b, q = x.shape[0], cbs.shape[0]
    xq, index, sq_err, commit = ref.forward(x, cbs, [q] * b)
    want_q, want_i, want_c = rvq.residual_quantize(x, cbs)
    assert torch.equal(xq, want_q) and torch.equal(index, want_i)
    assert abs(commit - float(want_c)) <= 1e-6 * abs(float(want_c))
    for stages in ([q] * b, [q + 4] * b, None):
        dx, dc, bound_dx, _, chosen, loss = ref.definition(x, cbs, index, stages, g_xq, g_l)
        x64 = x.double().requires_grad_(True)
        sq, idx, commit64 = rvq.residual_quantize_train(x64, cbs.double())
        assert torch.equal(idx, index)
        ((sq * g_xq.double()).sum() + g_l * commit64).backward()
        want_l = float(commit64.detach())
        assert abs(loss - want_l) <= 1e-6 * abs(want_l)
        assert abs(loss - commit) <= 1e-12 * abs(commit)                       # forward's sq_err and definition's L: one chain
        assert bool(((dx - x64.grad).abs() <= bound_dx).all())
        assert bool(chosen.any(dim=1).all()) and float(dc[~chosen].abs().max()) == 0.0


def test_staged_reference_rows_are_prefix_runs():
    x, cbs, g_xq, g_l = _case(seed=5, b=4)
    stages = [0, 9, -3, 1]                                                     # -> 0, 3, 0, 1
    xq, index, sq_err, commit = ref.forward(x, cbs, stages)
    full_q, full_i, _ = rvq.residual_quantize(x, cbs)
    assert torch.equal(xq[1], full_q[1]) and torch.equal(index[1], full_i[1])
    assert not xq[0].any() and not xq[2].any() and bool((index[0] == -1).all()) and bool((index[2] == -1).all())
    assert torch.equal(index[3, :, 0], full_i[3, :, 0]) and bool((index[3, :, 1:] == -1).all())
    assert torch.equal(xq[3], cbs[0][full_i[3, :, 0]])
    # sq_err[q]: the frames live at q only; commit: the mean over rows of each row's own loss
    own = [float(rvq.residual_quantize(x[r:r + 1], cbs, q_b)[2]) for r, q_b in enumerate(ref.taken(stages, 4, 3))]
    assert abs(commit - sum(own) / 4) <= 1e-6 * abs(commit)
    dx, dc, _, _, chosen, loss = ref.definition(x, cbs, index, stages, g_xq, g_l)
    assert abs(loss - commit) <= 1e-12 * abs(commit)
    assert torch.equal(dx[0], g_xq[0].double()) and torch.equal(dx[2], g_xq[2].double())       # q_b = 0: g_xq alone
    assert not torch.equal(dx[1], g_xq[1].double())
    assert not chosen[2].any() or bool((index[1, :, 2] >= 0).all())            # stage 2: row 1 only
    assert float(dc[~chosen].abs().max()) == 0.0
    # not the unstaged definition on the masked index: there a dead stage's residual still enters the loss
    from tests.test_gpu_rvq_backward import definition as unstaged
    assert not torch.equal(unstaged(x, cbs, index, g_xq, g_l)[0], dx)


def test_masked_ema_statistics():
    x, cbs, _, _ = _case(seed=7, b=4)
    stages = [3, 1, 0, 2]
    _, index, _, _ = ref.forward(x, cbs, stages)
    frames, flat = x.reshape(-1, 8), index.reshape(-1, 3)
    stats = ref.ema_stats(frames, cbs, flat)
    t = x.shape[1]
    assert stats[:, :, 0].sum(dim=1).tolist() == [3 * t, 2 * t, 1 * t]          # the rows live at each stage
    row0 = rvq.ema_assignment_stats(frames[:t], cbs, flat[:t])                 # a full row alone: the oracle's statistics
    rest = ref.ema_stats(frames[t:], cbs, flat[t:])
    assert torch.allclose(stats, row0 + rest, rtol=0, atol=1e-5)


def test_dropout_stages_draw():
    torch.manual_seed(0)
    m = ResidualQuantizer(num_quantizers=8, dim=4, codebook_sizes=4)
    a = m.dropout_stages(64, generator=torch.Generator().manual_seed(11))
    b = m.dropout_stages(64, generator=torch.Generator().manual_seed(11))
    assert a.dtype == torch.int64 and a.shape == (64,) and a.device == m.codebooks.device and a.is_contiguous()
    assert torch.equal(a, b) and not torch.equal(a, m.dropout_stages(64, generator=torch.Generator().manual_seed(12)))
    assert int(a.min()) >= 1 and int(a.max()) <= 8 and len(set(a.tolist())) > 3
    assert m.dropout_stages(64, p=0.0, generator=torch.Generator().manual_seed(1)).tolist() == [8] * 64
    for low in (0, 1, 5, 8):
        s = m.dropout_stages(256, p=1.0, low=low, generator=torch.Generator().manual_seed(low))
        assert int(s.min()) >= low and int(s.max()) <= 8
        assert set(s.tolist()) == set(range(low, 9))                           # 256 draws over at most 9 values: all of them
    half = m.dropout_stages(4096, p=0.5, low=1, generator=torch.Generator().manual_seed(2))
    assert 0.5 < float((half == 8).float().mean()) < 0.62                      # 1/2 + 1/2 * 1/8 = 0.5625, +- 7 sigma
    for bad in (dict(low=9), dict(low=-1), dict(p=1.5), dict(p=-0.1)):
        with pytest.raises(ValueError):
            m.dropout_stages(4, **bad)


def _bad_stages(batch):
    """(stages, why) that every entry must refuse: int32, the wrong length, a non-contiguous view, not a tensor."""
    return [(torch.zeros(batch, dtype=torch.int32), "int32"), (torch.zeros(batch + 1, dtype=torch.int64), "length"),
            (torch.zeros(2 * batch, dtype=torch.int64)[::2], "stride"), (torch.zeros(batch, 1, dtype=torch.int64), "2-d"),
            ([1] * batch, "a list")]


def test_op_refusals_precede_the_launch():
    """On the CPU nothing can be launched: a call that got past the checks raises the 'MI355X only' error instead."""
    x, cbs = torch.zeros(2, 3, 8), torch.zeros(2, 16, 8)
    packed, idx, good = torch.zeros(4), torch.zeros(2, 3, 2, dtype=torch.int64), torch.ones(2, dtype=torch.int64)
    for bad, why in _bad_stages(2):
        with pytest.raises(AgxError, match="rvq_forward: stages"):
            ops.rvq_forward(x, cbs, packed, 2, stages=bad)
        with pytest.raises(AgxError, match="rvq_backward: stages"):
            ops.rvq_backward(x, cbs, idx, None, None, stages=bad)
    with pytest.raises(AgxError, match="stages is on 'meta', the inputs are on 'cpu'"):
        ops.rvq_forward(x, cbs, packed, 2, stages=good.to("meta"))
    with pytest.raises(AgxError, match="stages is on 'meta', the inputs are on 'cpu'"):
        ops.rvq_backward(x, cbs, idx, None, None, stages=good.to("meta"))
    with pytest.raises(AgxError, match="MI355X only"):                                           # past the check: the launch is next
        ops.rvq_forward(x, cbs, packed, 2, stages=good)
    with pytest.raises(AgxError, match="MI355X only"):
        ops.rvq_backward(x, cbs, idx, None, None, stages=good)
    with pytest.raises(TypeError):
        ops.rvq_forward(x, cbs, packed, 2, "b l c", good)                                        # stages is keyword-only
    with pytest.raises(TypeError):
        ops.rvq_backward(x, cbs, idx, None, None, "b l c", False, good)


def test_module_and_model_refusals_precede_every_launch():
    m = ResidualQuantizer(num_quantizers=2, dim=8, codebook_sizes=16).eval()
    x, good = torch.zeros(2, 3, 8), torch.ones(2, dtype=torch.int64)
    with torch.no_grad():
        for bad, why in _bad_stages(2):
            with pytest.raises(AgxError, match="ResidualQuantizer: stages"):
                m(x, stages=bad)
            with pytest.raises(AgxError, match="ResidualQuantizer: stages"):
                m.quantize_bcl(x.transpose(1, 2), stages=bad)
        with pytest.raises(AgxError, match="MI355X only"):
            m(x, stages=good)
        with pytest.raises(TypeError):
            m(x, None, False, False, good)                                                       # keyword-only
    # a replacement bottleneck that only honours the reference call contract has no per-row stage count
    model = _model()

    class Plain(torch.nn.Module):
        def forward(self, z, codebook_n=None, update_codebook=False, prioritize_early=False):
            return z, torch.zeros(z.shape[0], z.shape[1], 2, dtype=torch.int64), z.new_zeros(())

    model.quantizer = Plain()
    model._run_encoders = lambda z: torch.zeros(2, 8, 3)                                         # (no kernel runs on the CPU)
    wave = torch.zeros(2, 1, 18)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="stages= needs the native quantiser"):
            model.encode(wave, stages=good)
        with pytest.raises(NotImplementedError, match="stages= needs the native quantiser"):
            model(wave, stages=good)
        zq, commit, index = model.encode(wave)                                                   # without stages: as before
        assert zq.shape == (2, 8, 3) and index.shape == (2, 3, 2)
