"""The input families and the shape list of ``tests/attention_cases.py`` do what they state (host only): each family's
property is proved in float64 on the float32 tensors the GPU tests feed the kernels, and the shape list reaches every attention
kernel row through the library's host-only name queries.  Without this file ``tests/test_gpu_attention_conditioned.py`` could
pass on inputs that exercise nothing."""
import pytest
import torch

from audio_generation_amd import ops
from oracle import attention as oattn
from tests import attention_cases as ac

# (b, heads, dh, tq, tk): the extremes of the GPU file's list -- smallest and largest head dim, tk across several 64-key blocks
# with a partial last one, and both orders of tq != tk
GEOMETRIES = [(2, 3, 8, 321, 321), (1, 3, 128, 129, 129), (2, 3, 16, 65, 130), (2, 3, 16, 130, 65), (1, 3, 33, 257, 257),
              (1, 3, 8, 64, 1025)]


def _logits(case):
    return ac.logits(case.q.double(), case.kv.double(), case.slopes, case.heads, case.dh)


def _block_max(s, width):
    tk = s.shape[-1]
    return torch.stack([s[..., j0:j0 + width].max(-1).values for j0 in range(0, tk, width)], dim=-1)


@pytest.fixture(scope="module")
def lib():
    from audio_generation_amd import build
    build.build()
    return ops._lib.load()


@pytest.mark.parametrize("b,heads,dh,tq,tk", GEOMETRIES)
@pytest.mark.parametrize("width", [32, 64])
def test_ramp_block_maxima_climb_or_fall_by_at_least_5(b, heads, dh, tq, tk, width):
    up = _block_max(_logits(ac.ramp_up(b, heads, dh, tq, tk, seed=3)), width)
    assert up.shape[-1] >= 2 and float((up[..., 1:] - up[..., :-1]).min()) >= 5.0
    s = _logits(ac.ramp_up(b, heads, dh, tq, tk, seed=3))
    assert bool((s.argmax(-1) >= (tk - 1) // width * width).all())          # the last (partial) block holds the row maximum
    down = _block_max(_logits(ac.ramp_down(b, heads, dh, tq, tk, seed=3)), width)
    assert float((down[..., :-1] - down[..., 1:]).min()) >= 5.0
    assert bool((_logits(ac.ramp_down(b, heads, dh, tq, tk, seed=3)).argmax(-1) < width).all())


@pytest.mark.parametrize("b,heads,dh,tq,tk", GEOMETRIES + [(2, 3, 16, 257, 1), (2, 3, 16, 1, 257), (2, 3, 8, 33, 33)])
def test_spike_margin_and_one_hot_rows(b, heads, dh, tq, tk):
    case = ac.spike(b, heads, dh, tq, tk, seed=5)
    s = _logits(case)
    jstar = ac.spike_key_of_query(tq, tk)
    assert set(jstar.tolist()) == set(ac.spike_targets(tk)) or tq < len(ac.spike_targets(tk))
    if tk >= 66:
        assert ac.spike_targets(tk) == [0, 31, 32, 63, 64, tk - 1]
    top = s.gather(-1, jstar.reshape(1, 1, tq, 1).expand(b, heads, tq, 1))
    rest = s.scatter(-1, jstar.reshape(1, 1, tq, 1).expand(b, heads, tq, 1), -float("inf"))
    if tk > 1:
        assert float((top.squeeze(-1) - rest.max(-1).values).min()) >= 40.0
    p = s.softmax(-1).gather(-1, jstar.reshape(1, 1, tq, 1).expand(b, heads, tq, 1))
    assert float(p.min()) >= 1 - 1e-12
    # hence the output is v[:, j*]
    out = ac.cross_core(case.q.double(), case.kv.double(), case.slopes, heads, dh, case.scale_div)
    v = case.kv[:, heads * dh:].double()
    assert float((out - v[:, :, jstar]).abs().max()) <= 1e-10


@pytest.mark.parametrize("b,heads,dh,tq,tk", GEOMETRIES)
def test_offset_logits_lie_between_expf_overflow_and_130(b, heads, dh, tq, tk):
    s = _logits(ac.offset(b, heads, dh, tq, tk, seed=7))
    assert ac.EXPF_OVERFLOW < float(s.min()) and float(s.max()) < 130.0
    assert not torch.isfinite(s.float().exp()).any()            # expf of any logit as it stands is inf in fp32
    assert 0.5 < float(s.std()) < 4.0                           # c + N(0, 1) under a slowly varying ALiBi term


@pytest.mark.parametrize("b,heads,dh,tq,tk", GEOMETRIES)
def test_local_probabilities_are_the_closed_form(b, heads, dh, tq, tk):
    case = ac.local(b, heads, dh, tq, tk, seed=9)
    assert case.slopes.tolist() == [0.0, 8.0, 0.5]
    p = _logits(case).softmax(-1)
    i = torch.arange(tq, dtype=torch.float64).reshape(-1, 1)
    j = torch.arange(tk, dtype=torch.float64).reshape(1, -1)
    closed = (-(i - j).abs().unsqueeze(0) * case.slopes.double().reshape(-1, 1, 1)).exp()
    closed = closed / closed.sum(-1, keepdim=True)
    assert float((p - closed.unsqueeze(0)).abs().max()) <= 1e-12
    v = case.kv[:, heads * dh:].reshape(b, heads, dh, tk)
    assert torch.equal(v[:, :, 0], torch.arange(tk, dtype=torch.float32).expand(b, heads, tk))
    # slope 8 leaves only |i - j| <= 2: everything farther away weighs less than exp(-24)
    rows = min(tq, tk)                                          # (queries past the last key see the last keys from afar)
    far = ((i - j).abs() > 2)[:rows]
    near = p[:, 1, :rows]
    assert float(near[:, far].max()) < 4e-11 and float(near.masked_fill(far, 0).sum(-1).min()) > 1 - 1e-10
    assert float((p[:, 0] - 1.0 / tk).abs().max()) <= 1e-12     # slope 0: plain softmax of identical keys


def test_gauss_is_the_suites_usual_input_and_self_core_is_the_flash_tests_definition():
    case = ac.gauss(2, 3, 16, 40, 40, seed=1)
    assert 0.6 < float(case.qkv.std()) < 0.8 and torch.equal(case.slopes, oattn.alibi_slopes(3))
    qkv = case.qkv.double()
    q, k, v = (z.reshape(2, 3, 16, 40) for z in qkv.chunk(3, dim=1))          # _core of tests/test_gpu_attention_flash.py
    s = torch.einsum("bhdi,bhdj->bhij", q, k) / 16 ** 0.5 + oattn.alibi_bias(3, 40, 40).double()
    want = torch.einsum("bhij,bhdj->bhdi", s.softmax(-1), v).reshape(2, 48, 40)
    # (that one rounds slope * |i - j| to fp32 before it widens it; here, as in cross_core, the product is exact)
    assert float((ac.self_core(qkv, case.slopes, 3, 16) - want).abs().max()) <= 2.0 ** -24 * 40 * float(want.abs().max())
    assert torch.equal(ac.self_core(qkv, case.slopes, 3, 16), ac.cross_core(case.q.double(), case.kv.double(), case.slopes, 3, 16, 4.0))


@pytest.mark.parametrize("family", list(ac.FAMILIES))
def test_yardstick_is_finite_and_nonzero_where_the_family_is_not_exact(family):
    case = ac.FAMILIES[family](2, 3, 16, 65, 65, seed=11)
    dout = torch.randn(2, 48, 65, generator=torch.Generator().manual_seed(2))
    for ref in (ac.self_reference(case, dout), ac.cross_reference(case, dout)):
        for name, want in ref.want.items():
            assert want.dtype == torch.float64 and torch.isfinite(want).all()
            assert ref.err_max[name] >= ref.err_rms[name] >= 0 and ref.err_max[name] < 1e-2 * max(1.0, float(want.abs().max()))
            if family in ("ramp_up", "ramp_down", "offset", "gauss"):
                assert ref.err_max[name] > 0 and ref.err_rms[name] > 0, name
    # the criterion's arithmetic
    assert ac.needed(1e-6, 1e-7, 2e-6) == 0.0 and ac.needed(5e-6, 1e-6, 1e-6) == pytest.approx(4.0)
    assert ac.needed(5e-6, 0.0, 1e-6) == float("inf")
    assert ac.floor_of(torch.tensor([0.5])) == 4 * 2.0 ** -23 and ac.floor_of(torch.tensor([-300.0])) == 1200 * 2.0 ** -23


def test_bf16_reference_rounds_operands_and_probabilities_only():
    """On operands that bf16 holds exactly and one key per row (p = 1) the rounded definition IS the definition; on random
    operands it differs from it by bf16 rounding (2^-9 relative per operand), not more."""
    case = ac.spike(1, 3, 8, 65, 65, seed=13)
    exact = ac.AttnCase(case.q.bfloat16().float(), case.kv.bfloat16().float(), case.slopes, 3, 8)
    got = ac.self_core_bf16(exact.qkv, exact.slopes, 3, 8)
    assert float((got - ac.self_core(exact.qkv.double(), exact.slopes, 3, 8)).abs().max()) <= 1e-12
    case = ac.gauss(1, 3, 33, 130, 130, seed=13)
    want = ac.self_core(case.qkv.double(), case.slopes, 3, 33)
    err = float((ac.self_core_bf16(case.qkv, case.slopes, 3, 33) - want).abs().max())
    assert 1e-5 < err < 1e-2 * float(want.abs().max())


# ------------------------------------------------------------------------------------------------ the shape list reaches every row
def test_forward_shapes_reach_every_single_pass_flash_and_bf16_row(lib):
    name = ops.attention_kernel_name
    assert {name(ac.B, ac.HEADS, dh, t) for dh, t in ac.SINGLE_PASS_SHAPES} == ac.ALL_SINGLE_PASS_ROWS
    assert all(t <= 256 and dh in (8, 33, 64, 65, 128) for dh, t in ac.SINGLE_PASS_SHAPES)
    flash32 = {name(ac.B, ac.HEADS, dh, t, ops.ATTN_FP32, flash) for dh, t, flash in ac.FLASH_SHAPES}
    bf16 = {name(ac.B, ac.HEADS, dh, t, ops.ATTN_BF16) for dh, t in ac.BF16_SHAPES}
    assert flash32 == {r for r in ac.ALL_FLASH_ROWS if r.endswith(",0>")}
    assert bf16 == ac.ALL_BF16_LDS_ROWS | {r for r in ac.ALL_FLASH_ROWS if r.endswith(",1>")}
    assert flash32 | bf16 == ac.ALL_FLASH_ROWS | ac.ALL_BF16_LDS_ROWS
    # without flash=True a fp32 shape of t <= 256 would run the single-pass kernel
    assert all(flash == (t <= 256) for _, t, flash in ac.FLASH_SHAPES)
    # the consistency check runs the online-softmax kernel on every single-pass shape as well
    assert {name(ac.B, ac.HEADS, dh, t, ops.ATTN_FP32, True) for dh, t in ac.SINGLE_PASS_SHAPES} == flash32


def test_cross_shapes_reach_every_cross_row(lib):
    name = ops.attention_cross_kernel_name
    assert {name(ac.B, ac.HEADS, dh, tq, tk) for dh, tq, tk in ac.CROSS_FORWARD_SHAPES} == ac.ALL_CROSS_ROWS
    assert {name(ac.B, ac.HEADS, dh, tq, tk, backward=True) for dh, tq, tk in ac.CROSS_BACKWARD_SHAPES} == \
        {"attn_cross_bwd_stats+attn_cross_bwd_dq+attn_cross_bwd_dkv"}
    assert {(tq, tk) for _, tq, tk in ac.CROSS_BACKWARD_SHAPES} == set(ac.CROSS_LENGTHS)
    assert {dh for dh, _, _ in ac.CROSS_BACKWARD_SHAPES} == {16, 128}


def test_backward_shapes_reach_both_single_launch_kernels_and_the_split(lib):
    name = ops.attention_backward_kernel_name
    got = {}
    for dh, t, split in ac.BACKWARD_SHAPES:
        if split:       # beyond the single-launch kernel: ops.attention_alibi_backward(..., out=out) takes the split path
            with pytest.raises(ops.AgxError):
                name(ac.HEADS, dh, t)
        got[(dh, t)] = name(ac.HEADS, dh, t, split=split)
    assert got == {(64, 225): "attention_alibi_bwd<16>", (64, 256): "attention_alibi_bwd<8>", (16, 40): "attention_alibi_bwd<16>",
                   (128, 130): "attn_bwd_stats+attn_bwd_dq+attn_bwd_dkv", (33, 257): "attn_bwd_stats+attn_bwd_dq+attn_bwd_dkv"}
    assert set(got.values()) == ac.ALL_BACKWARD_ROWS


# ------------------------------------------------------------------------------------------------ LayerNorm inputs
def test_layernorm_families():
    b, c, t = 2, 65, 17
    x = ac.ln_input("offset", b, c, t, seed=1)
    assert 990 < float(x.min()) and float(x.max()) < 1010 and 0.9 < float(x.double().std()) < 1.1
    x = ac.ln_input("constant", b, c, t, seed=1)
    cols = ac.ln_constant_columns(t)
    assert int(cols.sum()) == 6 and bool(cols[0])
    assert float(x[:, :, cols].double().var(dim=1, unbiased=False).max()) == 0.0
    assert float(x[:, :, ~cols].double().var(dim=1, unbiased=False).min()) > 0.3
    assert ac.ln_constant_columns(1).tolist() == [True]
    w, bias = ac.ln_params(c, seed=1)
    ref = ac.ln_reference(x, w, bias)
    assert torch.equal(ref.want["y"][:, :, cols], bias.double().reshape(1, c, 1).expand(b, c, 6))   # y == bias exactly
    x = ac.ln_input("outlier", b, c, t, seed=1)
    assert int((x == 1e4).sum()) == b * t and float(x.abs().median()) < 1.0
    dy = torch.randn(b, c, t, generator=torch.Generator().manual_seed(3))
    ref = ac.ln_reference(x, None, None, dy, add=dy)
    assert set(ref.want) == {"y", "dx", "dweight", "dbias"}
    assert all(0 < ref.err_rms[n] <= ref.err_max[n] < 1e-2 for n in ref.want)
    # every dispatch threshold of agx_layernorm_ct has a channel count on both sides, and a masked one in every instantiation
    for lo, hi in [(1, 64), (65, 128), (129, 256), (257, 512), (513, 1024), (1025, 2048), (2049, 1 << 30)]:
        inside = [ch for ch in ac.LN_CHANNELS if lo <= ch <= hi]
        assert inside and any(ch % 32 for ch in inside), (lo, hi)
    assert any(tt % 16 and tt % 64 for tt in ac.LN_LENGTHS)
