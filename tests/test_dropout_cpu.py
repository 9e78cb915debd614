"""Dropout, the host side (no kernel is launched): the Philox mirror of ``tests/philox.py`` against the known-answer vectors, the
modules that take the reference's ``dropout`` argument construct with the reference's module tree, and
``agx_attention_dropout_kernel_name`` answers from the pick the launcher uses (csrc/attention_dropout.hip: ``attn_drop_pick``)."""
import numpy as np
import pytest
import torch

from audio_generation_amd import _lib, ops
from audio_generation_amd._lib import AgxError
from audio_generation_amd.transformers import Attention, FeedForward, Transformer
from audio_generation_amd.vae import CausalResidualBlock1d
from audio_generation_amd.wavelets import CausalMultiresConv1d
from tests import philox


@pytest.fixture(scope="module")
def lib():
    from audio_generation_amd import build
    build.build()
    return _lib.load()


KAT = [  # (counter, key, output): the zero and all-ones vectors and the pi-digit vector of the Random123 known-answer file
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_the_mirror_reproduces_the_known_answer_vectors():
    for counter, key, want in KAT:
        assert tuple(int(w) for w in philox.philox4x32_10(*counter, *key)) == want
    # vectorised: the three at once
    c = np.array([k[0] for k in KAT], dtype=np.uint64).T
    k = np.array([k[1] for k in KAT], dtype=np.uint64).T
    got = np.stack(philox.philox4x32_10(*c, *k), axis=-1)
    assert got.dtype == np.uint32 and got.tolist() == [list(k[2]) for k in KAT]


def test_the_keep_rule():
    assert philox.thresh_scale(0.0) == (0, np.float32(1.0))
    assert philox.thresh_scale(0.5) == (2 ** 31, np.float32(2.0))
    assert philox.thresh_scale(0.1)[0] == 429496730 and philox.thresh_scale(0.1)[1] == np.float32(1.0 / 0.9)
    assert philox.thresh_scale(1.0 - 2.0 ** -40)[0] == 2 ** 32 - 1
    # the two packings: word j & 3 of the quartet's call; a mask is a function of (seed, stream, b H + h, i, j) alone
    w = philox.attention_words(0x0123456789ABCDEF, 5, 2, 3, 7, 10)
    assert w.shape == (2, 3, 7, 10)
    one = philox.philox4x32_10(9 >> 2, 6, 1 * 3 + 2, 5, 0x89ABCDEF, 0x01234567)
    assert int(w[1, 2, 6, 9]) == int(one[9 & 3])
    assert np.array_equal(philox.attention_words(0x0123456789ABCDEF, 5, 1, 3, 4, 6), w[:1, :, :4, :6])
    e = philox.elementwise_words(7, 2, 11)
    assert int(e[10]) == int(philox.philox4x32_10(2, 0, 0, 2, 7, 0)[2])


def test_modules_construct_with_dropout_and_keep_the_reference_module_tree():
    builds = [lambda p: Transformer(8, 1, heads=2, head_dim=4, dropout=p, context_x=8),
              lambda p: Attention(8, dropout=p),
              lambda p: FeedForward(8, 8, dropout=p)]
    for build in builds:
        with_p, without = build(0.1), build(0.0)
        assert list(with_p.state_dict()) == list(without.state_dict())
        assert [n for n, _ in with_p.named_modules()] == [n for n, _ in without.named_modules()]
        drops = [m for m in with_p.modules() if isinstance(m, torch.nn.Dropout)]
        assert drops and all(m.p == 0.1 for m in drops)
    tf = Transformer(8, 1, heads=2, head_dim=4, dropout=0.1, context_x=8)
    attention, ff = tf.layers[0]
    assert isinstance(attention.dropout, torch.nn.Dropout) and isinstance(ff.net[3], torch.nn.Dropout) and isinstance(ff.net[5], torch.nn.Dropout)
    assert tf.last_dropout_seed is None
    for bad in (-0.1, 1.5):      # nn.Dropout's own range check
        with pytest.raises(ValueError):
            Transformer(8, 1, heads=2, head_dim=4, dropout=bad, context_x=8)
    # p = 1 constructs; it is refused at the first training-mode call (before any tensor reaches a kernel)
    one = Transformer(8, 1, heads=2, head_dim=4, dropout=1.0, context_x=8)
    with pytest.raises(AgxError, match="0 <= p < 1"):
        one.train().run_bct(torch.zeros(1, 8, 4))


def test_conv_stack_layers_construct_with_dropout_and_refuse_training():
    block = CausalResidualBlock1d(4, 4, dropout=0.1)
    multires = CausalMultiresConv1d(4, 3, 2, dropout=0.1)
    assert list(block.state_dict()) == list(CausalResidualBlock1d(4, 4).state_dict())
    assert list(multires.state_dict()) == list(CausalMultiresConv1d(4, 3, 2).state_dict())
    assert block.dropout.p == 0.1 and multires.dropout_layer.p == 0.1
    x = torch.zeros(1, 4, 16)
    for layer in (block, multires):
        with pytest.raises(AgxError, match="in training mode has no kernel"):
            layer.train()(x)
        with pytest.raises(AgxError, match="in training mode has no kernel"):
            layer.units()
        with pytest.raises(AgxError, match="MI355X only"):      # eval mode: past the refusal, on to the kernels
            layer.eval()(x)


def test_the_float64_restatement_without_dropout_is_the_checker():
    """``tests/dropout_ref.py`` at p = 0 (every factor 1) against ``oracle.attention`` / ``tests/cross_attention_ref.py``, and the
    placement of its masks: with p > 0 the output moves, and the elementwise factors follow the channel-major linear index."""
    from oracle import attention as oattn
    from tests.cross_attention_ref import cross_core, cross_transformer
    from tests.dropout_ref import attention_factor, drop_core, dropout_transformer, elementwise_factor
    sd = {k: v.double() for k, v in oattn.init_state_dict(16, 2, 4, depth=2, seed=3).items()}
    gen = torch.Generator().manual_seed(1)
    x, y = torch.randn(2, 16, 9, generator=gen).double(), torch.randn(2, 16, 5, generator=gen).double()
    want = oattn.transformer(x.transpose(1, 2), sd, 2, depth=2).transpose(1, 2)
    assert torch.allclose(dropout_transformer(x, None, sd, 2, 2, 0.0, 99), want, rtol=0, atol=1e-12)
    want = cross_transformer(x.transpose(1, 2), y.transpose(1, 2), sd, 2, depth=2).transpose(1, 2)
    assert torch.allclose(dropout_transformer(x, y, sd, 2, 2, 0.0, 99), want, rtol=0, atol=1e-12)
    assert float((dropout_transformer(x, y, sd, 2, 2, 0.25, 99) - want).abs().max()) > 1e-2
    q, kv = torch.randn(2, 8, 9, generator=gen).double(), torch.randn(2, 16, 5, generator=gen).double()
    slopes = oattn.alibi_slopes(2)
    ones = attention_factor(1, 2, 0.0, 2, 2, 9, 5)
    assert float(ones.min()) == 1.0 and torch.equal(drop_core(q, kv, slopes, 2, 4, 2.0, ones), cross_core(q, kv, slopes, 2, 4, 2.0))
    f = elementwise_factor(5, 1, 0.5, (2, 3, 4))
    assert f.shape == (2, 3, 4) and set(f.unique().tolist()) == {0.0, 2.0}
    assert torch.equal(f.reshape(-1) != 0, torch.from_numpy(philox.elementwise_keep(5, 1, 0.5, 24)))


def test_seeds_come_from_the_default_generator():
    torch.manual_seed(1234)
    a = [ops.draw_dropout_seed() for _ in range(3)]
    torch.manual_seed(1234)
    assert [ops.draw_dropout_seed() for _ in range(3)] == a
    assert len(set(a)) == 3 and all(0 <= s < 2 ** 64 for s in a)


def test_dropout_kernel_name_answers_from_the_pick(lib):
    for dh, dvt in ((8, 1), (32, 1), (33, 2), (64, 2), (65, 4), (128, 4)):
        assert ops.attention_dropout_kernel_name(2, 4, dh, 130, 70, 0.1) == f"attention_drop<{dvt}>"
        assert ops.attention_dropout_kernel_name(2, 4, dh, 130, 70, 0.0) == f"attention_drop<{dvt}>"
        assert ops.attention_dropout_kernel_name(2, 4, dh, 130, 70, 0.5, backward=True) == \
            "attn_drop_bwd_stats+attn_drop_bwd_dq+attn_drop_bwd_dkv"
    for empty in ((0, 4, 64, 10, 10), (2, 0, 64, 10, 10), (2, 4, 64, 0, 10), (2, 4, 64, 10, 0)):
        assert ops.attention_dropout_kernel_name(*empty, 0.1) == "none"
        assert ops.attention_dropout_kernel_name(*empty, 0.1, backward=True) == "none"
    buf = __import__("ctypes").create_string_buffer(96)
    assert lib.agx_attention_dropout_kernel_name(2, 4, 129, 10, 10, 0.1, 0, buf, len(buf)) == -5
    assert b"head_dim=129 > 128" in lib.agx_last_error()
    assert lib.agx_attention_dropout_kernel_name(2, 4, 0, 10, 10, 0.1, 0, buf, len(buf)) == -1
    for p in (1.0, -0.25, 1.5, float("nan")):
        assert lib.agx_attention_dropout_kernel_name(2, 4, 64, 10, 10, p, 0, buf, len(buf)) == -1
        assert b"not in [0, 1)" in lib.agx_last_error()
    with pytest.raises(AgxError, match=r"not in \[0, 1\)"):
        ops.attention_dropout_kernel_name(2, 4, 64, 10, 10, 1.0)
    assert lib.agx_attention_dropout_backward_workspace_bytes(2, 3, 37) == 2 * 2 * 3 * 37 * 4
    assert lib.agx_attention_dropout_backward_workspace_bytes(0, 3, 37) == 0
    # host-side refusals of the entry points come before any launch (and before the NULL-pointer check)
    assert lib.agx_dropout_add(None, None, None, 16, 1.0, 0, 0, None) == -1
    assert lib.agx_dropout_add(None, None, None, 0, 0.5, 0, 0, None) == 0
    assert lib.agx_dropout_add(None, None, None, 16, 0.5, 0, 0, None) == -2
    assert lib.agx_attention_alibi_dropout(None, None, 0, 0, None, None, 2, 4, 64, 10, 10, 8.0, 1.0, 0, 0, None) == -1
    assert lib.agx_attention_alibi_dropout(None, None, 0, 0, None, None, 0, 4, 64, 10, 10, 8.0, 0.5, 0, 0, None) == 0
    assert lib.agx_attention_alibi_dropout(None, None, 0, 0, None, None, 2, 4, 64, 10, 10, 8.0, 0.5, 0, 0, None) == -2
    assert lib.agx_version() == 122
