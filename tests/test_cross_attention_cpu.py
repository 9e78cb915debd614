"""Cross-attention on the host (no kernel is launched): the modules construct with the reference's ``state_dict``, ``Alibi.M``
is the reference's array (g9: shape (H, context_y, context_x), the transposed one), the accepted-length rule is the union of
what the reference runs and the intended reading, the CPU checker of ``tests/cross_attention_ref.py`` reproduces the g9
outputs, and ``agx_attention_cross_kernel_name`` answers from the cross-attention pick of csrc/attention_cross.hip:
``attention_cross<DVT>`` with DVT = 1 / 2 / 4 for head_dim <= 32 / 64 / 128, refused beyond."""
import ctypes
import json
import os

import pytest
import torch

from audio_generation_amd import _lib, ops
from audio_generation_amd._lib import AgxError
from audio_generation_amd.transformers import Alibi, Attention, Transformer, TransformerBottleneck
from tests.cross_attention_ref import cross_attention, cross_transformer
from tests.helpers import GOLDEN, load_npz, max_abs, sub_sd

UNSUPPORTED, WORKSPACE, NULL_POINTER, BAD_SHAPE = -5, -3, -2, -1
BWD_NAME = "attn_cross_bwd_stats+attn_cross_bwd_dq+attn_cross_bwd_dkv"


@pytest.fixture(scope="module")
def lib():
    from audio_generation_amd import build
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def g9():
    return load_npz("g9_cross_attention.npz")


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLDEN, "meta_g9.json")) as f:
        return json.load(f)


def test_cross_modules_construct_with_the_references_state_dict(meta, g9):
    tf = Transformer(64, depth=1, heads=4, head_dim=16, context_x=48, context_y=32)
    assert tf.cross_attention and tf.layers[0][0].cross_attention
    assert list(tf.state_dict().keys()) == meta["state_dict_keys"]
    tf.load_state_dict(sub_sd(g9, "cx48_cy32/sd/"))            # strict: a reference checkpoint loads as is
    att = Attention(64, dim_head=16, n_heads=4, context_x=48, context_y=32)
    assert att.cross_attention and sorted(att.state_dict()) == sorted(k[len("layers.0.0."):] for k in meta["state_dict_keys"]
                                                                      if k.startswith("layers.0.0."))
    assert not Attention(64, dim_head=16, n_heads=4, context_x=48).cross_attention
    deep = Transformer(64, depth=3, heads=4, head_dim=16, context_x=48, context_y=32)
    assert [a.cross_attention for a, _ in deep.layers] == [True, False, False]     # transformers.py:272-273
    assert Transformer(64, depth=1, heads=4, head_dim=16, context_x=50, context_y=50).layers[0][0].cross_attention


def test_alibi_m_is_the_references_array(g9):
    for cx, cy in ((32, 48), (48, 32)):
        a = Alibi(cx, cy, 4)
        want = torch.from_numpy(g9[f"alibi_cx{cx}_cy{cy}_h4"])
        assert tuple(a.M.shape) == (4, cy, cx) and torch.equal(a.M, want)
        assert "M" not in a.state_dict() and "head_scalars" not in a.state_dict()
        assert tuple(a.get_M(crop=(5, 7)).shape) == (1, 4, 5, 7)
    g3 = load_npz("g3_attention.npz")
    assert torch.equal(Alibi(16, n_heads=8).get_M(), torch.from_numpy(g3["alibi_h8_t16"]))     # self-attention: unchanged


@pytest.mark.parametrize("tx,ty,ok", [(20, 30, True), (30, 20, True), (32, 32, True), (32, 48, True), (48, 32, True),
                                      (1, 1, True), (33, 33, False), (48, 33, False), (33, 48, False), (49, 1, False),
                                      (1, 49, False)])
def test_accepted_lengths_are_the_references_and_the_intended_reading(lib, tx, ty, ok):
    """contexts (48, 32): the reference runs Tx <= 32 and Ty <= 48 (its M is transposed); the intended reading is Tx <= 48
    and Ty <= 32.  Inside the union the shape check passes and the first op refuses the host tensors; outside it the layer
    refuses before anything else."""
    tf = Transformer(64, depth=1, heads=4, head_dim=16, context_x=48, context_y=32)
    x, y = torch.zeros(2, tx, 64), torch.zeros(2, ty, 64)
    with torch.no_grad(), pytest.raises(AgxError, match="MI355X only" if ok else
                                        rf"sequence lengths \({tx}, {ty}\) exceed the ALiBi contexts \(48, 32\) in both orders"):
        tf(x, y)
    with torch.no_grad(), pytest.raises(AgxError, match="MI355X only" if ok else "exceed the ALiBi contexts"):
        tf.layers[0][0](x, y)


def test_refusals_that_need_no_gpu(lib):
    tf = Transformer(64, depth=1, heads=4, head_dim=16, context_x=48, context_y=32)
    x, y = torch.zeros(2, 20, 64), torch.zeros(2, 30, 64)
    with torch.no_grad():
        with pytest.raises(AgxError, match="Cross attention requires two inputs"):
            tf(x)
        with pytest.raises(AgxError, match="Cross attention requires two inputs"):
            tf.layers[0][0](x)
        with pytest.raises(AgxError, match=r"cross-attention: y is \(2, 30, 64\), expected \(2, 64, Ty\)"):
            tf.run_bct(x.transpose(1, 2), y)                   # y in the wrong layout: the shape check precedes the length rule
        with pytest.raises(AgxError, match="takes no second sequence y"):
            Transformer(64, depth=1, heads=4, head_dim=16, context_x=48)(x, y)
        with pytest.raises(AgxError, match="carries no second sequence y"):
            TransformerBottleneck(tf)(x)
        tf.layers[0][0].attention_dtype = "bf16"
        with pytest.raises(AgxError, match="cross-attention runs in fp32"):
            tf(x, y)


def test_the_channel_count_check_of_the_wrappers():
    """``ops._attn_operands``: what ``attention_alibi_cross`` and ``attention_alibi_cross_backward`` call before anything else;
    its first three answers are (b, tq, tk)."""
    z = torch.zeros
    assert ops._attn_operands("op", z(2, 64, 4), z(2, 128, 5), 4, 16)[:3] == (2, 4, 5)
    with pytest.raises(AgxError, match=r"op: q has 60 channels, expected 64"):
        ops._attn_operands("op", z(1, 60, 4), z(1, 128, 5), 4, 16)
    with pytest.raises(AgxError, match=r"op: kv has 128 channels, expected 96"):
        ops._attn_operands("op", z(1, 48, 4), z(1, 128, 5), 3, 16)
    with pytest.raises(AgxError, match=r"op: q has batch 1, kv has batch 2"):
        ops._attn_operands("op", z(1, 64, 4), z(2, 128, 5), 4, 16)


def test_the_checker_reproduces_the_reference(g9, meta):
    """1e-6: what the oracle's other halves meet against their goldens (tests/test_oracle_golden.py)."""
    for name, m in meta["models"].items():
        sd = sub_sd(g9, f"{name}/sd/")
        for case, tx, ty in m["cases"]:
            x, y = (torch.from_numpy(g9[f"{name}/{case}/{k}"]) for k in ("x", "y"))
            assert tuple(x.shape) == (2, tx, 64) and tuple(y.shape) == (2, ty, 64)
            assert max_abs(cross_attention(x, y, sd, "layers.0.0.", 4), g9[f"{name}/{case}/attn"]) < 1e-6, (name, case)
            assert max_abs(cross_transformer(x, y, sd, 4), g9[f"{name}/{case}/out"]) < 1e-6, (name, case)
    # y matters, and it is not normalised: a checker that took LN(y) or ignored y would not pass the line above
    sd = sub_sd(g9, "cx48_cy32/sd/")
    x, y = (torch.from_numpy(g9[f"cx48_cy32/t20_30/{k}"]) for k in ("x", "y"))
    assert max_abs(cross_attention(x, 2.0 * y, sd, "layers.0.0.", 4), g9["cx48_cy32/t20_30/attn"]) > 1e-3


@pytest.mark.parametrize("shape,dvt", [((1, 2, 8, 1, 1), 1), ((2, 8, 64, 130, 65), 2), ((1, 2, 128, 33, 257), 4),
                                       ((1, 2, 32, 5, 5), 1), ((1, 2, 33, 5, 5), 2), ((1, 2, 65, 5, 5), 4)])
def test_cross_kernel_names(lib, shape, dvt):
    assert ops.attention_cross_kernel_name(*shape) == f"attention_cross<{dvt}>"
    assert ops.attention_cross_kernel_name(*shape, backward=True) == BWD_NAME


def test_the_cross_query_refuses_what_the_launchers_refuse(lib):
    buf = ctypes.create_string_buffer(96)
    for backward, op in ((0, "attention_alibi_cross"), (1, "attention_alibi_cross_backward")):
        assert lib.agx_attention_cross_kernel_name(1, 2, 129, 33, 257, backward, buf, len(buf)) == UNSUPPORTED
        assert lib.agx_last_error().decode() == f"{op}: head_dim=129 > 128"
        assert lib.agx_attention_cross_kernel_name(1, 2, 0, 33, 257, backward, buf, len(buf)) == BAD_SHAPE
        assert lib.agx_attention_cross_kernel_name(1, 65536, 64, 33, 257, backward, buf, len(buf)) == BAD_SHAPE
        assert lib.agx_last_error().decode() == f"{op}: grid too large"
    with pytest.raises(AgxError, match=r"agx_attention_cross_kernel_name failed \(-5\): attention_alibi_cross: head_dim=129 > 128"):
        ops.attention_cross_kernel_name(1, 2, 129, 4, 4)
    # the launchers, with pointers they never follow: the same answers, and the workspace check
    assert lib.agx_attention_alibi_cross(buf, buf, buf, buf, 1, 2, 129, 4, 4, 8.0, None) == UNSUPPORTED
    assert lib.agx_attention_alibi_cross_backward(buf, buf, buf, buf, buf, buf, buf, buf, 1 << 20, 1, 2, 129, 4, 4, 8.0, None) == UNSUPPORTED
    assert lib.agx_last_error().decode() == "attention_alibi_cross_backward: head_dim=129 > 128"
    assert lib.agx_attention_cross_backward_workspace_bytes(2, 3, 37) == 2 * 2 * 3 * 37 * 4
    assert lib.agx_attention_cross_backward_workspace_bytes(2, 3, 0) == 0
    assert lib.agx_attention_alibi_cross_backward(buf, buf, buf, buf, buf, buf, buf, buf, 2 * 2 * 3 * 37 * 4 - 1, 2, 3, 16, 37, 50, 4.0,
                                                  None) == WORKSPACE
    assert lib.agx_last_error().decode() == "attention_alibi_cross_backward: workspace too small"
    assert lib.agx_attention_alibi_cross(None, buf, buf, buf, 1, 2, 64, 4, 4, 8.0, None) == NULL_POINTER
    assert lib.agx_attention_alibi_cross_backward(buf, buf, buf, buf, buf, None, buf, buf, 1 << 20, 1, 2, 64, 4, 4, 8.0, None) == NULL_POINTER
    # empty shapes: AGX_OK, nothing is launched (no pointer is followed, NULL included)
    for b, h, tq, tk in ((0, 2, 4, 4), (1, 0, 4, 4), (1, 2, 0, 4), (1, 2, 4, 0), (-1, 2, 4, 4)):
        assert lib.agx_attention_alibi_cross(None, None, None, None, b, h, 64, tq, tk, 8.0, None) == 0
        assert lib.agx_attention_alibi_cross_backward(None, None, None, None, None, None, None, None, 0, b, h, 64, tq, tk, 8.0, None) == 0
        assert lib.agx_attention_cross_kernel_name(b, h, 64, tq, tk, 0, buf, len(buf)) == 0 and buf.value == b"none"


def test_a_short_buffer_truncates_and_no_buffer_is_an_error(lib):
    buf = ctypes.create_string_buffer(b"x" * 32, 32)
    assert lib.agx_attention_cross_kernel_name(1, 2, 64, 5, 7, 0, buf, 10) == 0 and buf.value == b"attention"
    assert lib.agx_attention_cross_kernel_name(1, 2, 64, 5, 7, 1, buf, 11) == 0 and buf.value == b"attn_cross"
    assert lib.agx_attention_cross_kernel_name(1, 2, 64, 5, 7, 0, None, 10) == NULL_POINTER
    assert lib.agx_attention_cross_kernel_name(1, 2, 64, 5, 7, 1, buf, 0) == NULL_POINTER
    assert lib.agx_last_error().decode() == "agx_attention_cross_kernel_name: NULL buffer"


def test_the_abi_only_grew(lib):
    assert lib.agx_version() == 122
    for name in ("agx_attention_alibi_cross", "agx_attention_alibi_cross_backward", "agx_attention_cross_backward_workspace_bytes",
                 "agx_attention_cross_kernel_name"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
