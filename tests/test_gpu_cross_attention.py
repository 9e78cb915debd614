"""ALiBi cross-attention on the GPU (csrc/attention_cross.hip): the op against the float64 definition, forward and backward,
and the drop-in modules against the reference's own outputs (g9) and the CPU checker of ``tests/cross_attention_ref.py``.

Tolerances are the ones the suite states for the same arithmetic: 3e-5 of max(1, max|o|) for the fp32 flash forward
(tests/test_gpu_attention_flash.py), 5e-5 / 1e-5 (max / rms) for the split backward, 1e-5 / 2e-5 for the attention sub-block
and the block against the goldens (tests/test_gpu_blocks.py), 2e-4 / 5e-4 for input / parameter gradients of a block
(tests/test_gpu_training.py)."""
import ctypes

import pytest
import torch

from audio_generation_amd import _lib, ops
from audio_generation_amd._lib import AgxError
from audio_generation_amd.transformers import Attention, Transformer, TransformerBottleneck
from oracle import attention as oattn
from tests.cross_attention_ref import cross_core, cross_transformer
from tests.helpers import load_npz, max_abs, rms, sub_sd

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _inputs(b, heads, dh, tq, tk):
    gen = torch.Generator().manual_seed(1000 * tq + 10 * tk + dh)
    q = 0.7 * torch.randn(b, heads * dh, tq, generator=gen)
    kv = 0.7 * torch.randn(b, 2 * heads * dh, tk, generator=gen)
    dout = torch.randn(b, heads * dh, tq, generator=gen)
    return q, kv, dout, oattn.alibi_slopes(heads)


@pytest.mark.parametrize("b,heads,dh,tq,tk", [(2, 1, 8, 1, 1), (2, 3, 16, 5, 1), (1, 2, 64, 1, 70), (2, 4, 16, 37, 50),
                                              (2, 8, 64, 130, 65), (2, 2, 100, 65, 130), (1, 2, 128, 33, 257),
                                              (1, 8, 64, 300, 64), (1, 2, 32, 513, 300)])
def test_cross_forward_against_the_definition(b, heads, dh, tq, tk):
    q, kv, _, slopes = _inputs(b, heads, dh, tq, tk)
    want = cross_core(q.double(), kv.double(), slopes, heads, dh, dh ** 0.5)
    got = ops.attention_alibi_cross(q.to(DEV), kv.to(DEV), slopes.to(DEV), heads, dh, dh ** 0.5)
    assert tuple(got.shape) == (b, heads * dh, tq)
    err, scale = max_abs(got.cpu(), want), float(want.abs().max())
    print(f"cross forward {(b, heads, dh, tq, tk)}: max err {err:.3e}, max|o| {scale:.3e}")
    assert err < 3e-5 * max(1.0, scale)


def test_cross_equals_self_attention_on_the_concatenated_tensor():
    b, heads, dh, t = 2, 5, 33, 64
    q, kv, _, slopes = _inputs(b, heads, dh, t, t)
    one = ops.attention_alibi(torch.cat([q, kv], dim=1).to(DEV), slopes.to(DEV), heads, dh, dh ** 0.5, flash=True)
    got = ops.attention_alibi_cross(q.to(DEV), kv.to(DEV), slopes.to(DEV), heads, dh, dh ** 0.5)
    assert max_abs(got, one) < 3e-5 * max(1.0, float(one.abs().max()))


@pytest.mark.parametrize("b,heads,dh,tq,tk", [(2, 8, 64, 130, 65), (1, 4, 16, 257, 40), (2, 3, 20, 37, 300), (1, 2, 128, 200, 33),
                                              (1, 2, 100, 65, 513), (1, 1, 8, 1, 1), (2, 2, 64, 1, 70), (2, 2, 64, 70, 1),
                                              (1, 5, 33, 64, 64)])
def test_cross_backward_against_float64_autograd(b, heads, dh, tq, tk):
    q, kv, dout, slopes = _inputs(b, heads, dh, tq, tk)
    q64, kv64 = q.double().requires_grad_(), kv.double().requires_grad_()
    cross_core(q64, kv64, slopes, heads, dh, dh ** 0.5).backward(dout.double())
    qd, kvd, sd, dd = q.to(DEV), kv.to(DEV), slopes.to(DEV), dout.to(DEV)
    out = ops.attention_alibi_cross(qd, kvd, sd, heads, dh, dh ** 0.5)
    dq, dkv = ops.attention_alibi_cross_backward(qd, kvd, sd, out, dd, heads, dh, dh ** 0.5)
    assert dq.shape == q.shape and dkv.shape == kv.shape
    for name, got, want in (("dq", dq, q64.grad), ("dkv", dkv, kv64.grad)):
        e_max, e_rms = max_abs(got.cpu(), want), rms(got.cpu(), want)
        s_max, s_rms = float(want.abs().max()), float(want.pow(2).mean().sqrt())
        print(f"cross backward {(b, heads, dh, tq, tk)} {name}: max err {e_max:.3e} (max {s_max:.3e}), rms err {e_rms:.3e} (rms {s_rms:.3e})")
        assert e_max < 5e-5 * max(1.0, s_max) and e_rms < 1e-5 * max(1.0, s_rms), name
    dq2, dkv2 = ops.attention_alibi_cross_backward(qd, kvd, sd, out, dd, heads, dh, dh ** 0.5)
    assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2)          # deterministic: no atomics


def test_cross_backward_refusals():
    lib = _lib.load()
    b, heads, dh, tq, tk = 1, 2, 16, 37, 50
    q, kv, dout, slopes = (t.to(DEV) for t in _inputs(b, heads, dh, tq, tk))
    out = ops.attention_alibi_cross(q, kv, slopes, heads, dh, 4.0)
    dq, dkv = torch.zeros_like(q), torch.zeros_like(kv)
    need = lib.agx_attention_cross_backward_workspace_bytes(b, heads, tq)
    assert need == 2 * b * heads * tq * 4
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    args = (p(q), p(kv), p(slopes), p(out), p(dout), p(dq), p(dkv), p(ws))
    assert lib.agx_attention_alibi_cross_backward(*args, need - 4, b, heads, dh, tq, tk, 4.0, None) == -3
    assert lib.agx_attention_alibi_cross_backward(*args, need, b, heads, 129, tq, tk, 4.0, None) == -5
    assert lib.agx_attention_alibi_cross(p(q), p(kv), p(slopes), p(out), b, heads, 129, tq, tk, 4.0, None) == -5
    torch.cuda.synchronize()
    assert float(dq.abs().max()) == 0.0 and float(dkv.abs().max()) == 0.0 and int(ws.max()) == 0     # nothing was launched


# ------------------------------------------------------------------------------------------------- modules
G9_MODELS = {"square50": (50, 50, ("full", "crop")), "cx48_cy32": (48, 32, ("t20_30", "t30_20", "t32_32", "t32_48"))}


@pytest.fixture(scope="module")
def g9():
    return load_npz("g9_cross_attention.npz")


@pytest.mark.parametrize("name", sorted(G9_MODELS))
def test_modules_reproduce_the_reference(name, g9):
    cx, cy, cases = G9_MODELS[name]
    tf = Transformer(64, depth=1, heads=4, head_dim=16, context_x=cx, context_y=cy)
    tf.load_state_dict(sub_sd(g9, f"{name}/sd/"))
    tf = tf.to(DEV).eval()
    att = Attention(64, dim_head=16, n_heads=4, context_x=cx, context_y=cy)
    att.load_state_dict(sub_sd(g9, f"{name}/sd/layers.0.0."))
    att = att.to(DEV).eval()
    for case in cases:
        x, y = (torch.from_numpy(g9[f"{name}/{case}/{k}"]).to(DEV) for k in ("x", "y"))
        with torch.no_grad():
            sub, out = att(x, y), tf(x, y)
            out_bct = tf.run_bct(x.transpose(1, 2).contiguous(), y.transpose(1, 2).contiguous())
            sub_bct = att.run_bct(x.transpose(1, 2).contiguous(), y=y.transpose(1, 2).contiguous())
        e_sub, e_out = max_abs(sub.cpu(), g9[f"{name}/{case}/attn"]), max_abs(out.cpu(), g9[f"{name}/{case}/out"])
        print(f"g9 {name}/{case}: sub-block err {e_sub:.3e}, block err {e_out:.3e}")
        assert e_sub < 1e-5 and e_out < 2e-5, (name, case)
        assert torch.equal(out, out_bct.transpose(1, 2)) and torch.equal(sub, sub_bct.transpose(1, 2))


def test_training_block_with_a_differentiable_second_sequence():
    """depth 2: layer 0 cross-attends to y, layer 1 is ALiBi self-attention; gradients reach x, y and every parameter."""
    dim, heads, dh = 64, 4, 32
    sd = oattn.init_state_dict(dim, heads, dh, depth=2, seed=91)
    tf = Transformer(dim, depth=2, heads=heads, head_dim=dh, context_x=80, context_y=120)
    tf.load_state_dict(sd)
    tf = tf.to(DEV).train()
    gen = torch.Generator().manual_seed(92)
    x, y, w = torch.randn(2, dim, 70, generator=gen), torch.randn(2, dim, 110, generator=gen), torch.randn(2, dim, 70, generator=gen)
    # the CPU checker in float64, reference layout
    sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    x64, y64 = x.double().requires_grad_(), y.double().requires_grad_()
    want = cross_transformer(x64.transpose(1, 2), y64.transpose(1, 2), sd64, heads, depth=2).transpose(1, 2)
    (want * w.double()).sum().backward()
    xd, yd = x.to(DEV).requires_grad_(), y.to(DEV).requires_grad_()
    out = tf.run_bct(xd, yd)
    (out * w.to(DEV)).sum().backward()
    assert max_abs(out.detach().cpu(), want.detach()) < 1e-4
    for name, got, ref, tol in (("dx", xd.grad, x64.grad, 2e-4), ("dy", yd.grad, y64.grad, 2e-4)):
        err, scale = max_abs(got.cpu(), ref), float(ref.abs().max())
        print(f"cross training {name}: err {err:.3e}, max|ref| {scale:.3e}")
        assert err < tol * max(1.0, scale), name
    params = dict(tf.named_parameters())
    assert list(params) == list(sd)
    for name, p in params.items():
        assert p.grad is not None, name
        ref = sd64[name].grad
        err, scale = max_abs(p.grad.cpu(), ref), float(ref.abs().max())
        print(f"cross training {name}: err {err:.3e}, max|ref| {scale:.3e}")
        assert err < 5e-4 * max(1.0, scale), name
    for name in ("layers.0.0.W_k.weight", "layers.0.0.W_v.weight"):
        assert float(params[name].grad.abs().max()) > 0.0
    # a frozen second sequence: no gradient for y (its backward-data conv is skipped), the same dx
    x3 = x.to(DEV).requires_grad_()
    (tf.run_bct(x3, y.to(DEV)) * w.to(DEV)).sum().backward()
    assert torch.equal(x3.grad, xd.grad)
    # y alone asking for a gradient takes the native backward too
    tf.requires_grad_(False)
    y2 = y.to(DEV).requires_grad_()
    (tf.run_bct(x.to(DEV), y2) * w.to(DEV)).sum().backward()
    assert max_abs(y2.grad.cpu(), y64.grad) < 2e-4 * max(1.0, float(y64.grad.abs().max()))


def test_cross_refusals_on_the_gpu():
    tf = Transformer(64, depth=1, heads=4, head_dim=16, context_x=48, context_y=32).to(DEV).eval()
    x, y = torch.zeros(2, 20, 64, device=DEV), torch.zeros(2, 30, 64, device=DEV)
    with torch.no_grad():
        with pytest.raises(AgxError, match="carries no second sequence y"):
            TransformerBottleneck(tf)(x)
        with pytest.raises(AgxError, match="Cross attention requires two inputs"):
            tf(x)
        with pytest.raises(AgxError, match="Cross attention requires two inputs"):
            tf.layers[0][0](x)
        with pytest.raises(AgxError, match="exceed the ALiBi contexts"):
            tf(torch.zeros(2, 33, 64, device=DEV), torch.zeros(2, 33, 64, device=DEV))
        assert tuple(tf(x, y).shape) == (2, 20, 64)
        tf.layers[0][0].attention_dtype = "bf16"
        with pytest.raises(AgxError, match="cross-attention runs in fp32"):
            tf(x, y)
