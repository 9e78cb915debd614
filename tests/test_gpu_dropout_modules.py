"""``Transformer`` / ``Attention`` / ``FeedForward`` with ``dropout > 0`` on the GPU: the training-mode walk (forward and native
backward) against the float64 restatement of ``tests/dropout_ref.py``, which applies the four masks per layer from
``last_dropout_seed`` and the stream ids; eval mode and ``dropout = 0`` against the walk without dropout, bit for bit and launch
for launch; the refusals.  Tolerances are the block tolerances of tests/test_gpu_cross_attention.py: output 1e-4, input
gradients 2e-4 max(1, .), parameter gradients 5e-4 max(1, .)."""
import pytest
import torch

from audio_generation_amd import ops
from audio_generation_amd._lib import AgxError
from audio_generation_amd.transformers import Attention, FeedForward, Transformer
from audio_generation_amd.vae import CausalResidualBlock1d
from oracle import attention as oattn
from tests.dropout_ref import dropout_transformer
from tests.helpers import max_abs

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIM, DEPTH, HEADS, DH, P = 64, 2, 2, 32, 0.25
B, TX, TY = 2, 40, 19
BUILDS = {"self": None, "cross": 24}      # context_y


def _model(context_y, dropout=P, seed=31):
    sd = oattn.init_state_dict(DIM, HEADS, DH, depth=DEPTH, seed=seed)
    tf = Transformer(DIM, DEPTH, heads=HEADS, head_dim=DH, dropout=dropout, context_x=48, context_y=context_y)
    tf.load_state_dict(sd)
    return tf.to(DEV), sd


def _data(context_y):
    gen = torch.Generator().manual_seed(77)
    x, w = torch.randn(B, DIM, TX, generator=gen), torch.randn(B, DIM, TX, generator=gen)
    y = torch.randn(B, DIM, TY, generator=gen) if context_y is not None else None
    return x, y, w


def _step(tf, x, y, w, manual_seed):
    """One training step on the device: (output, dx, dy, parameter gradients, the seed the forward drew)."""
    tf.zero_grad()
    xd = x.to(DEV).requires_grad_()
    yd = None if y is None else y.to(DEV).requires_grad_()
    torch.manual_seed(manual_seed)
    out = tf.run_bct(xd, yd)
    (out * w.to(DEV)).sum().backward()
    grads = {n: p.grad.clone() for n, p in tf.named_parameters()}
    return out.detach(), xd.grad, None if yd is None else yd.grad, grads, tf.last_dropout_seed


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_training_with_dropout_against_the_float64_restatement(build):
    context_y = BUILDS[build]
    tf, sd = _model(context_y)
    tf.train()
    x, y, w = _data(context_y)
    out, dx, dy, grads, seed = _step(tf, x, y, w, manual_seed=5)
    assert isinstance(seed, int) and 0 <= seed < 2 ** 64
    # the float64 restatement with the masks of (seed, stream ids) as constants
    sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    x64 = x.double().requires_grad_()
    y64 = None if y is None else y.double().requires_grad_()
    want = dropout_transformer(x64, y64, sd64, HEADS, DEPTH, P, seed)
    (want * w.double()).sum().backward()
    err = max_abs(out.cpu(), want.detach())
    print(f"dropout training ({build}): output err {err:.3e}")
    assert err < 1e-4
    pairs = [("dx", dx, x64.grad, 2e-4)] + ([("dy", dy, y64.grad, 2e-4)] if y is not None else [])
    assert list(grads) == list(sd)
    pairs += [(n, grads[n], sd64[n].grad, 5e-4) for n in grads]
    for name, got, ref, tol in pairs:
        assert got is not None, name
        e, scale = max_abs(got.cpu(), ref), float(ref.abs().max())
        print(f"dropout training ({build}) {name}: err {e:.3e}, max|ref| {scale:.3e}")
        assert e < tol * max(1.0, scale), name
    if y is not None:
        assert float(dy.abs().max()) > 0.0                               # y.grad flows
    # the masks did something: the same weights without dropout give another output
    with torch.no_grad():
        plain = tf.eval().run_bct(x.to(DEV), None if y is None else y.to(DEV))
    assert max_abs(plain, out) > 1e-2
    tf.train()
    # the same manual_seed: the same seed, bit-identical outputs and gradients; another one: another mask
    out2, dx2, dy2, grads2, seed2 = _step(tf, x, y, w, manual_seed=5)
    assert seed2 == seed and torch.equal(out2, out) and torch.equal(dx2, dx)
    assert y is None or torch.equal(dy2, dy)
    assert all(torch.equal(grads2[n], grads[n]) for n in grads)
    out3, _, _, _, seed3 = _step(tf, x, y, w, manual_seed=6)
    assert seed3 != seed and not torch.equal(out3, out)
    # grad mode plays no part: under no_grad a training-mode forward drops with the seed it draws
    torch.manual_seed(5)
    with torch.no_grad():
        out4 = tf.run_bct(x.to(DEV), None if y is None else y.to(DEV))
    assert tf.last_dropout_seed == seed and torch.equal(out4, out)


class _Trace:
    """Launch observer (``ops.set_observer``): the kernel each C-ABI compute call of the walk runs."""

    def __init__(self):
        self.names = []

    def begin(self, kind, info):
        if kind == "conv":
            self.names.append(f"{ops.conv_kernel_name(info)} {info.c_in}->{info.c_out} epi={info.epilogue}")
        else:
            self.names.append(info[0])
        return len(self.names)

    def end(self, token):
        pass


def _traced(tf, x, y):
    trace = _Trace()
    ops.set_observer(trace)
    try:
        with torch.no_grad():
            out = tf.run_bct(x, y)
    finally:
        ops.set_observer(None)
    return out, trace.names


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_eval_mode_and_p_zero_are_the_walk_without_dropout(build):
    context_y = BUILDS[build]
    dropped, _ = _model(context_y, dropout=P)
    plain, _ = _model(context_y, dropout=0.0)
    x, y, _ = _data(context_y)
    x, y = x.to(DEV), None if y is None else y.to(DEV)
    want, want_names = _traced(plain.eval(), x, y)
    per_layer = [8, 7] if context_y is not None else [7, 7]              # the cross layer: a Q and a KV projection
    assert len(want_names) == sum(per_layer)
    torch.manual_seed(3)
    state = torch.get_rng_state()
    got, names = _traced(dropped.eval(), x, y)
    assert torch.equal(got, want) and names == want_names
    assert dropped.last_dropout_seed is None and torch.equal(torch.get_rng_state(), state)     # no seed was drawn
    got, names = _traced(plain.train(), x, y)                            # training mode with dropout = 0
    assert torch.equal(got, want) and names == want_names and plain.last_dropout_seed is None
    # training mode with dropout: 10 launches per layer (11 for the cross layer), the dropout kernels among them
    _, names = _traced(dropped.train(), x, y)
    assert len(names) == sum(n + 3 for n in per_layer), names
    assert names.count("attention_alibi_dropout:flash") == DEPTH and names.count("dropout_add") == 3 * DEPTH
    assert not any(n.startswith("attention_alibi_cross") or n == "attention_alibi" for n in names)
    # the eval-mode native backward is the one without dropout too
    grads = []
    for tf in (dropped.eval(), plain.eval()):
        xg = x.clone().requires_grad_()
        tf.run_bct(xg, y).sum().backward()
        grads.append(xg.grad)
    assert torch.equal(grads[0], grads[1])


def test_sub_blocks_on_their_own_draw_their_own_seed():
    sd = oattn.init_state_dict(DIM, HEADS, DH, depth=1, seed=8)
    att = Attention(DIM, dim_head=DH, n_heads=HEADS, dropout=P, context_x=48)
    att.load_state_dict({k[len("layers.0.0."):]: v for k, v in sd.items() if k.startswith("layers.0.0.")})
    ff = FeedForward(DIM, DIM, dropout=P)
    ff.load_state_dict({k[len("layers.0.1."):]: v for k, v in sd.items() if k.startswith("layers.0.1.")})
    x = torch.randn(B, TX, DIM, generator=torch.Generator().manual_seed(4)).to(DEV)
    for mod in (att.to(DEV), ff.to(DEV)):
        mod.train()
        torch.manual_seed(11)
        with torch.no_grad():
            a = mod(x)
        seed = mod.last_dropout_seed
        torch.manual_seed(11)
        with torch.no_grad():
            b = mod(x)
        assert isinstance(seed, int) and mod.last_dropout_seed == seed and torch.equal(a, b)
        with torch.no_grad():
            c, d = mod(x), mod.eval()(x)
        assert not torch.equal(a, c) and not torch.equal(a, d)
        frac = float((a == 0).float().mean())        # the output site drops a quarter of the elements
        assert abs(frac - P) < 4 * (P * (1 - P) / a.numel()) ** 0.5


def test_refusals_on_the_device():
    x = torch.zeros(B, DIM, TX, device=DEV)
    tf, _ = _model(None)
    tf.train()
    tf.layers[0][0].attention_dtype = "bf16"
    with pytest.raises(AgxError, match="attention with dropout runs in fp32"):
        tf.run_bct(x)
    with torch.no_grad():
        assert tuple(tf.eval().run_bct(x).shape) == (B, DIM, TX)         # bf16 inference of the same model runs
    one = Transformer(DIM, 1, heads=HEADS, head_dim=DH, dropout=1.0, context_x=48).to(DEV)
    with pytest.raises(AgxError, match="0 <= p < 1"):
        one.train().run_bct(x)
    with torch.no_grad():
        assert tuple(one.eval().run_bct(x).shape) == (B, DIM, TX)
    wide = Transformer(256, 1, heads=1, head_dim=129, dropout=0.1, context_x=48).to(DEV).train()
    with pytest.raises(AgxError, match="head_dim"):
        wide.run_bct(torch.zeros(1, 256, 8, device=DEV))
    # a conv-stack layer built with dropout: eval mode is the dropout = 0 block, bit for bit; training mode is refused
    torch.manual_seed(0)
    block = CausalResidualBlock1d(32, 32, dilation=3, dropout=0.1).to(DEV)
    plain = CausalResidualBlock1d(32, 32, dilation=3).to(DEV)
    plain.load_state_dict(block.state_dict())
    h = torch.randn(2, 32, 100, device=DEV)
    with torch.no_grad():
        assert torch.equal(block.eval()(h), plain.eval()(h))
        with pytest.raises(AgxError, match="in training mode has no kernel"):
            block.train()(h)
