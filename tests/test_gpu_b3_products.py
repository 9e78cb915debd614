"""Every bf16x3 code path against the two instruments of tests/b3_probe.py: the exact piece-product probe (each output one
product of two operands with known non-zero pieces; |y - want64| <= 2^-22 |want64|, exact zeros where the reference has no
product) under four rotations of the hot (channel, tap) assignment, and the term projection on dense random data
(|c_ij| <= 0.1 for the six issued piece pairs, per 32 output rows).  All expected values are float64 references
(oracle/codec.py, torch conv2d on the CPU); the kernel name of every case is asserted through the host-only name queries.

Paths: the conv_b3 ring (fp32 input, plane input, plane output), conv_mfma:bf16x3 (the k9 s3 layer and every bf16x3 row of
tests/test_gpu_tile_variants.py), resblock_b3 and resblock_mfma:bf16x3, the Conv2d ring forward and backward-data (3 x 3,
the space-to-depth layers, the q == 2 plans with and without the peeled first column, the patch-tile fallback), and the
weight gradients whose contraction is bf16x3 (projection only: tests/test_gpu_weight_grad_training_size.py pins exactness).
tests/test_b3_probe_cpu.py shows on an emulation that a lost, doubled or partly lost term fails both instruments."""
import pytest
import torch

from audio_generation_amd import _lib, ops
from tests import b3_probe as P
from tests import test_gpu_tile_variants as TV
from tests.helpers import max_abs

pytestmark = pytest.mark.gpu
DEV = "cuda"
B3 = _lib.IMPL_MFMA_BF16X3
KIND = {"convt": _lib.CONV_TRANSPOSED, "upconv": _lib.CONV_UPSAMPLE, "causal": _lib.CONV_CAUSAL}


def _probe(y, want, what):
    worst = P.assert_probe(y, want, what)
    print(f"probe {what}: {worst:.3f} x 2^-22")


# ------------------------------------------------------------------------------------------------ 1-D convs
class Conv1d:
    """One bf16x3 layer: descriptor, asserted kernel name, forward from fp32 or plane input."""

    def __init__(self, kind, cin, cout, k, s, d, batch, length, name, exact_name=False):
        self.kind, self.shape = kind, (cin, cout, k, s, d)
        self.desc = ops.conv_desc(KIND[kind], batch, cin, cout, length, k, s, d, 0, 0.1, B3)
        got = ops.conv_kernel_name(self.desc)
        assert (got == name) if exact_name else (got.startswith(name) and got.endswith(":bf16x3")), (got, name)
        self.op = P.conv1d_op(kind, s, d)
        self.zero_bias = torch.zeros(cout, device=DEV)

    def forward(self, w, x, bias=None, planes=False, out_planes=False):
        packed = ops.conv_pack(self.desc, w.to(DEV))                 # no weight norm: the kernel splits w itself
        bias = self.zero_bias if bias is None else bias.to(DEV)
        if not planes:
            return ops.conv_forward(self.desc, x.to(DEV), packed, bias)
        y = ops.conv_forward_planes(self.desc, ops.planes_split(x.to(DEV)), packed, bias, out_planes=out_planes)
        return ops.planes_join(y) if out_planes else y

    def check(self, batch, length, what, feeds=((False, False),)):
        cin, cout, k, s, d = self.shape
        x = P.rich_activation((batch, cin, length), 31 * cin + length)
        for rot in range(P.ROTATIONS):
            w, _ = P.probe_weight_1d(self.kind, cin, cout, k, s, rot)
            want = self.op(w.double(), x.double())
            for planes, out_planes in feeds:
                _probe(self.forward(w, x, None, planes, out_planes), want, f"{what} rot {rot} planes {int(planes)}{int(out_planes)}")
        x, w, bias = P.dense_layer_1d(self.kind, cin, cout, k, batch, length, 7 * cin + length)
        want = self.op(w.double(), x.double(), bias.double())
        terms = P.term_tensors(*P.kernel_form(self.kind, s, d, w), x)       # (an upsampling layer splits its folded weights)
        for planes, out_planes in feeds:
            c = P.projection(self.forward(w, x, bias, planes, out_planes), want, terms)
            P.assert_projection(c, f"{what} planes {int(planes)}{int(out_planes)}")


@pytest.mark.parametrize("row,lengths", P.RING, ids=P.RING_IDS)
def test_conv_b3_ring(row, lengths):
    variant, kind, cin, cout, k, s = row
    for batch, length in lengths:
        layer = Conv1d(kind, cin, cout, k, s, 1, batch, length, f"conv_b3<{variant},")
        can = ops.conv_planes_supported(layer.desc)
        assert can == {"upconv": 1, "convt": 2, "causal": 0}[kind]
        feeds = [(False, False)] + [(True, False)] * (can >= 1) + [(True, True)] * (can == 2)
        layer.check(batch, length, f"conv_b3<{variant}> {cin}->{cout} {batch}x{length}", feeds)


def test_conv_mfma_k9_s3():
    kind, cin, cout, k, s, batch, length = P.MFMA_K9S3
    Conv1d(kind, cin, cout, k, s, 1, batch, length, "conv_mfma<").check(batch, length, "conv_mfma k9 s3")


TILE_CONV = [r for r in TV.ROWS if r[0] == "conv" and r[-1].endswith(":bf16x3")]
TILE_RB = [r for r in TV.ROWS if r[0] == "resblock" and r[-1].endswith(":bf16x3")]


@pytest.mark.parametrize("row", TILE_CONV, ids=[f"{r[-1]}-k{r[3]}" for r in TILE_CONV])
def test_conv_mfma_tile_rows(row):
    _, cin, cout, k, d, impl, knobs, name = row
    assert impl == B3
    with TV.knobs_set(knobs):
        Conv1d("causal", cin, cout, k, 1, d, TV.B, TV.L, name, exact_name=True).check(TV.B, TV.L, f"{name} k{k} d{d}")


def test_the_tile_tables_still_have_their_bf16x3_rows():
    assert len(TILE_CONV) == 8 and len(TILE_RB) == 24, (len(TILE_CONV), len(TILE_RB))


# ------------------------------------------------------------------------------------------------ residual blocks
def _resblock(c, k, d, batch, length, name, what, exact_name=False):
    desc = ops.conv_desc(_lib.CONV_CAUSAL, batch, c, c, length, k, 1, d, 0, 0.1, B3)
    d2 = ops.conv_desc(_lib.CONV_CAUSAL, batch, c, c, length, 1, 1, 1, 0, 0.1, B3)
    got = ops.resblock_kernel_name(desc)
    assert (got == name) if exact_name else (got.startswith(name) and got.endswith(":bf16x3")), (got, name)
    zero = torch.zeros(c, device=DEV)

    def run(x, w1, b1, w2, b2):
        return ops.resblock_forward(desc, x.to(DEV), ops.conv_pack(desc, w1.to(DEV)), zero if b1 is None else b1.to(DEV),
                                    ops.conv_pack(d2, w2.to(DEV)), zero if b2 is None else b2.to(DEV), post_act=False)

    for which in "AB":                  # A: conv1's terms (rich w1, power-of-two w2); B: conv2's
        for rot in range(P.ROTATIONS):
            x, w1, w2, _, _ = P.probe_resblock(c, k, d, batch, length, rot, which)
            want, _ = P.resblock_ref(x, w1, None, w2, None, d)
            y = run(x, w1, None, w2, None).cpu()
            _probe(y[:, 1::2], want[:, 1::2], f"{what} probe {which} rot {rot}")
            assert max_abs(y[:, ::2], want[:, ::2]) < 1e-5 * max(1.0, float(want.abs().max())), (what, which, rot)
    x, w1, b1, w2, b2 = P.dense_resblock(c, k, d, batch, length, 13 * c + d)
    want, h64 = P.resblock_ref(x, w1, b1, w2, b2, d)
    c_ij = P.projection(run(x, w1, b1, w2, b2), want, P.resblock_conv1_terms(x, w1, w2, h64, d))
    P.assert_projection(c_ij, f"{what} conv1")


@pytest.mark.parametrize("c,d", P.RB_RING)
def test_resblock_b3(c, d):
    for batch, length in P.rb_lengths(c):
        _resblock(c, 7, d, batch, length, "resblock_b3<", f"resblock_b3 C{c} d{d} {batch}x{length}")


def test_resblock_mfma_other_dilation():
    _resblock(64, 7, 2, 1, 512, "resblock_mfma<", "resblock_mfma C64 d2 1x512")


@pytest.mark.parametrize("row", TILE_RB, ids=[f"{r[-1]}-k{r[3]}-sched{r[-2]['bf_sched']}" for r in TILE_RB])
def test_resblock_mfma_tile_rows(row):
    _, c, _, k, d, impl, knobs, name = row
    assert impl == B3
    with TV.knobs_set(knobs):
        _resblock(c, k, d, TV.B, TV.L, name, f"{name} k{k} d{d} sched {knobs['bf_sched']}", exact_name=True)


# ------------------------------------------------------------------------------------------------ Conv2d
def _desc2d(f):
    b, cin, cout, h, w_, kh, kw, sh, sw, ph, pw = f
    return ops.conv2d_desc(b, cin, cout, h, w_, kh, kw, (sh, sw), (ph, pw), epilogue=0, impl=B3)


def _dense_weight_2d(f, gen):
    b, cin, cout, h, w_, kh, kw = f[:7]
    return torch.randn(cout, cin, kh, kw, generator=gen) * (1.5 / (cin * kh * kw) ** 0.5)


@pytest.mark.parametrize("f,name", P.C2D_FWD, ids=[n for _, n in P.C2D_FWD])
def test_conv2d_forward(f, name):
    b, cin, cout, h, w_, kh, kw, sh, sw, ph, pw = f
    desc = _desc2d(f)
    assert ops.conv2d_kernel_name(desc) == name, ops.conv2d_kernel_name(desc)
    op = P.conv2d_op((sh, sw), (ph, pw))
    zero = torch.zeros(cout, device=DEV)
    x = P.rich_activation((b, cin, h, w_), cin + h)
    for rot in range(P.ROTATIONS):
        w, _ = P.probe_weight_2d(cin, cout, kh, kw, rot)
        y = ops.conv2d_forward(desc, x.to(DEV), ops.conv2d_pack(desc, w.to(DEV)), zero)
        _probe(y, op(w.double(), x.double()), f"conv2d fwd {name} rot {rot}")
    gen = torch.Generator().manual_seed(cin + cout)
    w, bias, x = _dense_weight_2d(f, gen), torch.randn(cout, generator=gen) * 0.1, torch.randn(b, cin, h, w_, generator=gen)
    y = ops.conv2d_forward(desc, x.to(DEV), ops.conv2d_pack(desc, w.to(DEV)), bias.to(DEV))
    c = P.projection(y, op(w.double(), x.double(), bias.double()), P.term_tensors(op, w, x))
    P.assert_projection(c, f"conv2d fwd {name}")
    if not name.startswith("conv2d_b3"):
        # The patch-tile fallback's name carries no arithmetic (the fp32 row with conv_cc = 16 answers with the same string),
        # and an fp32 kernel passes both instruments.  That the bf16x3 arithmetic ran shows in the two larger DROPPED pairs:
        # a kernel that leaves m.l and l.m out reads -1 there, one that has them (fp32) reads 0; halfway decides.
        worst = P.worst_coefficients(c)
        assert worst[(1, 2)] < -0.5 and worst[(2, 1)] < -0.5, (name, worst[(1, 2)], worst[(2, 1)])


@pytest.mark.parametrize("f,name", P.C2D_BWD, ids=[f"{n}-w{f[4]}" for f, n in P.C2D_BWD])
def test_conv2d_backward_data(f, name):
    b, cin, cout, h, w_, kh, kw, sh, sw, ph, pw = f
    desc = _desc2d(f)
    assert ops.conv2d_bwd_data_kernel_name(desc) == name, ops.conv2d_bwd_data_kernel_name(desc)
    op = P.conv2d_bwd_data_op((sh, sw), (ph, pw), (b, cin, h, w_))
    dy = P.rich_activation(P.out_shape_2d(f), cout + h)
    for rot in range(P.ROTATIONS):
        w, _ = P.probe_weight_2d_bwd(cin, cout, kh, kw, sh, sw, rot)
        dx = ops.conv2d_bwd_data(desc, dy.to(DEV), ops.conv2d_pack_bwd(desc, w.to(DEV)))
        _probe(dx, op(w.double(), dy.double()), f"conv2d bwd-data {name} w{w_} rot {rot}")
    gen = torch.Generator().manual_seed(cin + cout + 1)
    w, dy = _dense_weight_2d(f, gen), torch.randn(P.out_shape_2d(f), generator=gen)
    dx = ops.conv2d_bwd_data(desc, dy.to(DEV), ops.conv2d_pack_bwd(desc, w.to(DEV)))
    c = P.projection(dx, op(w.double(), dy.double()), P.term_tensors(op, w, dy))
    P.assert_projection(c, f"conv2d bwd-data {name} w{w_}")


# ------------------------------------------------------------------------------------------------ weight gradients
@pytest.mark.parametrize("f,name", P.WGRAD_1D, ids=[f"{f[0]}-{n}" for f, n in P.WGRAD_1D])
def test_weight_gradient_1d_staged(f, name):
    """conv_bwd_weight_kernel<.., 1>: the default dispatch answers a bf16x3 descriptor with the fp32 direct kernel; knob
    dw_direct = 0 is what puts the bf16x3 contraction of the staged kernel on the 1-D op."""
    kind, cin, cout, k, s, batch, length = f
    desc = ops.conv_desc(KIND[kind], batch, cin, cout, length, k, s, 1, 0, 0.1, B3)
    shape = (cin, cout, k) if kind == "convt" else (cout, cin, k)
    fwd = P.conv1d_op(kind, s, 1)
    op = P.wgrad_op(fwd, shape)
    gen = torch.Generator().manual_seed(cin + cout + k)
    x = torch.randn(batch, cin, length, generator=gen)
    dy = torch.randn(batch, cout, ops.conv_out_len(desc), generator=gen)
    with TV.knobs_set({"dw_direct": 0}):
        got = ops.conv_bwd_weight_kernel_name(desc)
        assert got.startswith(name + " "), got
        dv, _, _ = ops.conv_bwd_weight(desc, x.to(DEV), dy.to(DEV), torch.zeros(shape, device=DEV), None)
    rows = 1 if kind == "convt" else 0           # the kernel's output rows are Cout: dim 1 of a transposed layer's (cin, cout, k)
    c = P.projection(dv, op(dy.double(), x.double()), P.term_tensors(op, dy, x), dim=rows)
    P.assert_projection(c, f"dW 1-D {kind} {name}")


@pytest.mark.parametrize("f,name", P.WGRAD_2D, ids=[n for _, n in P.WGRAD_2D])
def test_weight_gradient_2d(f, name):
    b, cin, cout, h, w_, kh, kw, sh, sw, ph, pw = f
    desc = _desc2d(f)
    got = ops.conv2d_bwd_weight_kernel_name(desc)
    assert got.startswith(name + " "), got
    op = P.wgrad_op(P.conv2d_op((sh, sw), (ph, pw)), (cout, cin, kh, kw))
    gen = torch.Generator().manual_seed(cin + cout)
    x, dy = torch.randn(b, cin, h, w_, generator=gen), torch.randn(P.out_shape_2d(f), generator=gen)
    dw, _ = ops.conv2d_bwd_weight(desc, x.to(DEV), dy.to(DEV))
    c = P.projection(dw, op(dy.double(), x.double()), P.term_tensors(op, dy, x), dim=0)
    P.assert_projection(c, f"dW 2-D {name}")
