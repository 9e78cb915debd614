"""Every row of the variant tables of the three tile families, launched once and compared with the float64 oracle.

csrc/conv_mfma.hip, csrc/resblock_mfma.hip and csrc/conv_direct.hip are what runs a layer the ring kernels refuse; most of
their rows are reached only under a selection knob (``conv_cc``, ``conv_shape``, ``conv_short``, ``rb_cc``, ``rb_sched``,
``rb_occ``, ``bf_sched``) or by a shape no model has.  ``ROWS`` lists one descriptor per row with the knobs that reach it and the
name the host-only query must answer for it (tools/tile_rows.py launches the same list for a kernel trace, where the full
template arguments show).  Shapes: B = 2, L = 700 (a partial tile in both directions for every tile width), k = 3 and k = 7
with dilation 3; the second-choice tiles of a class are reached by dilations whose halo no longer fits the first choice's LDS
budget.  Tolerances are those of tests/test_gpu_parity.py for the same family and arithmetic: 2e-5 x max(1, |y|) for the conv
kernels (fp32 and bf16x3), 3e-5 for the residual block.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from audio_generation_amd import _lib, ops
from oracle import codec
from tests.helpers import max_abs

DEV = "cuda"
AUTO, DIRECT, BF16X3 = _lib.IMPL_AUTO, _lib.IMPL_DIRECT, _lib.IMPL_MFMA_BF16X3
B, L = 2, 700
KD = ((3, 1), (7, 3))
TILES_OFF = {"conv_impl": 0, "rb_impl": 0}      # the ring kernels step aside: the tile families run


def _mfma_rows():
    """("conv", cin, cout, k, d, impl, knobs, name) for every row of conv_mfma.hip's tables on 1-D layers."""
    rows = []
    classes = [(32, "1,4,1,4", {}, True), (64, "2,2,1,4", {}, True), (128, "1,2,4,1", {}, True),
               (128, "2,2,2,2", {"conv_short": 0}, True), (128, "1,4,4,1", {"conv_shape": 1, "conv_short": 0}, False)]
    for cout, tile, knobs, has_bf in classes:
        for k, d in KD:
            rows.append(("conv", 16, cout, k, d, AUTO, knobs, f"conv_mfma<{tile},16>"))
            rows.append(("conv", 16, cout, k, d, AUTO, {**knobs, "conv_cc": 8}, f"conv_mfma<{tile},8>"))
            rows.append(("conv", 32, cout, k, d, AUTO, {**knobs, "conv_cc": 32}, f"conv_mfma<{tile},32>"))
            if has_bf:
                rows.append(("conv", 16, cout, k, d, BF16X3, knobs, f"conv_mfma<{tile},16>:bf16x3"))
    # second-choice tiles: a halo of 6 d columns that the class's wide tile cannot stage (72 KB, then 160 KB of LDS)
    rows += [("conv", 16, 32, 7, 110, AUTO, {}, "conv_mfma<1,1,1,4,8>"), ("conv", 16, 32, 7, 130, AUTO, {"conv_cc": 16}, "conv_mfma<1,1,1,4,16>"),
             ("conv", 16, 64, 7, 160, AUTO, {}, "conv_mfma<2,1,1,4,8>"), ("conv", 16, 64, 7, 180, AUTO, {"conv_cc": 16}, "conv_mfma<2,1,1,4,16>")]
    return rows


def _resblock_rows():
    rows = []
    for c, tile in ((32, "1,4"), (64, "2,2"), (128, "4,1"), (256, "8,1")):
        for k, d in KD:
            for knobs in ({"rb_sched": 0}, {"rb_sched": 1}, {"rb_sched": 2}, {"rb_occ": 3}):
                rows.append(("resblock", c, c, k, d, AUTO, knobs, f"resblock_mfma<{tile},16>"))
            rows.append(("resblock", c, c, k, d, AUTO, {"rb_cc": 32}, f"resblock_mfma<{tile},{32 if c < 256 else 16}>"))
            for s in (0, 1, 2):
                rows.append(("resblock", c, c, k, d, BF16X3, {"bf_sched": s}, f"resblock_mfma<{tile},16>:bf16x3"))
    return rows


def _direct_rows():
    few = {1: "conv_fewrows<1>", 2: "conv_fewrows<4>", 4: "conv_fewrows<4>", 8: "conv_fewrows<8>", 16: "conv_fewrows<16>", 32: "conv_direct<32>"}
    narrow = {1: "conv_narrow<1>", 2: "conv_narrow<2>", 32: "conv_narrow<16>"}      # the streaming form: causal k = 7, dilation 1
    rows = [("conv", 16, m, k, d, DIRECT, {}, few[m]) for k, d in KD for m in few]
    rows += [("conv", 16, m, 7, 1, DIRECT, {}, narrow[m]) for m in narrow]
    # grouped layers: the rows of a block share their group, one layer per class of Cout / groups
    for k, d in KD:
        rows += [("grouped", 16, cout, k, d, g, {}, f"conv_direct<{t}>") for cout, g, t in ((64, 2, 32), (64, 4, 16), (16, 4, 4), (16, 16, 1))]
    return rows


# Conv2d layers of tests/test_kernel_names_cpu.py (C2D_ODD): 24 -> 40 channels run row-folded (MODE 1, one output row per tile:
# the 128-column tile of narrow maps), 16 -> 32 as patches (MODE 2), fp32 and bf16x3
C2D_ROWS = [("conv2d", (2, 24, 40, 20, 33, 3, 3, 1, 1, 1, 1), AUTO, {}, "conv_mfma<1,1,1,4,16>"),
            ("conv2d", (1, 16, 32, 64, 64, 3, 3, 1, 1, 0, 0), AUTO, {}, "conv_mfma<1,4,1,4,8>"),
            ("conv2d", (1, 16, 32, 64, 64, 3, 3, 1, 1, 0, 0), AUTO, {"conv_cc": 16}, "conv_mfma<1,4,1,4,16>"),
            ("conv2d", (1, 16, 32, 64, 64, 3, 3, 1, 1, 0, 0), BF16X3, {}, "conv_mfma<1,4,1,4,16>")]
ROWS = _mfma_rows() + C2D_ROWS + _resblock_rows() + _direct_rows()


class knobs_set:
    """The tile families with `knobs`; every knob goes back to what it was."""

    def __init__(self, knobs):
        self.knobs = {**TILES_OFF, **knobs}

    def __enter__(self):
        lib = _lib.load()
        self.before = {k: lib.agx_get_tuning(k.encode()) for k in self.knobs}
        for k, v in self.knobs.items():
            assert lib.agx_set_tuning(k.encode(), v) == 0, k

    def __exit__(self, *exc):
        for k, v in self.before.items():
            _lib.load().agx_set_tuning(k.encode(), v)


@functools.lru_cache(maxsize=None)
def _layer(cin, cout, k, d, groups=1):
    """(x, v, g, bias, leaky(conv(x)) in float64) of a causal (dense) or zero-padded (grouped) layer: made once per shape."""
    gen = torch.Generator().manual_seed(1000 * cin + 10 * cout + k + d + groups)
    v = torch.randn(cout, cin // groups, k, generator=gen) / (cin // groups * k) ** 0.5
    g = torch.rand(cout, 1, 1, generator=gen) + 0.5
    bias = torch.randn(cout, generator=gen) * 0.1
    x = torch.randn(B, cin, L, generator=gen)
    if groups == 1:
        want = codec.causal_conv1d(x.double(), codec.fold_weight_norm(g.double(), v.double()), bias.double(), dilation=d)
    else:
        want = F.conv1d(x.double(), v.double(), bias.double(), padding=d * (k - 1) // 2, dilation=d, groups=groups)
    return x, v, g, bias, codec.leaky(want)


@functools.lru_cache(maxsize=None)
def _block(c, k, d):
    gen = torch.Generator().manual_seed(100 * c + k + d)
    sd = {}
    for name, kk in (("conv1", k), ("conv2", 1)):
        v = torch.randn(c, c, kk, generator=gen) / (c * kk) ** 0.5
        sd[f"{name}.conv.weight_v"] = v
        sd[f"{name}.conv.weight_g"] = v.reshape(c, -1).norm(dim=1).reshape(-1, 1, 1) * 1.1
        sd[f"{name}.conv.bias"] = torch.randn(c, generator=gen) * 0.1
    x = torch.randn(B, c, L, generator=gen)
    return x, sd, codec.leaky(codec.residual_block(x.double(), {n: t.double() for n, t in sd.items()}, "", d))


@functools.lru_cache(maxsize=None)
def _layer2d(f):
    b, cin, cout, h, w, kh, kw, sh, sw, ph, pw = f
    gen = torch.Generator().manual_seed(cin * 7 + cout)
    x = torch.randn(b, cin, h, w, generator=gen)
    wt = torch.randn(cout, cin, kh, kw, generator=gen) / (cin * kh * kw) ** 0.5
    bias = torch.randn(cout, generator=gen) * 0.1
    return x, wt, bias, F.leaky_relu(F.conv2d(x.double(), wt.double(), bias.double(), stride=(sh, sw), padding=(ph, pw)), 0.2)


def describe(row):
    """(descriptor, the name query's answer for it); the knobs must be set.  No GPU is needed."""
    if row[0] == "conv2d":
        f, impl = row[1], row[2]
        desc = ops.conv2d_desc(*f[:7], f[7:9], f[9:11], _lib.EPI_LEAKY_PRE, 0.2, impl)
        return desc, ops.conv2d_kernel_name(desc)
    op, cin, cout, k, d, impl = row[:6]
    if op == "resblock":
        desc = ops.conv_desc(_lib.CONV_CAUSAL, B, cin, cin, L, k, 1, d, 0, 0.1, impl)
        return desc, ops.resblock_kernel_name(desc)
    if op == "grouped":      # (the impl slot holds the groups)
        desc = ops.conv_desc(_lib.CONV_PADDED, B, cin, cout, L, k, 1, d, _lib.EPI_LEAKY_PRE, 0.1, AUTO, groups=impl, padding=d * (k - 1) // 2)
    else:
        desc = ops.conv_desc(_lib.CONV_CAUSAL, B, cin, cout, L, k, 1, d, _lib.EPI_LEAKY_PRE, 0.1, impl)
    return desc, ops.conv_kernel_name(desc)


def run_row(row):
    """(output, float64 reference, tolerance) of one row; the knobs must be set."""
    desc, name = describe(row)
    assert name == row[-1], row
    if row[0] == "conv2d":
        x, wt, bias, want = _layer2d(row[1])
        y = ops.conv2d_forward(desc, x.to(DEV), ops.conv2d_pack(desc, wt.to(DEV)), bias.to(DEV))
        return y, want, 2e-5 * max(1.0, float(want.abs().max()))
    op, cin, cout, k, d, impl = row[:6]
    if op == "resblock":
        x, sd, want = _block(cin, k, d)
        d2 = ops.conv_desc(_lib.CONV_CAUSAL, B, cin, cin, L, 1, 1, 1, 0, 0.1, impl)
        w = {n: t.to(DEV) for n, t in sd.items()}
        y = ops.resblock_forward(desc, x.to(DEV), ops.conv_pack(desc, w["conv1.conv.weight_v"], w["conv1.conv.weight_g"]), w["conv1.conv.bias"],
                                 ops.conv_pack(d2, w["conv2.conv.weight_v"], w["conv2.conv.weight_g"]), w["conv2.conv.bias"], post_act=True)
        return y, want, 3e-5
    x, v, g, bias, want = _layer(cin, cout, k, d, impl if op == "grouped" else 1)
    packed = ops.conv_pack(desc, v.to(DEV), None if op == "grouped" else g.to(DEV))
    return ops.conv_forward(desc, x.to(DEV), packed, bias.to(DEV)), want, 2e-5 * max(1.0, float(want.abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["conv_mfma", "resblock_mfma", "conv_direct"])
def test_every_table_row_matches_the_float64_oracle(family):
    lib = _lib.load()
    names = ("conv_direct<", "conv_narrow<", "conv_fewrows<") if family == "conv_direct" else (family + "<",)
    rows = [r for r in ROWS if r[-1].startswith(names)]
    assert len(rows) >= {"conv_mfma": 40, "resblock_mfma": 64, "conv_direct": 20}[family]
    before = {k.encode(): lib.agx_get_tuning(k.encode()) for r in ROWS for k in {**TILES_OFF, **r[-2]}}
    for row in rows:
        with knobs_set(row[-2]):
            y, want, tol = run_row(row)
        assert tuple(y.shape) == tuple(want.shape), row
        err = max_abs(y.cpu(), want)
        assert err < tol, (row, err)
    assert {k: lib.agx_get_tuning(k) for k in before} == before


def test_the_rows_name_every_instantiated_tile():
    """(no GPU) Each row's descriptor and knobs get the row's name from the host-only query, and ROWS reaches each name the
    three families can answer with."""
    for row in ROWS:
        with knobs_set(row[-2]):
            assert describe(row)[1] == row[-1], row
    want = {f"conv_mfma<{t},{cc}>" for t in ("2,2,2,2", "1,2,4,1", "1,4,4,1", "2,2,1,4", "1,4,1,4") for cc in (16, 8, 32)}
    want |= {f"conv_mfma<{t},{cc}>" for t in ("2,1,1,4", "1,1,1,4") for cc in (16, 8)}
    want |= {f"resblock_mfma<{t},{cc}>" for t in ("1,4", "2,2", "4,1") for cc in (16, 32)} | {"resblock_mfma<8,1,16>"}
    want |= {f"conv_narrow<{n}>" for n in (16, 2, 1)} | {f"conv_fewrows<{n}>" for n in (16, 8, 4, 1)} | {f"conv_direct<{n}>" for n in (32, 16, 4, 1)}
    assert {r[-1].split(":")[0] for r in ROWS} == want
