"""Memory contract of the C-ABI wrappers as shipped: every output, workspace, packed image and in/out buffer of a call lives
in a guarded, poisoned arena (tests/guarded.py), exactly as large as the wrapper asks for.  Each case runs under the fill
patterns 0x00, 0x00, 0xFF, 0x7F and must

1. leave every guard byte alone (no write before or after an output or past a reported workspace size),
2. produce outputs free of NaN/Inf and within the tolerance the op's own parity test uses against float64,
3. produce bitwise the same outputs whatever the memory held before (no unwritten output element, no accumulation into an
   uncleared workspace, no over-read of an input that reaches the result), and
4. run the kernel the case is there for (the family's name query).

This is not a second parity suite: one or two of the smallest shapes at which the edge exists per kernel name.  The reference
of a case is computed once (CPU, float64 or the oracle) and shared by its runs.

``test_operand_placement`` runs the same table with the caller's operands 4, 8 and 12 bytes past a 16-byte boundary (a crop
``wave[s:s + L]``, a batch slice, a parameter carved out of a flat buffer; what the wrapper allocates itself stays aligned)
and requires, besides (1) and (2), the bits of the aligned run: include/agx.h promises that operands need 4-byte alignment
only and that the result does not depend on it.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from audio_generation_amd import _lib, ops
from audio_generation_amd import signal_ops as sg
from oracle import attention as oattn
from oracle import bitstream, codec, rvq
from oracle import discriminator as od
from oracle import signal as osg
from oracle import wavelets as owv
from tests.guarded import PLACEMENT_RUNS, Out, routed, run_contract
from tests.test_gpu_attention_flash import BF16_MAX_REL, _core
from tests.test_gpu_attention_variants import CASES as ATTENTION_ROWS
from tests.test_gpu_conv_p import LAYERS, _ref_epilogue

DEV = "cuda"
KIND = {"conv": _lib.CONV_CAUSAL, "convt": _lib.CONV_TRANSPOSED, "upconv": _lib.CONV_UPSAMPLE, "same": _lib.CONV_SAME}
RAGGED = ((1, 4), (3, 45), (1, 77), (2, 131), (2, 225))     # clips shorter than a tile, ragged rows, last row of the last clip
CASES = {}
# case name -> the buffers known not to be bitwise reproducible run to run (invariance falls back to the reference check for
# them).  No float atomics exist in csrc/: empty, and an op that turns up here is a finding to write down.
NOT_REPRODUCIBLE = {}
# case name -> the buffers whose bits may legitimately depend on where an operand starts, each with the kernel line that makes
# its summation order depend on the address.  Empty: every wide access is base + 4 * index and every reduction runs in index
# order ("Operand placement").
PLACEMENT_DEPENDENT = {}


def _set(knob, v):
    assert _lib.load().agx_set_tuning(knob.encode(), v) == 0


def case(name, names=None):
    """Register ``make() -> (inputs, run)``: ``inputs`` is a dict of CPU tensors (built once from a seeded generator, with the
    references ``run`` closes over); ``run(**placed)`` calls the wrapper on the arena copies and returns the ``Out`` list.
    ``names()`` asserts the kernel names the case expects (host-only queries)."""
    def register(make):
        built = []

        def one_run(arena):
            if not built:
                built.append(make())
            inputs, run = built[0]
            placed = {k: None if v is None else arena.place(v) for k, v in inputs.items()}
            with routed(arena, ops, sg):
                return run(**placed)
        assert name not in CASES, name
        CASES[name] = (one_run, names, make)
        return make
    return register


def _rel(want, tol):
    """``tol * max(1, max|want|)``: the form the conv / attention parity tests state their tolerances in."""
    return tol * max(1.0, float(torch.as_tensor(want).abs().max()))


def _close(want, tol, floor=1e-7):
    """The ``close`` of tests/test_gpu_disc.py and tests/test_gpu_signal.py: ``tol * max|want| + floor``."""
    return tol * (float(torch.as_tensor(want).abs().max()) + 1e-12) + floor


# ------------------------------------------------------------------------------------------------ conv forward
def _conv_data(kind, cin, cout, k, s, d, b, length, gen, epi, kind_id=None):
    wshape = (cin, cout, k) if kind == "convt" else (cout, cin, k)
    v = torch.randn(wshape, generator=gen) / (cin * k) ** 0.5
    g = torch.rand((wshape[0], 1, 1), generator=gen) + 0.5
    bias = torch.randn(cout, generator=gen) * 0.1
    x = torch.randn(b, cin, length, generator=gen)
    w = codec.fold_weight_norm(g, v)
    if kind == "conv":
        pre = codec.causal_conv1d(x, w, bias, stride=s, dilation=d)
    elif kind == "convt":
        pre = codec.causal_conv_t1d(x, w, bias, stride=s)
    elif kind == "upconv":
        pre = codec.upsample_conv1d(x, w, bias, s)
    else:
        pre = F.conv1d(x, w, bias, padding="same")
    res = torch.randn(pre.shape, generator=gen) if epi & _lib.EPI_RESIDUAL else None
    return dict(v=v, g=g, bias=bias, x=x, res=res), _ref_epilogue(pre, epi, res)


def _conv_case(name, kind, cin, cout, k, s, d, shapes, impl, prefix, epis=(_lib.EPI_LEAKY_PRE,), suffix="", tol=2e-5, knob=1):
    """conv_pack + conv_forward at every (B, L) of ``shapes`` x every epilogue of ``epis``; the kernel name must start with
    ``prefix`` and end with ``suffix``."""
    combos = [(b, length, epi) for b, length in shapes for epi in epis]
    descs = [ops.conv_desc(KIND[kind], b, cin, cout, length, k, s, d, epi, 0.1, impl) for b, length, epi in combos]

    def names():
        try:
            _set("conv_impl", knob)
            for desc in descs:
                got = ops.conv_kernel_name(desc)
                assert got.startswith(prefix) and got.endswith(suffix), (got, prefix, suffix)
        finally:
            _set("conv_impl", 1)

    @case(name, names)
    def make():
        gen = torch.Generator().manual_seed(sum(map(ord, name)))
        inputs, wants = {}, []
        for n, (b, length, epi) in enumerate(combos):
            data, want = _conv_data(kind, cin, cout, k, s, d, b, length, gen, epi)
            inputs.update({f"{key}{n}": t for key, t in data.items()})
            wants.append(want)

        def run(**p):
            outs = []
            try:
                _set("conv_impl", knob)
                for n, desc in enumerate(descs):
                    packed = ops.conv_pack(desc, p[f"v{n}"], p[f"g{n}"])
                    y = ops.conv_forward(desc, p[f"x{n}"], packed, p[f"bias{n}"], res=p[f"res{n}"])
                    outs.append(Out(f"y[B={combos[n][0]},L={combos[n][1]},epi={combos[n][2]}]", y, wants[n], _rel(wants[n], tol)))
            finally:
                _set("conv_impl", 1)
            return outs
        return inputs, run


_conv_case("conv_forward/direct", "conv", 48, 40, 3, 1, 1, ((1, 77), (2, 131)), _lib.IMPL_DIRECT, "conv_direct")
_conv_case("conv_forward/direct_upsample", "upconv", 16, 8, 4, 3, 1, ((1, 33),), _lib.IMPL_DIRECT, "conv_direct")
_conv_case("conv_forward/direct_transposed", "convt", 32, 16, 9, 4, 1, ((1, 50),), _lib.IMPL_DIRECT, "conv_direct")
_conv_case("conv_forward/mfma", "conv", 64, 64, 7, 1, 3, RAGGED, _lib.IMPL_MFMA, "conv_mfma")
_conv_case("conv_forward/mfma_strided", "conv", 64, 128, 9, 4, 1, RAGGED, _lib.IMPL_AUTO, "conv_mfma", knob=0)
_conv_case("conv_forward/bf16x3", "conv", 64, 64, 7, 1, 3, RAGGED, _lib.IMPL_MFMA_BF16X3, "conv_", suffix=":bf16x3")
for _variant, _kind, _cin, _cout, _k, _s in LAYERS:
    _conv_case(f"conv_forward/conv_p/{_variant}-{_kind}-{_cin}-{_cout}", _kind, _cin, _cout, _k, _s, 1, RAGGED, _lib.IMPL_AUTO,
               f"conv_p<{_variant},")
EPIS = (0, _lib.EPI_LEAKY_PRE, _lib.EPI_GELU_PRE, _lib.EPI_RESIDUAL, _lib.EPI_RESIDUAL | _lib.EPI_LEAKY_POST,
        _lib.EPI_LEAKY_PRE | _lib.EPI_RESIDUAL | _lib.EPI_LEAKY_POST)
for _variant, _kind, _cin, _cout, _k in (("k1", "conv", 512, 512, 1), ("k1", "conv", 512, 1536, 1), ("k1", "conv", 256, 256, 1),
                                         ("k1", "conv", 128, 128, 1), ("same11", "same", 256, 512, 11),
                                         ("same3", "same", 512, 128, 3), ("k3", "conv", 512, 512, 3)):
    _conv_case(f"conv_forward/one_phase/{_variant}-{_cin}-{_cout}", _kind, _cin, _cout, _k, 1, 1, ((1, 77),), _lib.IMPL_AUTO,
               f"conv_p<{_variant},", epis=EPIS)


def _planes_case(name, variant, kind, cin, cout, k, s, b, length):
    desc = ops.conv_desc(KIND[kind], b, cin, cout, length, k, s, 1, _lib.EPI_LEAKY_PRE, 0.1, _lib.IMPL_MFMA_BF16X3)

    def names():
        assert ops.conv_kernel_name(desc).endswith(":bf16x3")
        assert ops.conv_planes_supported(desc) == (2 if kind == "convt" else 1)

    @case(name, names)
    def make():
        gen = torch.Generator().manual_seed(sum(map(ord, name)))
        data, want = _conv_data(kind, cin, cout, k, s, 1, b, length, gen, _lib.EPI_LEAKY_PRE)
        tol = _rel(want, 1e-5)                                  # tests/test_gpu_conv_b3.py: TOL

        def run(v, g, bias, x, res):
            packed = ops.conv_pack(desc, v, g)
            planes = ops.planes_split(x)
            outs = [Out("planes", planes, _split_reference(x), exact=True),
                    Out("y", ops.conv_forward_planes(desc, planes, packed, bias), want, tol)]
            if kind == "convt":
                yp = ops.conv_forward_planes(desc, planes, packed, bias, out_planes=True)
                outs.append(Out("y_planes", yp, yp.detach().cpu(), exact=True))          # bitwise invariance and guards ...
                outs.append(Out("y_planes_joined", ops.planes_join(yp), want, tol))   # ... and the values they stand for
            return outs
        return data, run


def _split_reference(x):
    """h = bf16(x), m = bf16(x - h), l = bf16(x - h - m): the exact three-piece split (h + m + l == x), planes layout."""
    x = x.detach().cpu()
    h = x.to(torch.bfloat16)
    m = (x - h.float()).to(torch.bfloat16)
    low = (x - h.float() - m.float()).to(torch.bfloat16)
    b, c, length = x.shape
    return torch.stack([h, m, low], dim=1).reshape(b, 3, c // 8, 8, length).permute(0, 2, 1, 4, 3).contiguous()


_planes_case("conv_forward_planes/k7-convt", "k7", "convt", 512, 512, 7, 1, 2, 77)
_planes_case("conv_forward_planes/up8", "up8", "upconv", 512, 256, 17, 8, 1, 45)


# ------------------------------------------------------------------------------------------------ residual block
def _resblock_case(name, c, d, shapes, impl, prefix, knob, tol):
    descs = [ops.conv_desc(_lib.CONV_CAUSAL, b, c, c, length, 7, 1, d, impl=impl) for b, length in shapes]

    def names():
        try:
            _set("rb_impl", knob)
            for desc in descs:
                assert ops.resblock_kernel_name(desc).startswith(prefix), (ops.resblock_kernel_name(desc), prefix)
        finally:
            _set("rb_impl", 1)

    @case(name, names)
    def make():
        gen = torch.Generator().manual_seed(100 + c + d)
        sd = {}
        for conv, k in (("conv1", 7), ("conv2", 1)):
            v = torch.randn(c, c, k, generator=gen) / (c * k) ** 0.5
            sd[f"{conv}.conv.weight_v"] = v
            sd[f"{conv}.conv.weight_g"] = v.reshape(c, -1).norm(dim=1).reshape(-1, 1, 1) * 1.1
            sd[f"{conv}.conv.bias"] = torch.randn(c, generator=gen) * 0.1
        inputs = {"v1": sd["conv1.conv.weight_v"], "g1": sd["conv1.conv.weight_g"], "b1": sd["conv1.conv.bias"],
                  "v2": sd["conv2.conv.weight_v"], "g2": sd["conv2.conv.weight_g"], "b2": sd["conv2.conv.bias"]}
        wants = []
        for n, (b, length) in enumerate(shapes):
            inputs[f"x{n}"] = torch.randn(b, c, length, generator=gen)
            wants.append(codec.leaky(codec.residual_block(inputs[f"x{n}"], sd, "", d)))

        def run(v1, g1, b1, v2, g2, b2, **xs):
            outs = []
            try:
                _set("rb_impl", knob)
                for n, desc in enumerate(descs):
                    d2 = ops.conv_desc(_lib.CONV_CAUSAL, desc.batch, c, c, desc.l_in, 1, 1, 1, impl=impl)
                    y = ops.resblock_forward(desc, xs[f"x{n}"], ops.conv_pack(desc, v1, g1), b1, ops.conv_pack(d2, v2, g2), b2)
                    outs.append(Out(f"y[B={desc.batch},L={desc.l_in}]", y, wants[n], _rel(wants[n], tol)))
            finally:
                _set("rb_impl", 1)
            return outs
        return inputs, run


for _c in (32, 64, 128, 256):
    for _d in (1, 3, 9):
        # resblock_p takes L % 4 == 0 only (tests/test_gpu_resblock_p.py); 77 and 225 reach the first kernel under it
        _resblock_case(f"resblock_forward/p/C{_c}-d{_d}", _c, _d, ((1, 4), (2, 76), (2, 224)), _lib.IMPL_AUTO, "resblock_p", 1, 3e-5)
        _resblock_case(f"resblock_forward/b3/C{_c}-d{_d}", _c, _d, ((1, 4), (1, 77), (2, 225)), _lib.IMPL_MFMA_BF16X3,
                       "resblock_b3", 1, 1e-5)
    _resblock_case(f"resblock_forward/mfma/C{_c}", _c, 3, ((1, 4), (1, 77), (2, 225)), _lib.IMPL_AUTO, "resblock_mfma", 0, 3e-5)
_resblock_case("resblock_forward/two_launches/C512", 512, 1, ((1, 4), (1, 77)), _lib.IMPL_AUTO, "2x:", 1, 3e-5)


# ------------------------------------------------------------------------------------------------ conv backward
def _empties(arena, since, dtype):
    """Byte sizes, sorted, of what the wrapper under test allocated in ``arena`` after its first ``since`` allocations, by
    dtype: independent of the order the wrapper allocates in."""
    return sorted(a.nbytes for a in arena.allocs[since:] if a.what == "empty" and a.dtype == dtype)


def _bwd_case(kernel, copy, kind, cin, cout, k, s, d, b, length, impl=_lib.IMPL_AUTO, dw_direct=3):
    """conv_pack_bwd, conv_bwd_data (plain, add + mask) and conv_bwd_weight (g and bias wanted / neither) of one layer whose
    weight gradient runs ``kernel`` -- one row of bw1_variants (csrc/conv_bwd_weight.hip) -- reading ``copy`` (the "op=" of the
    name query: the phase-split copy of x or dy behind the workspace's partial tiles, or none).  ``dw_direct`` = 0 keeps the
    layer on the staged kernels."""
    name = f"conv_bwd/{kernel}/op={copy}/{kind}-{cin}-{cout}-k{k}-s{s}"
    desc = ops.conv_desc(KIND[kind], b, cin, cout, length, k, s, d, 0, 0.1, impl)

    def names():
        try:
            _set("dw_direct", dw_direct)
            got = ops.conv_bwd_weight_kernel_name(desc)
        finally:
            _set("dw_direct", 3)
        assert got.split(" ")[0] == kernel and f" op={copy} " in got, (got, kernel, copy)

    @case(name, names)
    def make():
        gen = torch.Generator().manual_seed(sum(map(ord, name)))
        wshape = (cin, cout, k) if kind == "convt" else (cout, cin, k)
        v = (torch.randn(wshape, generator=gen) / (cin * k) ** 0.5).requires_grad_(True)
        g = (torch.rand((wshape[0], 1, 1), generator=gen) + 0.5).requires_grad_(True)
        bias = (torch.randn(cout, generator=gen) * 0.1).requires_grad_(True)
        pre = torch.randn(b, cin, length, generator=gen, requires_grad=True)
        x = codec.leaky(pre)
        conv = {"conv": lambda w, bb: codec.causal_conv1d(x, w, bb, stride=s, dilation=d),
                "convt": lambda w, bb: codec.causal_conv_t1d(x, w, bb, stride=s),
                "upconv": lambda w, bb: codec.upsample_conv1d(x, w, bb, s)}[kind]
        y = conv(codec.fold_weight_norm(g, v), bias)
        dy = torch.randn(y.shape, generator=gen)
        add = torch.randn(pre.shape, generator=gen)
        want_x, want_v, want_g, want_b = torch.autograd.grad(y, (x, v, g, bias), dy, retain_graph=True)
        mask = torch.where(x.detach() > 0, 1.0, 0.1)
        want_masked = (want_x + add) * mask
        w_plain = v.detach().clone().requires_grad_(True)
        (want_w,) = torch.autograd.grad(conv(w_plain, None), w_plain, dy)
        inputs = dict(v=v.detach(), g=g.detach(), x=x.detach(), dy=dy, add=add)

        def run(v, g, x, dy, add):
            arena = _arena_of(x)
            packed = ops.conv_pack_bwd(desc, v, g)
            dx = ops.conv_bwd_data(desc, dy, packed)
            dxm = ops.conv_bwd_data(desc, dy, packed, add=add, mask=x, slope=0.1)
            try:
                _set("dw_direct", dw_direct)
                ws_bytes = int(_lib.load().agx_conv_bwd_weight_workspace_bytes(ctypes.byref(desc)))
                n0 = len(arena.allocs)
                dv, dg, db = ops.conv_bwd_weight(desc, x, dy, v, g)
                assert _empties(arena, n0, torch.uint8) == [ws_bytes], "workspace exactly the queried bytes"
                n0 = len(arena.allocs)
                dw, no_g, no_b = ops.conv_bwd_weight(desc, x, dy, v, None, want_bias=False)
                assert _empties(arena, n0, torch.uint8) == [ws_bytes], "workspace exactly the queried bytes"
            finally:
                _set("dw_direct", 3)
            assert no_g is None and no_b is None
            return [Out("dx", dx, want_x, _rel(want_x, 3e-5)), Out("dx_add_mask", dxm, want_masked, _rel(want_masked, 3e-5)),
                    Out("dv", dv, want_v, _rel(want_v, 2e-4)), Out("dg", dg, want_g, _rel(want_g, 2e-4)),
                    Out("dbias", db, want_b, _rel(want_b, 2e-4)), Out("dw_plain", dw, want_w, _rel(want_w, 2e-4))]
        return inputs, run


# One row per row of bw1_variants, at a small ragged shape its selection accepts (bw_geometry: M = phases x C_out rows,
# NK = C_in x taps columns).  The direct kernels: M > 64 -> <2,2,2,2>; M > 32 -> <2,2,1,2> (NK > 64) or <2,2,1,1>; else
# <1,2,1,4> (NK > 32) or <1,1,1,1>; ",true" reads x through its phase-split copy (stride > 1); the transposed and upsampling
# layers read dy through one.  The staged kernels (dw_direct = 0): M >= 128 / >= 64 / below, ",1" = bf16x3.
_B3 = _lib.IMPL_MFMA_BF16X3
for _row in (("conv_bwd_weight_direct<2,2,2,2>", "none", "conv", 8, 72, 3, 1, 1, 2, 131),
             ("conv_bwd_weight_direct<2,2,1,2>", "phase_dy", "convt", 24, 20, 8, 2, 1, 1, 77),
             ("conv_bwd_weight_direct<2,2,1,1>", "none", "conv", 8, 40, 7, 1, 3, 3, 45),
             ("conv_bwd_weight_direct<1,2,1,4>", "phase_dy", "upconv", 16, 4, 4, 3, 1, 1, 33),
             ("conv_bwd_weight_direct<1,1,1,1>", "none", "conv", 4, 8, 7, 1, 1, 1, 77),
             ("conv_bwd_weight_direct<2,2,2,2,true>", "phase_x", "conv", 8, 72, 5, 2, 1, 2, 131),
             ("conv_bwd_weight_direct<2,2,1,2,true>", "phase_x", "conv", 24, 40, 5, 2, 1, 1, 77),
             ("conv_bwd_weight_direct<2,2,1,1,true>", "phase_x", "conv", 8, 40, 5, 2, 1, 3, 45),
             ("conv_bwd_weight_direct<1,2,1,4,true>", "phase_x", "conv", 16, 16, 9, 4, 1, 2, 131),
             ("conv_bwd_weight_direct<1,1,1,1,true>", "phase_x", "conv", 4, 8, 5, 2, 1, 1, 77),
             ("conv_bwd_weight<2,2,2,2>", "none", "conv", 8, 128, 7, 1, 3, 2, 131, _lib.IMPL_AUTO, 0),
             ("conv_bwd_weight<1,2,2,2>", "none", "conv", 8, 64, 5, 2, 1, 1, 77, _lib.IMPL_AUTO, 0),
             ("conv_bwd_weight<1,1,1,4>", "none", "convt", 8, 8, 9, 4, 1, 3, 45, _lib.IMPL_AUTO, 0),
             # (a bf16x3 descriptor's backward-data runs conv_mfma only: C_out % 16 == 0 and phases x C_in >= 32)
             ("conv_bwd_weight<2,2,2,2,1>", "none", "conv", 32, 128, 7, 1, 3, 2, 131, _B3, 0),
             ("conv_bwd_weight<1,2,2,2,1>", "none", "conv", 32, 64, 5, 2, 1, 1, 77, _B3, 0),
             ("conv_bwd_weight<1,1,1,4,1>", "none", "conv", 32, 16, 3, 1, 1, 3, 45, _B3, 0),
             # the direct implementation of the forward (a descriptor the backward ops take as well)
             ("conv_bwd_weight_direct<2,2,1,2>", "none", "conv", 48, 40, 3, 1, 1, 1, 77, _lib.IMPL_DIRECT)):
    _bwd_case(*_row)


@case("conv_bwd_data_gelu")
def _gelu_case():
    gen = torch.Generator().manual_seed(4)
    wt = torch.randn(32, 64, 1, generator=gen) / 8
    pre = torch.randn(2, 64, 50, generator=gen, requires_grad=True)
    dyc, add = torch.randn(2, 32, 50, generator=gen), torch.randn(2, 64, 50, generator=gen)
    gelu = F.gelu(pre)
    (want,) = torch.autograd.grad(F.conv1d(gelu, wt), pre, dyc, retain_graph=True)
    (want_add,) = torch.autograd.grad(gelu, pre, torch.autograd.grad(F.conv1d(gelu, wt), gelu, dyc, retain_graph=True)[0] + add)
    desc = ops.conv_desc(_lib.CONV_CAUSAL, 2, 64, 32, 50, 1)

    def run(wt, pre, dyc, add):          # add: the gradient arriving beside the conv's, ahead of the GELU derivative
        packed = ops.conv_pack_bwd(desc, wt)
        return [Out("dx", ops.conv_bwd_data_gelu(desc, dyc, packed, pre), want, 2e-5),
                Out("dx_add", ops.conv_bwd_data_gelu(desc, dyc, packed, pre, add=add), want_add, 2e-5)]
    return dict(wt=wt, pre=pre.detach(), dyc=dyc, add=add), run


def _grouped_case(name, cin, cout, k, s, g, pad, length, prefix):
    desc = ops.conv_desc(_lib.CONV_PADDED, 2, cin, cout, length, k, s, 1, 0, 0.2, 0, groups=g, padding=pad)

    def names():
        assert ops.conv_grouped_bwd_weight_kernel_name(desc).startswith(prefix), ops.conv_grouped_bwd_weight_kernel_name(desc)

    @case(name, names)
    def make():
        gen = torch.Generator().manual_seed(cin + k)
        x = F.leaky_relu(torch.randn(2, cin, length, generator=gen), 0.2).requires_grad_(True)
        w = (torch.randn(cout, cin // g, k, generator=gen) / (cin // g * k) ** 0.5).requires_grad_(True)
        b = torch.randn(cout, generator=gen).requires_grad_(True)
        sigma = torch.tensor([0.37])
        y = F.conv1d(x, w / sigma, b, stride=s, padding=pad, groups=g)
        dz, extra = torch.randn(y.shape, generator=gen), torch.randn(2, cin, length, generator=gen)
        gx, gw, gb = torch.autograd.grad(y, (x, w, b), dz)
        want_x = (gx + extra) * torch.where(x.detach() > 0, 1.0, 0.2)
        want_w = gw * sigma

        def run(x, w, bias, sigma, dz, extra):
            pk = ops.conv_pack_sigma(desc, w, sigma)
            pkb = ops.conv_pack_bwd_sigma(desc, w, sigma) if g == 1 else None
            y = ops.conv_forward(desc, x, pk, bias)
            dx = ops.conv_grouped_bwd_data(desc, dz, w, sigma, extra, x, 0.2)
            dw, db = ops.conv_grouped_bwd_weight(desc, x, dz)
            outs = [Out("y", y, y_want, _close(y_want, 1e-5)), Out("dx", dx, want_x, _close(want_x, 2e-5)),
                    Out("dw", dw, want_w, _close(want_w, 1e-4)), Out("dbias", db, gb, _close(gb, 2e-5))]
            if pkb is not None:
                outs.append(Out("dx_packed", ops.conv_bwd_data(desc, dz, pkb), gx, _rel(gx, 3e-5)))
            return outs
        y_want = y.detach()
        return dict(x=x.detach(), w=w.detach(), bias=b.detach(), sigma=sigma, dz=dz, extra=extra), run


_grouped_case("conv_grouped/tiled-16-64-g4", 16, 64, 41, 4, 4, 0, 300, "grouped_bwd_weight_tiled<")
_grouped_case("conv_grouped/simple-6-9-g3", 6, 9, 4, 3, 3, 2, 50, "grouped_bwd_weight op=")
_grouped_case("conv_grouped/dense-16-32-g1", 16, 32, 7, 2, 1, 5, 77, "grouped_bwd_weight op=")


# ------------------------------------------------------------------------------------------------ conv2d
def _conv2d_case(name, batch, cin, cout, kh, kw, sh, sw, ph, pw, h, w, impl, fwd, bwd, wgrad, few=False, b3=False):
    """Forward, backward-data (plain, add + mask), weight gradient (plain, spectral) of one Conv2d layer; ``fwd`` / ``bwd`` are
    the kernel names of the forward and backward-data ops (equality), ``wgrad`` the instantiation and operand copy of the weight
    gradient ("<kernel> op=<copy>").  ``b3``: the tolerances of tests/test_gpu_conv2d_b3.py (1e-5 of the largest magnitude)."""
    d = ops.conv2d_desc(batch, cin, cout, h, w, kh, kw, (sh, sw), (ph, pw), _lib.EPI_LEAKY_PRE, 0.2, impl)
    d0 = ops.conv2d_desc(batch, cin, cout, h, w, kh, kw, (sh, sw), (ph, pw), 0, 0.2, impl)

    def names():
        got = (ops.conv2d_kernel_name(d), ops.conv2d_bwd_data_kernel_name(d0), ops.conv2d_bwd_weight_kernel_name(d0))
        kernel, copy = wgrad.split(" op=")
        assert got[:2] == (fwd, bwd) and got[2].split(" ")[0] == kernel and f" op={copy} " in got[2], (got, fwd, bwd, wgrad)

    @case(name, names)
    def make():
        gen = torch.Generator().manual_seed(cin * 7 + kh)
        x32 = F.leaky_relu(torch.randn(batch, cin, h, w, generator=gen), 0.2)
        wt32 = torch.randn(cout, cin, kh, kw, generator=gen) / (cin * kh * kw) ** 0.5
        b32 = torch.randn(cout, generator=gen)
        u, v = F.normalize(torch.randn(cout, generator=gen), dim=0), F.normalize(torch.randn(cin * kh * kw, generator=gen), dim=0)
        sigma32 = torch.dot(u, torch.mv(wt32.reshape(cout, -1), v)).reshape(1)
        xin, wt, b = (t.double().requires_grad_(True) for t in (x32, wt32, b32))
        sigma = sigma32.double()
        y = F.conv2d(xin, wt, b, stride=(sh, sw), padding=(ph, pw))
        want_y = F.leaky_relu(y, 0.2).detach()
        dy, extra = torch.randn(y.shape, generator=gen), torch.randn(xin.shape, generator=gen)
        gx, gw, gb = torch.autograd.grad(y, (xin, wt, b), dy.double())
        want_masked = (gx + extra) * torch.where(x32 > 0, 1.0, 0.2)
        # spectrally normalised: sigma = u^T W v moves with the weight (tests/test_gpu_disc.py), gradient w.r.t. weight_orig
        sigma_w = torch.dot(u.double(), torch.mv(wt.reshape(cout, -1), v.double()))
        (gw_s,) = torch.autograd.grad(F.conv2d(xin.detach(), wt / sigma_w, b, stride=(sh, sw), padding=(ph, pw)), wt, dy.double())
        want_few = gx / sigma + extra
        if b3:
            def tol(want, _):
                return 1e-5 * float(want.abs().max())
        else:
            tol = _close                     # tests/test_gpu_disc.py

        def run(x, wt, bias, dy, extra, sigma, u, v):
            arena = _arena_of(x)
            outs = [Out("y", ops.conv2d_forward(d, x, ops.conv2d_pack(d, wt), bias), want_y, tol(want_y, 1e-5))]
            pk = ops.conv2d_pack_bwd(d0, wt)
            outs.append(Out("dx", ops.conv2d_bwd_data(d0, dy, pk), gx, tol(gx, 2e-5)))
            outs.append(Out("dx_add_mask", ops.conv2d_bwd_data(d0, dy, pk, x, 0.2, add=extra), want_masked, tol(want_masked, 2e-5)))
            ws_bytes = int(_lib.load().agx_conv2d_bwd_weight_workspace_bytes(ctypes.byref(d0)))
            n0 = len(arena.allocs)
            dw, db = ops.conv2d_bwd_weight(d0, x, dy)
            assert _empties(arena, n0, torch.uint8) == [ws_bytes], "workspace exactly the queried bytes"
            outs += [Out("dw", dw, gw, tol(gw, 1e-4)), Out("dbias", db, gb, tol(gb, 2e-5))]
            dws, _ = ops.conv2d_bwd_weight(d0, x, dy, wt, sigma, u, v, want_bias=False)
            outs.append(Out("dw_spectral", dws, gw_s, _close(gw_s, 1e-4)))
            if few:
                got = ops.conv2d_bwd_data_fewchannels(d0, dy, wt, sigma, extra)
                outs.append(Out("dx_fewchannels", got, want_few, _close(want_few, 2e-5)))
            return outs
        return dict(x=x32, wt=wt32, bias=b32, dy=dy, extra=extra, sigma=sigma32, u=u, v=v), run


_A, _SH4, _SH8, _ST8 = _lib.IMPL_AUTO, "conv2d_bwd_weight_shared<2,1,1,4>", "conv2d_bwd_weight_shared<2,2,2,2>", "conv2d_bwd_weight<1,1,1,4>"
# layers without a ring form: the direct, patch-tile, few-output and gather kernels
_conv2d_case("conv2d/direct-2-8", 2, 2, 8, 7, 7, 1, 1, 3, 3, 9, 64, _lib.IMPL_DIRECT, "conv_direct<16>", "conv_direct<4>", _ST8 + " op=none")
_conv2d_case("conv2d/first-2-32", 2, 2, 32, 7, 7, 1, 1, 3, 3, 21, 70, _A, "conv_mfma<1,1,1,4,16>", "conv_direct<4>", _ST8 + " op=none",
             few=True)
_conv2d_case("conv2d/mfma-16-32", 2, 16, 32, 3, 3, 1, 1, 1, 1, 5, 33, _lib.IMPL_MFMA, "conv_mfma<1,4,1,4,16>", "conv_direct<16>",
             _ST8 + " op=none")
_conv2d_case("conv2d/last-512-1", 2, 512, 1, 1, 8, 1, 1, 0, 3, 5, 16, _A, "conv2d_fewout<4>", "conv2d_bwd_data_gather", _ST8 + " op=none")
_conv2d_case("conv2d/odd-3-5", 2, 3, 5, 2, 2, 1, 1, 3, 2, 6, 7, _A, "conv_direct<16>", "conv2d_bwd_data_gather", _ST8 + " op=none")
# the ring kernel (csrc/conv_p.hip): the smallest row of each variant of tests/test_gpu_conv_p2d.py (forward and backward tables)
for _cin, _cout, _kh, _kw, _s2, _h, _w, _fwd, _bwd, _wg in (
        (64, 64, 3, 3, (1, 1), 5, 64, "conv_p2d<k3,64x256>", "conv_p2d<k3,64x256>", _SH4 + " op=none"),
        (128, 128, 3, 3, (1, 1), 6, 50, "conv_p2d<k3,128x128>", "conv_p2d<k3,128x128>", "conv2d_bwd_weight<2,2,2,2> op=none"),
        (32, 32, 3, 3, (1, 1), 9, 128, "conv_p2d<k3,32x512>", "conv_p2d<k3,32x512>", "conv2d_bwd_weight_direct<1,3,1,1> op=none"),
        (32, 64, 3, 4, (1, 2), 11, 128, "conv_p2d<k4s2,64x256>", "conv_p2d<bwd s(1,2),64x256>", _SH4 + " op=deinterleave"),
        (64, 128, 4, 4, (2, 2), 9, 60, "conv_p2d<k4s2,128x128>", "conv_p2d<bwd s(2,2),128x128>", _SH8 + " op=prepad"),
        (256, 256, 3, 4, (1, 2), 7, 64, "conv_p2d<k4s2,128x128>", "conv_p2d<bwd s(1,2),128x128>", _SH8 + " op=deinterleave")):
    _conv2d_case(f"conv2d/ring/{_cin}-{_cout}-{_kh}x{_kw}-{_h}x{_w}", 2, _cin, _cout, _kh, _kw, *_s2, (_kh - 1) // 2, 1, _h, _w, _A,
                 _fwd, _bwd, _wg)
# the bf16x3 ring kernel (csrc/conv_b3.hip): the smallest row of each variant of tests/test_gpu_conv2d_b3.py (SHAPES, STRIDED_FWD,
# STRIDED; a strided layer whose backward has no phase form runs the patch tiles there)
for _b, _cin, _cout, _h, _w, _kh, _kw, _sh, _sw, _fwd, _bwd, _wg in (
        (2, 32, 32, 37, 128, 3, 3, 1, 1, "3x3,32x256", "3x3,32x256", "conv2d_bwd_weight_direct<1,3,1,1> op=none"),
        (2, 32, 64, 21, 96, 3, 3, 1, 1, "3x3,64x256", "3x3,32x256", "conv2d_bwd_weight_shared<2,1,1,4,1> op=none"),
        (1, 64, 128, 19, 30, 3, 3, 1, 1, "3x3,128x128", "3x3,64x256", "conv2d_bwd_weight_shared<2,2,2,2,1> op=prepad"),
        (1, 128, 256, 15, 16, 3, 3, 1, 1, "3x3,128x128", "3x3,128x128", "conv2d_bwd_weight_shared<2,2,2,2,1> op=prepad"),
        (2, 32, 64, 21, 64, 3, 4, 1, 2, "3x4 s(1,2) as 3x2 s2d,64x256", None, "conv2d_bwd_weight_shared<2,1,1,4,1> op=deinterleave"),
        (2, 64, 128, 22, 64, 4, 4, 2, 2, "4x4 s2 as 2x2 s2d,128x128", None, "conv2d_bwd_weight_shared<2,2,2,2,1> op=deinterleave"),
        (2, 32, 64, 21, 62, 3, 4, 1, 2, "3x4 s(1,2) as 3x2 s2d,64x256", "3x2 phases 1x2,64x256",
         "conv2d_bwd_weight_shared<2,1,1,4,1> op=prepad"),
        (2, 64, 128, 22, 62, 4, 4, 2, 2, "4x4 s2 as 2x2 s2d,128x128", "2x2 phases 2x2,128x128",
         "conv2d_bwd_weight_shared<2,2,2,2,1> op=prepad"),
        (1, 128, 128, 17, 126, 3, 4, 1, 2, "3x4 s(1,2) as 3x2 s2d,128x128", "3x2 phases 1x2,128x128",
         "conv2d_bwd_weight<2,2,2,2,1> op=none")):
    _patch = "conv_mfma<2,2,1,4,16>" if _cout == 64 else "conv_mfma<2,2,2,2,16>"
    _conv2d_case(f"conv2d/bf16x3/{_cin}-{_cout}-{_kh}x{_kw}-{_h}x{_w}", _b, _cin, _cout, _kh, _kw, _sh, _sw, (_kh - 1) // 2,
                 (_kw - 1) // 2, _h, _w, _lib.IMPL_MFMA_BF16X3, f"conv2d_b3<{_fwd}>", f"conv2d_b3<{_bwd}>" if _bwd else _patch, _wg, b3=True)


# ------------------------------------------------------------------------------------------------ RVQ
def _rvq_case(name, b, t, d, k, q, seed, layout="b l c", sizes=None):
    @case(name)
    def make():
        gen = torch.Generator().manual_seed(seed)
        x = torch.randn(b, t, d, generator=gen)
        cbs = torch.randn(q, k, d, generator=gen)
        if sizes is not None:
            for i, kq in enumerate(sizes):
                cbs[i, kq:] = 0.0
        want_q, want_i, want_c = rvq.residual_quantize(x, cbs, sizes=sizes) if sizes is not None else rvq.residual_quantize(x, cbs)
        r, sq = x.double(), []
        for i in range(q):                                            # per-stage sums of squared residuals, float64
            r = r - cbs[i][want_i[..., i]].double()
            sq.append(float((r * r).sum()))
        sq = torch.tensor(sq, dtype=torch.float64)
        xin = x.transpose(1, 2).contiguous() if layout == "b c l" else x
        ws_bytes = int(_lib.load().agx_rvq_workspace_bytes(b, t, d, k, q))
        flat, r32 = want_i.reshape(-1, q), x.reshape(-1, d).clone()
        want_stats = torch.zeros(q, k, d + 1, dtype=torch.float64)     # counts (exact) | sums of the fp32 residuals, float64
        for i in range(q):
            want_stats[i, :, 0] = torch.bincount(flat[:, i], minlength=k).double()
            want_stats[i, :, 1:].index_add_(0, flat[:, i], r32.double())
            r32 = r32 - cbs[i][flat[:, i]]                             # fp32, stage order: what the kernel subtracts
        counts = int(want_stats[:, :, 0].max())

        def run(x, cbs):
            packed = ops.rvq_pack(cbs, sizes)
            n0 = len(_arena_of(x).allocs)
            xq, idx, sqe, commit = ops.rvq_forward(x, cbs, packed, q, layout)
            assert _empties(_arena_of(x), n0, torch.float64) == [8 * q + ws_bytes], "the f64 buffer is exactly q_used + workspace_bytes / 8"
            xq_blc = xq.transpose(1, 2) if layout == "b c l" else xq
            stats = ops.rvq_ema_stats(x.transpose(1, 2).reshape(-1, d) if layout == "b c l" else x.reshape(-1, d), cbs, idx.reshape(-1, q))
            return [Out("index", idx, want_i, exact=True), Out("x_q", xq_blc, want_q, exact=True),
                    # tests/test_gpu_parity.py: |commit - want| <= 1e-5 max(1, |want|), commit = sum(sq_err) / numel
                    Out("sq_err_sum_over_numel", sqe.sum().reshape(1) / x.numel(), sq.sum().reshape(1) / x.numel(), _rel(want_c, 1e-5)),
                    # the region ahead of the workspace, stage by stage, in the same units and form
                    Out("sq_err_over_numel", sqe / x.numel(), sq / x.numel(), _rel(sq / x.numel(), 1e-5)),
                    Out("commit", commit.reshape(1), want_c.reshape(1), _rel(want_c, 1e-5)),
                    Out("ema_counts", stats[:, :, 0], want_stats[:, :, 0], exact=True),
                    # tests/test_gpu_step.py: sums within 1e-6 * 4 * the largest count
                    Out("ema_sums", stats[:, :, 1:], want_stats[:, :, 1:], 4e-6 * counts)]
        return dict(x=xin, cbs=cbs), run


def _arena_of(t):
    """The arena a placed tensor lives in (the running case's), found through the routed module."""
    return ops.torch._arena


_rvq_case("rvq/one-frame", 1, 1, 8, 16, 1, seed=40)
_rvq_case("rvq/ragged-odd-D", 1, 37, 33, 100, 3, seed=5)
_rvq_case("rvq/ragged-channel-major", 2, 31, 64, 300, 4, seed=6, layout="b c l")
_rvq_case("rvq/K1024-partial-frame-tile", 1, 37, 64, 1024, 2, seed=41)
_rvq_case("rvq/K1024-channel-major", 2, 19, 64, 1024, 2, seed=42, layout="b c l")
_rvq_case("rvq/pack-sized", 1, 37, 64, 128, 3, seed=43, sizes=(128, 37, 100))


@case("rvq_dequantize")
def _dequant_case():
    gen = torch.Generator().manual_seed(44)
    cb = torch.randn(50, 24, generator=gen)
    idx = torch.randint(0, 50, (3, 7), generator=gen)
    acc = torch.randn(3, 7, 24, generator=gen)

    def run(cb, idx, acc):
        plain = ops.rvq_dequantize(cb, idx)
        both = ops.rvq_dequantize(cb, idx, out=acc, accumulate=True)
        assert both is acc
        return [Out("plain", plain, cb_cpu[idx_cpu], exact=True), Out("accumulated", both, acc_cpu + cb_cpu[idx_cpu], exact=True)]
    cb_cpu, idx_cpu, acc_cpu = cb, idx, acc
    return dict(cb=cb, idx=idx, acc=acc), run


# ------------------------------------------------------------------------------------------------ layernorm, attention
def _layernorm_case(t, c):
    @case(f"layernorm_ct/T{t}-C{c}")
    def make():
        gen = torch.Generator().manual_seed(t * 100 + c)
        x = torch.randn(3, c, t, generator=gen, requires_grad=True)
        w = (1 + 0.1 * torch.randn(c, generator=gen)).requires_grad_(True)
        b = torch.randn(c, generator=gen).requires_grad_(True)
        y = F.layer_norm(x.double().transpose(1, 2), (c,), w.double(), b.double(), 1e-5).transpose(1, 2)
        dy, extra = torch.randn(y.shape, generator=gen), torch.randn(y.shape, generator=gen)
        gx, gw, gb = torch.autograd.grad(y, (x, w, b), dy.double())
        want_dx = gx + extra
        ws_floats = 2 * 3 * ((t + 63) // 64) * c                     # include/agx.h: 2 * batch * ceil(t / 64) * channels floats

        def run(x, w, b, dy, extra):
            y_got = ops.layernorm_ct(x, w, b, 1e-5)
            n0 = len(_arena_of(x).allocs)
            dx, dw, db = ops.layernorm_ct_backward(x, w, dy, 1e-5, add=extra)
            assert _empties(_arena_of(x), n0, torch.float32) == sorted([4 * x.numel(), 4 * c, 4 * c, 4 * ws_floats]), \
                "dx, dweight, dbias and a workspace of exactly the header's formula"
            # tests/test_gpu_training.py: 2e-5 on dx, 1e-4 on dweight / dbias; tests/test_gpu_blocks.py: 2e-5 on y
            return [Out("y", y_got, y.detach(), 2e-5), Out("dx", dx, want_dx, 2e-5), Out("dweight", dw, gw, 1e-4),
                    Out("dbias", db, gb, 1e-4)]
        return dict(x=x.detach(), w=w.detach(), b=b.detach(), dy=dy, extra=extra), run


for _t in (1, 63, 64, 65):
    for _c in (5, 64):
        _layernorm_case(_t, _c)


def _attention_case(name, b, heads, dh, t, precision, flash, kernel):
    def names():
        got = ops.attention_kernel_name(b, heads, dh, t, precision, flash)
        assert got == kernel or (kernel.endswith("<") and got.startswith(kernel)), (got, kernel)

    @case(name, names)
    def make():
        qkv = 0.7 * torch.randn(b, 3 * heads * dh, t, generator=torch.Generator().manual_seed(t + dh))
        want = _core(qkv, heads, dh)
        scale = float(want.abs().max())
        tol = _rel(want, 3e-5) if precision == ops.ATTN_FP32 else BF16_MAX_REL * scale

        def run(qkv, slopes):
            return [Out("out", ops.attention_alibi(qkv, slopes, heads, dh, dh ** 0.5, precision=precision, flash=flash), want, tol)]
        return dict(qkv=qkv, slopes=oattn.alibi_slopes(heads)), run


for _t, _dh, _prec, _kernel in ATTENTION_ROWS:                      # each of the eighteen rows of the forward tables
    _attention_case(f"attention/{_kernel}-T{_t}-Dh{_dh}", 1, 2, _dh, _t, _prec, False, _kernel)
for _t, _dh, _flash, _prec in ((1, 16, False, 0), (33, 20, False, 0), (256, 64, False, 0), (256, 128, True, 0), (257, 16, False, 0),
                               (300, 20, False, 0), (300, 128, False, 0), (33, 64, True, 0), (1, 20, True, 0), (300, 64, False, 1),
                               (33, 16, False, 1)):
    _family = "attention_bf16_lds<" if _prec else ("attention_flash<" if _flash or _t > 256 else "attention_alibi<")
    _attention_case(f"attention/T{_t}-Dh{_dh}-{'flash' if _flash else 'auto'}-{'bf16' if _prec else 'fp32'}", 2, 3, _dh, _t, _prec,
                    _flash, _family)


def _attention_bwd_case(name, b, heads, dh, t, split, kernel_prefix):
    def names():
        assert ops.attention_backward_kernel_name(heads, dh, t, split).startswith(kernel_prefix), \
            ops.attention_backward_kernel_name(heads, dh, t, split)

    @case(name, names)
    def make():
        g = torch.Generator().manual_seed(t * 7 + dh)
        qkv = (0.5 * torch.randn(b, 3 * heads * dh, t, generator=g)).double().requires_grad_(True)
        q, k, v = (z.reshape(b, heads, dh, t) for z in qkv.chunk(3, dim=1))
        s = torch.einsum("bhdi,bhdj->bhij", q, k) / dh ** 0.5 + oattn.alibi_bias(heads, t, t).double()
        o = torch.einsum("bhij,bhdj->bhdi", s.softmax(-1), v).reshape(b, heads * dh, t)
        do = torch.randn(o.shape, generator=g)
        (want,) = torch.autograd.grad(o, qkv, do.double())
        nbytes = 2 * b * heads * t * 4

        def run(qkv, slopes, out, do):
            if not split:
                got = ops.attention_alibi_backward(qkv, slopes, do, heads, dh, dh ** 0.5)
            else:                       # the split path with exactly the queried workspace, whatever the single launch covers
                lib = _lib.load()
                assert int(lib.agx_attention_backward_workspace_bytes(b, heads, t)) == nbytes
                ws = ops._workspace(nbytes, qkv.device, "agx_attention_backward_workspace_bytes")
                got = ops.torch.empty_like(qkv)
                _lib.check(lib.agx_attention_alibi_backward_ex(ops._ptr(qkv), ops._ptr(slopes), ops._ptr(out), ops._ptr(do),
                                                               ops._ptr(got), ops._ptr(ws), nbytes, b, heads, dh, t, dh ** 0.5,
                                                               ops._stream()), "agx_attention_alibi_backward_ex")
                if t > 256 or dh > 64:
                    via = ops.attention_alibi_backward(qkv, slopes, do, heads, dh, dh ** 0.5, out=out)
                    assert torch.equal(via, got)
            return [Out("dqkv", got, want, _rel(want, 5e-5))]
        return dict(qkv=qkv.detach().float(), slopes=oattn.alibi_slopes(heads), out=o.detach().float(), do=do), run


_attention_bwd_case("attention_backward/single<16>", 2, 2, 64, 40, False, "attention_alibi_bwd<16>")
_attention_bwd_case("attention_backward/single<8>", 1, 2, 64, 256, False, "attention_alibi_bwd<8>")       # K, V, dS beyond 150 KiB at 16 queries
for _t, _dh in ((1, 8), (200, 128), (257, 16)):
    _attention_bwd_case(f"attention_backward/ex-T{_t}-Dh{_dh}", 2, 2, _dh, _t, True, "attn_bwd_stats+attn_bwd_dq+attn_bwd_dkv")


# ------------------------------------------------------------------------------------------------ wavelets
def _multires_case(c, k, depth, length):
    @case(f"multires/C{c}-K{k}-depth{depth}-L{length}")
    def make():
        gen = torch.Generator().manual_seed(depth)
        h0, h1 = ((torch.randn(c, 1, k, generator=gen) / k ** 0.5).requires_grad_(True) for _ in range(2))
        w = (torch.randn(c, depth + 2, generator=gen) / (depth + 2) ** 0.5).requires_grad_(True)
        x = torch.randn(2, c, length, generator=gen, requires_grad=True)
        want = owv.multires_conv(x, h0, h1, w, depth)
        dout = torch.randn(want.shape, generator=gen)
        grads = torch.autograd.grad(want, (x, h0, h1, w), dout)
        ws_bytes = int(_lib.load().agx_multires_backward_workspace_bytes(2, c, length, k, depth))

        def run(x, h0, h1, w, dout):
            outs = [Out("y", ops.multires_forward(x, h0, h1, w, depth), want.detach(), 1e-5)]       # tests/test_gpu_blocks.py
            n0 = len(_arena_of(x).allocs)
            got = ops.multires_backward(x, dout, h0, h1, w, depth)
            assert _empties(_arena_of(x), n0, torch.uint8) == [ws_bytes], "workspace exactly the queried bytes"
            # tests/test_gpu_blocks.py: 2e-5 max(1, |dx|) on the input, 1e-4 max(1, |ref|) on every parameter
            for nm, g_got, g_want, tol in zip(("dx", "dh0", "dh1", "dw"), got, grads, (2e-5, 1e-4, 1e-4, 1e-4)):
                outs.append(Out(nm, g_got, g_want, _rel(g_want, tol)))
            return outs
        return dict(x=x.detach(), h0=h0.detach(), h1=h1.detach(), w=w.detach(), dout=dout), run


_multires_case(3, 2, 1, 77)
_multires_case(5, 13, 4, 1500)


def _fold_case(channelwise, scale, n_points, length):
    @case(f"wavelet_fold/{'channelwise' if channelwise else 'shared'}-s{scale}-P{n_points}-L{length}")
    def make():
        gen = torch.Generator().manual_seed(scale * 10 + length)
        b, c = 3, 6
        h = torch.randn(b, c, length, generator=gen, requires_grad=True)
        space = torch.linspace(-10, 10, n_points)
        sigma = (40.0 + 5 * torch.rand(1, c, 1, 1, generator=gen) if channelwise else torch.tensor(33.0)).requires_grad_(True)
        dout = torch.randn(b, c, length * scale, generator=gen)
        gh, gs = torch.autograd.grad(owv.wavelet_fold(h, space, sigma, scale), (h, sigma), dout)

        want_y = owv.wavelet_fold(h, space, sigma, scale).detach()

        def run(h, dout, space, sigma):
            dh, dsig = ops.wavelet_fold_backward(h, dout, space, sigma, scale)
            # y: the 1e-5 of the wavelet layers in tests/test_gpu_blocks.py; gradients: tests/test_gpu_backward.py
            return [Out("y", ops.wavelet_fold(h, space, sigma, scale), want_y, 1e-5), Out("dh", dh, gh, 1e-5 * float(gh.abs().max()) + 1e-12), Out("dsigma", dsig, gs, 1e-4 * float(gs.abs().max()) + 1e-9)]
        return dict(h=h.detach(), dout=dout, space=space, sigma=sigma.detach()), run


for _cw in (True, False):
    for _scale, _points, _length in ((2, 16, 37), (5, 40, 300), (4, 8, 1), (1, 4, 19)):
        _fold_case(_cw, _scale, _points, _length)


@case("group_sum")
def _group_sum_case():
    gen = torch.Generator().manual_seed(8)
    g = torch.randn(2, 6, 5 * 77, generator=gen)
    pre = torch.randn(2, 6, 77, generator=gen, requires_grad=True)
    plain = g.double().reshape(2, 6, 77, 5).sum(-1)
    (fused,) = torch.autograd.grad(F.gelu(pre.double()), pre, plain)           # the sum times the exact-GELU derivative at pre

    def run(g, pre):             # part of the scale block's input gradient: 2e-5 max(1, |ref|), tests/test_gpu_blocks.py
        return [Out("plain", ops.group_sum(g, 5), plain, _rel(plain, 2e-5)),
                Out("gelu_pre", ops.group_sum(g, 5, gelu_pre=pre), fused, _rel(fused, 2e-5))]
    return dict(g=g, pre=pre.detach()), run


# ------------------------------------------------------------------------------------------------ discriminator ops
def _sigma_case(shape, n_iter):
    @case(f"spectral_sigma/{'x'.join(map(str, shape))}-iter{n_iter}")
    def make():
        gen = torch.Generator().manual_seed(len(shape) + n_iter)
        w = torch.randn(*shape, generator=gen)
        rows, cols = shape[0], w.numel() // shape[0]
        u, v = F.normalize(torch.randn(rows, generator=gen), dim=0), F.normalize(torch.randn(cols, generator=gen), dim=0)
        sd = {"weight_orig": w, "weight_u": u.clone(), "weight_v": v.clone()}
        wn = od.spectral_weight(sd, "", train=n_iter > 0)
        sigma_want = (w / wn).flatten()[:1].clone()
        gn = torch.randn(*shape, generator=gen)
        w2 = w.clone().requires_grad_(True)
        sg2 = torch.dot(sd["weight_u"], torch.mv(w2.reshape(rows, -1), sd["weight_v"]))
        (want_grad,) = torch.autograd.grad(w2 / sg2, w2, gn)

        def run(w, u, v, gn, sigma_ref, u_ref, v_ref):
            sigma = ops.spectral_sigma(w, u, v, n_iter)                   # u / v are in/out: initialised above, compared below
            grad = ops.spectral_grad_(gn, w, sigma_ref, u_ref, v_ref)     # in place on gn
            return [Out("sigma", sigma, sigma_want, 2e-5 * abs(float(sigma_want)) + 1e-7),
                    Out("u", u, sd["weight_u"], _close(sd["weight_u"], 2e-5)), Out("v", v, sd["weight_v"], _close(sd["weight_v"], 2e-5)),
                    Out("spectral_grad", grad, want_grad, _close(want_grad, 1e-5))]
        return dict(w=w, u=u, v=v, gn=gn, sigma_ref=sg2.detach().reshape(1), u_ref=sd["weight_u"].clone(),
                    v_ref=sd["weight_v"].clone()), run


_sigma_case((16, 1, 15), 0)
_sigma_case((16, 1, 15), 1)
_sigma_case((4, 2, 7, 7), 1)
_sigma_case((1, 512, 1, 8), 0)


def _reduce_case(n):
    @case(f"reduce_mean_feature_means/n{n}")
    def make():
        gen = torch.Generator().manual_seed(n % 1000)
        x, y = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        xd, yd = x.double(), y.double()
        refs = {ops.REDUCE_MEAN: xd, ops.REDUCE_HINGE_REAL: torch.clamp(xd - 1, max=0), ops.REDUCE_HINGE_FAKE: torch.clamp(-xd - 1, max=0),
                ops.REDUCE_L1: (xd - yd).abs(), ops.REDUCE_ABS_EPS: (x + 1e-3).double().abs()}
        refs = {m: r.mean().reshape(1) for m, r in refs.items()}
        inv = float(torch.tensor(1.0 / n, dtype=torch.float64).float())
        grad = torch.tensor([0.75])
        want_dx = torch.sign(x - y) * torch.tensor(0.75) * inv
        # d mean|x - y| and d mean|x + 1e-3|, weighted by the two arriving gradients (float64)
        want_fy = -0.37 * torch.sign(x - y).double() / n
        want_fx = -want_fy - 1.9 * torch.sign(x + 1e-3).double() / n

        def run(x, y, grad, grad2):
            outs = []
            for m, ref in refs.items():          # tests/test_gpu_disc.py: 2e-6 max(1, |ref|) + 2e-7
                out = ops.reduce_mean(x, m, y if m == ops.REDUCE_L1 else None)
                outs.append(Out(f"mean[mode {m}]", out.reshape(1), ref, 2e-6 * max(1.0, abs(float(ref))) + 2e-7))
            pair = ops.feature_means(x, y)
            outs.append(Out("feature_means", pair, torch.cat([refs[ops.REDUCE_L1], refs[ops.REDUCE_ABS_EPS]]),
                            2e-6 * max(1.0, float(refs[ops.REDUCE_L1])) + 2e-7))
            if n <= 5000:
                dx, dy = ops.reduce_mean_backward(x, ops.REDUCE_L1, grad, y, True)
                # rtol 1e-6 of tests/test_gpu_disc.py, on values of magnitude 0.75 / n
                outs += [Out("dx", dx, want_dx, 1e-6 * 0.75 * inv), Out("dy", dy, -want_dx, 1e-6 * 0.75 * inv)]
                fx, fy = ops.feature_means_backward(x, y, grad2)
                # tests/test_gpu_disc.py: bit for bit the sum of the two separate means' gradients; values at the same rtol 1e-6
                dx1, dy1 = ops.reduce_mean_backward(x, ops.REDUCE_L1, grad2[0:1].clone(), y, True)
                dx2, _ = ops.reduce_mean_backward(x, ops.REDUCE_ABS_EPS, grad2[1:2].clone())
                assert torch.equal(fx, dx1 + dx2) and torch.equal(fy, dy1)
                outs += [Out("feature_dx", fx, want_fx, 1e-6 * (0.37 + 1.9) * inv), Out("feature_dy", fy, want_fy, 1e-6 * 0.37 * inv)]
            return outs
        return dict(x=x, y=y, grad=grad, grad2=torch.tensor([0.37, -1.9])), run


for _n in (1, 4095, 4097, 4096 * 1024 + 5):
    _reduce_case(_n)


@case("avgpool1d_sigmoid")
def _small_disc_case():
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(3, 2, 101, generator=gen, requires_grad=True)
    y = F.avg_pool1d(x, 4, stride=2, padding=2)
    dy, extra = torch.randn(y.shape, generator=gen), torch.randn(3, 2, 101, generator=gen)
    (gx,) = torch.autograd.grad(y, x, dy)
    want_pool_dx = gx + extra
    z = torch.randn(4, 1, 77, generator=gen, requires_grad=True)
    s = torch.sigmoid(z)
    ds = torch.randn(s.shape, generator=gen)
    (gz,) = torch.autograd.grad(s, z, ds)
    want_s = s.detach()

    def run(x, dy, extra, z, s, ds):
        return [Out("avgpool", ops.avgpool1d(x, 4, 2, 2), y.detach(), _close(y, 1e-6)),
                Out("avgpool_backward", ops.avgpool1d_backward(dy, 101, 4, 2, 2, add=extra), want_pool_dx, _close(want_pool_dx, 1e-6)),
                Out("sigmoid", ops.sigmoid(z), want_s, _close(want_s, 1e-6)),
                Out("sigmoid_backward", ops.sigmoid_backward(ds, s), gz, _close(gz, 1e-6))]
    return dict(x=x.detach(), dy=dy, extra=extra, z=z.detach(), s=s.detach(), ds=ds), run


# ------------------------------------------------------------------------------------------------ spectral
def _stft_case(n_fft, length):
    @case(f"stft/n_fft{n_fft}-L{length}")
    def make():
        gen = torch.Generator().manual_seed(n_fft)
        x = (0.3 * torch.randn(2, length, generator=gen)).requires_grad_(True)
        y = od.stft_two_sided(x, n_fft, n_fft // 4)
        dy = torch.randn(y.shape, generator=gen)
        (gx,) = torch.autograd.grad(y, x, dy)
        ws_bytes = int(_lib.load().agx_stft_workspace_bytes(2, length, n_fft))

        def run(x, dy):
            arena = _arena_of(x)
            n0 = len(arena.allocs)
            got = ops.stft(x, n_fft, True)
            assert _empties(arena, n0, torch.uint8) == [ws_bytes], "workspace exactly the queried bytes"
            back = ops.stft_backward(dy, length, n_fft, True)
            return [Out("y", got, y.detach(), _close(y, 2e-5)), Out("dx", back, gx, _close(gx, 2e-5))]      # tests/test_gpu_disc.py
        return dict(x=x.detach(), dy=dy), run


# agx_stft_* takes powers of two >= 64 only (the framed DFT behind the mel spectrogram, below, runs n_fft = 32 and 400)
_stft_case(64, 203)       # 203 = 12 hops of 16 + 11: a partial last frame
_stft_case(256, 1234)


def _mel_case(n_fft, win, hop, length):
    @case(f"fdft_melpower/n_fft{n_fft}-win{win}-hop{hop}-L{length}")
    def make():
        gen = torch.Generator().manual_seed(n_fft + win)
        x = (0.2 * torch.randn(2, length, generator=gen)).double().requires_grad_(True)
        w = torch.hann_window(win, periodic=True, dtype=torch.float64)
        st = torch.stft(x, n_fft, hop, win, window=w, center=True, pad_mode="reflect", normalized=False, return_complex=True)
        fb = osg.mel_fbanks(n_fft // 2 + 1, 24000, 40)
        want = torch.einsum("bft,fm->bmt", (st.real ** 2 + st.imag ** 2) / float((w * w).sum()), fb.double())
        g = torch.randn(want.shape, generator=gen, dtype=torch.float64)
        (gx,) = torch.autograd.grad(want, x, g)
        spec = sg.MelSpectrogram(24000, n_fft, win, hop, 40, True)

        def run(x, g, fb):
            spec._img.clear()                                          # the packed images are arena allocations of this run
            spec.fb = fb                                               # the filter bank is an input: placed like the others
            cv, mel = spec._forward_raw(x)
            dx = spec._backward_raw(cv, g, length)
            # tests/test_gpu_signal.py: close(..., 5e-5), floor 1e-9
            return [Out("mel", mel, want.detach(), _close(want, 5e-5, 1e-9)), Out("dx", dx, gx, _close(gx, 5e-5, 1e-9)),
                    Out("cv", cv, cv.detach().cpu(), exact=True)]
        return dict(x=x.detach().float(), g=g.float(), fb=sg.melscale_fbanks(n_fft // 2 + 1, 24000, 40)), run


_mel_case(32, 32, 8, 203)
_mel_case(400, 100, 25, 1234)


@case("preemphasis_biquad_resample")
def _signal_case():
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(3, 1, 1000, generator=gen, requires_grad=True)
    y = osg.preemphasis(x, 0.97)
    dy = torch.randn(y.shape, generator=gen)
    (gx,) = torch.autograd.grad(y, x, dy)
    clip = (0.5 * torch.randn(4, 1, 3000, generator=gen)).clamp(-1, 1)
    low = osg.lowpass_biquad(clip, 24000, 800.0)
    wave = torch.randn(2, 1, 1234, generator=gen)
    res = osg.resample(wave, 44100, 24000)
    mod = sg.Resample(44100, 24000)

    def run(x, dy, clip, wave, table):
        mod.kernel = table
        return [Out("preemphasis", sg._preemph_raw(x, 0.97, 0), y.detach(), _close(y, 1e-6, 1e-9)),       # tests/test_gpu_signal.py
                Out("preemphasis_adjoint", sg._preemph_raw(dy, 0.97, 1), gx, _close(gx, 1e-6, 1e-9)),
                Out("lowpass_biquad", sg.lowpass_biquad(clip, 24000, 800.0), low, _close(low, 2e-5, 1e-9)),
                Out("resample", mod(wave), res, _close(res, 2e-6, 1e-9))]
    return dict(x=x.detach(), dy=dy, clip=clip, wave=wave, table=mod.kernel.clone()), run


# ------------------------------------------------------------------------------------------------ bitstream, time folding
def _codes_case(bits, n):
    @case(f"codes/bits{bits}-n{n}")
    def make():
        codes = torch.randint(0, 2 ** bits, (n,), generator=torch.Generator().manual_seed(bits * 1000 + n))
        want = torch.from_numpy(bitstream.pack(codes.numpy(), bits).astype(np.uint8))

        def run(codes):
            packed = ops.codes_pack(codes, bits)
            return [Out("packed", packed, want, exact=True), Out("unpacked", ops.codes_unpack(packed, n, bits), codes_cpu, exact=True)]
        codes_cpu = codes
        return dict(codes=codes), run


for _bits, _n in ((10, 7), (9, 1001), (1, 64), (16, 33)):
    _codes_case(_bits, _n)


def _fold_unfold_case(c, b, length, s, hop, w, off):
    @case(f"time_fold/C{c}-B{b}-L{length}-S{s}-hop{hop}-W{w}-off{off}")
    def make():
        gen = torch.Generator().manual_seed(c)
        x = torch.randn(b, c, length, generator=gen)
        folded = torch.stack([x[:, :, off + i * hop: off + i * hop + w] for i in range(s)], dim=1).reshape(b * s, c, w)
        keep = hop if hop else w - 2
        src_off, dst_off = min((w - keep) // 2 + 1, w - keep), 3
        out_len = dst_off + s * keep + 11
        out0 = torch.randn(b, c, out_len, generator=gen)             # in/out: what is not placed must survive
        want = out0.clone()
        g4 = folded.reshape(b, s, c, w)
        for i in range(s):
            want[:, :, dst_off + i * keep: dst_off + (i + 1) * keep] = g4[:, i, :, src_off:src_off + keep]

        def run(x, out):
            got = ops.time_fold(x, s, hop, w, off)
            assert ops.time_unfold(got, out, s, keep, src_off, dst_off) is out
            return [Out("folded", got, folded, exact=True), Out("unfolded", out, want, exact=True)]
        return dict(x=x, out=out0), run


for _c, _rows in ((2, ((2, 101, 4, 17, 33, 5), (3, 67, 1, 0, 29, 38))), (512, ((1, 225, 6, 32, 54, 0), (2, 64, 3, 8, 48, 0)))):
    for _row in _rows:
        _fold_unfold_case(_c, *_row)


# ------------------------------------------------------------------------------------------------ the test
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_memory_contract(name):
    one_run, names, _ = CASES[name]
    if names is not None:
        names()
    report = run_contract(one_run, DEV)
    assert set(report["irreproducible"]) == set(NOT_REPRODUCIBLE.get(name, ())), \
        f"{name}: buffers that differ between two runs on clean memory (largest difference): {report['irreproducible']}"


def _assert_placed_as_asked(name, arena):
    """A case cannot pass by not being skewed: every placement of a run sits where the run's schedule puts it."""
    placed = [a for a in arena.allocs if a.what == "place"]
    assert placed, f"{name}: the case places no operand"
    for i, a in enumerate(placed):
        asked = arena.skews[i % len(arena.skews)]
        # float32, bfloat16 and uint8 get the run's skew as it is; the only placements that may stay behind it are the 8-byte
        # types (int64, float64), which cannot start 4 bytes off their item size
        want = asked // 8 * 8 if a.dtype in (torch.int64, torch.float64) else asked
        assert a.asked == asked and a.skew == want, f"{name}: {a.describe()} was asked {a.asked} and got {a.skew}, the run says {asked}"
    return any(a.skew for a in placed)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_operand_placement(name):
    one_run, names, _ = CASES[name]
    if names is not None:
        names()
    skewed = []

    def watched(arena):
        outs = one_run(arena)
        if any(arena.skews):
            skewed.append(_assert_placed_as_asked(name, arena))
        return outs
    report = run_contract(watched, DEV, PLACEMENT_RUNS, irreproducible=tuple(PLACEMENT_DEPENDENT.get(name, ())))
    assert len(skewed) == len(PLACEMENT_RUNS) - 1 and any(skewed), f"{name}: no operand was ever off alignment"
    # only a case whose every operand is an 8-byte type has a run (skew 4) in which nothing moves
    assert all(skewed) or name.split("/")[0] in ("codes",), f"{name}: runs without a skewed operand: {skewed}"
    assert set(report["irreproducible"]) <= set(PLACEMENT_DEPENDENT.get(name, ()))


def test_the_table_covers_every_family():
    """Host-only: the case table is what the file's docstring promises (no GPU needed to notice a family dropping out)."""
    families = {n.split("/")[0] for n in CASES}
    assert families >= {"conv_forward", "conv_forward_planes", "resblock_forward", "conv_bwd", "conv_bwd_data_gelu", "conv_grouped",
                        "conv2d", "rvq", "rvq_dequantize", "layernorm_ct", "attention", "attention_backward", "multires", "group_sum",
                        "wavelet_fold", "spectral_sigma", "reduce_mean_feature_means", "avgpool1d_sigmoid", "stft",
                        "fdft_melpower", "preemphasis_biquad_resample", "codes", "time_fold"}
    for name, (_, names, _) in CASES.items():
        if names is not None:
            names()
