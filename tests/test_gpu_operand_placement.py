"""Operands that do not start on a 16-byte boundary, at the entry points users call: a crop of a waveform
(``wave[s:s + L].view(1, 1, L)`` is contiguous and starts ``4 s`` bytes into its allocation), an ``out=`` carved out of a flat
buffer, and the second launch of a row loop.  include/agx.h: operands need 4-byte alignment only and the result does not
depend on it -- so every comparison here is bit for bit against the same call on ``.clone()``d (aligned) operands.
tests/test_gpu_memory_contract.py::test_operand_placement runs the kernel table the same way between guard bands."""
import ctypes

import numpy as np
import pytest
import torch

from audio_generation_amd import _lib, ops
from audio_generation_amd import signal_ops as sg
from audio_generation_amd.ops import AgxError
from audio_generation_amd.vae import CausalVQAE
from tests import signal_ref as ref
from tests.test_gpu_signal import close

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0x7FC0BEEF                      # a NaN with a payload: an activation of real numbers is never this


def test_a_crop_of_a_waveform_gives_the_bits_of_its_copy():
    torch.manual_seed(0)
    model = CausalVQAE(in_channels=1, n_blocks=2, strides=(2, 3), codebook_dim=16, num_quantizers=2, codebook_size=32,
                       wavelet_decoders=False, input_format="n c l").eval().to(DEV)
    length, dim = 480, 16                                             # a multiple of 4 and of the scale factor 6
    frames = length // 6
    # the layers a crop reaches read and write float4 because L % 4 == 0, whatever the pointer
    assert ops.conv_kernel_name(model.encoders[0][1].desc((1, 1, length))).startswith("conv_narrow<")
    assert ops.conv_kernel_name(model.decoders[-1].desc((1, 32, length))).startswith("conv_narrow<")
    gen = torch.Generator().manual_seed(1)
    wave = (0.1 * torch.randn(length + 3, generator=gen)).to(DEV)
    flat = torch.randn(dim * frames + 3, generator=gen).to(DEV)
    assert wave.data_ptr() % 16 == 0 and flat.data_ptr() % 16 == 0
    seen = set()
    with torch.no_grad():
        for s in range(4):
            x = wave[s:s + length].view(1, 1, length)
            assert x.is_contiguous() and x.data_ptr() % 16 == (wave.data_ptr() + 4 * s) % 16 == 4 * s
            y, _, index = model(x)
            y_ref, _, index_ref = model(x.clone())
            assert torch.equal(y, y_ref) and torch.equal(index, index_ref), s
            assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
            zq = flat[s:s + dim * frames].view(1, dim, frames)
            assert zq.is_contiguous() and zq.data_ptr() % 16 == 4 * s
            out = model.decode(zq)
            assert torch.equal(out, model.decode(zq.clone())), s
            assert tuple(out.shape) == (1, 1, length) and bool(torch.isfinite(out).all())
            seen.add(x.data_ptr() % 16)
    assert seen == {0, 4, 8, 12}


def _carved(shape, off):
    """A contiguous float32 tensor of ``shape`` that starts ``off`` bytes past a 16-byte boundary inside a flat buffer: NaN
    inside, a band of POISON on both sides that ends at its first and begins after its last element."""
    n, band = int(np.prod(shape)), 4096
    buf = torch.full((2 * band + n + 4,), float("nan"), device=DEV)
    bits = buf.view(torch.int32)
    lo = band + off // 4
    bits[:lo] = POISON
    bits[lo + n:] = POISON
    out = buf[lo:lo + n].view(shape)
    assert buf.data_ptr() % 16 == 0 and out.data_ptr() % 16 == off and out.is_contiguous()
    return out, bits, lo, n


@pytest.mark.parametrize("kind,cin,cout,k,s,b,length,kernel", [
    (_lib.CONV_UPSAMPLE, 128, 64, 9, 4, 2, 132, "conv_p<up4,"),        # a ring layer with 16-byte phase stores
    (_lib.CONV_CAUSAL, 32, 1, 7, 1, 2, 700, "conv_narrow<")])          # the last layer of every codec: float4 stores
def test_out_carved_from_a_flat_buffer(kind, cin, cout, k, s, b, length, kernel):
    desc = ops.conv_desc(kind, b, cin, cout, length, k, s, 1, _lib.EPI_LEAKY_PRE, 0.1)
    assert ops.conv_kernel_name(desc).startswith(kernel), ops.conv_kernel_name(desc)
    gen = torch.Generator().manual_seed(cin + k)
    v = (torch.randn(cout, cin, k, generator=gen) / (cin * k) ** 0.5).to(DEV)
    g = (torch.rand(cout, 1, 1, generator=gen) + 0.5).to(DEV)
    bias = (0.1 * torch.randn(cout, generator=gen)).to(DEV)
    x = torch.randn(b, cin, length, generator=gen).to(DEV)
    packed = ops.conv_pack(desc, v, g)
    want = ops.conv_forward(desc, x, packed, bias)
    assert want.data_ptr() % 16 == 0 and bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    for off in (4, 8, 12):
        out, bits, lo, n = _carved(tuple(want.shape), off)
        assert ops.conv_forward(desc, x, packed, bias, out=out) is out
        torch.cuda.synchronize()
        assert bool((bits[:lo] == POISON).all()) and bool((bits[lo + n:] == POISON).all()), off
        assert not bool(torch.isnan(out).any()), off                  # every element written
        assert torch.equal(out, want), off


def test_second_launch_of_the_resampler_row_loop():
    """The row index rides on grid.y, so ``Resample`` steps through its rows by 65535; the second launch starts
    65535 * 33 floats into x (12 bytes off alignment) and 65535 * 22 floats into y (8 bytes off)."""
    rows, length = 65537, 33
    mod = sg.Resample(3, 2).to(DEV)
    x = torch.randn(rows, length, generator=torch.Generator().manual_seed(33)).to(DEV)
    assert x.data_ptr() % 16 == 0 and (65535 * length * 4) % 16 == 12
    got = mod(x)
    out_len = ref.resample_out_len(length, mod.of, mod.nf)
    assert tuple(got.shape) == (rows, out_len) and (65535 * out_len * 4) % 16 == 8
    ends = [0, 1, rows - 2, rows - 1]
    want = ref.resample_f64(x[ends].cpu().numpy(), mod.kernel.cpu().numpy(), mod.of, mod.nf, mod.width)
    close(got[ends].double(), torch.from_numpy(want), 2e-6)             # tests/test_gpu_signal.py: test_resample
    tail = x[rows - 2:]
    assert tail.data_ptr() % 16 == 12
    assert torch.equal(got[rows - 2:], mod(tail.clone()))             # the two rows of the second launch, resampled alone
    assert torch.equal(got[:2], mod(x[:2].clone()))


def test_conv_wrapper_refusals_precede_the_launch():
    """An image that is too short is an over-read no guard band can see: the wrappers compare every image with the
    library's size query, every bias with c_out and ``out`` with what the layer writes, before anything is launched."""
    b, c, length = 2, 32, 64
    desc = ops.conv_desc(_lib.CONV_CAUSAL, b, c, c, length, 7, 1, 3)
    d2 = ops.conv_desc(_lib.CONV_CAUSAL, b, c, c, length, 1)
    gen = torch.Generator().manual_seed(7)
    v1, v2 = (torch.randn(c, c, k, generator=gen).to(DEV) / (c * k) ** 0.5 for k in (7, 1))
    bias = torch.zeros(c, device=DEV)
    x = torch.randn(b, c, length, generator=gen).to(DEV)
    p1, p2, pb = ops.conv_pack(desc, v1), ops.conv_pack(d2, v2), ops.conv_pack_bwd(desc, v1)
    lib = _lib.load()
    assert p1.numel() == lib.agx_conv_packed_floats(ctypes.byref(desc)) != p2.numel()
    assert pb.numel() == lib.agx_conv_bwd_packed_floats(ctypes.byref(desc)) != p1.numel()
    out = torch.full((b, c, length), 7.0, device=DEV)
    wide = torch.full((b, c, 2 * length), 7.0, device=DEV)
    short, odd = p1[:-1], torch.zeros(c + 1, device=DEV)
    for bad in (dict(packed=short), dict(packed=p2), dict(packed=p1.double()), dict(packed=torch.cat([p1, p1])[::2]), dict(bias=odd),
                dict(bias=bias[:1]), dict(out=out[:1]), dict(out=out.double()), dict(out=out.cpu()), dict(out=wide[:, :, ::2]),
                dict(out=out.view(b, length, c)), dict(out=wide)):
        args = dict(packed=p1, bias=bias, out=out)
        args.update(bad)
        with pytest.raises(AgxError):
            ops.conv_forward(desc, x, args["packed"], args["bias"], out=args["out"])
    assert ops.resblock_q4_supported(desc)
    for block in (ops.resblock_forward, ops.resblock_forward_q4):
        for packed1, bias1, packed2, bias2 in ((short, bias, p2, bias), (p1, bias, p2[:-1], bias), (p2, bias, p1, bias),
                                               (p1, odd, p2, bias), (p1, bias, p2, odd), (p1, bias, p2.double(), bias)):
            with pytest.raises(AgxError):
                block(desc, x, packed1, bias1, packed2, bias2)
    for packed in (pb[:-1], p1, pb.double()):
        with pytest.raises(AgxError):
            ops.conv_bwd_data(desc, x, packed)
    for xs, dys, vs in ((x[:1], x, v1), (x, x[:, :, :-1], v1), (x, x, v2), (x, x, v1.transpose(0, 1)[:, :-1]), (x[:, :-1], x, v1)):
        with pytest.raises(AgxError):
            ops.conv_bwd_weight(desc, xs, dys, vs, None)
    # the planes entry point: a bf16x3 ring layer
    d3 = ops.conv_desc(_lib.CONV_TRANSPOSED, b, 512, 512, 16, 7, 1, 1, _lib.EPI_LEAKY_PRE, 0.1, _lib.IMPL_MFMA_BF16X3)
    assert ops.conv_planes_supported(d3) == 2
    p3 = torch.zeros(int(lib.agx_conv_packed_floats(ctypes.byref(d3))), device=DEV)
    planes = torch.zeros(b, 512 // 8, 3, 16, 8, dtype=torch.bfloat16, device=DEV)
    for packed, bias3 in ((p3[:-1], None), (p1, None), (p3, odd), (p3.double(), None)):
        with pytest.raises(AgxError):
            ops.conv_forward_planes(d3, planes, packed, bias3)
    torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0 and float((wide - 7.0).abs().max()) == 0.0
    # and what they let through is what they always did
    y = ops.conv_forward(desc, x, p1, bias, out=out)
    assert y is out and torch.equal(out, ops.conv_forward(desc, x, p1, bias))
    assert torch.equal(ops.resblock_forward(desc, x, p1, bias, p2, bias), ops.resblock_forward(desc, x, p1, None, p2, None))
