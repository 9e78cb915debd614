"""CPU-side checks of the C-ABI library and the host logic (no kernel is launched)."""
import ctypes
import os
import re

import pytest
import torch

from audio_generation_amd import _lib, ops
from audio_generation_amd.vae import CausalVQAE
from oracle import codec
from tests.helpers import load_meta, load_npz, sub_sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from audio_generation_amd import build
    build.build()
    return _lib.load()


def _declared_symbols():
    names = set()
    for fn in os.listdir(os.path.join(ROOT, "include")):
        if fn.endswith(".h"):
            text = open(os.path.join(ROOT, "include", fn)).read()
            text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
            names |= set(re.findall(r"\b(agx_[a-z0-9_]+)\s*\(", text))
    return names


def test_every_declared_symbol_is_exported_and_bound_at_abi_122(lib):
    declared = _declared_symbols()
    assert declared, "no declarations found in include/*.h"
    assert declared == set(_lib.SIGNATURES), (declared ^ set(_lib.SIGNATURES))
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/agx.h but not exported by libagx.so"
    assert lib.agx_version() == 122


def test_out_len_matches_reference_padding_rule(lib):
    # CAUSAL: vae.py:32-43; checked against the oracle's restatement (itself pinned by goldens)
    for (k, s, d) in [(7, 1, 1), (7, 1, 3), (7, 1, 9), (5, 2, 1), (9, 4, 1), (11, 5, 1), (17, 8, 1), (3, 1, 1),
                      (1, 1, 1), (5, 3, 2), (1, 2, 1)]:
        for length in (17, 50, 51, 53, 61, 64, 225, 1600, 72000):
            left, right = codec.causal_pads(length, k, s, d)
            want = (length + left + right - d * (k - 1) - 1) // s + 1
            desc = ops.conv_desc(_lib.CONV_CAUSAL, 1, 4, 4, length, k, s, d)
            assert ops.conv_out_len(desc) == want, (k, s, d, length)
    for s in (1, 2, 4, 5, 8):
        assert ops.conv_out_len(ops.conv_desc(_lib.CONV_UPSAMPLE, 1, 4, 4, 225, 2 * s + 1, s)) == 225 * s
        assert ops.conv_out_len(ops.conv_desc(_lib.CONV_TRANSPOSED, 1, 4, 4, 225, 2 * s + 1, s)) == 225 * s
    assert ops.conv_out_len(ops.conv_desc(_lib.CONV_SAME, 1, 4, 4, 77, 3, 1)) == 77
    # 72000 -> 225 known answer (vae.py:354)
    length = 72000
    for s in (2, 4, 5, 8):
        length = ops.conv_out_len(ops.conv_desc(_lib.CONV_CAUSAL, 1, 4, 4, length, 2 * s + 1, s))
    assert length == 225


def test_bad_descriptors_report_errors(lib):
    bad = ops.conv_desc(_lib.CONV_CAUSAL, 1, 0, 4, 10, 3)
    assert lib.agx_conv_out_len(ctypes.byref(bad)) == -1
    assert b"non-positive" in lib.agx_last_error()
    with pytest.raises(_lib.AgxError):
        ops.conv_out_len(ops.conv_desc(99, 1, 4, 4, 10, 3))
    with pytest.raises(_lib.AgxError):
        ops.conv_out_len(ops.conv_desc(_lib.CONV_TRANSPOSED, 1, 4, 4, 10, 3, 5))  # K < stride
    assert lib.agx_rvq_packed_floats(0, 4, 4) < 0
    assert lib.agx_rvq_packed_floats(8, 1024, 512) == 8 * (512 * 1024 + 2 * 1024 + 4 + 512)


def test_no_cpu_fallback():
    with pytest.raises(_lib.AgxError, match="MI355X only"):
        ops.conv_pack(ops.conv_desc(_lib.CONV_CAUSAL, 1, 4, 4, 16, 3), torch.zeros(4, 4, 3))
    model = CausalVQAE(in_channels=1, n_blocks=2, strides=(2, 2), first_block_channels=4, codebook_dim=8,
                       num_quantizers=1, codebook_size=8, input_format="n c l", wavelet_decoders=False)
    with pytest.raises(_lib.AgxError):
        model(torch.zeros(1, 1, 64))


def test_state_dict_layout_is_the_references():
    g6 = load_meta()["g6"]
    model = CausalVQAE(in_channels=1, n_blocks=4, strides=(2, 4, 5, 8), num_quantizers=8, codebook_size=1024,
                       codebook_dim=512, input_format="n c l", wavelet_decoders=False)
    keys = {k for k in model.state_dict() if not k.startswith("quantizer.")}
    assert keys == set(g6["state_dict_keys"])
    assert sum(p.numel() for p in model.encoders.parameters()) == g6["params_encoders"]
    assert sum(p.numel() for p in model.decoders.parameters()) == g6["params_decoders"]
    assert model.scale_factor == 320 and model.num_quantizers == 8 and model.codebook_size == [1024] * 8
    # a reference checkpoint loads as is (conv stacks; the quantiser's keys are external)
    g1, meta = load_npz("g1_tiny_vqae.npz"), load_meta()["g1"]["kwargs"]
    tiny = CausalVQAE(**{**meta, "strides": tuple(meta["strides"])})
    missing, unexpected = tiny.load_state_dict(sub_sd(g1, "sd/"), strict=False)
    assert unexpected == [] and all(k.startswith("quantizer.") for k in missing)


def test_quantizer_surface():
    from audio_generation_amd.quantizer import ResidualQuantizer, tuple_checker
    q = ResidualQuantizer(num_quantizers=3, dim=8, quantizer_class="base", codebook_sizes=12)
    assert q.num_quantizers == 3 and len(q.quantizers) == 3 and q.use_som
    assert (q.quantizers[0].som.height, q.quantizers[0].som.width) == (3, 4)
    assert len(list(q.parameters())) == 1 and q.get_stale_clusters() == [0, 0, 0]
    q.update_cutoff(new_cutoff=2.0)
    assert q.get_stale_clusters() == [12, 12, 12]
    q.update_cutoff(ratio=0.25)
    assert q.vq_cutoff_freq == 0.5
    assert tuple_checker(3, 2) == [3, 3]
    ema = ResidualQuantizer(num_quantizers=2, dim=4, quantizer_class="ema", codebook_sizes=4)
    assert len(list(ema.parameters())) == 0 and "codebooks" in ema.state_dict()
    # one codebook size per stage (the reference's codebook_size tuple, vae.py:233): (Q, max K, D) storage, padded rows zero
    mixed = ResidualQuantizer(num_quantizers=3, dim=4, codebook_sizes=(16, 5, 9))
    assert mixed.codebook_sizes == (16, 5, 9) and mixed.codebooks.shape == (3, 16, 4)
    assert [tuple(st.codebook.shape) for st in mixed.quantizers] == [(16, 4), (5, 4), (9, 4)]
    assert float(mixed.codebooks[1, 5:].abs().max()) == 0.0 and float(mixed.codebooks[1, :5].abs().min()) > 0.0
    mixed.update_cutoff(new_cutoff=2.0)
    assert mixed.get_stale_clusters() == [16, 5, 9]
    from audio_generation_amd.vae import CausalVQAE
    model = CausalVQAE(in_channels=1, n_blocks=2, strides=(2, 2), first_block_channels=8, num_quantizers=2,
                       codebook_size=(32, 8), codebook_dim=32, input_format="n c l", wavelet_decoders=False)
    assert model.quantizer.codebook_sizes == (32, 8) and list(model.codebook_size) == [32, 8]


def test_descriptor_structs_match_the_header_layout(tmp_path):
    """sizeof / offsetof of the two descriptor structs as gcc lays them out from include/agx.h against the
    ctypes mirrors in _lib.py (ABI drift would silently scramble every conv call)."""
    import ctypes
    import subprocess
    from audio_generation_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "layout.c"
    fields1 = [f for f, _ in _lib.ConvDesc._fields_]
    fields2 = [f for f, _ in _lib.Conv2dDesc._fields_]
    body = ['#include <stdio.h>', '#include <stddef.h>', '#include "agx.h"', 'int main(void) {',
            'printf("%zu\\n", sizeof(agx_conv_desc));']
    body += [f'printf("%zu\\n", offsetof(agx_conv_desc, {f}));' for f in fields1]
    body += ['printf("%zu\\n", sizeof(agx_conv2d_desc));']
    body += [f'printf("%zu\\n", offsetof(agx_conv2d_desc, {f}));' for f in fields2]
    body += ['return 0; }']
    src.write_text("\n".join(body))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(_lib.ConvDesc)] + [getattr(_lib.ConvDesc, f).offset for f in fields1]
    want += [ctypes.sizeof(_lib.Conv2dDesc)] + [getattr(_lib.Conv2dDesc, f).offset for f in fields2]
    assert nums == want


def test_tuning_knobs_from_the_environment():
    """AGX_TUNING=knob=value,... is applied once by _lib.load(); an unknown knob fails loudly (fresh interpreters:
    the library handle of this process is already loaded)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("from audio_generation_amd import _lib; lib = _lib.load(); "
            "print(lib.agx_get_tuning(b'dw_direct'), lib.agx_get_tuning(b'patch_tie'))")
    env = dict(os.environ, AGX_TUNING="dw_direct=1, patch_tie=0")
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["1", "0"]
    bad = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, AGX_TUNING="no_such_knob=1"),
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "no_such_knob" in bad.stderr


def _struct_fields_in_header(name):
    text = open(os.path.join(ROOT, "include", "agx.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for typ, names in re.findall(r"\b(int32_t|float)\s+([a-z_0-9,\s]+?)\s*;", body):
        out += [(typ, n.strip()) for n in names.split(",")]
    return out


def test_descriptor_structs_agree_between_header_binding_and_documented_stub(lib):
    """An ABI bump must not desync the binding a maintainer copies from INTEGRATION.md (VERDICT r1, row b):
    header fields == ctypes fields of _lib.py == fields of the documented stub == sizeof() inside the library."""
    ctype = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    for cname, struct, sizeof in (("agx_conv_desc", _lib.ConvDesc, lib.agx_sizeof_conv_desc),
                                  ("agx_conv2d_desc", _lib.Conv2dDesc, lib.agx_sizeof_conv2d_desc)):
        hdr = _struct_fields_in_header(cname)
        assert [(n, ctype[t]) for t, n in hdr] == list(struct._fields_), cname
        assert sizeof() == ctypes.sizeof(struct) == 4 * len(hdr)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    stub = re.search(r"class ConvDesc\(Structure\):.*?_fields_ = \[(.*?)\]\s*(?:#[^\n]*)?\n\n", doc, flags=re.S).group(1)
    doc_fields = re.findall(r'\("([a-z_0-9]+)",\s*(c_int32|c_float)\)', stub)
    want = [(n, "c_int32" if t is ctypes.c_int32 else "c_float") for n, t in _lib.ConvDesc._fields_]
    assert doc_fields == want, "INTEGRATION.md's ConvDesc stub is out of date with include/agx.h"
    # the stub's positional ConvDesc(...) call passes one value per field
    call = re.search(r"d = ConvDesc\((.*?)\)\n", doc, flags=re.S).group(1)
    depth, n_args = 0, 1
    for ch in call:
        depth += ch in "([" 
        depth -= ch in ")]"
        n_args += ch == "," and depth == 0
    assert n_args == len(want)
    assert "agx_sizeof_conv_desc() == ctypes.sizeof(ConvDesc)" in doc


def test_parameter_order_matches_torch_weight_norm():
    """``parameters()`` order must be torch's (bias, weight_g, weight_v) so that an index-based optimizer
    state saved by the reference trainer (training.py:225-242) lands on the right tensors."""
    import warnings
    from audio_generation_amd.vae import CausalConv1d, CausalConvT1d
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = torch.nn.utils.weight_norm(torch.nn.Conv1d(4, 6, 7))
        ref_t = torch.nn.utils.weight_norm(torch.nn.ConvTranspose1d(4, 6, 7))
    for mine, theirs in ((CausalConv1d(4, 6, 7).conv, ref), (CausalConvT1d(4, 6, 7).conv, ref_t)):
        assert [(n, tuple(p.shape)) for n, p in mine.named_parameters()] == \
               [(n, tuple(p.shape)) for n, p in theirs.named_parameters()]
    model = CausalVQAE(in_channels=1, n_blocks=4, strides=(2, 4, 5, 8), first_block_channels=4, num_quantizers=1,
                       codebook_size=8, codebook_dim=16, wavelet_decoders=False)
    names = [n for n, _ in model.named_parameters() if n.startswith("encoders.1.")][:3]
    assert [n.rsplit(".", 1)[1] for n in names] == ["bias", "weight_g", "weight_v"]


def test_ring_kernels_refuse_clips_beyond_their_32_bit_offsets(lib):
    """conv_p / resblock_p address inside a clip with 32-bit byte offsets; a clip with Cout * Lout * 4 >= 2^32
    (or 16 * Lin * 4 >= 2^31) must be lowered to the 64-bit-addressed first-round kernels, decided from the shape alone."""
    leaky = _lib.EPI_LEAKY_PRE
    short = ops.conv_desc(_lib.CONV_CAUSAL, 1, 32, 64, 72000, 5, 2, 1, leaky)
    assert ops.conv_kernel_name(short).startswith("conv_p<down2")
    for length in (1 << 24, 1 << 25):           # 16 * Lin * 4 = 2^30 (still fine) / 2^31 (must fall back)
        name = ops.conv_kernel_name(ops.conv_desc(_lib.CONV_CAUSAL, 1, 32, 64, length, 5, 2, 1, leaky))
        assert name.startswith("conv_p<down2") == (length == 1 << 24), (length, name)
    up = ops.conv_desc(_lib.CONV_UPSAMPLE, 1, 64, 32, 1 << 23, 5, 2, 1, leaky)          # Cout * Lout * 4 = 2^31: ring
    assert ops.conv_kernel_name(up).startswith("conv_p<up2")
    up = ops.conv_desc(_lib.CONV_UPSAMPLE, 1, 64, 32, 1 << 24, 5, 2, 1, leaky)          # = 2^32: not the ring
    assert not ops.conv_kernel_name(up).startswith("conv_p")
    rb = ops.conv_desc(_lib.CONV_CAUSAL, 1, 256, 256, 1 << 21, 7, 1, 1)                 # C * L * 4 = 2^31: ring
    assert ops.resblock_kernel_name(rb).startswith("resblock_p")
    rb = ops.conv_desc(_lib.CONV_CAUSAL, 1, 256, 256, 1 << 22, 7, 1, 1)                 # = 2^32: first fused kernel
    assert not ops.resblock_kernel_name(rb).startswith("resblock_p")


def test_discriminator_arithmetic_modes_are_flags_only():
    """set_arithmetic only marks the Conv2d layers (no kernel is chosen here: the library decides per feature map at call
    time); unknown modes are refused.  discriminator.py:101-114 (STFT discriminator Conv2d stack)."""
    import pytest
    from audio_generation_amd import _lib, discriminator as ad
    d = ad.STFTDiscriminator(win_length=256)
    convs = [m for m in d.modules() if isinstance(m, ad._SNConv)]
    assert convs and all(m.impl == _lib.IMPL_AUTO and not m.ring_only for m in convs)
    ad.set_arithmetic(d, "bf16x3_ring")
    assert all(m.impl == _lib.IMPL_MFMA_BF16X3 and m.ring_only for m in convs if m.nd == 2)
    ad.set_arithmetic(d, "bf16x3")
    assert all(m.impl == _lib.IMPL_MFMA_BF16X3 and not m.ring_only for m in convs if m.nd == 2)
    ad.set_arithmetic(d, "fp32")
    assert all(m.impl == _lib.IMPL_AUTO for m in convs)
    with pytest.raises(ValueError):
        ad.set_arithmetic(d, "fp16")


def test_multires_placement_is_off_by_default_and_adds_only_its_own_keys():
    """The build-defined multires placement (CausalVQAE docstring) leaves the reference's state dict untouched when off and adds
    exactly ``{encoders,decoders}.<block>.multires.{h0,h1,w}`` when on; the oracle's init_state_dict names the same keys."""
    from audio_generation_amd.vae import CausalVQAE
    from oracle import codec
    kw = dict(in_channels=1, n_blocks=2, strides=(2, 4), first_block_channels=4, codebook_dim=8, num_quantizers=1, codebook_size=16,
              wavelet_decoders=False)
    base = set(CausalVQAE(**kw).state_dict())
    on = set(CausalVQAE(multires_encoders=[True, False], multires_decoders=True, multires_kernel_size=3, multires_depth=2, **kw).state_dict())
    extra = on - base
    assert base <= on
    assert extra == {f"{a}.multires.{n}" for a in ("encoders.1", "decoders.1", "decoders.2") for n in ("h0", "h1", "w")}
    spec = codec.CodecSpec(in_channels=1, n_blocks=2, strides=(2, 4), first_block_channels=4, codebook_dim=8, wavelet_decoders=False,
                           multires_encoders=[True, False], multires_decoders=True, multires_kernel_size=3, multires_depth=2)
    sd = codec.init_state_dict(spec)
    assert extra <= set(sd) and sd["decoders.2.multires.w"].shape == (4, 4) and sd["encoders.1.multires.h0"].shape == (8, 1, 3)


def test_round4_entry_points_and_knobs_on_the_host(lib):
    """Activation planes, verify mode and the probe-only diagnostics: what can be checked without a GPU."""
    import ctypes
    assert lib.agx_planes_bytes(32, 512, 225) == 32 * 64 * 3 * 225 * 16      # 6 bytes per element
    assert lib.agx_planes_bytes(1, 12, 8) == 0                               # channels not a multiple of 8
    assert lib.agx_planes_split(None, None, 1, 12, 8, None) == -1            # AGX_ERR_BAD_SHAPE before anything is touched
    d = _lib.ConvDesc(_lib.CONV_UPSAMPLE, 2, 512, 256, 225, 17, 8, 1, 0, 0.1, _lib.IMPL_MFMA_BF16X3, 1, 0)
    assert lib.agx_conv_planes_supported(ctypes.byref(d)) == 1               # reads planes
    d = _lib.ConvDesc(_lib.CONV_TRANSPOSED, 2, 512, 512, 225, 7, 1, 1, 0, 0.1, _lib.IMPL_MFMA_BF16X3, 1, 0)
    assert lib.agx_conv_planes_supported(ctypes.byref(d)) == 2               # ... and writes them
    d = _lib.ConvDesc(_lib.CONV_CAUSAL, 2, 64, 128, 4000, 9, 4, 1, 0, 0.1, _lib.IMPL_MFMA_BF16X3, 1, 0)
    assert lib.agx_conv_planes_supported(ctypes.byref(d)) == 0               # strided: fp32 input (its own ring form)
    buf = ctypes.create_string_buffer(96)
    assert lib.agx_conv_kernel_name(ctypes.byref(d), buf, 96) == 0 and buf.value.decode().startswith("conv_b3<down4,")
    d = _lib.ConvDesc(_lib.CONV_UPSAMPLE, 2, 512, 256, 225, 17, 8, 1, 0, 0.1, _lib.IMPL_AUTO, 1, 0)
    assert lib.agx_conv_planes_supported(ctypes.byref(d)) == 0               # fp32 descriptor
    d = _lib.ConvDesc(_lib.CONV_CAUSAL, 32, 512, 1536, 225, 1, 1, 1, 0, 0.1, _lib.IMPL_AUTO, 1, 0)
    assert lib.agx_conv_kernel_name(ctypes.byref(d), buf, 96) == 0 and buf.value.decode().startswith("conv_p<k1,")
    # knobs: the verify mode is a product knob; the ones that weaken the RVQ bound exist in the probe build only
    assert lib.agx_set_tuning(b"rvq_verify", 1) == 0 and lib.agx_get_tuning(b"rvq_verify") == 1
    assert lib.agx_set_tuning(b"rvq_verify", 0) == 0
    for v in (7, 8, 9):
        assert lib.agx_set_tuning(b"b3_dbg", v) == -5                        # AGX_ERR_UNSUPPORTED
    assert lib.agx_get_tuning(b"b3_dbg") == 0
    assert lib.agx_rvq_debug_stamps(None, 0) == -5


def test_bench_roofline_of_a_forward_that_mixes_the_two_matrix_pipes():
    """bench.arithmetic_roofline: bf16x3 kernels against 2500 / 6, the step against the blended floor (never a bf16x3 figure over the fp32 peak)."""
    import bench
    per = {"resblock_b3<2,2,x2>:bf16x3": dict(ms=2.0, launches=2, macs=2 * 100e9, ref_macs=0, bytes=0, avg_us=1000.0, tflops=200.0, gbps=0.0,
                                              launches_per_step=1.0, ms_per_step=1.0),
           "resblock_p<2,2,8>": dict(ms=4.0, launches=2, macs=2 * 125e9, ref_macs=0, bytes=0, avg_us=2000.0, tflops=125.0, gbps=0.0,
                                     launches_per_step=1.0, ms_per_step=2.0)}
    r = bench.arithmetic_roofline(per, 3.2)
    assert r["kernel"].endswith(":bf16x3") and abs(r["peak"] - 2500.0 / 6) < 1e-9 and abs(r["frac"] - 200.0 / (2500.0 / 6)) < 1e-12
    floor = 1e3 * (200e9 / (2500e12 / 6) + 250e9 / 157.3e12)
    assert abs(r["blended_floor_ms"] - floor) < 1e-9 and abs(r["frac_of_blended_roofline"] - floor / 3.2) < 1e-12
    assert "frac_of_fp32_mfma_peak" not in r


def test_weight_gradient_kernel_names_pin_the_production_slicing(lib):
    """The weight-gradient name queries (host only) at config-5 shapes: kernel, operand copy, contraction slices and items.
    These are the long-run regimes tests/test_gpu_weight_grad_training_size.py replays exactly; a dispatch change that
    moves them (e.g. back to one item per slice) must show up here."""
    from tests.wgrad_ref import parse_plan
    c1, c2 = ops.conv_desc, ops.conv2d_desc
    cases = [
        (ops.conv_bwd_weight_kernel_name, c1(_lib.CONV_CAUSAL, 32, 32, 32, 72000, 7, 1, 1),
         "conv_bwd_weight_direct<1,2,1,4> cfg=13 op=none slices=768 items=72000", 94),
        (ops.conv_bwd_weight_kernel_name, c1(_lib.CONV_CAUSAL, 32, 512, 512, 225, 3, 1, 1),
         "conv_bwd_weight_direct<2,2,2,2> cfg=10 op=none slices=16 items=256", 16),
        (ops.conv_bwd_weight_kernel_name, c1(_lib.CONV_CAUSAL, 32, 32, 64, 72000, 5, 2, 1),
         "conv_bwd_weight_direct<2,2,1,2,true> cfg=11 op=phase_x slices=768 items=36000", 47),
        (ops.conv_bwd_weight_kernel_name, c1(_lib.CONV_TRANSPOSED, 32, 64, 32, 36000, 5, 2, 1),
         "conv_bwd_weight_direct<2,2,1,2> cfg=11 op=phase_dy slices=768 items=36000", 47),
        (ops.conv_bwd_weight_kernel_name, c1(_lib.CONV_UPSAMPLE, 32, 64, 32, 36000, 5, 2, 1),
         "conv_bwd_weight_direct<2,2,1,2> cfg=11 op=phase_dy slices=768 items=36000", 47),
        (ops.conv_grouped_bwd_weight_kernel_name, c1(_lib.CONV_PADDED, 32, 16, 64, 18000, 41, 4, 1, groups=4, padding=20),
         "grouped_bwd_weight_tiled<16> op=none slices=1024 items=576", 1),
        (ops.conv2d_bwd_weight_kernel_name, c2(32, 32, 32, 2251, 128, 3, 3, (1, 1), (1, 1)),
         "conv2d_bwd_weight_direct<1,3,1,1> cfg=17 op=none slices=2048 items=288128", 141),
        (ops.conv2d_bwd_weight_kernel_name, c2(32, 32, 64, 2251, 128, 3, 4, (1, 2), (1, 1)),
         "conv2d_bwd_weight_shared<2,1,1,4> cfg=15 op=deinterleave slices=512 items=144064", 282),
        (ops.conv2d_bwd_weight_kernel_name, c2(32, 128, 128, 1125, 32, 3, 3, (1, 1), (1, 1), impl=_lib.IMPL_MFMA_BF16X3),
         "conv2d_bwd_weight_shared<2,2,2,2,1> cfg=10 op=none slices=171 items=36000", 211),
        (ops.conv2d_bwd_weight_kernel_name, c2(32, 256, 256, 281, 8, 3, 3, (1, 1), (1, 1)),
         "conv2d_bwd_weight_shared<2,2,2,2> cfg=10 op=prepad slices=43 items=2816", 66),
        (ops.conv2d_bwd_weight_kernel_name, c2(32, 2, 32, 2251, 128, 7, 7, (1, 1), (3, 3)),
         "conv2d_bwd_weight<1,1,1,4> cfg=2 op=none slices=1536 items=144064", 94),
    ]
    for query, desc, want, per in cases:
        name = query(desc)
        assert name == want, (name, want)
        assert parse_plan(name)["per"] == per, name
    # the queries read the knobs the launchers read
    lib.agx_set_tuning(b"dw1_wgs", 1)
    try:
        assert ops.conv_bwd_weight_kernel_name(cases[0][1]).endswith("slices=1 items=72000")
    finally:
        lib.agx_set_tuning(b"dw1_wgs", 768)
    with pytest.raises(_lib.AgxError):
        ops.conv_grouped_bwd_weight_kernel_name(c1(_lib.CONV_CAUSAL, 1, 4, 4, 64, 3, 1, 1))
