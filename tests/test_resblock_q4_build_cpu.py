"""Host-side check of the built channel-quad variants of the fp32 ring residual block (csrc/resblock_p.hip): read from the
metadata of the gfx950 code object in libagx.so, no GPU.  A variant ships only without scratch or spills, within 256 VGPRs and
at the workgroups-per-CU of its standard twin (same launch bounds, same LDS: the kernels declare none, the launcher asks for
``RbpGeom::LDS_BYTES`` of the geometry the two share)."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import device_code_diff  # noqa: E402

NAME = re.compile(r"_ZN3agx17resblock_p_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEE")
FIELDS = ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count", "agpr_count",
          "group_segment_fixed_size", "max_flat_workgroup_size")


def _kernels():
    """{(MW, NW, CCH, D, NSQ): {field: int}} of the residual-block ring kernels in the built library."""
    from audio_generation_amd import _lib
    _lib.load()
    lib = os.path.join(ROOT, "audio_generation_amd", "lib", "libagx.so")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for elf in device_code_diff.code_objects(lib, tmp):
            if b"resblock_p_kernel" not in elf:
                continue
            path = os.path.join(tmp, "co.elf")
            open(path, "wb").write(elf)
            notes = subprocess.run([os.path.join(device_code_diff.LLVM, "llvm-readelf"), "--notes", path], check=True,
                                   capture_output=True, text=True).stdout
            for entry in re.split(r"\n  - (?=\.agpr_count)", notes):      # one metadata entry per kernel
                m = NAME.search(entry)
                if m:
                    out[tuple(map(int, m.groups()))] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, entry).group(1)) for f in FIELDS}
    return out


def test_quad_variants_fit_like_their_standard_twins():
    ks = _kernels()
    quad = {k: v for k, v in ks.items() if k[4] >= 16}
    # C = 32, 64, 128 x d = 1, 3, 9 x (x, y, both in quads); the C = 256 row (MW = 8) opted out: its variants spill
    assert sorted(quad) == sorted((mw, nw, cch, d, 3 + q) for mw, nw, cch in ((1, 4, 8), (2, 2, 8), (4, 1, 4)) for d in (1, 3, 9)
                                  for q in (16, 32, 48))
    for k, v in quad.items():
        twin = ks[k[:4] + (k[4] % 16,)]
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
        assert v["vgpr_count"] + v["agpr_count"] <= 256, (k, v)
        assert 512 // 256 == 512 // max(256, twin["vgpr_count"] + twin["agpr_count"])      # two waves per SIMD, both
        assert v["group_segment_fixed_size"] == twin["group_segment_fixed_size"] == 0
        assert v["max_flat_workgroup_size"] == twin["max_flat_workgroup_size"] == 256
