#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds of libagx.so identical?

    python tools/device_code_diff.py OLD/libagx.so NEW/libagx.so

Extracts every gfx950 code object of each library (one per translation unit, inside the .hip_fatbin section), and compares, per
kernel symbol, the machine code (the bytes llvm-objdump would disassemble) and the 64-byte kernel descriptor (NAME.kd:
registers, LDS, scratch, launch bounds).  Where a kernel sits inside its code object does not count (the order of the
instantiations moves it): the descriptor's offset to the entry point is left out, and a 32-bit literal may differ when, added to
its own address, it names the same offset of the same data symbol in both builds (the pc-relative address of a __device__
array).  Prints the counts of compared, identical, only-in-one and differing kernels; exit status 1 unless the two sets of
kernels are the same and every kernel is identical.  A refactor of host code must give "0 differ, 0 only in one".
Needs llvm-objcopy and llvm-readelf (ROCM_LLVM, default /opt/rocm/llvm/bin).
"""
import os
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib, tmp):
    """The gfx950 ELF images of the library's fat binary."""
    fat = os.path.join(tmp, "fatbin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", lib, os.devnull], check=True)
    blob = open(fat, "rb").read()
    if blob.count(b"CCOB"):
        sys.exit(f"{lib}: compressed offload bundles are not handled (build without --offload-compress)")
    out, at = [], blob.find(MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        pos = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, pos)
            triple = blob[pos + 24:pos + 24 + tlen].decode()
            pos += 24 + tlen
            if "gfx950" in triple and size:
                out.append(blob[at + off:at + off + size])
        at = blob.find(MAGIC, at + 1)
    return out


class Kernel:
    def __init__(self, code, addr, kd, data):
        self.code, self.addr, self.data = code, addr, data     # data: [(address, size, name)] of the code object's data symbols
        self.kd = kd[:16] + kd[24:]                             # without kernel_code_entry_byte_offset

    def target(self, i):
        """(data symbol, offset) the literal at byte i points to when it is taken relative to its own address."""
        at = self.addr + i + struct.unpack_from("<i", self.code, i)[0]
        for addr, size, name in self.data:
            if addr - 64 <= at < addr + size + 64:              # (the literal is relative to an address a few instructions away)
                return name, at - addr
        return None

    def same_code(self, other):
        if len(self.code) != len(other.code):
            return False
        for i in range(0, len(self.code), 4):
            if self.code[i:i + 4] != other.code[i:i + 4]:
                ta, tb = self.target(i), other.target(i)
                if ta is None or ta != tb:
                    return False
        return True


def kernels(elf, tmp):
    """{kernel symbol: Kernel} of one code object."""
    path = os.path.join(tmp, "co.elf")
    open(path, "wb").write(elf)
    text = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-SsW", path], check=True, capture_output=True, text=True).stdout
    sections, syms, data = {}, {}, []
    for line in text.splitlines():
        f = line.replace("[ ", "[").split()
        if len(f) >= 6 and f[0].startswith("[") and f[0].endswith("]") and f[0][1:-1].isdigit() and int(f[0][1:-1]) > 0:
            sections[int(f[0][1:-1])] = (int(f[3], 16), int(f[4], 16))      # address, file offset
        elif len(f) >= 8 and f[0].endswith(":") and f[0][:-1].isdigit() and f[3] in ("FUNC", "OBJECT") and f[6].isdigit():
            addr, size, sec = int(f[1], 16), int(f[2], 0), int(f[6])
            saddr, soff = sections[sec]
            syms[f[7]] = (elf[soff + addr - saddr:soff + addr - saddr + size], addr)
            if f[3] == "OBJECT" and not f[7].endswith(".kd"):
                data.append((addr, size, f[7]))
    return {name: Kernel(code, addr, syms[name + ".kd"][0], data) for name, (code, addr) in syms.items() if name + ".kd" in syms}


def library_kernels(lib):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for elf in code_objects(lib, tmp):
            for name, body in kernels(elf, tmp).items():
                assert name not in out, f"{lib}: kernel {name} in two code objects"
                out[name] = body
    return out


def main(old, new):
    a, b = library_kernels(old), library_kernels(new)
    both = sorted(set(a) & set(b))
    only = sorted(set(a) ^ set(b))
    differ = [k for k in both if a[k].kd != b[k].kd or not a[k].same_code(b[k])]
    print(f"kernels: {len(a)} in {old}, {len(b)} in {new}")
    print(f"compared {len(both)}: {len(both) - len(differ)} identical, {len(differ)} differ; {len(only)} only in one")
    for k in only:
        print("  only in", old if k in a else new, ":", k)
    for k in differ:
        what = ["code"] * (not a[k].same_code(b[k])) + ["descriptor"] * (a[k].kd != b[k].kd)
        print("  differs (" + ", ".join(what) + "):", k)
    return 1 if only or differ or not both else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
