#!/usr/bin/env python3
"""Digest of every gfx950 kernel in libplagnn.so or in object files, to compare two builds.

Usage: python scripts/kernel_digest.py pla-gnn_amd/plagnn/libplagnn.so [more .so / .o ...] > digest.txt

One line per kernel and code object: mangled name, code size in bytes, SHA-256 over the
function's bytes in .text followed by its 64-byte kernel descriptor (the <name>.kd symbol).
The descriptor's kernel_code_entry_byte_offset (bytes 16-23: the distance from the descriptor
to the code, which moves with the kernel's place in the file) is hashed as zero; everything
else is the raw bytes, but for the PC-relative address of a global (s_getpc_b64 s[n:n+1];
s_add_u32 sn, sn, literal; s_addc_u32 sn+1, sn+1, literal: the distance from the instruction
to the global, which moves with the kernel's place in the file as well): both literals are
hashed as zero. A kernel that calls a function it did not inline would differ in the call's
PC-relative offset when the layout changes; none of this library's does.
Needs only the ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, llvm-readelf,
llvm-objdump); opens no GPU. A comparison aid, not a test.
"""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "lib", "llvm", "bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def code_objects(path, tmp):
    """The gfx950 code objects of a host file: its .hip_fatbin holds one bundle per source."""
    fat = os.path.join(tmp, "fatbin")
    tool("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, path, os.path.join(tmp, "copy"))
    data = open(fat, "rb").read()
    starts = [i for i in range(len(data)) if data.startswith(MAGIC, i)]
    for n, (a, b) in enumerate(zip(starts, starts[1:] + [len(data)])):
        bundle, co = os.path.join(tmp, f"bundle{n}"), os.path.join(tmp, f"co{n}")
        open(bundle, "wb").write(data[a:b])
        if TARGET not in tool("clang-offload-bundler", "--list", "--type=o", "--input=" + bundle).split():
            continue
        tool("clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + bundle,
             "--output=" + co)
        yield co


def mask_pcrel(code):
    """The function's bytes with the literals of every PC-relative global address zeroed."""
    w = list(struct.unpack("<%dI" % (len(code) // 4), code[:len(code) // 4 * 4]))
    for i in range(len(w) - 4):
        if w[i] & 0xFF80FFFF != 0xBE801C00:  # s_getpc_b64 s[n:n+1]
            continue
        n = (w[i] >> 16) & 0x7F
        lo = 0x8000FF00 | n << 16 | n  # s_add_u32 sn, sn, literal
        hi = 0x8200FF00 | (n + 1) << 16 | (n + 1)  # s_addc_u32 sn+1, sn+1, literal
        if w[i + 1] == lo and w[i + 3] == hi:
            w[i + 2] = w[i + 4] = 0
    return struct.pack("<%dI" % len(w), *w) + code[len(w) * 4:]


def kernels(co):
    """(name, size, digest) of every function of the code object that has a kernel descriptor."""
    sec = {}  # section name -> (address, file offset)
    for line in tool("llvm-readelf", "-S", "-W", co).splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) > 5 and f[0].isdigit() and f[1].startswith("."):
            sec[f[1]] = (int(f[3], 16), int(f[4], 16))
    sym = {}  # name -> (address, section, size)
    for line in tool("llvm-objdump", "-t", co).splitlines():
        f = line.split()  # address, binding, type, section, size, [visibility,] name
        if len(f) >= 6 and f[3] in sec:
            sym[f[-1]] = (int(f[0], 16), f[3], int(f[4], 16))
    data = open(co, "rb").read()

    def raw(name, size=None):
        addr, s, n = sym[name]
        off = addr - sec[s][0] + sec[s][1]
        return data[off:off + (n if size is None else size)]

    for name in sorted(sym):
        if name + ".kd" in sym and sym[name][1] == ".text":
            kd = bytearray(raw(name + ".kd", 64))
            kd[16:24] = bytes(8)
            yield name, sym[name][2], hashlib.sha256(mask_pcrel(raw(name)) + bytes(kd)).hexdigest()


def main(paths):
    for path in paths:
        with tempfile.TemporaryDirectory() as tmp:
            for co in code_objects(path, tmp):
                for name, size, digest in kernels(co):
                    print(name, size, digest)


if __name__ == "__main__":
    main(sys.argv[1:])
