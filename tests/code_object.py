"""Kernel resource figures of a built library, read from its code objects (test infrastructure; also used by tools/)."""
import os
import re
import shutil
import struct
import subprocess


def kernel_resources(lib_path):
    """{kernel symbol: {metadata key: int}} of every gfx950 kernel in the library's offload bundles (the AMDGPU metadata note of
    each code object, read with the llvm-readelf of the ROCm that provides hipcc)."""
    hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc not found"
    readelf = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "llvm-readelf")
    if not os.path.exists(readelf):
        readelf = shutil.which("llvm-readelf")
    assert readelf, "llvm-readelf not found"
    data = open(lib_path, "rb").read()
    magic, found, pos = b"__CLANG_OFFLOAD_BUNDLE__", {}, 0
    while (p := data.find(magic, pos)) >= 0:
        n, = struct.unpack_from("<Q", data, p + 24)
        q = p + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, q)
            triple = data[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" not in triple or size == 0:
                continue
            notes = subprocess.run([readelf, "--notes", "-"], input=data[p + off:p + off + size], capture_output=True, check=True).stdout.decode()
            for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
                name = re.search(r"\n\s+\.name:\s+(\S+)", block).group(1)
                found[name] = {k: int(v) for k, v in re.findall(r"\n\s+\.(\w+):\s+(\d+)\s*(?=\n)", block)}
        pos = p + len(magic)
    return found
