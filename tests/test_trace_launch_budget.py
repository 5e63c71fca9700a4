"""The raycast + request launch at six waves per SIMD (VK_TR_WAVES 6, vk_trace.hip): the built library's own metadata for
trace_and_request_kernel<true, 2> must say 80 VGPRs or fewer (the allocation granule is 8: 512 / 80 = 6 waves) and no
private segment (no spill to scratch memory) — what tools/kres.py prints from the compiler's remarks, read from the code
object inside vulcan_amd/lib/libvk_hip.so with llvm-readelf."""
import os
import re
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "vulcan_amd", "lib", "libvk_hip.so")
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def launch_waves():
    text = open(os.path.join(ROOT, "vulcan_amd", "csrc", "vk_trace.hip")).read()
    return int(re.search(r"#define VK_TR_WAVES (\d+)", text).group(1))


def code_objects(path):
    """The gfx950 code objects of every offload bundle in the library."""
    data = open(path, "rb").read()
    at = data.find(MAGIC)
    while at >= 0:
        (entries,) = struct.unpack_from("<Q", data, at + len(MAGIC))
        cursor = at + len(MAGIC) + 8
        for _ in range(entries):
            offset, size, triple_size = struct.unpack_from("<QQQ", data, cursor)
            triple = data[cursor + 24:cursor + 24 + triple_size].decode()
            cursor += 24 + triple_size
            if "gfx950" in triple and size:
                yield data[at + offset:at + offset + size]
        at = data.find(MAGIC, at + len(MAGIC))


def kernel_metadata(path, tmp_path, mangled_part):
    for i, blob in enumerate(code_objects(path)):
        if mangled_part.encode() not in blob:
            continue
        obj = tmp_path / f"code_{i}.co"
        obj.write_bytes(blob)
        notes = subprocess.run([READELF, "--notes", str(obj)], stdout=subprocess.PIPE, text=True, check=True).stdout
        for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and mangled_part in name.group(1):
                return {k: int(v) for k, v in re.findall(r"\.(vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count):\s+(\d+)", block)}
    return None


@pytest.mark.skipif(launch_waves() != 6, reason="six waves per SIMD for the raycast + request launch were not adopted: "
                    "VK_TR_WAVES stays 5 (DESIGN.md section 4, docs/rounds/r07.md)")
@pytest.mark.skipif(not os.path.exists(READELF), reason="needs llvm-readelf")
def test_the_raycast_and_request_launch_fits_six_waves_per_simd(tmp_path):
    assert os.path.exists(LIB), "build the library first"
    meta = kernel_metadata(LIB, tmp_path, "trace_and_request_kernelILb1ELi2E")
    assert meta is not None, "trace_and_request_kernel<true, 2> is not in the library"
    assert meta["vgpr_count"] <= 80, meta
    assert meta["private_segment_fixed_size"] == 0 and meta.get("vgpr_spill_count", 0) == 0, meta
