"""Register budget of the texture build's f32 tracer kernels (rtc::textured::), read from the
gfx950 code objects inside librtc.so (no GPU needed), as tests/test_isa_budget.py does for the plain build.

The caps are the instance build's: trace_direct* at most 64 VGPRs (8 waves per SIMD), trace_pool* at most 80 (6
waves).  Scratch: the texture build drops the plain path of prepare_hit, so no f32 kernel of it may need more
scratch than its counterpart of the instance build in the same library.
"""
import os
import re
import subprocess

import pytest

from conftest import PKG

LIB = os.path.join(PKG, "rtc_amd", "_lib", "librtc.so")
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
CAPS = {"trace_direct": 64, "trace_pool": 80}


def all_kernels(tmp):
    """{kernel name: (VGPRs, private bytes)} over every code object bundled in the library (one per TU)."""
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("ROCm LLVM tools not installed")
    fb = os.path.join(tmp, "fatbin")
    subprocess.run([tools[0], "--dump-section", f".hip_fatbin={fb}", LIB, os.path.join(tmp, "lib.so")], check=True)
    data = open(fb, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    kernels = {}
    for i, at in enumerate(starts):
        one, co = os.path.join(tmp, f"bundle{i}"), os.path.join(tmp, f"co{i}.elf")
        with open(one, "wb") as f:
            f.write(data[at:starts[i + 1] if i + 1 < len(starts) else len(data)])
        subprocess.run([tools[1], "--unbundle", "--type=o", f"--input={one}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--output={co}"], check=True)
        notes = subprocess.run([tools[2], "--notes", co], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n\s+- \.", notes):
            name = re.search(r"\.name:\s+(\S+)", block)
            vgpr = re.search(r"\.vgpr_count:\s+(\d+)", block)
            priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
            if name and vgpr and priv:
                kernels[name.group(1)] = (int(vgpr.group(1)), int(priv.group(1)))
    return kernels


def test_texture_build_keeps_the_instance_builds_budget(tmp_path):
    kernels = all_kernels(str(tmp_path))
    tex = {k: v for k, v in kernels.items() if k.startswith("_ZN3rtc8textured") and re.search(r"trace_\w+If", k)}
    checked = 0
    for name, (vgpr, priv) in tex.items():
        kind = re.search(r"\d+(trace_direct|trace_pool)(_ss)?If", name)
        if not kind:
            continue  # (trace_rays: no cap)
        twin = name.replace("_ZN3rtc8textured", "_ZN3rtc9instanced")
        assert twin in kernels, f"no instance-build counterpart of {name}"
        print(name, vgpr, priv, "instance build:", kernels[twin])
        assert vgpr <= CAPS[kind.group(1)], f"{name}: {vgpr} VGPRs > {CAPS[kind.group(1)]} (occupancy cliff)"
        assert priv <= kernels[twin][1], f"{name}: {priv} B/lane of scratch > the instance build's {kernels[twin][1]}"
        checked += 1
    assert checked == 12, sorted(tex)  # direct x 2, pool x 4, and their supersampled twins
