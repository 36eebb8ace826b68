"""Register budget of the map build's f32 tracer kernels (rtc::mapped::), read from the gfx950
code objects inside librtc.so (no GPU needed) with tests/test_isa_budget_texture.py's reader: register counts and
scratch sizes from the code-object notes, nothing else.

The caps are the other builds': trace_direct* at most 64 VGPRs (8 waves per SIMD), trace_pool* at most 80 (6
waves).  Scratch: the map build is the area build plus the maps of image_color, so no f32 kernel of it may need
more scratch than its counterpart of the area build in the same library.  And the reason the build exists: the
texture and area builds hold none of the map code (their kernels are the sizes they were).
"""
import re

from test_isa_budget_texture import CAPS, all_kernels


def test_map_build_keeps_the_area_builds_budget(tmp_path):
    kernels = all_kernels(str(tmp_path))
    mapped = {k: v for k, v in kernels.items() if k.startswith("_ZN3rtc6mapped") and re.search(r"trace_\w+If", k)}
    checked = 0
    for name, (vgpr, priv) in mapped.items():
        kind = re.search(r"\d+(trace_direct|trace_pool)(_ss|_lens)?If", name)
        if not kind:
            continue  # (trace_rays: no cap)
        twin = name.replace("_ZN3rtc6mapped", "_ZN3rtc4area")
        assert twin in kernels, f"no area-build counterpart of {name}"
        print(name, vgpr, priv, "area build:", kernels[twin])
        assert vgpr <= CAPS[kind.group(1)], f"{name}: {vgpr} VGPRs > {CAPS[kind.group(1)]} (occupancy cliff)"
        assert priv <= kernels[twin][1], f"{name}: {priv} B/lane of scratch > the area build's {kernels[twin][1]}"
        checked += 1
    assert checked == 18, sorted(mapped)  # direct x 2, pool x 4, and their supersampled and lens twins
