"""Register budget of the motion build's f32 tracer kernels (rtc::moving::), read from the
gfx950 code objects inside librtc.so (no GPU needed), with tests/test_isa_budget_texture.py's reader.

The caps are the project's occupancy conditions: trace_direct* (the shutter kernel among them) at most 64 VGPRs
(8 waves per SIMD), trace_pool* at most 80 (6 waves).  Scratch: tau is live through a ray's tree and a moving
record costs a velocity, so equality with the map build's twin is not demanded; each kernel's scratch is printed
beside its twin's and may not exceed the value recorded in DESIGN.md §3.17 (RECORDED below), so that a later
regression shows.  The shutter kernels have no twin; the lens kernels of the map build stand beside them.
"""
import re

from test_isa_budget_texture import CAPS, all_kernels

# B/lane of scratch, by kernel family and (lds, dup) template arguments, as built and recorded in DESIGN.md §3.17
RECORDED = {
    "trace_direct": 24, "trace_direct_ss": 44, "trace_direct_lens": 60, "trace_direct_shutter": 64,
    "trace_pool": 104, "trace_pool_ss": 188, "trace_pool_lens": 196, "trace_pool_shutter": 208,
    "trace_rays": 0,
}


def _family(name, space):
    m = re.match(rf"_ZN3rtc\d+{space}\d+(trace_\w+?)If(Lb\dE(?:Lb\dE)?)E", name)
    return (m.group(1), m.group(2)) if m else None


def test_motion_build_keeps_the_caps_and_its_recorded_scratch(tmp_path):
    kernels = all_kernels(str(tmp_path))
    moving = {_family(k, "moving"): v for k, v in kernels.items() if _family(k, "moving")}
    mapped = {_family(k, "mapped"): v for k, v in kernels.items() if _family(k, "mapped")}
    assert len(moving) == 2 * 4 + 4 * 4 + 4 and len(mapped) == len(moving) - 6  # (the six shutter kernels are the motion build's own)
    for (family, args), (vgprs, scratch) in sorted(moving.items()):
        twin = mapped.get((family.replace("shutter", "lens"), args))
        print(f"rtc::moving::{family}<float, {args}>: {vgprs} VGPRs, {scratch} B/lane of scratch "
              f"(rtc::mapped::{family.replace('shutter', 'lens')}: {twin[0]} VGPRs, {twin[1]} B)")
        cap = next((c for prefix, c in CAPS.items() if family.startswith(prefix)), None)
        if cap is not None:
            assert vgprs <= cap, (family, args, vgprs)
        assert scratch <= RECORDED[family], (family, args, scratch)
    for family in RECORDED:  # the recorded value is some kernel's, not a loose bound
        assert max(s for (f, _), (_, s) in moving.items() if f == family) == RECORDED[family], family
