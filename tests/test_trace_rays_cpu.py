"""CPU checks of the ray-batch path (rt_trace_rays*, Context.trace_rays): no GPU.

* The per-lane stack bound (rtc_internal.hpp ray_stack_entries), compiled into
  a host program (tests/ray_stack.cpp) and compared with a model of
  trace_rays's walk (rtc_kernels.hip): the lane holds one ray, shading it
  pushes its 0-2 children at remaining - 1 (none at remaining 0), and the
  lane pops its next ray.  With two children everywhere the peak equals the
  bound (it is tight); with random children it never exceeds it.
* The C entry points without a device, and Context.trace_rays's argument
  checks, which come before any library call.
"""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(PKG, "rtc_amd", "_lib", "librtc.so")
RT_ERR_INVALID = -1
MAX_DEPTH = 16


@pytest.fixture(scope="module")
def bound(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ray_stack") / "ray_stack"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", str(exe), os.path.join(HERE, "ray_stack.cpp")],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split()[-1] == "ok", (out.returncode, out.stdout, out.stderr)
    table = {}
    for line in out.stdout.splitlines():
        if line.startswith("entries"):
            _, d, n = line.split()
            table[int(d)] = int(n)
    assert sorted(table) == list(range(MAX_DEPTH + 1))
    return table


def _walk_peak(depth, children):
    """Peak entries of one lane's LIFO over the depth-first walk of one tree."""
    stack, peak = [], 0
    rem = depth  # the ray in the lane's registers
    while True:
        if rem > 0:
            stack += [rem - 1] * children()
            peak = max(peak, len(stack))
        if not stack:
            return peak
        rem = stack.pop()


def test_stack_bound_is_tight(bound):
    for depth in range(MAX_DEPTH + 1):
        assert _walk_peak(depth, lambda: 2) == bound[depth], depth


def test_stack_bound_holds_for_random_trees(bound):
    rng = random.Random(11)
    for depth in range(MAX_DEPTH + 1):
        for weights in ((0, 1, 2), (1, 2, 2, 2), (0, 2), (1,)):
            for _ in range(4 if depth > 12 else 20):
                assert _walk_peak(depth, lambda: rng.choice(weights)) <= bound[depth], (depth, weights)


def test_structs_match_the_header(rtc, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtc.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rt_ray_options), offsetof(rt_ray_options, flags),\n'
                   '         sizeof(rt_ray_hit_f32), offsetof(rt_ray_hit_f32, shape), sizeof(rt_ray_hit_f64),\n'
                   '         offsetof(rt_ray_hit_f64, shape), offsetof(rt_ray_options, precision));\n  return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                   check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(rtc.RayOptions), rtc.RayOptions.flags.offset, rtc.RAY_HIT_F32.itemsize,
                   rtc.RAY_HIT_F32.fields["shape"][1], rtc.RAY_HIT_F64.itemsize, rtc.RAY_HIT_F64.fields["shape"][1],
                   rtc.RayOptions.precision.offset]
    assert got == [16, 8, 8, 4, 16, 8, 4]


def test_rust_shim_declares_the_ray_batch_entry_points():
    """INTEGRATION.md's Rust declarations of rt_trace_rays* against the header: same names, same number of
    parameters (tests/test_rust_shim_layout.py lays out the Rt* structs of every rust block)."""
    import re
    rust = "\n".join(re.findall(r"```rust\n(.*?)```", open(os.path.join(ROOT, "INTEGRATION.md")).read(), re.S))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtc.h")).read(), flags=re.S)
    for name in ("rt_trace_rays_device", "rt_trace_rays"):
        r = re.search(r"fn " + name + r"\((.*?)\)\s*->\s*c_int;", re.sub(r"/\*.*?\*/", "", rust, flags=re.S), re.S)
        c = re.search(r"int " + name + r"\((.*?)\);", header, re.S)
        assert r and c, name
        assert len(r.group(1).split(",")) == len(c.group(1).split(",")) == 7, name
    for struct in ("RtRayOptions", "RtRayHitF32", "RtRayHitF64"):
        assert f"pub struct {struct} " in rust, struct


def test_entry_points_reject_null_arguments():
    lib = C.CDLL(LIB)
    lib.rt_trace_rays_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
    lib.rt_trace_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rt_last_error.restype = C.c_char_p
    buf = (C.c_double * 6)()
    opts = (C.c_uint32 * 4)(6, 1, 0, 0)
    assert lib.rt_trace_rays_device(None, buf, 1, opts, buf, None, None) == RT_ERR_INVALID
    assert b"null context" in lib.rt_last_error()
    assert lib.rt_trace_rays(None, buf, 1, opts, buf, None, None) == RT_ERR_INVALID
    assert lib.rt_trace_rays_device(None, None, 0, None, None, None, None) == RT_ERR_INVALID
    assert lib.rt_trace_rays(None, None, 0, None, None, None, None) == RT_ERR_INVALID


def _no_context(rtc):
    """A Context object with no handle: argument checks come before any library call."""
    ctx = object.__new__(rtc.Context)
    ctx._h, ctx.device, ctx.scene = None, 0, None
    return ctx


@pytest.mark.parametrize("bad", [
    np.zeros((4, 5)), np.zeros(6), np.zeros((2, 3, 6)), np.zeros((4, 6), dtype=np.int32),
    np.zeros((4, 6), dtype=np.float16), np.zeros((4, 12))[:, ::2], np.zeros((6, 4)).T, [[0.0] * 6], None,
], ids=["cols", "1d", "3d", "int32", "f16", "strided", "transposed", "list", "none"])
def test_trace_rays_rejects_bad_arrays(rtc, bad):
    with pytest.raises(ValueError):
        _no_context(rtc).trace_rays(bad)


def test_trace_rays_rejects_bad_precision_and_tensors(rtc):
    ctx = _no_context(rtc)
    with pytest.raises(ValueError, match="precision"):
        ctx.trace_rays(np.zeros((4, 6)), precision="f16")
    import torch
    for bad in (torch.zeros((4, 6)),                          # on the CPU
                torch.zeros((4, 6), dtype=torch.float16),     # ... and a wrong dtype
                torch.zeros((4, 12))[:, ::2]):                # ... and strided
        with pytest.raises(ValueError):
            ctx.trace_rays(bad)
