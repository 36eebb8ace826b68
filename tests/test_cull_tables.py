"""The direct kernel's cull tables as a launch builds them, without a GPU.

csrc/cull_tables.hpp fill_cull_tables turns the rectangles of primary_rect.hpp
into the miss bits per block column and block row that a launch of the
per-scene f32 direct kernel uploads (rtc_internal.hpp LaunchParams::cull_cols,
cull_rows, ShadowLayout), from toggles and a running XOR.  tests/cull_tables.cpp
states every entry a second time by its definition and compares every word of
both tables: canvases of 1x1, 16x4, 17x5, 64x48, 100x37 and 2048x2048, worlds
from three_sphere's shape to eight slots, with and without planes, with shadow
bits that fit and that do not, lights on either side of a plane, and odd values
(NaN, infinities, denormals, huge) in a caster's bound and a light.  Compiled
here without contraction, as the library is, and run as a child process.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_cull_tables_equal_their_definition(tmp_path):
    exe = tmp_path / "cull_tables"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(HERE, "cull_tables.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "ok", out.stdout + out.stderr
    assert "0 failed checks" in lines
    # every world of the list ran, and the ones whose shadow bits fit have some
    for name in ("three_sphere", "two planes, four casters", "one plane, three casters, two lights",
                 "three planes, three casters, two lights", "eight slots", "no plane", "a sphere behind the eye",
                 "a sphere over the whole canvas", "lights on both sides of the plane"):
        assert any(line.startswith(name + ":") for line in lines), name
