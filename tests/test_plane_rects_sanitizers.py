"""The plane rectangles' host code under the address and undefined-behaviour sanitizers (no GPU).

tests/plane_rects.cpp calls what a launch calls (csrc/primary_rect.hpp
plane_view, plane_line, plane_rect) on the edge inputs of
tests/test_plane_rects.py and on NaN, infinite, zero, denormal and huge rows,
heights and cameras, singular camera matrices and canvases from one pixel to
2048 x 2048.  It is compiled here as a stand-alone program with
-fsanitize=address,undefined and run as a child process (no preload, nothing of
Python under a sanitizer): any report ends it with a non-zero status.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_plane_rectangles_stand_alone_under_sanitizers(tmp_path):
    exe = tmp_path / "plane_rects"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", str(exe), os.path.join(HERE, "plane_rects.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "ok", out.stdout + out.stderr
    assert "0 failed checks" in lines and "runtime error" not in out.stderr and "Sanitizer" not in out.stderr


def test_plane_rectangles_with_optimisation(tmp_path):
    """The library's own optimisation level: the same answers (no sanitizer)."""
    exe = tmp_path / "plane_rects_o3"
    subprocess.run(["g++", "-std=c++17", "-O3", "-Wall", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(HERE, "plane_rects.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "ok", out.stdout + out.stderr
