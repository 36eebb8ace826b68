"""The cull tables' host code under the address and undefined-behaviour sanitizers (no GPU).

tests/cull_tables.cpp calls what a launch calls (csrc/cull_tables.hpp
fill_cull_tables, over primary_rect.hpp) on canvases from one pixel to
2048 x 2048, on worlds of up to eight slots and on NaN, infinite, denormal and
huge values in a caster's bound and a light, and compares every word with its
definition.  It is compiled here as a stand-alone program with
-fsanitize=address,undefined and run as a child process (no preload, nothing of
Python under a sanitizer): any report ends it with a non-zero status.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_cull_tables_stand_alone_under_sanitizers(tmp_path):
    exe = tmp_path / "cull_tables"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", str(exe), os.path.join(HERE, "cull_tables.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "ok", out.stdout + out.stderr
    assert "0 failed checks" in lines and "runtime error" not in out.stderr and "Sanitizer" not in out.stderr


def test_cull_tables_with_optimisation(tmp_path):
    """The library's own optimisation level: the same answers (no sanitizer)."""
    exe = tmp_path / "cull_tables_o3"
    subprocess.run(["g++", "-std=c++17", "-O3", "-Wall", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(HERE, "cull_tables.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "ok", out.stdout + out.stderr
