"""The host side of mesh instances (csrc/instances.hpp; CPU only).

tests/instances.cpp, built with g++ against the headers the library includes,
checks: the world-index <-> (instance, local) maps for every triangle of nine
instances of three meshes (the first and last of each among them) through the
kernels' own search over the bases, and against the expansion; a mesh's
local-to-position table against its tree's leaf order, with and without
records outside the tree; every mesh node's ball, cast to f32 and to f64 as
the kernels hold it, holding the ball of every record below it; the
instance's world ball holding the image of the mesh's root ball under a
rotation x shear and under a mirrored non-uniform scale (20 000 surface points
each, f32 and f64), and none for a singular matrix; and the identity
decisions: equal inverse with equal material, with a different material, a
repeated face, a plain triangle equal to a virtual one, and agreement with
shape_identity's classes of the expansion.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_instances_cpp(tmp_path):
    exe = tmp_path / "instances"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(HERE, "instances.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "ok", out.stdout + out.stderr
