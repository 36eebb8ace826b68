"""The launch terms of the per-scene f32 direct kernel on the host (no GPU).

The host's launch_terms (csrc/launch_terms.hpp) must give the bits the
kernel's lanes compute from the origin, must write every field and must give
the same table when called again: tests/launch_terms.cpp states the kernel's
expressions a second time and compares over random records and origins,
compiled stand-alone with contraction off like the library, under the host
sanitizers where g++ has them (a stand-alone program: no preload).  And the
kernel argument block, with the terms appended, still fits its 4 KB segment.
"""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "ray-tracer-challenge-rs_amd", "csrc")


def _sanitize_flags(tmp_path):
    """-fsanitize=address,undefined where this g++ links them."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    ok = subprocess.run(["g++", *flags, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0
    return flags if ok else []


def test_host_terms_are_the_kernels_bits_stand_alone(tmp_path):
    exe = tmp_path / "launch_terms"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", *_sanitize_flags(tmp_path), "-o",
                    str(exe), os.path.join(HERE, "launch_terms.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "ok", out.stdout + out.stderr
    assert "4000 worlds, 0 failed checks" in lines


def test_host_terms_with_optimisation(tmp_path):
    """The library's own optimisation level, contraction off: the same bits (no sanitizer)."""
    exe = tmp_path / "launch_terms_o3"
    subprocess.run(["g++", "-std=c++17", "-O3", "-Wall", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(HERE, "launch_terms.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "ok", out.stdout + out.stderr


def test_the_terms_are_appended_and_the_block_fits():
    text = open(os.path.join(CSRC, "rtc_internal.hpp")).read()
    body = text[text.index("struct LaunchParams {"):]
    body = body[:body.index("\n};")]
    fields = re.findall(r"^\s+[\w:<>\* ]+?\b(\w+)(?:\[\w+\])?;", body, re.M)
    assert fields[-1] == "terms", fields[-3:]  # after every field the shipped kernels load
    assert "static_assert(sizeof(LaunchParams<float>) + 4 * sizeof(void*) <= 4096" in text
