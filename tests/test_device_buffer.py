"""CPU checks of the host layer's buffer owner (no GPU).

tests/device_buffer.cpp instantiates DeviceBuffer (csrc/device_memory.hpp)
with a counting host allocator that can be told to fail, built with g++ and
AddressSanitizer + UBSan and run as a child: reserve within capacity does
nothing, growth frees before it allocates (never two live blocks), a failed
allocation leaves the buffer empty and usable, moves transfer the block and
free the target's old one once, reset() is idempotent, and at exit every
allocation has been freed (LeakSanitizer agrees or the child fails).
"""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_device_buffer_cpp(tmp_path):
    exe = tmp_path / "device_buffer"
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), os.path.join(HERE, "device_buffer.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = out.stdout.split("\n")
    assert out.returncode == 0 and lines[-2] == "ok" and not out.stderr, out.stdout + out.stderr
    m = re.match(r"checks (\d+) allocs (\d+) frees (\d+)", lines[-3])
    assert m and int(m.group(1)) > 30 and int(m.group(2)) == int(m.group(3)) > 0, out.stdout
