"""The two staging plans of orbx_internal.hpp ("Host staging"): UploadPlan states every host table of a device form once
(offset, source, bytes; 256-byte aligned pieces; a null source or no bytes reserve and copy nothing) and OutputPlan every output of a
host form (device address, host destination, the copy back: whole, or the n elements the download itself tells).  tests/plan_check.cpp
runs them over a ring and a host-call skeleton of its own, whose buffers are exactly as large as asked for: empty pieces, null sources,
a piece of 1 byte beside one of 257, pieces made in place, the partial copy, and one piece more than a plan holds.  Host-only C++, built
with g++ (once more with -fsanitize=address,undefined)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True])
def test_plans(tmp_path, sanitize):
    exe = str(tmp_path / "plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "plan_check.cpp"), "-o", exe] +
                   (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []), check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "plans ok" in r.stdout, r.stdout + r.stderr
