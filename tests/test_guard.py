"""The guard of the C boundary (orbx_internal.hpp orbx_guard: every extern "C" entry point that can allocate runs its body inside
it): return values pass through, std::bad_alloc and anything else become ORBX_ERR_HIP with their two texts, a null handle gets the
code alone, nothing escapes.  Host-only C++, built with g++ (once more with -fsanitize=address,undefined)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True])
def test_guard(tmp_path, sanitize):
    exe = str(tmp_path / "guard_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "guard_check.cpp"), "-o", exe] +
                   (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []), check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "guard ok" in r.stdout, r.stdout + r.stderr
