"""The descriptor-list helpers of csrc/kept.h (allocate zeroed, free, zero, get,
set and set's null-pointer rule) on host memory: tests/c/kept_arrays_main.cpp
renames the HIP calls to stubs, so no GPU is needed.  The lists are shaped like
the four accumulators': an absent array (no histogram, no pend), 5 of 7
arrays, 16 bytes of slack, slack alone."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_kept_arrays(tmp_path):
    exe = str(tmp_path / "kept_arrays")
    subprocess.run([HIPCC, "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c", "kept_arrays_main.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)
