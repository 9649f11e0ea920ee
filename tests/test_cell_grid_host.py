"""The descriptor of the shared cell grid (csrc/cell_grid.h: table size, cell clamp, dense / hashed decision, keys, bucket
count, slack) on the host: tests/host/cell_grid_check.cpp states every expectation from DESIGN.md section 3.9 and is built
with the host C++ compiler under AddressSanitizer and UBSan (their runtimes linked in statically; the float-to-int check is
switched on for the clamp of ``cell_of``), not linked against the HIP runtime, and run as a program of its own.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cell_grid_descriptor_under_sanitizers(tmp_path):
    exe = str(tmp_path / "cell_grid_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=undefined,float-cast-overflow", "-static-libasan",
           "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
           os.path.join(ROOT, "tests", "host", "cell_grid_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert built.returncode == 0, built.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout
    assert "cell_grid_check ok" in run.stdout
