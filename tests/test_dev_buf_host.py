"""The owning buffers of the lattice, the FilterReg plan and the CPD plan (csrc/dev_buf.h, and csrc/cpd_buffers.h: the CPD
plan's all-or-nothing groups - every position of a failing allocation in the source group, the target group and a sweep queue
leaves the group empty with extents 0, unchanged extents allocate nothing, a queue larger in any one extent is re-created as a
whole and says so) on the host: tests/host/dev_buf_check.cpp is
built with the host C++ compiler under AddressSanitizer and UBSan (their runtimes linked in statically) against a fake
allocator, not linked against the HIP runtime, and run as a program of its own.  It checks that a failed allocation leaves a
buffer empty with the old block freed exactly once, that ``ensure`` allocates only above the capacity and then ``max(need, want)``, and that nothing is live after
destruction; the sanitizers add double frees, leaks and out-of-extent accesses.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dev_buf_under_sanitizers(tmp_path):
    exe = str(tmp_path / "dev_buf_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__",
           "-I" + os.path.join(rocm, "include"),
           os.path.join(ROOT, "tests", "host", "dev_buf_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert built.returncode == 0, built.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout
    assert "dev_buf_check ok" in run.stdout
