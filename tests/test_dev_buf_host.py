"""The owning buffers of the lattice, the FilterReg plan and the CPD plan (csrc/dev_buf.h, and csrc/cpd_buffers.h: the CPD
plan's all-or-nothing groups - every position of a failing allocation in the source group, the target group and a sweep queue
leaves the group empty with extents 0, unchanged extents allocate nothing, a queue larger in any one extent is re-created as a
whole and says so) on the host: tests/host/dev_buf_check.cpp is
built with the host C++ compiler under AddressSanitizer and UBSan (their runtimes linked in statically) against a fake
allocator, not linked against the HIP runtime, and run as a program of its own.  It checks that a failed allocation leaves a
buffer empty with the old block freed exactly once, that ``ensure`` allocates only above the capacity and then ``max(need, want)``, and that nothing is live after
destruction; the sanitizers add double frees, leaks and out-of-extent accesses.  The same program checks ``reset_group``, the
all-or-nothing step for buffers of different element types that every handle of the library sizes its groups with.  No GPU.

``test_no_raw_device_allocation`` keeps the rule that makes this enough: dev_buf.h is the only file of the library that calls
the device allocator (of any flavour, in any subdirectory)."""
import os
import re
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


# any allocator or release call of the HIP runtime, whatever its flavour: hipMalloc, hipMallocAsync, hipMallocManaged,
# hipExtMallocWithFlags, hipHostMalloc, hipMemAllocPitch, hipFree, hipFreeAsync, hipHostFree, ... with or without a space
RAW_ALLOCATION = re.compile(r"\bhip\w*(Malloc|Alloc|Free)\w*\s*\(")
SOURCE_SUFFIXES = (".hip", ".h", ".hpp", ".hh", ".inc", ".cpp", ".cc", ".cu", ".cuh")


def test_no_raw_device_allocation():
    csrc = os.path.join(ROOT, "probreg_amd", "csrc")
    sources = sorted(os.path.join(d, f) for d, _, files in os.walk(csrc) for f in files if f.endswith(SOURCE_SUFFIXES))
    assert len(sources) > 20 and os.path.join(csrc, "dev_buf.h") in sources
    raw = []
    for path in sources:
        if path == os.path.join(csrc, "dev_buf.h"):
            continue
        with open(path) as f:
            for no, line in enumerate(f, 1):
                if RAW_ALLOCATION.search(line):
                    raw.append("%s:%d: %s" % (os.path.relpath(path, ROOT), no, line.strip()))
    assert not raw, "device and pinned memory is owned through csrc/dev_buf.h (DevBuf, HostBuf):\n" + "\n".join(raw)
    for call in ("hipMalloc(&p, n)", "hipFree (p)", "hipMallocAsync(&p, n, st)", "hipFreeAsync(p, st)", "hipHostMalloc(&p, n, 0)",
                 "hipExtMallocWithFlags(&p, n, f)", "hipMemAllocPitch(&p, &pitch, w, h, 4)"):
        assert RAW_ALLOCATION.search(call), call
    for call in ("hipMemcpyAsync(a, b, n, k, st)", "hipGetLastError()", "buf.reset(n)", "// hipFree drains the device"):
        assert not RAW_ALLOCATION.search(call), call
