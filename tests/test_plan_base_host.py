"""The host side that every handle of the library shares (csrc/plan_base.h) on the host: tests/host/plan_base_check.cpp is built
with the host C++ compiler under AddressSanitizer and UBSan (their runtimes linked in statically) against fakes of the HIP
runtime, not linked against it, and run as a program of its own.  With a toy handle it checks that a create with a NULL
``out`` or a device out of range constructs nothing and leaves ``*out`` alone, that a device that cannot be selected is
PRG_ERR_HIP with nothing live, that a failing per-handle init returns its status after exactly one destruction, that destroy
takes NULL, deletes after a failing drain and gives the caller's device back, that the checked entry (PRG_ENTER) restores the
device on every return path and does not run the body when the selection fails, and that the copy-out skips a NULL optional
output, drains the stream before the first copy and copies exactly ``count`` elements; the sanitizers add leaks, double frees
and overruns.  No GPU.

``test_every_device_selection_is_checked`` keeps the rule that makes this enough: plan_base.h is the only file of the library
that constructs a DeviceGuard or asks for the device count (besides prg_device_count itself)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "probreg_amd", "csrc")


def test_plan_base_under_sanitizers(tmp_path):
    exe = str(tmp_path / "plan_base_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__",
           "-I" + os.path.join(rocm, "include"),
           os.path.join(ROOT, "tests", "host", "plan_base_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert built.returncode == 0, built.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout
    assert "plan_base_check ok" in run.stdout


def test_every_device_selection_is_checked():
    sources = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))
    assert len(sources) > 20 and "plan_base.h" in sources
    found = []
    for name in sources:
        with open(os.path.join(CSRC, name)) as f:
            for no, line in enumerate(f, 1):
                code = line.split("//")[0]
                if re.search(r"\bDeviceGuard\b", code) and name != "plan_base.h":
                    found.append("%s:%d: %s" % (name, no, line.strip()))
                if "hipGetDeviceCount" in code and name not in ("plan_base.h", "misc.hip"):
                    found.append("%s:%d: %s" % (name, no, line.strip()))
    assert not found, "entry points select their device with PRG_ENTER and handles are created by create_handle:\n" + "\n".join(found)
