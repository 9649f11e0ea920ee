"""The workspace layout of the non-rigid and BCPD solve drivers (csrc/cpd_solve_layout.h: the low-rank split, the small /
look-ahead decision, and one carving per driver) on the host: tests/host/solve_layout_check.cpp writes out every total and
region order as a formula and is built with the host C++ compiler under AddressSanitizer and UBSan (their runtimes linked in
statically), includes nothing but that header, and is run as a program of its own.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_solve_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "solve_layout_check")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "host", "solve_layout_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert built.returncode == 0, built.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout
    assert "solve_layout_check ok" in run.stdout
