"""The union-find of the DBSCAN link (csrc/union_find.h: find with path halving, hook of the larger root under the smaller, by
atomic minimum and compare-and-swap only) on the host: tests/host/union_find_check.cpp drives the header with random graphs,
paths and sparse vertex sets of up to 4000 vertices, edges in random orders, against a sequential reference (the root of every
component is its smallest vertex), checks parent[x] <= x after every operation, and repeats it with eight threads over
std::atomic<int>.  Built with the host C++ compiler under AddressSanitizer and UBSan (their runtimes linked in statically), not
linked against the HIP runtime, and run as a program of its own.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_union_find_under_sanitizers(tmp_path):
    exe = str(tmp_path / "union_find_check")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "host", "union_find_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert built.returncode == 0, built.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout
    assert "union_find_check ok" in run.stdout
