"""The geometry of the multi-level grid search (csrc/grid_search.h: centre cell, clip, shell predicate, box distance, shell
bound - what the 1-NN walk, the k-NN walk and the radius count of csrc/grid_search.hip are correct by) on the host:
tests/host/grid_search_check.cpp drives the header with a plain CPU shell loop over small clouds on dense and hashed grids of
two to four levels and compares with brute force (every cell of a clipped cube on exactly one shell; a finished walk holds the
k best of the whole cloud, k = 1, 8, 64; the clip keeps every point within rho; the radius count's cube counts every point
within r once), with queries inside, on the box, 10^6 extents away and near 2^52 cell edges.  It is built with the host C++
compiler under AddressSanitizer and UBSan (their runtimes linked in statically, the float-to-int check switched on) with
-ffp-contract=off, as the header asks, not linked against the HIP runtime, and run as a program of its own.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grid_search_geometry_under_sanitizers(tmp_path):
    exe = str(tmp_path / "grid_search_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow",
           "-fno-sanitize-recover=undefined,float-cast-overflow", "-static-libasan", "-static-libubsan",
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
           os.path.join(ROOT, "tests", "host", "grid_search_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert built.returncode == 0, built.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout
    assert "grid_search_check ok" in run.stdout
