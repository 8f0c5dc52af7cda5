"""The offset arithmetic of the host-pointer calls (packing, tree slices, the scratch of the
shards: libsbn_amd/csrc/mi_phylo_host_arrays.h) is plain C++ without HIP: tests/cpp/host_arrays_check.cpp
walks every call kind's array lists on the CPU, built with the address and undefined-behaviour
sanitizers (their runtimes linked into it), as a stand-alone program.  No GPU, and nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_array_offsets_cover_slice_and_add_up(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/host_arrays_check.cpp"
    exe = str(tmp_path / "host_arrays_check")
    build = subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                            os.path.join(REPO, "tests", "cpp", "host_arrays_check.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "0 failures" in run.stdout
