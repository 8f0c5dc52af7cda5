"""The tip forms of engine creation (state byte, mask, look-up code, 0/1 partial row, and the way
back from caller-supplied partials: libsbn_amd/csrc/mi_phylo_tip_forms.h) are plain C++ that the
preparation kernel and the host path share: tests/cpp/tip_forms_check.cpp checks the rule on the
CPU, built with the address and undefined-behaviour sanitizers (their runtimes linked into it), as
a stand-alone program.  No GPU, and nothing is loaded into this process."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tip_forms_follow_their_tables(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/tip_forms_check.cpp"
    exe = str(tmp_path / "tip_forms_check")
    build = subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                            os.path.join(REPO, "tests", "cpp", "tip_forms_check.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "0 failures" in run.stdout
