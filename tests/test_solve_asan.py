"""Host sanitizer run of the exact endgame solver's CPU side: uttt_solve_host (csrc/rules_api.cpp,
csrc/uttt_solve.h) built with AddressSanitizer + UBSan into a stand-alone program
(tests/solve_asan/solve_asan.cpp) and run on late positions of random games, a budget stop and the deepest
accepted position. CPU only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None or shutil.which("make") is None, reason="needs g++ and make")
def test_solve_host_under_asan_ubsan(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(HERE, "solve_asan"), f"OUT={tmp_path}"], capture_output=True,
                       text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert " 0 failures" in out and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
