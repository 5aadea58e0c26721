"""Host sanitizer run of the solver overlay's CPU side: uttt_solve_overlay_host (csrc/rules_api.cpp,
csrc/uttt_solve.h) built with AddressSanitizer + UBSan into a stand-alone program
(tests/solve_leaves_asan/solve_leaves_asan.cpp) and run over exact-size row buffers on late positions of random
games, with both priors modes, a budget stop, a padded row stride and a NULL status. CPU only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None or shutil.which("make") is None, reason="needs g++ and make")
def test_solve_overlay_host_under_asan_ubsan(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(HERE, "solve_leaves_asan"), f"OUT={tmp_path}"],
                       capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert " 0 failures" in out and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
