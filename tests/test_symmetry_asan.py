"""Host sanitizer run of the board symmetries' CPU side: uttt_sym_action_perm, uttt_sym_compose, uttt_sym_inverse,
uttt_states_transform_host and uttt_states_symmetry_host (csrc/rules_api.cpp, csrc/uttt_sym.h) built with
AddressSanitizer + UBSan into a stand-alone program (tests/symmetry_asan/symmetry_asan.cpp) and run on 400 positions
of random games. CPU only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None or shutil.which("make") is None, reason="needs g++ and make")
def test_symmetry_host_under_asan_ubsan(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(HERE, "symmetry_asan"), f"OUT={tmp_path}"], capture_output=True,
                       text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert " 0 failures" in out and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
