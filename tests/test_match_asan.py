"""Host sanitizer run of match play's CPU side: uttt_match_move_host, uttt_match_draw_host and uttt_match_check_host
(csrc/rules_api.cpp, csrc/uttt_match.h) built with AddressSanitizer + UBSan into a stand-alone program
(tests/match_asan/match_asan.cpp) and run over 400 games played through the move rule. CPU only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None or shutil.which("make") is None, reason="needs g++ and make")
def test_match_host_under_asan_ubsan(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(HERE, "match_asan"), f"OUT={tmp_path}"], capture_output=True,
                       text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert " 0 failures" in out and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
