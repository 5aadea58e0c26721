"""Host sanitizer run of the root noise's CPU side: uttt_root_noise_host (csrc/rules_api.cpp, csrc/uttt_noise.h)
built with AddressSanitizer + UBSan into a stand-alone program (tests/noise_asan/noise_asan.cpp) and run on 300
positions of random games, for alpha from 1/32 to 32. CPU only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None or shutil.which("make") is None, reason="needs g++ and make")
def test_noise_host_under_asan_ubsan(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(HERE, "noise_asan"), f"OUT={tmp_path}"], capture_output=True,
                       text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert " 0 failures" in out and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
