"""Host sanitizer run of tree reuse's CPU side: uttt_reroot_host (csrc/rules_api.cpp, csrc/uttt_reroot.h) built
with AddressSanitizer + UBSan into a stand-alone program (tests/tree_reuse_asan/tree_reuse_asan.cpp) and run on
trees grown with the engine's append semantics, re-rooted at every move of their roots. CPU only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None or shutil.which("make") is None, reason="needs g++ and make")
def test_reroot_host_under_asan_ubsan(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(HERE, "tree_reuse_asan"), f"OUT={tmp_path}"], capture_output=True,
                       text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert " 0 failures" in out and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
