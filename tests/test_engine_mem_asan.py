"""Host sanitizer run of the engine's owning buffer type (csrc/engine_mem.h): the template instantiated with a
counting malloc / free policy that can fail the N-th allocation, built with AddressSanitizer (leak detection
on) + UBSan into a stand-alone program (tests/engine_mem_asan/engine_mem_asan.cpp). Grow / regrow / destroy,
a failing grow, and a group growth whose second of three allocations fails all end with no live block, nothing
freed twice and no capacity that a buffer does not have. CPU only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None or shutil.which("make") is None, reason="needs g++ and make")
def test_engine_buffers_under_asan_ubsan(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(HERE, "engine_mem_asan"), f"OUT={tmp_path}"], capture_output=True,
                       text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert " 0 live blocks" in out and " 0 failures" in out, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "ERROR: LeakSanitizer" not in out and "runtime error" not in out, \
        out[-4000:]
