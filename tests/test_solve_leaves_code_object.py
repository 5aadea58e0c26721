"""The overlay kernel in the built gfx950 code object: as k_solve_states, no scratch (each lane's node is a state
in registers, its frames are LDS words addressed by depth) and at most 64 KB of LDS per workgroup. Reads the
kernel's metadata as test_solve_code_object does; no GPU needed."""
import os
import re
import shutil

import pytest

import test_code_object
from test_code_object import LIB, LLVM, code_objects

KERNEL = "14k_solve_leavesE"


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(f"{LLVM}/llvm-readelf")),
                    reason="library not built or ROCm LLVM tools missing")
def test_solve_leaves_kernel_uses_no_scratch_and_fits_lds(tmp_path, monkeypatch):
    # on a copy: the unbundling helpers may rewrite their input, and earlier tests have loaded the library
    copy = tmp_path / "libuttt_engine_copy.so"
    shutil.copyfile(LIB, copy)
    monkeypatch.setattr(test_code_object, "LIB", str(copy))
    notes, _ = code_objects(tmp_path)
    found = 0
    for block in re.split(r"\n\s+- \.", notes):
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or KERNEL not in name.group(1) or name.group(1).endswith(".kd"):
            continue
        priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
        group = re.search(r"\.group_segment_fixed_size:\s+(\d+)", block)
        assert priv and group, block[:400]
        assert int(priv.group(1)) == 0, f"k_solve_leaves uses {priv.group(1)} bytes of scratch"
        # 4 B x 32 frames x 64 lanes x 4 waves
        assert 0 < int(group.group(1)) <= 65536, f"k_solve_leaves uses {group.group(1)} bytes of LDS"
        found += 1
    assert found, "k_solve_leaves not found in the code object"
