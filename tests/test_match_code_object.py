"""k_match_move and k_match_lists are in the built gfx950 code object and run without scratch: the move rule's
reductions and prefix sum stay in registers, the list scan in registers and LDS (csrc/engine/match.h). Reads the
kernel descriptors' metadata as test_tree_reuse_code_object does; no GPU needed."""
import os
import shutil

import pytest

import test_code_object
from test_code_object import LIB, LLVM, kernel_metadata

KERNELS = {"k_match_move": "12k_match_moveE", "k_match_lists": "13k_match_listsE"}


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(f"{LLVM}/llvm-readelf")),
                    reason="library not built or ROCm LLVM tools missing")
def test_match_kernels_use_no_scratch(tmp_path, monkeypatch):
    # on a copy: objcopy without an output file rewrites its input in place (see test_playout_code_object)
    copy = tmp_path / "libuttt_engine_copy.so"
    shutil.copyfile(LIB, copy)
    monkeypatch.setattr(test_code_object, "LIB", str(copy))
    meta = kernel_metadata(tmp_path)
    for label, frag in KERNELS.items():
        hits = {k: v for k, v in meta.items() if frag in k}
        assert hits, f"{label} not found in the code object"
        for k, v in hits.items():
            assert v == 0, f"{label} ({k}) uses {v} bytes of scratch"
