"""The playout kernels in the built gfx950 code object run without scratch: each lane carries its game's
32-byte state and the legal mask in registers (csrc/uttt_playout.h picks words by selects, never by a dynamic
index into a local array). Reads the kernel descriptors' metadata as test_code_object does; no GPU needed."""
import os
import shutil

import pytest

import test_code_object
from test_code_object import LIB, LLVM, kernel_metadata

KERNELS = {"k_playout_leaves": "16k_playout_leavesE", "k_playout_states": "16k_playout_statesE"}


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(f"{LLVM}/llvm-readelf")),
                    reason="library not built or ROCm LLVM tools missing")
def test_playout_kernels_use_no_scratch(tmp_path, monkeypatch):
    # on a copy: objcopy without an output file rewrites its input in place, and by now earlier tests have
    # loaded the library into this process (a rewritten mapped file loses its relocations)
    copy = tmp_path / "libuttt_engine_copy.so"
    shutil.copyfile(LIB, copy)
    monkeypatch.setattr(test_code_object, "LIB", str(copy))
    meta = kernel_metadata(tmp_path)
    for label, frag in KERNELS.items():
        hits = {k: v for k, v in meta.items() if frag in k}
        assert hits, f"{label} not found in the code object"
        for k, v in hits.items():
            assert v == 0, f"{label} ({k}) uses {v} bytes of scratch"
