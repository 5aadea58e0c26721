#!/usr/bin/env python3
"""The identity of a built library's device code, for a refactor that must leave it as it was: per library the
sha256 of its gfx950 code objects' concatenated .text, of their concatenated .rodata and of their
`llvm-readelf --notes` output (kernel names, register counts, LDS and scratch sizes). Two builds with the same three
hashes run the same device code. No GPU needed.
usage: python tools/code_object_sha.py LIBRARY.so [LIBRARY.so ...]"""
import hashlib
import os
import pathlib
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import test_code_object  # noqa: E402


def section(obj, name, tmp):
    out = tmp / "section.bin"
    subprocess.run([f"{test_code_object.LLVM}/llvm-objcopy", "-O", "binary", f"--only-section={name}", str(obj),
                    str(out)], check=True, capture_output=True)
    return out.read_bytes()


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    for lib in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as d:
            tmp = pathlib.Path(d)
            # on a copy: objcopy without an output file rewrites its input in place
            test_code_object.LIB = shutil.copyfile(lib, tmp / "lib_copy.so")
            notes, objs = test_code_object.code_objects(tmp)
            parts = {".text": b"".join(section(o, ".text", tmp) for o in objs),
                     ".rodata": b"".join(section(o, ".rodata", tmp) for o in objs), "notes": notes.encode()}
            for name, data in parts.items():
                print(f"{hashlib.sha256(data).hexdigest()}  {lib} {name} ({len(data)} bytes, {len(objs)} code objects)")


if __name__ == "__main__":
    main()
