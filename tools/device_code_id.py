#!/usr/bin/env python3
"""Identity of the DEVICE code of a built library: sha256 of the .text section of its gfx950 code object.

A change of the host layer alone (csrc/rem2d.hip below "host side") must leave it as it was: the same kernels, byte for byte, in the
same order -- "same results, same kernel speed" without running anything.  Hashes and compares; inspects no instruction.  Runs
anywhere (no GPU):

    python tools/device_code_id.py [lib.so ...]            # one line per library (default: the three builds beside the package)
    python tools/device_code_id.py --against DIR [lib.so ...]   # ... and compared with the libraries of the same names in DIR; exit 1 if one differs
"""
import hashlib
import os
import sys
import tempfile

from check_handover_asm import LLVM, _run, code_object, default_libraries


def device_code_id(lib_path):
    """(sha256 hex, size in bytes) of the code object's .text."""
    with tempfile.TemporaryDirectory() as tmp:
        text = os.path.join(tmp, "text.bin")
        _run(LLVM + "/llvm-objcopy", "-O", "binary", "--only-section=.text", code_object(lib_path, tmp), text)
        with open(text, "rb") as f:
            blob = f.read()
    return hashlib.sha256(blob).hexdigest(), len(blob)


def main(argv):
    against = None
    if argv[:1] == ["--against"]:
        against, argv = argv[1], argv[2:]
    same = True
    for path in argv or default_libraries():
        digest, size = device_code_id(path)
        line = "%-20s .text %8d bytes  sha256 %s" % (os.path.basename(path), size, digest)
        if against is not None:
            other = device_code_id(os.path.join(against, os.path.basename(path)))
            line += "  " + ("== " if other[0] == digest else "!= %s in " % other[0]) + against
            same = same and other[0] == digest
        print(line)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
