#!/usr/bin/env python3
"""Compare the compiled gfx950 kernels of two builds of the library (no GPU needed).

    python tools/isa_diff.py A.so B.so        # exit code 1 on any difference, missing or added kernel symbol

For every kernel symbol: the disassembled instruction list and the metadata record (registers, spills, scratch) must be equal.
The gate of a change that is meant to leave every kernel as it was (a refactor of the sources, a header that moves).
"""
import sys
import tempfile

from lint_device_isa import code_objects, disassemble, kernel_metadata


def kernels(lib: str):
    """-> ({symbol: [instruction, ...]}, {kernel name: metadata record}) over every code object of a library."""
    ins, meta = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            ins.update(disassemble(co))
            meta.update({m["name"]: m for m in kernel_metadata(co)})
    return ins, meta


def main(a: str, b: str) -> int:
    (ia, ma), (ib, mb) = kernels(a), kernels(b)
    bad = 0
    for what, xa, xb in (("instructions", ia, ib), ("metadata", ma, mb)):
        for k in sorted(set(xa) | set(xb)):
            if k not in xa or k not in xb:
                bad += 1
                print(f"{what}: {k} only in {b if k not in xa else a}")
            elif xa[k] != xb[k]:
                bad += 1
                print(f"{what}: {k} differs")
    print(f"{len(ia)} / {len(ib)} kernel symbols, {len(ma)} / {len(mb)} metadata records, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
