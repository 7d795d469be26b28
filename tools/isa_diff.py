"""Are the gfx950 kernels of two builds of the library the same, instruction for instruction?
    python tools/isa_diff.py <libA> <libB> [<regex>]
<regex>: removed from every kernel name before the two sides are matched (a template that gained a defaulted trailing argument
renames all its instantiations: "(?<=k_gcn_layer_psILb.ELb.ELi.ELb.ELi.ELb.E)Lb0E" matches the old names to the new ones).
Compares, per kernel, the whole stream of (mnemonic, operands) of the disassembly; prints the kernels that differ or exist on one
side only and exits non-zero if there are any.  The check of a refactoring that must not touch the device code; no GPU."""
import sys

import isa_census


def streams(lib):
    # (entries without an address are llvm-objdump's file-header lines: they hold the path of a temporary file)
    return {k: [(mn, tuple(ops)) for a, mn, ops, _t, _code in ins if a is not None] for k, ins in isa_census.kernels(lib).items()}


if __name__ == "__main__":
    if len(sys.argv) not in (3, 4):
        sys.exit(__doc__)
    a, b = streams(sys.argv[1]), streams(sys.argv[2])
    if len(sys.argv) == 4:
        import re
        a, b = ({re.sub(sys.argv[3], "", k): v for k, v in side.items()} for side in (a, b))
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"only in {sys.argv[2] if k not in a else sys.argv[1]}: {k}")
        elif a[k] != b[k]:
            first = next((i for i, (p, q) in enumerate(zip(a[k], b[k])) if p != q), min(len(a[k]), len(b[k])))
            print(f"differs: {k}\n    {len(a[k])} / {len(b[k])} instructions, first difference at instruction {first}")
        else:
            continue
        bad += 1
    print(f"{len(a)} / {len(b)} kernels, {bad} differ or are on one side only")
    sys.exit(1 if bad else 0)
