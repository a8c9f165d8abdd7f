"""Kernel-by-kernel comparison of the gfx950 code of two libti_hip.so builds (CPU only: ROCm's LLVM tools).

    python tools/isa_compare.py OLD.so NEW.so

Every kernel symbol of OLD must exist in NEW with the same instructions (branch targets and other addresses masked, since a
kernel's offset inside its code object moves when others are added next to it).  Prints one line per differing or missing
kernel, the counts, and the kernels NEW adds; exits 1 if any kernel of OLD differs or is missing.  llvm-objdump's "..." (zero fill it
skips behind a kernel's last instruction; whether there is any depends on what follows the kernel in its code object) is no instruction
and is left out.
"""
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from test_build_isa import code_objects, kernels as co_kernels  # noqa: E402  (the fat-binary unbundling and disassembly)


def kernels(lib):
    """{demangled kernel symbol: [instructions]} over every gfx950 code object of `lib` (first occurrence of a symbol), branch
    targets masked, zero-fill marks dropped."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            for name, insns in co_kernels(co).items():
                if name not in out:
                    out[name] = [re.sub(r"\b0x[0-9a-f]+\b|<[^>]*>", "#", i) if i.startswith(("s_cbranch", "s_branch")) else i for i in insns if i != "..."]
    return out


def main(old, new):
    a, b = kernels(old), kernels(new)
    same = [k for k in a if k in b and a[k] == b[k]]
    diff = [k for k in a if k in b and a[k] != b[k]]
    missing = [k for k in a if k not in b]
    added = sorted(k for k in b if k not in a)
    for k in diff:
        print("DIFFERS", k)
    for k in missing:
        print("MISSING", k)
    print(f"{len(a)} symbols in {old}; identical in {new}: {len(same)}; differing: {len(diff)}; missing: {len(missing)}; "
          f"added: {len(added)} ({sum(len(b[k]) for k in added)} instructions)")
    for k in added:
        print("ADDED", k)
    return 1 if diff or missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
