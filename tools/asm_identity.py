#!/usr/bin/env python3
"""Codegen identity of a refactor: compare two device assembly files kernel by kernel.

    hipcc <FLAGS + EXTRA_FLAGS of elvis_amd/_build.py> --offload-device-only -S csrc/X.hip -o X.s     (old and new tree)
    python tools/asm_identity.py old/X.s new/X.s

A kernel is identical when its instruction text (comments and directives dropped, the file-wide numbering of local
labels .LBB<n>_<m> / .Lpost_getpc<n> normalised) and its .amdhsa_ block (registers, LDS, scratch) are equal.
Exit status 1 when a kernel present in both files differs or a kernel was added."""
import re
import sys


def kernels(path):
    text, hsa, cur, blk = {}, {}, None, None
    for line in open(path):
        st = line.split(";")[0].strip()
        if not st:
            continue
        if st.startswith(".amdhsa_kernel"):
            blk = hsa.setdefault(st.split()[1], [])
        elif st.startswith(".end_amdhsa_kernel"):
            blk = None
        elif blk is not None:
            blk.append(st)
        elif st.startswith(".Lfunc_end"):
            cur = None
        elif re.match(r"^[A-Za-z_]\w*:$", st):
            cur = text.setdefault(st[:-1], [])
        elif cur is not None and (st.startswith(".L") or not st.startswith(".")):
            cur.append(re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc#", re.sub(r"\.LBB\d+_", ".LBB#_", st)))
    return {k: (text[k], hsa[k]) for k in hsa}


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
differ = sorted(k for k in old.keys() & new.keys() if old[k] != new[k])
added = sorted(new.keys() - old.keys())
print(f"{sys.argv[2]}: {len(old)} -> {len(new)} kernels, {len(old.keys() & new.keys()) - len(differ)} identical "
      f"({sum(len(new[k][0]) for k in new)} instructions), {len(differ)} differ, {len(old.keys() - new.keys())} removed, "
      f"{len(added)} added")
for tag, names in (("differs", differ), ("added", added), ("removed", sorted(old.keys() - new.keys()))):
    for k in names:
        print(f"  {tag} {k}")
sys.exit(1 if differ or added else 0)
