"""Regenerate tests/golden/vmaf_fvmd_statement.npz: what the numpy statements tests/_vmaf_ref.py and tests/_fvmd_ref.py
give on their own fixtures when called without `mutant=` and `counts=`.

    python tools/make_vmaf_fvmd_statement_golden.py            # writes the file
    python tools/make_vmaf_fvmd_statement_golden.py --check    # compares with the file, byte for byte, and writes nothing

The file was first written from the statements as they stood before they took those two arguments;
tests/test_vmaf_fvmd_ledger.py holds today's statements to its bytes, so the arguments can only add.  Regenerate it only
when the contract itself changes, and say so in that change.

Stored: `vmaf_<h>x<w>` = features [3, 6] of `fixture(h, w)` for the first three of `SHAPES`, `vmaf_branch_pair` [2, 6],
`fvmd_border_64_rows` [3, 2176], `fvmd_border_static_gram` [3, 2] and `fvmd_border_static_scalars` [3] of the pair
("border_64", "static_64")."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _fvmd_ref as FR  # noqa: E402
import _vmaf_ref as VR  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "vmaf_fvmd_statement.npz")


def arrays():
    out = {f"vmaf_{h}x{w}": VR.features(*VR.fixture(h, w)) for h, w in VR.SHAPES[:3]}
    out["vmaf_branch_pair"] = VR.features(*VR.branch_pair())
    rows = FR.tracked("border_64")["rows"]
    gram, scalars = FR.gram_parts(rows, FR.tracked("static_64")["rows"])
    out["fvmd_border_64_rows"], out["fvmd_border_static_gram"], out["fvmd_border_static_scalars"] = rows, gram, scalars
    return out


if __name__ == "__main__":
    got = arrays()
    if "--check" in sys.argv:
        want = np.load(PATH)
        bad = [k for k in got if k not in want.files or got[k].tobytes() != want[k].tobytes()] + [k for k in want.files if k not in got]
        print("the same bytes" if not bad else f"differ: {bad}")
        sys.exit(1 if bad else 0)
    np.savez_compressed(PATH, **got)
    print(f"wrote {PATH}: {', '.join(f'{k} {v.shape}' for k, v in got.items())}")
