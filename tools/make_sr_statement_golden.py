"""Regenerate tests/golden/sr_statement.npz: what the float64 statements tests/_rrdb_ref.py and tests/_srvgg_ref.py give
on 9 x 33 inputs when called without `mutant=`.

    python tools/make_sr_statement_golden.py            # writes the file
    python tools/make_sr_statement_golden.py --check    # compares with the file, byte for byte, and writes nothing

The file was first written from the statements as they stood before they took that argument; tests/test_sr_ledger.py
holds today's statements to its bytes, so the argument can only add.  Regenerate it only when the contract itself
changes, and say so in that change.

The inputs are written out by formula (no random generator) and are dyadic - activations in sixteenths, weights in
256ths, biases in eighths - so every sum of the statements is exact in float64 whatever order a convolution routine adds
in, and the recorded bytes do not depend on the machine.  Stored, a few channels or rows of each to keep the file small:
`rrdb_ref` / `rrdb_e` (cin 64, cout 32, lrelu, s0 0.2, s1 0.5, r1 and r2), `rrdb_ups_ref` / `rrdb_ups_e` (cin 32, cout 64,
upsample), `rrdb_u8_byte` / `rrdb_u8_near`, `layer_ref` / `layer_e`, `tail_ref` / `tail_e`, `tail_u8_byte` / `tail_u8_near`."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _rrdb_ref as RR  # noqa: E402
import _srvgg_ref as SR  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "sr_statement.npz")
H, W = 9, 33


def _grid(*dims):
    return torch.meshgrid(*[torch.arange(d) for d in dims], indexing="ij")


def _x(n, c, h, w, k):
    i, cc, yy, xx = _grid(n, c, h, w)
    return ((i * 29 + cc * 5 + yy * 37 + xx * 11 + k) % 129 - 64).double() / 16.0          # NCHW, sixteenths in [-4, 4]


def _w(cout, cin, k):
    co, ci, ky, kx = _grid(cout, cin, 3, 3)
    return ((co * 13 + ci * 7 + ky * 31 + kx * 17 + (co * ci) % 5 + k) % 65 - 32).float() / 256.0


def _b(cout, k):
    return ((torch.arange(cout) * 5 + k) % 17 - 8).float() / 8.0


def arrays():
    out = {}
    r = RR.conv_ref(_x(1, 64, H, W, 0), _w(32, 64, 0), _b(32, 0), lrelu=True, s0=0.2, s1=0.5, r1=_x(1, 32, H, W, 3), r2=_x(1, 32, H, W, 7))
    out["rrdb_ref"], out["rrdb_e"] = r.ref[:, ::4].numpy(), r.e[:, ::4].numpy()
    r = RR.conv_ref(_x(1, 32, H, W, 1), _w(64, 32, 1), _b(64, 1), upsample=True)
    out["rrdb_ups_ref"], out["rrdb_ups_e"] = r.ref[:, ::16].numpy(), r.e[:, ::16].numpy()
    r = RR.conv_ref(_x(1, 32, H, W, 2) / 16.0, _w(3, 32, 2), _b(3, 2) / 4.0 + 0.5, s1=0.5, r1=_x(1, 3, H, W, 5) / 8.0)
    byte, near = RR.u8_ref(r)
    out["rrdb_u8_byte"], out["rrdb_u8_near"] = byte.numpy().astype(np.uint8), near.numpy()
    slope = ((torch.arange(64) * 11) % 23 - 9).float() / 8.0
    r = SR.conv_ref(_x(1, 64, H, W, 4), _w(64, 64, 4), _b(64, 4), slope)
    out["layer_ref"], out["layer_e"] = r.ref[:, ::8].numpy(), r.e[:, ::8].numpy()
    r = SR.tail_ref(_x(1, 64, H, W, 6) / 16.0, _w(48, 64, 6), _b(48, 6) / 8.0, _x(1, 3, H, W, 8) / 4.0 + 0.5)
    out["tail_ref"], out["tail_e"] = r.ref[:, :, ::3].numpy(), r.e[:, :, ::3].numpy()
    byte, near = SR.u8_ref(r)
    out["tail_u8_byte"], out["tail_u8_near"] = byte.numpy().astype(np.uint8), near.numpy()
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


if __name__ == "__main__":
    got = arrays()
    if "--check" in sys.argv:
        want = np.load(PATH)
        bad = [k for k in got if k not in want.files or got[k].tobytes() != want[k].tobytes()] + [k for k in want.files if k not in got]
        print("the same bytes" if not bad else f"differ: {bad}")
        sys.exit(1 if bad else 0)
    np.savez_compressed(PATH, **got)
    print(f"wrote {PATH}: {', '.join(f'{k} {v.shape}' for k, v in got.items())}")
