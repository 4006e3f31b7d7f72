"""Mutants of the 3x3 sum that tests/_rrdb_ref.py and tests/_srvgg_ref.py share: the statement's sum with one clause of
csrc/sr_conv3x3.h changed, each a plausible slip of the tile body.  `mutated_sum` gives z = sum x^ w^ (no bias) of the
mutant; the statements put it in the place of their own sum and keep their own error model, so that the ledger
(tests/test_sr_ledger.py) can count the distance in the case's bounds.

The tile is the kernel's, SR_TY x SR_TX pixels and SR_KC channels a chunk, read from the header's text.

    tap_corner_00     pixel (0, 0) of every image misses the tap (ky, kx) = (2, 2), the one corner tap that reads a pixel there
    halo_col_32       output column SR_TX (the first of the second tile column) is summed over a halo one column on
    halo_row_8        output row SR_TY (the first of the second tile row) is summed over a halo one row on
    frag_col_16       where the image ends at the seam of the two 16-column fragments (w % SR_TX == 16) the zero border right
                      of it holds the last column again: the halo column the second fragment begins on, read one column off
    kchunk_last       tile (0, 0) of image 0 misses its last K chunk
    taps_transposed   ky and kx exchanged
    weights_trunc     the weights rounded to f16 toward zero (`weights` gives them; the sum itself is the statement's)
"""
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from _convref import rne16, trunc16

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "elvis_amd", "csrc", "sr_conv3x3.h")


def constants():
    """(SR_TY, SR_TX, SR_KC) as the header states them."""
    m = re.search(r"constexpr\s+int\s+SR_TY\s*=\s*(\d+)\s*,\s*SR_TX\s*=\s*(\d+)\s*,\s*SR_KC\s*=\s*(\d+)\s*;", open(HEADER).read())
    return int(m.group(1)), int(m.group(2)), int(m.group(3))


SR_TY, SR_TX, SR_KC = constants()
SUM = ("tap_corner_00", "halo_col_32", "halo_row_8", "frag_col_16", "kchunk_last", "taps_transposed")
WEIGHTS = ("weights_trunc",)


def weights(w, mutant=None):
    """w^ of the statement: fp32 OIHW rounded to f16, to nearest even - or toward zero."""
    return trunc16(w.double()) if mutant == "weights_trunc" else rne16(w.double())


def round_u8(q, mutant=None):
    """q = 255 clamp(y, 0, 1) in float64 -> the byte (int64): half to even, as numpy rounds and as the two epilogues say they do;
    "u8_half_up": floor(q + 0.5); "u8_truncate": floor(q)."""
    if mutant is None:
        return torch.from_numpy(np.round(q.numpy())).to(torch.int64)
    if mutant not in ("u8_half_up", "u8_truncate"):
        raise ValueError("unknown mutant")
    return torch.floor(q + 0.5 if mutant == "u8_half_up" else q).to(torch.int64)


def mutated_sum(x_hat, w_hat, mutant):
    """x_hat NCHW float64 on the output grid (after any upsample), w_hat OIHW float64: the mutant's sum, no bias."""
    conv = lambda t, k: F.conv2d(t, k, None, padding=1)
    z = conv(x_hat, w_hat)
    n, c, h, w = x_hat.shape
    if mutant == "tap_corner_00":
        if h > 1 and w > 1:
            z[:, :, 0, 0] -= torch.einsum("nc,oc->no", x_hat[:, :, 1, 1], w_hat[:, :, 2, 2])
    elif mutant == "halo_col_32":
        if w > SR_TX:
            z[..., SR_TX] = conv(F.pad(x_hat[..., 1:], (0, 1)), w_hat)[..., SR_TX]
    elif mutant == "halo_row_8":
        if h > SR_TY:
            z[..., SR_TY, :] = conv(F.pad(x_hat[..., 1:, :], (0, 0, 0, 1)), w_hat)[..., SR_TY, :]
    elif mutant == "frag_col_16":
        if w % SR_TX == SR_TX // 2:
            z = F.conv2d(F.pad(torch.cat((x_hat, x_hat[..., -1:]), -1), (1, 0, 1, 1)), w_hat, None)
    elif mutant == "kchunk_last":
        less = conv(x_hat[:, :c - SR_KC], w_hat[:, :c - SR_KC]) if c > SR_KC else torch.zeros_like(z)
        z[0, :, :SR_TY, :SR_TX] = less[0, :, :SR_TY, :SR_TX]
    elif mutant == "taps_transposed":
        z = conv(x_hat, w_hat.transpose(2, 3))
    else:
        raise ValueError("unknown mutant")
    return z
