"""Regenerate tests/golden/lpips.npz from the reference's own `calculate_lpips_per_frame`.

    python tools/make_lpips_golden.py   # needs the reference (ELVIS_REFERENCE, see oracle/make_golden.py)

What is pinned is the reference's wrapper (elvis.py:3163-3195), run from its own code through
`oracle.make_golden.import_reference()`: the BGR -> RGB flip, `.float() / 127.5 - 1.0`, the pairing of the two lists
(zip: the longer one is cut), the skipping of pairs with a None, the empty-input return.

The network itself stays BUILD-DEFINED: the `lpips` package and its weights are absent, so `_get_lpips_model` is
answered by the torch restatement of tests/_lpips_ref.py (float32, CPU) with the seed-0 synthetic weights of
`elvis_amd.weights.make_lpips_weights`, and `cv2.cvtColor(..., COLOR_BGR2RGB)` by a channel flip.

Only inputs and outputs are stored; the largest frame is 33 x 40.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import make_golden  # noqa: E402
import _lpips_ref as R  # noqa: E402

SEED = 0
H, W = 33, 40
H2, W2 = 31, 47


def main() -> None:
    ref_elvis, _ = make_golden.import_reference()
    cv2_stub = sys.modules["cv2"]
    assert not hasattr(cv2_stub, "GaussianBlur") and ref_elvis.lpips.LPIPS is object, "real cv2 / lpips installed: pin the packages instead"
    cv2_stub.COLOR_BGR2RGB = 4

    def cvt(img, code):
        assert code == cv2_stub.COLOR_BGR2RGB
        return img[:, :, ::-1]

    from elvis_amd.weights import make_lpips_weights
    net = R.Net(make_lpips_weights(SEED), torch.float32)
    asked = []

    def get_model(device="cpu"):
        asked.append(device)
        return net

    cv2_stub.cvtColor, ref_elvis._get_lpips_model = cvt, get_model
    rng = np.random.default_rng(20261019)

    def pair(h, w, sigma):
        yy, xx = np.mgrid[:h, :w]
        base = np.stack([120 + 70 * np.sin(yy / 4.0 + c) * np.cos(xx / 6.0 - 2 * c) for c in range(3)], axis=-1)
        ref = np.clip(base + rng.normal(0, 7, base.shape), 0, 255).astype(np.uint8)
        return ref, np.clip(ref.astype(np.float64) + rng.normal(0, sigma, ref.shape), 0, 255).astype(np.uint8)

    same = [pair(H, W, s) for s in (3, 10, 25, 6)]
    other = pair(H2, W2, 12)
    # entries 0, 1: scored; 2: reference missing; 3: decoded missing; 4: another size; the decoded list is one longer
    refs = [same[0][0], same[1][0], None, same[3][0], other[0]]
    decs = [same[0][1], same[1][1], same[2][1], None, other[1], same[2][1]]
    keep = [None if f is None else f.copy() for f in refs + decs]
    scores = ref_elvis.calculate_lpips_per_frame(refs, decs, device="cpu")
    assert len(scores) == 3 and asked == ["cpu"]
    assert all((k is None and f is None) or np.array_equal(k, f) for k, f in zip(keep, refs + decs))
    assert ref_elvis.calculate_lpips_per_frame([], decs, device="cpu") == [] and ref_elvis.calculate_lpips_per_frame(refs, [], device="cpu") == []
    swapped = ref_elvis.calculate_lpips_per_frame([f[:, :, ::-1] for f in (same[0][0], same[1][0])],
                                                  [f[:, :, ::-1] for f in (same[0][1], same[1][1])], device="cpu")
    out = dict(seed=np.asarray(SEED), frames_ref=np.stack([p[0] for p in same]), frames_dec=np.stack([p[1] for p in same]),
               other_ref=other[0], other_dec=other[1], scores=np.asarray(scores, np.float64),
               scores_channels_reversed=np.asarray(swapped, np.float64))
    path = os.path.join(make_golden.OUT, "lpips.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes; scores {scores}")


if __name__ == "__main__":
    main()
