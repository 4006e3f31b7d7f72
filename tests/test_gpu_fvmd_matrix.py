"""The edge matrix of csrc/fvmd.hip on the device (tests/_fvmdcases.py): the Jacobi sweeps on both sides of 64 KiB and of
128 KiB of LDS and on the skinniest shapes, the histogram kernel on hand-made tracks (bin boundaries, zero vectors, -0.0,
1e-300 and 1e6), the Gram kernels' block edges, and the shortest clip the tracker takes.

Bound: the project's own, R.BAR = 1e-9 * max(1, |value|) against tests/_fvmd_ref.py and np.linalg.svd, and for the
distance 1e-9 * max(1, tr S1 + tr S2 + |dmu|^2), as tests/test_gpu_fvmd.py carries them; nothing new.  A vote on a bin
boundary is continuous in the result (the two shares are (1 - f) m and f m), so a last-bit difference in atan2 moves a
histogram value by rounding only, whichever bin the device chooses."""
import numpy as np
import pytest
import torch

import _fvmd_ref as R
import _fvmdcases as K
from elvis_amd import _lib, fvmd

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)                        # a copy: the shared inputs are read-only


def _launch():
    return _lib.lib().elvis_last_launch().decode()


def _report(name, got, want, scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    denom = np.maximum(1.0, np.abs(want)) if scale is None else max(1.0, scale)
    worst = float((np.abs(got - want) / denom).max()) if got.size else 0.0
    print(f"{name}: worst |device - statement| / scale = {worst:.3g} (bar {R.BAR:g})")
    return worst


@pytest.mark.parametrize("k,ln", list(K.JACOBI), ids=lambda v: str(v))
def test_jacobi_at_the_lds_boundaries(gpu_device, k, ln):
    mat = _dev(K.jacobi_matrix(k, ln), gpu_device)
    first = fvmd.singular_values_device(mat)
    assert _launch() == K.jacobi_kernels(k, ln)[0], K.JACOBI[k, ln]
    assert torch.equal(fvmd.singular_values_device(mat), first)                                    # two runs: the same bytes
    assert torch.equal(mat, _dev(K.jacobi_matrix(k, ln), gpu_device))                              # a copy was rotated
    got = np.sort(first.cpu().numpy())[::-1]
    want = K.jacobi_expected(k, ln)
    r = min(k, ln)
    assert got.shape == (k,) and np.isfinite(got).all()
    assert _report(f"jacobi {k} x {ln} ({K.JACOBI[k, ln]})", got[:r], want) <= R.BAR
    tail = float(np.abs(got[r:]).max(initial=0.0))
    print(f"jacobi {k} x {ln}: largest value past min(k, len) = {tail:.3g} (bar {R.BAR * max(1.0, got[0]):.3g})")
    assert tail <= R.BAR * max(1.0, got[0])


@pytest.mark.parametrize("n,m,d", K.FRECHET, ids=lambda v: str(v))
def test_distance_at_the_lds_boundary(gpu_device, n, m, d):
    a, b = K.frechet_rows(n, m, d)
    a_d, b_d = _dev(a, gpu_device), _dev(b, gpu_device)
    # the Jacobi form the distance takes: _frechet_tensor rotates the fewer vectors, so the Gram matrix is min x max
    lo, hi = (a_d, b_d) if n <= m else (b_d, a_d)
    gram, _ = fvmd.gram_device(lo, hi)
    assert tuple(gram.shape) == (min(n, m), max(n, m))
    sv = fvmd.singular_values_device(gram)
    assert _launch() == K.jacobi_kernels(min(n, m), max(n, m))[0] == K.FRECHET_JACOBI[n, m, d]
    want_sv = np.linalg.svd(R.gram_parts(*((a, b) if n <= m else (b, a)))[0], compute_uv=False)
    assert _report(f"singular values of the {min(n, m)} x {max(n, m)} Gram matrix", np.sort(sv.cpu().numpy())[::-1], want_sv) <= R.BAR
    got = fvmd.frechet_distance_device(a_d, b_d)
    assert _launch() == "fvmd_finish_kernel"
    assert _report(f"distance {n} x {m} x {d}", got, R.frechet(a, b), scale=R.fd_scale(a, b)) <= R.BAR
    assert fvmd.frechet_distance_device(a_d, b_d) == got
    back = fvmd.frechet_distance_device(b_d, a_d)
    assert abs(back - R.frechet(a, b)) <= R.BAR * max(1.0, R.fd_scale(a, b))


@pytest.mark.parametrize("name", list(K.HIST))
def test_histograms_of_hand_made_tracks(gpu_device, name):
    tracks = _dev(K.hist_tracks(name), gpu_device)
    want = K.hist_expected(name)
    rows = fvmd.motion_features_device(tracks)
    assert _launch() == "fvmd_hist_kernel"
    assert rows.shape == want.shape == (K.HIST[name][0], fvmd.feature_length(K.HIST[name][1]))
    assert _report(f"rows {name}", rows.cpu().numpy(), want) <= R.BAR
    assert torch.equal(fvmd.motion_features_device(tracks), rows)
    if name.startswith("zero"):
        assert (rows == 0.0).all()


@pytest.mark.parametrize("n,m,d", K.GRAM, ids=lambda v: str(v))
def test_gram_block_edges(gpu_device, n, m, d):
    a, b = K.gram_rows(n, m, d)
    gram, scalars = fvmd.gram_device(_dev(a, gpu_device), _dev(b, gpu_device))
    assert _launch() == "fvmd_gram_kernel"
    want_gram, want_scalars = R.gram_parts(a, b)
    assert _report(f"gram {n} x {m} x {d}", gram.cpu().numpy(), want_gram) <= R.BAR
    assert _report(f"scalars {n} x {m} x {d}", scalars.cpu().numpy(), want_scalars) <= R.BAR
    again = fvmd.gram_device(_dev(a, gpu_device), _dev(b, gpu_device))
    assert torch.equal(again[0], gram) and torch.equal(again[1], scalars)


def test_tracker_on_a_clip_of_exactly_one_segment(gpu_device):
    """seq_len = FVMD_MIN_SEQ frames: one segment, whose last step reads the clip's last frame."""
    kind, h, w, s = K.TRACKER
    want = K.tracker_expected()
    assert R.margins_clear(want["margins"]), "the clip must keep lambda_min / 225 a factor 10 from the threshold"
    luma = _dev(want["clip"], gpu_device)
    assert luma.shape == (s, h, w)
    tracks = fvmd.track_keypoints_device(luma, s)
    assert _launch() == "fvmd_track_kernel" and tracks.shape == (1, s, 400, 2)
    assert _report("tracks of one segment", tracks.cpu().numpy(), want["tracks"]) <= R.BAR
    rows = fvmd.motion_features_device(tracks)
    assert _report("rows of one segment", rows.cpu().numpy(), want["rows"]) <= R.BAR
    assert torch.equal(fvmd.track_keypoints_device(luma, s), tracks)


def test_tracker_on_a_clip_one_frame_short(gpu_device):
    """seq_len - 1 frames: no segment, an empty result and no launch."""
    kind, h, w, s = K.TRACKER
    luma = _dev(K.tracker_expected()["clip"][:s - 1], gpu_device)
    a, b = K.gram_rows(2, 2, 1)
    fvmd.gram_device(_dev(a, gpu_device), _dev(b, gpu_device))
    assert _launch() == "fvmd_gram_kernel"
    tracks = fvmd.track_keypoints_device(luma, s)
    assert tracks.shape == (0, s, 400, 2) and tracks.dtype == torch.float64
    rows = fvmd.motion_features_device(tracks)
    assert rows.shape == (0, fvmd.feature_length(s))
    assert _launch() == "fvmd_gram_kernel", "neither the pyramid, the tracker nor the histograms were launched"
