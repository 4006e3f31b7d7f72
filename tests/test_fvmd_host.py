"""FVMD, host side (no GPU): the numpy statement of the contract (tests/_fvmd_ref.py) and what it must satisfy - it is a
tracker, the Gram / nuclear-norm identity, the distance's properties, the soft vote; the control flow of
`calculate_fvmd` against the reference's own code (tests/golden/fvmd.npz); the module's surface."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _fvmd_ref as R
import elvis_amd
from elvis_amd import _build, _lib, fvmd, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("elvis_fvmd_pyramid_bytes", "elvis_fvmd_pyramid_f64", "elvis_fvmd_track_f64", "elvis_fvmd_features_f64",
                "elvis_fvmd_gram_workspace_bytes", "elvis_fvmd_gram_f64", "elvis_fvmd_singular_values_f64", "elvis_fvmd_finish_f64")
PAN_BAR = 2 * 0.0466           # twice the worst interior error measured (see test_the_statement_is_a_tracker)
IDENTITY_BAR = 10 * 2.44e-14   # ten times the worst relative disagreement measured (see test_gram_form_is_the_textbook_distance)


# ----------------------------------------------------------------------------- the statement
def test_the_statement_is_a_tracker():
    """A smooth textured clip (a sum of low-frequency sinusoids, rounded to 8 bits, no noise) panned by (vy, vx) =
    (0.6, -0.85) pixels a frame: the velocities of the interior points (rows and columns 5 .. 14 of the 20 x 20 grid, whose
    level-0 windows stay inside the frame) recover the pan.  Measured here: worst |v - pan| = 0.0342 pixels (x) and 0.0466
    (y) over 9 steps x 100 points; the bar is twice the larger, there only to catch a sign or an axis mix-up."""
    field = R.texture(64, 64, 7)
    clean = np.stack([np.clip(np.rint(R.shifted(field, 64, 64, 0.6 * t, -0.85 * t)), 0, 255).astype(np.uint8) for t in range(10)])
    tr = R.track(clean, 10, 1)
    assert tr.shape == (1, 10, 400, 2)
    v = (tr[0, 1:] - tr[0, :-1]).reshape(9, 20, 20, 2)[:, 5:15, 5:15]
    ex, ey = np.abs(v[..., 0] + 0.85).max(), np.abs(v[..., 1] - 0.6).max()
    print(f"pan recovery: worst |vx + 0.85| = {ex:.4g}, worst |vy - 0.6| = {ey:.4g} (bar {PAN_BAR:g})")
    assert ex <= PAN_BAR and ey <= PAN_BAR


def test_static_and_black_clips_do_not_move():
    static = np.ascontiguousarray(np.broadcast_to(R.clip("pan", 11, 64, 64)[0], (10, 64, 64)))
    tr = R.track(static, 10)
    assert (tr == tr[:, :1]).all() and (R.features(tr) == 0.0).all()
    black = np.full((10, 64, 64), 16, np.uint8)
    margins = []
    tr = R.track(black, 10, margins=margins)
    assert (tr == tr[:, :1]).all() and (np.concatenate(margins) == 0.0).all()


def test_pyramid_sizes_and_flat_planes():
    lv0, lv1, lv2 = R.pyramid(np.full((2, 67, 81), 200, np.uint8))
    assert lv1.shape == (2, 34, 41) and lv2.shape == (2, 17, 21) and (lv1 == 200.0).all() and (lv2 == 200.0).all()
    with pytest.raises(ValueError, match="smaller than 64"):
        R.track(np.zeros((10, 63, 64), np.uint8), 10)


def _rows(rng, n, d, scale=1.0, shift=0.0):
    return rng.normal(0.0, 1.0, (n, d)) @ (np.eye(d) + 0.3 * rng.normal(0.0, 1.0, (d, d))) * scale + shift


def test_gram_form_is_the_textbook_distance():
    """Full-rank cases, n, m > d: the Gram / nuclear-norm form against np.cov + scipy.linalg.sqrtm.  The agreement is
    sqrtm's: measured here, worst |gram form - textbook| / (tr S1 + tr S2 + |dmu|^2) = 2.44e-14 over these 24 cases; the
    bar is ten times the worst seen."""
    worst = 0.0
    for seed in (11, 12, 13, 14):
        rng = np.random.default_rng(seed)
        for n, m, d in ((9, 9, 3), (12, 20, 5), (40, 17, 8), (30, 30, 12), (64, 50, 6), (200, 150, 40)):
            a, b = _rows(rng, n, d, 2.0, 1.0), _rows(rng, m, d, 1.5, -0.5)
            got, want, scale = R.frechet(a, b), R.frechet_textbook(a, b), R.fd_scale(a, b)
            worst = max(worst, abs(got - want) / scale)
            assert want > 0
    print(f"identity: worst |gram form - textbook| / scale = {worst:.3g} (bar {IDENTITY_BAR:g})")
    assert worst <= IDENTITY_BAR


def test_distance_properties():
    rng = np.random.default_rng(12)
    for n, m, d in ((5, 7, 40), (3, 3, 128), (20, 9, 6)):
        a, b = _rows(rng, n, d), _rows(rng, m, d, 1.3, 0.2)
        assert abs(R.frechet(a, a)) <= 1e-9 * R.fd_scale(a, a)
        ab, ba = R.frechet(a, b), R.frechet(b, a)
        assert abs(ab - ba) <= 1e-12 * R.fd_scale(a, b) and ab > 0
        assert abs(R.frechet(a[rng.permutation(n)], b[rng.permutation(m)]) - ab) <= 1e-12 * R.fd_scale(a, b)
    with pytest.raises(R.NoTrajectories):
        R.frechet(_rows(rng, 1, 4), _rows(rng, 3, 4))


def test_soft_vote():
    rng = np.random.default_rng(13)
    vx = rng.uniform(0.5, 3.0, 400)
    up, down = R.field_hist(vx, np.full(400, 1e-17)), R.field_hist(vx, np.full(400, -1e-17))
    assert np.abs(up - down).max() <= 1e-12 and np.abs(up.reshape(16, 8)[:, 0].sum() - vx.sum()) <= 1e-9       # a pure pan votes for bin 0
    assert np.abs(up.reshape(16, 8)[:, 1:]).max() <= 1e-12 and np.abs(down.reshape(16, 8)[:, 1:]).max() <= 1e-12
    assert (R.field_hist(np.zeros(400), np.zeros(400)) == 0.0).all()                                   # magnitude 0 adds nothing
    some = np.zeros(400)
    some[R.cell_point(5, 3)] = 2.0
    one = R.field_hist(some, np.zeros(400)).reshape(16, 8)
    assert one[5, 0] == 2.0 and one.sum() == 2.0                                                        # the cell of the point, no other
    ang = -np.pi / 8                                                                                   # half way between bins 7 and 0
    wrap = R.field_hist(np.full(400, np.cos(ang)), np.full(400, np.sin(ang))).reshape(16, 8)
    assert np.abs(wrap[:, 7] - 12.5).max() <= 1e-9 and np.abs(wrap[:, 0] - 12.5).max() <= 1e-9 and np.abs(wrap[:, 1:7]).max() == 0.0
    mid = R.field_hist(np.zeros(400), np.full(400, -1.0)).reshape(16, 8)                               # straight down: bin 6
    assert (mid[:, 6] == 25.0).all() and mid.sum() == 400.0


def test_feature_rows_layout():
    rng = np.random.default_rng(14)
    tr = rng.uniform(0, 63, (2, 10, 400, 2))
    rows = R.features(tr)
    assert rows.shape == (2, fvmd.feature_length(10)) == (2, 17 * 128)
    v = tr[:, 1:] - tr[:, :-1]
    assert np.array_equal(rows[1, 3 * 128:4 * 128], R.field_hist(v[1, 3, :, 0], v[1, 3, :, 1]))
    a = v[:, 1:] - v[:, :-1]
    assert np.array_equal(rows[0, (9 + 2) * 128:(9 + 3) * 128], R.field_hist(a[0, 2, :, 0], a[0, 2, :, 1]))


# ----------------------------------------------------------------------------- the control flow, against the reference's code
def _golden_cases(golden_dir):
    z = np.load(os.path.join(golden_dir, "fvmd.npz"))
    for i in range(int(z["cases"])):
        frames, stride, max_frames, delta, window = z[f"case{i}_args"]
        calls = [[int(v) for v in row if v >= 0] for row in z[f"case{i}_calls"]]
        yield (int(frames), int(stride), int(max_frames) or None, float(delta), int(window), str(z[f"case{i}_script"]), calls,
               z[f"case{i}_result"], str(z[f"case{i}_error"]))


def _scripted(kind, calls):
    def score(indices):
        calls.append([int(i) for i in indices])
        try:
            return R.scripted_score(kind, indices)
        except R.NoTrajectories as exc:
            raise fvmd.FvmdNoTrajectories(str(exc))
    return score


def test_control_flow_is_the_references(golden_dir):
    """Every case of tools/make_fvmd_golden.py: the same index lists are scored in the same order and the same pair (or
    the same exception class) comes back, from `fvmd_control_flow` and from `calculate_fvmd` with its scorer replaced."""
    seen = set()
    for frames, stride, max_frames, delta, window, script, want_calls, want, error in _golden_cases(golden_dir):
        calls = []
        try:
            got, got_error = fvmd.fvmd_control_flow(frames, _scripted(script, calls), stride, max_frames, delta, window, lambda *a, **k: None), ""
        except (ValueError, RuntimeError) as exc:
            got, got_error = (float("nan"), float("nan")), type(exc).__name__
        assert got_error == error, (frames, stride, script, got_error, error)
        assert calls == want_calls, (frames, stride, script)
        assert np.array_equal(np.asarray(got, np.float64), want, equal_nan=True), (frames, stride, script, got, want)
        seen.add(error or ("std" if want[1] > 0 else "plain"))
    assert seen == {"ValueError", "RuntimeError", "std", "plain"}


def test_calculate_fvmd_runs_that_control_flow(golden_dir, monkeypatch):
    for frames, stride, max_frames, delta, window, script, want_calls, want, error in _golden_cases(golden_dir):
        calls = []
        monkeypatch.setattr(fvmd, "_make_scorer_host", lambda *a, **k: _scripted(script, calls))
        clip = [np.full((1, 1), i % 256, np.uint8) for i in range(frames)]
        if error:
            with pytest.raises(ValueError if error == "ValueError" else RuntimeError):
                fvmd.calculate_fvmd(clip, clip, None, stride, max_frames, delta, window, None, False)
        else:
            got = fvmd.calculate_fvmd(clip, clip, "ignored", stride, max_frames, delta, window, None, False)
            assert np.array_equal(np.asarray(got), want) and isinstance(got[0], float) and isinstance(got[1], float)
        assert calls == want_calls


def test_prepare_is_told_each_attempts_indices():
    told = []

    class Scorer:
        def prepare(self, indices):
            told.append(list(indices))

        def __call__(self, indices):
            if indices[1] - indices[0] > 1:
                raise fvmd.FvmdNoTrajectories("wide")
            return 1.0

    assert fvmd.fvmd_control_flow(40, Scorer(), stride=2, printer=lambda *a: None) == (1.0, 0.0)
    assert told == [list(range(0, 40, 2)), list(range(40))]


# ----------------------------------------------------------------------------- the surface
def test_docstrings_state_the_status():
    header = open(os.path.join(ROOT, "include", "elvis_amd.h")).read()
    source = open(os.path.join(ROOT, "elvis_amd", "csrc", "fvmd.hip")).read()
    for text in (fvmd.__doc__, header[header.index("FVMD (fvmd.hip"):header.index("PNG writer")], source[:source.index("#include")], R.__doc__):
        assert "BUILD-DEFINED" in text and "NOT claim parity" in text and re.search(r"elvis\.py:\d+-\d+", text)
    assert "elvis.py:3358-3597" in fvmd.__doc__ and "elvis.py:3358-3597" in fvmd.calculate_fvmd.__doc__
    for fn in (fvmd.track_keypoints_device, fvmd.motion_features_device, fvmd.frechet_distance_device, fvmd.fvmd_device):
        assert "BUILD-DEFINED" in fn.__doc__ and re.search(r"elvis\.py:\d+", fn.__doc__)
    assert "segment_step" in fvmd.FvmdConfig.__doc__ and "stride=1" in fvmd.FvmdConfig.__doc__
    assert elvis_amd.fvmd is fvmd


def test_signature_is_the_references():
    params = list(inspect.signature(fvmd.calculate_fvmd).parameters.values())
    names = [p.name for p in params if p.kind is p.POSITIONAL_OR_KEYWORD]
    assert names == ["reference_frames", "decoded_frames", "log_root", "stride", "max_frames", "early_stop_delta", "early_stop_window",
                     "device", "verbose"]
    assert [p.default for p in params[2:9]] == [None, 1, None, 0.002, 50, None, True]
    assert inspect.signature(metrics.evaluate_fg_bg_metrics).parameters["fvmd"].default is None
    assert issubclass(fvmd.FvmdNoTrajectories, RuntimeError)
    cfg = fvmd.FvmdConfig()
    assert (cfg.segment_step, cfg.grid, cfg.pyramid_levels, cfg.window_radius, cfg.iterations, cfg.min_eigenvalue, cfg.cells, cfg.bins) == \
        (1, 20, 3, 7, 8, 1e-3, 4, 8)
    with pytest.raises(Exception):
        cfg.segment_step = 2                                                # frozen
    with pytest.raises(ValueError, match="segment_step"):
        fvmd.FvmdConfig(segment_step=0)
    with pytest.raises(ValueError, match="constant of the contract"):
        fvmd.FvmdConfig(grid=10)
    assert [fvmd.clip_seq_len(f) for f in (2, 10, 13, 16, 300)] == [10, 10, 13, 16, 16] == [R.seq_len_of(f) for f in (2, 10, 13, 16, 300)]
    assert [fvmd.segment_count(f, 16, s) for f, s in ((15, 1), (16, 1), (24, 1), (24, 2), (25, 2), (300, 1))] == [0, 1, 9, 5, 5, 285]


def test_value_errors_without_a_gpu():
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)                        # noqa: E731
    with pytest.raises(ValueError, match="smaller than 64"):
        fvmd.track_keypoints_device(u8(10, 63, 64), 10)
    with pytest.raises(ValueError, match="smaller than 64"):
        fvmd.fvmd_device(u8(20, 64, 60), u8(20, 64, 60))
    with pytest.raises(ValueError, match="smaller than 64"):
        fvmd.calculate_fvmd([np.zeros((40, 64, 3), np.uint8)] * 20, [np.zeros((40, 64, 3), np.uint8)] * 20, verbose=False)
    with pytest.raises(ValueError, match="CUDA"):
        fvmd.track_keypoints_device(u8(10, 64, 64), 10)
    with pytest.raises(ValueError, match="at least 10"):
        fvmd.calculate_fvmd([np.zeros((64, 64), np.uint8)] * 9, [np.zeros((64, 64), np.uint8)] * 9, verbose=False)
    with pytest.raises(ValueError, match="at least one frame"):
        fvmd.calculate_fvmd([], [])
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64)                     # noqa: E731
    with pytest.raises(ValueError, match="CUDA"):
        fvmd.frechet_distance_device(f64(3, 8), f64(3, 8))
    with pytest.raises(ValueError, match=r"tracks must be \[B, S, 400, 2\]"):
        fvmd.motion_features_device(f64(1, 10, 399, 2).as_subclass(_FakeCuda))


class _FakeCuda(torch.Tensor):
    """A host tensor that says it is resident: the shape checks that come before the device is touched."""
    is_cuda = True


def test_mismatched_clips_and_the_row_cap_are_refused_before_the_device():
    fake = lambda t: t.as_subclass(_FakeCuda)                               # noqa: E731
    a, b = fake(torch.zeros((20, 64, 64), dtype=torch.uint8)), fake(torch.zeros((20, 64, 66), dtype=torch.uint8))
    with pytest.raises(ValueError, match="of one shape"):
        fvmd.fvmd_device(a, b)
    with pytest.raises(ValueError, match="of one shape"):
        fvmd.calculate_fvmd_device(a, b)
    over = fake(torch.zeros((fvmd.MAX_ROWS + 1, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="segment_step"):
        fvmd.frechet_distance_device(over, over)
    with pytest.raises(fvmd.FvmdNoTrajectories):
        fvmd.frechet_distance_device(over[:1], over[:3])
    long_clip = fake(torch.zeros((fvmd.MAX_ROWS + 16, 64, 64), dtype=torch.uint8))
    with pytest.raises(ValueError, match="segment_step"):
        fvmd.fvmd_device(long_clip, long_clip)
    with pytest.raises(fvmd.FvmdNoTrajectories):
        fvmd.fvmd_device(a[:16], a[:16])
    assert fvmd.MAX_ROWS >= 512


def test_entry_points_are_built_and_bound(built_lib):
    assert "fvmd.hip" in _build.SOURCES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "elvis_amd.h")).read(), flags=re.S)
    lib = _lib.lib()
    for name in ENTRY_POINTS:
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;{]*?)\)\s*;", header, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name]), name
        assert hasattr(lib, name)
    full = open(os.path.join(ROOT, "include", "elvis_amd.h")).read()
    for name in ENTRY_POINTS:
        assert "elvis.py:3476-3505" in full[:full.index(name + "(")].rsplit("/*", 1)[1], name


def test_arguments_are_validated_without_a_gpu(built_lib):
    lib = _lib.lib()
    assert lib.elvis_fvmd_pyramid_bytes(3, 64, 64) == 3 * (32 * 32 + 16 * 16) * 8
    assert lib.elvis_fvmd_pyramid_bytes(3, 67, 81) == 3 * (34 * 41 + 17 * 21) * 8
    assert lib.elvis_fvmd_pyramid_bytes(3, 63, 64) == 0 and lib.elvis_fvmd_pyramid_bytes(70000, 64, 64) == 0
    assert lib.elvis_fvmd_gram_workspace_bytes(3, 5, 100) == (200 + 8) * 8
    assert lib.elvis_fvmd_gram_workspace_bytes(1, 5, 100) == 0 and lib.elvis_fvmd_gram_workspace_bytes(3, 1025, 100) == 0
    one = 8                                                                   # any non-null address: nothing is dereferenced
    bad = (
        (lib.elvis_fvmd_pyramid_f64, (one, one, 4, 63, 64, 0), "at least 64 x 64"),
        (lib.elvis_fvmd_pyramid_f64, (0, one, 4, 64, 64, 0), "null pointer"),
        (lib.elvis_fvmd_track_f64, (one, one, one, 20, 64, 64, 9, 1, 0), "seq_len"),
        (lib.elvis_fvmd_track_f64, (one, one, one, 20, 64, 64, 17, 1, 0), "seq_len"),
        (lib.elvis_fvmd_track_f64, (one, one, one, 20, 64, 64, 10, 0, 0), "segment_step"),
        (lib.elvis_fvmd_track_f64, (one, one, one, 20, 60, 64, 10, 1, 0), "at least 64 x 64"),
        (lib.elvis_fvmd_track_f64, (one, one, 0, 20, 64, 64, 10, 1, 0), "null pointer"),
        (lib.elvis_fvmd_features_f64, (one, one, 2, 9, 0), "seq_len"),
        (lib.elvis_fvmd_features_f64, (one, 0, 2, 10, 0), "null pointer"),
        (lib.elvis_fvmd_features_f64, (one, one, -1, 10, 0), "segment count"),
        (lib.elvis_fvmd_gram_f64, (one, one, one, one, one, 1, 2, 8, 0), "bad shape"),
        (lib.elvis_fvmd_gram_f64, (one, one, one, one, one, 2, 1025, 8, 0), "bad shape"),
        (lib.elvis_fvmd_gram_f64, (one, one, 0, one, one, 2, 2, 8, 0), "null pointer"),
        (lib.elvis_fvmd_singular_values_f64, (one, one, 0, 4, 0), "bad shape"),
        (lib.elvis_fvmd_singular_values_f64, (one, one, 4, 1025, 0), "bad shape"),
        (lib.elvis_fvmd_singular_values_f64, (one, 0, 4, 4, 0), "null pointer"),
        (lib.elvis_fvmd_finish_f64, (one, one, one, 2, 1, 2, 0), "bad shape"),
        (lib.elvis_fvmd_finish_f64, (one, one, 0, 2, 2, 2, 0), "null pointer"),
    )
    for fn, args, what in bad:
        assert fn(*args) == -1, (fn.__name__, args)
        assert what in lib.elvis_last_error().decode(), (fn.__name__, lib.elvis_last_error())
    assert lib.elvis_fvmd_track_f64(0, 0, 0, 9, 64, 64, 10, 1, 0) == 0          # shorter than one segment: a no-op
    assert lib.elvis_fvmd_features_f64(0, 0, 0, 10, 0) == 0 and lib.elvis_fvmd_pyramid_f64(0, 0, 0, 64, 64, 0) == 0
