"""VMAF, host side (no GPU): the numpy statement of the contract (tests/_vmaf_ref.py) and what it must satisfy; the
fixture's branch counts; the model loader, the SVR and the statistics block; stride sampling and Y-plane offsets; the C
entry points' export and validation; the kernels' names."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import _vmaf_ref as R
import elvis_amd
from elvis_amd import _build, _lib, handoff, vmaf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "elvis_amd", "csrc", "vmaf.hip")
LIBVMAF_NAMES = {"adm2": "VMAF_feature_adm2_score", "motion2": "VMAF_feature_motion2_score", "vif_scale0": "VMAF_feature_vif_scale0_score",
                 "vif_scale1": "VMAF_feature_vif_scale1_score", "vif_scale2": "VMAF_feature_vif_scale2_score",
                 "vif_scale3": "VMAF_feature_vif_scale3_score"}


# ----------------------------------------------------------------------------- the statement
def test_tables_are_the_contract():
    t = vmaf.vmaf_tables()
    assert t.dtype == np.float64 and t.shape == (56,) and np.array_equal(t, R.tables())
    for at, n in ((0, 17), (17, 9), (26, 5), (31, 3), (34, 5)):
        assert abs(t[at:at + n].sum() - 1.0) < 1e-15 and np.array_equal(t[at:at + n], t[at:at + n][::-1]) and t[at + n // 2] == t[at:at + n].max()
    lo, hi = t[39:43], t[43:47]
    assert abs(lo.sum() - math.sqrt(2.0)) < 1e-15 and abs(hi.sum()) < 1e-15 and abs((lo * lo).sum() - 1.0) < 1e-15
    assert t[47] == math.cos(math.pi / 180.0) ** 2 and (t[48:] > 0).all()


def test_identical_planes():
    """Flat identical planes give vif = 1 and adm2 = 1 within 1e-12 and motion 0.  On textured identical planes adm2 is 1
    within 1e-12 as well; vif falls short of 1 by the contract's own terms - a pixel with eps <= s1 < nsq contributes
    1 - 4 s2 / 65025 >= 1 - 4 nsq / 65025 against 1, and a log term g = s1 / (s1 + eps) < 1 - so it lies in
    [1 - 4 nsq / 65025, 1 + 1e-12]."""
    for level in (0, 77, 255):
        flat = np.full((2, 64, 70), level, np.uint8)
        f = R.features(flat, flat)
        assert np.abs(f[:, 0] - 1.0).max() <= 1e-12 and np.abs(f[:, 2:] - 1.0).max() <= 1e-12 and (f[:, 1] == 0.0).all()
    ref, _ = R.fixture(66, 70)
    f = R.features(ref, ref)
    print(f"identical textured planes: adm2 - 1 = {np.abs(f[:, 0] - 1).max():.3g}, 1 - vif = {(1 - f[:, 2:]).max():.3g}")
    assert np.abs(f[:, 0] - 1.0).max() <= 1e-12
    assert (f[:, 2:] <= 1.0 + 1e-12).all() and (f[:, 2:] >= 1.0 - 4.0 * R.NSQ / 65025.0).all()
    m, m2 = R.motion(ref)
    assert m[0] == 0.0 and (m[1:] > 0).all() and m2[0] == 0.0 and m2[1] == min(m[1], m[2]) and m2[2] == m[2]


def test_a_stronger_blur_scores_lower_on_every_feature():
    ref, _ = R.fixture(71, 93)
    rng = np.random.default_rng(3)
    once = R.blur_u8(ref, 0.0, rng)
    twice = R.blur_u8(R.blur_u8(once, 0.0, rng), 0.0, rng)
    a, b = R.features(ref, once), R.features(ref, twice)
    print("one blur", a[1], "three blurs", b[1])
    assert (b[:, 0] < a[:, 0]).all() and (b[:, 2:] < a[:, 2:]).all()
    assert np.array_equal(a[:, 1], b[:, 1])                                # motion reads the reference alone


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fixture_reaches_every_branch(shape):
    """The three VIF pixel classes (s1 < eps; eps <= s1 < nsq; s1 >= nsq) at every scale, and both values of the ADM
    flag at every scale.  The corrections s2 < eps and g < 0 are not in this fixture's reach (its distorted plane carries
    noise everywhere); `branch_pair` is there for them."""
    ref, dis = R.fixture(*shape)
    counts = R.new_counts()
    got = R.features(ref, dis, counts=counts)
    print(shape, counts)
    assert np.array_equal(got, R.expected(*shape))
    for key in ("s1_below_eps", "low_term", "log_term", "adm_flag_set", "adm_flag_clear"):
        assert all(c > 0 for c in counts[key]), (key, counts[key])
    assert (got[:, 2] < 0.6).all() and (got[:, 0] < 0.9).all() and (got[1:, 1] > 1.0).all()


def test_branch_pair_reaches_the_corrections():
    ref, dis = R.branch_pair()
    counts = R.new_counts()
    R.vif(ref[:1], dis[:1], counts)
    assert all(c > 0 for c in counts["s2_below_eps"])
    counts = R.new_counts()
    R.vif(ref[1:], dis[1:], counts)
    assert all(c > 0 for c in counts["gain_negative"])


def test_chunked_motion_is_the_whole_clips():
    ref, dis = R.fixture(64, 64)
    whole = R.features(ref, dis)
    parts = [R.features(ref[i:i + 1], dis[i:i + 1], prev=ref[i - 1] if i else None, nxt=ref[i + 1] if i < 2 else None) for i in range(3)]
    assert np.array_equal(np.concatenate(parts), whole)


def test_small_planes_are_refused():
    small = np.zeros((1, 63, 64), np.uint8)
    with pytest.raises(ValueError, match="smaller than 64"):
        R.features(small, small)
    with pytest.raises(ValueError, match="smaller than 64"):
        vmaf.calculate_vmaf_frames([np.zeros((64, 63, 3), np.uint8)], [np.zeros((64, 63, 3), np.uint8)])
    with pytest.raises(ValueError, match="smaller than 64"):
        vmaf.calculate_vmaf("a.yuv", "b.yuv", 64, 62, 30.0)
    with pytest.raises(ValueError, match="CUDA"):
        vmaf.vmaf_features_device(torch.zeros((1, 64, 64), dtype=torch.uint8), torch.zeros((1, 64, 64), dtype=torch.uint8))
    with pytest.raises(ValueError, match="CUDA"):
        vmaf.luma_device(torch.zeros((1, 64, 64, 3), dtype=torch.uint8))
    assert vmaf.calculate_vmaf_frames([], []) == []


# ----------------------------------------------------------------------------- the model
def _model_json(svr, names=None, **over):
    order = list(range(6)) if names is None else names
    text = ["svm_type nu_svr", "kernel_type rbf", f"gamma {svr.gamma!r}", "nr_class 2", f"total_sv {len(svr.coef)}", f"rho {svr.rho!r}", "SV"]
    for c, v in zip(svr.coef, svr.sv):
        text.append(" ".join([repr(float(c))] + [f"{k + 1}:{float(v[slot])!r}" for k, slot in enumerate(order)]))
    md = {"model_type": "LIBSVMNUSVR", "norm_type": "linear_rescale",
          "feature_names": [LIBVMAF_NAMES[vmaf.FEATURE_KEYS[slot]] for slot in order],
          "slopes": [float(svr.slopes[0])] + [float(svr.slopes[1 + slot]) for slot in order],
          "intercepts": [float(svr.intercepts[0])] + [float(svr.intercepts[1 + slot]) for slot in order],
          "score_clip": list(svr.score_clip),
          "score_transform": {"p0": svr.transform[0], "p1": svr.transform[1], "p2": svr.transform[2], "out_gte_in": "true"},
          "model": "\n".join(text) + "\n"}
    md.update(over)
    return {"model_dict": {k: v for k, v in md.items() if v is not ...}}


def _write(tmp_path, doc, name="model.json"):
    path = tmp_path / name
    path.write_text(json.dumps(doc))
    return str(path)


def test_model_round_trips_in_any_feature_order(tmp_path):
    model = vmaf.make_vmaf_model(0)
    assert model.sv.shape == (32, 6) and model.enable_transform is False and model.score_clip == (0.0, 100.0)
    again = vmaf.make_vmaf_model(0)
    assert np.array_equal(model.packed(), again.packed()) and not np.array_equal(model.packed(), vmaf.make_vmaf_model(1).packed())
    for order in (None, [2, 3, 4, 5, 0, 1], [5, 1, 0, 3, 2, 4]):
        got = vmaf.load_vmaf_model(_write(tmp_path, _model_json(model, order)))
        for name in ("slopes", "intercepts", "sv", "coef"):
            assert np.array_equal(getattr(got, name), getattr(model, name)), name
        assert (got.rho, got.gamma, got.score_clip, got.transform, got.enable_transform) == (model.rho, model.gamma, model.score_clip,
                                                                                         model.transform, False)
        assert np.array_equal(got.packed(), model.packed()) and got.flags == model.flags == 0b110
    assert "UNVERIFIED" in vmaf.load_vmaf_model.__doc__


@pytest.mark.parametrize("over, word", [
    (dict(model_type="RESIDUEBOOTSTRAP_LIBSVMNUSVR"), "model_type"),
    (dict(norm_type="clip_0to1"), "norm_type"),
    (dict(model="svm_type nu_svr\nkernel_type linear\ngamma 0.5\ntotal_sv 1\nrho 0\nSV\n1 1:0\n"), "kernel_type"),
    (dict(feature_names=["VMAF_feature_adm2_score", "VMAF_feature_motion_score"] + ["x"] * 4), "feature_names"),
    (dict(slopes=[1.0] * 6), "count mismatch"),
    (dict(model="svm_type nu_svr\nkernel_type rbf\ngamma 0.5\ntotal_sv 3\nrho 0\nSV\n1 1:0\n"), "total_sv"),
    (dict(model="svm_type nu_svr\nkernel_type rbf\ntotal_sv 1\nrho 0\nSV\n1 1:0\n"), "gamma"),
    (dict(slopes=...), "slopes"),
    (dict(intercepts=...), "intercepts"),
    (dict(score_clip=...), "score_clip"),
    (dict(model=...), "model_dict.model "),
    (dict(feature_names=...), "feature_names"),
])
def test_model_value_errors_name_the_field(tmp_path, over, word):
    with pytest.raises(ValueError, match=word):
        vmaf.load_vmaf_model(_write(tmp_path, _model_json(vmaf.make_vmaf_model(0), **over)))


def test_model_without_model_dict(tmp_path):
    with pytest.raises(ValueError, match="model_dict"):
        vmaf.load_vmaf_model(_write(tmp_path, {"model": "x"}))
    with pytest.raises(ValueError, match="7 values"):
        vmaf.VmafModel(np.ones(6), np.zeros(7), np.zeros((1, 6)), np.ones(1), 0.0, 1.0)


def _svr_by_hand(f, m):
    x = [m.slopes[i + 1] * f[i] + m.intercepts[i + 1] for i in range(6)]
    p = 0.0
    for j in range(len(m.coef)):
        p += m.coef[j] * math.exp(-m.gamma * sum((m.sv[j][i] - x[i]) ** 2 for i in range(6)))
    return ((p - m.rho) - m.intercepts[0]) / m.slopes[0]


def test_svr_transform_and_clip():
    m = vmaf.make_vmaf_model(0)
    feats = np.concatenate([R.expected(64, 64), [[1.0, 0.0, 1.0, 1.0, 1.0, 1.0], [0.2, 30.0, 0.05, 0.3, 0.5, 0.6]]])
    raw = np.asarray([_svr_by_hand(f, m) for f in feats])
    print("scores", raw)
    assert np.abs(R.score(feats, m) - np.clip(raw, 0.0, 100.0)).max() < 1e-11 and raw.min() > 0.0 and raw.max() < 100.0 and np.ptp(raw) > 1.0
    m.enable_transform = True
    p0, p1, p2, _ = m.transform
    bent = np.maximum(p0 + p1 * raw + p2 * raw * raw, raw)
    assert np.abs(R.score(feats, m) - bent).max() < 1e-11 and (bent != raw).any() and m.flags == 0b111
    m.transform = (p0, p1, p2, False)
    assert np.abs(R.score(feats, m) - (p0 + p1 * raw + p2 * raw * raw)).max() < 1e-11 and m.flags == 0b101
    m.enable_transform, m.score_clip = False, (46.0, 48.0)
    assert np.abs(R.score(feats, m) - np.clip(raw, 46.0, 48.0)).max() < 1e-11 and (raw < 46.0).any() and (raw > 48.0).any()
    m.score_clip = None
    assert np.abs(R.score(feats, m) - raw).max() < 1e-11 and m.flags == 0


# ----------------------------------------------------------------------------- statistics, sampling, offsets
def test_vmaf_stats_is_the_references_block():
    for scores in ([93.5, 12.25, 0.0, 77.0], [0.0005, 50.0], [41.0]):
        got = vmaf.vmaf_stats(scores)
        arr = np.array(scores)
        want = {"mean": float(np.mean(arr)), "min": float(np.min(arr)), "max": float(np.max(arr)), "std": float(np.std(arr)),
                "harmonic_mean": float(len(scores) / np.sum([1.0 / max(s, 0.001) for s in scores]))}
        assert got == want and list(got) == ["mean", "min", "max", "std", "harmonic_mean"]
    assert vmaf.vmaf_stats([0.0, 100.0])["harmonic_mean"] == 2 / (1000.0 + 0.01)
    with pytest.raises(ValueError, match="no scores"):
        vmaf.vmaf_stats([])


def test_stride_sampling():
    assert vmaf.sampled_frames(5, 1) == [0, 1, 2, 3, 4] and vmaf.sampled_frames(5, 2) == [0, 2, 4] and vmaf.sampled_frames(6, 3) == [0, 3]
    assert vmaf.sampled_frames(2, 5) == [0] and vmaf.sampled_frames(0, 2) == []
    with pytest.raises(ValueError, match="frame_stride"):
        vmaf.sampled_frames(4, 0)


def test_luma_plane_offsets(tmp_path):
    w, h, n = 66, 64, 3
    frame = w * h * 3 // 2
    rng = np.random.default_rng(0)
    payload = rng.integers(0, 256, (n, frame), dtype=np.uint8)
    yuv, y4m, odd = str(tmp_path / "clip.yuv"), str(tmp_path / "clip.y4m"), str(tmp_path / "clip.mp4")
    open(yuv, "wb").write(payload.tobytes())
    head = handoff.y4m_header(w, h, 30.0)
    with open(y4m, "wb") as f:
        f.write(head)
        for i in range(n):
            f.write(b"FRAME\n" if i != 1 else b"FRAME Xtag\n")
            f.write(payload[i].tobytes())
    open(odd, "wb").write(b"x")
    assert vmaf.luma_plane_offsets(yuv, w, h) == [0, frame, 2 * frame]
    want = [len(head) + 6, len(head) + 6 + frame + 11, len(head) + 6 + frame + 11 + frame + 6]
    assert vmaf.luma_plane_offsets(y4m, w, h) == want
    data = open(y4m, "rb").read()
    for i, at in enumerate(want):
        assert data[at:at + w * h] == payload[i, :w * h].tobytes()
    with pytest.raises(ValueError, match="header says"):
        vmaf.luma_plane_offsets(y4m, h, w)
    with pytest.raises(ValueError, match="whole number"):
        vmaf.luma_plane_offsets(yuv, w, h + 2)
    with pytest.raises(ValueError, match="no converter"):
        vmaf.luma_plane_offsets(odd, w, h)
    with pytest.raises(ValueError, match="no converter"):
        vmaf.calculate_vmaf(odd, yuv, w, h, 30.0)
    short = str(tmp_path / "short.yuv")
    open(short, "wb").write(payload[:2].tobytes())
    with pytest.raises(ValueError, match="holds 3 frames"):
        vmaf.calculate_vmaf(yuv, short, w, h, 30.0)
    with pytest.raises(ValueError, match="frame_stride"):
        vmaf.calculate_vmaf(yuv, yuv, w, h, 30.0, frame_stride=0)


def test_names_are_exported():
    for name in ("luma_device", "vmaf_features_device", "vmaf_device", "get_vmaf_model", "load_vmaf_model", "make_vmaf_model",
                 "calculate_vmaf", "calculate_vmaf_frames", "vmaf_stats"):
        assert callable(getattr(elvis_amd, name)), name
    assert "elvis.py:3197" in vmaf.calculate_vmaf.__doc__ and "presley.py:262" in vmaf.calculate_vmaf_frames.__doc__
    assert "BUILD-DEFINED" in vmaf.__doc__ and "NOT claim parity" in vmaf.__doc__
    import inspect
    from elvis_amd import metrics
    assert inspect.signature(metrics.evaluate_fg_bg_metrics).parameters["vmaf_model"].default is None
    assert "NOT reproduced" in metrics.evaluate_fg_bg_metrics.__doc__


# ----------------------------------------------------------------------------- the built library
def test_entry_points_refuse_bad_arguments_without_a_gpu(built_lib):
    h = _lib.lib()
    assert "vmaf.hip" in _build.SOURCES

    def bad(rc, word):
        assert rc == -1 and word in h.elvis_last_error(), (rc, h.elvis_last_error())
    p = 256                                                                       # never dereferenced: every call is refused
    for hh, ww in ((63, 64), (64, 63), (0, 64), (8, 8)):
        bad(h.elvis_vmaf_features_f64(p, p, None, None, p, p, p, 1, hh, ww, None), b"smaller than 64")
        assert h.elvis_vmaf_workspace_bytes(1, hh, ww) == 0
    bad(h.elvis_vmaf_features_f64(p, p, None, None, p, p, p, -1, 64, 64, None), b"frame count")
    bad(h.elvis_vmaf_features_f64(p, p, None, None, p, p, p, 65535, 64, 64, None), b"frame count")
    for k in (0, 1, 4, 5, 6):                                                     # ref, dis, tables, workspace, out
        args = [p, p, None, None, p, p, p]
        args[k] = None
        bad(h.elvis_vmaf_features_f64(*args, 1, 64, 64, None), b"null")
    assert h.elvis_vmaf_features_f64(None, None, None, None, None, None, None, 0, 64, 64, None) == 0       # n == 0: no-op
    for k in (0, 2):
        args = [p, None, p]
        args[k] = None
        bad(h.elvis_vmaf_luma_u8(*args, 1, 64, 64, 1, 0, 0, 64, 0, 64, None), b"null")
    bad(h.elvis_vmaf_luma_u8(p, None, p, 1, 64, 64, 2, 0, 0, 64, 0, 64, None), b"order")
    bad(h.elvis_vmaf_luma_u8(p, None, p, 1, 64, 64, 0, 0, 0, 65, 0, 64, None), b"rectangle")
    bad(h.elvis_vmaf_luma_u8(p, None, p, 1, 64, 64, 0, 0, 5, 5, 0, 64, None), b"rectangle")
    bad(h.elvis_vmaf_luma_u8(p, None, p, 1, 0, 64, 0, 0, 0, 0, 0, 64, None), b"bad shape")
    for k in range(3):
        args = [p, p, p]
        args[k] = None
        bad(h.elvis_vmaf_predict_f64(*args, 1, 32, 0, None), b"null")
    bad(h.elvis_vmaf_predict_f64(p, p, p, 1, 0, 0, None), b"bad shape")
    bad(h.elvis_vmaf_predict_f64(p, p, p, 1, 32, 8, None), b"flags")
    assert h.elvis_vmaf_predict_f64(None, None, None, 0, 32, 0, None) == 0


def test_workspace_plan(built_lib):
    """The pyramids of at most four frames, and per frame one (num, den) pair per 16 x 32 VIF tile, six partials per
    16 x 16 ADM tile and one motion partial per 16 x 32 tile (one frame more: `following`)."""
    h = _lib.lib()

    def expect(n, hh, ww):
        cd = lambda a, b: -(-a // b)
        resident = min(n, 4)
        doubles = per_frame = 0
        vh, vw = hh, ww
        for s in range(4):
            if s:
                vh, vw = vh // 2, vw // 2
                doubles += resident * 2 * vh * vw
            per_frame += 2 * cd(vh, 16) * cd(vw, 32)
        ah, aw = hh, ww
        for s in range(4):
            ah, aw = (ah + 1) // 2, (aw + 1) // 2
            doubles += resident * 8 * ah * aw
            per_frame += 6 * cd(ah, 16) * cd(aw, 16)
        return 8 * (doubles + (n + 1) * cd(hh, 16) * cd(ww, 32) + n * per_frame)
    for n, hh, ww in ((1, 64, 64), (3, 71, 93), (4, 270, 480), (9, 270, 480), (30, 1080, 1920)):
        assert h.elvis_vmaf_workspace_bytes(n, hh, ww) == expect(n, hh, ww), (n, hh, ww)
    assert h.elvis_vmaf_workspace_bytes(0, 64, 64) == 0 and h.elvis_vmaf_workspace_bytes(30, 1080, 1920) < 256 << 20


def test_kernels_of_the_source(built_lib):
    from _glueref import kernel_stems
    from _qualitycases import kernel_names
    stems = kernel_stems(SOURCE)
    assert stems == {"vmaf_luma_kernel", "vmaf_vif_down_kernel", "vmaf_vif_stat_kernel", "vmaf_dwt_kernel", "vmaf_adm_pool_kernel",
                     "vmaf_motion_kernel", "vmaf_finish_kernel", "vmaf_predict_kernel"}
    built = kernel_names(built_lib, SOURCE)
    assert {"vmaf_vif_stat_kernel<17>", "vmaf_vif_stat_kernel<9>", "vmaf_vif_stat_kernel<5>", "vmaf_vif_stat_kernel<3>",
            "vmaf_vif_down_kernel<9>", "vmaf_vif_down_kernel<5>", "vmaf_vif_down_kernel<3>"} <= built
    assert {b.split("<")[0] for b in built} == stems
    text = open(SOURCE).read()
    assert not re.search(r"\batomic\w*\s*\(", text) and not re.search(r"\bfma[f]?\s*\(", text)     # fixed orders, the stated products
    assert '#include "i420.h"' in text and "269484" not in text                   # the hand-off's luma, not a second copy
    assert "-ffp-contract=off" in _build.FLAGS
