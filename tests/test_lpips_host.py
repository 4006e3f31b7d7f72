"""LPIPS (AlexNet), host side (no GPU): the torch statement of the contract (tests/_lpips_ref.py) against the reference's
own wrapper (tests/golden/lpips.npz, tools/make_lpips_golden.py), its mutants, the CPU float32 figure the device bar is
derived from, the state_dict loader, the Python argument errors, the C entry points' export and validation, and the
kernel ledger."""
import os
import re

import numpy as np
import pytest
import torch

import _lpips_ref as R
import elvis_amd
from elvis_amd import _build, _lib, lpips, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "elvis_amd", "csrc", "lpips.hip")
ENTRIES = {"elvis_lpips_stem_u8": 15, "elvis_lpips_conv5_f32": 10, "elvis_lpips_maxpool_f32": 9,
           "elvis_lpips_distance_workspace_bytes": 3, "elvis_lpips_distance_f64": 12}


# ----------------------------------------------------------------------------- the torch statement
def test_float32_restatement_reproduces_the_reference_wrapper(golden_dir):
    """The scores the reference's calculate_lpips_per_frame returned (BGR flip, / 127.5 - 1, pairing, None skipping)
    with the float32 restatement as its model: entries 0 and 1 of the equal-sized frames and the other-sized pair."""
    g = np.load(os.path.join(golden_dir, "lpips.npz"))
    sd = weights.make_lpips_weights(int(g["seed"]))
    pairs = [(g["frames_ref"][0], g["frames_dec"][0]), (g["frames_ref"][1], g["frames_dec"][1]), (g["other_ref"], g["other_dec"])]
    got = [float(R.score(a[None], b[None], sd, "bgr", dtype=torch.float32)[0]) for a, b in pairs]
    print("golden", list(g["scores"]), "restated", got)
    assert len(g["scores"]) == 3
    assert R.rel(got, g["scores"]) <= R.CPU_F32_WORST
    # the same frames handed over with their channels reversed: what order="rgb" computes on the originals
    rev = [float(R.score(a[None], b[None], sd, "rgb", dtype=torch.float32)[0]) for a, b in pairs[:2]]
    assert R.rel(rev, g["scores_channels_reversed"]) <= R.CPU_F32_WORST
    assert R.rel(rev, g["scores"][:2]) > 100 * R.DEVICE_BAR


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_every_mutant_moves_its_case_by_a_hundred_bars(mutant):
    case_id = R.MUTANTS[mutant]
    moved = R.rel(R.expected(case_id, mutant), R.expected(case_id))
    print(f"{mutant}: moves {case_id} by {moved:.3g} (100 bars = {R.MUTANT_MIN_BARS * R.DEVICE_BAR:.3g})")
    assert moved >= R.MUTANT_MIN_BARS * R.DEVICE_BAR


def test_the_named_cases_are_what_the_mutants_need():
    for name in ("masked_to_zero", "mask_ignored", "rect_origin_ignored"):
        case = R.BY_ID[R.MUTANTS[name]]
        assert case.masked and case.rect is not None and case.rect[0] % 2 == 1 and case.rect[2] % 2 == 1
    n, h, w = R.BY_ID[R.MUTANTS["ceil_mode"]].shape
    s = lambda v: (v - 7) // 4 + 1
    assert (s(h) - 3) % 2 or (s(w) - 3) % 2                                  # floor and ceil pooling differ
    assert R.BY_ID[R.MUTANTS["channels_not_swapped"]].order == "bgr"
    assert R.BY_ID["min_31x31"].shape[1:] == (R.MIN_SIDE, R.MIN_SIDE) == (lpips.MIN_SIDE,) * 2
    assert [t.shape[2:] for t in R.taps(torch.zeros(1, 3, 31, 31, dtype=torch.float64), R.weights())][-1] == (1, 1)
    with pytest.raises(RuntimeError):                                        # 30 x 31: nothing left for the second pool
        R.taps(torch.zeros(1, 3, 30, 31, dtype=torch.float64), R.weights())


def test_cpu_float32_figure_behind_the_device_bar():
    """DEVICE_BAR = 32 x the worst float32-vs-float64 distance of the restatement over the case matrix.  The figure
    was measured as 1.986e-6 (the one-LSB case, a score of 3.4e-8 against the 1e-6 floor); torch's float32 summation
    order follows the CPU's vector width, so a factor 4 is allowed before the constant has to be measured again."""
    worst = max(R.rel(R.expected(c.id, dtype=torch.float32), R.expected(c.id)) for c in R.CASES)
    print(f"CPU float32 worst {worst:.4g}; constant {R.CPU_F32_WORST:.4g}; device bar {R.DEVICE_BAR:.4g}")
    assert worst <= 4 * R.CPU_F32_WORST
    assert R.DEVICE_BAR == 32 * R.CPU_F32_WORST
    assert float(R.expected("identical")[0]) == 0.0 and 0.0 < float(R.expected("one_lsb")[0]) < 1e-6
    assert float(R.expected("black_white")[0]) > 0.1


# ----------------------------------------------------------------------------- weights and the loader
def test_state_dict_loader_round_trips_both_spellings_and_refuses_negative_weights():
    sd = weights.make_lpips_weights(0)
    assert sd.keys() == weights.make_lpips_weights(0).keys() and all(torch.equal(v, weights.make_lpips_weights(0)[k]) for k, v in sd.items())
    assert not torch.equal(sd["features.0.weight"], weights.make_lpips_weights(1)["features.0.weight"])
    assert all(bool((sd[f"lin{k}.model.1.weight"] >= 0).all()) and sd[f"lin{k}.model.1.weight"].shape == (1, c, 1, 1)
               for k, c in enumerate(R.TAP_CHANNELS))
    plain = lpips.load_lpips_state_dict(sd)
    assert plain.keys() == sd.keys() and all(torch.equal(plain[k], sd[k]) for k in sd)
    wrapped = {}
    for k, v in sd.items():
        if k.startswith("features."):
            idx = int(k.split(".")[1])
            wrapped[f"net.slice{R.CONV_IDX.index(idx) + 1}.{k[len('features.'):]}"] = v.double()
        else:
            wrapped[k] = v
    wrapped["scaling_layer.shift"] = torch.zeros(1, 3, 1, 1)                 # other keys are ignored
    back = lpips.load_lpips_state_dict(wrapped)
    assert back.keys() == sd.keys() and all(torch.equal(back[k], sd[k]) and back[k].dtype == torch.float32 for k in sd)
    bad = dict(sd)
    bad["lin2.model.1.weight"] = sd["lin2.model.1.weight"].clone()
    bad["lin2.model.1.weight"][0, 5, 0, 0] = -1e-3
    with pytest.raises(ValueError, match="negative"):
        lpips.load_lpips_state_dict(bad)
    for drop in ("features.6.bias", "lin4.model.1.weight"):
        with pytest.raises(ValueError, match="missing|present"):
            lpips.load_lpips_state_dict({k: v for k, v in sd.items() if k != drop})
    with pytest.raises(ValueError, match="shape"):
        lpips.load_lpips_state_dict({**sd, "lin0.model.1.weight": sd["lin0.model.1.weight"].reshape(64)})
    assert "UNVERIFIED" in lpips.load_lpips_state_dict.__doc__


def test_python_surface_without_a_gpu():
    for name in ("LpipsAlex", "get_lpips_model", "lpips_device", "calculate_lpips_per_frame", "calculate_lpips", "load_lpips_state_dict"):
        assert getattr(elvis_amd, name) is getattr(lpips, name)
    frame = np.zeros((31, 31, 3), np.uint8)
    assert lpips.calculate_lpips_per_frame([], [frame]) == [] and lpips.calculate_lpips_per_frame([frame], []) == []
    assert lpips.calculate_lpips_per_frame([None, frame], [frame, None]) == []      # nothing to score: no device is asked for
    assert lpips.calculate_lpips([], [frame], model=None) == []
    with pytest.raises(ValueError, match="uint8"):
        lpips.calculate_lpips_per_frame([frame], [frame.astype(np.float32)])
    with pytest.raises(ValueError, match="uint8"):
        lpips.calculate_lpips_per_frame([frame], [frame[:30]])
    assert "does NOT claim parity with the\nlpips package" in lpips.__doc__


# ----------------------------------------------------------------------------- the built library
def test_library_exports_the_entries(built_lib):
    h = _lib.lib()
    text = open(os.path.join(ROOT, "include", "elvis_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for entry, nargs in ENTRIES.items():
        assert hasattr(h, entry) and len(_lib.SIGNATURES[entry]) == nargs
        decl = re.search(r"\b(?:int|size_t)\s+" + entry + r"\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
        assert decl and len([a for a in decl.group(1).split(",") if a.strip()]) == nargs
        before = text[:text.index(entry + "(")]
        assert "elvis.py:3163-3195" in before[before.rindex("/*"):], f"{entry} does not cite the reference"
    assert "lpips.hip" in _build.SOURCES
    assert h.elvis_lpips_distance_workspace_bytes(3, 5, 27) == 3 * 3 * 8 and h.elvis_lpips_distance_workspace_bytes(1, 8, 8) == 8
    assert h.elvis_lpips_distance_workspace_bytes(-1, 8, 8) == 0 and h.elvis_lpips_distance_workspace_bytes(1, 0, 8) == 0


def test_argument_errors_without_a_gpu(built_lib):
    h = _lib.lib()

    def bad(rc, word):
        assert rc == -1 and word in h.elvis_last_error(), (rc, h.elvis_last_error())
    p = 256                                                                   # never dereferenced: every call is refused
    stem = lambda *a: h.elvis_lpips_stem_u8(*a, None)
    bad(stem(p, None, p, p, p, 1, 70, 90, 5, 64, 9, 82, 2, 64), b"order")
    bad(stem(p, None, p, p, p, 1, 70, 90, 5, 64, 9, 82, -1, 64), b"order")
    for rect in ((-1, 64, 9, 82), (5, 71, 9, 82), (5, 64, -2, 82), (5, 64, 9, 91), (5, 35, 9, 82), (5, 64, 9, 39), (40, 30, 9, 82)):
        bad(stem(p, None, p, p, p, 1, 70, 90, *rect, 1, 64), b"rect")
    bad(stem(p, None, p, p, p, 1, 30, 90, 0, 30, 0, 90, 1, 64), b"rect")
    for pitch in (60, 68, 56, 0):
        bad(stem(p, None, p, p, p, 1, 70, 90, 5, 64, 9, 82, 1, pitch), b"pitch")
    bad(stem(p, None, p, p, p, -1, 70, 90, 5, 64, 9, 82, 1, 64), b"bad shape")
    for k in (0, 2, 3, 4):                                                    # frames, weight, bias, out (the mask may be null)
        args = [p, None, p, p, p]
        args[k] = None
        bad(stem(*args, 1, 70, 90, 5, 64, 9, 82, 1, 64), b"null")
    bad(stem(p, None, p, p, p + 4, 1, 70, 90, 5, 64, 9, 82, 1, 64), b"aligned")
    assert stem(None, None, None, None, None, 0, 70, 90, 5, 64, 9, 82, 1, 64) == 0       # n == 0: no-op

    conv = lambda *a: h.elvis_lpips_conv5_f32(*a, None)
    for pitches in ((60, 192), (68, 192), (64, 188), (64, 196), (56, 192), (64, 184)):
        bad(conv(p, p, p, p, 1, 9, 9, *pitches), b"pitch")
    bad(conv(p, p, p, p, 1, 0, 9, 64, 192), b"bad shape")
    for k in range(4):
        args = [p, p, p, p]
        args[k] = None
        bad(conv(*args, 1, 9, 9, 64, 192), b"null")
    bad(conv(p + 8, p, p, p, 1, 9, 9, 64, 192), b"aligned")
    assert conv(None, None, None, None, 0, 9, 9, 64, 192) == 0

    pool = lambda *a: h.elvis_lpips_maxpool_f32(*a, None)
    bad(pool(p, p, 1, 2, 9, 64, 64, 64), b"bad shape")
    bad(pool(p, p, 1, 9, 9, 62, 64, 64), b"fours")
    for pitches in ((60, 64), (64, 68), (56, 64), (64, 56)):
        bad(pool(p, p, 1, 9, 9, 64, *pitches), b"pitch")
    bad(pool(None, p, 1, 9, 9, 64, 64, 64), b"null")
    bad(pool(p, None, 1, 9, 9, 64, 64, 64), b"null")
    assert pool(None, None, 0, 9, 9, 64, 64, 64) == 0

    dist = lambda *a: h.elvis_lpips_distance_f64(*a, None)
    bad(dist(p, p, p, p, p, 1, 5, 5, 0, 64, 0), b"channels")
    bad(dist(p, p, p, p, p, 1, 5, 5, 385, 392, 0), b"channels")
    for c, pitch in ((64, 60), (64, 68), (64, 56), (192, 184)):
        bad(dist(p, p, p, p, p, 1, 5, 5, c, pitch, 0), b"pitch")
    bad(dist(p, p, p, p, p, 1, 5, 5, 64, 64, 2), b"accumulate")
    bad(dist(p, p, p, p, p, 1, 0, 5, 64, 64, 0), b"bad shape")
    for k in range(5):
        args = [p, p, p, p, p]
        args[k] = None
        bad(dist(*args, 1, 5, 5, 64, 64, 0), b"null")
    assert dist(None, None, None, None, None, 0, 5, 5, 64, 64, 0) == 0


def test_kernel_ledger(built_lib):
    """Both directions: no kernel of lpips.hip that the GPU cases do not name, no case naming a kernel the library lacks;
    every kernel carries the lpips_ prefix; no atomics."""
    from _glueref import kernel_stems
    from _qualitycases import kernel_names
    stems = kernel_stems(SOURCE)
    assert stems == {"lpips_stem_kernel", "lpips_conv5_kernel", "lpips_maxpool_kernel", "lpips_distance_kernel", "lpips_finish_kernel"}
    built = kernel_names(built_lib, SOURCE)
    named = {k for c in R.CASES for k in c.kernels}
    assert not built - named, f"kernels of lpips.hip without a case: {sorted(built - named)}"
    assert not named - built, f"cases naming kernels the library does not build: {sorted(named - built)}"
    assert len(built) == 6
    text = open(SOURCE).read()
    assert len(re.findall(r"hipLaunchKernelGGL\(", text)) == 5 and not re.search(r"\batomic\w*\s*\(", text)
    for name in built:
        assert f'"{name.split("<")[0]}' in text                                # what elvis_last_launch reports
