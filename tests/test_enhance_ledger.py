"""The ledger of csrc/sr_enhance.hip (the kernels in the built library are exactly the ones the cases of
tests/test_gpu_enhance.py name) and the discrimination test of its statement (tests/_enhance_ref.py): every mutant of a
rule differs from the true statement on the stated inputs - otherwise the inputs could not tell a wrong kernel from a
right one."""
import os

import numpy as np
import pytest

import _enhance_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "elvis_amd", "csrc", "sr_enhance.hip")
CHANNELS = E.CHANNELS                 # what every resize case runs with
# what elvis_last_launch reports per entry point in the GPU cases: every channel count the entry point takes has a case
CASE_CHANNELS = {c for name in E.RESIZE_CASES for c in E.CHANNELS + E.EXTRA_CHANNELS.get(name, ())}
NAMED = {f"resize_lanczos4_u8_kernel<{c}>" for c in CASE_CHANNELS} | {"sr_gather_tiles_u8_kernel", "sr_paste_tiles_u8_kernel"}


def test_kernel_ledger(built_lib):
    built = E.kernel_names(built_lib, SOURCE)
    from _glueref import kernel_stems
    assert kernel_stems(SOURCE) == {"resize_lanczos4_u8_kernel", "sr_gather_tiles_u8_kernel", "sr_paste_tiles_u8_kernel"}
    assert CASE_CHANNELS == {1, 2, 3, 4}
    assert built == NAMED, (sorted(built - NAMED), sorted(NAMED - built))
    text = open(SOURCE).read()
    for name in NAMED:
        assert f'"{name}"' in text


def _resize_differs(mutant, names=E.RESIZE_CASES):
    hits = []
    for name in names:
        hs, ws, hd, wd = E.RESIZE_CASES[name]
        for c in CHANNELS:
            for kind in ("random", "checker"):
                x = E.resize_inputs(name, c, kind)
                if not np.array_equal(E.resize(x, hd, wd), E.resize(x, hd, wd, mutant)):
                    hits.append((name, c, kind))
    return hits


def test_rounding_constant_mutant():
    hits = _resize_differs("round0")
    assert {h[0] for h in hits} >= {"down2", "down4", "up2", "mixed", "narrow"}
    assert not any(h[0] == "identity" for h in hits)


def test_clamp_off_by_one_mutant():
    hits = _resize_differs("clamp")
    assert {h[0] for h in hits} >= {"down2", "up2", "mixed", "narrow"} and {h[1] for h in hits} == set(CHANNELS)


def test_floor_versus_trunc_mutant():
    """fx is negative only for the first destination indices of an upscale: trunc gives sx = 0 where floor gives -1."""
    hits = _resize_differs("trunc")
    assert {h[0] for h in hits} == {"up2", "mixed", "narrow"}             # the cases with an axis that grows
    first, _ = E.taps(8, 16)
    assert first[0] == -4 and E.taps(8, 16, "trunc")[0][0] == -3


def _frames(H, W, n=2):
    return np.random.default_rng(H * 100 + W).integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)


def test_reflect_including_the_edge_mutant():
    """The padding reaches the output only as the network's context (post_process crops it off), so a context-free
    stand-in network cannot see it: the maps and the padded image are compared, as the GPU gather case does."""
    rows, cols = E.index_maps(9, 13, 3, 2)
    bad_rows, bad_cols = E.index_maps(9, 13, 3, 2, "edge")
    assert rows.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 7, 6, 5] and bad_rows.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 7, 6]
    assert cols.tolist()[13:] == [11, 10, 9] and bad_cols.tolist()[13:] == [12, 11, 10]
    x = _frames(9, 13)
    assert not np.array_equal(x[:, rows][:, :, cols], x[:, bad_rows][:, :, bad_cols])
    # the mod pad alone (an odd side, x2)
    r2, _ = E.index_maps(9, 13, 0, 2)
    assert r2.tolist()[-1] == 7 and E.index_maps(9, 13, 0, 2, "edge")[0].tolist()[-1] == 8


def test_paste_crop_offset_mutant():
    for (H, W) in ((16, 24), (9, 13)):
        for s in (2, 4):
            x = _frames(H, W)
            mod = 2 if s == 2 else 1
            for tile, pad in ((8, 3), (6, 10)):
                true = E.compose(x, E.nearest_forward(s), s, tile, pad, mod=mod)
                assert not np.array_equal(true, E.compose(x, E.nearest_forward(s), s, tile, pad, mod=mod, mutant="crop_no_s"))
            # without tile_pad the crop starts at 0 either way: the mutant is invisible there
            assert np.array_equal(E.compose(x, E.nearest_forward(s), s, 8, 0, mod=mod),
                                  E.compose(x, E.nearest_forward(s), s, 8, 0, mod=mod, mutant="crop_no_s"))


def test_every_mutant_has_its_test():
    assert set(E.MUTANTS) == {"round0", "clamp", "trunc", "edge", "crop_no_s"}
