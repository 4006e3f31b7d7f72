"""CPU-side checks of elvis_amd/enhance.py: the Lanczos4 tables against the existing per-block ones and against the numpy
statement (tests/_enhance_ref.py), the int32 bound, the LDS tile plan, the reflect maps against torch's own padding, the
tile plan's partition, every ValueError, the exports and the C ABI's argument checks."""
import inspect
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _enhance_ref as E
import elvis_amd
from elvis_amd import _lib, classical, drivers, enhance, restore

PHASE_2_1 = (-26, 122, -340, 1267, 1267, -340, 122, -26)


# ----------------------------------------------------------------------------- tables
@pytest.mark.parametrize("f", [2, 4, 8, 16, 32])
def test_taps_equal_the_per_block_upscale_tables(f):
    for b in (32, 64):
        first, taps = enhance.lanczos4_resize_taps(b // f, b)
        want_first, want_taps = classical.lanczos_taps(f, b)
        assert first.dtype == np.int32 and taps.dtype == np.int16 and taps.shape == (b, 8)
        assert np.array_equal(first, want_first) and np.array_equal(taps, want_taps)


def test_integer_downscales_have_one_phase():
    for ratio, offset in ((2, -3), (4, -2)):
        first, taps = enhance.lanczos4_resize_taps(ratio * 24, 24)
        assert np.array_equal(first, ratio * np.arange(24) + offset)
        assert all(tuple(t) == PHASE_2_1 for t in taps.tolist())


def test_taps_equal_the_statement_and_are_cached():
    pairs = set(E.DRIVER_RATIOS[12:])
    for hs, ws, hd, wd in E.RESIZE_CASES.values():
        pairs |= {(hs, hd), (ws, wd)}
    for n_src, n_dst in sorted(pairs):
        first, taps = enhance.lanczos4_resize_taps(n_src, n_dst)
        want_first, want_taps = E.taps(n_src, n_dst)
        assert np.array_equal(first, want_first) and np.array_equal(taps, want_taps), (n_src, n_dst)
        assert first.min() >= -4 and first.max() <= n_src - 4 and (np.diff(first) >= 0).all()
    assert enhance.lanczos4_resize_taps(13, 9)[1] is enhance.lanczos4_resize_taps(13, 9)[1]
    assert not enhance.lanczos4_resize_taps(13, 9)[1].flags.writeable
    with pytest.raises(ValueError, match="positive"):
        enhance.lanczos4_resize_taps(0, 4)


def test_the_statement_resizes_to_the_same_size_as_the_identity():
    x = E.resize_inputs("identity", 3, "random")
    out = E.resize(x, 8, 12)
    assert np.array_equal(out, x) and out is not x
    # and through the taps themselves: every phase of a 1:1 resize is the unit tap
    first, taps = enhance.lanczos4_resize_taps(12, 12)
    assert np.array_equal(first, np.arange(12) - 3) and (taps == np.array([0, 0, 0, 2048, 0, 0, 0, 0])).all()
    assert np.array_equal(np.clip((E.resize_raw(x, 8, 12) + (1 << 21)) >> 22, 0, 255), x)


def test_the_checkerboards_saturate_both_ways():
    low = high = False
    for name, (hs, ws, hd, wd) in E.RESIZE_CASES.items():
        raw = (E.resize_raw(E.resize_inputs(name, 1, "checker"), hd, wd) + (1 << 21)) >> 22
        low, high = low or bool((raw < 0).any()), high or bool((raw > 255).any())
    assert low and high


def test_the_int32_bound_holds_for_every_ratio_used():
    pairs = [((hs, hd), (ws, wd)) for hs, ws, hd, wd in E.gpu_resizes()]
    assert ((36, 22), (52, 32)) in pairs                 # outscale 2.5 of the 9 x 13 image
    pairs += [(E.DRIVER_RATIOS[i], E.DRIVER_RATIOS[i + 1]) for i in range(0, len(E.DRIVER_RATIOS), 2)]
    worst = 0
    for (hs, hd), (ws, wd) in pairs:
        xt, yt = enhance.lanczos4_resize_taps(ws, wd)[1], enhance.lanczos4_resize_taps(hs, hd)[1]
        bound = enhance.lanczos4_sum_bound(xt, yt)
        assert bound == E.sum_bound(np.unique(xt.astype(np.int64), axis=0), np.unique(yt.astype(np.int64), axis=0))
        assert bound < 2 ** 31, (hs, ws, hd, wd, bound)
        worst = max(worst, bound)
    assert worst > 2 ** 30                       # the margin is thin: the check is not vacuous


def test_a_bound_of_2_31_is_refused(monkeypatch):
    """The host refuses tables whose sums could leave int32, before any launch: `_checked_tables` is what
    `resize_lanczos4_device` and `resize_tile_plan` get their tables from."""
    first = np.arange(4, dtype=np.int32) - 3
    big = np.full((4, 8), 2000, np.int16)
    assert enhance.lanczos4_sum_bound(big, big) >= 2 ** 31
    monkeypatch.setattr(enhance, "lanczos4_resize_taps", lambda n_src, n_dst: (first, big))
    with pytest.raises(ValueError, match="int32 limit is 2147483647"):
        enhance._checked_tables.__wrapped__(4, 4, 4, 4)
    monkeypatch.undo()
    # the comparison itself: exactly 2^31 is refused, 2^31 - 1 is taken
    assert enhance.INT32_LIMIT == 2 ** 31
    monkeypatch.setattr(enhance, "lanczos4_sum_bound", lambda xt, yt: 2 ** 31)
    with pytest.raises(ValueError, match=f"allow a sum of {2 ** 31}"):
        enhance._checked_tables.__wrapped__(16, 24, 8, 12)
    monkeypatch.setattr(enhance, "lanczos4_sum_bound", lambda xt, yt: 2 ** 31 - 1)
    xf, xt, yf, yt = enhance._checked_tables.__wrapped__(16, 24, 8, 12)
    assert xf is enhance.lanczos4_resize_taps(24, 12)[0] and yt is enhance.lanczos4_resize_taps(16, 8)[1]
    monkeypatch.undo()
    # and the two callers go through it: a refused table reaches neither the tile plan nor a launch
    monkeypatch.setattr(enhance, "lanczos4_sum_bound", lambda xt, yt: 2 ** 31)
    with pytest.raises(ValueError, match="int32 limit"):
        enhance.resize_tile_plan.__wrapped__(30, 40, 10, 20, 3)


def test_resize_tile_plan(built_lib):
    plus_one = set()
    for (name, c), tile in E.RESIZE_TILE_OF.items():
        hs, ws, hd, wd = E.RESIZE_CASES[name]
        th, tw, need = enhance.resize_tile_plan(hs, ws, hd, wd, c)
        assert (th, tw) == tile and 0 < need <= enhance.LDS_LIMIT
        if (hd, wd) == (th + 1, tw + 1):
            plus_one.add((c, tile))
    assert plus_one == {(1, (16, 64)), (3, (16, 64)), (3, (16, 32))}
    # the 1080p shapes of the two paths fit, with two workgroups per CU (160 KiB of LDS)
    for hs, ws in ((2160, 3840), (4320, 7680)):
        th, tw, need = enhance.resize_tile_plan(hs, ws, 1080, 1920, 3)
        assert (th, tw) in enhance.RESIZE_TILES and 2 * need <= 160 * 1024
    assert enhance.LDS_LIMIT * 2 <= 160 * 1024
    with pytest.raises(ValueError, match="LDS"):
        enhance.resize_tile_plan(6400, 6400, 100, 100, 3)


# ----------------------------------------------------------------------------- padding
@pytest.mark.parametrize("H,W,pre_pad,mod", list(itertools.product((5, 8, 9), (5, 8, 9), (0, 1, 4), (1, 2))))
def test_reflect_index_maps_equal_torch_padding(H, W, pre_pad, mod):
    img = torch.arange(H * W, dtype=torch.float32).reshape(1, 1, H, W)
    padded = F.pad(img, (0, pre_pad, 0, pre_pad), "reflect") if pre_pad else img
    ph, pw = (-padded.shape[2]) % mod, (-padded.shape[3]) % mod
    padded = F.pad(padded, (0, pw, 0, ph), "reflect")
    rows, cols = enhance.reflect_index_maps(H, W, pre_pad, mod)
    assert rows.dtype == np.int32 and cols.dtype == np.int32
    assert np.array_equal(img[0, 0].numpy()[rows][:, cols], padded[0, 0].numpy())
    want_rows, want_cols = E.index_maps(H, W, pre_pad, mod)
    assert np.array_equal(rows, want_rows) and np.array_equal(cols, want_cols)


# ----------------------------------------------------------------------------- tiles
@pytest.mark.parametrize("H,W", [(8, 12), (9, 13), (16, 24)])
@pytest.mark.parametrize("tile", [4, 6, 8, 64])
def test_plan_tiles_partitions_the_output(H, W, tile):
    for tile_pad in (0, 3, 10, tile + 5):
        for s in (2, 4):
            plan = enhance.plan_tiles(H, W, tile, tile_pad, s)
            assert [tuple(t) for t in plan] == E.plan_tiles(H, W, tile, tile_pad, s)
            assert len(plan) == -(-H // tile) * -(-W // tile)
            hits = np.zeros((s * H, s * W), np.int32)
            for t in plan:
                hits[t.out_y:t.out_y + t.out_h, t.out_x:t.out_x + t.out_w] += 1
                assert 0 <= t.y0 and t.y0 + t.h <= H and 0 <= t.x0 and t.x0 + t.w <= W
                assert t.crop_y + t.out_h <= s * t.h and t.crop_x + t.out_w <= s * t.w
                assert t.crop_y == s * (t.out_y // s - t.y0) and t.crop_x == s * (t.out_x // s - t.x0)
            assert (hits == 1).all()
            # shape classes: per axis the first, the inner, the last tile and, when the pad reaches over the last one, the
            # one before it
            assert len({(t.h, t.w) for t in plan}) <= 16
    assert len({(t.h, t.w) for t in enhance.plan_tiles(1080, 1920, 512, 10, 4)}) == 9
    assert [tuple(t) for t in enhance.plan_tiles(H, W, 0, 10, 4)] == [(0, 0, H, W, 0, 0, 0, 0, 4 * H, 4 * W)]


# ----------------------------------------------------------------------------- errors, exports, ABI
class _FakeModel:
    def __init__(self, scale):
        self.scale, self.device = scale, torch.device("cuda:0")


def test_value_errors():
    with pytest.raises(ValueError, match="odd"):
        enhance.RealESRGANer(_FakeModel(2), tile=7)
    enhance.RealESRGANer(_FakeModel(4), tile=7)
    with pytest.raises(ValueError, match="negative"):
        enhance.RealESRGANer(_FakeModel(4), tile_pad=-1)
    for H, W, p in ((8, 5, 5), (4, 9, 4), (5, 5, 7)):
        with pytest.raises(ValueError, match="pre_pad"):
            enhance.reflect_index_maps(H, W, p, 1)
    with pytest.raises(ValueError, match="reflect"):
        enhance.reflect_index_maps(1, 8, 0, 2)              # the mod pad of a one-pixel side
    enh = enhance.RealESRGANer(_FakeModel(4))
    for bad in (np.zeros((8, 8), np.uint8), np.zeros((8, 8, 4), np.uint8), np.zeros((8, 8, 3), np.uint16)):
        with pytest.raises(ValueError, match="gray, RGBA and 16-bit"):
            enh.enhance(bad)
    with pytest.raises(ValueError, match="uint8"):
        enhance.resize_lanczos4_device(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), 2, 2)      # not on the device
    with pytest.raises(ValueError, match="plan_tiles"):
        enhance.plan_tiles(8, 8, -1, 0)
    # the wiring: an unknown mode, and the departures of the default mode stay
    with pytest.raises(ValueError, match="enhance"):
        restore._check_realesrgan_args(1.0, 0, False, None, "lanczos")
    with pytest.raises(ValueError, match="pre_pad"):
        restore._check_realesrgan_args(1.0, 4, False)
    with pytest.raises(ValueError, match="pre_pad"):
        restore._check_realesrgan_args(1.0, 4, False, None, "area")
    assert restore._check_realesrgan_args(1.0, 4, False, None, "reference") is None
    with pytest.raises(ValueError, match="negative"):
        restore._check_realesrgan_args(1.0, -1, False, None, "reference")
    with pytest.raises(ValueError, match="fp32"):
        restore._check_realesrgan_args(1.0, 0, True, None, "reference")


def test_the_driver_takes_the_keyword(tmp_path):
    src = tmp_path / "in"
    src.mkdir()
    with pytest.raises(ValueError, match="enhance"):
        drivers.restore_downsampled_with_realesrgan(str(src), str(tmp_path / "o"), np.zeros((1, 1, 1)), 8, enhance="cubic")
    with pytest.raises(ValueError, match="No frames found"):          # pre_pad passes the checks with "reference"
        drivers.restore_downsampled_with_realesrgan(str(src), str(tmp_path / "o"), np.zeros((1, 1, 1)), 8, enhance="reference",
                                                    pre_pad=4, tile=8)


def test_exports_and_defaults():
    for name in ("RealESRGANer", "lanczos4_resize_taps", "plan_tiles", "reflect_index_maps", "resize_lanczos4_device",
                 "upscale_with_realesrgan"):
        assert getattr(elvis_amd, name) is getattr(enhance, name)
    for fn in (restore.get_realesrgan_upsample_fn, restore.restore_frames_realesrgan, restore.restore_frames_realesrgan_device,
               restore.restore_with_realesrgan_naive, drivers.restore_downsampled_with_realesrgan):
        assert inspect.signature(fn).parameters["enhance"].default == "area", fn.__name__
    sig = inspect.signature(enhance.RealESRGANer.__init__).parameters
    assert (sig["tile"].default, sig["tile_pad"].default, sig["pre_pad"].default) == (0, 10, 0)
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("tile", "tile_pad", "pre_pad"))
    assert enhance.upscale_with_realesrgan([np.zeros((2, 2, 3), np.uint8)], None, degradation_level=0)[0].shape == (2, 2, 3)
    assert len(_lib.SIGNATURES["elvis_resize_lanczos4_u8"]) == 17 and len(_lib.SIGNATURES["elvis_resize_lanczos4_lds_bytes"]) == 9
    assert len(_lib.SIGNATURES["elvis_sr_gather_tiles_u8"]) == 17 and len(_lib.SIGNATURES["elvis_sr_paste_tiles_u8"]) == 11


def test_entry_points_validate_before_any_launch(built_lib):
    h = _lib.lib()
    xf, xt = enhance.lanczos4_resize_taps(24, 12)
    yf, yt = enhance.lanczos4_resize_taps(16, 8)
    xt, yt = np.array(xt), np.array(yt)
    p = lambda a: a.ctypes.data
    ok = (16, 16, 2, 16, 24, 8, 12, 3, p(xf), p(yf), p(xf), p(xt), p(yf), p(yt), 16, 64, None)

    def resize(**kw):
        names = ("src", "dst", "n", "hs", "ws", "hd", "wd", "c", "xfh", "yfh", "xf", "xt", "yf", "yt", "th", "tw", "stream")
        args = dict(zip(names, ok))
        args.update(kw)
        rc = h.elvis_resize_lanczos4_u8(*[args[k] for k in names])
        return rc, h.elvis_last_error()

    for kw, msg in ((dict(src=None), b"null"), (dict(xfh=None), b"null"), (dict(yt=None), b"null"), (dict(n=0), b"frame count"),
                    (dict(hd=0), b"bad shape"), (dict(c=5), b"channels"), (dict(th=0), b"tile"), (dict(tw=512), b"tile"),
                    (dict(xt=p(xt) + 2), b"aligned")):
        rc, err = resize(**kw)
        assert rc == -1 and msg in err, (kw, err)
    bad = np.array(xf)
    bad[3] = 24
    rc, err = resize(xfh=p(bad))
    assert rc == -1 and b"column table entry 3" in err
    bad = np.array(yf)
    bad[5] = bad[4] - 1
    rc, err = resize(yfh=p(bad))
    assert rc == -1 and b"row table entry 5" in err
    # a footprint over the limit: 64:1 both ways at the largest tile
    sxf, syf = enhance.lanczos4_resize_taps(6400, 100)[0], enhance.lanczos4_resize_taps(6400, 100)[0]
    assert h.elvis_resize_lanczos4_lds_bytes(p(sxf), p(syf), 6400, 6400, 100, 100, 3, 4, 16) > enhance.LDS_LIMIT
    rc = h.elvis_resize_lanczos4_u8(16, 16, 1, 6400, 6400, 100, 100, 3, p(sxf), p(syf), 16, 16, 16, 16, 4, 16, None)
    assert rc == -1 and b"bytes of LDS" in h.elvis_last_error()
    assert h.elvis_resize_lanczos4_lds_bytes(None, p(yf), 16, 24, 8, 12, 3, 16, 64) == -1

    desc = np.array([[0, 0, 0], [1, 2, 4]], np.int32)
    rows, cols = enhance.reflect_index_maps(9, 13, 3, 2)
    g_ok = dict(src=16, dst=16, n=2, H=9, W=13, T=2, th=8, tw=8, dh=p(desc), d=16, rh=p(rows), r=16, Hp=12, ch=p(cols), c=16, Wp=16,
                stream=None)

    def gather(**kw):
        args = dict(g_ok)
        args.update(kw)
        return h.elvis_sr_gather_tiles_u8(*args.values()), h.elvis_last_error()

    for kw, msg in ((dict(dst=None), b"null"), (dict(rh=None), b"null"), (dict(T=0), b"bad shape"), (dict(th=13), b"does not fit"),
                    (dict(n=1), b"tile 1"), (dict(H=8), b"row map entry"), (dict(W=12), b"column map entry")):
        rc, err = gather(**kw)
        assert rc == -1 and msg in err, (kw, err)
    far = np.array([[0, 5, 0]], np.int32)
    rc, err = gather(T=1, dh=p(far))
    assert rc == -1 and b"tile 0" in err

    pd = np.array([[0, 4, 4, 0, 0, 8, 8]], np.int32)

    def paste(desc_h, **kw):
        args = dict(tiles=16, dst=16, T=1, tth=16, ttw=16, n=1, OH=32, OW=32, dh=p(desc_h), d=16, stream=None)
        args.update(kw)
        return h.elvis_sr_paste_tiles_u8(*args.values()), h.elvis_last_error()

    for kw, msg in ((dict(tiles=None), b"null"), (dict(d=None), b"null"), (dict(OH=0), b"bad shape"), (dict(tth=11), b"outside the"),
                    (dict(n=0), b"bad shape")):
        rc, err = paste(pd, **kw)
        assert rc == -1 and msg in err, (kw, err)
    for col, val, msg in ((0, 1, b"names frame"), (3, -1, b"negative destination"), (5, 0, b"outside the"), (2, 9, b"outside the")):
        e = pd.copy()
        e[0, col] = val
        rc, err = paste(e)
        assert rc == -1 and msg in err, (col, err)
