"""The cases of the stream tests (tests/test_gpu_streams.py) that tests/_dirtycases.py does not hold, and the ledger of
the streamed entry points.

SPLITS: one split case per family - the 20 of tests/_dirtycases.py and jpeg_write, resize, vq_index, gn_fused.  A split
case keeps its inputs apart from the call, so that the test can put DECOYS into the argument tensors, queue the copy of
the real inputs behind a stall on the current stream, and call the surface while the device still holds the decoys:
work that escapes to another stream computes on the decoy.  A decoy is a valid input of the same shape and dtype (masks
stay masks, maps stay in range): a kernel that reads one computes a wrong answer, never a wrong address.  Every
statement is the family's own (tests/_*_ref.py); nothing is restated here.

CASES: cases of `_dirtycases.Case`'s shape for test (a) - every split case as one run, and what neither table reached:
the JPEG writer's restart, ROI and optimised forms, the run-length PNG writer, the codebook scan, and one case each of
the norm / misc, model-kernel and glue matrices for `elvis_affine_act`, `elvis_convert_act`, `elvis_swin_mlp` (with its
packer), `elvis_select_levels_u8` and `elvis_sse_u8`, through those matrices' own runners.

REACHED: every streamed entry point of include/elvis_amd.h -> the ids of the cases (of `_dirtycases.CASES` and of CASES
here) whose recorded run calls it, or a reason why no case does.  tests/test_gpu_streams.py checks each claim.

Nothing here touches the GPU at import; references are computed on first use.
"""
import importlib
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

import _dirtycases as D
from _dirtycases import Case, _exact, _once, _rel


@dataclass(frozen=True)
class Split:
    id: str
    family: str
    source: str                         # the reference module / test the case is borrowed from
    inputs: Callable                    # () -> {name: ndarray}, the real inputs
    decoy: Callable                     # () -> {name: ndarray}, same names, shapes and dtypes, valid inputs
    call: Callable                      # (tensors {name: device tensor}, box) -> {name: tensor | ndarray | bytes}
    expected: Callable                  # (inputs {name: ndarray}) -> what `compare` takes, from the statement only
    compare: Callable                   # (got {name: ndarray | bytes}, want) -> None, raises AssertionError
    outputs: Callable                   # (want) -> {name: ndarray | bytes}: the named outputs, for the ledger
    syncs: str = ""                     # where the surface waits for the stream inside (read from its code); "" if nowhere
    bound: Optional[Callable] = None    # float families: (want) -> {name: the comparison's bound per element}; None: byte for byte
    prepare: Optional[Callable] = None  # (device) -> box, before the stall: weights, packed images, models


SPLITS = {}
CASES = {}


def _split(s: Split):
    assert s.id not in SPLITS and s.id not in D.CASES, s.id
    SPLITS[s.id] = s

    def run(dev):
        box = s.prepare(dev) if s.prepare else None
        return s.call({k: torch.from_numpy(np.array(v)).to(dev) for k, v in s.inputs().items()}, box)

    _case(Case(s.id, s.family, (0, 0, 0), s.source, run, _once(lambda: s.expected(s.inputs())), s.compare))


def _case(c: Case):
    assert c.id not in CASES and c.id not in D.CASES, c.id
    CASES[c.id] = c


PIXELS = ("frames", "a", "b", "src", "ref", "dis", "prev", "odd", "wide")       # inputs that are images: every byte is a valid one


def _named(want):
    return want


def _flip(a):
    """A valid twin of a uint8 image clip: inverted and turned upside down."""
    return np.ascontiguousarray(255 - a[:, ::-1])


def _turn(m):
    """A valid twin of a mask or a per-block map: the same values, turned by half a turn."""
    return np.ascontiguousarray(m[:, ::-1, ::-1])


# ----------------------------------------------------------------------------------------------------------- segment
def _segment():
    R = importlib.import_module("_segment_ref")
    name = "21x23_n3"
    given = _once(lambda: R.cases()[name])

    def call(t, box):
        from elvis_amd import segment
        _, order, kw = given()
        return {"masks": segment.foreground_masks_device(t["frames"], order, segment.SegmentConfig(**kw))}

    def expected(inp):
        _, order, kw = given()
        return {"masks": R.segment(inp["frames"], order, R.SegmentConfig(**kw))}

    _split(Split(f"split_segment_{name}", "segment", "_segment_ref.cases", lambda: {"frames": given()[0]},
                 lambda: {"frames": np.ascontiguousarray(given()[0][::-1, :, ::-1])}, call, expected, _exact, _named))


# ----------------------------------------------------------------------------------------------------------- LPIPS, SSIM, VMAF, FVMD
def _lpips():
    R = importlib.import_module("_lpips_ref")
    case = R.BY_ID["min_31x31"]

    def call(t, box):
        from elvis_amd import lpips
        return {"score": lpips.lpips_device(t["a"], t["b"], box, rect=case.rect, order=case.order)}

    def prepare(dev):
        from elvis_amd import lpips
        return lpips.LpipsAlex(None, dev)

    def compare(got, want):
        err = R.rel(got["score"], want["score"])
        assert got["score"].dtype == np.float64 and err <= R.DEVICE_BAR, (got["score"], want, err)

    def inputs():
        a, b, _ = R.inputs(case)
        return {"a": a, "b": b}

    _split(Split("split_lpips_min_31x31", "lpips", "_lpips_ref.CASES", inputs,
                 lambda: {"a": _flip(inputs()["b"]), "b": np.ascontiguousarray(inputs()["a"][:, :, ::-1])}, call,
                 lambda inp: {"score": R.score(inp["a"], inp["b"], R.weights(), case.order, None, case.rect)}, compare, _named,
                 bound=lambda want: {"score": R.DEVICE_BAR * np.maximum(np.abs(want["score"]), 1e-6)}, prepare=prepare))


def _swapped_inputs(K, case, arrays, fn):
    """`fn()` with the statement module's cached inputs of `case` replaced by `arrays` for its length."""
    K.inputs(case)
    kept = K._INPUTS[case.id]
    K._INPUTS[case.id] = arrays
    try:
        return fn()
    finally:
        K._INPUTS[case.id] = kept


def _ssim():
    K = importlib.import_module("_qualitycases")
    case = K.BY_ID["batch_luma_reflect"]

    def call(t, box):
        from elvis_amd import _lib, metrics
        C1, C2 = case.constants
        rects = box
        return {"ssim": metrics.ssim_mean_device(
            t["a"], t["b"], K.window(case.window), source=_lib.SSIM_LUMA if case.source == "luma" else _lib.SSIM_CHANNELS,
            border=_lib.SSIM_REFLECT if case.border == "reflect" else _lib.SSIM_VALID, C1=C1, C2=C2, cov_norm=1.0,
            pad=_lib.SSIM_PAD_AUTO if case.pad is None else case.pad, scale=case.scale, masks=t.get("m"), rects=rects)}

    def prepare(dev):
        return None if case.rects is None else torch.tensor(case.rects, dtype=torch.int32, device=dev)

    def inputs():
        a, b, m = K.inputs(case)
        return {"a": a, "b": b} if m is None else {"a": a, "b": b, "m": m}

    def decoy():
        inp = inputs()
        out = {"a": _flip(inp["a"]), "b": np.ascontiguousarray(inp["b"][:, :, ::-1])}
        if "m" in inp:
            out["m"] = _turn(inp["m"])
        return out

    def expected(inp):
        return {"ssim": _swapped_inputs(K, case, (inp["a"], inp["b"], inp.get("m")), lambda: K.expected(case))}

    def compare(got, want):
        g, w = got["ssim"], want["ssim"]
        assert g.shape == w.shape and g.dtype == np.float64
        assert (np.abs(g - w) <= K.BAR).all(), (g, w)

    _split(Split("split_ssim_batch_luma_reflect", "ssim", "_qualitycases.CASES", inputs, decoy, call, expected, compare, _named,
                 syncs="the window is uploaded from pageable host memory, which waits for the stream",
                 bound=lambda want: {"ssim": np.full(want["ssim"].shape, K.BAR)}, prepare=prepare))


def _vmaf():
    K = importlib.import_module("_vmafcases")
    R = importlib.import_module("_vmaf_ref")
    cid = "shape_64x65"

    def call(t, box):
        from elvis_amd import vmaf
        feats = vmaf.vmaf_features_device(t["ref"], t["dis"])
        return {"features": feats, "scores": vmaf.vmaf_predict_device(feats, box)}

    def prepare(dev):
        from elvis_amd import vmaf
        model = vmaf.make_vmaf_model(0)
        model.on(dev)                     # the model and the filter tables are uploaded on first use: before the stall
        vmaf._device_tables(dev)
        return model

    def inputs():
        ref, dis, _, _ = K.inputs(cid)
        return {"ref": ref, "dis": dis}

    def expected(inp):
        from elvis_amd import vmaf
        feats = R.features(inp["ref"], inp["dis"], None, None)
        return {"features": feats, "scores": R.score(feats, vmaf.make_vmaf_model(0))}

    def compare(got, want):
        for name in ("features", "scores"):
            assert _rel(got[name], want[name]) <= R.BAR, (name, got[name], want[name])

    _split(Split(f"split_vmaf_{cid}", "vmaf", "_vmafcases.CASES", inputs,
                 lambda: {"ref": _flip(inputs()["dis"]), "dis": _flip(inputs()["ref"])}, call, expected, compare, _named,
                 bound=lambda want: {k: R.BAR * np.maximum(1.0, np.abs(want[k])) for k in ("features", "scores")}, prepare=prepare))


def _fvmd():
    K = importlib.import_module("_fvmdcases")
    R = importlib.import_module("_fvmd_ref")
    n, m, d = K.FRECHET[0]

    def call(t, box):
        from elvis_amd import fvmd
        gram, scalars = fvmd.gram_device(t["a"], t["b"])
        return {"gram": gram, "scalars": scalars, "distance": fvmd._frechet_tensor(t["a"], t["b"])}

    def inputs():
        a, b = K.frechet_rows(n, m, d)
        return {"a": a, "b": b}

    def decoy():
        a, b = K.frechet_rows(n, m, d)
        return {"a": np.ascontiguousarray(a[::-1] * 0.5 + 1.0), "b": np.ascontiguousarray(b[:, ::-1] * 2.0 - 1.0)}

    def expected(inp):
        gram, scalars = R.gram_parts(inp["a"], inp["b"])
        return {"gram": gram, "scalars": scalars, "distance": np.array([R.frechet(inp["a"], inp["b"])]),
                "scale": R.fd_scale(inp["a"], inp["b"])}

    def compare(got, want):
        assert _rel(got["gram"], want["gram"]) <= R.BAR and _rel(got["scalars"], want["scalars"]) <= R.BAR
        err = abs(float(got["distance"][0]) - float(want["distance"][0])) / max(1.0, want["scale"])
        assert err <= R.BAR, (got["distance"], want["distance"], err)

    def bound(want):
        out = {k: R.BAR * np.maximum(1.0, np.abs(want[k])) for k in ("gram", "scalars")}
        out["distance"] = np.array([R.BAR * max(1.0, want["scale"])])
        return out

    _split(Split(f"split_fvmd_frechet_{n}x{m}x{d}", "fvmd", "_fvmdcases.FRECHET", inputs, decoy, call, expected, compare,
                 lambda want: {k: want[k] for k in ("gram", "scalars", "distance")}, bound=bound))


# ----------------------------------------------------------------------------------------------------------- inpaint, tfill, complexity, shrink
def _inpaint():
    R = importlib.import_module("_inpaint_ref")
    name = "odd_random60"
    given = _once(lambda: R.cases()[name])

    def call(t, box):
        from elvis_amd import inpaint
        return {"out": inpaint.inpaint_device(t["frames"], t["masks"])}

    _split(Split(f"split_inpaint_{name}", "inpaint", "_inpaint_ref.cases", lambda: {"frames": given()[0], "masks": given()[1]},
                 lambda: {"frames": _flip(given()[0]), "masks": _turn(given()[1])}, call,
                 lambda inp: {"out": R.inpaint(inp["frames"], inp["masks"])}, _exact, _named,
                 syncs="the per-wave histogram comes down to size the fill launches"))


def _tfill():
    R = importlib.import_module("_tfill_ref")
    name = "search3"
    given = _once(lambda: R.cases()[name])

    def call(t, box):
        tf = importlib.import_module("elvis_amd.inpaint_temporal")
        out, left = tf.temporal_fill_device(t["frames"], t["masks"], **given()[2])
        return {"out": out, "left": left}

    def expected(inp):
        out, left = R.temporal_fill(inp["frames"], inp["masks"], **given()[2])
        return {"out": out, "left": left}

    _split(Split(f"split_tfill_{name}", "tfill", "_tfill_ref.cases", lambda: {"frames": given()[0], "masks": given()[1]},
                 lambda: {"frames": _flip(given()[0]), "masks": _turn(given()[1])}, call, expected, _exact, _named))


def _complexity():
    R = importlib.import_module("_complexity_ref")
    case = R.BY_ID["named_b16_rgb_prev"]

    def call(t, box):
        from elvis_amd import complexity
        sc, tc = complexity.block_complexity_device(t["frames"], case.block, case.order, prev=t["prev"])
        return {"sc": sc, "tc": tc}

    def inputs():
        frames, prev = R.inputs(case)
        return {"frames": frames, "prev": prev}

    def expected(inp):
        sc, tc = R.complexity(inp["frames"], case.block, case.order, inp["prev"])
        return {"sc": sc, "tc": tc}

    def compare(got, want):
        assert R.within_bar(got["sc"], want["sc"]) and R.within_bar(got["tc"], want["tc"]), (R.worst(got["sc"], want["sc"]),
                                                                                             R.worst(got["tc"], want["tc"]))

    _split(Split(f"split_complexity_{case.id}", "complexity", "_complexity_ref.NAMED", inputs,
                 lambda: {"frames": np.ascontiguousarray(inputs()["frames"][::-1, :, ::-1]), "prev": np.ascontiguousarray(255 - inputs()["prev"][::-1])},
                 call, expected, compare, _named, bound=lambda want: {k: R.BAR * np.maximum(1.0, np.abs(want[k])) for k in ("sc", "tc")}))


def _shrink():
    def call(t, box):
        from elvis_amd import shrink
        _, _, b, amount = D._shrink_inputs()
        out, mask, src_of = shrink.shrink_topk_device(t["frames"], t["scores"], b, amount)
        back, full = shrink.stretch_device(out, mask, b, "flat", fullres_mask=True)
        return {"out": out, "mask": mask, "src_of": src_of, "back": back, "full": full}

    def inputs():
        frames, scores, _, _ = D._shrink_inputs()
        return {"frames": frames, "scores": scores}

    def expected(inp):
        _, _, b, amount = D._shrink_inputs()
        return D.shrink_topk_statement(inp["frames"], inp["scores"], b, amount)

    _split(Split("split_shrink_topk_stretch_40x104_b8", "shrink", "_dirtycases._shrink_inputs", inputs,
                 lambda: {"frames": _flip(inputs()["frames"]), "scores": _turn(inputs()["scores"])}, call, expected, _exact, _named))


# ----------------------------------------------------------------------------------------------------------- the codecs
def _png_write():
    R = importlib.import_module("_png_ref")
    case = _once(lambda: R.CASES[R.CASE_IDS.index("content-diag-fadaptive")])

    def call(t, box):
        from elvis_amd import png
        c = case()
        return {f"file{i}": f for i, f in enumerate(png.encode_png_device(t["frames"], c.order, c.filt, c.segment_rows))}

    def expected(inp):
        c = case()
        return {f"file{i}": R.encode(f, c.order, c.filt, c.segment_rows).file for i, f in enumerate(inp["frames"])}

    _split(Split("split_png_write_diag_adaptive", "png_write", "_png_ref.CASES", lambda: {"frames": case().frames()},
                 lambda: {"frames": _flip(case().frames())}, call, expected, _exact, _named,
                 syncs="the segment statistics come down to size the output"))


def _png_read():
    """The reader takes files from the host, so its split case is the round trip: the device writer's files of the clip
    through the device reader.  A PNG is lossless: the statement is the clip, and PIL's decoding of the statement's file."""
    R = importlib.import_module("_png_ref")
    case = _once(lambda: R.CASES[R.CASE_IDS.index("content-diag-fadaptive")])

    def call(t, box):
        from elvis_amd import png
        c = case()
        files = png.encode_png_device(t["frames"], c.order, c.filt, c.segment_rows)
        return {"pixels": png.decode_png_device(files, t["frames"].device, c.order, t["frames"].shape[3])}

    def expected(inp):
        c = case()
        back = np.stack([R.decode_with_pil(R.encode(f, c.order, c.filt, c.segment_rows).file, c.order) for f in inp["frames"]])
        assert np.array_equal(back.reshape(inp["frames"].shape), inp["frames"])
        return {"pixels": inp["frames"]}

    _split(Split("split_png_read_round_trip", "png_read", "_png_ref.CASES + png.decode_png_device", lambda: {"frames": case().frames()},
                 lambda: {"frames": _flip(case().frames())}, call, expected, _exact, _named,
                 syncs="the writer's statistics and the reader's status words come down"))


def _jpeg_case(W):
    return next(c for c in W.cases() if (c.w, c.h) == (53, 37) and c.sampling == "420" and c.kind == "noise")


def _jpeg_write():
    W = importlib.import_module("_jpeg_write_ref")
    case = _once(lambda: _jpeg_case(W))

    def call(t, box):
        from elvis_amd import jpeg_write
        c = case()
        return {"file0": jpeg_write.encode_jpeg_device(t["frames"], "rgb", c.quality, c.subsampling)[0]}

    def expected(inp):
        c = case()
        return {"file0": W.encode(inp["frames"][0], c.quality, c.subsampling, "rgb").data}

    _split(Split("split_jpeg_write_37x53_420", "jpeg_write", "_jpeg_write_ref.cases", lambda: {"frames": case().frame()[None]},
                 lambda: {"frames": _flip(case().frame()[None])}, call, expected, _exact, _named,
                 syncs="the bit counts and the segment sizes come down between the passes"))


def _jpeg_read():
    """The reader takes files from the host, so its split case is the round trip (`jpeg_roundtrip_device`): the statement's
    decoding of the statement's file, restart interval of one MCU row so that the reader decodes segments side by side."""
    R = importlib.import_module("_jpeg_ref")
    S = importlib.import_module("_jpeg_restart_ref")
    W = importlib.import_module("_jpeg_write_ref")
    case = _once(lambda: _jpeg_case(W))

    def call(t, box):
        from elvis_amd import jpeg_write
        c = case()
        pixels, nbytes = jpeg_write.jpeg_roundtrip_device(t["frames"], c.quality, c.subsampling, "rgb", restart_rows=1)
        return {"pixels": pixels, "bytes": nbytes}

    def expected(inp):
        c = case()
        data = S.encode(inp["frames"][0], c.quality, c.subsampling, "rgb", restart_rows=1).data
        return {"pixels": R.decode(data, "rgb").pixels[None], "bytes": np.array([len(data)], np.int64)}

    _split(Split("split_jpeg_round_trip_37x53_420", "jpeg", "_jpeg_restart_ref.encode + _jpeg_ref.decode", lambda: {"frames": case().frame()[None]},
                 lambda: {"frames": _flip(case().frame()[None])}, call, expected, _exact, lambda want: {"pixels": want["pixels"]},
                 syncs="the writer's sizes and the reader's status words come down"))


def _i420():
    F = importlib.import_module("_handoff_ref")
    R = importlib.import_module("_i420_in_ref")
    shapes = {"odd": (3, 6, 18), "wide": (2, 18, 66)}

    def frames(shape):
        n, h, w = shape
        return np.random.default_rng(1000 * h + w + n).integers(0, 256, (n, h, w, 3), dtype=np.uint8)

    def call(t, box):
        from elvis_amd import handoff
        got = {}
        for name in shapes:
            planes = handoff.rgb_to_i420_device(t[name], "rgb")
            got[f"planes_{name}"] = planes
            got[f"back_{name}"] = handoff.i420_to_rgb_device(planes, "bgr")
        return got

    def expected(inp):
        want = {}
        for name in shapes:
            planes = F.rgb_to_i420(inp[name], "rgb")
            want[f"planes_{name}"] = planes
            want[f"back_{name}"] = R.i420_to_rgb(planes, "bgr")
        return want

    _split(Split("split_i420_both_ways", "i420", "_handoff_ref + _i420_in_ref", lambda: {k: frames(s) for k, s in shapes.items()},
                 lambda: {k: _flip(frames(s)) for k, s in shapes.items()}, call, expected, _exact, _named))


# ----------------------------------------------------------------------------------------------------------- per-block families
def _blocks():
    R = importlib.import_module("_blockref")
    cid = "lanczos_c3_b8"
    case = _once(lambda: next(c for c in R.CASES if c.id == cid))

    def call(t, box):
        from elvis_amd import classical
        return {"out": classical.lanczos_restore_device(t["frames"], t["levels"], case().block)}

    def inputs():
        frames, m = R.inputs(case())
        return {"frames": frames, "levels": m}

    _split(Split(f"split_blocks_{cid}", "blocks", "_blockref.CASES", inputs,
                 lambda: {"frames": _flip(inputs()["frames"]), "levels": _turn(inputs()["levels"])}, call,
                 lambda inp: {"out": R.lanczos_ref(inp["frames"], inp["levels"], case().block)}, _exact, _named))


def _presley():
    R = importlib.import_module("_presley_degrade_ref")
    b = 8

    def call(t, box):
        from elvis_amd import degrade
        return {"out": degrade.degrade_scale_device(t["frames"], t["maps"], b)}

    def inputs():
        frames, maps = D.presley_given("scale", b)
        return {"frames": frames, "maps": maps}

    _split(Split("split_presley_scale_b8", "presley", "_dirtycases.presley_given", inputs,
                 lambda: {"frames": _flip(inputs()["frames"]), "maps": _turn(inputs()["maps"])}, call,
                 lambda inp: {"out": R.scale_clip(inp["frames"], inp["maps"], b)}, _exact, _named))


def _enhance():
    E = importlib.import_module("_enhance_ref")
    name = "tile16x64_plus1"
    hs, ws, hd, wd = E.RESIZE_CASES[name]

    def call(t, box):
        from elvis_amd import enhance
        return {"out": enhance.resize_lanczos4_device(t["src"], hd, wd)}

    _split(Split(f"split_enhance_resize_{name}", "enhance", "_enhance_ref.RESIZE_CASES", lambda: {"src": E.resize_inputs(name, 3, "random")},
                 lambda: {"src": _flip(E.resize_inputs(name, 3, "random"))}, call, lambda inp: {"out": E.resize(inp["src"], hd, wd)}, _exact,
                 _named))


def _resize():
    R = importlib.import_module("_resize_ref")
    hs, ws, hd, wd = R.FRACTIONAL["7x10->3x4"]
    up = (9, 13)

    def call(t, box):
        from elvis_amd import intake
        return {"area": intake.resize_area_device(t["src"], hd, wd), "nearest": intake.resize_nearest_device(t["src"], *up)}

    _split(Split("split_resize_7x10", "resize", "_resize_ref.FRACTIONAL", lambda: {"src": R.frames(hs, ws, 3, 3)},
                 lambda: {"src": _flip(R.frames(hs, ws, 3, 3))}, call,
                 lambda inp: {"area": R.resize_area_u8(inp["src"], hd, wd), "nearest": R.resize_nearest_u8(inp["src"], *up)}, _exact, _named))


# ----------------------------------------------------------------------------------------------------------- the model kernels
def _conv():
    """tests/_convref.py's `f16_16_ks1_a0` (halo f16, 1x1, cin 48, cout 3) as tests/test_gpu_conv_matrix.py runs it: the
    weights are the case's, packed before the stall; the activation is the argument."""
    R = importlib.import_module("_convref")
    cid = "f16_16_ks1_a0"
    case = _once(lambda: next(c for c in R.CASES if c.id == cid))

    def weights():
        import math
        c = case()
        assert c.kind == "conv" and c.dt == "f16" and not (c.cin2 or c.prologue or c.residual or c.upsample)
        g = torch.Generator().manual_seed(1000 + c.seed)
        wt = torch.randn(c.cout, c.cin, c.ksize, c.ksize, generator=g) / math.sqrt(c.ksize * c.ksize * c.cin)
        return wt, torch.randn(c.cout, generator=g) * 0.1

    def x_of(seed):
        c = case()
        return torch.randn(c.n, c.h, c.w, c.cin, generator=torch.Generator().manual_seed(seed)).half().numpy()

    def prepare(dev):
        from elvis_amd import ops
        wt, b = weights()
        return ops.PackedConv(wt, b, torch.float16, dev, case().cin, 0)

    def call(t, box):
        from elvis_amd import ops
        c = case()
        x = t["x"]
        if ops.pitch_for(c.cin) != c.cin:
            raise AssertionError("the case's input has pad channels; pick one without")
        y = box(ops.Act(x, c.cin), None, stride=c.stride, pad=c.pad, act=c.act)
        return {"y": y.t[..., :c.cout], "pads": y.t[..., c.cout:]}

    def expected(inp):
        c = case()
        wt, b = weights()
        x64 = torch.from_numpy(inp["x"]).double().permute(0, 3, 1, 2)
        pad = (c.ksize // 2) if c.pad is None else c.pad
        return R.conv_ref(x64, wt.half().double(), b.double(), None, ksize=c.ksize, stride=c.stride, pad=pad, act=c.act, out_f16=True)

    def compare(got, want):
        y = torch.from_numpy(got["y"].astype(np.float64)).permute(0, 3, 1, 2)
        ok, worst, at = R.tier1(y, want)
        assert ok, f"{cid}: tier 1 fails at {at} (worst {worst:.3f})"
        assert got["pads"].size == 0 or (got["pads"] == 0).all(), f"{cid}: pad channels not zeroed"

    _split(Split(f"split_conv_{cid}", "conv", "_convref.CASES", lambda: {"x": x_of(5)}, lambda: {"x": x_of(6)}, call, expected, compare,
                 lambda want: {"y": want.ref.numpy()}, bound=lambda want: {"y": want.bound().numpy()}, prepare=prepare))


def _swin():
    """tests/test_gpu_model_kernels_matrix.py::_run_swin's PROJ + MLP call on the first mode-2 case of tests/_modelref.py:
    the block's weights are the case's, packed before the stall; the attention output x and the residual stream y are
    the arguments."""
    R = importlib.import_module("_modelref")
    case = _once(lambda: next(c for c in R.CASES if c.op == "swin" and c.mode == 2))
    eps = float(np.float32(1e-5))

    def weights():
        import math
        c = case()
        g = torch.Generator().manual_seed(3000 + c.seed)
        rn = lambda *s: torch.randn(*s, generator=g)
        C, n1 = c.c, c.n1
        return dict(gam=torch.rand(C, generator=g) + 0.5, bet=rn(C) * 0.2, w1=rn(n1, C) / math.sqrt(C), b1=rn(n1) * 0.1,
                    w2=rn(C, n1) / math.sqrt(n1), b2=rn(C) * 0.1, wp=rn(C, C) / math.sqrt(C), bp=rn(C) * 0.1)

    def tokens(seed):
        c = case()
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(c.tokens, c.c, generator=g)
        y = c.offset + c.spread * torch.randn(c.tokens, c.c, generator=g) + 0.5 * torch.randn(c.tokens, 1, generator=g)
        return {"x": x.half().numpy(), "y": y.half().numpy()}

    def prepare(dev):
        from elvis_amd import ops
        w = weights()
        return ops.SwinFused(w["gam"], w["bet"], w["w1"], w["b1"], w["w2"], w["b2"], proj_w=w["wp"], proj_b=w["bp"], device=dev)

    def call(t, sf):
        from elvis_amd._lib import check, lib, ptr, stream_handle
        c = case()
        x, y = t["x"], t["y"]
        out = torch.zeros((c.tokens, c.c), dtype=torch.float16, device=x.device)
        check(lib().elvis_swin_proj_mlp(ptr(x), ptr(y), ptr(out), ptr(sf.packed), ptr(sf.bp), ptr(sf.b1), ptr(sf.b2), ptr(sf.gamma),
                                        ptr(sf.beta), c.tokens, c.c, c.n1, c.c, c.c, c.c, eps, stream_handle(x.device)), x.device)
        return {"out": out}

    def expected(inp):
        w = weights()
        h16 = lambda a: a.half().double()
        f64 = lambda a: a.float().double()
        x, y = torch.from_numpy(inp["x"]).double(), torch.from_numpy(inp["y"]).double()
        return R.swin_ref(2, x, f64(w["gam"]), f64(w["bet"]), h16(w["w1"]), f64(w["b1"]), h16(w["w2"]), f64(w["b2"]), y=y, wp=h16(w["wp"]),
                          bp=f64(w["bp"]), eps=eps)

    def compare(got, want):
        ok, worst, at = R.tier1(torch.from_numpy(got["out"].astype(np.float64)), want)
        assert ok, f"swin: tier 1 fails at {tuple(int(i) for i in at)} (worst {worst:.3f})"

    _split(Split("split_swin_proj_mlp", "swin", "_modelref.CASES", lambda: tokens(11), lambda: tokens(12), call, expected, compare,
                 lambda want: {"out": want.ref.numpy()}, bound=lambda want: {"out": want.bound().numpy()}, prepare=prepare))


def _vq_index():
    """ops.vq_index and the indexed search on the codes of tests/_vq_grid_ref.py's `p257` (257 codes, 257 pixels: two
    workgroups, the second with one pixel), against the first-minimum scan `_normref.vq_ref`.  The index is built inside
    the call: it reads the codebook back, so the call waits for the stream."""
    N = importlib.import_module("_normref")
    V = importlib.import_module("_vq_grid_ref")

    def arrays(cid):
        cb, z = V.BY_ID[cid].arrays()
        zp = np.zeros((1, 1, z.shape[0], 8), np.float32)
        zp[0, 0, :, :3] = z
        return {"z": zp, "cb": np.array(cb)}

    def call(t, box):
        from elvis_amd import ops
        index = ops.vq_index(t["cb"])
        assert index is not None
        zq, idx = ops.vq_nearest(ops.Act(t["z"], 3), t["cb"], want_idx=True, index=index)
        return {"idx": idx, "zq": zq.t}

    def expected(inp):
        idx, zq = N.vq_ref(inp["z"][0, 0, :, :3], inp["cb"])
        out = np.zeros(inp["z"].shape, np.float32)
        out[0, 0, :, :3] = zq
        return {"idx": idx.reshape(1, 1, -1), "zq": out}

    def compare(got, want):
        assert np.array_equal(got["idx"], want["idx"]), "the indices differ from the first-minimum scan"
        assert N.bits_equal(got["zq"], want["zq"]), "zq differs from the stored codebook[idx]"

    _split(Split("split_vq_index_p257", "vq_index", "_vq_grid_ref.CASES + _normref.vq_ref", lambda: arrays("p257"),
                 lambda: {"z": arrays("p257")["z"][:, :, ::-1].copy() * np.float32(0.5), "cb": np.ascontiguousarray(arrays("p257")["cb"][::-1])},
                 call, expected, compare, _named, syncs="the index build reads the codebook back and waits for its own upload"))


def _gn_fused():
    """ops.groupnorm_affine on one buffer of fused partials (`elvis_gn_partials_affine`), against the bit-exact model
    tests/_gn_fused_model.py: c = 64, 32 groups, 7 tiles - the span of 16 with a ragged tail."""
    M = importlib.import_module("_gn_fused_model")
    c, groups, tiles, n = 64, 32, 7, M.N_IMAGES

    def params():
        gam, bet, _, _ = M.params(c, False)
        return gam, bet

    def prepare(dev):
        gam, bet = params()
        return torch.from_numpy(np.array(gam)).to(dev), torch.from_numpy(np.array(bet)).to(dev)

    def call(t, box):
        from elvis_amd import ops
        p = t["partials"]
        x = ops.Act(torch.zeros((n, 16, 16 * tiles, c), dtype=torch.float16, device=p.device), c, p.view(n * tiles, c, 2))
        pa, pb = ops.groupnorm_affine([x], box[0], box[1], groups, M.EPS)
        return {"pa": pa, "pb": pb}

    def expected(inp):
        gam, bet = params()
        pa, pb = M.model(inp["partials"], gam, bet, None, None, tiles * 256, groups, M.EPS)
        return {"pa": pa.reshape(n, c), "pb": pb.reshape(n, c)}

    def compare(got, want):
        for k in ("pa", "pb"):
            assert got[k].dtype == np.float32 and np.array_equal(got[k].view(np.int32), np.asarray(want[k], np.float32).view(np.int32)), \
                f"{k}: differs from the model's bits"

    _split(Split("split_gn_fused_c64_t7", "gn_fused", "_gn_fused_model", lambda: {"partials": np.array(M.partials(n, tiles, c, c // groups))},
                 lambda: {"partials": np.ascontiguousarray(M.partials(n, tiles, c, c // groups)[::-1, ::-1])}, call, expected, compare, _named,
                 prepare=prepare))


# ----------------------------------------------------------------------------------------------------------- masks, pipeline
def _quality():
    K = importlib.import_module("_qualitycases")
    case = K.BY_ID["apply_c3_p17_off0_inv"]

    def call(t, box):
        from elvis_amd import metrics
        return {"out": metrics.apply_mask_device(t["frames"], t["mask"], case.invert)}

    def inputs():
        frames, mask = K.inputs(case)
        return {"frames": frames, "mask": mask}

    _split(Split(f"split_quality_{case.id}", "quality", "_qualitycases.CASES", inputs,
                 lambda: {"frames": _flip(inputs()["frames"]), "mask": np.where(inputs()["mask"] != 0, 0, 255).astype(np.uint8)}, call,
                 lambda inp: {"out": _swapped_inputs(K, case, (inp["frames"], inp["mask"]), lambda: K.expected(case))}, _exact, _named))


def _pipeline():
    f0, nsel = D.PLANE_MERGE[:2]

    def call(t, box):
        from elvis_amd import ops
        return {"out": ops.plane_merge(t["frames"], ops.Act(t["res"], 1), f0, nsel)}

    def pair(seed):
        frames, res = D.plane_merge_given(seed)
        return {"frames": frames, "res": res}

    _split(Split("split_pipeline_plane_merge_9x13", "pipeline", "_dirtycases.plane_merge_statement", lambda: pair(33), lambda: pair(34), call,
                 lambda inp: D.plane_merge_statement(inp["frames"], inp["res"]), _exact, _named))


for _make in (_segment, _lpips, _ssim, _vmaf, _fvmd, _inpaint, _tfill, _complexity, _shrink, _png_write, _png_read, _jpeg_write, _jpeg_read,
              _i420, _blocks, _presley, _enhance, _resize, _conv, _swin, _vq_index, _gn_fused, _quality, _pipeline):
    _make()

FAMILIES = ("segment", "lpips", "ssim", "vmaf", "fvmd", "inpaint", "tfill", "complexity", "shrink", "png_write", "png_read", "jpeg", "i420",
            "blocks", "presley", "enhance", "conv", "swin", "quality", "pipeline", "jpeg_write", "resize", "vq_index", "gn_fused")


# ----------------------------------------------------------------------------------------------------------- (a): further surfaces
def _jpeg_forms():
    """The JPEG writer's restart, ROI and optimised forms at their 37 x 53 cases, one frame each."""
    for form, module, extra in (("restart", "_jpeg_restart_ref", lambda c: c.restart),
                                ("roi", "_jpeg_roi_ref", lambda c: dict(roi_levels=c.levels()[None], roi_block_size=c.B)),
                                ("opt", "_jpeg_opt_ref", lambda c: dict(c.restart, optimize=True))):
        M = importlib.import_module(module)
        pick = _once(lambda M=M, form=form: next(c for c in M.cases() if {c.w, c.h} == {37, 53} and c.sampling == "420" and
                                                  (form != "roi" or c.map_kind == "random")))

        def run(dev, M=M, pick=pick, extra=extra):
            from elvis_amd import jpeg_write
            c = pick()
            frames = torch.from_numpy(np.ascontiguousarray(c.frame()[None])).to(dev)
            return {"file0": jpeg_write.encode_jpeg_device(frames, "rgb", c.quality, c.subsampling, **extra(c))[0]}

        _case(Case(f"jpeg_write_{form}_37x53_420", "jpeg_write", (1, 37, 53), f"{module}.cases", run,
                   lambda M=M, pick=pick: {"file0": M.encoded(pick().name).data}, _exact))


def _png_rle():
    S = importlib.import_module("_png_rle_ref")
    index = _once(lambda: S.CASE_IDS.index("offset-1"))

    def run(dev):
        from elvis_amd import png
        c = S.CASES[index()]
        frames = torch.from_numpy(np.ascontiguousarray(c.frames())).to(dev)
        return {f"file{i}": f for i, f in enumerate(png.encode_png_device(frames, c.order, c.filt, c.segment_rows, deflate="rle"))}

    _case(Case("png_write_rle_17x63", "png_write", (3, 17, 63), "_png_rle_ref.CASES", run,
               lambda: {f"file{i}": e.file for i, e in enumerate(S.expected(index()))}, _exact))


def _matrix_runner(cid, family, test_module, ref_module, pick):
    """A case of one of the kernel matrices through that matrix's own runner (the operands are seeded by the case, the
    reference is float64 with the family's tier-1 bound), as tests/_dirtycases.py's `swin_block_pack` does."""
    box = {}

    def run(dev):
        T, R = importlib.import_module(test_module), importlib.import_module(ref_module)
        case = pick(R)
        name, y, b = T.RUN[case.op](case, dev)
        assert name == case.expect, (cid, name)
        box.update(ref=b, R=R)
        return {"y": y}

    def compare(got, want):
        ok, worst, at = box["R"].tier1(torch.from_numpy(got["y"]), want)
        assert ok, f"{cid}: tier 1 fails at {tuple(int(i) for i in at)} (worst {worst:.3f})"

    _case(Case(cid, family, (0, 0, 0), f"{ref_module}.CASES", run, lambda: box["ref"], compare))


def _glue_runner(cid, op):
    """A case of tests/_glueref.py through tests/test_gpu_glue_matrix.py's runner, which compares with the reference
    itself (sentinels, two fills); it is given the current stream, as that test gives it."""
    def run(dev):
        from elvis_amd._lib import stream_handle
        T, R = importlib.import_module("test_gpu_glue_matrix"), importlib.import_module("_glueref")
        case = next(c for c in R.CASES if c.op == op)
        T.RUN[op](case, dev, stream_handle(dev))
        return {"compared_by_the_runner": np.array([1])}

    _case(Case(cid, "glue", (0, 0, 0), "_glueref.CASES", run, lambda: {"compared_by_the_runner": np.array([1])}, _exact))


def _vq_scan():
    N = importlib.import_module("_normref")
    V = importlib.import_module("_vq_grid_ref")

    def given():
        cb, z = V.BY_ID["p257"].arrays()
        zp = np.zeros((1, 1, z.shape[0], 8), np.float32)
        zp[0, 0, :, :3] = z
        return zp, np.array(cb)

    def run(dev):
        from elvis_amd import ops
        zp, cb = given()
        zq, idx = ops.vq_nearest(ops.Act(torch.from_numpy(zp).to(dev), 3), torch.from_numpy(cb).to(dev), want_idx=True)
        return {"idx": idx, "zq": zq.t[..., :3]}

    def expected():
        zp, cb = given()
        idx, zq = N.vq_ref(zp[0, 0, :, :3], cb)
        return {"idx": idx.reshape(1, 1, -1), "zq": zq.reshape(1, 1, -1, 3)}

    _case(Case("vq_nearest_scan_p257", "vq_index", (0, 0, 0), "_vq_grid_ref.CASES + _normref.vq_ref", run, expected, _exact))


def _convert_act():
    N = importlib.import_module("_normref")

    def run(dev):
        from elvis_amd._lib import F16, F32, check, lib, ptr, stream_handle
        a = N.f32_to_f16_inputs()
        xd = torch.from_numpy(np.array(a)).to(dev)
        out = torch.zeros(a.size, dtype=torch.float16, device=dev)
        check(lib().elvis_convert_act(ptr(xd), F32, ptr(out), F16, a.size // 8, 8, stream_handle(dev)), dev)
        return {"out": out}

    def compare(got, want):
        g = got["out"]
        assert g.shape == want.shape and g.dtype == np.float16
        assert ((g.view(np.uint16) == want.view(np.uint16)) | (np.isnan(g) & np.isnan(want))).all()

    _case(Case("convert_act_f32_to_f16", "conv", (0, 0, 0), "_normref.f32_to_f16_inputs", run, lambda: N.convert_ref(N.f32_to_f16_inputs(), True),
               compare))


_jpeg_forms()
_png_rle()
_matrix_runner("norm_affine_act", "conv", "test_gpu_norm_misc_matrix", "_normref", lambda R: next(c for c in R.CASES if c.op == "affine_act"))
_matrix_runner("swin_mlp", "swin", "test_gpu_model_kernels_matrix", "_modelref", lambda R: next(c for c in R.CASES if c.op == "swin" and c.mode == 1))
_glue_runner("glue_select_levels", "select")
_glue_runner("glue_sse", "sse")
_vq_scan()
_convert_act()


def all_cases():
    """Every case test (a) runs: the 62 of tests/_dirtycases.py and the ones above."""
    out = dict(D.CASES)
    out.update(CASES)
    return out


# ----------------------------------------------------------------------------------------------------------- the ledger
# entry point -> the ids of cases whose recorded run calls it (tests/test_gpu_streams.py checks every claim), or why none does
REACHED = {
    "elvis_recompose_u8": ("pipeline_realesrgan_frames_32x48",),
    "elvis_area_downscale_u8": ("pipeline_realesrgan_frames_32x48",),
    "elvis_blend_u8": ("pipeline_tiler_blend_64x96",),
    "elvis_select_levels_u8": ("glue_select_levels",),
    "elvis_tile_accumulate_f32": ("pipeline_tiler_blend_64x96",),
    "elvis_tile_normalize_u8": ("pipeline_tiler_blend_64x96",),
    "elvis_sse_u8": ("glue_sse",),
    "elvis_block_ssim_u8": ("quality_block_ssim_50x70_b12",),
    "elvis_mask_bbox_u8": ("quality_bbox_n3_5x7_empty_middle",),
    "elvis_apply_mask_u8": ("quality_apply_c3_p17_off0_inv", "split_quality_apply_c3_p17_off0_inv",),
    "elvis_ssim_mean_f64": ("ssim_batch_channels_reflect", "split_ssim_batch_luma_reflect",),
    "elvis_u8_to_float": ("pipeline_single4x_host_64x96",),
    "elvis_float_to_u8": ("pipeline_single4x_host_64x96",),
    "elvis_conv_pack_weights": ("conv_f16_16_ks3_a0", "split_conv_f16_16_ks1_a0",),
    "elvis_conv2d": ("conv_f16_16_ks3_a0", "split_conv_f16_16_ks1_a0",),
    "elvis_gn_partials_to_sums": ("pipeline_single4x_host_64x96",),
    "elvis_groupnorm_sums": ("pipeline_single4x_host_64x96",),
    "elvis_groupnorm_affine": ("pipeline_single4x_host_64x96",),
    "elvis_gn_partials_affine": ("pipeline_single4x_host_64x96", "split_gn_fused_c64_t7",),
    "elvis_affine_act": ("norm_affine_act",),
    "elvis_layernorm": ("pipeline_single4x_host_64x96",),
    "elvis_swin_pack_weights": ("swin_mlp",),
    "elvis_swin_mlp": ("swin_mlp",),
    "elvis_swin_ln_linear": ("pipeline_single4x_host_64x96",),
    "elvis_swin_pack_proj_mlp": ("swin_block_pack", "split_swin_proj_mlp",),
    "elvis_swin_proj_mlp": ("pipeline_single4x_host_64x96", "split_swin_proj_mlp",),
    "elvis_window_attention": ("pipeline_single4x_host_64x96",),
    "elvis_bicubic_upsample": ("pipeline_single4x_host_64x96",),
    "elvis_vq_nearest": ("vq_nearest_scan_p257",),
    "elvis_vq_index_build": ("split_vq_index_p257",),
    "elvis_vq_nearest_indexed": ("pipeline_single4x_host_64x96", "split_vq_index_p257",),
    "elvis_pad_reflect_axpy": ("pipeline_single4x_host_64x96",),
    "elvis_crop_copy": ("pipeline_single4x_host_64x96",),
    "elvis_convert_act": ("convert_act_f32_to_f16",),
    "elvis_degrade_downsample_u8": ("blocks_downsample_b8_c1_n3",),
    "elvis_degrade_gaussian_u8": ("blocks_gaussian_b5_total64_n1_c1",),
    "elvis_degrade_dct_u8": ("blocks_dct_noise_c3",),
    "elvis_degrade_scale_u8": ("presley_scale_b8_whole_blocks", "split_presley_scale_b8",),
    "elvis_degrade_gaussian_fx_u8": ("presley_gaussian_b8_whole_blocks",),
    "elvis_rgb_to_i420_u8": ("i420_both_ways", "split_i420_both_ways",),
    "elvis_i420_to_rgb_u8": ("i420_both_ways", "split_i420_both_ways",),
    "elvis_classical_lanczos_u8": ("blocks_lanczos_c3_b8", "split_blocks_lanczos_c3_b8",),
    "elvis_classical_unsharp_u8": ("blocks_unsharp_c3_b8_halo0",),
    "elvis_temporal_blend_u8": ("blocks_blend_five_frames_tb1",),
    "elvis_block_gather_u8": ("shrink_passes_rows_40x104_b8", "split_shrink_topk_stretch_40x104_b8",),
    "elvis_shrink_select_topk": ("shrink_topk_stretch_40x104_b8", "split_shrink_topk_stretch_40x104_b8",),
    "elvis_shrink_select_passes": ("shrink_passes_rows_40x104_b8",),
    "elvis_stretch_index": ("shrink_passes_rows_40x104_b8", "split_shrink_topk_stretch_40x104_b8",),
    "elvis_inpaint_prepare": ("inpaint_blocks_44x61_b8", "split_inpaint_odd_random60",),
    "elvis_inpaint_fill": ("inpaint_blocks_44x61_b8", "split_inpaint_odd_random60",),
    "elvis_tfill": ("tfill_ragged_33x49_c3", "split_tfill_search3",),
    "elvis_segment_foreground_u8": ("segment_21x23_n1", "split_segment_21x23_n3",),
    "elvis_block_complexity_f64": ("complexity_named_b16_rgb_prev", "split_complexity_named_b16_rgb_prev",),
    "elvis_lpips_stem_u8": ("lpips_min_31x31", "split_lpips_min_31x31",),
    "elvis_lpips_conv5_f32": ("lpips_min_31x31", "split_lpips_min_31x31",),
    "elvis_lpips_maxpool_f32": ("lpips_min_31x31", "split_lpips_min_31x31",),
    "elvis_lpips_distance_f64": ("lpips_distance_tap0", "split_lpips_min_31x31",),
    "elvis_vmaf_luma_u8": ("vmaf_luma_rect_odd_masked",),
    "elvis_vmaf_features_f64": ("vmaf_pass_64x64_n5", "split_vmaf_shape_64x65",),
    "elvis_vmaf_predict_f64": ("vmaf_pass_64x64_n5", "split_vmaf_shape_64x65",),
    "elvis_fvmd_pyramid_f64": ("fvmd_tracker_64x65_s10",),
    "elvis_fvmd_track_f64": ("fvmd_tracker_64x65_s10",),
    "elvis_fvmd_features_f64": ("fvmd_hist_axes_S10_B1",),
    "elvis_fvmd_gram_f64": ("fvmd_frechet_128x128x384", "split_fvmd_frechet_128x128x384",),
    "elvis_fvmd_singular_values_f64": ("fvmd_frechet_128x128x384", "split_fvmd_frechet_128x128x384",),
    "elvis_fvmd_finish_f64": ("fvmd_frechet_128x128x384", "split_fvmd_frechet_128x128x384",),
    "elvis_png_stats": ("png_write_diag_adaptive_33x65", "split_png_read_round_trip",),
    "elvis_png_pack": ("png_write_diag_adaptive_33x65", "split_png_read_round_trip",),
    "elvis_png_stats_rle": ("png_write_rle_17x63",),
    "elvis_png_pack_rle": ("png_write_rle_17x63",),
    "elvis_png_gather": ("jpeg_bad_between_good_17x33", "split_png_read_round_trip",),
    "elvis_png_inflate": ("jpeg_bad_between_good_17x33", "split_png_read_round_trip",),
    "elvis_png_unfilter": ("jpeg_bad_between_good_17x33", "split_png_read_round_trip",),
    "elvis_jpeg_entropy": ("jpeg_bad_between_good_17x33", "split_jpeg_round_trip_37x53_420",),
    "elvis_jpeg_idct": ("jpeg_bad_between_good_17x33", "split_jpeg_round_trip_37x53_420",),
    "elvis_jpeg_colour": ("jpeg_bad_between_good_17x33", "split_jpeg_round_trip_37x53_420",),
    "elvis_jpeg_fdct": ("jpeg_write_restart_37x53_420", "split_jpeg_round_trip_37x53_420",),
    "elvis_jpeg_fdct_roi": ("jpeg_write_roi_37x53_420",),
    "elvis_jpeg_bits": ("jpeg_write_roi_37x53_420", "split_jpeg_write_37x53_420",),
    "elvis_jpeg_pack": ("jpeg_write_roi_37x53_420", "split_jpeg_write_37x53_420",),
    "elvis_jpeg_stuff": ("jpeg_write_roi_37x53_420", "split_jpeg_write_37x53_420",),
    "elvis_jpeg_bits_rst": ("jpeg_write_restart_37x53_420", "split_jpeg_round_trip_37x53_420",),
    "elvis_jpeg_pack_rst": ("jpeg_write_restart_37x53_420", "split_jpeg_round_trip_37x53_420",),
    "elvis_jpeg_stuff_rst": ("jpeg_write_restart_37x53_420", "split_jpeg_round_trip_37x53_420",),
    "elvis_jpeg_tally": ("jpeg_write_opt_37x53_420",),
    "elvis_jpeg_bits_ftab": ("jpeg_write_opt_37x53_420",),
    "elvis_jpeg_pack_ftab": ("jpeg_write_opt_37x53_420",),
    "elvis_rrdb_conv3x3": ("enhance_tiles_pre_pad_RealESRGAN_x4plus_anime_6B",),
    "elvis_rrdb_input_u8": ("enhance_tiles_pre_pad_RealESRGAN_x4plus_anime_6B",),
    "elvis_srvgg_conv3x3": ("enhance_tiles_pre_pad_realesr-animevideov3",),
    "elvis_srvgg_tail": ("enhance_tiles_pre_pad_realesr-animevideov3",),
    "elvis_resize_lanczos4_u8": ("enhance_resize_tile16x64_plus1", "split_enhance_resize_tile16x64_plus1",),
    "elvis_sr_gather_tiles_u8": ("enhance_tiles_pre_pad_RealESRGAN_x4plus_anime_6B",),
    "elvis_sr_paste_tiles_u8": ("enhance_tiles_pre_pad_RealESRGAN_x4plus_anime_6B",),
    "elvis_resize_area_u8": ("split_resize_7x10",),
    "elvis_resize_nearest_u8": ("split_resize_7x10",),
    "elvis_dcnv2": ("pipeline_slot_host_dct_64x96",),
    "elvis_temporal_stack": ("pipeline_slot_host_dct_64x96",),
    "elvis_plane_merge": ("pipeline_plane_merge_9x13", "split_pipeline_plane_merge_9x13",),
}
