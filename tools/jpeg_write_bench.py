"""The device JPEG writer (csrc/jpeg_write.hip, elvis_amd/jpeg_write.py) on a resident 1080p clip.

    python tools/jpeg_write_bench.py [--frames 30] [--reps 10] [--height 1080] [--width 1920] [--out DIR]
                                     [--restart-rows R | --restart-mcus K] [--roi-levels none|zero|random] [--roi-block-size B]
                                     [--optimize] [--measure encode,roundtrip,writers,sizes,search,roi_table,optimize_split]

The clip is `synth.synth_clip`.  `--restart-rows` / `--restart-mcus` give the device writer a restart interval (PIL's
files of the comparison get the same one).  `--roi-levels zero|random` gives the `encode` and `search` measurements a map of
ROI levels on a grid of `--roi-block-size` (16) luma pixels: all 0, or uniform in 0..48.  `ELVIS_AMD_LIB` names another build of the library, for a comparison in one
session.  `--optimize` gives every measurement of the device writer `optimize=True`, a frame's own optimal Huffman tables
(PIL's quality-95 files of the comparison get `optimize=True` as well).  Prints one JSON line per measurement:

  encode      device time between events on the stream around `jpeg_write._encode_clip` - the four calls with their two
              small downloads in between - median of `reps` after a warm-up, per frame, with the bytes the algorithm
              needs (the clip read once, the scans written once) as a fraction of the HBM peak
  roundtrip   `jpeg_write.jpeg_roundtrip_device` - encode, the files down, the device reader's decode of them: a host clock
              around the call and a final synchronise (median, min, max), and in one more run device events around
              each C-ABI call of the writer and of the reader (the reader's entropy launch decodes a segment per lane)
  writers     a host clock from the resident clip to the files on disk: `jpeg_write.save_jpeg_frames_device` (encode, one
              download, write) against the path it replaces, the clip brought down and `frameio.save_frame` to `.jpg`
              per frame (PIL at its own quality 75); and PIL asked for the device writer's settings, quality 95 and
              4:2:0, for the like-for-like cost
  sizes       bytes per frame of the three
  search      `jpeg_write.jpeg_quality_for_bytes` for the bytes the clip has at quality 75: a host clock around the search and
              a final synchronise, the probes it made, and the same clock around one `encode_jpeg_device` at quality 95
  roi_table   bytes per frame and PSNR against the source of the round trip at quality 95 with a map of levels 0 / 12 / 24 on
              the 8-pixel grid, drawn as `synth.synth_level_maps` draws the benchmark's maps (shares 0.35 / 0.25 / 0.40 - its
              two deepest levels are one here - then the 5 x 5 majority filter), and of the uniform quality that the
              search finds for the same bytes
  optimize_split  what `optimize=True` adds to an encode, step by step on a clip whose coefficients are resident: the tally
              (device events around `elvis_jpeg_tally`), the download of the histograms, the table builder with the
              headers (`jpeg_optimal_tables` and the headers as `_encode_clip` makes them) and the upload of the code words (host clocks, each
              ended by a synchronise), medians of `reps`; beside them the whole encode with and without `optimize` and
              the bytes per frame of both
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elvis_amd import frameio, jpeg, jpeg_write, recompose, synth  # noqa: E402

HBM_PEAK_GBS = 8000.0


def report(**kw):
    print(json.dumps(kw), flush=True)


def host_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def call_events(fn):
    """Device events around every `elvis_jpeg_*` call that `fn` makes through jpeg_write.py and jpeg.py: {name: ms}."""
    from elvis_amd import _lib
    handle, marks = _lib.lib(), []

    class Timed:
        def __getattr__(self, name):
            real = getattr(handle, name)
            if not name.startswith("elvis_jpeg_") or name in ("elvis_jpeg_frame_blocks", "elvis_jpeg_segments"):
                return real

            def call(*args):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                rc = real(*args)
                b.record()
                marks.append((name, a, b))
                return rc
            return call

    saved = jpeg_write.lib, jpeg.lib
    jpeg_write.lib = jpeg.lib = lambda: Timed()
    try:
        fn()
    finally:
        jpeg_write.lib, jpeg.lib = saved
    torch.cuda.synchronize()
    ms = {}
    for name, a, b in marks:
        ms[name] = round(ms.get(name, 0.0) + a.elapsed_time(b), 4)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--out", default=None)
    ap.add_argument("--restart-rows", type=int, default=0)
    ap.add_argument("--restart-mcus", type=int, default=0)
    ap.add_argument("--roi-levels", choices=("none", "zero", "random"), default="none")
    ap.add_argument("--roi-block-size", type=int, default=16)
    ap.add_argument("--optimize", action="store_true")
    ap.add_argument("--measure", default="encode,roundtrip,writers,sizes")
    args = ap.parse_args()
    measure = set(args.measure.split(","))
    restart = (args.restart_rows, args.restart_mcus)
    restart_kw = {k: v for k, v in (("restart_rows", args.restart_rows), ("restart_mcus", args.restart_mcus)) if v}
    pil_kw = {k: v for k, v in (("restart_marker_rows", args.restart_rows), ("restart_marker_blocks", args.restart_mcus)) if v}
    setting = dict(restart_kw, library=os.environ.get("ELVIS_AMD_LIB") or "built")
    opt_kw = {"optimize": True} if args.optimize else {}          # the default calls are the ones they always were
    setting.update(opt_kw)
    pil_kw.update(opt_kw)
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    n, h, w = args.frames, args.height, args.width
    clip = torch.from_numpy(np.ascontiguousarray(synth.synth_clip(7, n, h, w)[..., ::-1])).to(dev)     # BGR, as the drivers hold it
    out = args.out or tempfile.mkdtemp(prefix="jpeg_write_bench_")
    dirs = {k: os.path.join(out, k) for k in ("device", "pil75", "pil95")}
    for d in dirs.values():
        os.makedirs(d, exist_ok=True)
    paths = {k: [os.path.join(d, f"{i + 1:05d}.jpg") for i in range(n)] for k, d in dirs.items()}

    roi_kw = {}
    if args.roi_levels != "none":
        B = args.roi_block_size
        grid = (n, -(-h // B), -(-w // B))
        levels = np.zeros(grid, np.uint8) if args.roi_levels == "zero" else np.random.default_rng(11).integers(0, 49, size=grid).astype(np.uint8)
        roi_kw = dict(roi_levels=torch.from_numpy(levels).to(dev), roi_block_size=B)
        setting.update(roi_levels=args.roi_levels, roi_block_size=B)
    if roi_kw or opt_kw:
        encode = lambda: jpeg_write._encode_clip(clip, "bgr", 95, "420", "bench", restart=restart, **roi_kw, **opt_kw)
    elif any(restart):
        encode = lambda: jpeg_write._encode_clip(clip, "bgr", 95, "420", "bench", restart=restart)
    else:
        encode = lambda: jpeg_write._encode_clip(clip, "bgr", 95, "420", "bench")
    if "encode" in measure:
        times = []
        encode()
        torch.cuda.synchronize()
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            got = encode()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        scan_bytes = int(got["out_off"][-1])
        ms = statistics.median(times)
        report(measurement="encode", **setting, frames=n, height=h, width=w, ms_per_clip=round(ms, 3), ms_per_frame=round(ms / n, 4),
               ms_min=round(min(times), 3), ms_max=round(max(times), 3), segments_per_frame=got.get("segments", 1),
               bytes_per_frame=round((sum(len(x) for x in got["headers"]) if "headers" in got else len(got["header"]) * n) / n + scan_bytes / n), algorithmic_bytes=clip.numel() + scan_bytes,
               fraction_of_hbm_peak=round((clip.numel() + scan_bytes) / (ms * 1e-3) / (HBM_PEAK_GBS * 1e9), 5), calls_ms=call_events(encode))

    if "roundtrip" in measure:
        def roundtrip():
            return jpeg_write.jpeg_roundtrip_device(clip, 95, "420", **restart_kw, **opt_kw)

        med, lo, hi = host_ms(roundtrip, args.reps)
        calls = call_events(roundtrip)
        report(measurement="roundtrip", **setting, frames=n, ms_per_clip=round(med, 2), ms_min=round(lo, 2), ms_max=round(hi, 2), calls_ms=calls,
               encode_calls_ms=round(sum(v for k, v in calls.items() if k in ("elvis_jpeg_fdct", "elvis_jpeg_bits", "elvis_jpeg_pack", "elvis_jpeg_stuff",
                                                                             "elvis_jpeg_bits_rst", "elvis_jpeg_pack_rst", "elvis_jpeg_stuff_rst",
                                                                             "elvis_jpeg_tally", "elvis_jpeg_bits_ftab", "elvis_jpeg_pack_ftab")), 3),
               reader_entropy_ms=calls.get("elvis_jpeg_entropy"), bytes_per_frame=round(float(roundtrip()[1].mean())))

    if "search" in measure:
        kw = dict(restart_kw, **roi_kw, **opt_kw)
        target = int(jpeg_write.jpeg_encoded_sizes_device(clip, 75, **kw).sum())
        probes = []
        real = jpeg_write.jpeg_encoded_sizes_device

        def counted(frames_d, quality, *a, **k):
            probes.append(int(quality))
            return real(frames_d, quality, *a, **k)

        jpeg_write.jpeg_encoded_sizes_device = counted
        try:
            quality, sizes, fits = jpeg_write.jpeg_quality_for_bytes(clip, target, **kw)
            count = len(probes)
            search = host_ms(lambda: jpeg_write.jpeg_quality_for_bytes(clip, target, **kw), args.reps)
        finally:
            jpeg_write.jpeg_encoded_sizes_device = real
        one = host_ms(lambda: jpeg_write.encode_jpeg_device(clip, **kw), args.reps)
        probe = host_ms(lambda: jpeg_write.jpeg_encoded_sizes_device(clip, 95, **kw), args.reps)
        report(measurement="search", **setting, frames=n, target_bytes=target, quality=quality, fits=fits, clip_bytes=int(sizes.sum()), probes=count,
               probed=probes[:count], search_ms=round(search[0], 2), search_ms_min=round(search[1], 2), search_ms_max=round(search[2], 2),
               one_encode_ms=round(one[0], 2), one_sizes_probe_ms=round(probe[0], 2), search_over_one_encode=round(search[0] / one[0], 2))

    if "roi_table" in measure:
        def psnr(decoded):
            err = (decoded.to(torch.float32) - clip.to(torch.float32)).pow(2).mean().item()
            return round(10 * np.log10(255.0 ** 2 / err), 2) if err else float("inf")

        B, shares = 8, (0.35, 0.25, 0.40)
        levels = (synth.synth_level_maps(20260502, n, -(-h // B), -(-w // B), shares) * 12).astype(np.uint8)
        plain, plain_bytes = jpeg_write.jpeg_roundtrip_device(clip, 95, restart_rows=1, **opt_kw)
        mapped, mapped_bytes = jpeg_write.jpeg_roundtrip_device(clip, 95, restart_rows=1, roi_levels=levels, roi_block_size=B, **opt_kw)
        equal, equal_bytes, quality, fits = jpeg_write.jpeg_roundtrip_at_bytes_device(clip, int(mapped_bytes.sum()), restart_rows=1, **opt_kw)
        report(measurement="roi_table", **opt_kw, frames=n, height=h, width=w, roi_block_size=B, level_shares_drawn=dict(zip(("0", "12", "24"), shares)),
               level_shares_of_cells={str(v): round(float((levels == v).mean()), 3) for v in (0, 12, 24)},
               q95_bytes_per_frame=round(float(plain_bytes.mean())), q95_psnr=psnr(plain),
               q95_roi_bytes_per_frame=round(float(mapped_bytes.mean())), q95_roi_psnr=psnr(mapped),
               uniform_quality_at_equal_bytes=quality, uniform_fits=fits, uniform_bytes_per_frame=round(float(equal_bytes.mean())), uniform_psnr=psnr(equal))

    if "optimize_split" in measure:
        from elvis_amd._lib import check, lib, ptr
        scode = jpeg_write.SUBSAMPLINGS.index("420")
        ri = jpeg_write.jpeg_restart_interval(w, h, 3, "420", *restart)
        blocks = int(lib().elvis_jpeg_frame_blocks(h, w, 3, scode))
        coef = torch.empty(n * blocks * 64, dtype=torch.int16, device=dev)
        hist_d = torch.empty(n * 2 * jpeg_write.HUFF_WORDS, dtype=torch.int32, device=dev)
        check(lib().elvis_jpeg_fdct(ptr(clip), ptr(coef), n, h, w, 3, 1, 95, scode, None), dev)
        rows = {k: [] for k in ("tally", "download", "builder", "upload")}
        for rep_i in range(args.reps + 1):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            check(lib().elvis_jpeg_tally(ptr(coef), ptr(hist_d), n, h, w, 3, scode, ri, None), dev)
            e1.record()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hist = hist_d.cpu().numpy().view(np.uint32).reshape(n, 2, jpeg_write.HUFF_WORDS)
            t1 = time.perf_counter()
            tables, ehuff = jpeg_write.jpeg_optimal_tables(hist, 3)
            heads = jpeg_write._frame_headers(w, h, 3, 95, "420", ri, tables)
            t2 = time.perf_counter()
            ehuff_d = torch.from_numpy(ehuff.view(np.int32)).to(dev)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            if rep_i:           # the first pass warms up
                for k, v in zip(rows, (e0.elapsed_time(e1), (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3)):
                    rows[k].append(v)
        del ehuff_d, heads

        def whole(**kw):
            times = []
            for rep_i in range(args.reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = jpeg_write._encode_clip(clip, "bgr", 95, "420", "bench", restart=restart, **roi_kw, **kw)
                torch.cuda.synchronize()
                if rep_i:
                    times.append((time.perf_counter() - t0) * 1e3)
            heads = sum(len(x) for x in got["headers"]) if "headers" in got else len(got["header"]) * n
            return statistics.median(times), min(times), max(times), round((heads + int(got["out_off"][-1])) / n)

        std, opt = whole(), whole(optimize=True)
        steps = {k: round(statistics.median(v), 3) for k, v in rows.items()}
        report(measurement="optimize_split", **{k: v for k, v in setting.items() if k != "optimize"}, frames=n, height=h, width=w, steps_ms=steps,
               steps_ms_min={k: round(min(v), 3) for k, v in rows.items()}, steps_ms_max={k: round(max(v), 3) for k, v in rows.items()},
               encode_ms=round(std[0], 3), encode_ms_min=round(std[1], 3), encode_ms_max=round(std[2], 3),
               encode_optimize_ms=round(opt[0], 3), encode_optimize_ms_min=round(opt[1], 3), encode_optimize_ms_max=round(opt[2], 3),
               rest_ms=round(opt[0] - sum(steps.values()), 3), bytes_per_frame=std[3], bytes_per_frame_optimize=opt[3],
               saved_fraction=round(1 - opt[3] / std[3], 4))

    if not measure & {"writers", "sizes"}:
        return

    def device_writer():
        jpeg_write.save_jpeg_frames_device(clip, paths["device"], **restart_kw, **opt_kw)

    def pil_path():
        for f, p in zip(recompose.frames_to_host(clip), paths["pil75"]):
            frameio.save_frame(f, p)

    def pil_95():
        for f, p in zip(recompose.frames_to_host(clip), paths["pil95"]):
            Image.fromarray(np.ascontiguousarray(f[:, :, ::-1]), "RGB").save(p, quality=95, subsampling=2, **pil_kw)

    rows = {}
    for name, fn in (("device", device_writer), ("pil75", pil_path), ("pil95", pil_95)):
        med, lo, hi = host_ms(fn, max(3, args.reps // 2))
        rows[name] = med
        report(measurement="writers", writer=name, ms_per_clip=round(med, 2), ms_min=round(lo, 2), ms_max=round(hi, 2),
               frames_per_second=round(n / (med * 1e-3), 1))
    report(measurement="writers", device_over_pil75=round(rows["pil75"] / rows["device"], 2), device_over_pil95=round(rows["pil95"] / rows["device"], 2))
    report(measurement="sizes", **{k: round(sum(os.path.getsize(p) for p in ps) / n) for k, ps in paths.items()})
    same = all(open(a, "rb").read().split(b"\xff\xda", 1)[1] == open(b, "rb").read().split(b"\xff\xda", 1)[1]
               for a, b in zip(paths["device"], paths["pil95"]))
    report(measurement="sizes", device_scan_equals_pil95=same)


if __name__ == "__main__":
    main()
