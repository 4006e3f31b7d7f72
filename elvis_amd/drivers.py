"""Directory-level restoration drivers: the two functions `run_elvis` calls on the client side
(elvis.py:4722, 4794) with the MI355X restorers in the model slots.

  restore_downsampled_with_sinsr   <- restore_downsampled_with_realesrgan  (elvis.py:2685-2769)
  restore_downsampled_with_realesrgan  <- the same function, with the networks the reference runs there (RRDBNet, SRVGGNetCompact)
  restore_blur_adaptive            <- restore_with_instantir_adaptive      (elvis.py:3000-3160)
  restore_dct_adaptive             -  the DCT slot the reference never wrote, given the
                                      Blur driver's shape
  stretch_shrunk_frames            <- the ELVIS v1 client-side stretch loop   (elvis.py:4534-4580)
  restore_shrunk_frames            <- the same loop and the CV2 inpaint loop after it (elvis.py:4534-4610), with the
                                      build-defined wavefront Telea (inpaint.py) in cv2.inpaint's place; with
                                      inpainter="temporal" the slot of inpaint_with_propainter / inpaint_with_e2fgvi
                                      (elvis.py:1458, 1693): the build-defined temporal fill (inpaint_temporal.py), then Telea
  calculate_removability_scores_from_frames
                                   <- calculate_removability_scores (elvis.py:968-1224) from frames and masks in memory,
                                      with the build-defined block complexity (complexity.py) in EVCA's place
  restore_yuv_clip                 -  the three model slots from a clip file (.y4m / raw .yuv, what a decoder emits) to
                                      a clip file, no PNG directory in between (described at the function)

Same arguments, file naming and errors as the reference: a directory of PNG frames (BGR on read) and a
`(frames, blocks_y, blocks_x)` map; the Downsample driver writes `output_dir/<same names>`, the Blur /
DCT drivers rewrite the frames in place.  Frames are dealt to the devices by the `chunk_for_devices`
rule.  One device: in-process.  Several devices: one spawned process per GPU (what
`restore_with_instantir_adaptive` does, elvis.py:3124-3158), each reading its own frame range and
writing its own files - the file system is the gather, exactly as in the reference (elvis.py:2983-2985).
Sampler noise is keyed on the global frame index and the DCT restorer reads its temporal halo frames
from the directory, so results do not depend on the device count.

Every driver that writes frames takes `png_writer="pil"` (the default: frameio.save_frame / save_mask, files as before)
or `"device"`: the PNGs are then written by the GPU (png.py) - decodable by any PNG reader to the same pixels, bytes not
PIL's or cv2's.  `"device-rle"` is "device" with `deflate="rle"` on everything it writes - frames, stretched frames and
full-resolution masks: a mask or a stretched frame, whose filtered bytes are nearly all 0, is then a match per 258 bytes
instead of a bit per byte.  Every built-in shard function returns a resident clip, and the writer takes it as it is
(`png.save_frames_device`: only finished files come down), as it takes a v1 shard's stretched frames and full-resolution
masks; only the host frames of a replaced `_shard_fn` go up once more (`png.save_frames`).  Any other value is a
ValueError; "device" or "device-rle" without a GPU raises.

Every such driver also takes `jpeg_writer="pil"` (the default: nothing changes - a `.jpg` / `.jpeg` name goes where
`png_writer` sends it, and "pil" writes it through PIL at PIL's quality 75) or `"device"`: output names that end in `.jpg`
or `.jpeg` are then written by the GPU from the resident clip (jpeg_write.py: baseline JPEG at quality 95, 4:2:0, what
`cv2.imwrite` uses; masks as gray), and every other name still goes where `png_writer` sends it.  Same errors as
`png_writer`.  With it goes `jpeg_restart_rows=0` (the default: no restart interval, as `cv2.imwrite` writes) or r > 0: the
device writes a restart interval of r MCU rows (jpeg_write.py `restart_rows=`) - any decoder reads the files, and the
device reader (`png_reader="device"` of the next driver) decodes an interval per lane instead of a frame per lane, so
turn it on whenever that reader will read the directory.  Non-zero with `jpeg_writer="pil"` is a ValueError.
And `jpeg_optimize=False` (the default: the Annex K Huffman tables) or True: the device codes every frame with its own
optimal tables (jpeg_write.py `optimize=True`, libjpeg's `optimize_coding`) - smaller files of the same pixels that any
decoder reads.  True with `jpeg_writer="pil"`, or a value that is no bool, is a ValueError.

Every driver also takes `png_reader="pil"` (the default: frameio.load_frame per file) or `"device"`: a worker's frame
range is then decoded by the GPU (jpeg.load_images_device: PNG and JPEG files, told apart by their first bytes; a
directory of PNGs is one call of png.load_frames_device) into one resident clip.  The built-in shard functions - v1
and the model slots' `restore_frames_*_device` alike - take that clip as it is: with both options "device" a worker's
pixels never visit the host.  A replaced `_shard_fn` gets `frames_to_host` of it.  Same errors as `png_writer`.

One worker (`_shard_worker`) serves every driver, the clip-file one included: a `ShardJob` names the shard function, the
source it loads its frame range from and the sink it saves it to (a PNG directory or a clip file), and whether the shard
function works on a resident clip or on host frames.
"""
from __future__ import annotations

import multiprocessing
import os
from dataclasses import dataclass, replace
from typing import Callable, List, Optional, Sequence, Union

import numpy as np
import torch

from . import recompose   # frames_to_device / frames_to_host are looked up at the call, where tests replace them
from .frameio import clear_directory, get_frame_paths, load_block_masks, load_frame, save_frame, save_mask
from .sharding import ChunkSpec, chunk_for_devices, resolve_device_list

DeviceSpec = Union[int, str, torch.device]
# (frames, maps, block_size, device, first_frame_index, **kw) -> frames ; replaceable for host-only tests
ShardFn = Callable[..., List[np.ndarray]]
# (clip, maps, block_size, device, first_frame_index, **kw) -> clip ; resident [n,H,W,3] u8 BGR in and out
ClipShardFn = Callable[..., torch.Tensor]


PNG_WRITERS = ("pil", "device", "device-rle")
_DEVICE_DEFLATE = {"device": "literal", "device-rle": "rle"}   # the device writers and the deflate= they pass to png.py
PNG_READERS = ("pil", "device")
JPEG_WRITERS = ("pil", "device")
JPEG_QUALITY, JPEG_SUBSAMPLING = 95, "420"      # what cv2.imwrite uses for a .jpg name


def _check_png_io(png_writer, png_reader, jpeg_writer="pil", jpeg_restart_rows=0, jpeg_optimize=False) -> None:
    """`png_writer=` of the directory drivers: "pil" (frameio.save_frame / save_mask, the default) or "device" (png.py:
    the files are written by the GPU - any PNG reader decodes them to the same pixels, the bytes are not PIL's) or
    "device-rle" (the same with `deflate="rle"`: runs of equal filtered bytes become matches, for masks and flat frames).
    `png_reader=`: "pil" (frameio.load_frame, the default) or "device" (png.py, jpeg.py: the PNG and JPEG files are
    decoded by the GPU into a resident clip - the same pixels).  `jpeg_writer=`: "pil" (nothing changes, the default) or
    "device" (jpeg_write.py: names ending in .jpg / .jpeg are written by the GPU at quality 95, 4:2:0).
    `jpeg_restart_rows=`: 0 (no restart interval, the default) or the MCU rows of the interval the device writer
    writes; PIL's writer here has none, so a non-zero value needs `jpeg_writer="device"`.  `jpeg_optimize=`: False (the
    Annex K Huffman tables, the default) or True (the device writer's `optimize=True`: every frame's own optimal
    tables); a bool, and True needs `jpeg_writer="device"` as well."""
    if jpeg_writer not in JPEG_WRITERS:
        raise ValueError(f"jpeg_writer must be one of {JPEG_WRITERS}, got {jpeg_writer!r}")
    if isinstance(jpeg_restart_rows, bool) or not isinstance(jpeg_restart_rows, (int, np.integer)) or jpeg_restart_rows < 0:
        raise ValueError(f"jpeg_restart_rows must be a non-negative integer, got {jpeg_restart_rows!r}")
    if jpeg_restart_rows and jpeg_writer != "device":
        raise ValueError(f"jpeg_restart_rows={jpeg_restart_rows} needs jpeg_writer='device', got jpeg_writer={jpeg_writer!r}")
    if not isinstance(jpeg_optimize, (bool, np.bool_)):
        raise ValueError(f"jpeg_optimize must be a bool, got {jpeg_optimize!r}")
    if jpeg_optimize and jpeg_writer != "device":
        raise ValueError(f"jpeg_optimize=True needs jpeg_writer='device', got jpeg_writer={jpeg_writer!r}")
    if png_writer not in PNG_WRITERS:
        raise ValueError(f"png_writer must be one of {PNG_WRITERS}, got {png_writer!r}")
    if png_reader not in PNG_READERS:
        raise ValueError(f"png_reader must be one of {PNG_READERS}, got {png_reader!r}")


def _is_jpeg_name(path) -> bool:
    return os.fspath(path).lower().endswith((".jpg", ".jpeg"))


def _write_jpeg_names(frames, paths: Sequence, device, restart_rows: int = 0, optimize: bool = False):
    """`jpeg_writer="device"`: the frames whose path ends in .jpg / .jpeg are written by jpeg_write.py - a resident clip
    as it is (only finished files come down), host frames through one upload - with a restart interval of
    `restart_rows` MCU rows where that is not 0, and with every frame's own optimal Huffman tables where `optimize` is
    set.  Returns the frames and paths that are left for the other writer, in
    their order."""
    mine = [i for i, p in enumerate(paths) if _is_jpeg_name(p)]
    if not mine:
        return frames, paths
    from . import jpeg_write
    rest = [i for i in range(len(paths)) if not _is_jpeg_name(paths[i])]
    kw = dict(quality=JPEG_QUALITY, subsampling=JPEG_SUBSAMPLING)
    if restart_rows:
        kw["restart_rows"] = int(restart_rows)      # the default call is the one it always was
    if optimize:
        kw["optimize"] = True
    if isinstance(frames, torch.Tensor):
        clip = frames if not rest else frames[torch.as_tensor(mine, device=frames.device)]
        jpeg_write.save_jpeg_frames_device(clip.contiguous(), [paths[i] for i in mine], **kw)
        left = frames[torch.as_tensor(rest, device=frames.device)] if rest else frames[:0]
    else:
        jpeg_write.save_jpeg_frames([frames[i] for i in mine], [paths[i] for i in mine], device, **kw)
        left = [frames[i] for i in rest]
    return left, [paths[i] for i in rest]


def _device_str(dev: torch.device) -> str:
    return f"cuda:{dev.index or 0}" if dev.type == "cuda" else str(dev)


# ----------------------------------------------------------------------------- where a worker's frames come from and go to
@dataclass(frozen=True)
class PngDirSource:
    """Frames `names` of the directory `in_dir`: a host list (`reader` "pil") or a resident clip ("device")."""
    in_dir: str
    names: Sequence[str]
    reader: str = "pil"

    @property
    def total(self) -> int:
        return len(self.names)

    def load(self, lo: int, hi: int, device):
        paths = [os.path.join(self.in_dir, n) for n in self.names[lo:hi]]
        if self.reader == "device":
            from .jpeg import load_images_device
            return load_images_device(paths, device)
        return [load_frame(p) for p in paths]


@dataclass(frozen=True)
class PngDirSink:
    """Frames written to `out_dir` under `names`: host frames through the save_frame loop (`writer` "pil"; a resident
    clip comes down first), or a resident clip through png.save_frames_device ("device": only finished files come down;
    host frames, what a replaced `_shard_fn` returns, go up once through png.save_frames).  `jpeg_writer` "device": the
    names that end in .jpg / .jpeg go through jpeg_write.py first (`jpeg_restart_rows`: its restart interval in MCU
    rows, 0 for none), the others as `writer` says."""
    out_dir: str
    names: Sequence[str]
    writer: str = "pil"
    jpeg_writer: str = "pil"
    jpeg_restart_rows: int = 0
    jpeg_optimize: bool = False

    def save(self, frames, start: int, device) -> None:
        paths = [os.path.join(self.out_dir, n) for n in self.names[start:start + len(frames)]]
        if self.jpeg_writer == "device":
            frames, paths = _write_jpeg_names(frames, paths, device, self.jpeg_restart_rows, self.jpeg_optimize)
            if not paths:
                return
        if self.writer in _DEVICE_DEFLATE:
            from .png import save_frames, save_frames_device
            if isinstance(frames, torch.Tensor):
                save_frames_device(frames.contiguous(), paths, deflate=_DEVICE_DEFLATE[self.writer])
            else:
                save_frames(frames, paths, device, deflate=_DEVICE_DEFLATE[self.writer])
            return
        for f, p in zip(recompose.frames_to_host(frames) if isinstance(frames, torch.Tensor) else frames, paths):
            save_frame(f, p)


_FRAME_MARKER = b"FRAME\n"


@dataclass(frozen=True)
class ClipFileSource:
    """The `total` frames of the clip file `path` ("y4m" | "yuv", `width` x `height`): the pixels go up as I420, 1.5
    bytes per pixel, and are a resident BGR clip from the conversion on."""
    path: str
    format: str
    width: int
    height: int
    total: int

    def load(self, lo: int, hi: int, device) -> torch.Tensor:
        from .handoff import load_y4m_device, load_yuv420p_device
        if self.format == "y4m":
            return load_y4m_device(self.path, device, "bgr", start=lo, count=hi - lo)
        return load_yuv420p_device(self.path, self.width, self.height, device, "bgr", start=lo, count=hi - lo)


@dataclass(frozen=True)
class ClipFileSink:
    """The clip file `path` ("y4m" | "yuv", `head` header bytes, `width` x `height` frames), which exists at full
    length: a resident BGR clip is converted back, comes down once as I420 and is written at its frames' own offsets."""
    path: str
    format: str
    head: int
    width: int
    height: int

    def save(self, clip: torch.Tensor, start: int, device) -> None:
        from .handoff import rgb_to_i420_device
        if tuple(clip.shape[1:]) != (self.height, self.width, 3):
            raise RuntimeError(f"restorer returned {tuple(clip.shape[1:])} frames for the {self.width}x{self.height} clip {self.path}")
        planes = rgb_to_i420_device(clip.contiguous(), "bgr")
        host = torch.empty(planes.shape, dtype=torch.uint8).pin_memory()
        host.copy_(planes, non_blocking=True)
        torch.cuda.current_stream(device).synchronize()
        rows = host.numpy()
        frame_bytes = self.width * self.height * 3 // 2
        with open(self.path, "r+b") as f:
            if self.format == "yuv":
                f.seek(start * frame_bytes)
                f.write(memoryview(rows).cast("B"))
            else:
                f.seek(self.head + start * (len(_FRAME_MARKER) + frame_bytes))
                for i in range(len(rows)):
                    f.write(_FRAME_MARKER)
                    f.write(memoryview(rows[i]).cast("B"))


# ----------------------------------------------------------------------------- jobs and workers
@dataclass(frozen=True, eq=False)
class ShardJob:
    """One worker's share of a driver call: frames [start, end) of `source` through `shard_fn` on `device` into `sink`.
    `resident`: the shard function takes and returns a resident [n,H,W,3] u8 clip (every built-in one, and a replaced
    `_shard_fn` of the clip driver), else a list of host frames (a replaced `_shard_fn` of a directory driver)."""
    shard_fn: Callable
    source: Union[PngDirSource, ClipFileSource]
    sink: Union[PngDirSink, ClipFileSink]
    resident: bool
    start: int
    end: int
    halo: int
    maps: np.ndarray
    block_size: int
    device: str
    kw: dict


def _shard_worker(job: ShardJob) -> None:
    """Restore frames [start, end) of the job's source on one device and hand them to its sink.  `halo` extra frames on
    each side are read (never written) for restorers with a temporal window; their maps are taken as given.  The frames
    reach the shard function in the form the job declares: whatever the source loaded is uploaded or downloaded once
    where it is in the other form, and passed through where it is not."""
    device = torch.device(job.device)
    if device.type == "cuda":
        torch.cuda.set_device(device)
    start, end = job.start, job.end
    lo, hi = max(0, start - job.halo), min(job.source.total, end + job.halo)
    frames = job.source.load(lo, hi, device)
    if job.resident and not isinstance(frames, torch.Tensor):
        frames = recompose.frames_to_device(frames, device)
    elif not job.resident and isinstance(frames, torch.Tensor):
        frames = recompose.frames_to_host(frames)
    restored = job.shard_fn(frames, np.asarray(job.maps[lo:hi]), job.block_size, device, lo, **job.kw)
    if len(restored) != hi - lo:
        raise RuntimeError(f"restorer returned {len(restored)} frames for {hi - lo} inputs on {job.device}")
    # a resident result has the clip's layout; its frame size is the sink's to judge (the v1 shards stretch theirs)
    if job.resident and (not isinstance(restored, torch.Tensor) or restored.dtype != torch.uint8
                         or restored.dim() != 4 or restored.shape[3] != frames.shape[3]):
        raise RuntimeError(f"restorer did not return the resident uint8 clip {tuple(frames.shape)} it was given on {job.device}")
    job.sink.save(restored[start - lo:end - lo], start, device)


def _shard_process(err_path: str, job: ShardJob) -> None:
    """Entry point of a spawned per-GPU worker: a failure is written to stderr and to `err_path` as
    `device / [start, end) / traceback`, so the parent can say WHICH shard failed and why."""
    import sys
    import traceback
    try:
        _shard_worker(job)
    except BaseException:
        msg = f"shard on {job.device}, frames [{job.start}, {job.end}):\n{traceback.format_exc()}"
        sys.stderr.write(msg)
        try:
            with open(err_path, "w") as f:
                f.write(msg)
        finally:
            raise SystemExit(1)


def _run_jobs(jobs: List[ShardJob]) -> None:
    """One job: in-process.  Several: one spawned process per job, failures gathered and reported by device and frame
    range (`_shard_process`)."""
    if len(jobs) == 1:
        _shard_worker(jobs[0])
        return
    import tempfile
    ctx = multiprocessing.get_context("spawn")   # never fork a process that may hold a GPU context
    with tempfile.TemporaryDirectory(prefix="elvis_shards_") as errdir:
        errs = [os.path.join(errdir, f"shard{i}.err") for i in range(len(jobs))]
        procs = [ctx.Process(target=_shard_process, args=(e, job)) for e, job in zip(errs, jobs)]
        for p in procs:
            p.start()
        failed = []
        for p, e, job in zip(procs, errs, jobs):
            p.join()
            if p.exitcode not in (0, None):
                detail = open(e).read() if os.path.exists(e) else \
                    f"shard on {job.device}, frames [{job.start}, {job.end}): exit code {p.exitcode} (no traceback: killed?)"
                failed.append(detail)
    if failed:
        raise RuntimeError("restoration worker(s) failed:\n" + "\n".join(failed))


def _png_jobs(builtin: Callable, _shard_fn: Optional[ShardFn], in_dir: str, out_dir: str, names: List[str],
              chunks: List[ChunkSpec], maps: np.ndarray, block_size: int, halo: int, kw: dict, png_writer: str,
              png_reader: str, jpeg_writer: str = "pil", jpeg_restart_rows: int = 0, jpeg_optimize: bool = False) -> List[ShardJob]:
    """The jobs of a directory driver, one per chunk: the resident `builtin` shard function, or the caller's `_shard_fn`
    on host frames.  `png_writer` / `png_reader` / `jpeg_writer` "device" need a GPU on every chunk."""
    for what, value in (("png_writer", png_writer), ("png_reader", png_reader), ("jpeg_writer", jpeg_writer)):
        if value != "pil":
            for c in chunks:
                if c.device.type != "cuda":
                    raise RuntimeError(f"{what}='{value}' needs a GPU (got device '{c.device}'); there is no CPU path")
    source, sink = PngDirSource(in_dir, names, png_reader), PngDirSink(out_dir, names, png_writer, jpeg_writer, jpeg_restart_rows, jpeg_optimize)
    return [ShardJob(_shard_fn or builtin, source, sink, _shard_fn is None, c.start, c.end, halo, maps, block_size,
                     _device_str(c.device), kw) for c in chunks]


# ----------------------------------------------------------------------------- the shard functions
def _sinsr_clip_shard(clip, maps, block_size, device, first_frame_index, **kw):
    from .restore import restore_frames_sinsr_device
    return restore_frames_sinsr_device(clip, maps, block_size, first_frame_index=first_frame_index, **kw)


def _blur_clip_shard(clip, maps, block_size, device, first_frame_index, **kw):
    from .restore import restore_frames_blur_device
    return restore_frames_blur_device(clip, maps, block_size, **kw)


def _dct_clip_shard(clip, maps, block_size, device, first_frame_index, **kw):
    from .restore import restore_frames_dct_device
    return restore_frames_dct_device(clip, maps, block_size, **kw)


def _realesrgan_clip_shard(clip, maps, block_size, device, first_frame_index, **kw):
    from .restore import restore_frames_realesrgan_device
    return restore_frames_realesrgan_device(clip, maps, block_size, **kw)


_CLIP_SHARDS = {"sinsr": _sinsr_clip_shard, "blur": _blur_clip_shard, "dct": _dct_clip_shard,
                "realesrgan": _realesrgan_clip_shard}


def _write_clip(clip: torch.Tensor, directory: str, names: Sequence[str], png_writer: str, jpeg_writer: str = "pil",
                jpeg_restart_rows: int = 0, jpeg_optimize: bool = False) -> None:
    """A resident clip of frames [n,H,W,3] or of masks [n,H,W] as PNGs `names` of `directory`, with either writer: the
    device writer takes the clip as it is and only finished files come down.  `jpeg_writer` "device": names ending in
    .jpg / .jpeg are written as JPEG by the device, masks as gray, with a restart interval of `jpeg_restart_rows` MCU rows
    where that is not 0."""
    paths = [os.path.join(directory, name) for name in names]
    if jpeg_writer == "device":
        clip, paths = _write_jpeg_names(clip, paths, clip.device, jpeg_restart_rows, jpeg_optimize)
        if not paths:
            return
    if png_writer in _DEVICE_DEFLATE:
        from .png import save_frames_device
        save_frames_device(clip.contiguous(), paths, deflate=_DEVICE_DEFLATE[png_writer])
    elif clip.dim() == 4:
        for f, p in zip(recompose.frames_to_host(clip), paths):
            save_frame(f, p)
    else:
        for m, p in zip(clip.cpu().numpy(), paths):
            save_mask(m, p)


def _v1_shard(clip, maps, block_size, device, first_frame_index, inpaint=False, stretched_dir=None,
              fullres_masks_dir=None, png_writer="pil", inpainter="telea", inpaint_params=None, own=None, jpeg_writer="pil",
              jpeg_restart_rows=0, jpeg_optimize=False, **kw):
    """Stretch a run of decoded shrunk frames in one launch pair and, with `inpaint`, fill their holes without leaving
    the device: the hole mask goes from the gather to the inpainter as a resident tensor.  The stretched frames and the
    full-resolution masks are written only where a directory asks for them, under the global frame numbers.

    `own` = (start, end), global frame numbers: the frames of the run that are this worker's (all of them when None);
    the others are temporal context read for `inpainter="temporal"`.  Only the worker's own frames are written to the
    side directories and go through the spatial inpainter; the context frames come back temporally filled at most, and
    the worker drops them."""
    from .shrink import stretch_device
    a, b = (0, len(clip)) if own is None else (own[0] - first_frame_index, own[1] - first_frame_index)
    if not 0 <= a <= b <= len(clip):
        raise ValueError(f"frames [{own[0]}, {own[1]}) are not in the run of {len(clip)} from {first_frame_index}")
    with torch.cuda.device(device):
        md = torch.from_numpy(np.ascontiguousarray(np.asarray(maps) != 0).view(np.uint8)).to(device)
        out, full = stretch_device(clip, md, block_size, "flat", fullres_mask=True)
        names = [f"{first_frame_index + i + 1:05d}.png" for i in range(a, b)]
        jpeg_kw = {} if jpeg_writer == "pil" else {"jpeg_writer": jpeg_writer}    # the default call is the one it always was
        if jpeg_restart_rows:
            jpeg_kw["jpeg_restart_rows"] = jpeg_restart_rows
        if jpeg_optimize:
            jpeg_kw["jpeg_optimize"] = True
        if stretched_dir is not None:
            _write_clip(out[a:b], stretched_dir, names, png_writer, **jpeg_kw)
        if fullres_masks_dir is not None:
            _write_clip(full[a:b], fullres_masks_dir, names, png_writer, **jpeg_kw)
        if inpaint:
            from .inpaint import inpaint_device
            if inpainter == "temporal":
                from .inpaint_temporal import temporal_fill_device
                out, full = temporal_fill_device(out, full, **(inpaint_params or {}))
            if b > a:
                inpaint_device(out[a:b], full[a:b], out=out[a:b])
        return out


def _frames_and_maps(frames_dir: str, maps, what: str):
    paths = get_frame_paths(frames_dir)
    if not paths:
        raise ValueError(f"No frames found in {frames_dir}")
    maps = np.asarray(maps)
    if maps.ndim != 3 or maps.shape[0] != len(paths):
        raise ValueError(f"{what} length ({maps.shape[0] if maps.ndim else 0}) does not match frame count ({len(paths)}).")
    return [p.name for p in paths], maps


def _restore_downsampled(builtin: Callable, kw: dict, input_frames_dir: str, output_frames_dir: str, downscale_maps,
                         block_size: int, devices, png_writer: str, png_reader: str, _shard_fn: Optional[ShardFn],
                         jpeg_writer: str = "pil", jpeg_restart_rows: int = 0, jpeg_optimize: bool = False) -> None:
    """What the two Downsample drivers share once their own arguments are checked: `output_frames_dir` is cleared and
    every frame of `input_frames_dir` is written to it under the same name."""
    names, maps = _frames_and_maps(input_frames_dir, downscale_maps, "Downscale maps")
    clear_directory(output_frames_dir)
    os.makedirs(output_frames_dir, exist_ok=True)
    devs = resolve_device_list(devices, prefer_cuda=True, allow_cpu_fallback=_shard_fn is not None)
    _run_jobs(_png_jobs(builtin, _shard_fn, input_frames_dir, output_frames_dir, names, chunk_for_devices(len(names), devs),
                        maps, block_size, 0, kw if _shard_fn is None else {}, png_writer, png_reader, jpeg_writer,
                        jpeg_restart_rows, jpeg_optimize))


def restore_downsampled_with_sinsr(
    input_frames_dir: str,
    output_frames_dir: str,
    downscale_maps: np.ndarray,
    block_size: int,
    *,
    fp32: bool = False,
    devices: Optional[Sequence[DeviceSpec]] = None,
    parallel_chunk_length: Optional[int] = None,
    per_device_workers: int = 1,
    seed: int = 42,
    schedule: str = "staged",
    png_writer: str = "pil",
    png_reader: str = "pil",
    jpeg_writer: str = "pil",
    jpeg_restart_rows: int = 0,
    jpeg_optimize: bool = False,
    _shard_fn: Optional[ShardFn] = None,
    **model_kwargs,
) -> None:
    """Adaptive SinSR restoration over a directory of frames: drop-in for
    `restore_downsampled_with_realesrgan`.  `downscale_maps[f, by, bx]` = log2 of the block's downscale
    factor (elvis.py:2146, 2558).  `schedule="staged"` is the reference's coarse-to-fine loop
    (elvis.py:2570-2598) with 4x stages; "single4x" is the north-star single 4x call from the /4 level.
    The Real-ESRGAN keywords of the reference call (model_name, denoise_strength, tile, tile_pad, pre_pad)
    are accepted and ignored, as are `parallel_chunk_length` / `per_device_workers` (the reference ignores
    them too, elvis.py:2698-2699)."""
    _ = (parallel_chunk_length, per_device_workers)
    _check_png_io(png_writer, png_reader, jpeg_writer, jpeg_restart_rows, jpeg_optimize)
    kw = dict(fp32=fp32, seed=seed, schedule=schedule)
    kw.update({k: v for k, v in model_kwargs.items() if k in ("cfg",)})
    _restore_downsampled(_sinsr_clip_shard, kw, input_frames_dir, output_frames_dir, downscale_maps, block_size, devices,
                         png_writer, png_reader, _shard_fn, jpeg_writer, jpeg_restart_rows, jpeg_optimize)


def restore_downsampled_with_realesrgan(
    input_frames_dir: str,
    output_frames_dir: str,
    downscale_maps: np.ndarray,
    block_size: int,
    *,
    model_name: str = "RealESRGAN_x4plus",
    denoise_strength: float = 1.0,
    tile: int = 0,
    tile_pad: int = 10,
    pre_pad: int = 0,
    fp32: bool = False,
    devices: Optional[Sequence[DeviceSpec]] = None,
    parallel_chunk_length: Optional[int] = None,
    per_device_workers: int = 1,
    model_path: Optional[str] = None,
    schedule: str = "staged",
    png_writer: str = "pil",
    png_reader: str = "pil",
    jpeg_writer: str = "pil",
    jpeg_restart_rows: int = 0,
    jpeg_optimize: bool = False,
    _shard_fn: Optional[ShardFn] = None,
    enhance: str = "area",
) -> None:
    """Adaptive Real-ESRGAN restoration over a directory of frames: the reference's function of this name
    (elvis.py:2685-2769) with its own networks, RRDBNet or SRVGGNetCompact by `model_name`, in the model slot
    (`restore.restore_frames_realesrgan`, which lists the departures: no fp32, no pre_pad, `tile` / `tile_pad` ignored;
    `denoise_strength` is honoured for `realesr-general-x4v3` and refused elsewhere).  `model_path` is the checkpoint
    file (e.g. "RealESRGAN_x4plus.pth"; for `denoise_strength != 1` a pair of files, or one with
    `realesr-general-wdn-x4v3.pth` beside it); without it the weights are seeded and synthetic.
    `parallel_chunk_length` / `per_device_workers` are accepted and ignored, as in the reference (elvis.py:2698-2699).
    `enhance="reference"` (default "area"): `tile`, `tile_pad` and `pre_pad` are honoured and every stage resizes with
    Lanczos4, as `restore.restore_frames_realesrgan` describes."""
    _ = (parallel_chunk_length, per_device_workers)
    _check_png_io(png_writer, png_reader, jpeg_writer, jpeg_restart_rows, jpeg_optimize)
    if _shard_fn is None:
        from .restore import _check_realesrgan_args
        _check_realesrgan_args(denoise_strength, pre_pad, fp32, model_name, enhance)
    kw = dict(model_name=model_name, denoise_strength=denoise_strength, tile=tile, tile_pad=tile_pad, pre_pad=pre_pad,
              fp32=fp32, model_path=model_path, schedule=schedule, enhance=enhance)
    _restore_downsampled(_realesrgan_clip_shard, kw, input_frames_dir, output_frames_dir, downscale_maps, block_size, devices,
                         png_writer, png_reader, _shard_fn, jpeg_writer, jpeg_restart_rows, jpeg_optimize)


def _restore_in_place(builtin: Callable, _shard_fn: Optional[ShardFn], frames_dir: str, maps, block_size: int, devices,
                      halo: int, kw: dict, what: str, png_writer: str, png_reader: str, jpeg_writer: str = "pil",
                      jpeg_restart_rows: int = 0, jpeg_optimize: bool = False) -> None:
    _check_png_io(png_writer, png_reader, jpeg_writer, jpeg_restart_rows, jpeg_optimize)
    names, maps = _frames_and_maps(frames_dir, maps, what)
    if maps.size == 0 or int(np.max(maps)) <= 0:
        return   # nothing degraded: the frames stay as decoded (elvis.py:3042-3044)
    devs = resolve_device_list(devices, prefer_cuda=True, allow_cpu_fallback=_shard_fn is not None)
    gpus = [d for d in devs if d.type == "cuda"]
    workers = gpus or devs[:1]            # the reference uses every GPU, else the first device (elvis.py:3030-3031)
    chunks = chunk_for_devices(len(names), workers)
    if halo and len(chunks) > 1:
        # in-place rewrite with a temporal halo: neighbours must read the DECODED halo frames, so restore
        # into a scratch directory first and move the files over once every worker is done
        scratch = os.path.join(frames_dir, ".elvis_restore_tmp")
        os.makedirs(scratch, exist_ok=True)
        try:
            _run_jobs(_png_jobs(builtin, _shard_fn, frames_dir, scratch, names, chunks, maps, block_size, halo, kw,
                                png_writer, png_reader, jpeg_writer, jpeg_restart_rows, jpeg_optimize))
            for n in names:
                os.replace(os.path.join(scratch, n), os.path.join(frames_dir, n))
        finally:
            for n in os.listdir(scratch):
                os.unlink(os.path.join(scratch, n))
            os.rmdir(scratch)
    else:
        _run_jobs(_png_jobs(builtin, _shard_fn, frames_dir, frames_dir, names, chunks, maps, block_size, halo, kw,
                            png_writer, png_reader, jpeg_writer, jpeg_restart_rows, jpeg_optimize))


def restore_blur_adaptive(
    input_frames_dir: str,
    blur_maps: np.ndarray,
    block_size: int,
    cfg: float = 7.0,
    creative_start: float = 1.0,
    preview_start: float = 0.0,
    seed: Optional[int] = 42,
    devices: Optional[Sequence[DeviceSpec]] = None,
    batch_size: int = 4,
    parallel_chunk_length: Optional[int] = None,
    *,
    fp32: bool = False,
    png_writer: str = "pil",
    png_reader: str = "pil",
    jpeg_writer: str = "pil",
    jpeg_restart_rows: int = 0,
    jpeg_optimize: bool = False,
    _shard_fn: Optional[ShardFn] = None,
) -> None:
    """ELVIS v2 Blur client side over a directory, IN PLACE: drop-in for `restore_with_instantir_adaptive`
    with the SwinTormer-style deblurrer in the model slot.  `blur_maps[f, by, bx]` = blur rounds
    (elvis.py:2176); per round every still-active frame is restored, finished blocks are re-pasted from
    the decoded frame, positive entries are decremented (elvis.py:2947-2981).  The diffusion keywords
    (cfg, creative_start, preview_start) and the seed have no meaning for a deterministic forward pass
    and are ignored; `parallel_chunk_length` is ignored like in the reference (elvis.py:3015)."""
    _ = (cfg, creative_start, preview_start, seed, parallel_chunk_length)
    _check_png_io(png_writer, png_reader, jpeg_writer, jpeg_restart_rows, jpeg_optimize)
    if batch_size < 1:
        raise ValueError("`batch_size` must be at least 1.")
    kw = {} if _shard_fn is not None else dict(batch_size=batch_size, fp32=fp32)
    _restore_in_place(_blur_clip_shard, _shard_fn, input_frames_dir, blur_maps, block_size, devices, 0, kw, "blur_maps",
                      png_writer, png_reader, jpeg_writer, jpeg_restart_rows, jpeg_optimize)


def restore_dct_adaptive(
    input_frames_dir: str,
    strength_maps: np.ndarray,
    block_size: int,
    devices: Optional[Sequence[DeviceSpec]] = None,
    *,
    fp32: bool = False,
    temporal_radius: int = 3,
    png_writer: str = "pil",
    png_reader: str = "pil",
    jpeg_writer: str = "pil",
    jpeg_restart_rows: int = 0,
    jpeg_optimize: bool = False,
    _shard_fn: Optional[ShardFn] = None,
) -> None:
    """ELVIS v2 DCT client side over a directory, IN PLACE (the build's definition of the slot; the
    reference has none): one pass of the LaplacianVCAR-style restorer, `level > 0 ? restored : decoded`.
    Each worker also reads `temporal_radius` decoded frames on either side of its range (read-only
    overlap, the expand-then-trim pattern of elvis.py:1550-1566, 1650-1657)."""
    kw = {} if _shard_fn is not None else dict(fp32=fp32)
    _restore_in_place(_dct_clip_shard, _shard_fn, input_frames_dir, strength_maps, block_size, devices,
                      max(0, int(temporal_radius)), kw, "strength_maps", png_writer, png_reader, jpeg_writer, jpeg_restart_rows, jpeg_optimize)


def _v1_clip(frames_dir: str, masks_npz: str, block_size: int):
    """The removal masks of `masks_npz` and the names `00001.png` ... of the shrunk frames they belong to, checked:
    every frame exists and holds exactly as many blocks as its mask keeps (`stretch_frame`'s rule)."""
    masks = load_block_masks(masks_npz)
    if masks.ndim != 3 or masks.shape[0] == 0:
        raise ValueError(f"removal masks must be (frames, blocks_y, blocks_x); got {masks.shape}")
    names = [f"{i + 1:05d}.png" for i in range(masks.shape[0])]
    missing = [n for n in names if not os.path.isfile(os.path.join(frames_dir, n))]
    if missing:
        raise ValueError(f"No frame {missing[0]} in {frames_dir} ({len(missing)} of {len(names)} frames missing)")
    from PIL import Image
    for i, n in enumerate(names):
        with Image.open(os.path.join(frames_dir, n)) as im:
            w, h = im.size
        kept = int(masks[i].size - np.count_nonzero(masks[i]))
        if h % block_size or w % block_size or (h // block_size) * (w // block_size) != kept:
            raise ValueError(f"{n}: a {h}x{w} frame does not hold the {kept} blocks of {block_size} its mask keeps")
    return masks, names


def _v1_kw(png_writer: str, jpeg_writer: str = "pil", jpeg_restart_rows: int = 0, jpeg_optimize: bool = False, **dirs) -> dict:
    """The keywords of a v1 shard step: its directories, and each writer where it is not the default (a replaced
    `_shard_fn` of the default path sees the keywords it always saw)."""
    kw = dict(dirs, png_writer=png_writer) if png_writer != "pil" else dirs
    kw = dict(kw, jpeg_writer=jpeg_writer) if jpeg_writer != "pil" else kw
    kw = dict(kw, jpeg_restart_rows=jpeg_restart_rows) if jpeg_restart_rows else kw
    return dict(kw, jpeg_optimize=True) if jpeg_optimize else kw


INPAINTERS = ("telea", "temporal")


def _check_inpainter(inpainter, inpaint_params) -> dict:
    """`inpainter=` of `restore_shrunk_frames`: "telea" (the wavefront Telea of inpaint.py alone, the default; it takes
    no parameters) or "temporal" (inpaint_temporal.py: the temporal fill, then Telea on what is left; `inpaint_params`
    are the fill's block, margin, radius, search, max_mad).  Returns the fill's parameters with the defaults filled in
    ({} for "telea"); ValueError for anything else."""
    if inpainter not in INPAINTERS:
        raise ValueError(f"inpainter must be one of {INPAINTERS}, got {inpainter!r}")
    if inpaint_params is not None and not isinstance(inpaint_params, dict):
        raise ValueError(f"inpaint_params must be a dict or None, got {type(inpaint_params).__name__}")
    if inpainter == "telea":
        if inpaint_params:
            raise ValueError(f"inpainter='telea' takes no inpaint_params, got {sorted(inpaint_params)}")
        return {}
    from .inpaint_temporal import check_params
    return check_params("restore_shrunk_frames", **(inpaint_params or {}))


def _run_v1(inpaint: bool, frames_dir: str, masks_npz: str, block_size: int, out_dir: str, block_masks_dir: Optional[str],
            devices, png_writer: str, png_reader: str, _shard_fn: Optional[ShardFn], inpainter: str = "telea",
            inpaint_params: Optional[dict] = None, jpeg_writer: str = "pil", jpeg_restart_rows: int = 0, jpeg_optimize: bool = False, **dirs) -> np.ndarray:
    """What the two v1 drivers share: the checks, the directories (`dirs`: the ones the shard step writes, by keyword),
    the block-resolution masks, and the stretch (and `inpaint`) of every frame of `frames_dir` into `out_dir`.  With the
    temporal inpainter every worker also reads `radius` frames on either side of its own, and its shard step is told
    which frames are its own (`own`): no two workers write the same file."""
    _check_png_io(png_writer, png_reader, jpeg_writer, jpeg_restart_rows, jpeg_optimize)
    params = _check_inpainter(inpainter, inpaint_params)
    masks, names = _v1_clip(frames_dir, masks_npz, block_size)
    for d in (out_dir, *dirs.values(), block_masks_dir):
        if d is not None:
            os.makedirs(d, exist_ok=True)
    if block_masks_dir is not None:
        for i, n in enumerate(names):
            save_mask((masks[i] * 255).astype(np.uint8), os.path.join(block_masks_dir, n))
    devs = resolve_device_list(devices, prefer_cuda=True, allow_cpu_fallback=_shard_fn is not None)
    gpus = [d for d in devs if d.type == "cuda"]
    workers = gpus or (devs if _shard_fn is not None else devs[:1])
    kw = _v1_kw(png_writer, jpeg_writer, jpeg_restart_rows, jpeg_optimize, **dirs)
    temporal = inpainter == "temporal"
    if temporal:
        kw = dict(kw, inpainter=inpainter, inpaint_params=params)
    jobs = _png_jobs(_v1_shard, _shard_fn, frames_dir, out_dir, names, chunk_for_devices(len(names), workers), masks,
                     block_size, params["radius"] if temporal else 0, kw if _shard_fn is not None else dict(kw, inpaint=inpaint),
                     png_writer, png_reader, jpeg_writer, jpeg_restart_rows, jpeg_optimize)
    if temporal:
        jobs = [replace(job, kw=dict(job.kw, own=(job.start, job.end))) for job in jobs]
    _run_jobs(jobs)
    return masks


def stretch_shrunk_frames(
    frames_dir: str,
    masks_npz: str,
    block_size: int,
    out_dir: Optional[str] = None,
    fullres_masks_dir: Optional[str] = None,
    block_masks_dir: Optional[str] = None,
    devices: Optional[Sequence[DeviceSpec]] = None,
    *,
    png_writer: str = "pil",
    png_reader: str = "pil",
    jpeg_writer: str = "pil",
    jpeg_restart_rows: int = 0,
    jpeg_optimize: bool = False,
    _shard_fn: Optional[ShardFn] = None,
) -> np.ndarray:
    """ELVIS v1 client side over a directory (elvis.py:4534-4580): unpack the removal masks of `masks_npz`
    (`frameio.load_block_masks`), stretch the decoded shrunk frames `00001.png` ... (one per mask) - in place, or
    into `out_dir` - and write the masks for the inpainter as PNGs under the same `{i+1:05d}.png` names: 0/255 at
    block resolution into `block_masks_dir`, 0/255 at frame resolution into `fullres_masks_dir` (either may be None).
    Frames are dealt to the devices by the `chunk_for_devices` rule.  Returns the unpacked masks.

    Every frame must hold exactly as many blocks as its mask keeps (`stretch_frame`'s rule): ValueError otherwise,
    before anything is written."""
    return _run_v1(False, frames_dir, masks_npz, block_size, out_dir or frames_dir, block_masks_dir, devices, png_writer,
                   png_reader, _shard_fn, jpeg_writer=jpeg_writer, jpeg_restart_rows=jpeg_restart_rows, jpeg_optimize=jpeg_optimize,
                   fullres_masks_dir=fullres_masks_dir)


def restore_shrunk_frames(
    frames_dir: str,
    masks_npz: str,
    block_size: int,
    out_dir: str,
    stretched_dir: Optional[str] = None,
    fullres_masks_dir: Optional[str] = None,
    block_masks_dir: Optional[str] = None,
    devices: Optional[Sequence[DeviceSpec]] = None,
    *,
    png_writer: str = "pil",
    png_reader: str = "pil",
    jpeg_writer: str = "pil",
    jpeg_restart_rows: int = 0,
    jpeg_optimize: bool = False,
    inpainter: str = "telea",
    inpaint_params: Optional[dict] = None,
    _shard_fn: Optional[ShardFn] = None,
) -> np.ndarray:
    """The whole ELVIS v1 client side over a directory (elvis.py:4534-4610): unpack the removal masks of `masks_npz`,
    stretch the decoded shrunk frames `00001.png` ... of `frames_dir` (one per mask) and inpaint the holes - the
    reference's `cv2.inpaint(frame, mask, 3, cv2.INPAINT_TELEA)` loop, here the build-defined wavefront Telea of
    `inpaint.py` (not cv2's bytes).  The inpainted frames go to `out_dir` under the same names and
    `frames_dir` is left as it is.  The hole masks stay on the device between the two steps; the stretched frames
    (`stretched_dir`), the 0/255 masks at frame resolution (`fullres_masks_dir`) and at block resolution
    (`block_masks_dir`) are written only where a directory is given.  Validation and sharding are those of
    `stretch_shrunk_frames`: ValueError before anything is written, frames dealt by the `chunk_for_devices` rule,
    one worker per GPU.  Returns the unpacked masks.

    `inpainter="temporal"` stands where the reference runs its video inpainters (`inpaint_with_propainter` /
    `inpaint_with_e2fgvi`, elvis.py:1458, 1693): the build-defined temporal fill of `inpaint_temporal.py` - neither of
    those networks - takes what it can from the `radius` frames on either side, and the wavefront Telea fills the rest.
    `inpaint_params` are that fill's block, margin, radius, search and max_mad.  Every worker reads `radius` extra
    frames on either side of its own, so the result is the same for every device count.  Any other `inpainter` is a
    ValueError, before anything is written."""
    if out_dir is None:
        raise ValueError("restore_shrunk_frames: out_dir is required")
    return _run_v1(True, frames_dir, masks_npz, block_size, out_dir, block_masks_dir, devices, png_writer, png_reader,
                   _shard_fn, inpainter, inpaint_params, jpeg_writer=jpeg_writer, jpeg_restart_rows=jpeg_restart_rows, jpeg_optimize=jpeg_optimize,
                   stretched_dir=stretched_dir,
                   fullres_masks_dir=fullres_masks_dir)


# ----------------------------------------------------------------------------- clip files: decoder output in, encoder input out
YUV_CLIP_KINDS = {"sinsr": "Downscale maps", "blur": "blur_maps", "dct": "strength_maps", "realesrgan": "Downscale maps"}


def _clip_format(path: str, what: str) -> str:
    ext = os.path.splitext(os.fspath(path))[1].lower()
    if ext not in (".y4m", ".yuv"):
        raise ValueError(f"restore_yuv_clip: {what} must be a .y4m or a .yuv file, got {os.fspath(path)!r}")
    return ext[1:]


def restore_yuv_clip(
    kind: str,
    input_path: str,
    output_path: str,
    maps: np.ndarray,
    block_size: int,
    *,
    width: Optional[int] = None,
    height: Optional[int] = None,
    framerate: Optional[float] = None,
    devices: Optional[Sequence[DeviceSpec]] = None,
    _shard_fn: Optional[ClipShardFn] = None,
    **kw,
) -> None:
    """One of the model slots - `kind` "sinsr" (`restore_frames_sinsr`), "realesrgan" (`restore_frames_realesrgan`),
    "blur" (`restore_frames_blur`) or "dct" (`restore_frames_dct`) - from a clip file to a clip file: what a decoder emits (`ffmpeg -f yuv4mpegpipe`, or
    `-f rawvideo -pix_fmt yuv420p`) in, what the encoders and VMAF take out, no directory of PNGs in between.

    `input_path` is a `.y4m` file, or a raw `.yuv` with `width` and `height`; `output_path` is a `.y4m` (`handoff.y4m_header`
    and the `FRAME\\n` framing of `write_y4m`; the frame rate is the input's, or `framerate`, which a raw input needs) or
    a `.yuv`, chosen by extension, and another file than the input.  `maps` is `(frames, blocks_y, blocks_x)`.  Keywords
    are the restorer's (`fp32`, `seed`, `schedule`, `cfg`, `batch_size`, ...); `temporal_radius` (3) is the DCT
    restorer's halo.

    Frames are dealt to the devices by the `chunk_for_devices` rule: one device runs in-process, several use one
    spawned process per GPU.  Every frame has a fixed size, so the output file is created at full length and each
    worker writes its own frame range at its own offsets - the file system is the gather.  A worker loads its range
    (`handoff.load_y4m_device` / `load_yuv420p_device`; for "dct" with `temporal_radius` halo frames on either side, read
    from the input, never written), runs the `*_device` restorer, converts back (`handoff.rgb_to_i420_device`) and
    downloads 1.5 bytes per pixel: RGB pixels never visit the host.  Decoded frames are BGR inside, as in the directory
    drivers.  PARITY UNPINNED vs cv2 for both conversions (handoff.py)."""
    from .handoff import parse_y4m, y4m_header, yuv420p_frame_count
    if kind not in YUV_CLIP_KINDS:
        raise ValueError(f"restore_yuv_clip: kind must be one of {tuple(YUV_CLIP_KINDS)}, got {kind!r}")
    in_format, out_format = _clip_format(input_path, "input_path"), _clip_format(output_path, "output_path")
    input_path, output_path = os.fspath(input_path), os.fspath(output_path)
    if os.path.realpath(input_path) == os.path.realpath(output_path) or \
            (os.path.exists(output_path) and os.path.exists(input_path) and os.path.samefile(input_path, output_path)):
        raise ValueError(f"restore_yuv_clip: input and output must be different files, got {input_path!r} twice")
    if in_format == "y4m":
        info = parse_y4m(input_path)
        for name, given, found in (("width", width, info.width), ("height", height, info.height)):
            if given is not None and int(given) != found:
                raise ValueError(f"restore_yuv_clip: {name}={given} but {input_path} says {found}")
        width, height, total = info.width, info.height, info.frame_count
        if framerate is None:
            framerate = info.framerate
    else:
        if width is None or height is None:
            raise ValueError("restore_yuv_clip: a raw .yuv input needs width= and height=")
        width, height = int(width), int(height)
        total = yuv420p_frame_count(os.path.getsize(input_path), width, height, input_path)
    if out_format == "y4m" and framerate is None:
        raise ValueError("restore_yuv_clip: a .y4m output needs a frame rate: pass framerate= (the input gives none)")
    if total == 0:
        raise ValueError(f"No frames found in {input_path}")
    maps = np.asarray(maps)
    if maps.ndim != 3 or maps.shape[0] != total:
        raise ValueError(f"{YUV_CLIP_KINDS[kind]} length ({maps.shape[0] if maps.ndim else 0}) does not match frame count ({total}).")
    if kind == "blur" and int(kw.get("batch_size", 4)) < 1:
        raise ValueError("`batch_size` must be at least 1.")
    halo = max(0, int(kw.pop("temporal_radius", 3))) if kind == "dct" else 0
    devs = resolve_device_list(devices, prefer_cuda=True, allow_cpu_fallback=False)
    for d in devs:
        if d.type != "cuda":
            raise RuntimeError(f"restore_yuv_clip needs a GPU (got device '{d}'); there is no CPU path")
    head = y4m_header(width, height, framerate) if out_format == "y4m" else b""
    frame_bytes = width * height * 3 // 2
    with open(output_path, "wb") as f:
        f.write(head)
        f.truncate(len(head) + total * (frame_bytes + (len(_FRAME_MARKER) if out_format == "y4m" else 0)))
    source = ClipFileSource(input_path, in_format, width, height, total)
    sink = ClipFileSink(output_path, out_format, len(head), width, height)
    _run_jobs([ShardJob(_shard_fn or _CLIP_SHARDS[kind], source, sink, True, c.start, c.end, halo, maps, block_size,
                        _device_str(c.device), {} if _shard_fn is not None else kw) for c in chunk_for_devices(total, devs)])


def calculate_removability_scores_from_frames(frames, foreground_masks, block_size: int, alpha: float = 0.5,
                                              smoothing_beta: float = 1, device="cuda:0", *, order: str = "bgr",
                                              chunk_frames: Optional[int] = None) -> np.ndarray:
    """The server side's first stage from frames in memory: stands in for `calculate_removability_scores`
    (elvis.py:968-1224), which runs EVCA and UFO as outside programs over files and then combines their outputs
    (elvis.py:1159-1218).  Here `analyze_frames` gives the SC / TC maps on the device in EVCA's place
    (elvis.py:1014-1055 and the CSV reads of :1160-1170) and `removability_from_complexity` is the reference's own
    combination (elvis.py:1172-1218).  UFO stays outside: `foreground_masks` are its masks, one 2-D array of any size
    (0 = background) or None per frame, or None for no masks at all.  `frames` is a uint8 clip [F,H,W,C] (or a list of
    frames), BGR as the reference holds decoded frames (`order`).  Returns float64 [F, H // block_size,
    W // block_size] in [0, 1], what `apply_selective_removal` and the shrinks take per frame as it is.
    EVCA'S PIXELS ARE NOT REPRODUCED: the maps are the build-defined block complexity of complexity.py;
    what is pinned against the reference's own code is the combination after them."""
    from .complexity import EVCAConfig, analyze_frames, removability_from_complexity
    maps = analyze_frames(frames, EVCAConfig(block_size=block_size), device, order=order, chunk_frames=chunk_frames)
    return removability_from_complexity(maps.SC, maps.TC, foreground_masks, alpha, smoothing_beta)


def calculate_removability_scores_device(frames, block_size: int, alpha: float = 0.5, smoothing_beta: float = 1, device="cuda:0",
                                         *, order: str = "bgr", cfg=None, chunk_frames: Optional[int] = None,
                                         return_masks: bool = False):
    """`calculate_removability_scores_from_frames` with the foreground masks made here too: `segment_frames` in UFO's
    place (elvis.py:1057-1158), then the existing function with those masks - decoded frames to removability scores
    without an outside program.  `cfg`: a `segment.SegmentConfig`.  Returns the scores, float64 [F, H // block_size,
    W // block_size]; with `return_masks=True` the pair (scores, masks uint8 [F,H,W] of 0 / 1).
    THE MASKS ARE NOT UFO'S: the segmenter is build-defined, its defaults untuned and unmeasured on real video
    (segment.py), as the complexity maps are not EVCA's pixels."""
    from .segment import segment_frames
    masks = segment_frames(frames, device, order=order, cfg=cfg, chunk_frames=chunk_frames)
    scores = calculate_removability_scores_from_frames(frames, list(masks), block_size, alpha, smoothing_beta, device, order=order,
                                                       chunk_frames=chunk_frames)
    return (scores, masks) if return_masks else scores


def analyze_clip_file(path: str, width: int, height: int, block_size: int, alpha: float = 0.5, smoothing_beta: float = 1,
                      device="cuda:0", **load_kw):
    """From a source file to removability scores: `intake.load_clip_device(path, width, height, device, **load_kw)` -
    the `.y4m` or raw `.yuv` clip decoded, strided, capped and INTER_AREA-resized to the working size on the device
    (presley.py:177-198) - then `calculate_removability_scores_device` on that clip, in the `order` the clip was loaded
    in ("rgb" unless `load_kw` says otherwise).  `load_kw`: `src_width`, `src_height`, `frame_stride`, `max_frames`,
    `order`, `chunk_frames`.  The working-size clip comes down once: the analysis functions take host clips and upload
    them in their own chunks.  Returns float64 [k, height // block_size, width // block_size]."""
    from .intake import load_clip_device
    clip_d, _ = load_clip_device(path, width, height, device, **load_kw)
    return calculate_removability_scores_device(clip_d.cpu().numpy(), block_size, alpha, smoothing_beta, device,
                                                order=load_kw.get("order", "rgb"))
