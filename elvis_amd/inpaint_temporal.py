"""Temporal inpainting of the ELVIS v1 holes on the device: a removed block's content is taken from neighbouring frames
where the same scene point was not removed, and only what no neighbour can give is left to the spatial inpainter.

The slot in the reference, numpy in and numpy out, with a trailing `device`:

  inpaint_with_propainter(frames, masks) / inpaint_with_e2fgvi(frames, masks)    presley.py:854-885  -> inpaint_temporal
  inpaint_propainter / inpaint_e2fgvi                                            utils.py:1395-1425
  inpaint_with_propainter / inpaint_with_e2fgvi (directories, subprocesses)      elvis.py:1458, 1693 -> drivers.restore_shrunk_frames(inpainter="temporal")

and the clip forms on resident tensors (`temporal_fill_device`, `temporal_fill_blocks_device`,
`inpaint_temporal_device`): `[n,H,W,C]` uint8 frames and uint8 masks (non-zero = hole), a whole clip per call.

This is a BUILD-DEFINED inpainter and NEITHER OF THOSE NETWORKS: it is the part of their image
propagation that needs no training, restated in integers.  For every block of a frame that holds a hole, the block and
a margin of context are matched against the frames t-1, t+1, t-2, ... over a small range of displacements (mean absolute
difference over the pixels known in both, compared exactly); the best displacement's known pixels are copied under the
hole.  "Known" is always the input mask and sources are always input bytes, so the result depends on no order and is
the same for every sharding that reads `radius` frames on either side.  tests/_tfill_ref.py states it in numpy; the
kernel (csrc/tfill.hip) equals that bit for bit.  It claims no parity with ProPainter or E2FGVI, its defaults are
untuned and unmeasured on real video, and where the same blocks are removed in every frame of a static scene no
neighbour has what is missing: those holes go to the wavefront Telea of `inpaint.py`.

One launch per clip, no synchronisation, no workspace.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib, ptr
from .ops import _s
from .recompose import frames_to_device

MIN_CONTEXT = 64                       # fewest known pixels of a block's window (a constant of the kernel)
DEFAULTS = dict(block=16, margin=8, radius=2, search=7, max_mad=6)
LIMITS = dict(block=(1, 32), margin=(0, 16), radius=(0, 8), search=(0, 7), max_mad=(0, 255))


def check_params(who: str, **params) -> dict:
    """The parameters of the fill with the defaults filled in, each an integer inside its limits; ValueError otherwise."""
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise ValueError(f"{who}: unknown parameter(s) {sorted(unknown)} (the fill takes {sorted(DEFAULTS)})")
    out = dict(DEFAULTS, **params)
    for name, v in out.items():
        lo, hi = LIMITS[name]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"{who}: {name} must be an integer in {lo}..{hi}, got {v!r}")
        out[name] = int(v)
    return out


def _chk_clip(frames_d, masks_d, mask_shape, mask_dtypes, who: str) -> None:
    """The argument checks of the device forms, all before the library is touched."""
    if not isinstance(frames_d, torch.Tensor) or frames_d.dtype != torch.uint8 or frames_d.dim() != 4 or frames_d.shape[0] < 1:
        raise ValueError(f"{who}: frames must be a [n,H,W,C] uint8 tensor with n >= 1")
    n, h, w, c = frames_d.shape
    if c not in (1, 3):
        raise ValueError(f"{who}: {c} channels (C must be 1 or 3)")
    if h < 1 or w < 1:
        raise ValueError(f"{who}: empty frames {tuple(frames_d.shape)}")
    if not isinstance(masks_d, torch.Tensor) or masks_d.dtype not in mask_dtypes:
        raise ValueError(f"{who}: masks must be a {' / '.join(str(d).replace('torch.', '') for d in mask_dtypes)} tensor")
    if tuple(masks_d.shape) != tuple(mask_shape):
        raise ValueError(f"{who}: masks {tuple(masks_d.shape)} do not match the expected {tuple(mask_shape)}")
    for t in (frames_d, masks_d):
        if not t.is_cuda or t.device != frames_d.device:
            raise ValueError(f"{who}: frames and masks must be CUDA tensors on one device")


def _fill(frames_d: torch.Tensor, masks_d: torch.Tensor, block_mask_size: int, p: dict, who: str) -> Tuple[torch.Tensor, torch.Tensor]:
    n, h, w, c = frames_d.shape
    dev = frames_d.device
    if not lib().elvis_tfill_limits_ok(n, h, w, c, p["block"], p["margin"], p["radius"], p["search"], p["max_mad"]):
        raise ValueError(f"{who}: a [{n},{h},{w},{c}] clip is beyond the kernel's limits (H, W <= 32767, n*H*W*C < 2^31)")
    with torch.cuda.device(dev):
        f = frames_d.contiguous()
        m = masks_d.contiguous().view(torch.uint8)
        out = torch.empty_like(f)                      # never the frames themselves: sources stay input bytes
        left = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
        check(lib().elvis_tfill(ptr(f), ptr(m), block_mask_size, ptr(out), ptr(left), n, h, w, c, p["block"], p["margin"],
                                p["radius"], p["search"], p["max_mad"], _s(f)), dev)
    return out, left


def temporal_fill_device(frames_d: torch.Tensor, masks_d: torch.Tensor, *, block: int = 16, margin: int = 8, radius: int = 2,
                         search: int = 7, max_mad: int = 6) -> Tuple[torch.Tensor, torch.Tensor]:
    """The temporal fill of a resident clip: frames [n,H,W,C] u8 (C in {1, 3}), masks [n,H,W] u8 with non-zero = hole.
    Returns `(out, left)`: a new clip in which the hole pixels a neighbouring frame could give hold that frame's bytes
    (known pixels and the bytes under remaining holes are the input's), and `left` [n,H,W] u8, 255 where a hole stayed
    unfilled and 0 elsewhere - the mask for `inpaint_device`.  The inputs are not written.

    `block`: the fill unit (grid anchored at (0, 0)); `margin`: context around it; `radius`: neighbour frames on each
    side, taken as t-1, t+1, t-2, ...; `search`: displacements -search..search in both directions; `max_mad`: the
    largest accepted mean absolute difference a channel.  A block whose window has fewer than MIN_CONTEXT known pixels
    is left as it is."""
    p = check_params("temporal_fill_device", block=block, margin=margin, radius=radius, search=search, max_mad=max_mad)
    shape = tuple(frames_d.shape[:3]) if isinstance(frames_d, torch.Tensor) and frames_d.dim() == 4 else ()
    _chk_clip(frames_d, masks_d, shape, (torch.uint8,), "temporal_fill_device")
    return _fill(frames_d, masks_d, 0, p, "temporal_fill_device")


def temporal_fill_blocks_device(frames_d: torch.Tensor, block_masks_d: torch.Tensor, block_size: int,
                                **params) -> Tuple[torch.Tensor, torch.Tensor]:
    """`temporal_fill_device` with removal masks [n,By,Bx] (bool / int8 / uint8, non-zero = removed) expanded over whole
    blocks of `block_size`, as `inpaint_blocks_device` takes them; pixels past the last whole block are known.  The
    fill's own `block` is independent of `block_size`."""
    p = check_params("temporal_fill_blocks_device", **params)
    if isinstance(block_size, bool) or not isinstance(block_size, (int, np.integer)) or block_size < 1:
        raise ValueError("block_size must be an integer >= 1")
    b = int(block_size)
    if isinstance(frames_d, torch.Tensor) and frames_d.dim() == 4:
        shape = (frames_d.shape[0], frames_d.shape[1] // b, frames_d.shape[2] // b)
    else:
        shape = ()
    _chk_clip(frames_d, block_masks_d, shape, (torch.bool, torch.int8, torch.uint8), "temporal_fill_blocks_device")
    if shape[1] == 0 or shape[2] == 0:                 # no whole block: nothing is a hole
        return frames_d.clone(memory_format=torch.contiguous_format), torch.zeros(tuple(frames_d.shape[:3]), dtype=torch.uint8,
                                                                                   device=frames_d.device)
    return _fill(frames_d, block_masks_d, b, p, "temporal_fill_blocks_device")


def inpaint_temporal_device(frames_d: torch.Tensor, masks_d: torch.Tensor, **params) -> torch.Tensor:
    """Every hole of a resident clip filled: `temporal_fill_device`, then `inpaint_device` (the wavefront Telea) on what
    is left, in place on the fill's result - Telea reads the temporally filled pixels as known.  Returns a new clip."""
    from .inpaint import inpaint_device
    out, left = temporal_fill_device(frames_d, masks_d, **check_params("inpaint_temporal_device", **params))
    return inpaint_device(out, left, out=out)


def inpaint_temporal(frames: Union[np.ndarray, Sequence[np.ndarray]], masks, device="cuda:0", **params) -> np.ndarray:
    """The call surface of Presley's `inpaint_with_propainter(frames, masks)` / `inpaint_with_e2fgvi(frames, masks)`
    (presley.py:854-885; `utils.inpaint_propainter` / `inpaint_e2fgvi`), as `inpaint_with_opencv` takes its arguments:
    frames [n,H,W,C] uint8 (an array or a list of frames), masks [n,By,Bx] bool with True = removed; the block size is
    H // By.  Returns an np.ndarray of the frames' shape.

    It is NEITHER ProPainter NOR E2FGVI and claims no parity with them: the build-defined temporal fill of this module
    followed by the wavefront Telea.  `params`: block, margin, radius, search, max_mad of `temporal_fill_device`."""
    from .inpaint import inpaint_device
    p = check_params("inpaint_temporal", **params)
    fs = np.asarray(frames)
    ms = np.asarray(masks)
    if fs.dtype != np.uint8 or fs.ndim != 4 or fs.shape[0] < 1 or fs.shape[3] not in (1, 3):
        raise ValueError("inpaint_temporal: frames are a uint8 [n,H,W,C] array (or a list of equal frames), C in {1, 3}")
    if ms.ndim != 3 or ms.shape[0] != fs.shape[0] or ms.dtype.kind not in "biu" or ms.shape[1] < 1 or ms.shape[2] < 1:
        raise ValueError(f"inpaint_temporal: masks are [n,By,Bx] bool for {fs.shape[0]} frame(s); got {ms.shape}")
    b = fs.shape[1] // ms.shape[1]
    if b < 1 or fs.shape[1] != ms.shape[1] * b or fs.shape[2] != ms.shape[2] * b:
        raise ValueError(f"inpaint_temporal: {fs.shape[1]}x{fs.shape[2]} frames are not a {ms.shape[1]}x{ms.shape[2]} grid of "
                         "whole square blocks")
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        fd = frames_to_device([fs[i] for i in range(fs.shape[0])], dev)
        md = torch.from_numpy(np.ascontiguousarray(ms != 0).view(np.uint8)).to(dev)
        out, left = temporal_fill_blocks_device(fd, md, b, **p)
        return inpaint_device(out, left, out=out).cpu().numpy()
