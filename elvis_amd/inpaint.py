"""The ELVIS v1 inpaint step on the device: the holes a stretch leaves are filled with Telea's estimator.

The reference's call surface, numpy in and numpy out, with a trailing `device`:

  cv2.inpaint(stretched_frame, mask, inpaintRadius=3, flags=cv2.INPAINT_TELEA)   elvis.py:4601-4606  -> inpaint_frame
  inpaint_with_opencv(frames, masks)                                             presley.py:838-850

and the clip forms on resident tensors (`inpaint_device`, `inpaint_blocks_device`, `stretch_and_inpaint_device`):
`[n,H,W,C]` uint8 frames and uint8 masks (non-zero = hole), a whole clip per call.

This is a BUILD-DEFINED inpainter ("wavefront Telea"), like the DCT slot: it takes the reference's call
surface, radius 3 and Telea's weights, on a fill order a GPU can run (waves by exact Euclidean distance, every wave
computed from known pixels and earlier waves only).  It does not claim parity with cv2.  tests/_inpaint_ref.py states
it in numpy; the kernels (csrc/inpaint.hip) equal that bit for bit.

Synchronisation: one per clip.  The number of fill launches is the deepest wave of the clip, which only the device
knows after the preparation pass, so `inpaint_device` downloads the per-wave pixel counts (h + w + 2 int32) once -
a blocking copy on the current stream - and then queues one fill launch per non-empty wave.  A clip without holes
launches no fill kernel.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib, ptr
from .ops import _s
from .recompose import frames_to_device


def _chk_clip(frames_d, masks_d, mask_shape, mask_dtypes, out, who: str) -> torch.Tensor:
    """The argument checks of the device forms (all before the library is touched); returns the output tensor."""
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
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != tuple(frames_d.shape):
            raise ValueError(f"{who}: out must be a uint8 tensor of the frames' shape {tuple(frames_d.shape)}")
        if not out.is_contiguous():
            raise ValueError(f"{who}: out must be contiguous")
    for t in (frames_d, masks_d) + (() if out is None else (out,)):
        if not t.is_cuda or t.device != frames_d.device:
            raise ValueError(f"{who}: frames, masks and out must be CUDA tensors on one device")
    if out is None:
        return frames_d.clone(memory_format=torch.contiguous_format)
    if out.data_ptr() != frames_d.data_ptr() or not frames_d.is_contiguous():
        out.copy_(frames_d)
    return out


def _inpaint(out: torch.Tensor, masks_d: torch.Tensor, block_size: int) -> torch.Tensor:
    n, h, w, c = out.shape
    dev = out.device
    nbytes = lib().elvis_inpaint_workspace_bytes(n, h, w)
    if nbytes == 0:
        raise ValueError(f"inpaint: a [{n},{h},{w}] clip is beyond the kernels' limits (H, W <= 32767, n*H*W < 2^31)")
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        m = masks_d.contiguous().view(torch.uint8)
        check(lib().elvis_inpaint_prepare(ptr(m), block_size, ptr(ws), n, h, w, _s(out)), dev)
        # the one synchronisation of a clip: how many waves there are, and how many pixels each has
        counts = ws[:(h + w + 2) * 4].view(torch.int32).cpu().numpy()
        filled = np.flatnonzero(counts)
        if filled.size:
            k = int(filled[-1])
            host = np.ascontiguousarray(counts[:k + 1], dtype=np.int32)
            check(lib().elvis_inpaint_fill(ptr(out), ptr(ws), n, h, w, c, host.ctypes.data_as(C.c_void_p), k + 1, _s(out)), dev)
    return out


def inpaint_device(frames_d: torch.Tensor, masks_d: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fill the holes of a resident clip: frames [n,H,W,C] u8 (C in {1, 3}), masks [n,H,W] u8 with non-zero = hole,
    as for cv2.inpaint.  The bytes under the holes are ignored, known pixels are never written; a frame without a hole
    or without a known pixel comes back as it is.  `out` may be `frames_d` itself (in place).  Returns `out`."""
    if isinstance(frames_d, torch.Tensor) and frames_d.dim() == 4:
        shape = tuple(frames_d.shape[:3])
    else:
        shape = ()
    return _inpaint(_chk_clip(frames_d, masks_d, shape, (torch.uint8,), out, "inpaint_device"), masks_d, 0)


def inpaint_blocks_device(frames_d: torch.Tensor, block_masks_d: torch.Tensor, block_size: int,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`inpaint_device` with removal masks [n,By,Bx] (bool / int8 / uint8, non-zero = removed) expanded over whole
    blocks, as `stretch_device(..., fullres_mask=True)` writes them; pixels past the last whole block are known."""
    if int(block_size) != block_size or block_size < 1:
        raise ValueError("block_size must be an integer >= 1")
    b = int(block_size)
    if isinstance(frames_d, torch.Tensor) and frames_d.dim() == 4:
        shape = (frames_d.shape[0], frames_d.shape[1] // b, frames_d.shape[2] // b)
    else:
        shape = ()
    out = _chk_clip(frames_d, block_masks_d, shape, (torch.bool, torch.int8, torch.uint8), out, "inpaint_blocks_device")
    if shape[1] == 0 or shape[2] == 0:
        return out                                           # no whole block: nothing is a hole
    return _inpaint(out, block_masks_d, b)


def stretch_and_inpaint_device(shrunk_d: torch.Tensor, masks_d: torch.Tensor, block_size: int, mode: str = "flat") -> torch.Tensor:
    """The v1 client path on resident tensors: `stretch_device` with its full-resolution mask, then the inpaint in
    place on the stretched clip.  Nothing but the per-wave counts leaves the device."""
    from .shrink import stretch_device
    stretched, full = stretch_device(shrunk_d, masks_d, block_size, mode, fullres_mask=True)
    return inpaint_device(stretched, full, out=stretched)


# ----------------------------------------------------------------------------- the reference's call surface
def inpaint_frame(stretched_frame: np.ndarray, mask_img: np.ndarray, device="cuda:0") -> np.ndarray:
    """The cv2.inpaint(stretched_frame, mask_img, 3, cv2.INPAINT_TELEA) call of elvis.py:4605 (module docstring: the
    build-defined wavefront Telea, not cv2's bytes).  One HxWxC (or HxW) uint8 frame, one HxW uint8 mask."""
    f = np.asarray(stretched_frame)
    m = np.asarray(mask_img)
    if f.dtype != np.uint8 or f.ndim not in (2, 3) or (f.ndim == 3 and f.shape[2] not in (1, 3)):
        raise ValueError("inpaint_frame: the frame is a uint8 (H,W), (H,W,1) or (H,W,3) array")
    if m.dtype != np.uint8 or m.shape != f.shape[:2]:
        raise ValueError(f"inpaint_frame: the mask is a uint8 {f.shape[:2]} array; got {m.dtype} {m.shape}")
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        fd = torch.from_numpy(np.ascontiguousarray(f.reshape(f.shape[0], f.shape[1], -1)[None])).to(dev)
        md = torch.from_numpy(np.ascontiguousarray(m[None])).to(dev)
        return inpaint_device(fd, md, out=fd)[0].cpu().numpy().reshape(f.shape)


def inpaint_with_opencv(frames: Union[np.ndarray, Sequence[np.ndarray]], masks, device="cuda:0") -> np.ndarray:
    """presley.py:838-850: frames [n,H,W,3] (an array or a list of frames), masks [n,By,Bx] bool with True = removed;
    the block size is H // By.  Returns an np.ndarray of the frames' shape."""
    fs = np.asarray(frames)
    ms = np.asarray(masks)
    if fs.dtype != np.uint8 or fs.ndim != 4 or fs.shape[0] < 1 or fs.shape[3] not in (1, 3):
        raise ValueError("inpaint_with_opencv: frames are a uint8 [n,H,W,C] array (or a list of equal frames), C in {1, 3}")
    if ms.ndim != 3 or ms.shape[0] != fs.shape[0] or ms.dtype.kind not in "biu" or ms.shape[1] < 1 or ms.shape[2] < 1:
        raise ValueError(f"inpaint_with_opencv: masks are [n,By,Bx] bool for {fs.shape[0]} frame(s); got {ms.shape}")
    # the reference resizes the mask to the frame with INTER_NEAREST: on whole blocks that is the block expansion
    b = fs.shape[1] // ms.shape[1]
    if b < 1 or fs.shape[1] != ms.shape[1] * b or fs.shape[2] != ms.shape[2] * b:
        raise ValueError(f"inpaint_with_opencv: {fs.shape[1]}x{fs.shape[2]} frames are not a {ms.shape[1]}x{ms.shape[2]} grid of "
                         "whole square blocks")
    dev = L.resolve_device(device)
    with torch.cuda.device(dev):
        fd = frames_to_device([fs[i] for i in range(fs.shape[0])], dev)
        md = torch.from_numpy(np.ascontiguousarray(ms != 0).view(np.uint8)).to(dev)
        return inpaint_blocks_device(fd, md, b, out=fd).cpu().numpy()
