"""Picklable stand-in for the device step of `drivers.restore_shrunk_frames` (spawned workers import this module by
name): the numpy restatements of the stretch and of the inpaint, writing the stretched frames and the
full-resolution masks the way the device step does."""
import os

import numpy as np

import _inpaint_ref as I
import _shrink_ref as R
from elvis_amd import frameio


def restore_on_host(frames, maps, block_size, device, first_frame_index, stretched_dir=None, fullres_masks_dir=None, **kw):
    out = []
    for i, f in enumerate(frames):
        name = f"{first_frame_index + i + 1:05d}.png"
        src_of = R.flat_rank_src_of(maps[i], (f.shape[0] // block_size, f.shape[1] // block_size))
        stretched = R.gather_blocks(f, src_of, block_size)
        full = R.fullres_mask(src_of, block_size)
        if stretched_dir is not None:
            frameio.save_frame(stretched, os.path.join(stretched_dir, name))
        if fullres_masks_dir is not None:
            frameio.save_mask(full, os.path.join(fullres_masks_dir, name))
        out.append(I.inpaint_frame(stretched, full))
    return out
