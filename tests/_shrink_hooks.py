"""Picklable stand-in for the device step of `drivers.stretch_shrunk_frames` (spawned workers import this module by
name): the numpy restatement, writing the full-resolution masks the way the device step does."""
import os

import numpy as np

import _shrink_ref as R
from elvis_amd import frameio


def stretch_on_host(frames, maps, block_size, device, first_frame_index, fullres_masks_dir=None, **kw):
    out = []
    for i, f in enumerate(frames):
        src_of = R.flat_rank_src_of(maps[i], (f.shape[0] // block_size, f.shape[1] // block_size))
        out.append(R.gather_blocks(f, src_of, block_size))
        if fullres_masks_dir is not None:
            frameio.save_mask(R.fullres_mask(src_of, block_size),
                              os.path.join(fullres_masks_dir, f"{first_frame_index + i + 1:05d}.png"))
    return out
