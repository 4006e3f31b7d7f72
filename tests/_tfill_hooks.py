"""Picklable stand-in for the device step of `drivers.restore_shrunk_frames(inpainter="temporal")` (spawned workers
import this module by name): the numpy restatements of the stretch, of the temporal fill and of the wavefront Telea,
writing the stretched frames and the full-resolution masks of the worker's own frames the way the device step does."""
import os

import numpy as np

import _inpaint_ref as I
import _shrink_ref as R
import _tfill_ref as T
from elvis_amd import frameio


def restore_on_host(frames, maps, block_size, device, first_frame_index, stretched_dir=None, fullres_masks_dir=None,
                    inpainter="telea", inpaint_params=None, own=None, **kw):
    assert inpainter == "temporal" and own is not None
    a, b = own[0] - first_frame_index, own[1] - first_frame_index
    stretched, full = [], []
    for i, f in enumerate(frames):
        src_of = R.flat_rank_src_of(maps[i], (f.shape[0] // block_size, f.shape[1] // block_size))
        stretched.append(R.gather_blocks(f, src_of, block_size))
        full.append(R.fullres_mask(src_of, block_size))
        if a <= i < b:
            name = f"{first_frame_index + i + 1:05d}.png"
            for d in (stretched_dir, fullres_masks_dir):
                if d is not None:                      # a second write of the same file, by any worker, fails here
                    os.makedirs(d + "_once", exist_ok=True)
                    os.close(os.open(os.path.join(d + "_once", name), os.O_CREAT | os.O_EXCL | os.O_WRONLY))
            if stretched_dir is not None:
                frameio.save_frame(stretched[-1], os.path.join(stretched_dir, name))
            if fullres_masks_dir is not None:
                frameio.save_mask(full[-1], os.path.join(fullres_masks_dir, name))
    out, left = T.temporal_fill(np.stack(stretched), np.stack(full), **inpaint_params)
    out[a:b] = I.inpaint(out[a:b], left[a:b])
    return [out[i] for i in range(len(frames))]
