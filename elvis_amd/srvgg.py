"""Real-ESRGAN's SRVGGNetCompact on the MI355X: the network `RealESRGANer.enhance` (elvis.py:2515) runs for the model
names `realesr-animevideov3` and `realesr-general-x4v3` of the reference's table (elvis.py:2431-2441), f16 with fp32
accumulation - the reference's own GPU precision (`half=True`, elvis.py:2480).  Every layer is `elvis_srvgg_conv3x3`,
the last conv with all that follows it is `elvis_srvgg_tail` (csrc/srvgg.hip).

    x     = the RGB image / 255
    feat  = prelu(conv(x))                          3 -> 64, one slope per channel
    feat  = prelu(conv(feat))                       num_conv times, 64 -> 64
    out   = pixel_shuffle(conv(feat), 4) + nearest4x(x)      64 -> 48; then clamp to [0, 1], * 255, round half to even

The input stage is `elvis_rrdb_input_u8` with s = 1 (a 32-channel buffer, channels past 2 zero), which is also the
base the tail adds: the stored f16 pixel.  The layers ping-pong two 64-channel buffers.  What is pinned is the float64
statement of this network (tests/_srvgg_ref.py); cv2's Lanczos4 in `enhance(outscale=2)` and the outputs of the trained
checkpoints are not.

Without a state dict the weights are SEEDED AND SYNTHETIC (`weights.make_srvgg_weights`): they exercise the network
and restore nothing.  The trained checkpoints load through `weights.load_srvgg_state_dict`; `denoise_strength` blends
two of them with `weights.dni_state_dicts` before they come here (restore.get_realesrgan_upsampler); nothing is
downloaded.
"""
from __future__ import annotations

from typing import List

import numpy as np
import torch

from . import _lib as L
from ._srnet import SRModel, pack_conv as _pack_conv
from .weights import SRVGGConfig, load_srvgg_state_dict, make_srvgg_weights

# device bytes one low-resolution pixel of one frame costs inside `forward`: the 32-channel input, two 64-channel
# buffers, and 16 output pixels of 3 channels (f16 for the float output)
BYTES_PER_LR_PIXEL = 2 * (32 + 64 + 64) + 16 * 3 * 2
MAX_INVOCATION_BYTES = 12 << 30


def pack_conv(w_oihw: torch.Tensor, bias: torch.Tensor):
    """(packed f16 weights as a uint16 numpy array, fp32 bias, cin, cout) of one conv: `elvis_srvgg_pack_weights` on
    the host, input channels padded to a multiple of 32 with zeros."""
    return _pack_conv("srvgg", w_oihw, bias, pad_cout=False)


class _Layer:
    __slots__ = ("w", "b", "a", "cin", "cout")

    def __init__(self, w_oihw, bias, slope, device):
        packed, b, self.cin, self.cout = pack_conv(w_oihw, bias)
        self.w = torch.from_numpy(packed.view(np.int16)).to(device)
        self.b = torch.from_numpy(b).to(device)
        self.a = None if slope is None else slope.detach().to(device, torch.float32).contiguous()   # fp32, not rounded


class SRVGGModel(SRModel):
    """The packed network on one device, with the interface of `realesrgan.RRDBNetModel`.  `state_dict` is a checked
    dict (`load_srvgg_state_dict`), a path, a checkpoint dict, or None for the seeded synthetic weights (`weight_seed`).
    `forward` (`SRModel.forward`) scales by 4; its `as_float` gives the f16 sum of the shuffled last conv and the base."""

    def __init__(self, cfg: SRVGGConfig = SRVGGConfig(), state_dict=None, device="cuda:0", weight_seed: int = 0):
        super().__init__(device)
        self.cfg = cfg
        self.scale = cfg.upscale
        sd = make_srvgg_weights(cfg, weight_seed) if state_dict is None else load_srvgg_state_dict(state_dict, cfg)
        last = cfg.num_conv + 1
        with torch.cuda.device(self.device):
            self.layers: List[_Layer] = [
                _Layer(sd[f"body.{2 * i}.weight"], sd[f"body.{2 * i}.bias"],
                       None if i == last else sd[f"body.{2 * i + 1}.weight"], self.device) for i in range(last + 1)]

    def _alloc_buffers(self, n: int, h: int, w: int):
        f16 = dict(dtype=torch.float16, device=self.device)
        return torch.empty((n, h, w, 32), **f16), torch.empty((n, h, w, 64), **f16), torch.empty((n, h, w, 64), **f16)

    def _forward_batch(self, lr: torch.Tensor, swap_rb: bool, as_float: bool) -> torch.Tensor:
        n, h, w, _ = lr.shape
        x0, a, b = self._buffers(n, h, w)
        lib, stream = L.lib(), L.stream_handle(self.device)
        L.check(lib.elvis_rrdb_input_u8(lr.data_ptr(), x0.data_ptr(), n, h, w, 1, int(swap_rb), stream), self.device)
        src = x0
        for layer in self.layers[:-1]:
            dst = b if src is a else a
            L.check(lib.elvis_srvgg_conv3x3(src.data_ptr(), src.shape[-1], layer.w.data_ptr(), layer.b.data_ptr(),
                                            layer.a.data_ptr(), dst.data_ptr(), 64, n, h, w, layer.cin, stream), self.device)
            src = dst
        tail = self.layers[-1]
        out = torch.empty((n, 4 * h, 4 * w, 3), dtype=torch.float16 if as_float else torch.uint8, device=self.device)
        L.check(lib.elvis_srvgg_tail(src.data_ptr(), 64, tail.w.data_ptr(), tail.b.data_ptr(), x0.data_ptr(), 32,
                                     out.data_ptr(), n, h, w, int(not as_float), int(swap_rb), stream), self.device)
        return out

    def _lr_pixels(self, H: int, W: int) -> int:
        return H * W
