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

import ctypes as C
from typing import List

import numpy as np
import torch

from . import _lib as L
from .weights import SRVGGConfig, load_srvgg_state_dict, make_srvgg_weights

# device bytes one low-resolution pixel of one frame costs inside `forward`: the 32-channel input, two 64-channel
# buffers, and 16 output pixels of 3 channels (f16 for the float output)
BYTES_PER_LR_PIXEL = 2 * (32 + 64 + 64) + 16 * 3 * 2
MAX_INVOCATION_BYTES = 12 << 30


def pack_conv(w_oihw: torch.Tensor, bias: torch.Tensor):
    """(packed f16 weights as a uint16 numpy array, fp32 bias, cin, cout) of one conv: `elvis_srvgg_pack_weights` on
    the host, input channels padded to a multiple of 32 with zeros."""
    w = np.ascontiguousarray(w_oihw.detach().to("cpu", torch.float32).numpy())
    cout, cin_real = w.shape[:2]
    cin = (cin_real + 31) // 32 * 32
    lib = L.lib()
    nbytes = lib.elvis_srvgg_packed_weight_bytes(cin, cout)
    if nbytes == 0:
        raise ValueError(f"no SRVGG conv kernel for {cin_real} -> {cout} channels")
    packed = np.empty(nbytes // 2, dtype=np.uint16)
    L.check(lib.elvis_srvgg_pack_weights(w.ctypes.data_as(C.c_void_p), cin_real, cout, cin, cout,
                                         packed.ctypes.data_as(C.c_void_p)))
    b = np.ascontiguousarray(bias.detach().to("cpu", torch.float32).numpy())
    return packed, b, cin, cout


class _Layer:
    __slots__ = ("w", "b", "a", "cin", "cout")

    def __init__(self, w_oihw, bias, slope, device):
        packed, b, self.cin, self.cout = pack_conv(w_oihw, bias)
        self.w = torch.from_numpy(packed.view(np.int16)).to(device)
        self.b = torch.from_numpy(b).to(device)
        self.a = None if slope is None else slope.detach().to(device, torch.float32).contiguous()   # fp32, not rounded


class SRVGGModel:
    """The packed network on one device, with the interface of `realesrgan.RRDBNetModel`.  `state_dict` is a checked
    dict (`load_srvgg_state_dict`), a path, a checkpoint dict, or None for the seeded synthetic weights (`weight_seed`)."""

    def __init__(self, cfg: SRVGGConfig = SRVGGConfig(), state_dict=None, device="cuda:0", weight_seed: int = 0):
        self.cfg = cfg
        self.device = L.resolve_device(device)
        self.dtype = torch.float16
        self.scale = cfg.upscale
        sd = make_srvgg_weights(cfg, weight_seed) if state_dict is None else load_srvgg_state_dict(state_dict, cfg)
        last = cfg.num_conv + 1
        with torch.cuda.device(self.device):
            self.layers: List[_Layer] = [
                _Layer(sd[f"body.{2 * i}.weight"], sd[f"body.{2 * i}.bias"],
                       None if i == last else sd[f"body.{2 * i + 1}.weight"], self.device) for i in range(last + 1)]
        self._bufs = None

    def _buffers(self, n: int, h: int, w: int):
        key = (n, h, w)
        if self._bufs is None or self._bufs[0] != key:
            self._bufs = None   # free the previous shape's buffers first
            f16 = dict(dtype=torch.float16, device=self.device)
            self._bufs = (key, (torch.empty((n, h, w, 32), **f16), torch.empty((n, h, w, 64), **f16),
                                torch.empty((n, h, w, 64), **f16)))
        return self._bufs[1]

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

    def max_batch(self, H: int, W: int) -> int:
        """Frames of H x W one invocation takes: capped by the bytes of its activations."""
        return max(1, MAX_INVOCATION_BYTES // (BYTES_PER_LR_PIXEL * H * W))

    def forward(self, lr_u8_d: torch.Tensor, swap_rb: bool = True, as_float: bool = False) -> torch.Tensor:
        """[n,h,w,3] uint8 on the device -> [n,4h,4w,3] uint8 on the device.  `swap_rb`: the frames are BGR (the
        reference's decoded frames); the network sees RGB and the output is BGR again.  `as_float`: the f16 sum of the
        shuffled last conv and the base before `clamp * 255, round`, for tests.  Frames go through in groups capped by
        bytes; every kernel is per-sample, so the result does not depend on the grouping."""
        if lr_u8_d.dtype != torch.uint8 or lr_u8_d.dim() != 4 or lr_u8_d.shape[-1] != 3:
            raise ValueError(f"SRVGGModel.forward takes [n,h,w,3] uint8, got {tuple(lr_u8_d.shape)} {lr_u8_d.dtype}")
        if lr_u8_d.device != self.device:
            raise ValueError(f"SRVGGModel.forward: frames on {lr_u8_d.device}, model on {self.device}")
        n, H, W, _ = lr_u8_d.shape
        if n == 0 or H == 0 or W == 0:
            return torch.empty((n, 4 * H, 4 * W, 3), dtype=torch.float16 if as_float else torch.uint8, device=self.device)
        lr = lr_u8_d.contiguous()
        step = self.max_batch(H, W)
        with torch.cuda.device(self.device):
            outs = [self._forward_batch(lr[i:i + step], swap_rb, as_float) for i in range(0, n, step)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)
