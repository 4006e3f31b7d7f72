"""What the two Real-ESRGAN networks (`realesrgan.RRDBNetModel`, `srvgg.SRVGGModel`) share on the host: the weight
packing in front of the 3x3 tile of csrc/sr_conv3x3.h, and a model's buffer cache, input checks and grouping loop."""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np
import torch

from . import _lib as L


def pack_conv(net: str, w_oihw: torch.Tensor, bias: torch.Tensor, pad_cout: bool):
    """(packed f16 weights as a uint16 numpy array, fp32 bias of the kernel's cout, cin, cout) of one conv, by
    `elvis_<net>_packed_weight_bytes` and `elvis_<net>_pack_weights` on the host.  The input channels are padded to a
    multiple of 32 with zeros, and with `pad_cout` the output channels and the bias too."""
    w = np.ascontiguousarray(w_oihw.detach().to("cpu", torch.float32).numpy())
    cout_real, cin_real = w.shape[:2]
    cin = (cin_real + 31) // 32 * 32
    cout = (cout_real + 31) // 32 * 32 if pad_cout else cout_real
    lib = L.lib()
    nbytes = getattr(lib, f"elvis_{net}_packed_weight_bytes")(cin, cout)
    if nbytes == 0:
        raise ValueError(f"no {net.upper()} conv kernel for {cin_real} -> {cout_real} channels")
    packed = np.empty(nbytes // 2, dtype=np.uint16)
    L.check(getattr(lib, f"elvis_{net}_pack_weights")(w.ctypes.data_as(C.c_void_p), cin_real, cout_real, cin, cout,
                                                      packed.ctypes.data_as(C.c_void_p)))
    b = np.zeros(cout, dtype=np.float32)
    b[:cout_real] = bias.detach().to("cpu", torch.float32).numpy()
    return packed, b, cin, cout


class SRModel:
    """A packed f16 network on one device.  A subclass sets `scale` and gives
    `_forward_batch(lr, swap_rb, as_float)`, `_alloc_buffers(n, h, w)` and `_lr_pixels(H, W)`; its module holds
    `MAX_INVOCATION_BYTES` and `BYTES_PER_LR_PIXEL`, read at call time."""

    def __init__(self, device):
        self.device = L.resolve_device(device)
        self.dtype = torch.float16
        self._bufs = None

    def _buffers(self, n: int, h: int, w: int):
        key = (n, h, w)
        if self._bufs is None or self._bufs[0] != key:
            self._bufs = None   # free the previous shape's buffers first
            self._bufs = (key, self._alloc_buffers(n, h, w))
        return self._bufs[1]

    def max_batch(self, H: int, W: int) -> int:
        """Frames of H x W one invocation takes: capped by the bytes of its activations."""
        mod = sys.modules[type(self).__module__]
        return max(1, mod.MAX_INVOCATION_BYTES // (mod.BYTES_PER_LR_PIXEL * self._lr_pixels(H, W)))

    def forward(self, lr_u8_d: torch.Tensor, swap_rb: bool = True, as_float: bool = False) -> torch.Tensor:
        """[n,h,w,3] uint8 on the device -> [n,s*h,s*w,3] uint8 on the device (s = `scale`).  `swap_rb`: the frames
        are BGR (the reference's decoded frames); the network sees RGB and the output is BGR again.  `as_float`: the
        f16 output before `clamp * 255, round`, for tests.  Frames go through in groups capped by bytes; every kernel
        is per-sample, so the result does not depend on the grouping."""
        name = type(self).__name__
        if lr_u8_d.dtype != torch.uint8 or lr_u8_d.dim() != 4 or lr_u8_d.shape[-1] != 3:
            raise ValueError(f"{name}.forward takes [n,h,w,3] uint8, got {tuple(lr_u8_d.shape)} {lr_u8_d.dtype}")
        if lr_u8_d.device != self.device:
            raise ValueError(f"{name}.forward: frames on {lr_u8_d.device}, model on {self.device}")
        n, H, W, _ = lr_u8_d.shape
        s = self.scale
        if n == 0 or H == 0 or W == 0:
            return torch.empty((n, s * H, s * W, 3), dtype=torch.float16 if as_float else torch.uint8, device=self.device)
        lr = lr_u8_d.contiguous()
        step = self.max_batch(H, W)
        with torch.cuda.device(self.device):
            outs = [self._forward_batch(lr[i:i + step], swap_rb, as_float) for i in range(0, n, step)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)
