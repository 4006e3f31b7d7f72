"""Real-ESRGAN's RRDBNet on the MI355X: the network `RealESRGANer.enhance` runs in the reference's Downsample slot
(`restore_frames_realesrgan` -> `_instantiate_realesrgan_upsampler`, elvis.py:2384-2519), f16 with fp32 accumulation -
the reference's own GPU precision (`half=True`, elvis.py:2480).  Every conv is `elvis_rrdb_conv3x3` (csrc/rrdb.hip).

    feat  = conv_first(x)                     x: the image / 255, for scale 2 pixel-unshuffled by 2 (12 channels)
    body  : num_block RRDBs; an RRDB is three dense blocks and `out * 0.2 + x`; a dense block is
            x1 = lrelu(conv1(x)), x2 = lrelu(conv2(x, x1)), ... x5 = conv5(x, x1..x4), `x5 * 0.2 + x`
    feat  = feat + conv_body(body(feat))
    feat  = lrelu(conv_up1(nearest2x(feat))); feat = lrelu(conv_up2(nearest2x(feat)))
    out   = conv_last(lrelu(conv_hr(feat)))   then clamp to [0, 1], * 255, round half to even (`enhance`)

A dense block lives in one [n,h,w,192] buffer: the input in channels [0, 64), x1..x4 appended in place by the convs'
channel offset, no concat.  Three such buffers rotate through the three dense blocks of an RRDB, so that the RRDB's own
input is still there for its tail, which is folded into the third block's conv5: `0.04 x5 + 0.2 x_rdb3 + x_rrdb`, written
over x_rrdb.  What is pinned is the float64 statement of this network (tests/_rrdb_ref.py); cv2's Lanczos4 in
`enhance(outscale=...)` and the outputs of the trained checkpoints are not.

Without a state dict the weights are SEEDED AND SYNTHETIC (`weights.make_rrdbnet_weights`): they exercise the network
and restore nothing.  The trained checkpoints (`RealESRGAN_x4plus.pth`, ...) load through
`weights.load_realesrgan_state_dict`; nothing is downloaded.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from ._srnet import SRModel, pack_conv as _pack_conv
from .weights import RRDBNetConfig, load_realesrgan_state_dict, make_rrdbnet_weights, rrdbnet_layout

# device bytes one low-resolution pixel of one frame costs inside `forward`: three 192-channel buffers, the 64-channel
# features and the 32-channel input at h x w, 64 channels at 2h x 2w, two times 64 (and 32 for the float output) at 4h x 4w
BYTES_PER_LR_PIXEL = 2 * (3 * 192 + 64 + 32) + 4 * 2 * 64 + 16 * 2 * (64 + 64 + 32)
MAX_INVOCATION_BYTES = 12 << 30


def pack_conv(w_oihw: torch.Tensor, bias: torch.Tensor):
    """(packed f16 weights as a uint16 numpy array, fp32 bias padded to the kernel's cout, cin, cout) of one conv:
    `elvis_rrdb_pack_weights` on the host, input and output channels padded to multiples of 32 with zeros."""
    return _pack_conv("rrdb", w_oihw, bias, pad_cout=True)


class _Conv:
    __slots__ = ("w", "b", "cin", "cout")

    def __init__(self, w_oihw, bias, device):
        packed, b, self.cin, self.cout = pack_conv(w_oihw, bias)
        self.w = torch.from_numpy(packed.view(np.int16)).to(device)
        self.b = torch.from_numpy(b).to(device)


class RRDBNetModel(SRModel):
    """The packed network on one device.  `state_dict` is a checked dict (`load_realesrgan_state_dict`), a path, a
    checkpoint dict, or None for the seeded synthetic weights (`weight_seed`).  `forward` (`SRModel.forward`) scales by
    `cfg.scale`; its `as_float` gives the f16 output of conv_last."""

    def __init__(self, cfg: RRDBNetConfig = RRDBNetConfig(), state_dict=None, device="cuda:0", weight_seed: int = 0):
        super().__init__(device)
        self.cfg = cfg
        self.scale = cfg.scale
        sd = make_rrdbnet_weights(cfg, weight_seed) if state_dict is None else load_realesrgan_state_dict(state_dict, cfg)
        with torch.cuda.device(self.device):
            self.convs: Dict[str, _Conv] = {key: _Conv(sd[key + ".weight"], sd[key + ".bias"], self.device)
                                            for key, _, _ in rrdbnet_layout(cfg)}

    # ------------------------------------------------------------------ plumbing
    def _conv(self, key: str, x: torch.Tensor, out: torch.Tensor, n: int, h: int, w: int, *, out_coff: int = 0,
              upsample: bool = False, lrelu: bool = False, s0: float = 1.0, s1: float = 0.0, r1=None, r2=None,
              out_u8: bool = False, swap_rb: bool = False, cin: Optional[int] = None) -> None:
        cv = self.convs[key]
        L.check(L.lib().elvis_rrdb_conv3x3(
            x.data_ptr(), x.shape[-1], cv.w.data_ptr(), cv.b.data_ptr(), out.data_ptr(), out.shape[-1], out_coff,
            L.ptr(r1), 0 if r1 is None else r1.shape[-1], L.ptr(r2), 0 if r2 is None else r2.shape[-1],
            n, h, w, cv.cin if cin is None else cin, cv.cout, int(upsample), int(lrelu), s0, s1, int(out_u8), int(swap_rb),
            L.stream_handle(self.device)), self.device)

    def _alloc_buffers(self, n: int, h: int, w: int):
        f16 = dict(dtype=torch.float16, device=self.device)
        return dict(
            x0=torch.empty((n, h, w, 32), **f16),
            dense=[torch.empty((n, h, w, 192), **f16) for _ in range(3)],
            feat=torch.empty((n, h, w, 64), **f16),
            up1=torch.empty((n, 2 * h, 2 * w, 64), **f16),
            up2=torch.empty((n, 4 * h, 4 * w, 64), **f16),
            hr=torch.empty((n, 4 * h, 4 * w, 64), **f16))

    def _dense_block(self, prefix: str, src: torch.Tensor, dst: torch.Tensor, n, h, w, *, tail_of: Optional[torch.Tensor] = None):
        """One dense block on `src` ([n,h,w,192], input in channels [0, 64)): x1..x4 appended in place, then
        `x5 * 0.2 + x` into channels [0, 64) of `dst`.  `tail_of` (the RRDB's input buffer, which is `dst`) folds the
        RRDB tail in: `0.04 x5 + 0.2 x + x_rrdb`."""
        for c in range(1, 5):
            self._conv(f"{prefix}.conv{c}", src, src, n, h, w, out_coff=32 + 32 * c, lrelu=True)
        if tail_of is None:
            self._conv(f"{prefix}.conv5", src, dst, n, h, w, s0=0.2, r2=src)
        else:
            self._conv(f"{prefix}.conv5", src, dst, n, h, w, s0=0.04, s1=0.2, r1=src, r2=tail_of)

    def _forward_batch(self, lr: torch.Tensor, swap_rb: bool, as_float: bool) -> torch.Tensor:
        n, H, W, _ = lr.shape
        s_in = 2 if self.cfg.scale == 2 else 1
        h, w = (H + s_in - 1) // s_in, (W + s_in - 1) // s_in
        B = self._buffers(n, h, w)
        a, b, c = B["dense"]
        L.check(L.lib().elvis_rrdb_input_u8(lr.data_ptr(), B["x0"].data_ptr(), n, H, W, s_in, int(swap_rb),
                                            L.stream_handle(self.device)), self.device)
        self._conv("conv_first", B["x0"], B["feat"], n, h, w)
        a[..., :64].copy_(B["feat"])
        for i in range(self.cfg.num_block):
            self._dense_block(f"body.{i}.rdb1", a, b, n, h, w)
            self._dense_block(f"body.{i}.rdb2", b, c, n, h, w)
            self._dense_block(f"body.{i}.rdb3", c, a, n, h, w, tail_of=a)
        self._conv("conv_body", a, B["feat"], n, h, w, r2=B["feat"])          # feat + conv_body(body(feat)), in place
        self._conv("conv_up1", B["feat"], B["up1"], n, h, w, upsample=True, lrelu=True)
        self._conv("conv_up2", B["up1"], B["up2"], n, 2 * h, 2 * w, upsample=True, lrelu=True)
        self._conv("conv_hr", B["up2"], B["hr"], n, 4 * h, 4 * w, lrelu=True)
        if as_float:
            out = torch.empty((n, 4 * h, 4 * w, 32), dtype=torch.float16, device=self.device)
            self._conv("conv_last", B["hr"], out, n, 4 * h, 4 * w)
            out = out[..., :3]
            if swap_rb:
                out = out.flip(-1)
        else:
            out = torch.empty((n, 4 * h, 4 * w, 3), dtype=torch.uint8, device=self.device)
            self._conv("conv_last", B["hr"], out, n, 4 * h, 4 * w, out_u8=True, swap_rb=swap_rb)
        s = self.cfg.scale
        if out.shape[1] != s * H or out.shape[2] != s * W:      # an odd size went in with one reflected row / column
            out = out[:, :s * H, :s * W]
        return out.contiguous()

    def _lr_pixels(self, H: int, W: int) -> int:
        s_in = 2 if self.cfg.scale == 2 else 1
        return ((H + s_in - 1) // s_in) * ((W + s_in - 1) // s_in)
