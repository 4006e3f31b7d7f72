"""ctypes binding of libelvis_amd.so (the C ABI declared in include/elvis_amd.h).

The product path has NO CPU fallback: if the shared object is missing or fails to load,
`lib()` raises RuntimeError.  Error codes from the C side are mapped to the reference's
exception conventions: ELVIS_E_INVALID -> ValueError, everything else ->
RuntimeError carrying the device label.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
# ELVIS_AMD_LIB: alternative build of the same library (kernel A/B experiments, tools/build_variant.py)
LIBPATH = os.environ.get("ELVIS_AMD_LIB") or os.path.join(HERE, "lib", "libelvis_amd.so")

F32, F16 = 0, 1
ROUND_CV2, ROUND_HALF_UP = 0, 1
SSIM_LUMA, SSIM_CHANNELS = 0, 1
SSIM_REFLECT, SSIM_VALID = 0, 1
SSIM_PAD_AUTO = -1

_lock = threading.Lock()
_lib: Optional[C.CDLL] = None

vp, i32, f32, i64, f64 = C.c_void_p, C.c_int, C.c_float, C.c_longlong, C.c_double


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "dtype", "n", "h", "w", "cin", "cin_pitch", "cin2", "cin2_pitch", "cout", "cout_pitch",
        "ksize", "stride", "pad_before", "upsample", "ho", "wo", "act", "prologue", "subpixel")]


# name -> argtypes (every symbol include/elvis_amd.h declares; checked by tests/test_cabi.py)
SIGNATURES = {
    "elvis_abi_version": [],
    "elvis_last_error": [],
    "elvis_last_launch": [],
    "elvis_recompose_u8": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "elvis_area_downscale_u8": [vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "elvis_blend_u8": [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, vp],
    "elvis_select_levels_u8": [vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "elvis_tile_accumulate_f32": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, vp],
    "elvis_tile_normalize_u8": [vp, vp, vp, i32, i32, i32, vp],
    "elvis_sse_u8": [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "elvis_block_ssim_u8": [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp],
    "elvis_mask_bbox_u8": [vp, vp, i32, i32, i32, vp],
    "elvis_apply_mask_u8": [vp, vp, vp, i32, i32, i32, i32, i32, vp],
    "elvis_ssim_workspace_bytes": [i32, i32, i32, i32],
    "elvis_ssim_mean_f64": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f64, f64, f64, i32, f64, vp],
    "elvis_u8_to_float": [vp, vp, i32, i32, i32, i32, i32, f32, f32, i32, i32, vp],
    "elvis_float_to_u8": [vp, i32, vp, vp, i32, i32, i32, i32, f32, f32, i32, i32, vp],
    "elvis_conv_packed_weight_bytes": [C.POINTER(ConvDesc)],
    "elvis_conv_pack_weights": [C.POINTER(ConvDesc), vp, vp, vp],
    "elvis_conv2d": [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp],
    "elvis_conv_stats_tiles": [C.POINTER(ConvDesc)],
    "elvis_conv_kernel_name": [C.POINTER(ConvDesc), C.c_char_p, C.c_size_t],
    "elvis_conv_kernel_name_for_call": [C.POINTER(ConvDesc), i32, i32, C.c_char_p, C.c_size_t],
    "elvis_conv_x3_eligible": [C.POINTER(ConvDesc)],
    "elvis_conv_debug_set": [C.c_char_p, i32],
    "elvis_gn_partials_to_sums": [vp, i32, i32, i32, vp, i32, i32, vp],
    "elvis_groupnorm_workspace_floats": [i32, i32, i32, i32],
    "elvis_groupnorm_sums": [vp, i32, i32, i32, i32, i32, vp, i32, i32, vp, vp],
    "elvis_groupnorm_affine": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, vp],
    "elvis_gn_partials_affine_span": [i32, i32],
    "elvis_gn_partials_affine": [vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, vp],
    "elvis_affine_act": [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp],
    "elvis_layernorm": [vp, vp, i32, i64, i32, i32, i32, vp, vp, f32, vp],
    "elvis_swin_packed_bytes": [i32, i32, i32],
    "elvis_swin_pack_weights": [vp, vp, vp, i32, i32, i32, vp],
    "elvis_swin_mlp": [vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, f32, vp],
    "elvis_swin_ln_linear": [vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, f32, vp],
    "elvis_swin_pack_proj_mlp": [vp, vp, vp, vp, i32, i32, vp],
    "elvis_swin_proj_mlp": [vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, f32, vp],
    "elvis_window_attention": [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, f32, vp],
    "elvis_bicubic_upsample": [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "elvis_vq_nearest": [vp, vp, vp, i32, i64, i32, i32, i32, vp, i32, vp],
    "elvis_vq_index_bytes": [i32, i32],
    "elvis_vq_index_build": [vp, i32, i32, vp, vp],
    "elvis_vq_nearest_indexed": [vp, vp, vp, i32, i64, i32, i32, i32, vp, i32, vp, vp],
    "elvis_pad_reflect_axpy": [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, f32, vp, f32, vp],
    "elvis_crop_copy": [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "elvis_convert_act": [vp, i32, vp, i32, i64, i32, vp],
    "elvis_degrade_downsample_u8": [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "elvis_degrade_gaussian_u8": [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, f32, f32, vp],
    "elvis_degrade_dct_u8": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "elvis_degrade_scale_u8": [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp],
    "elvis_degrade_gaussian_fx_u8": [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "elvis_rgb_to_i420_u8": [vp, vp, i32, i32, i32, i32, vp],
    "elvis_i420_to_rgb_u8": [vp, vp, i32, i32, i32, i32, vp],
    "elvis_classical_lanczos_u8": [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp],
    "elvis_classical_unsharp_u8": [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp],
    "elvis_temporal_blend_u8": [vp, vp, i32, i64, f64, f64, vp],
    "elvis_block_gather_u8": [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "elvis_shrink_select_topk": [vp, vp, vp, i32, i32, i32, i32, vp],
    "elvis_shrink_passes_plan": [i32, i32, i32, i32, vp, vp, vp, i32],
    "elvis_shrink_select_passes": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "elvis_stretch_index": [vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "elvis_inpaint_workspace_bytes": [i32, i32, i32],
    "elvis_inpaint_prepare": [vp, i32, vp, i32, i32, i32, vp],
    "elvis_inpaint_fill": [vp, vp, i32, i32, i32, i32, vp, i32, vp],
    "elvis_tfill_limits_ok": [i32, i32, i32, i32, i32, i32, i32, i32, i32],
    "elvis_tfill": [vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "elvis_segment_workspace_bytes": [i32, i32, i32, i32],
    "elvis_segment_foreground_u8": [vp, vp, i32, vp, i32, vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32,
                                    i32, i32, vp],
    "elvis_block_complexity_f64": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "elvis_lpips_stem_u8": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "elvis_lpips_conv5_f32": [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp],
    "elvis_lpips_maxpool_f32": [vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "elvis_lpips_distance_workspace_bytes": [i32, i32, i32],
    "elvis_lpips_distance_f64": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "elvis_vmaf_luma_u8": [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "elvis_vmaf_workspace_bytes": [i32, i32, i32],
    "elvis_vmaf_features_f64": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp],
    "elvis_vmaf_predict_f64": [vp, vp, vp, i32, i32, i32, vp],
    "elvis_fvmd_pyramid_bytes": [i32, i32, i32],
    "elvis_fvmd_pyramid_f64": [vp, vp, i32, i32, i32, vp],
    "elvis_fvmd_track_f64": [vp, vp, vp, i32, i32, i32, i32, i32, vp],
    "elvis_fvmd_features_f64": [vp, vp, i32, i32, vp],
    "elvis_fvmd_gram_workspace_bytes": [i32, i32, i32],
    "elvis_fvmd_gram_f64": [vp, vp, vp, vp, vp, i32, i32, i32, vp],
    "elvis_fvmd_singular_values_f64": [vp, vp, i32, i32, vp],
    "elvis_fvmd_finish_f64": [vp, vp, vp, i32, i32, i32, vp],
    "elvis_png_stats": [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "elvis_png_pack": [vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, vp],
    "elvis_png_stats_rle": [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "elvis_png_pack_rle": [vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, vp],
    "elvis_png_gather": [vp, i64, vp, i32, vp, i64, vp, vp],
    "elvis_png_inflate": [vp, i64, vp, vp, i64, vp, vp, i32, vp],
    "elvis_png_unfilter": [vp, i64, vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "elvis_jpeg_entropy": [vp, i64, vp, i32, vp, i32, vp, vp, vp, vp, i64, vp, vp],
    "elvis_jpeg_idct": [vp, i64, vp, i32, vp, vp],
    "elvis_jpeg_colour": [vp, i64, vp, vp, i32, i32, i32, i32, i32, vp],
    "elvis_jpeg_frame_blocks": [i32, i32, i32, i32],
    "elvis_jpeg_fdct": [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "elvis_jpeg_fdct_roi": [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, i32, i32, i32, vp],
    "elvis_jpeg_bits": [vp, vp, vp, i32, i32, i32, i32, i32, vp],
    "elvis_jpeg_pack": [vp, vp, vp, vp, vp, i64, vp, i32, vp, i32, i32, i32, i32, i32, vp],
    "elvis_jpeg_stuff": [vp, vp, vp, i64, vp, i32, vp, vp, i64, i32, i32, i32, i32, i32, vp],
    "elvis_jpeg_segments": [i32, i32, i32, i32, i32],
    "elvis_jpeg_bits_rst": [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "elvis_jpeg_pack_rst": [vp, vp, vp, vp, vp, i64, vp, i32, vp, i32, i32, i32, i32, i32, i32, vp],
    "elvis_jpeg_stuff_rst": [vp, vp, vp, i64, vp, i32, vp, vp, i64, i32, i32, i32, i32, i32, i32, vp],
    "elvis_jpeg_tally": [vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "elvis_jpeg_optimal_tables": [vp, i32, i32, vp, vp, vp, vp],
    "elvis_jpeg_bits_ftab": [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "elvis_jpeg_pack_ftab": [vp, vp, vp, vp, vp, i64, vp, i32, vp, i32, i32, i32, i32, i32, i32, vp],
    "elvis_rrdb_packed_weight_bytes": [i32, i32],
    "elvis_rrdb_pack_weights": [vp, i32, i32, i32, i32, vp],
    "elvis_rrdb_conv3x3": [vp, i32, vp, vp, vp, i32, i32, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, f32, f32, i32, i32, vp],
    "elvis_rrdb_input_u8": [vp, vp, i32, i32, i32, i32, i32, vp],
    "elvis_srvgg_packed_weight_bytes": [i32, i32],
    "elvis_srvgg_pack_weights": [vp, i32, i32, i32, i32, vp],
    "elvis_srvgg_conv3x3": [vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp],
    "elvis_srvgg_tail": [vp, i32, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, vp],
    "elvis_resize_lanczos4_u8": [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp],
    "elvis_resize_lanczos4_lds_bytes": [vp, vp, i32, i32, i32, i32, i32, i32, i32],
    "elvis_sr_gather_tiles_u8": [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp],
    "elvis_sr_paste_tiles_u8": [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp],
    "elvis_resize_area_u8": [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "elvis_resize_nearest_u8": [vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "elvis_dcnv2": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "elvis_temporal_stack": [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "elvis_plane_merge": [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
}


def lib() -> C.CDLL:
    """Load (once) and return the shared library; fail loudly when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIBPATH):
            raise RuntimeError(
                f"libelvis_amd.so not found at {LIBPATH}. Build it with `python -m elvis_amd._build` "
                "(needs hipcc). There is no CPU fallback for the restoration path.")
        # torch must be imported first so that libamdhip64.so.7 resolves to the HIP runtime torch
        # already loaded (same SONAME) - streams and device pointers are then shared.
        import torch  # noqa: F401
        try:
            handle = C.CDLL(LIBPATH)
        except OSError as exc:
            raise RuntimeError(f"failed to load {LIBPATH}: {exc}") from exc
        for name, argtypes in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.argtypes = argtypes
            fn.restype = C.c_int
        handle.elvis_last_error.restype = C.c_char_p
        handle.elvis_last_launch.restype = C.c_char_p
        handle.elvis_conv_packed_weight_bytes.restype = C.c_size_t
        handle.elvis_groupnorm_workspace_floats.restype = C.c_size_t
        handle.elvis_swin_packed_bytes.restype = C.c_size_t
        handle.elvis_vq_index_bytes.restype = C.c_size_t
        handle.elvis_ssim_workspace_bytes.restype = C.c_size_t
        handle.elvis_inpaint_workspace_bytes.restype = C.c_size_t
        handle.elvis_lpips_distance_workspace_bytes.restype = C.c_size_t
        handle.elvis_segment_workspace_bytes.restype = C.c_size_t
        handle.elvis_rrdb_packed_weight_bytes.restype = C.c_size_t
        handle.elvis_srvgg_packed_weight_bytes.restype = C.c_size_t
        handle.elvis_vmaf_workspace_bytes.restype = C.c_size_t
        handle.elvis_fvmd_pyramid_bytes.restype = C.c_size_t
        handle.elvis_fvmd_gram_workspace_bytes.restype = C.c_size_t
        if handle.elvis_abi_version() != 1:
            raise RuntimeError("libelvis_amd.so ABI version mismatch")
        _lib = handle
    return _lib


def check(rc: int, device=None) -> None:
    if rc == 0:
        return
    msg = lib().elvis_last_error().decode("utf-8", "replace")
    if rc == -1:
        raise ValueError(msg)
    label = str(device) if device is not None else "unknown device"
    raise RuntimeError(f"elvis_amd kernel failed on {label}: {msg}")


def ptr(t) -> int:
    """Device pointer of a torch tensor (None -> NULL)."""
    return 0 if t is None else t.data_ptr()


def stream_handle(device=None) -> int:
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def require_gpu(device) -> None:
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(
            f"elvis_amd runs on MI355X only (got device '{dev}'); there is no CPU path in the product. "
            "Use the reference implementation on CPU.")
    if not torch.cuda.is_available():
        raise RuntimeError("no ROCm GPU visible to torch; elvis_amd cannot run")


def resolve_device(device):
    """The torch.device of a `device=` argument ("cuda" is "cuda:0"), checked by `require_gpu`."""
    import torch
    dev = torch.device("cuda:0" if str(device) == "cuda" else device)
    require_gpu(dev)
    return dev


def dtype_code(torch_dtype) -> int:
    import torch
    if torch_dtype == torch.float32:
        return F32
    if torch_dtype == torch.float16:
        return F16
    raise ValueError(f"unsupported dtype {torch_dtype}")
