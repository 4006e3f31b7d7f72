"""elvis_amd - MI355X-native implementation of ELVIS's client-side restoration hot path.

Drop-in for the reference's `elvis.py` / `utils.py` call surface: the names
below keep the reference's spelling, argument meaning and error behaviour; the arithmetic runs
as hand-written HIP (gfx950) kernels in `elvis_amd/lib/libelvis_amd.so` behind the C ABI of
`include/elvis_amd.h`.  There is no CPU fallback: without a ROCm GPU (or without the built
library) the restoration entry points raise RuntimeError.
"""
from .sharding import (ChunkSpec, chunk_for_devices, parallel_process_frames, rank_frame_range,  # noqa: F401
                       resolve_device_list, _resolve_device_list)
from .recompose import (combine_blocks_into_image, split_image_into_blocks,  # noqa: F401
                        restore_video_adaptively)
from .tiler import (adaptive_restore, blended_restoration, resource_aware_restore,  # noqa: F401
                    _extract_tile_with_halo, extract_tile_with_halo)
from .frameio import (clear_directory, decode_strength_maps_from_npz, encode_strength_maps_to_npz,  # noqa: F401
                      get_frame_paths, load_block_masks, load_frame, load_strength_maps, save_block_masks, save_frame, save_mask)
from .degrade import (blur_block, degrade_adaptive_blur, degrade_adaptive_downsample, degrade_frame,  # noqa: F401
                      degrade_gaussian_fx_device, degrade_scale_device, degrade_video_adaptive, downscale_block,
                      filter_frame_dct, filter_frame_downsample, filter_frame_gaussian, generate_degradation_map)
from .handoff import (calculate_importance_scores, convert_frames_to_yuv420p, create_kvazaar_roi_file,  # noqa: F401
                      create_svtav1_roi_file, kvazaar_delta_qp, rgb_to_i420_device, svtav1_delta_qp, write_y4m)
from .handoff import (Y4MInfo, i420_to_rgb_device, load_y4m_device, load_yuv420p_device, parse_y4m, read_y4m)  # noqa: F401
from .handoff import encode_with_roi_device, roi_levels_from_importance  # noqa: F401
from .classical import (lanczos_restore_device, restore_blur_opencv_unsharp_mask,  # noqa: F401
                        restore_downsample_opencv_lanczos, restore_with_opencv_lanczos, restore_with_opencv_unsharp,
                        temporal_blend_device, unsharp_restore_device)
from .metrics import calculate_block_ssim, calculate_mse, calculate_psnr, masked_mse, masked_psnr  # noqa: F401
from .metrics import (apply_binary_mask, calculate_foreground_metric, calculate_ssim, compute_fg_bg_ssim,  # noqa: F401
                      compute_mask_union_bbox, evaluate_fg_bg_metrics, masked_ssim, masked_ssim_device)
from .shrink import (apply_selective_removal, block_gather_device, shrink_frame_position_map,  # noqa: F401
                     shrink_frame_removal_indices, shrink_frame_row_only, shrink_passes_device, shrink_topk_device,
                     shrink_video_frames, stretch_device, stretch_frame, stretch_frame_position_map,
                     stretch_frame_removal_indices, stretch_frame_row_only, stretch_index_device, stretch_video_frames)
from .inpaint import (inpaint_blocks_device, inpaint_device, inpaint_frame, inpaint_with_opencv,  # noqa: F401
                      stretch_and_inpaint_device)
from .inpaint_temporal import (inpaint_temporal, inpaint_temporal_device, temporal_fill_blocks_device,  # noqa: F401
                               temporal_fill_device)
from .complexity import (BlockComplexity, EVCAConfig, analyze_frames, block_complexity_device,  # noqa: F401
                         removability_from_complexity, resize_masks_nearest)
from .lpips import (LpipsAlex, calculate_lpips, calculate_lpips_per_frame, get_lpips_model,  # noqa: F401
                    load_lpips_state_dict, lpips_device)
from .vmaf import (VmafModel, calculate_vmaf, calculate_vmaf_frames, get_vmaf_model, load_vmaf_model, luma_device,  # noqa: F401
                   make_vmaf_model, vmaf_device, vmaf_features_device, vmaf_stats)
from .fvmd import (FvmdConfig, FvmdNoTrajectories, calculate_fvmd, calculate_fvmd_device, frechet_distance_device,  # noqa: F401
                   fvmd_device, motion_features_device, track_keypoints_device)
from .png import decode_png_device, encode_png_device, load_frames_device, save_frames, save_frames_device  # noqa: F401
from .jpeg import decode_jpeg_device, load_images_device, load_jpeg_frames_device, parse_jpeg  # noqa: F401
from .jpeg_write import (JPEG_ROI_MAX_LEVEL, encode_jpeg_device, jpeg_encoded_sizes_device, jpeg_file_header, jpeg_quality_for_bytes,  # noqa: F401
                         jpeg_optimal_tables, jpeg_quant_tables, jpeg_restart_interval, jpeg_roi_levels, jpeg_roi_scale16, jpeg_roundtrip_at_bytes_device,
                         jpeg_roundtrip_device, save_jpeg_frames, save_jpeg_frames_device)
from .segment import SegmentConfig, foreground_masks_device, save_foreground_masks, segment_frames  # noqa: F401
from .drivers import calculate_removability_scores_device  # noqa: F401
from .drivers import (calculate_removability_scores_from_frames, restore_blur_adaptive, restore_dct_adaptive,  # noqa: F401
                      restore_downsampled_with_sinsr, restore_shrunk_frames, restore_yuv_clip, stretch_shrunk_frames)
from .restore import (get_sinsr_model, get_sinsr_upsample_fn, restore_frames_blur, restore_frames_blur_device,  # noqa: F401
                      restore_frames_dct, restore_frames_dct_device, restore_frames_rounds, restore_frames_sinsr,
                      restore_frames_sinsr_device, restore_with_sinsr_naive)
from .restore import (get_realesrgan_upsample_fn, get_realesrgan_upsampler, restore_frames_realesrgan,  # noqa: F401
                      restore_frames_realesrgan_device, restore_with_realesrgan_naive)
from .drivers import restore_downsampled_with_realesrgan  # noqa: F401
from .enhance import (RealESRGANer, lanczos4_resize_taps, plan_tiles, reflect_index_maps, resize_lanczos4_device,  # noqa: F401
                      upscale_with_realesrgan)
from .intake import (intake_device, load_clip_device, resize_area, resize_area_device, resize_area_plan,  # noqa: F401
                     resize_masks_nearest_device, resize_nearest_device)
from .drivers import analyze_clip_file  # noqa: F401
from .weights import RRDBNetConfig, load_realesrgan_state_dict  # noqa: F401
from .weights import SRVGGConfig, dni_state_dicts, load_srvgg_state_dict  # noqa: F401

__version__ = "0.1.0"
