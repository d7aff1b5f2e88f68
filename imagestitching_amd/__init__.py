"""imagestitching_amd — MI355X-native strip stitcher (the Canvas-2D concatenation path of Iamctb/ImageStitching).

Everything that touches pixels is hand-written HIP behind the C-ABI in include/imagestitch.h
(imagestitching_amd/libimagestitch.so).  Importing this package fails if that library has not been built.
"""
from ._lib import (FILTER_BILINEAR, FILTER_NEAREST, HORIZONTAL, VERTICAL, StitchError, last_error)  # noqa: F401
from .stitch import (DEFAULT_OPTS, Bitmap, GroupJob, StitchGroup, Stitcher, StitchJob, StitchPlan, decode_files_device, decode_image, decode_png, encode_png, encode_png_batch_device, encode_png_device, encode_jpeg, encode_jpeg_device, encode_jpeg_batch_device, stitch_jpeg, stitch_jpeg_batch, image_info, last_phase_times, plan, set_phase_timing,  # noqa: F401
                     launch_jobs, stitch, stitch_batch, stitch_files, stitch_png, stitch_png_batch, decode_bitmaps, upload_bitmap, preview_device, preview_fit, thumbnail_layout, thumbnails, thumbnails_device, debug_cells, debug_png_grid, debug_jpeg_gpu_coefficients, scaled_size, decode_scale_fit, thumbnails_from_files, find_overlaps, find_overlaps_device, overlap_rows, crop_overlaps, image_color, icc_tables, convert_color_device, jpeg_join_check, join_jpeg)

__all__ = ["stitch", "stitch_batch", "launch_jobs", "stitch_png", "stitch_png_batch", "encode_png", "encode_png_device", "encode_png_batch_device", "encode_jpeg", "encode_jpeg_device", "stitch_jpeg", "decode_png", "decode_image", "decode_files_device", "image_info", "set_phase_timing", "last_phase_times", "stitch_files", "decode_bitmaps", "upload_bitmap", "preview_device", "preview_fit", "thumbnail_layout", "thumbnails", "thumbnails_device", "thumbnails_from_files", "find_overlaps", "find_overlaps_device", "overlap_rows", "crop_overlaps", "image_color", "icc_tables", "convert_color_device", "jpeg_join_check", "join_jpeg", "scaled_size", "decode_scale_fit", "debug_cells", "debug_png_grid", "debug_jpeg_gpu_coefficients", "Bitmap", "plan", "Stitcher", "StitchGroup", "GroupJob", "StitchJob", "StitchPlan", "StitchError",
           "DEFAULT_OPTS"]
