"""ctypes binding of libicelk.so -- the thin shim between the Python host code and the HIP kernels.

Signatures mirror include/icelk.h one to one.  There is no CPU fallback: if the library is missing
or no GPU is present the calls raise.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ICELK_LIBRARY: another build of this same library (A/B measurements of kernel variants: tools/build_variant.sh)
LIB_PATH = os.environ.get("ICELK_LIBRARY") or os.path.join(_HERE, "libicelk.so")

OK, EARG, ENOMEM, EHIP, ECAP, ESTATE, EUNSUP = 0, -1, -2, -3, -4, -5, -6

u8p = C.POINTER(C.c_uint8)
f32p = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int)
i64p = C.POINTER(C.c_int64)
f64p = C.POINTER(C.c_double)
vp = C.c_void_p
handle_p = C.c_void_p
i16p = C.POINTER(C.c_int16)


class JpegInfo(C.Structure):
    """icelk_jpeg_info_t of include/icelk.h"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("ncomp", C.c_int32), ("hmax", C.c_int32), ("vmax", C.c_int32),
                ("mcus_x", C.c_int32), ("mcus_y", C.c_int32), ("restart_interval", C.c_int32),
                ("comp_w", C.c_int32 * 3), ("comp_h", C.c_int32 * 3), ("blocks_x", C.c_int32 * 3), ("blocks_y", C.c_int32 * 3),
                ("coef_offset", C.c_uint64 * 3), ("coef_count", C.c_uint64), ("quant", (C.c_uint16 * 64) * 3)]


jpeg_info_p = C.POINTER(JpegInfo)


class JpegScan(C.Structure):
    """icelk_jpeg_scan_t"""
    _fields_ = [("segments", C.c_uint32), ("blocks_per_mcu", C.c_uint32), ("blocks_per_segment", C.c_uint32),
                ("total_blocks", C.c_uint32), ("component", C.c_uint8 * 8), ("dc_table", C.c_uint8 * 8), ("ac_table", C.c_uint8 * 8)]


class JpegHuffStats(C.Structure):
    """icelk_jpeg_huff_stats_t"""
    _fields_ = [("segments", C.c_uint32), ("subsequences", C.c_uint32), ("rounds", C.c_uint32), ("max_hops", C.c_uint32),
                ("lanes_in_step", C.c_uint32), ("spanning_blocks", C.c_uint32), ("fallback", C.c_uint32), ("reserved", C.c_uint32),
                ("total_hops", C.c_uint64)]


class JpegCropStats(C.Structure):
    """icelk_jpeg_crop_stats_t"""
    _fields_ = [("huff", JpegHuffStats), ("route", C.c_uint32), ("blocks", C.c_uint32), ("budget", C.c_uint64), ("stream_len", C.c_uint64)]


class GridStats(C.Structure):
    """icelk_grid_stats_t: six host float64 arrays laid out as mean_u is"""
    _fields_ = [(k, f64p) for k in ("std_u", "std_v", "median_u", "median_v", "mad_u", "mad_v")]


grid_stats_p = C.POINTER(GridStats)


class Boxes(C.Structure):
    """icelk_boxes_t: nboxes polygons, box b's vertices at xy[2 * offset[b]] .. xy[2 * offset[b + 1])"""
    _fields_ = [("xy", f64p), ("offset", i32p), ("nboxes", C.c_int)]


boxes_p = C.POINTER(Boxes)


class DayTables(C.Structure):
    """icelk_day_tables_t: the file and window tables of icelk_grid_bin_windows"""
    _fields_ = [("file_offset", i64p), ("file_cam", i32p), ("win_f0", i32p), ("win_f1", i32p), ("nfiles", C.c_int),
                ("t_lo", i64p), ("t_hi", i64p), ("ncam", C.c_int), ("nw", C.c_int)]


day_tables_p = C.POINTER(DayTables)


class MapPanel(C.Structure):
    """icelk_map_panel_t"""
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("bar_x0", C.c_int32), ("bar_w", C.c_int32),
                ("xmin", C.c_double), ("xmax", C.c_double), ("ymin", C.c_double), ("ymax", C.c_double),
                ("cells", C.c_void_p), ("measured", C.c_void_p), ("n_cells", C.c_int32), ("n_outline", C.c_int32),
                ("outline", C.c_void_p), ("arrows", C.c_void_p), ("n_arrows", C.c_int32), ("resident", C.c_int32),
                ("group", C.c_int32), ("pivot", C.c_int32), ("width", C.c_double), ("alpha", C.c_double), ("vmax", C.c_double),
                ("cameras", C.c_void_p), ("n_cameras", C.c_int32), ("reserved", C.c_int32)]


class MapText(C.Structure):
    """icelk_map_text_t"""
    _fields_ = [("px", C.c_int32), ("py", C.c_int32), ("text", C.c_char * 56)]


class MapDesc(C.Structure):
    """icelk_map_desc_t"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("n_panels", C.c_int32), ("n_texts", C.c_int32), ("quality", C.c_int32),
                ("reserved", C.c_int32), ("panel", MapPanel * 2), ("text", MapText * 16), ("table", C.c_void_p)]


map_desc_p = C.POINTER(MapDesc)


class MapInset(C.Structure):
    """icelk_map_inset_t"""
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("index", C.c_int32), ("label_px", C.c_int32), ("label_py", C.c_int32),
                ("reserved", C.c_int32), ("label", C.c_char * 56)]


class MapInsetPixels(C.Structure):
    """icelk_map_inset_pixels_t"""
    _fields_ = [("rgb", C.c_void_p), ("w", C.c_int32), ("h", C.c_int32), ("stride", C.c_int32), ("reserved", C.c_int32)]


map_inset_p = C.POINTER(MapInset)
MAP_INSETS_MAX = 8


class OrthoRaster(C.Structure):
    """icelk_ortho_raster_t"""
    _fields_ = [("x0", C.c_double), ("y0", C.c_double), ("res", C.c_double), ("width", C.c_int), ("height", C.c_int)]


class OrthoOpts(C.Structure):
    """icelk_ortho_opts_t"""
    _fields_ = [("max_range", C.c_double), ("sampling", C.c_int), ("fill", C.c_uint8 * 3)]


ortho_raster_p = C.POINTER(OrthoRaster)
ortho_opts_p = C.POINTER(OrthoOpts)
ORTHO_MAX_INDEX = 254



class StabParams(C.Structure):
    """icelk_stab_params_t"""
    _fields_ = [("model", C.c_int), ("rounds", C.c_int), ("min_anchors", C.c_int), ("reserved", C.c_int), ("threshold", C.c_double),
                ("start_gate", C.c_double), ("min_spread", C.c_double)]


stab_params_p = C.POINTER(StabParams)
STAB_TOO_FEW, STAB_LOST, STAB_DEGENERATE, STAB_NOT_CONVERGED = 1, 2, 4, 8
STAB_MAX_VERTICES = 17

class ValidateLattice(C.Structure):
    """icelk_validate_lattice_t"""
    _fields_ = [("left", C.c_double), ("top", C.c_double), ("side", C.c_double), ("cols", C.c_int), ("rows", C.c_int)]


class ValidateParams(C.Structure):
    """icelk_validate_params_t"""
    _fields_ = [("threshold", C.c_double), ("eps", C.c_double), ("min_neighbours", C.c_int), ("reserved", C.c_int)]


class ValidateCells(C.Structure):
    """icelk_validate_cells_t: five host arrays per (group, cell)"""
    _fields_ = [("pool_n", i32p), ("med_u", f64p), ("med_v", f64p), ("mad_u", f64p), ("mad_v", f64p)]


validate_lattice_p = C.POINTER(ValidateLattice)
validate_params_p = C.POINTER(ValidateParams)
validate_cells_p = C.POINTER(ValidateCells)
VALIDATE_KEPT, VALIDATE_REJECTED, VALIDATE_FEW_NEIGHBOURS, VALIDATE_NOT_JUDGED = 0, 1, 2, 3


class DriftLattice(C.Structure):
    """icelk_drift_lattice_t"""
    _fields_ = [("x0", C.c_double), ("y0", C.c_double), ("dx", C.c_double), ("dy", C.c_double), ("rows", C.c_int), ("cols", C.c_int)]


class DriftParams(C.Structure):
    """icelk_drift_params_t"""
    _fields_ = [("step", C.c_double), ("nsteps", C.c_int), ("every", C.c_int), ("order", C.c_int), ("min_nodes", C.c_int)]


class DriftOut(C.Structure):
    """icelk_drift_out_t: host arrays"""
    _fields_ = [(k, f64p) for k in ("x", "y", "last_x", "last_y", "length")] + [(k, i32p) for k in ("status", "stop_step", "visits")]


drift_lattice_p = C.POINTER(DriftLattice)
drift_params_p = C.POINTER(DriftParams)
drift_out_p = C.POINTER(DriftOut)
DRIFT_ALIVE, DRIFT_LEFT, DRIFT_TOO_FEW, DRIFT_NO_FIELD, DRIFT_NEVER_RELEASED = 0, 1, 2, 3, 4

JPEG_CROP_ROUTES =("device", "host-huffman", "over-budget")   # ICELK_JPEG_CROP_*
JPEG_TABLE_BYTES = 11328
JPEG_FALLBACK_NONE, JPEG_FALLBACK_BOUND, JPEG_FALLBACK_STREAM, JPEG_FALLBACK_SIZE = 0, 1, 2, 3
jpeg_stats_p = C.POINTER(JpegHuffStats)

# name -> (restype, argtypes); the single source of truth for the symbol-export test as well
SIGNATURES = {
    "icelk_version": (C.c_int, []),
    "icelk_last_error": (C.c_char_p, [handle_p]),
    "icelk_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(handle_p)]),
    "icelk_destroy": (C.c_int, [handle_p]),
    "icelk_set_stream": (C.c_int, [handle_p, vp]),
    "icelk_sync": (C.c_int, [handle_p]),
    "icelk_set_fb_distance": (C.c_int, [handle_p, C.c_int]),
    "icelk_set_lk_kernel": (C.c_int, [handle_p, C.c_int]),
    "icelk_upload_gray": (C.c_int, [handle_p, C.c_int, u8p, C.c_int, C.c_int, C.c_int]),
    "icelk_upload_bgr": (C.c_int, [handle_p, C.c_int, u8p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "icelk_jpeg_describe": (C.c_int, [vp, C.c_uint64, jpeg_info_p]),
    "icelk_jpeg_read_coefficients": (C.c_int, [vp, C.c_uint64, vp, C.c_uint64]),
    "icelk_upload_jpeg": (C.c_int, [handle_p, C.c_int, jpeg_info_p, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "icelk_jpeg_decode_rgb": (C.c_int, [handle_p, jpeg_info_p, vp, u8p, C.c_int]),
    "icelk_jpeg_index": (C.c_int, [vp, C.c_uint64, jpeg_info_p, C.POINTER(JpegScan), vp, vp, C.c_uint64, vp]),
    "icelk_jpeg_read_coefficients_lanes": (C.c_int, [vp, C.c_uint64, vp, C.c_uint64, C.c_int, C.c_int, C.c_int, jpeg_stats_p]),
    "icelk_jpeg_huff_config": (C.c_int, [handle_p, C.c_int, C.c_int, C.c_int]),
    "icelk_jpeg_huff_stats": (C.c_int, [handle_p, jpeg_stats_p]),
    "icelk_upload_jpeg_file": (C.c_int, [handle_p, C.c_int, vp, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "icelk_upload_jpeg_file_async": (C.c_int, [handle_p, C.c_int, vp, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "icelk_jpeg_async_poll": (C.c_int, [handle_p, C.c_int, C.POINTER(C.c_int)]),
    "icelk_jpeg_async_finish": (C.c_int, [handle_p, C.c_int, jpeg_stats_p]),
    "icelk_jpeg_decode_rgb_file": (C.c_int, [handle_p, vp, C.c_uint64, u8p, C.c_int]),
    "icelk_jpeg_device_coefficients": (C.c_int, [handle_p, vp, C.c_uint64, vp, C.c_uint64]),
    "icelk_jpeg_resave_tables": (C.c_int, [C.c_int, vp, vp]),
    "icelk_jpeg_resave_coefficients_host": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, jpeg_info_p, vp, C.c_uint64]),
    "icelk_jpeg_resave_divide_host": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, vp]),
    "icelk_jpeg_resave_rgb": (C.c_int, [handle_p, u8p, C.c_int, C.c_int, C.c_int, C.c_int, u8p, C.c_int]),
    "icelk_jpeg_resave_device_coefficients": (C.c_int, [handle_p, u8p, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_uint64]),
    "icelk_upload_bgr_resave": (C.c_int, [handle_p, C.c_int, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "icelk_upload_jpeg_resave": (C.c_int, [handle_p, C.c_int, jpeg_info_p, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "icelk_upload_jpeg_file_resave": (C.c_int, [handle_p, C.c_int, vp, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "icelk_jpeg_encode_header": (C.c_int, [jpeg_info_p, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "icelk_jpeg_encode_coefficients_host": (C.c_int, [jpeg_info_p, vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "icelk_jpeg_resave_file_host": (C.c_int, [u8p, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_uint64, vp, C.c_uint64,
                                              C.POINTER(C.c_uint64)]),
    "icelk_jpeg_encode_coefficients": (C.c_int, [handle_p, jpeg_info_p, vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "icelk_jpeg_resave_encode": (C.c_int, [handle_p, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "icelk_jpeg_enc_budget": (C.c_int, [C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "icelk_jpeg_encode_budgeted_host": (C.c_int, [jpeg_info_p, vp, C.c_int, C.POINTER(C.c_uint32), C.c_uint32, vp, C.c_uint64, vp, C.c_uint64,
                                                  C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "icelk_jpeg_crop_config": (C.c_int, [handle_p, C.c_int]),
    "icelk_jpeg_crop_start": (C.c_int, [handle_p, vp, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, i32p]),
    "icelk_jpeg_crop_poll": (C.c_int, [handle_p, C.c_int, i32p]),
    "icelk_jpeg_crop_finish": (C.c_int, [handle_p, C.c_int, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(JpegCropStats)]),
    "icelk_jpeg_crop_cancel": (C.c_int, [handle_p, C.c_int]),
    "icelk_upload_jpeg_file_async_resave": (C.c_int, [handle_p, C.c_int, vp, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "icelk_jpeg_async_finish_file": (C.c_int, [handle_p, C.c_int, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(JpegCropStats)]),
    "icelk_jpeg_crop_fwd_device_coefficients": (C.c_int, [handle_p, vp, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_uint64]),
    "icelk_plot_size": (C.c_int, [C.c_int, C.c_int, C.c_int, i32p, i32p]),
    "icelk_plot_glyph": (C.c_int, [C.c_int, u8p]),
    "icelk_plot_overlay_host": (C.c_int, [u8p, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_char_p, u8p, C.c_int]),
    "icelk_plot_tracks": (C.c_int, [handle_p, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, u8p, C.c_int, vp, C.c_uint64,
                                    C.POINTER(C.c_uint64)]),
    "icelk_seg_plot": (C.c_int, [handle_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, u8p, C.c_int, vp, C.c_uint64,
                                 C.POINTER(C.c_uint64), i32p]),
    "icelk_map_glyph": (C.c_int, [C.c_int, u8p]),
    "icelk_map_overlay_host": (C.c_int, [map_desc_p, f64p, i32p, C.c_int, u8p, C.c_int]),
    "icelk_map_arrows_set": (C.c_int, [handle_p, f64p, i32p, C.c_int]),
    "icelk_map_arrows_release": (C.c_int, [handle_p]),
    "icelk_map_draw": (C.c_int, [handle_p, map_desc_p, u8p, C.c_int, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "icelk_thumb_size": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, i32p, i32p]),
    "icelk_thumb_host": (C.c_int, [u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, u8p, C.c_int]),
    "icelk_map_overlay_insets_host": (C.c_int, [map_desc_p, f64p, i32p, C.c_int, map_inset_p, C.c_int, C.POINTER(MapInsetPixels), u8p, C.c_int]),
    "icelk_jpeg_thumb_file": (C.c_int, [handle_p, vp, C.c_uint64, C.c_int, C.c_int, u8p, C.c_int]),
    "icelk_map_inset_set_file": (C.c_int, [handle_p, C.c_int, vp, C.c_uint64, C.c_int, C.c_int]),
    "icelk_map_inset_set_pixels": (C.c_int, [handle_p, C.c_int, u8p, C.c_int, C.c_int, C.c_int]),
    "icelk_map_inset_release": (C.c_int, [handle_p]),
    "icelk_map_draw_insets": (C.c_int, [handle_p, map_desc_p, map_inset_p, C.c_int, u8p, C.c_int, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "icelk_png_bound": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_uint64)]),
    "icelk_png_filter_host": (C.c_int, [u8p, C.c_int, C.c_int, C.c_int, u8p]),
    "icelk_png_encode_host": (C.c_int, [u8p, C.c_int, C.c_int, C.c_int, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "icelk_png_encode_rgb": (C.c_int, [handle_p, u8p, C.c_int, C.c_int, C.c_int, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "icelk_map_draw_png": (C.c_int, [handle_p, map_desc_p, map_inset_p, C.c_int, u8p, C.c_int, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "icelk_movie_size": (C.c_int, [C.c_int, C.c_int, C.c_int, i32p, i32p]),
    "icelk_resize_host": (C.c_int, [u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, u8p, C.c_int]),
    "icelk_resize_rgb": (C.c_int, [handle_p, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, u8p, C.c_int]),
    "icelk_picture_size": (C.c_int, [handle_p, i32p, i32p]),
    "icelk_picture_frame": (C.c_int, [handle_p, C.c_int, C.c_int, C.c_int, u8p, C.c_int, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "icelk_ortho_coords_host": (C.c_int, [vp, ortho_raster_p, C.c_int, C.c_int, C.c_double, f64p, f64p, f64p, u8p]),
    "icelk_ortho_begin_host": (C.c_int, [ortho_raster_p, ortho_opts_p, u8p, C.c_int, u8p, C.c_int, f64p]),
    "icelk_ortho_add_host": (C.c_int, [ortho_raster_p, ortho_opts_p, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, u8p, C.c_int, u8p,
                                       C.c_int, f64p]),
    "icelk_ortho_begin": (C.c_int, [handle_p, ortho_raster_p, ortho_opts_p]),
    "icelk_ortho_add_pixels": (C.c_int, [handle_p, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "icelk_ortho_add_jpeg_file": (C.c_int, [handle_p, vp, C.c_int, vp, C.c_uint64]),
    "icelk_ortho_add_slot": (C.c_int, [handle_p, vp, C.c_int, C.c_int]),
    "icelk_ortho_write": (C.c_int, [handle_p, C.c_int, C.c_int, u8p, C.c_int, u8p, C.c_int, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "icelk_stab_tracks_host": (C.c_int, [f32p, u8p, C.c_int, C.c_int, stab_params_p, f32p, f64p, i32p, f64p, i32p, i32p, i32p]),
    "icelk_stab_anchor_flags_host": (C.c_int, [f32p, C.c_int, C.c_int, u8p, C.c_int, C.c_int, C.c_int, u8p]),
    "icelk_stab_tracks": (C.c_int, [handle_p, f32p, u8p, C.c_int, C.c_int, stab_params_p, f32p, f64p, i32p, f64p, i32p, i32p, i32p]),
    "icelk_stab_set_anchor_mask": (C.c_int, [handle_p, u8p, C.c_int, C.c_int, C.c_int]),
    "icelk_seg_stab_read": (C.c_int, [handle_p, C.c_int, stab_params_p, f32p, f32p, u8p, C.c_int, C.c_int, i32p, i32p, f64p, i32p, f64p,
                                      i32p, i32p, i32p]),
    "icelk_validate": (C.c_int, [handle_p, f64p, f64p, f64p, f64p, C.c_int, i32p, C.c_int, validate_lattice_p, validate_params_p, u8p,
                                 f64p, validate_cells_p]),
    "icelk_validate_host": (C.c_int, [f64p, f64p, f64p, f64p, C.c_int, i32p, C.c_int, validate_lattice_p, validate_params_p, u8p, f64p,
                                      validate_cells_p]),
    "icelk_grid_bin_windows_validated": (C.c_int, [handle_p, f64p, f64p, f64p, f64p, f64p, C.c_int, i64p, i32p, i32p, i32p,
                                                   C.c_int, i64p, i64p, C.c_int, C.c_int, C.c_double, C.c_double,
                                                   C.c_double, C.c_int, C.c_int, u8p, i32p, f64p, f64p, f64p, i32p, f64p,
                                                   f64p, f64p, grid_stats_p, validate_lattice_p, validate_params_p, u8p, i32p]),
    "icelk_cube_tide_fit": (C.c_int, [handle_p, f64p, C.c_int, C.c_int, C.c_double, C.c_int, f64p, f64p, f64p, f64p, f64p, f64p, i32p, i32p,
                                      i32p, i32p, f64p, f64p, f64p]),
    "icelk_cube_tide_predict": (C.c_int, [handle_p, f64p, f64p, i32p, C.c_int, C.c_int, f64p, C.c_int, f64p, f64p]),
    "icelk_tide_fit_host": (C.c_int, [f64p, f64p, f64p, C.c_int, C.c_int, f64p, C.c_int, C.c_double, C.c_int, f64p, f64p, f64p, f64p, f64p,
                                      f64p, i32p, i32p, i32p, i32p, f64p, f64p]),
    "icelk_cube_drift": (C.c_int, [handle_p, drift_lattice_p, drift_params_p, i32p, i32p, f64p, i32p, C.c_double, f64p, f64p, i32p, C.c_int,
                                   drift_out_p, f64p]),
    "icelk_drift_tide": (C.c_int, [handle_p, drift_lattice_p, drift_params_p, f64p, f64p, i32p, C.c_int, f64p, f64p, f64p, i32p, C.c_int,
                                   drift_out_p, f64p]),
    "icelk_drift_host": (C.c_int, [drift_lattice_p, drift_params_p, f64p, f64p, f64p, C.c_int, i32p, i32p, f64p, i32p, C.c_double, f64p, f64p,
                                   i32p, C.c_int, f64p, f64p, f64p, i32p, C.c_int, drift_out_p]),
    "icelk_set_gray_device":(C.c_int, [handle_p, C.c_int, vp, C.c_int, C.c_int, C.c_int]),
    "icelk_cvt_bgr_device": (C.c_int, [handle_p, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "icelk_upload_gray_async": (C.c_int, [handle_p, C.c_int, vp, C.c_int, C.c_int, C.c_int]),
    "icelk_host_alloc": (C.c_int, [C.POINTER(vp), C.c_uint64]),
    "icelk_host_free": (C.c_int, [vp]),
    "icelk_synth_frame": (C.c_int, [handle_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_uint32]),
    "icelk_synth_frame_affine": (C.c_int, [handle_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_uint32, i32p]),
    "icelk_drop_pyramid": (C.c_int, [handle_p, C.c_int]),
    "icelk_download_level": (C.c_int, [handle_p, C.c_int, C.c_int, u8p, C.c_int, i32p, i32p]),
    "icelk_build_pyramid": (C.c_int, [handle_p, C.c_int, C.c_int, C.c_int, C.c_int, i32p]),
    "icelk_pyrlk": (C.c_int, [handle_p, C.c_int, C.c_int, f32p, f32p, u8p, f32p, C.c_int, C.c_int, C.c_int, C.c_int,
                              C.c_int, C.c_int, C.c_double, C.c_int, C.c_double]),
    "icelk_track_fb": (C.c_int, [handle_p, C.c_int, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_int, C.c_double, C.c_double, C.c_float, f32p, f32p, u8p, u8p, f32p, f32p, f32p,
                                 u8p]),
    "icelk_fb_filter": (C.c_int, [handle_p, f32p, f32p, C.c_int, C.c_float, f32p, u8p]),
    "icelk_set_mask": (C.c_int, [handle_p, u8p, C.c_int, C.c_int, C.c_int]),
    "icelk_min_eig_map": (C.c_int, [handle_p, C.c_int, C.c_int, f32p, C.c_int]),
    "icelk_harris_map": (C.c_int, [handle_p, C.c_int, C.c_int, C.c_double, f32p, C.c_int]),
    "icelk_set_detector": (C.c_int, [handle_p, C.c_int, C.c_double]),
    "icelk_get_detector": (C.c_int, [handle_p, i32p, C.POINTER(C.c_double)]),
    "icelk_good_features": (C.c_int, [handle_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, f32p,
                                      C.c_int, i32p]),
    "icelk_detect_stats": (C.c_int, [handle_p, i32p, i32p]),
    "icelk_seg_detect": (C.c_int, [handle_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, i32p]),
    "icelk_set_mask_polygon": (C.c_int, [handle_p, f64p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int]),
    "icelk_download_mask": (C.c_int, [handle_p, u8p, C.c_int, i32p, i32p]),
    "icelk_build_pyramid_ahead": (C.c_int, [handle_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "icelk_seg_detect_prepare": (C.c_int, [handle_p, C.c_int, C.c_int, C.c_int]),
    "icelk_seg_detect_begin": (C.c_int, [handle_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]),
    "icelk_seg_detect_finish": (C.c_int, [handle_p, C.c_int, i32p]),
    "icelk_seg_detect_cancel": (C.c_int, [handle_p]),
    "icelk_set_variant": (C.c_int, [handle_p, C.c_char_p, C.c_int]),
    "icelk_seg_detect_stage_try": (C.c_int, [handle_p, C.c_int, i32p, i32p]),
    "icelk_detect_fast_stats": (C.c_int, [handle_p, C.c_int, C.c_int, C.POINTER(C.c_longlong)]),
    "icelk_detect_max_key": (C.c_int, [handle_p, C.POINTER(C.c_uint)]),
    "icelk_seg_detect_stage": (C.c_int, [handle_p, C.c_int, i32p]),
    "icelk_seg_switch": (C.c_int, [handle_p]),
    "icelk_seg_track": (C.c_int, [handle_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_double, C.c_double, C.c_float, i32p]),
    "icelk_seg_track_async": (C.c_int, [handle_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_double, C.c_double, C.c_float]),
    "icelk_seg_track_defer": (C.c_int, [handle_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_double, C.c_double, C.c_float]),
    "icelk_seg_flush": (C.c_int, [handle_p]),
    "icelk_seg_track_len_hint": (C.c_int, [handle_p, C.c_int]),
    "icelk_seg_template_stats": (C.c_int, [handle_p, C.POINTER(C.c_longlong)]),
    "icelk_seg_tail_stats": (C.c_int, [handle_p, C.POINTER(C.c_longlong)]),
    "icelk_seg_template_info": (C.c_int, [handle_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), i32p]),
    "icelk_seg_read_closed": (C.c_int, [handle_p, f32p, f32p, C.c_int, C.c_int, i32p, i32p]),
    "icelk_seg_archive_closed": (C.c_int, [handle_p, vp, vp, vp, C.c_int, i32p]),
    "icelk_seg_live": (C.c_int, [handle_p, i32p, i64p]),
    "icelk_seg_archive": (C.c_int, [handle_p, vp, vp, vp, C.c_int, i32p]),
    "icelk_project_tracks": (C.c_int, [handle_p, f32p, C.c_int, C.c_int, vp, vp, f64p, f64p, f64p, f64p, f64p, u8p]),
    "icelk_seg_project": (C.c_int, [handle_p, vp, vp, C.c_int, C.c_int, f64p, f64p, f64p, f64p, f64p, u8p, i32p, i32p]),
    "icelk_points_in_polygon": (C.c_int, [handle_p, f64p, C.c_int, f64p, C.c_int, u8p]),
    "icelk_grid_bin": (C.c_int, [handle_p, f64p, f64p, f64p, f64p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int,
                                 C.c_int, u8p, i32p, f64p, f64p, f64p]),
    "icelk_grid_bin_windows": (C.c_int, [handle_p, f64p, f64p, f64p, f64p, f64p, C.c_int, i64p, i32p, i32p, i32p,
                                         C.c_int, i64p, i64p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                         C.c_int, C.c_int, u8p, i32p, f64p, f64p, f64p, i32p, f64p, f64p, f64p]),
    "icelk_grid_bin_stats": (C.c_int, [handle_p, f64p, f64p, f64p, f64p, C.c_int, C.c_double, C.c_double, C.c_double,
                                       C.c_int, C.c_int, u8p, i32p, f64p, f64p, f64p, grid_stats_p]),
    "icelk_grid_bin_windows_stats": (C.c_int, [handle_p, f64p, f64p, f64p, f64p, f64p, C.c_int, i64p, i32p, i32p, i32p,
                                               C.c_int, i64p, i64p, C.c_int, C.c_int, C.c_double, C.c_double,
                                               C.c_double, C.c_int, C.c_int, u8p, i32p, f64p, f64p, f64p, i32p, f64p,
                                               f64p, f64p, grid_stats_p]),
    "icelk_grid_cell_stats_host": (C.c_int, [f64p, C.c_int, f64p, f64p, f64p]),
    "icelk_boxes_check": (C.c_int, [boxes_p]),
    "icelk_boxes_bin": (C.c_int, [handle_p, f64p, f64p, f64p, f64p, C.c_int, boxes_p, f64p, i32p, f64p, f64p, f64p,
                                  grid_stats_p]),
    "icelk_boxes_bin_windows": (C.c_int, [handle_p, f64p, f64p, f64p, f64p, f64p, C.c_int, day_tables_p, boxes_p, f64p,
                                          i32p, f64p, f64p, f64p, grid_stats_p, i32p, f64p, f64p, f64p]),
    "icelk_cube_set": (C.c_int, [handle_p, f64p, f64p, f64p, C.c_int, C.c_int]),
    "icelk_cube_release": (C.c_int, [handle_p]),
    "icelk_cube_average": (C.c_int, [handle_p, i32p, i32p, C.c_int, C.c_int, C.c_int, C.c_int, f64p, f64p, f64p, f64p,
                                     i32p, f64p]),
    "icelk_calib_set": (C.c_int, [handle_p, f64p, C.c_int, f64p, C.c_int, C.c_double, C.c_double]),
    "icelk_calib_release": (C.c_int, [handle_p]),
    "icelk_calib_residuals": (C.c_int, [handle_p, f64p, C.c_int, f64p, f64p, f64p, f64p]),
    "icelk_calib_cost": (C.c_int, [handle_p, f64p, C.c_int, f64p, f64p]),
    "icelk_seg_read": (C.c_int, [handle_p, f32p, f32p, C.c_int, C.c_int, i32p, i32p]),
    "icelk_prof_enable": (C.c_int, [handle_p, C.c_int]),
    "icelk_prof_reset": (C.c_int, [handle_p]),
    "icelk_prof_iterations": (C.c_int, [handle_p, C.POINTER(C.c_uint32), C.c_int, i32p]),
    "icelk_stream_probe_info": (C.c_int, [handle_p, i32p, f64p, f64p]),
    "icelk_prof_count": (C.c_int, []),
    "icelk_prof_name": (C.c_char_p, [C.c_int]),
    "icelk_prof_get": (C.c_int, [handle_p, C.c_int, i32p, f64p]),
}

_lib = None


class IcelkError(RuntimeError):
    """Raised for ICELK_EHIP / ICELK_ECAP / ICELK_ESTATE; bad arguments raise ValueError."""


def load():
    """Load libicelk.so.  Raises if it has not been built -- there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IcelkError(
                "libicelk.so is missing (%s). Build it with `python -m iceberg_tracking_code_amd.build` "
                "(needs hipcc); this package has no CPU fallback." % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc, handle=None):
    if rc == OK:
        return
    msg = load().icelk_last_error(handle)
    msg = msg.decode() if msg else ""
    text = "icelk error %d: %s" % (rc, msg)
    if rc == EARG:
        raise ValueError(text)
    if rc == ENOMEM:
        raise MemoryError(text)
    raise IcelkError(text)
