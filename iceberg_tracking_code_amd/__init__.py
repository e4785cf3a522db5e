"""MI355X-native sparse Lucas-Kanade tracking: the hot path of glacierbliss/iceberg_tracking_code
(s1_lucaskanade_tracking.py:307-450) as hand-written HIP kernels behind a C ABI (include/icelk.h).

    import iceberg_tracking_code_amd as cv2          # cvtColor / goodFeaturesToTrack / calcOpticalFlowPyrLK
    from iceberg_tracking_code_amd import SegmentTracker   # device-resident form of the same loop

There is no CPU fallback: calls raise if libicelk.so has not been built or no GPU is present.
"""
from .api import (COLOR_BGR2GRAY, COLOR_RGB2GRAY, calcOpticalFlowPyrLK, cornerHarris, cornerMinEigenVal, cvtColor,  # noqa: F401
                  default_context,
                  goodFeaturesToTrack, release, set_device, set_gray_variant, set_variant)
from .context import (Context, DEFAULT_CRITERIA, GRAY_CV3, GRAY_CV4, OPTFLOW_LK_GET_MIN_EIGENVALS,  # noqa: F401
                      OPTFLOW_USE_INITIAL_FLOW, TERM_CRITERIA_COUNT, TERM_CRITERIA_EPS, TERM_CRITERIA_MAX_ITER)
from .tracker import (REF_FB_THRESHOLD, REF_FEATURE_PARAMS, REF_LK_PARAMS, SegmentTracker,  # noqa: F401
                      npz_name, save_tracks, segment_time_ok)
from .utm import CameraModel, REF_UTM_FILTER, cam_to_utm, project_segment, project_tracks, utm_name  # noqa: F401
from .sequence import track_image_sequence  # noqa: F401
from .crop import crop_image_sequence  # noqa: F401
from .gridding import bin_velocities, create_grid_across_fjord, grid_cell_stats_host, points_in_polygon  # noqa: F401
from .day_grid import closest_image, utm_to_gridded_utm, utm_to_gridded_utm_days  # noqa: F401
from .transect import (BoxSet, azimuth_transect, bin_boxes, create_squares_along_transect, create_squares_around_mooring,  # noqa: F401
                       create_squares_rot, locate_points_along_transect, utm_to_transect, utm_to_transect_days)
from .postprocess import (VelocityCube, average_periods, average_spatially_temporally, combine_npzs,  # noqa: F401
                          daily_averages, npz_to_csv, npz_to_mat, save_csv, velocities_to_regular_grid)
from .calibration import CalibrationResult, ShorelineScene, calibrate, run_calibration  # noqa: F401
from .jpeg import (JpegCoefficients, UnsupportedJpeg, decode_jpeg, read_jpeg, read_jpeg_lanes, resave_coefficients,  # noqa: F401
                   resave_rgb, resave_tables, encode_jpeg, resave_bytes, source_comment, thumbnail, thumbnail_host,
                   thumbnail_size)
from .plot import plot_glyph, plot_name, plot_overlay_host, plot_size, plot_stamp  # noqa: F401
from .velocity_map import (gist_rainbow_table, map_descriptor, map_glyph, map_inset_array, map_layout, map_name, map_overlay_host, map_picture,  # noqa: F401
                           map_insets, map_strings, map_texts, map_view, scaled_arrows)
from .png import encode_png_host, png_bound, png_filter_host  # noqa: F401
from .movie import MovieWriter, frame_host, movie_size, read_avi, resize_host  # noqa: F401
from .orthophoto import (ortho_coords_host, ortho_movie_name, ortho_raster, orthophoto, orthophoto_host, orthophoto_sequence,  # noqa: F401
                         read_world_file, world_file)
from .stabilize import (STAB_DEGENERATE, STAB_LOST, STAB_NOT_CONVERGED, STAB_TOO_FEW, anchor_flags, stabilize_tracks,  # noqa: F401
                        stabilize_tracks_host)
from .validate import validate_velocities, validate_velocities_host, validation_lattice  # noqa: F401
from .tides import CONSTITUENTS, TideFit, fit_tides, fit_tides_host, load_tides, tide_basis  # noqa: F401
from .drift import (DriftResult, drift, drift_host, drift_lattice, drift_schedule, load_drift, seed_line, seed_nodes)  # noqa: F401
from ._lib import IcelkError  # noqa: F401

__version__ = "0.1.0"
