"""Builds libicelk.so (HIP kernels + C ABI) in-tree for gfx950 with hipcc.

    python -m iceberg_tracking_code_amd.build [--force]

-ffp-contract=off is part of the contract, not a tuning flag: the float sequences of the LK 2x2
solve and of the min-eigenvalue map must not be fused into FMAs or the results stop being
bit-identical to the CPU oracle (and to a non-FMA OpenCV build).
"""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "obj")
LIB = os.path.join(HERE, "libicelk.so")
SOURCES = ["abi_handle.hip", "abi_frames.hip", "abi_lk.hip", "abi_detect.hip", "abi_segments.hip", "abi_post.hip", "abi_calib.hip", "abi_jpeg.hip", "abi_jpeg_ingest.hip", "abi_jpeg_job.hip", "abi_jpeg_async.hip", "abi_jpeg_resave.hip", "abi_jpeg_enc.hip", "abi_jpeg_crop.hip", "abi_plot.hip", "abi_map.hip", "abi_picture.hip", "abi_thumb.hip", "abi_png.hip", "abi_movie.hip", "abi_ortho.hip", "abi_stab.hip", "abi_validate.hip", "abi_tides.hip", "abi_drift.hip",
           "k_image.hip", "k_pyramid.hip", "k_lk.hip", "k_lk_fast.hip", "k_lk_multi.hip", "k_corners.hip", "k_corners_fast.hip", "k_min_distance.hip", "k_sort.hip", "k_tail.hip", "k_tracks.hip", "k_utm.hip", "k_mask.hip", "k_grid.hip", "k_cube.hip", "k_calib.hip", "k_jpeg.hip", "k_jpeg_huff.hip", "k_jpeg_fwd.hip", "k_jpeg_enc.hip", "k_plot.hip", "k_map.hip", "k_thumb.hip", "k_png.hip", "k_resize.hip", "k_ortho.hip", "k_stab.hip", "k_validate.hip", "k_tides.hip", "k_drift.hip"]
# every header under csrc/ plus the public one: a new header cannot be forgotten by the staleness check
HEADERS = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join(HERE, "..", "include", "icelk.h")]
ARCH = "gfx950"
FLAGS = ["--offload-arch=" + ARCH, "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
         "-Wall", "-Wno-unused-result", "-Wno-unused-value"]


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: libicelk.so cannot be built (ROCm toolchain required)")
    return exe


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _compile(src, force, obj_dir, extra_flags):
    obj = os.path.join(obj_dir, os.path.splitext(src)[0] + ".o")
    path = os.path.join(CSRC, src)
    if force or _stale(obj, [path] + HEADERS):
        cmd = [_hipcc()] + FLAGS + list(extra_flags) + ["-c", path, "-o", obj]
        subprocess.check_call(cmd)
    return obj


def build(force=False, verbose=False, lib=LIB, obj_dir=OBJ, extra_flags=()):
    """lib / obj_dir / extra_flags: a second build beside the package's own (tools/build_variant.sh)."""
    os.makedirs(obj_dir, exist_ok=True)
    with ThreadPoolExecutor(max_workers=min(6, len(SOURCES))) as ex:
        objs = list(ex.map(lambda s: _compile(s, force, obj_dir, extra_flags), SOURCES))
    if force or _stale(lib, objs):
        cmd = [_hipcc(), "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", lib] + objs
        subprocess.check_call(cmd)
        if verbose:
            print("built", lib)
    return lib


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
