"""Camera shake fitted to land anchors: an opt-in stage between tracking and saving.

A time-lapse camera on a tripod shakes in wind and settles over a day; a whole-frame shift of 1 px between two photos 60 s
apart, at 5 m per pixel, adds the same false 0.08 m/s to every velocity of that pair, and neither the forward-backward
test nor the speed filters can see it, because it is coherent.  The tracks of a segment that start on static ground -- inside
an *anchor mask* -- are the anchors: for every vertex k >= 1 the motion of the picture from the segment's first frame to
frame k is fitted to them (a robust translation or similarity), and every track's vertex k is mapped back through the fit.
The table comes out in the coordinates of the segment's first frame, so `cam_to_utm` and everything after it run unchanged.

The rules are csrc/stab.h; the kernels are csrc/k_stab.hip (`stabilize_tracks`, `Context.seg_stabilize`), the host
statement is `stabilize_tracks_host`, and tests/stab_restatement.py restates them in numpy.  The three agree bit for bit.

Parameters: `threshold` (1.0 px) is the reference's forward-backward bound (s1:333).  `start_gate` 8.0 px, `rounds` 8,
`min_anchors` 10 and `min_spread` 64.0 px are policy defaults, not measurements.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import STAB_DEGENERATE, STAB_LOST, STAB_NOT_CONVERGED, STAB_TOO_FEW  # noqa: F401

MODELS = ("translation", "similarity")
DEFAULTS = dict(model="translation", threshold=1.0, start_gate=8.0, rounds=8, min_anchors=10, min_spread=64.0)


def params_struct(model="translation", threshold=1.0, start_gate=8.0, rounds=8, min_anchors=10, min_spread=64.0):
    """icelk_stab_params_t of the keywords; what it cannot express raises ValueError, the ranges are the library's to check."""
    if model not in MODELS:
        raise ValueError("model must be 'translation' or 'similarity'")
    return _lib.StabParams(model=MODELS.index(model), rounds=int(rounds), min_anchors=int(min_anchors), reserved=0,
                           threshold=float(threshold), start_gate=float(start_gate), min_spread=float(min_spread))


def _table(tracks):
    t = np.ascontiguousarray(tracks, dtype=np.float32)
    if t.ndim != 3 or t.shape[2] != 2 or not 2 <= t.shape[1] <= _lib.STAB_MAX_VERTICES:
        raise ValueError("tracks must be (n, V, 2) with 2 <= V <= 17")
    return t


def _flags(anchors, n):
    f = np.ascontiguousarray(np.asarray(anchors).reshape(-1) != 0, dtype=np.uint8)
    if f.shape != (n,):
        raise ValueError("anchors must hold one flag per track")
    return f


class _Results:
    """The per-vertex arrays of one call and their pointers, in the order the C calls take them."""

    def __init__(self, V):
        self.motion = np.zeros((max(V - 1, 0), 4), np.float64)
        self.inliers = np.zeros(max(V - 1, 0), np.int32)
        self.rms = np.zeros(max(V - 1, 0), np.float64)
        self.status = np.zeros(max(V - 1, 0), np.int32)
        self.rounds_used = np.zeros(max(V - 1, 0), np.int32)
        self.n_anchors = C.c_int(0)

    def pointers(self):
        return (self.motion.ctypes.data_as(_lib.f64p), self.inliers.ctypes.data_as(_lib.i32p), self.rms.ctypes.data_as(_lib.f64p),
                self.status.ctypes.data_as(_lib.i32p), self.rounds_used.ctypes.data_as(_lib.i32p), C.byref(self.n_anchors))

    def as_dict(self, tracks, anchors):
        return dict(tracks=tracks, motion=self.motion, inliers=self.inliers, rms=self.rms, status=self.status,
                    rounds_used=self.rounds_used, anchors=anchors, n_anchors=self.n_anchors.value)


def _stabilize(call, handle, tracks, anchors, params):
    t = _table(tracks)
    f = _flags(anchors, len(t))
    P = params_struct(**params)
    out, R = np.empty_like(t), _Results(t.shape[1])
    rc = call(t.ctypes.data_as(_lib.f32p), f.ctypes.data_as(_lib.u8p), len(t), t.shape[1], C.byref(P), out.ctypes.data_as(_lib.f32p),
              *R.pointers())
    _lib.check(rc, handle)
    return R.as_dict(out, f.astype(bool))


def stabilize_tracks_host(tracks, anchors, **params):
    """The host statement of the rules (icelk_stab_tracks_host: no handle, no GPU).  Returns what `stabilize_tracks` does."""
    return _stabilize(_lib.load().icelk_stab_tracks_host, None, tracks, anchors, params)


def stabilize_tracks(ctx, tracks, anchors, model="translation", threshold=1.0, start_gate=8.0, rounds=8, min_anchors=10, min_spread=64.0):
    """Fit the camera's motion to the anchor rows of `tracks` (n, V, 2) and map every row back through it, on the device.

    `anchors`: one flag per row, non-zero = the track starts on static ground (`anchor_flags`).  Returns a dict: `tracks`
    (n, V, 2) float32 in the coordinates of vertex 0's frame; per vertex k = 1 .. V - 1 (entry k - 1) `motion` (a, b, tx, ty)
    float64, `inliers`, `rms` (NaN without a model), `status` (bits STAB_TOO_FEW, STAB_LOST, STAB_DEGENERATE,
    STAB_NOT_CONVERGED) and `rounds_used`; `anchors` (the flags as booleans) and `n_anchors` (the flagged rows whose
    coordinates are all finite).  A vertex whose fit is TOO_FEW or LOST is returned as it came."""
    params = dict(model=model, threshold=threshold, start_gate=start_gate, rounds=rounds, min_anchors=min_anchors, min_spread=min_spread)
    return _stabilize(lambda *a: ctx._lib.icelk_stab_tracks(ctx._h, *a), ctx._h, tracks, anchors, params)


def _mask2d(anchor_mask):
    m = np.ascontiguousarray(anchor_mask)
    if m.ndim != 2 or m.size == 0:
        raise ValueError("anchor_mask must be a non-empty 2-D array")
    return np.ascontiguousarray(m != 0, dtype=np.uint8)


def anchor_flags(tracks, anchor_mask):
    """One boolean per row: vertex 0, rounded to the nearest pixel (floor(x + 0.5)), lies on a non-zero pixel of the mask."""
    t = np.ascontiguousarray(tracks, dtype=np.float32)
    if t.ndim != 3 or t.shape[2] != 2 or t.shape[1] < 1:
        raise ValueError("tracks must be (n, V, 2)")
    m = _mask2d(anchor_mask)
    flags = np.zeros(len(t), np.uint8)
    _lib.check(_lib.load().icelk_stab_anchor_flags_host(t.ctypes.data_as(_lib.f32p), len(t), t.shape[1], m.ctypes.data_as(_lib.u8p),
                                                        m.shape[1], m.shape[0], m.shape[1], flags.ctypes.data_as(_lib.u8p)), None)
    return flags.astype(bool)


def set_anchor_mask(ctx, anchor_mask):
    """`Context.stab_set_anchor_mask`: the mask goes up once and stays; None releases it."""
    if anchor_mask is None:
        ctx._ck(ctx._lib.icelk_stab_set_anchor_mask(ctx._h, None, 0, 0, 0))
        return
    m = _mask2d(anchor_mask)
    ctx._ck(ctx._lib.icelk_stab_set_anchor_mask(ctx._h, m.ctypes.data_as(_lib.u8p), m.shape[1], m.shape[0], m.shape[1]))


def seg_stabilize(ctx, closed=False, **params):
    """`Context.seg_stabilize`: the current (closed: the latest closed) segment read through the stabilisation.  Returns the
    dict of `stabilize_tracks` plus `trackquality`; `anchors` are the rows that start under the resident anchor mask."""
    P = params_struct(**params)
    n, nv = C.c_int(0), C.c_int(0)
    none = (None,) * 6
    ctx._ck(ctx._lib.icelk_seg_stab_read(ctx._h, int(bool(closed)), C.byref(P), None, None, None, 0, 0, C.byref(n), C.byref(nv), *none))
    tracks = np.zeros((n.value, nv.value, 2), np.float32)
    quality = np.zeros((n.value, max(nv.value - 1, 0)), np.float32)
    flags = np.zeros(n.value, np.uint8)
    R = _Results(nv.value)
    ctx._ck(ctx._lib.icelk_seg_stab_read(ctx._h, int(bool(closed)), C.byref(P), tracks.ctypes.data_as(_lib.f32p),
                                         quality.ctypes.data_as(_lib.f32p), flags.ctypes.data_as(_lib.u8p), max(n.value, 1),
                                         max(nv.value, 1), C.byref(n), C.byref(nv), *R.pointers()))
    out = R.as_dict(tracks, flags.astype(bool))
    out["trackquality"] = quality
    return out
