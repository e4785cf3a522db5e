"""The Harris detector on the GPU against tests/harris_restatement.py, bit for bit: the response map of every kernel that
carries it, the corner list behind it (order included), the maximum <= 0 case, the named form, what a detection in flight
keeps, the device-resident frame loop.

Frames: harris_restatement.blob_frame.  Every map test first holds the eigenvalue map of its frame against
np_restatement.min_eig_map, so that a difference in the Harris map is the response's and not the sums'.
  96 x 70     top and bottom reflected in every strip
  250 x 130   the frame loop's
  517 x 203   at every strip block size at least two strips across and two down lie inside the frame and take the strip
              kernel's FAST row phase (StripCfg: TW 245 .. 252 columns, SH 54 .. 58 rows, NROWS <= 69 rows read)
"""
import numpy as np
import pytest

import harris_restatement as H
import np_restatement as R

pytestmark = pytest.mark.gpu

STRIP_BLOCK_SIZES = (3, 5, 7, 10)
BLOCK_SIZES = STRIP_BLOCK_SIZES + (4,)         # 4: the any-blockSize kernels
KS = (0.04, 0.15)
SIZES = ((96, 70, 3), (250, 130, 4), (517, 203, 5))      # w, h, seed

_frames, _maps = {}, {}


def frame(size):
    if size not in _frames:
        _frames[size] = H.blob_frame(*size)
    return _frames[size]


def harris(size, bs, k, tail=0):
    """the restatement's map of a frame, computed once"""
    key = (size, bs, k, tail)
    if key not in _maps:
        _maps[key] = H.harris_map(frame(size), bs, k, tail)
    return _maps[key]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same_corners(got, want):
    if got is None or want is None:
        return got is None and want is None
    return same(got, want)


def masks(ctx, size):
    """(tag, use_mask, what the restatement is given, how the handle gets it)"""
    w, h, seed = size
    rng = np.random.RandomState(seed)
    arr = np.kron(rng.randint(0, 4, ((h + 7) // 8, (w + 7) // 8)) > 0, np.ones((8, 8)))[:h, :w].astype(np.uint8) * 255
    poly = np.array([[0.1 * w, 0.15 * h], [0.8 * w, 0.05 * h], [0.95 * w, 0.6 * h], [0.5 * w, 0.9 * h], [0.3 * w, 0.5 * h],
                     [0.05 * w, 0.8 * h]])
    yield "none", False, None
    ctx.set_mask(arr)
    yield "array", True, arr
    ctx.set_mask_polygon(poly, 0, 0, w, h)
    yield "polygon", True, ctx.download_mask()


@pytest.fixture()
def hctx(ctx):
    """the session's context, handed over and taken back with the default detector and form"""
    ctx.set_detector(False)
    ctx.set_variant("harris_tail", 0)
    yield ctx
    ctx.set_detector(False)
    ctx.set_variant("harris_tail", 0)


def test_strip_geometry_of_the_large_frame():
    """the constants this file's choice of 517 x 203 rests on (csrc/k_corners.hip StripCfg), restated"""
    w, h = SIZES[2][:2]
    for bs in STRIP_BLOCK_SIZES:
        unroll = bs * 4 // np.gcd(bs, 4)
        eh = 64 // unroll * unroll
        tw, sh, nrows, an = 256 - (bs - 1) - 2, eh - 2, eh + bs - 1, bs // 2
        inside = [(bx, by) for bx in range((w + tw - 1) // tw) for by in range((h + sh - 1) // sh)
                  if (bx + 1) * tw <= w and by * sh - 1 - an - 1 >= 0 and by * sh - 1 - an + nrows <= h - 1]
        assert len(inside) >= 4, bs
        assert (h + sh - 1) // sh == 4 and (w + tw - 1) // tw == 3


@pytest.mark.parametrize("size", SIZES[::2], ids=lambda s: "%dx%d" % s[:2])
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_map_bit_for_bit(hctx, size, bs):
    img = frame(size)
    hctx.upload_gray(0, img)
    assert same(hctx.min_eig_map(0, bs), R.min_eig_map(img, bs))
    for k in KS:
        want = harris(size, bs, k)
        assert (want > 0).mean() > 0.2 and (k < 0.1 or (want < 0).mean() > 0.2)      # both signs are in the map
        assert same(hctx.harris_map(0, bs, k), want), k
        assert hctx.detect_max_key() == _key(want.max())
    assert hctx.get_detector() == (False, 0.04)       # the map took its k as an argument


def _key(v):
    b = int(np.float32(v).view(np.uint32))
    return (~b & 0xffffffff) if b & 0x80000000 else (b | 0x80000000)


def test_cv2_shaped_maps(hctx):
    import iceberg_tracking_code_amd as cv
    img = frame(SIZES[0])
    assert same(cv.cornerHarris(img, 5, 3, 0.06), H.harris_map(img, 5, 0.06))
    assert same(cv.cornerMinEigenVal(img, 5), R.min_eig_map(img, 5))
    assert same(cv.cornerMinEigenVal(img, 4, ksize=3), R.min_eig_map(img, 4))
    assert same_corners(cv.goodFeaturesToTrack(img, 30, 0.01, 5, blockSize=5, useHarrisDetector=True, k=0.06),
                        H.good_features(img, 30, 0.01, 5, None, 5, True, 0.06))
    # the default is what it was
    assert same_corners(cv.goodFeaturesToTrack(img, 30, 0.01, 5, blockSize=5), R.good_features(img, 30, 0.01, 5, None, 5))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s[:2])
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_corner_list_equal_order_included(hctx, size, bs):
    img = frame(size)
    hctx.upload_gray(0, img)
    assert same(hctx.min_eig_map(0, bs), R.min_eig_map(img, bs))
    counts = []
    for tag, use_mask, mask in masks(hctx, size):
        for k in KS:
            resp = harris(size, bs, k)
            assert H.ties(resp, 0.01, mask) == 0          # the order is the responses' alone
            for q in (0.01, 0.3):
                for md in (0, 5, 10):
                    for maxc in (0, 17):
                        want = H.select(resp, maxc, q, md, mask)
                        got = hctx.good_features(0, maxc, q, md, use_mask, bs, useHarrisDetector=True, k=k)
                        assert same_corners(got, want), (tag, k, q, md, maxc)
                        if (tag, q, md, maxc) == ("none", 0.01, 5, 0):
                            counts.append(len(want))
    assert min(counts) >= {96: 12, 250: 40, 517: 150}[size[0]], counts
    assert hctx.get_detector() == (False, 0.04)       # the keyword set the detector for its call only


def test_ramp_gives_no_corner_and_no_candidate(hctx):
    ramp = H.ramp_frame()
    hctx.upload_gray(0, ramp)
    for bs in (5, 4):
        want = H.harris_map(ramp, bs, 0.04)
        assert want.max() < 0
        assert same(hctx.harris_map(0, bs, 0.04), want)
        for md in (0, 5):
            assert hctx.good_features(0, 0, 0.01, md, False, bs, useHarrisDetector=True, k=0.04) is None
            assert hctx.detect_stats()["candidates"] == 0
            assert hctx.detect_max_key() == _key(want.max()) and hctx.detect_max_key() < 0x80000000
    # a ramp as wide as three strips: interior strips (the FAST row phase) see nothing but negative values either
    wide = np.tile(np.linspace(0, 255, 600).astype(np.uint8), (200, 1))
    hctx.upload_gray(0, wide)
    want = H.harris_map(wide, 5, 0.04)
    assert want.max() <= 0
    assert hctx.good_features(0, 0, 0.01, 5, False, 5, useHarrisDetector=True, k=0.04) is None
    assert hctx.detect_stats()["candidates"] == 0
    # ... and the maximum they publish, from signed extremes of the bits in place of keys, is the map's negative maximum
    assert want.max() < 0 and hctx.detect_max_key() == _key(want.max()) and hctx.detect_max_key() < 0x80000000


@pytest.mark.parametrize("bs", [3, 4])
def test_mask_of_the_negative_pixels_gives_no_corner(hctx, bs):
    size, k = SIZES[0], 0.15
    img, resp = frame(size), harris(size, bs, 0.15)
    neg = (resp < 0).astype(np.uint8) * 255
    assert 0.3 < (neg != 0).mean() < 0.8
    hctx.upload_gray(0, img)
    assert same(hctx.min_eig_map(0, bs), R.min_eig_map(img, bs))
    hctx.set_mask(neg)
    for md in (0, 5):
        assert H.select(resp, 0, 0.01, md, neg) is None
        assert hctx.good_features(0, 0, 0.01, md, True, bs, useHarrisDetector=True, k=k) is None
        assert hctx.detect_stats()["candidates"] == 0
        assert hctx.detect_max_key() == _key(resp[neg != 0].max())
        want = H.select(resp, 0, 0.01, md, None)
        assert len(want) > 10 and same_corners(hctx.good_features(0, 0, 0.01, md, False, bs, useHarrisDetector=True, k=k), want)


def test_harris_tail_form(hctx):
    size = SIZES[0]
    img = frame(size)
    hctx.upload_gray(0, img)
    for bs in (4, 10):
        assert same(hctx.min_eig_map(0, bs), R.min_eig_map(img, bs))
        for k in KS:
            lanes, tail = harris(size, bs, k, 0), harris(size, bs, k, 1)
            assert not same(lanes, tail)
            hctx.set_variant("harris_tail", 1)
            assert same(hctx.harris_map(0, bs, k), tail)
            assert same_corners(hctx.good_features(0, 0, 0.01, 5, False, bs, useHarrisDetector=True, k=k),
                                H.select(tail, 0, 0.01, 5))
            assert same(hctx.min_eig_map(0, bs), R.min_eig_map(img, bs))      # not the eigenvalue map's business
            hctx.set_variant("harris_tail", 0)
            assert same(hctx.harris_map(0, bs, k), lanes)


def test_bad_detector_arguments_on_a_live_handle(hctx):
    hctx.set_detector(True, 0.06)
    for kind, k in ((7, 0.04), (-1, 0.04), (1, float("nan")), (1, float("inf")), (0, float("nan"))):
        assert hctx._lib.icelk_set_detector(hctx._h, kind, k) == -1
        assert hctx.get_detector() == (True, 0.06)
    with pytest.raises(ValueError):
        hctx.harris_map(0, 3, float("nan"))


def one_call(ctx, slot, args, harris_on, k=0.04):
    return ctx.good_features(slot, *args) if not harris_on else ctx.good_features(slot, *args, useHarrisDetector=True, k=k)


def first_vertices(c):
    return c.seg_read()[0][:, 0, :]


def test_a_detection_in_flight_keeps_its_detector(hctx):
    a, b = frame(SIZES[1]), H.blob_frame(250, 130, 9)
    hctx.upload_gray(0, a)
    hctx.upload_gray(1, b)
    for bs in (5, 4):
        args = (40, 0.01, 7, False, bs)
        want_a, want_b = one_call(hctx, 0, args, False), one_call(hctx, 1, args, True)
        assert same_corners(want_a, R.good_features(a, 40, 0.01, 7, None, bs))
        assert same_corners(want_b, H.good_features(b, 40, 0.01, 7, None, bs, True, 0.04))
        assert not same_corners(one_call(hctx, 0, args, True), want_a)
        hctx.seg_detect_begin(0, *args)
        hctx.set_detector(True, 0.04)
        hctx.seg_detect_begin(1, *args)
        hctx.set_detector(True, 0.2)          # neither detection in flight looks at the handle again
        assert hctx.seg_detect_finish(40) == len(want_a)
        assert same(first_vertices(hctx), want_a.reshape(-1, 2))
        hctx.set_detector(False)
        assert hctx.seg_detect_finish(40) == len(want_b)
        assert same(first_vertices(hctx), want_b.reshape(-1, 2))


@pytest.mark.parametrize("prepared,begun", [((False, 0.04), (True, 0.04)), ((True, 0.04), (False, 0.04)), ((True, 0.04), (True, 0.15))])
def test_prepared_candidates_of_another_detector_are_not_adopted(hctx, prepared, begun):
    img = frame(SIZES[1])
    args = (0, 0.01, 7, False, 5)
    hctx.upload_gray(0, img)
    want = one_call(hctx, 0, args, *begun)
    hctx.upload_gray(0, img)              # a new generation of the slot: nothing prepared before holds
    hctx.seg_detect_prepare(0, False, 5, useHarrisDetector=prepared[0], k=prepared[1])
    hctx.seg_detect_begin(0, *args, useHarrisDetector=begun[0], k=begun[1])
    assert hctx.seg_detect_finish(0) == len(want)
    assert same(first_vertices(hctx), want.reshape(-1, 2))
    # and the same detector's are: same result (that they were adopted is the profile's business, not this test's)
    hctx.upload_gray(0, img)
    hctx.seg_detect_prepare(0, False, 5, useHarrisDetector=begun[0], k=begun[1])
    hctx.seg_detect_begin(0, *args, useHarrisDetector=begun[0], k=begun[1])
    assert hctx.seg_detect_finish(0) == len(want)
    assert same(first_vertices(hctx), want.reshape(-1, 2))


LOOP_FP = dict(maxCorners=60, qualityLevel=0.01, minDistance=7, blockSize=5, useHarrisDetector=True, k=0.04)
LOOP_LK = dict(winSize=(21, 21), maxLevel=2, criteria=(3, 25, 0.03))


@pytest.fixture(scope="module")
def loop():
    from reference_loops import run_reference_loop
    frames = [H.blob_frame(250, 130, 11, shift=(1.3 * i, -0.8 * i)) for i in range(7)]
    ref = run_reference_loop(frames, 2, LOOP_FP, LOOP_LK, cv=H.HarrisRestatementCv)
    plain = run_reference_loop(frames, 2, dict(LOOP_FP, useHarrisDetector=False), LOOP_LK, cv=H.HarrisRestatementCv)
    assert len(ref) == 3 and [np.float32(t).shape for _, t, _ in ref] != [] and \
        not all(np.array_equal(np.float32(a[1]), np.float32(b[1])) for a, b in zip(ref, plain))
    return frames, [(f, np.asarray(t, np.float32).reshape(len(t), -1, 2), np.asarray(q, np.float32).reshape(len(q), -1))
                    for f, t, q in ref]


def same_segments(got, ref):
    assert len(got) == len(ref) == 3
    for (gf, gt, gq), (rf, rt, rq) in zip(got, ref):
        assert gf == rf and len(gt) == len(rt) > 20
        assert same(gt, rt) and same(gq, rq)


def test_segment_tracker_push(loop):
    from iceberg_tracking_code_amd import SegmentTracker
    frames, ref = loop
    trk = SegmentTracker(250, 130, 2, LOOP_FP, LOOP_LK, max_pts=4096)
    try:
        got = [s for s in (trk.push(f) for f in frames) if s is not None]
        assert trk.ctx.get_detector() == (False, 0.04)
    finally:
        trk.close()
    same_segments(got, ref)


def test_segment_tracker_look_ahead(loop):
    """frames resident and announced six steps ahead: the candidates of a detection frame are prepared, its detection
    begun and staged before the frame is reached (seg_detect_prepare / _begin / _stage), under the tracker's detector"""
    from iceberg_tracking_code_amd import Context, SegmentTracker
    frames, ref = loop
    n = len(frames)
    ctx = Context(250, 130, n_slots=n, max_pts=4096)
    try:
        for i, f in enumerate(frames):
            ctx.upload_gray(i, f)
        trk = SegmentTracker(250, 130, 2, LOOP_FP, LOOP_LK, ctx=ctx)
        ctx.prof_enable(True)
        got = [s for s in (trk.push_slot(i, True, *[i + j if i + j < n else None for j in range(1, 7)]) for i in range(n))
               if s is not None]
        ctx.sync()
        ctx.prof_enable(False)
        launches = ctx.prof_table()["corner_candidates"]["launches"]
    finally:
        ctx.close()
    same_segments(got, ref)
    assert launches == 4          # one candidate launch per detection frame (0, 2, 4, 6): what was prepared was adopted


def test_default_untouched(hctx):
    img = frame(SIZES[1])
    hctx.upload_gray(0, img)
    args = (50, 0.01, 7, False, 5)
    before = hctx.good_features(0, *args)
    assert same_corners(before, R.good_features(img, 50, 0.01, 7, None, 5))
    hctx.set_detector(harris=True, k=0.04)
    assert hctx.get_detector() == (True, 0.04)
    during = hctx.good_features(0, *args)
    assert same_corners(during, H.good_features(img, 50, 0.01, 7, None, 5, True, 0.04)) and not same_corners(during, before)
    # an explicit False is honoured for its call, and the handle's setting is back behind it
    assert same_corners(hctx.good_features(0, *args, useHarrisDetector=False), before)
    assert hctx.get_detector() == (True, 0.04)
    assert same_corners(hctx.good_features(0, *args), during)
    hctx.set_detector(harris=False)
    assert hctx.get_detector() == (False, 0.04)
    assert same_corners(hctx.good_features(0, *args), before)
