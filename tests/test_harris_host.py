"""The Harris restatement's known answers, and what the library refuses before it touches a GPU.  No GPU needed."""
import ctypes as C
import itertools

import numpy as np
import pytest

import harris_restatement as H
import np_restatement as R

BLOCK_SIZES = (3, 4, 5, 7, 10)


@pytest.fixture(scope="module")
def frames():
    return [H.blob_frame(96, 70, 3), H.blob_frame(250, 130, 4)]


def test_constant_frame_gives_an_all_zero_map_and_no_corner():
    img = np.full((40, 50), 77, np.uint8)
    for bs in BLOCK_SIZES:
        for tail in (0, 1):
            m = H.harris_map(img, bs, 0.04, tail)
            assert m.dtype == np.float32 and m.shape == img.shape and not m.any()
        assert H.good_features(img, 0, 0.01, 5, None, bs, True, 0.04) is None


def test_ramp_is_negative_everywhere_and_gives_no_corner():
    """One gradient direction: det = 0 up to rounding, the trace is not.  -2.5e-8 in numpy."""
    m = H.harris_map(H.ramp_frame(), 5, 0.04)
    assert -1e-7 < m.max() < 0 and abs(m.max() + 2.5e-8) < 1e-9
    for md in (0, 5):
        assert H.good_features(H.ramp_frame(), 0, 0.01, md, None, 5, True, 0.04) is None
    # under a mask too: the masked maximum is negative, the cut above it, and nothing inside the mask passes
    mask = np.zeros((40, 60), np.uint8)
    mask[5:30, 10:50] = 255
    assert H.good_features(H.ramp_frame(), 0, 0.01, 5, mask, 5, True, 0.04) is None


def test_lattice_of_blobs_gives_corners_at_the_blobs():
    img, pos = H.lattice_frame()
    for bs, md, slack in ((5, 10, 0), (5, 0, 0), (3, 10, 1), (7, 15, 1)):
        p = H.good_features(img, 0, 0.05, md, None, bs, True, 0.04)
        got = [(int(x), int(y)) for x, y in p.reshape(-1, 2)]
        assert len(got) == len(pos), (bs, md)
        for x, y in pos:      # every blob has its corner, at the blob (blockSize 5: the very pixel)
            assert any(max(abs(x - gx), abs(y - gy)) <= slack for gx, gy in got), (bs, md, x, y)
        for (ax, ay), (bx, by) in itertools.combinations(got, 2):
            assert (ax - bx) ** 2 + (ay - by) ** 2 >= md * md
    # stronger blobs first: amplitudes fall along the lattice
    p = H.good_features(img, 5, 0.05, 10, None, 5, True, 0.04)
    assert [(int(x), int(y)) for x, y in p.reshape(-1, 2)] == pos[:5]


def test_min_distance_holds_between_every_pair(frames):
    for img in frames:
        for md in (5, 10):
            p = H.good_features(img, 0, 0.01, md, None, 5, True, 0.04).reshape(-1, 2)
            d = p[:, None, :] - p[None, :, :]
            d2 = (d ** 2).sum(-1) + np.eye(len(p)) * 1e9
            assert len(p) > 10 and d2.min() >= md * md


def test_a_larger_k_never_raises_the_map(frames):
    for img in frames:
        for bs in BLOCK_SIZES:
            for tail in (0, 1):
                maps = [H.harris_map(img, bs, k, tail) for k in (0.0, 0.04, 0.06, 0.15, 0.25)]
                for lo, hi in zip(maps[1:], maps[:-1]):
                    assert (lo <= hi).all(), (bs, tail)


def test_both_forms_give_the_same_corner_list(frames):
    """... and different last bits in a good part of the map: the forms are two, the list is one."""
    for img in frames + [H.blob_frame(517, 203, 5)]:
        for bs in BLOCK_SIZES:
            for k in (0.04, 0.15):
                m0, m1 = H.harris_map(img, bs, k, 0), H.harris_map(img, bs, k, 1)
                assert (m0.view(np.uint32) != m1.view(np.uint32)).mean() > 0.1
                p0, p1 = H.select(m0, 0, 0.01, 5), H.select(m1, 0, 0.01, 5)
                assert p0 is not None and len(p0) >= 15 and np.array_equal(p0, p1), (img.shape, bs, k)
                assert H.ties(m0, 0.01) == 0


def test_harris_off_is_the_default_restatement(frames):
    img = frames[0]
    assert np.array_equal(H.good_features(img, 0, 0.01, 5, None, 5), R.good_features(img, 0, 0.01, 5, None, 5))
    assert np.array_equal(H.HarrisRestatementCv.goodFeaturesToTrack(img, maxCorners=0, qualityLevel=0.01, minDistance=5),
                          R.good_features(img, 0, 0.01, 5, None, 3))
    assert np.array_equal(H.HarrisRestatementCv.goodFeaturesToTrack(img, maxCorners=0, qualityLevel=0.01, minDistance=5,
                                                                    useHarrisDetector=True, k=0.06, blockSize=5),
                          H.select(H.harris_map(img, 5, 0.06), 0, 0.01, 5))


def test_the_maps_share_their_sums_with_the_eigenvalue_map(frames):
    """cov_sums restates np_restatement.min_eig_map's sums: the eigenvalue formed from them is that map, bit for bit."""
    for img in frames:
        for bs in BLOCK_SIZES:
            a, b, c = H.cov_sums(img, bs)
            a, c = a * R.F(0.5), c * R.F(0.5)
            t = a - c
            assert np.array_equal(((a + c) - np.sqrt(t * t + b * b)).view(np.uint32), R.min_eig_map(img, bs).view(np.uint32))


def test_detector_calls_exist_and_refuse_a_null_handle():
    """What can be asked without a GPU: no handle exists there, so ICELK_EARG here is the handle check's, for a good kind
    and k as for kind 7 and k = nan.  The validation of kind and k itself needs a live handle:
    test_gpu_harris.py::test_bad_detector_arguments_on_a_live_handle."""
    from iceberg_tracking_code_amd import _lib
    lib = _lib.load()
    for name in ("icelk_set_detector", "icelk_get_detector", "icelk_harris_map"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.icelk_set_detector(None, 7, 0.04) == _lib.EARG
    assert lib.icelk_set_detector(None, 1, float("nan")) == _lib.EARG
    assert lib.icelk_set_detector(None, 1, 0.04) == _lib.EARG
    kind, k = C.c_int(-5), C.c_double(-5.0)
    assert lib.icelk_get_detector(None, C.byref(kind), C.byref(k)) == _lib.EARG and (kind.value, k.value) == (-5, -5.0)
    out = np.zeros((4, 4), np.float32)
    assert lib.icelk_harris_map(None, 0, 3, 0.04, out.ctypes.data_as(_lib.f32p), 4) == _lib.EARG


def test_api_refuses_what_it_does_not_do_before_the_gpu():
    import iceberg_tracking_code_amd as cv
    gray = np.zeros((48, 64), np.uint8)
    with pytest.raises(ValueError):
        cv.cornerHarris(gray, 3, 5, 0.04)
    with pytest.raises(ValueError):
        cv.cornerMinEigenVal(gray, 3, 5)
    with pytest.raises(ValueError):
        cv.cornerHarris(np.zeros((48, 64), np.float32), 3, 3, 0.04)
    with pytest.raises(ValueError):
        cv.cornerMinEigenVal(np.zeros((48, 64, 3), np.uint8), 3)
    with pytest.raises(ValueError):
        cv.cornerHarris(gray, 3, 3, float("nan"))
    with pytest.raises(ValueError):
        cv.goodFeaturesToTrack(gray, 10, 0.01, 5, useHarrisDetector=True, k=float("inf"))
    with pytest.raises(ValueError):     # the image is looked at before the detector: still the old refusal
        cv.goodFeaturesToTrack(np.zeros((48, 64), np.float32), 10, 0.01, 5, useHarrisDetector=True)
