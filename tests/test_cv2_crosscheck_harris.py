"""Opportunistic cross-check of the Harris restatement against a real OpenCV, where `import cv2` works; SKIPPED elsewhere.

It pins nothing: both forms of tests/harris_restatement.py are written from knowledge of upstream OpenCV, and which of them
(if either) an OpenCV build computes bit for bit depends on how it was built.  What is stated here is the agreement
tests/test_cv2_crosscheck.py asks of the default detector: the same corner set."""
import numpy as np
import pytest

import harris_restatement as H

cv2 = pytest.importorskip("cv2", reason="OpenCV not installed: the Harris forms stay unpinned")


def test_corner_harris_map_is_one_of_the_two_forms_or_close():
    g = H.blob_frame(250, 130, 4)
    for bs in (3, 5, 10):
        ref = cv2.cornerHarris(g, bs, 3, 0.04)
        forms = [H.harris_map(g, bs, 0.04, tail) for tail in (0, 1)]
        print("blockSize", bs, "bit-identical to lanes / tail:", [bool(np.array_equal(ref, f)) for f in forms])
        assert min(np.abs(ref - f).max() for f in forms) <= 1e-6 * np.abs(ref).max()


def test_good_features_with_harris():
    g = H.blob_frame(517, 203, 5)
    for kw in (dict(maxCorners=100, qualityLevel=0.01, minDistance=5, blockSize=5),
               dict(maxCorners=0, qualityLevel=0.01, minDistance=10, blockSize=3)):
        ref = cv2.goodFeaturesToTrack(g, mask=None, useHarrisDetector=True, k=0.04, **kw)
        got = H.good_features(g, kw["maxCorners"], kw["qualityLevel"], kw["minDistance"], None, kw["blockSize"], True, 0.04)
        assert ref is not None and got is not None
        assert set(map(tuple, ref.reshape(-1, 2))) == set(map(tuple, got.reshape(-1, 2)))
