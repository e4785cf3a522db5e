"""The corner detector's host driver at its edges: calls out of order, a failed stage with a second detection in flight,
the paths no device-driven tail can take, the unpruned redo behind a device verdict, and every forced verdict.  These
record what the driver does (errors, what stays in flight, which tail staged the segment); the happy paths are in
test_gpu_api.py and test_gpu_parity.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 320, 240
DET = (300, 0.007, 8, False, 10)    # maxCorners, qualityLevel, minDistance, use_mask, blockSize
LK = dict(winSize=(21, 21), maxLevel=3, criteria=(3, 30, 0.01))
SWITCHES = ("ICELK_HOST_TAIL", "ICELK_TAIL_FORCE_STATUS", "ICELK_NO_PRUNE", "ICELK_GENERIC_CORNERS", "ICELK_TWO_PASS_CORNERS")
ESTATE, ECAP = "-5", "-4"


def clear_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def context(synth, n_frames=2, max_pts=4096, seed=61):
    from iceberg_tracking_code_amd import Context
    c = Context(W, H, n_slots=n_frames, max_pts=max_pts)
    for i in range(n_frames):
        c.upload_gray(i, synth.frame(W, H, 300 * i, -200 * i, seed))
    return c


def first_vertices(c):
    return c.seg_read()[0][:, 0, :]


def same(corners, want):
    return np.array_equal(np.asarray(corners).reshape(-1, 2), np.asarray(want).reshape(-1, 2))


def test_stage_and_finish_with_nothing_in_flight(synth, monkeypatch):
    clear_switches(monkeypatch)
    from iceberg_tracking_code_amd._lib import IcelkError
    c = context(synth)
    try:
        for call in (c.seg_detect_stage, c.seg_detect_finish):
            with pytest.raises(IcelkError, match=ESTATE):
                call(DET[0])
        want = c.good_features(0, *DET)
        assert c.seg_detect(0, *DET) == len(want) > 100      # and the handle is as good as new
        with pytest.raises(IcelkError, match=ESTATE):
            c.seg_detect_stage(DET[0])
    finally:
        c.close()


def test_stage_while_a_staged_segment_waits(synth, monkeypatch):
    clear_switches(monkeypatch)
    from iceberg_tracking_code_amd._lib import IcelkError
    c = context(synth)
    try:
        want = [c.good_features(i, *DET) for i in range(2)]
        c.seg_detect_begin(0, *DET)
        c.seg_detect_begin(1, *DET)
        assert c.seg_detect_stage(DET[0]) == len(want[0])
        with pytest.raises(IcelkError, match=ESTATE):
            c.seg_detect_stage(DET[0])
        with pytest.raises(IcelkError, match=ESTATE):
            c.seg_detect_finish(DET[0])
        c.seg_switch()
        assert same(first_vertices(c), want[0])
        assert c.seg_detect_finish(DET[0]) == len(want[1]) > 100      # the one in flight is still there
        assert same(first_vertices(c), want[1])
    finally:
        c.close()


def test_stage_with_another_max_corners_drops_the_detection(synth, monkeypatch):
    clear_switches(monkeypatch)
    from iceberg_tracking_code_amd._lib import IcelkError
    c = context(synth)
    try:
        want = c.good_features(0, *DET)
        before = c.seg_tail_stats()
        c.seg_detect_begin(0, *DET)
        with pytest.raises(IcelkError, match=ESTATE):
            c.seg_detect_stage(DET[0] - 100)
        with pytest.raises(IcelkError, match=ESTATE):      # gone: nothing is in flight
            c.seg_detect_stage(DET[0])
        assert c.seg_tail_stats() == before
        c.seg_detect_begin(0, *DET)
        assert c.seg_detect_finish(DET[0]) == len(want) == DET[0]
        assert same(first_vertices(c), want)
        assert c.seg_tail_stats() == (before[0] + 1, before[1])
    finally:
        c.close()


@pytest.mark.parametrize("how", ["max_corners", "max_pts"])
def test_failed_stage_of_the_older_detection_strands_the_younger(synth, monkeypatch, how):
    """The younger detection's tail has written the set behind the one the older reserved; with the older gone, its
    stage is offered another set and refused, until icelk_seg_detect_cancel."""
    clear_switches(monkeypatch)
    from iceberg_tracking_code_amd._lib import IcelkError
    c = context(synth, max_pts=64 if how == "max_pts" else 4096)
    try:
        begun = (0,) + DET[1:] if how == "max_pts" else DET      # uncapped: more corners than max_pts = 64
        good = (64,) + DET[1:] if how == "max_pts" else DET
        want = [c.good_features(i, *good) for i in range(2)]
        c.seg_detect_begin(0, *begun)
        c.seg_detect_begin(1, *begun)
        if how == "max_pts":
            with pytest.raises(IcelkError, match=ECAP):
                c.seg_detect_stage(begun[0])
        else:
            with pytest.raises(IcelkError, match=ESTATE):
                c.seg_detect_stage(begun[0] - 100)
        with pytest.raises(IcelkError, match=ESTATE):
            c.seg_detect_stage(begun[0])
        with pytest.raises(IcelkError, match=ESTATE):      # both are gone now
            c.seg_detect_stage(begun[0])
        c.seg_detect_cancel()
        for i in range(2):
            assert same(c.good_features(i, *good), want[i])
            assert c.seg_detect(i, *good) == len(want[i]) >= 64
            assert same(first_vertices(c), want[i])
    finally:
        c.close()


def test_min_distance_zero_on_the_segment_path(synth, monkeypatch):
    clear_switches(monkeypatch)
    c = context(synth)
    try:
        det = (500, 0.007, 0, False, 10)
        want = c.good_features(0, *det)
        before = c.seg_tail_stats()
        assert c.seg_detect(0, *det) == len(want) == 500
        assert same(first_vertices(c), want)
        assert c.seg_tail_stats() == (before[0], before[1] + 1)
        stats = c.detect_stats()
        assert stats["candidates"] == stats["accepted"] > 500
    finally:
        c.close()


def test_unpruned_redo_behind_a_device_verdict(synth, monkeypatch):
    """A mask and a minDistance that leave fewer corners than maxCorners although there are more than 8 * maxCorners
    candidates: the pruned set falls short, the device's verdict says so, and the host runs the stage again on all."""
    clear_switches(monkeypatch)
    c = context(synth)
    try:
        mask = np.zeros((H, W), np.uint8)
        mask[20:220, 20:300] = 255
        c.set_mask(mask)
        det = (80, 0.007, 25, True, 10)
        monkeypatch.setenv("ICELK_NO_PRUNE", "1")
        want = c.good_features(0, *det)
        monkeypatch.delenv("ICELK_NO_PRUNE")
        before = c.seg_tail_stats()
        n = c.seg_detect(0, *det)
        assert n == len(want) and same(first_vertices(c), want)
        assert c.seg_tail_stats() == (before[0], before[1] + 1)
        stats = c.detect_stats()
        assert 20 < n < det[0] and stats["accepted"] == n and stats["candidates"] > 8 * det[0]
    finally:
        c.close()


_unforced = {}


def one_segment(synth, max_corners):
    c = context(synth, max_pts=256)
    try:
        n = c.seg_detect(0, max_corners, *DET[1:])
        c.seg_track(0, 1, **LK)
        tracks, quality = c.seg_read()
        return n, tracks, quality, c.seg_tail_stats()
    finally:
        c.close()


@pytest.mark.parametrize("status", [2, 3, 4])
def test_forced_device_verdicts(synth, monkeypatch, status):
    """ICELK_TAIL_FORCE_STATUS: pruned set fell short (2) and skewed bins (4) hand the tail to the host, which gives the
    segment the device would have; more corners than the tables hold (3) is an error."""
    clear_switches(monkeypatch)
    from iceberg_tracking_code_amd._lib import IcelkError
    if not _unforced:
        _unforced["run"] = one_segment(synth, 200)
    n, tracks, quality, tails = _unforced["run"]
    assert n == 200 and len(tracks) > 50 and tails == (1, 0)
    monkeypatch.setenv("ICELK_TAIL_FORCE_STATUS", str(status))
    if status == 3:
        with pytest.raises(IcelkError, match=ECAP):
            one_segment(synth, 200)
        return
    fn, ft, fq, ftails = one_segment(synth, 200)
    assert fn == n and np.array_equal(ft, tracks) and np.array_equal(fq, quality) and ftails == (0, 1)
