"""The schedule of `SegmentTracker` -- which `Context` calls it makes, in which order, with which arguments -- against
the recorded traces of tests/golden/tracker_traces.json.gz (tests/tracker_trace.py has the recorder and the
scenarios).  Host only: the tracker drives whatever object it is given, so a change that leaves every trace equal
sends the device what it was sent before.  A change of schedule regenerates the file
(tests/golden/make_tracker_traces.py) and shows up as its difference."""
import gzip
import json
import os

import pytest

import tracker_trace

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tracker_traces.json.gz")

# every Context method iceberg_tracking_code_amd/tracker.py calls (`self.ctx.<name>(`)
CONTEXT_METHODS = (
    "build_pyramid_ahead", "close", "drop_pyramid", "jpeg_async_finish", "jpeg_async_finish_file", "jpeg_async_poll",
    "jpeg_resave_file", "seg_detect_begin", "seg_detect_cancel", "seg_detect_finish", "seg_detect_prepare",
    "seg_detect_stage", "seg_detect_stage_try", "seg_flush", "seg_live", "seg_plot", "seg_read", "seg_switch",
    "seg_track", "seg_track_defer", "seg_track_len_hint", "set_gray_device", "set_mask", "set_mask_polygon",
    "synth_frame", "upload_bgr", "upload_gray", "upload_gray_async", "upload_jpeg", "upload_jpeg_file",
    "upload_jpeg_file_async")


@pytest.fixture(scope="module")
def golden():
    with gzip.open(GOLDEN, "rb") as f:
        return json.loads(f.read().decode())


def _mismatch(key, got, want):
    i = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
    lines = ["%s: first difference at entry %d (%d entries, golden %d)" % (key, i, len(got), len(want))]
    for name, trace in (("golden", want), ("now", got)):
        lines += ["  %-6s %4d%s %s" % (name, j, ">" if j == i else " ", trace[j])
                  for j in range(max(i - 3, 0), min(i + 4, len(trace)))]
    return "\n".join(lines)


def test_every_scenario_replays_its_golden_trace(golden, monkeypatch):
    assert set(golden) == set(tracker_trace.SCENARIOS)
    wrong = []
    for key in sorted(golden):
        got = tracker_trace.run(key, monkeypatch)
        if got != golden[key]:
            wrong.append(_mismatch(key, got, golden[key]))
    assert not wrong, "%d of %d scenarios differ\n%s" % (len(wrong), len(golden), "\n".join(wrong[:3]))


def test_golden_is_not_hollow(golden):
    assert len(golden) >= 500
    called = {e[0] for trace in golden.values() for e in trace}
    assert not set(CONTEXT_METHODS) - called
    assert len(CONTEXT_METHODS) == 31


def _names(trace):
    return [e[0] for e in trace]


def test_golden_holds_a_joint_launch(golden):
    def joint(trace):
        n = _names(trace)
        return any(n[i:i + 3] == ["seg_track_defer", "seg_switch", "seg_track"] for i in range(len(n)))
    assert any(joint(t) for t in golden.values())


def test_golden_holds_a_try_that_was_not_ready_and_came_again_a_step_later(golden):
    def retried(key, trace):
        # the recorder's first answer to seg_detect_stage_try is None in these scenarios (tracker_trace.TRIES)
        if "/tries=F" not in key:
            return False
        n = _names(trace)
        if n.count("seg_detect_stage_try") < 2:
            return False
        first = n.index("seg_detect_stage_try")
        between = n[first + 1:n.index("seg_detect_stage_try", first + 1)]
        return between.count("returns") == 1 and "seg_detect_stage" not in between
    assert any(retried(k, t) for k, t in golden.items())


def test_golden_holds_two_detections_in_flight(golden):
    def two(trace):
        n = [x for x in _names(trace) if x in ("seg_detect_begin", "seg_detect_finish", "seg_detect_stage",
                                               "seg_detect_stage_try")]
        return any(a == b == "seg_detect_begin" for a, b in zip(n, n[1:]))
    assert any(two(t) for t in golden.values())


def test_golden_holds_on_close_both_ways(golden):
    seen = {e[2] for trace in golden.values() for e in trace if e[0] == "on_close"}
    assert seen == {True, False}
