"""The reset of a detector set's counters, by every route a detection can leave them, in every order -- a recording test:
written against the library before the three statements of the reset became one (corner_keys.h reset_counters), it passes
on that library and unchanged on this one.

What a detection leaves zeroed for the next one of its set (cell counts and fills, chunk totals, undecided counters,
accepted / candidate counts, prune key, key histogram) is reset by one of:

  D  device tail     seg_detect, minDistance >= 1: k_tail_order resets
  H  host tail       the same on a handle made under ICELK_HOST_TAIL=1: k_tail resets
  F  forced verdict  the same on a handle made under ICELK_TAIL_FORCE_STATUS: the device tail declines, resets nothing but
                     its own histogram, and the host's tail (k_tail) resets
  S  short           on a plain handle: a mask and a minDistance that leave fewer corners than maxCorners although pruning
                     is on -- the device tail declines by itself, the host redoes the stage unpruned (k_detect_reset mode 0
                     in between) and its tail (k_tail) resets
  Z  no grid         seg_detect with minDistance 0: no min-distance stage, k_tail resets a grid of no cells, and the next
                     detection finds its grid grown (k_detect_reset runs first)
  N  no segment      good_features: k_detect_reset resets

A stale counter shows only in the detection AFTER the one that left it, so the walks hold every ordered pair of routes.
ICELK_HOST_TAIL and ICELK_TAIL_FORCE_STATUS are read when a handle is made (icelk_create), not at the call, so no one
handle can take D, H and F: there are three handles, and each walks every ordered pair of the routes it can take --
plain {D, S, Z, N}: 16 pairs in 17 steps; host tail {H, N} and forced {F, N}: 4 pairs in 5 steps each.

Detector sets.  A handle has two (Ctx::dset[2], icelk_ctx.h) and a detection takes the first that has none in flight,
so set 1 works only while set 0 is busy.  Every segment step is therefore TWO detections, begun one after the other
(set 0: frame 0, set 1: frame 1), then staged / finished in that order: both sets see the walk.  good_features refuses to
run with a detection in flight, so route N exists on set 0 only; set 1 sees the walk without its N steps, which still
holds every ordered pair of the other routes (asserted below).  That is why the walks are no longer than for one set.

The steps alternate minDistance 3, 8, 25 (8560, 1200, 130 cells: five scan chunks against one, a grown and a shrunk
grid) and maxCorners 300, 0 (pruning on: prune key and key histogram live; and off).  After every detection its corners,
in order, equal those of a fresh handle given the same frame and arguments with no switch set."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 320, 240
SWITCHES = ("ICELK_HOST_TAIL", "ICELK_TAIL_FORCE_STATUS", "ICELK_NO_PRUNE", "ICELK_GENERIC_CORNERS", "ICELK_TWO_PASS_CORNERS")
MIN_DISTANCES, MAX_CORNERS = (3, 8, 25), (300, 0)
QUALITY, BLOCK = 0.007, 10
MAX_PTS = 8192
# every ordered pair of four routes (a de Bruijn sequence closed), and of two
WALK4 = (0, 0, 1, 0, 2, 0, 3, 1, 1, 2, 1, 3, 2, 2, 3, 3, 0)
WALK2 = (0, 0, 1, 1, 0)
HANDLES = {
    "plain": (None, "DSZN", WALK4),
    "host": (("ICELK_HOST_TAIL", "1"), "HN", WALK2),
    "forced": (("ICELK_TAIL_FORCE_STATUS", "4"), "FN", WALK2),
}


def pairs(seq):
    return set(zip(seq, seq[1:]))


def test_walks_hold_every_ordered_pair_on_both_sets():
    for _, routes, walk in HANDLES.values():
        on_set0 = [routes[i] for i in walk]
        on_set1 = [r for r in on_set0 if r != "N"]
        assert pairs(on_set0) == {(a, b) for a in routes for b in routes}
        seg = routes.replace("N", "")
        assert pairs(on_set1) == {(a, b) for a in seg for b in seg}


def frames(synth):
    return [synth.frame(W, H, 300 * i, -200 * i, 61) for i in range(2)]


def mask():
    m = np.zeros((H, W), np.uint8)
    m[40:200, 40:280] = 255      # room for fewer than 80 corners 25 px apart
    return m


def arguments(route, step):
    """maxCorners, qualityLevel, minDistance, use_mask, blockSize of a step"""
    if route == "S":
        return (80, QUALITY, 25, True, BLOCK)
    md = 0 if route == "Z" else MIN_DISTANCES[step % 3]
    return (MAX_CORNERS[step % 2], QUALITY, md, False, BLOCK)


_fresh = {}


def fresh(synth, slot, args):
    """the corners of a fresh handle, no switch set, for frame `slot` and these arguments; computed once"""
    if (slot, args) not in _fresh:
        from iceberg_tracking_code_amd import Context
        c = Context(W, H, n_slots=1, max_pts=MAX_PTS)
        try:
            c.upload_gray(0, frames(synth)[slot])
            if args[3]:
                c.set_mask(mask())
            got = c.good_features(0, *args)
            _fresh[(slot, args)] = np.zeros((0, 2), np.float32) if got is None else got.reshape(-1, 2)
        finally:
            c.close()
    return _fresh[(slot, args)]


def first_vertices(c):
    return c.seg_read()[0][:, 0, :]


@pytest.mark.parametrize("kind", list(HANDLES))
def test_corners_after_every_reset_route_equal_a_fresh_handles(synth, monkeypatch, kind):
    from iceberg_tracking_code_amd import Context
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    switch, routes, walk = HANDLES[kind]
    if switch:
        monkeypatch.setenv(*switch)
    c = Context(W, H, n_slots=2, max_pts=MAX_PTS)      # the two switches are read here
    if switch:
        monkeypatch.delenv(switch[0])
    try:
        for i, f in enumerate(frames(synth)):
            c.upload_gray(i, f)
        c.set_mask(mask())
        for step, r in enumerate(walk):
            route, where = routes[r], "%s step %d route %s" % (kind, step, routes[r])
            args = arguments(route, step)
            want = [fresh(synth, slot, args) for slot in range(2)]
            before = c.seg_tail_stats()
            if route == "N":
                got = c.good_features(0, *args)
                assert np.array_equal(got.reshape(-1, 2), want[0]), where
                assert c.seg_tail_stats() == (before[0], before[1] + 1), where      # the host's tail, no segment
                continue
            c.seg_detect_begin(0, *args)      # set 0
            c.seg_detect_begin(1, *args)      # set 1: set 0 has a detection in flight
            assert c.seg_detect_stage(args[0]) == len(want[0]), where
            c.seg_switch()
            assert np.array_equal(first_vertices(c), want[0]), where + " set 0"
            assert c.seg_detect_finish(args[0]) == len(want[1]), where
            assert np.array_equal(first_vertices(c), want[1]), where + " set 1"
            # which tail staged the two segments: the route is the one the step names
            by_device = 2 if route == "D" else 0
            assert c.seg_tail_stats() == (before[0] + by_device, before[1] + 2 - by_device), where
            assert len(want[0]) > 20 and len(want[1]) > 20, where
            if route == "S":
                assert len(want[0]) < args[0] and len(want[1]) < args[0], where
    finally:
        c.close()
