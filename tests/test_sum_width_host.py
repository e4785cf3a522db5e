"""Host-side statement of the tuned tracker's narrow-sum guard (lk_common.h, "narrow sums behind a guard"): the inputs of
test_gpu_sum_width.py reach the regimes claimed there -- stretched noise that passes the guard everywhere (k = 4), that
splits the points between the two arms (k = 8), stripes that never pass -- and wherever the guard passes, the int64 total
fits 32 bits and its one conversion is the float the 64-bit path's sum_to_float gives.  No GPU."""
import numpy as np
import pytest

import extreme_frames as xf
from test_lk_limits import sum_to_float

W, H = 400, 300
WIN = (21, 21)
SEG = 7                      # Cfg<21, 21>::S: a lane holds one row segment of 7 pixels, 63 lanes busy
GUARD_BIAS = 1 << 25         # kSumGuardBias
GUARD = 1 << 26              # LKParams::sum_guard
SEED = 9                     # k = 4: largest lane partial 0.89 of the bound; k = 8: 24 % of the points at or above it


def sum_width_points(n=300):
    """Points whose 21x21 (and every odd) window has an integer top-left corner, 15 px inside the frame."""
    return np.floor(xf.points(np.random.RandomState(1), n, W, H, border=15)).astype(np.float32)


def sum_width_inputs():
    return {
        "stretched4": xf.stretched(W, H, SEED, k=4)[:2],
        "stretched8": xf.stretched(W, H, SEED, k=8)[:2],
        "stripes": xf.stripes(W, H)[:2],
    }


def lane_partials(b_px):
    """The 64 lane partials of a 21x21 window's per-pixel products: lane l = pixels (l % 3) * 7 .. + 6 of row l // 3."""
    lanes = np.asarray(b_px, np.int64).reshape(WIN[1], WIN[0] // SEG, SEG).sum(2).ravel()
    return np.concatenate([lanes, np.zeros(64 - lanes.size, np.int64)])


def guard_passes(lanes):
    """The kernel's test on one sum: no lane with (unsigned)(v + 2^25) >= 2^26 (v is an int32 in the lane)."""
    v = np.asarray(lanes, np.int64)
    assert np.abs(v).max() < 2 ** 31
    return bool((((v + GUARD_BIAS) & 0xffffffff) < GUARD).all())


@pytest.fixture(scope="module")
def partials():
    pts = sum_width_points()
    out = {}
    for name, (I, J) in sum_width_inputs().items():
        sums = xf.window_sums(I, J, pts, WIN)
        assert len(sums) == len(pts) == 300
        out[name] = [(lane_partials(s["b1_px"]), s["b1"]) for s in sums]
    return out


def _share_at_or_above(rows):
    return np.mean([np.abs(l).max() >= GUARD_BIAS for l, _ in rows])


def test_stretched8_splits_the_points_between_the_arms(partials):
    share = _share_at_or_above(partials["stretched8"])
    print("stretched k=8: %.3f of the points have a lane partial of diff*Ix at or above 2^25" % share)
    assert 0.10 <= share <= 0.90


def test_stretched4_passes_the_guard_everywhere(partials):
    top = max(np.abs(l).max() for l, _ in partials["stretched4"])
    print("stretched k=4: largest lane partial %.3f of 2^25" % (top / GUARD_BIAS))
    assert top < GUARD_BIAS
    assert _share_at_or_above(partials["stretched4"]) == 0.0


def test_stripes_never_pass_the_guard(partials):
    assert _share_at_or_above(partials["stripes"]) == 1.0
    assert not any(guard_passes(l) for l, _ in partials["stripes"])


def _check_narrow(lanes, total):
    """Where the guard passes: every prefix of the lanes and the total fit int32, and one conversion is sum_to_float's."""
    assert int(lanes.sum()) == total
    if not guard_passes(lanes):
        return False
    pre = np.cumsum(lanes)
    assert -2 ** 31 <= pre.min() and pre.max() <= 2 ** 31 - 1
    narrow = np.float32(np.int32(total))
    assert narrow.view(np.uint32) == sum_to_float(total).astype(np.float32).view(np.uint32), total
    return True


def test_guard_implies_int32_total_and_the_same_float(partials):
    passed = {name: sum(_check_narrow(l, t) for l, t in rows) for name, rows in partials.items()}
    print("points that pass the guard:", passed)
    assert passed["stretched4"] == 300 and passed["stripes"] == 0 and 30 <= passed["stretched8"] <= 270
    # the extremes the guard lets through: 64 lanes at 2^25 - 1 and at -(2^25 - 1) (totals +-(2^31 - 64)), and at -2^25
    for v in (GUARD_BIAS - 1, -(GUARD_BIAS - 1), -GUARD_BIAS):
        lanes = np.full(64, v, np.int64)
        assert _check_narrow(lanes, 64 * v)
    assert 64 * (GUARD_BIAS - 1) == 2 ** 31 - 64
    # one step beyond on either side does not pass
    for v in (GUARD_BIAS, -GUARD_BIAS - 1):
        lanes = np.zeros(64, np.int64)
        lanes[17] = v
        assert not guard_passes(lanes)


def test_unsigned_rule_of_the_matrix_sums():
    """a11 and a22 are never negative: lanes below 2^26 give totals below 2^32, converted as unsigned."""
    for v in (GUARD - 1, 12345, 0):
        lanes = np.full(64, v, np.int64)
        assert ((lanes & 0xffffffff) < GUARD).all()
        t = int(lanes.sum())
        assert t < 2 ** 32 and np.cumsum(lanes).max() < 2 ** 32
        assert np.float32(np.uint32(t)).view(np.uint32) == sum_to_float(t).astype(np.float32).view(np.uint32)
    assert 64 * (GUARD - 1) == 2 ** 32 - 64
