"""GPU parity of the tuned kernels' template build at every position a template can take against the frame edge.

The template of k_lk_fast / k_lk_multi is built from derivatives formed four times too large, whose rounding shift,
packing and window mask are one v_perm with a per-lane selector, from pixel pairs taken out of unaligned LDS dwords;
a template that reaches over the frame edge clears its out-of-frame derivatives under one branch for both derivative
rows.  Here each window of the tuned kernels is centred at every offset from -(half window + 2) to +(half window + 2)
px across each of the four edges -- on every pyramid level, since the points are scaled down level by level -- on
content whose derivatives reach the Scharr bound.  Forward and fused forward + backward results must match the oracle
bit for bit through both tuned kernels."""
import numpy as np
import pytest

import extreme_frames as xf

pytestmark = pytest.mark.gpu

W, H = 320, 240
CRIT = (3, 30, 0.01)
# window -> the maxLevel the bench / the parity tests run it at
WINDOWS = {(15, 15): 2, (21, 21): 3, (31, 31): 5, (35, 35): 4}
KEYS_FB = ("p1", "p0r", "err_fwd", "err_bwd", "dist", "st_fwd", "st_bwd", "valid")


@pytest.fixture(scope="module")
def gctx():
    from iceberg_tracking_code_amd import Context
    c = Context(W, H, n_slots=2, max_pts=1 << 14)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def edge_points(win, w, h, seed):
    """Window centres at every integer offset across the four edges (the window's own half-size past the edge down to
    as far inside: every byte phase of the patch origin), each with a fraction from a fixed set (quarters, ties,
    near-integers)."""
    rng = np.random.RandomState(seed)
    r = win[0] // 2 + 2
    fr = np.array([0.0, 0.25, 0.5, 0.75, 0.125, 0.999, 0.001, 0.6], np.float32)
    offs = np.arange(-r, r + 1, dtype=np.float32)
    pts = []
    for k, o in enumerate(offs):
        f = fr[k % len(fr)]
        x, y = rng.uniform(2 * r, w - 2 * r), rng.uniform(2 * r, h - 2 * r)
        pts += [(o + f, y), (w - 1 - o - f, y), (x, o + f), (x, h - 1 - o - f)]   # left, right, top, bottom
    # the four corners
    pts += [(cx + f, cy + f) for cx in (1.0 - r, w - r) for cy in (1.0 - r, h - r) for f in (0.0, 0.5)]
    return np.asarray(pts, np.float32)


@pytest.mark.parametrize("family", ["mondrian", "stretched16"])
@pytest.mark.parametrize("win", list(WINDOWS))
def test_templates_across_the_frame_edge(gctx, orc, family, win):
    from iceberg_tracking_code_amd.context import LK_MULTI_PER_WAVE
    I, J, _ = xf.FAMILIES[family](W, H, 5)
    gctx.upload_gray(0, I)
    gctx.upload_gray(1, J)
    pts = edge_points(win, W, H, 7 + win[0])
    for level in (0, WINDOWS[win]):
        ref = orc.pyrlk(I, J, pts, None, win, level, CRIT)
        ref_fb = orc.track_fb(I, J, pts, win, level, CRIT)
        assert ref[1].sum() >= 0.3 * len(pts), (family, win, level, int(ref[1].sum()))
        for which in (0, LK_MULTI_PER_WAVE):
            gctx.set_lk_kernel(which)
            try:
                got = gctx.pyrlk(0, 1, pts, None, win, level, CRIT)
                got_fb = gctx.track_fb(0, 1, pts, win, level, CRIT)
            finally:
                gctx.set_lk_kernel(0)
            tag = (family, win, level, which)
            for x, z, name in zip(got, ref, ("nextPts", "status", "err")):
                assert np.array_equal(_bits(x), _bits(z)), tag + (name, int((_bits(x) != _bits(z)).sum()))
            for k in KEYS_FB:
                assert np.array_equal(_bits(got_fb[k]), _bits(ref_fb[k])), tag + (k,)
