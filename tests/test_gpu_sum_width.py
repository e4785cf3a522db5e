"""The tuned tracker's two sum widths (lk_common.h, "narrow sums behind a guard") against the oracle, bit for bit: content
that passes the guard everywhere (synth, stretched k = 4), content that splits the waves between the arms (stretched
k = 8) and content that never passes (stripes), through icelk_pyrlk, the fused forward + backward call and the segment
loop, each with "lk_wide_sums" 0 and 1.  test_sum_width_host.py shows on the host that the inputs reach these regimes."""
import numpy as np
import pytest

import extreme_frames as xf
from test_sum_width_host import SEED, H, W, sum_width_points

pytestmark = pytest.mark.gpu

CRIT = (3, 30, 0.01)
# window -> the maxLevel test_gpu_extremes.py runs it at
WINDOWS = {(15, 15): 2, (21, 21): 3, (31, 31): 5, (35, 35): 4}
COUNTS = (1, 63, 64, 65, 300)     # waves around one group of 8 workgroups' worth of lanes; a joint launch has both jobs
FAMILIES = ("synth", "stretched4", "stretched8", "stripes")
N_FRAMES = 5                      # two three-frame segments (track_len 2): their pairs (1, 2) and (2, 3) share a launch
KEYS_FB = ("p1", "p0r", "err_fwd", "err_bwd", "dist", "st_fwd", "st_bwd", "valid")


def _stripe_frame(i):
    xs = np.arange(W) + i
    f = np.repeat(np.where((xs % 4) >= 2, 255, 0).astype(np.uint8)[None, :], H, 0)
    f[xf.band_rows(H), :] = 128
    return np.ascontiguousarray(f)


_frames = {}


def frames_of(family):
    """Five frames moving by 3 px / 2 px (stripes: one column) a frame; the first two are the pair of the host test."""
    if family not in _frames:
        from iceberg_tracking_code_amd import synth
        if family == "stripes":
            fr = [_stripe_frame(i) for i in range(N_FRAMES)]
            I, J, _ = xf.stripes(W, H)
        else:
            k = {"synth": 1, "stretched4": 4, "stretched8": 8}[family]
            fr = [synth.frame(W, H, 300 * i, -200 * i, SEED) for i in range(N_FRAMES)]
            fr = [xf.stretch(f, k) if k > 1 else f for f in fr]
            I, J = (xf.stretched(W, H, SEED, k=k)[:2]) if k > 1 else fr[:2]
        assert np.array_equal(fr[0], I) and np.array_equal(fr[1], J)
        _frames[family] = fr
    return _frames[family]


def _points():
    """The host test's 300 integer-cornered points; every second one moved off the pixel grid."""
    pts = sum_width_points(300).copy()
    pts[1::2] += np.random.RandomState(5).uniform(0.05, 0.95, (150, 2)).astype(np.float32)
    return pts


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def gctx():
    from iceberg_tracking_code_amd import Context
    c = Context(W, H, n_slots=2, max_pts=4096)
    yield c
    c.close()


_refs = {}


def _reference(orc, family, win):
    key = (family, win)
    if key not in _refs:
        I, J = frames_of(family)[:2]
        pts = _points()
        _refs[key] = (orc.pyrlk(I, J, pts, None, win, WINDOWS[win], CRIT), orc.track_fb(I, J, pts, win, WINDOWS[win], CRIT))
    return _refs[key]


@pytest.mark.parametrize("win", list(WINDOWS))
@pytest.mark.parametrize("family", FAMILIES)
def test_pyrlk_and_track_fb_under_both_sum_widths(gctx, orc, family, win):
    I, J = frames_of(family)[:2]
    gctx.upload_gray(0, I)
    gctx.upload_gray(1, J)
    pts = _points()
    ref, ref_fb = _reference(orc, family, win)
    if family != "stripes":
        assert ref[1].sum() > 150, int(ref[1].sum())
    level = WINDOWS[win]
    for n in COUNTS:
        for wide in (0, 1):
            gctx.set_variant("lk_wide_sums", wide)
            try:
                got = gctx.pyrlk(0, 1, pts[:n], None, win, level, CRIT)
                got_fb = gctx.track_fb(0, 1, pts[:n], win, level, CRIT)
            finally:
                gctx.set_variant("lk_wide_sums", 0)
            for x, z, name in zip(got, ref, ("nextPts", "status", "err")):
                assert np.array_equal(_bits(x), _bits(z[:n])), (family, win, n, wide, name)
            for k in KEYS_FB:
                assert np.array_equal(_bits(got_fb[k]), _bits(ref_fb[k][:n])), (family, win, n, wide, k)


def _feature_params(n):
    return dict(maxCorners=n, qualityLevel=0.005, minDistance=4, blockSize=5)


def _run_segments(frames, fp, lk, wide):
    from iceberg_tracking_code_amd import Context, SegmentTracker
    ctx = Context(W, H, n_slots=len(frames), max_pts=4096)
    try:
        ctx.set_variant("lk_wide_sums", wide)
        for i, f in enumerate(frames):
            ctx.upload_gray(i, f)
        trk = SegmentTracker(W, H, 2, fp, lk, ctx=ctx)
        segs = []
        trk.on_close = lambda first, closed: segs.append((first,) + ctx.seg_read(closed=closed))
        ctx.prof_enable(True)
        for i in range(len(frames)):
            trk.push_slot(i, False, *[i + k if i + k < len(frames) else None for k in range(1, 7)])
        trk.flush()
        ctx.sync()
        joint = ctx.prof_table().get("lk_fb_pair", {}).get("launches", 0)
    finally:
        ctx.close()
    return segs, joint


def _same_segments(got, ref, tag):
    assert len(got) == len(ref) == 2, tag
    for (gf, gt, gq), (rf, rt, rq) in zip(got, ref):
        assert gf == rf and len(gt) == len(rt), tag
        if len(rt) == 0:
            continue
        rt = np.asarray(rt, np.float32).reshape(len(rt), -1, 2)
        rq = np.asarray(rq, np.float32).reshape(len(rq), -1)
        assert gt.shape == rt.shape, tag
        assert np.array_equal(_bits(gt), _bits(rt)) and np.array_equal(_bits(gq), _bits(rq)), tag


@pytest.mark.parametrize("win", list(WINDOWS))
@pytest.mark.parametrize("family", FAMILIES)
def test_segments_under_both_sum_widths(orc, family, win):
    """Three-frame segments through SegmentTracker (templates handed from pair to pair, the pairs across the segment change
    in one joint launch) against the reference loop on the oracle."""
    from reference_loops import OracleCv, run_reference_loop
    frames = frames_of(family)
    lk = dict(winSize=win, maxLevel=WINDOWS[win], criteria=CRIT)
    for n in COUNTS:
        fp = _feature_params(n)
        ref = run_reference_loop(frames, 2, fp, lk, cv=OracleCv(orc))
        if family != "stripes" and n == 300:
            assert len(ref[0][1]) > 50, (family, win, len(ref[0][1]))
        for wide in (0, 1):
            got, joint = _run_segments(frames, fp, lk, wide)
            assert joint >= 1, (family, win, n, wide)
            _same_segments(got, ref, (family, win, n, wide))


@pytest.mark.parametrize("family", ["stretched8", "synth"])
def test_variant_switched_between_the_pairs_of_a_segment(family):
    """The pairs (0, 1) and (1, 2) of a segment under different settings (the second takes the templates the first left),
    the waiting pair (1, 2) and the next segment's first pair (2, 3) under different settings too: the tracks are those of
    one setting throughout, and pairs under different settings never share a launch."""
    from iceberg_tracking_code_amd import Context
    frames = frames_of(family)[:4]
    det = (300, 0.005, 4, False, 5)
    lk = ((21, 21), 3, CRIT, 1e-4, 1.0)
    ctx = Context(W, H, n_slots=4, max_pts=4096)
    try:
        for i, f in enumerate(frames):
            ctx.upload_gray(i, f)
        ctx.prof_enable(True)

        def run(settings):
            """settings: "lk_wide_sums" for the pairs (0, 1), (1, 2), (2, 3)"""
            ctx.prof_reset()
            ctx.seg_detect(0, *det)
            ctx.set_variant("lk_wide_sums", settings[0])
            ctx.seg_track(0, 1, *lk)
            ctx.set_variant("lk_wide_sums", settings[1])
            ctx.seg_track_defer(1, 2, *lk)
            ctx.seg_detect(2, *det)                  # the switch: the pair keeps waiting for a partner
            ctx.set_variant("lk_wide_sums", settings[2])
            ctx.seg_track(2, 3, *lk)
            ctx.set_variant("lk_wide_sums", 0)
            first = ctx.seg_read(closed=True)
            second = ctx.seg_read()
            prof = ctx.prof_table()
            return first, second, prof.get("lk_fb", {}).get("launches", 0), prof.get("lk_fb_pair", {}).get("launches", 0)

        want = run((0, 0, 0))
        assert want[2:] == (1, 1) and len(want[0][0]) > 50 and want[0][0].shape[1] == 3
        for settings in ((0, 1, 0), (1, 0, 1), (1, 1, 0), (0, 0, 1)):
            got = run(settings)
            assert got[2:] == (3, 0), (settings, got[2:])
            for a, b in zip(got[:2], want[:2]):
                assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])), settings
        assert run((1, 1, 1))[2:] == (1, 1)
    finally:
        ctx.close()
