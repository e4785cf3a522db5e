"""GPU parity at the limits of the tracker's integer arithmetic: the content families of extreme_frames.py (saturated
blocks, stretched noise, inverted frames, bound-hitting stripes, flat saturated patches) through every LK kernel, the
fused forward + backward launch, the lk_sums variants, the segment loop with its template hand-over and the corner
detectors -- every output bit for bit against the oracle.  test_lk_limits.py checks on the host that these frames reach
the regimes claimed here (sums beyond 2^31 / 2^32, generic-kernel lanes near 2^31) and that the oracle is right there."""
import time

import numpy as np
import pytest

import extreme_frames as xf

pytestmark = pytest.mark.gpu

W, H = 400, 300
CRIT_DEFAULT = (3, 30, 0.01)
# window -> the maxLevel the bench / the existing parity tests run it at
WINDOWS = {(15, 15): 2, (21, 21): 3, (31, 31): 5, (35, 35): 4, (41, 41): 2, (64, 64): 1}
KEYS_FB = ("p1", "p0r", "err_fwd", "err_bwd", "dist", "st_fwd", "st_bwd", "valid")


@pytest.fixture(scope="module")
def gctx():
    from iceberg_tracking_code_amd import Context
    c = Context(1024, 768, n_slots=4, max_pts=1 << 16)
    yield c
    c.close()


def _kernels():
    from iceberg_tracking_code_amd.context import LK_GENERIC_KERNEL, LK_MULTI_PER_WAVE
    return (0, LK_MULTI_PER_WAVE, LK_GENERIC_KERNEL)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same_lk(got, ref, tag):
    for x, z, name in zip(got, ref, ("nextPts", "status", "err")):
        assert np.array_equal(_bits(x), _bits(z)), (tag, name, int((_bits(x) != _bits(z)).sum()))


def _same_fb(got, ref, tag):
    for k in KEYS_FB:
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), (tag, k)


def _family_points(family, w, h, win, seed):
    rng = np.random.RandomState(seed)
    if family == "stripes":
        return np.concatenate([xf.stripe_points(w, h, win, n=60), xf.points(rng, 40, w, h)])
    pts = xf.points(rng, 300, w, h, border=-15.0)
    if family == "saturated":
        pts = np.concatenate([xf.saturated_points(w, h), pts])
    return pts


def _min_alive(family, win, level, n):
    """How many points must stay alive (status 1) for the comparison to be about tracked points.  Inverted pairs keep
    fewer (the residual never vanishes); stripes keep the band points."""
    if family == "inverted":
        return 0.1 * n
    if family == "stripes":
        return 20
    return 0.3 * n


@pytest.mark.parametrize("family", list(xf.FAMILIES))
def test_pyrlk_and_track_fb_on_extreme_content(gctx, orc, family):
    """Every window of the tuned kernels and two generic ones, at maxLevel 0 and at the bench level, through each kernel
    (the default, several features per wave, the generic one), points inside and up to 15 px beyond the borders."""
    I, J, _ = xf.FAMILIES[family](W, H, 3)
    gctx.upload_gray(0, I)
    gctx.upload_gray(1, J)
    for k, (win, bench_level) in enumerate(WINDOWS.items()):
        pts = _family_points(family, W, H, win, 100 + k)
        for level in (0, bench_level):
            tag = (family, win, level)
            ref = orc.pyrlk(I, J, pts, None, win, level, CRIT_DEFAULT)
            ref_fb = orc.track_fb(I, J, pts, win, level, CRIT_DEFAULT)
            assert ref[1].sum() >= _min_alive(family, win, level, len(pts)), (tag, int(ref[1].sum()))
            for which in _kernels():
                gctx.set_lk_kernel(which)
                try:
                    got = gctx.pyrlk(0, 1, pts, None, win, level, CRIT_DEFAULT)
                    got_fb = gctx.track_fb(0, 1, pts, win, level, CRIT_DEFAULT)
                finally:
                    gctx.set_lk_kernel(0)
                _same_lk(got, ref, tag + (which,))
                _same_fb(got_fb, ref_fb, tag + (which,))


@pytest.mark.parametrize("crit", [(1, 1, 0.0), CRIT_DEFAULT])
def test_bound_hitting_stripes(gctx, orc, crit):
    """Integer-cornered windows on the stripes, zero guess: the first iteration's b1 has lane partials of the generic
    kernel within a few per cent of 2^31 at 64x64 and the largest group sums at 21/35/41."""
    I, J, _ = xf.stripes(W, H)
    gctx.upload_gray(0, I)
    gctx.upload_gray(1, J)
    for win in ((64, 64), (21, 21), (35, 35), (41, 41), (15, 15), (31, 31)):
        pts = xf.stripe_points(W, H, win, n=64)
        ref = orc.pyrlk(I, J, pts, None, win, 0, crit)
        assert ref[1].sum() == len(pts), win
        for which in _kernels():
            gctx.set_lk_kernel(which)
            try:
                got = gctx.pyrlk(0, 1, pts, None, win, 0, crit)
                got_fb = gctx.track_fb(0, 1, pts, win, 0, crit)
            finally:
                gctx.set_lk_kernel(0)
            _same_lk(got, ref, (win, crit, which))
            _same_fb(got_fb, orc.track_fb(I, J, pts, win, 0, crit), (win, crit, which))


@pytest.mark.parametrize("family", ["stretched16", "blocks2", "mondrian"])
def test_sub_ulp_weight_points(gctx, orc, family):
    """Positions whose float32 fractions give iw11 = -1 or a rounding tie: as the template position (prevPts) and as the
    iteration's position (an INITIAL_FLOW guess there, COUNT 1), at maxLevel 0 so they reach the kernel unscaled."""
    I, J, _ = xf.FAMILIES[family](W, H, 9)
    gctx.upload_gray(0, I)
    gctx.upload_gray(1, J)
    for win in ((15, 15), (21, 21), (31, 31), (35, 35), (41, 41)):
        pts, wts = xf.sub_ulp_points(win, base=(110.0, 110.0))
        pts2, _ = xf.sub_ulp_points(win, base=(250.0, 190.0))
        pts = np.concatenate([pts, pts2])
        assert any(t[3] == -1 for t in wts) and len(pts) >= 20
        shifted = pts + np.float32([1.25, -0.75])
        for which in _kernels():
            gctx.set_lk_kernel(which)
            try:
                for p0, p1, flags, crit in ((pts, None, 0, CRIT_DEFAULT), (pts, None, 0, (1, 1, 0.0)),
                                            (shifted, pts, 4, (1, 1, 0.0)), (pts, pts, 12, CRIT_DEFAULT)):
                    got = gctx.pyrlk(0, 1, p0, p1, win, 0, crit, flags)
                    ref = orc.pyrlk(I, J, p0, p1, win, 0, crit, flags)
                    assert ref[1].sum() > len(pts) // 2
                    _same_lk(got, ref, (win, which, flags, crit))
            finally:
                gctx.set_lk_kernel(0)


@pytest.mark.parametrize("value", [1, 2])
@pytest.mark.parametrize("family", ["blocks2", "stretched16"])
def test_lk_sums_variants_on_extreme_content(orc, family, value):
    """The float-lane sums of the x86 SIMD blocks round at almost every addition when the terms are near 10^10."""
    from iceberg_tracking_code_amd import Context
    I, J, _ = xf.FAMILIES[family](W, H, 4)
    pts = _family_points(family, W, H, (21, 21), 7)
    c = Context(W, H, n_slots=2, max_pts=4096)
    try:
        c.upload_gray(0, I)
        c.upload_gray(1, J)
        for win, lvl in (((21, 21), 3), ((35, 35), 4), ((21, 21), 0), ((35, 35), 0)):
            base = c.track_fb(0, 1, pts, win, lvl, CRIT_DEFAULT)
            c.set_variant("lk_sums", value)
            try:
                got = c.track_fb(0, 1, pts, win, lvl, CRIT_DEFAULT)
            finally:
                c.set_variant("lk_sums", 0)
            with orc.variants(lk_sums=value):
                ref = orc.track_fb(I, J, pts, win, lvl, CRIT_DEFAULT)
            _same_fb(got, ref, (win, lvl))
            assert ref["st_fwd"].sum() > len(pts) // 3
            if lvl == 0:
                assert (got["p1"] != base["p1"]).any(), "the variant is not live"
    finally:
        c.close()


def _sequence(w, h, n, inverted_at):
    """Stretched synth frames moving by up to 2 px per frame, one of them inverted."""
    from iceberg_tracking_code_amd import synth
    sh = synth.shifts(n, seed=61, max_step_px=2.0)
    frames = [xf.stretch(synth.frame(w, h, int(sx), int(sy), 61), 16) for sx, sy in sh]
    frames[inverted_at] = (255 - frames[inverted_at]).astype(np.uint8)
    return frames


@pytest.mark.parametrize("win,levels", [((21, 21), 3), ((35, 35), 4)])
@pytest.mark.parametrize("track_len", [1, 2, 3])
def test_segments_with_template_hand_over(orc, monkeypatch, win, levels, track_len):
    """SegmentTracker against the reference loop on the oracle, with and without the template hand-over (35x35 keeps the
    handed-over window as 16-bit samples); the hand-over did take place."""
    from iceberg_tracking_code_amd import Context, SegmentTracker
    from reference_loops import OracleCv, run_reference_loop
    w, h, n = 400, 300, 9
    frames = _sequence(w, h, n, inverted_at=5)
    fp = dict(maxCorners=0, qualityLevel=0.005, minDistance=4, blockSize=5)
    lk = dict(winSize=win, maxLevel=levels, criteria=CRIT_DEFAULT)
    ref = run_reference_loop(frames, track_len, fp, lk, cv=OracleCv(orc))

    def run():
        ctx = Context(w, h, n_slots=n, max_pts=8192)
        for i, f in enumerate(frames):
            ctx.upload_gray(i, f)
        trk = SegmentTracker(w, h, track_len, fp, lk, ctx=ctx)
        segs = []
        trk.on_close = lambda first, closed: segs.append((first,) + ctx.seg_read(closed=closed))
        for i in range(n):
            trk.push_slot(i, False, *[i + k if i + k < n else None for k in range(1, 7)])
        trk.flush()
        ctx.sync()
        st = ctx.seg_template_stats()
        trk.close()
        return segs, st

    a, (taken, left) = run()
    monkeypatch.setenv("ICELK_NO_TEMPLATE_REUSE", "1")
    b, off = run()
    monkeypatch.delenv("ICELK_NO_TEMPLATE_REUSE")
    assert off == (0, 0)
    if track_len > 1:
        assert taken >= 1 and left >= taken
    assert len(a) == len(b) == len(ref) >= 2
    for segs in (a, b):
        for (gf, gt, gq), (rf, rt, rq) in zip(segs, ref):
            assert gf == rf and len(gt) == len(rt)
            if len(rt) == 0:            # every track of the segment was lost across the inverted frame
                continue
            rt = np.asarray(rt, np.float32).reshape(len(rt), -1, 2)
            rq = np.asarray(rq, np.float32).reshape(len(rq), -1)
            assert gf == rf and gt.shape == rt.shape
            assert np.array_equal(_bits(gt), _bits(rt)) and np.array_equal(_bits(gq), _bits(rq)), gf
    assert max(len(s[1]) for s in a) > 100


@pytest.mark.parametrize("family", ["blocks2", "blocks3", "mondrian", "stripes"])
@pytest.mark.parametrize("bs", [3, 5, 7, 10])
def test_detection_on_binary_content(gctx, orc, monkeypatch, family, bs):
    """goodFeaturesToTrack and the segment detector on 0/255 content (|dxi| = 1 020 at most pixels, ties everywhere),
    fused and generic corner kernels.  Binary content stays at or below 1024x768 (k_tail_rank's bin path)."""
    w, h = (1024, 768) if family == "mondrian" else (640, 480)
    I, _, _ = xf.FAMILIES[family](w, h, 2)
    gctx.upload_gray(2, I)
    for maxc, q, md in ((0, 0.01, 5), (500, 0.05, 10)):
        ref = orc.good_features(I, maxc, q, md, None, bs)
        for generic in (False, True):
            if generic:
                monkeypatch.setenv("ICELK_GENERIC_CORNERS", "1")
            t0 = time.perf_counter()
            got = gctx.good_features(2, maxc, q, md, False, bs)
            dt = time.perf_counter() - t0
            n = gctx.seg_detect(2, maxc, q, md, False, bs)
            seg, _ = gctx.seg_read()
            if generic:
                monkeypatch.delenv("ICELK_GENERIC_CORNERS")
            if dt > 1.0:
                print("\n%s bs %d generic %s: detection took %.2f s" % (family, bs, generic, dt))
            assert (got is None) == (ref is None)
            if ref is not None:
                assert np.array_equal(_bits(got), _bits(ref)), (maxc, generic)
                assert n == len(ref) and np.array_equal(_bits(seg[:, 0]), _bits(ref.reshape(-1, 2)))


def test_full_frame_c2_on_stretched_content(orc):
    """C2 geometry (4 000 x 3 000, 10 000 corners, 21x21, maxLevel 3) on stretched synth built on the host: detection and
    forward + backward tracking of every corner, bit for bit."""
    from iceberg_tracking_code_amd import Context
    w, h = 4000, 3000
    I, J, flow = xf.stretched(w, h, 1234, k=16, ux=500, uy=-330)
    lk = dict(winSize=(21, 21), maxLevel=3, criteria=CRIT_DEFAULT)
    c = Context(w, h, n_slots=2, max_pts=1 << 15)
    try:
        c.upload_gray(0, I)
        c.upload_gray(1, J)
        ref = orc.good_features(I, 10000, 0.007, 10, None, 10)
        got = c.good_features(0, 10000, 0.007, 10, False, 10)
        assert ref is not None and len(ref) == 10000 and np.array_equal(_bits(got), _bits(ref))
        pts = ref.reshape(-1, 2)
        g = c.track_fb(0, 1, pts, **lk)
        r = orc.track_fb(I, J, pts, **lk)
        _same_fb(g, r, "C2")
        assert r["valid"].mean() > 0.5
    finally:
        c.close()
