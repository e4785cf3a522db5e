"""The CPU oracle against tests/np_restatement.py, bit for bit (CPU only, runs anywhere).

The GPU tests hold the HIP kernels to oracle/icelk_oracle.c; kernels and oracle come from one reading of SURVEY.md
Appendix A.  Here a third, independent statement of that text (numpy only) is held against the oracle on every stage
of the tracking path -- no tolerance, no point or case left out: the default variant is IEEE float32 around exact
integer sums, so two statements of it agree to the bit or one of them is wrong.  The case lists of this file are also
what tests/test_gpu_restatement.py runs the HIP path over.
"""
import numpy as np

import np_restatement as R
from reference_loops import OracleCv, run_reference_loop

CRIT_DEFAULT = (3, 30, 0.01)
CRIT_REF = (3, 25, 0.03)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------ integer stages
def test_gray_both_variants_all_small_sizes_and_large(orc):
    rng = np.random.RandomState(31)
    sizes = [(h, w) for h in range(1, 6) for w in range(1, 6)] + [(240, 320), (307, 5), (3, 411), (199, 257)]
    for h, w in sizes:
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        for variant in (3, 4):
            assert same(orc.bgr2gray(img, variant), R.bgr2gray(img, variant)), (h, w, variant)
    # the extremes of every channel: the rounding bias and the shift at the ends of the range
    ext = np.array([[[a, b, c] for a in (0, 1, 127, 128, 254, 255) for b in (0, 1, 128, 255) for c in (0, 127, 255)]], np.uint8)
    for variant in (3, 4):
        assert same(orc.bgr2gray(ext, variant), R.bgr2gray(ext, variant))


def pyramid_sizes():
    """(h, w): every shape narrower than the filter, then twenty random ones up to 300 x 300."""
    rng = np.random.RandomState(2027)
    return [(1, 1), (1, 9), (8, 1), (2, 2), (2, 5), (3, 3)] + [(int(rng.randint(1, 301)), int(rng.randint(1, 301)))
                                                               for _ in range(20)]


def test_pyrdown_pyramids_and_scharr_from_one_pixel_up(orc):
    rng = np.random.RandomState(5)
    for k, (h, w) in enumerate(pyramid_sizes()):
        img = rng.randint(0, 256, (h, w)).astype(np.uint8)
        if k % 4 == 3:
            img = (img // 128 * 255).astype(np.uint8)          # black / white only: sums at the ends of the range
        assert same(orc.pyrdown(img), R.pyrdown(img)), (h, w)
        assert same(orc.scharr(img), R.scharr(img)), (h, w)
        a, b = orc.build_pyramid(img, (3, 3), 8), R.build_pyramid(img, (3, 3), 8)
        assert len(a) == len(b), (h, w)
        for l, (x, y) in enumerate(zip(a, b)):
            assert same(x, y), (h, w, l)
            assert same(orc.scharr(x), R.scharr(y)), (h, w, l)
    for v in (0, 255):
        flat = np.full((7, 6), v, np.uint8)
        assert same(orc.pyrdown(flat), R.pyrdown(flat)) and same(orc.scharr(flat), R.scharr(flat))


def test_pyramid_stop_rule(orc):
    pairs = [(640, 480, (21, 21), 3), (640, 480, (35, 35), 10), (640, 480, (35, 35), 2), (4000, 3000, (21, 21), 3),
             (5760, 3840, (31, 31), 5), (40, 40, (21, 21), 3)]                      # test_pyramid_stop_rule_by_hand
    pairs += [(43, 43, (21, 21), 3), (44, 43, (21, 21), 3), (44, 44, (21, 21), 3), (640, 480, (100, 100), 5),
              (640, 480, (400, 400), 3), (97, 61, (7, 7), 5), (1, 1, (3, 3), 4), (300, 7, (3, 5), 8), (640, 480, (21, 21), 0)]
    by_hand = [3, 3, 2, 3, 5, 0]
    for k, (w, h, win, ml) in enumerate(pairs):
        got = R.pyramid_levels(w, h, win, ml)
        assert got == orc.pyramid_levels(w, h, win, ml), (w, h, win, ml)
        if k < len(by_hand):
            assert got == by_hand[k]
    assert [l.shape for l in R.build_pyramid(np.zeros((480, 640), np.uint8), (35, 35), 10)] == \
        [(480, 640), (240, 320), (120, 160), (60, 80)]


def test_reflect101_by_hand():
    assert [R.reflect101(i, 5) for i in range(-6, 11)] == [2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2]
    assert [R.reflect101(i, 2) for i in range(-3, 5)] == [1, 0, 1, 0, 1, 0, 1, 0]
    assert [R.reflect101(i, 1) for i in range(-3, 4)] == [0] * 7


# ------------------------------------------------------------------------------------------ pyramidal LK
def lk_points(rng, n, w, h, win, top):
    """Points inside, on and either side of every border, at the bound of the window test of level 0 and of the top
    level, and far outside."""
    ww, wh = win
    hx, hy = (ww - 1) * 0.5, (wh - 1) * 0.5
    m = 12.0
    out = [np.stack([rng.uniform(-m, w + m, n // 2), rng.uniform(-m, h + m, n // 2)], 1)]
    q = max(n // 8, 2)
    for x0, x1, y0, y1 in ((-m, m, -m, h + m), (w - 1 - m, w - 1 + m, -m, h + m), (-m, w + m, -m, m),
                           (-m, w + m, h - 1 - m, h - 1 + m)):
        out.append(np.stack([rng.uniform(x0, x1, q), rng.uniform(y0, y1, q)], 1))
    exact = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w / 2, 0), (0, h / 2), (w - 1, h / 2), (w / 2, h - 1),
             (w, h), (-1, -1), (w - 0.5, h - 0.5), (-0.5, -0.5)]
    for level in {0, top}:
        s = float(1 << level)
        cols, rows = w, h
        for _ in range(level):
            cols, rows = (cols + 1) // 2, (rows + 1) // 2
        for d in (-0.5, 0.0, 0.5):
            exact += [((hx - ww + d) * s, h / 2), (w / 2, (hy - wh + d) * s), ((cols + hx + d) * s, h / 2),
                      (w / 2, (rows + hy + d) * s)]
    out.append(np.array(exact))
    far = max(n // 8, 2)
    sx, sy = (ww + 2) * (1 << top), (wh + 2) * (1 << top)
    out.append(np.stack([rng.uniform(-sx, w + sx, far), rng.uniform(-sy, h + sy, far)], 1))
    return np.concatenate(out).astype(np.float32)


def period4_pair():
    """A 4 x 4 tile repeated: central differences see it at level 0, level 1 has period 2 (every Scharr derivative
    exactly 0), level 2 is flat -- minEig rejects at every coarse level and only there."""
    tile = np.random.RandomState(44).randint(0, 256, (4, 4)).astype(np.uint8)
    a = np.tile(tile, (20, 24))
    return a, np.roll(a, 1, axis=1)


def flat_with_a_square():
    img = np.full((160, 200), 77, np.uint8)
    img[40:80, 50:120] = 200
    return img


def lk_cases(synth):
    """The LK matrix: dicts of img0, img1, pts, guess, win, maxLevel, crit, flags, thr, tag."""
    rng = np.random.RandomState(20261016)
    cases = []

    def add(tag, img0, img1, win, ml, crit, n=80, flags=0, thr=1e-4, pts=None, guess=None):
        h, w = img0.shape
        top = R.pyramid_levels(w, h, win, ml)
        if pts is None:
            pts = lk_points(rng, n, w, h, win, top)
        if flags & 4 and guess is None:
            guess = pts + rng.uniform(-2, 2, pts.shape).astype(np.float32)
            guess[::7] = pts[::7] + np.float32([3.0 * w, -2.0 * h])       # a guess whose window is outside at every level
        cases.append(dict(tag=tag, img0=img0, img1=img1, pts=pts, guess=guess, win=win, maxLevel=ml, crit=crit,
                          flags=flags, thr=thr))

    big = synth.frame(640, 480, 0, 0, 1234), synth.frame(640, 480, 410, -333, 1234)
    for win, ml, crit in (((15, 15), 2, CRIT_REF), ((21, 21), 3, CRIT_DEFAULT), ((31, 31), 5, CRIT_DEFAULT),
                          ((35, 35), 4, CRIT_REF)):
        add("tuned %dx%d" % win, big[0], big[1], win, ml, crit, n=160)
    mid = synth.frame(320, 240, 0, 0, 5), synth.frame(320, 240, 300, -170, 5)
    small = synth.frame(200, 150, 0, 0, 3), synth.frame(200, 150, 400, 100, 3)
    odd = synth.frame(131, 77, 0, 0, 8), synth.frame(131, 77, -260, 190, 8)
    tiny = synth.frame(64, 48, 0, 0, 2), synth.frame(64, 48, 180, 90, 2)
    add("5x7", small[0], small[1], (5, 7), 2, CRIT_DEFAULT)
    add("9x13", odd[0], odd[1], (9, 13), 1, CRIT_DEFAULT)
    add("20x20", mid[0], mid[1], (20, 20), 4, CRIT_REF)
    add("41x41", mid[0], mid[1], (41, 41), 2, CRIT_REF, n=40)
    add("level 0 only", tiny[0], tiny[1], (21, 21), 0, CRIT_DEFAULT)
    add("maxLevel 5, stops at 3", synth.frame(97, 61, 0, 0, 6), synth.frame(97, 61, 150, -120, 6), (7, 7), 5, CRIT_DEFAULT)
    add("large step at level 0", mid[0], synth.frame(320, 240, 256 * 6, -256 * 5, 5), (21, 21), 0, CRIT_DEFAULT)
    # frames smaller than the window: the reflected border is wider than the frame
    for (w, h), win in (((24, 24), (31, 31)), ((13, 9), (21, 21)), ((20, 30), (35, 15))):
        add("frame %dx%d under window" % (w, h), synth.frame(w, h, 0, 0, 9), synth.frame(w, h, 200, -150, 9), win, 3,
            CRIT_DEFAULT, n=32)
    # every criteria type; counts 0, 1, small, 100+ (clamped); eps 0, 0.03, 10+ (clamped)
    for crit in ((1, 0, 0.0), (1, 1, 0.0), (3, 1, 0.0), (3, 3, 0.0), (2, 5, 0.03), (3, 150, 1e-9), (3, 30, 25.0),
                 (3, 30, 0.0), (0, 5, 5.0), (1, 7, 0), (3, 0, 0.03), (2, 0, 11.0)):
        add("criteria %r" % (crit,), small[0], small[1], (15, 15), 2, crit, n=32)
    for flags in (4, 8, 12):
        add("flags %d" % flags, mid[0], mid[1], (21, 21), 3, CRIT_DEFAULT, n=48, flags=flags)
        add("flags %d, threshold 0" % flags, small[0], small[1], (9, 13), 2, CRIT_REF, n=32, flags=flags, thr=0.0)
    # texture-less windows: minEig exactly 0, D exactly 0; an edge: one eigenvalue 0
    sq = flat_with_a_square()
    sq_pts = np.float32([[10, 10], [150, 140], [50, 40], [119, 79], [85, 60], [85, 40], [50, 60], [120, 60], [85, 79.5],
                         [30.25, 20.5], [185.5, 150.25], [-100, -100], [500, 500]])
    for thr in (1e-4, 0.0):
        for flags in (0, 8):
            add("flat and square, threshold %g, flags %d" % (thr, flags), sq, np.roll(sq, 1, axis=0), (21, 21), 2,
                CRIT_DEFAULT, flags=flags, thr=thr, pts=sq_pts)
    add("textured, threshold 0", mid[0], mid[1], (15, 15), 3, CRIT_REF, n=40, thr=0.0)
    # weight products that land exactly on k + 0.5: a = 0.5, b an odd multiple of 2^-14 (and the other way round)
    halves = []
    for k in (1, 3, 5, 7, 4095, 8191, 8193, 16381, 16383):
        halves += [(60.5, 50 + k / 16384.0), (70 + k / 16384.0, 40.5), (80.5 + 0.0, 30.5 + k / 16384.0 / 2)]
    halves = np.float32(halves)
    add("exact halves, level 0 only", small[0], small[1], (21, 21), 0, CRIT_DEFAULT, pts=halves)
    add("exact halves, three levels", small[0], small[1], (15, 15), 2, CRIT_REF, pts=halves)
    # an epsilon that a step meets with equality: steps of a run with eps = 0 whose squared length s has a double e
    # with e * e == s; `<=` stops there, `<` would go on
    pts = lk_points(rng, 60, 200, 150, (15, 15), 0)
    trace = []
    R.pyrlk(small[0], small[1], pts, None, (15, 15), 0, (3, 30, 0.0), trace=trace)
    ties = sorted({float(np.sqrt(t)) for _, _, t in trace if isinstance(t, float) and 1e-6 < t < 1.0
                   and float(np.sqrt(t)) * float(np.sqrt(t)) == t})
    assert len(ties) >= 3
    for e in (ties[0], ties[len(ties) // 2], ties[-1]):
        add("epsilon %r met with equality" % e, small[0], small[1], (15, 15), 0, (3, 30, e), pts=pts)
    p4 = period4_pair()
    add("period 4: minEig rejects at coarse levels only", p4[0], p4[1], (9, 9), 2, CRIT_DEFAULT, n=40)
    return cases


LK_REQUIRED = {
    "outside@coarse",          # template window outside at a coarse level: the point carries on
    "outside@0",               # ... at level 0, before anything is iterated
    "outside_first@0",         # search window outside at level 0 before the first iteration (from an initial guess)
    "outside_iter@0",          # ... during the iterations
    "mineig@coarse only",      # rejected at a coarse level, tracked at level 0: the propagated guess survived
    "mineig@0",
    "det@0",                   # D < FLT_EPSILON with the minEig test passed (minEigThreshold = 0)
    "eps@0", "oscillation@0", "count@0", "zero_iter@0",
    "eps_tie@0",               # a step of non-zero length whose squared length EQUALS eps^2: `<=`, not `<`
    "half_weight@0",           # a weight that was an exact half before rounding
}


def lk_seen(trace, status):
    """The branch names of LK_REQUIRED that a trace of R.pyrlk (and the status it returned) shows."""
    seen = set()
    st = np.asarray(status).ravel()
    for i, level, tag in trace:
        if not isinstance(tag, str):          # the squared length of a step
            continue
        seen.add("%s@%s" % (tag, "coarse" if level > 0 else "0"))
        if tag == "mineig" and level > 0 and st[i]:
            seen.add("mineig@coarse only")
    return seen


def run_lk_case(c, fn, trace=None):
    kw = {} if trace is None else dict(trace=trace)
    return fn(c["img0"], c["img1"], c["pts"], c["guess"], c["win"], c["maxLevel"], c["crit"], c["flags"], c["thr"], **kw)


def test_pyrlk_matrix_bit_for_bit_and_every_branch_reached(orc, synth):
    """Every case of lk_cases: nextPts, status and err of the oracle equal the restatement's, all points, all bits.
    The restatement's trace then has to show every exit of A.6 (LK_REQUIRED) -- a matrix that never leaves a level
    through one of them would prove nothing about it."""
    seen = set()
    npts = 0
    for c in lk_cases(synth):
        trace = []
        want = run_lk_case(c, R.pyrlk, trace)
        got = run_lk_case(c, orc.pyrlk)
        for name, g, r in zip(("nextPts", "status", "err"), got, want):
            assert same(g, r), (c["tag"], name, np.nonzero((bits(g) != bits(r)).reshape(len(c["pts"]), -1).any(1))[0][:10])
        seen |= lk_seen(trace, want[1])
        npts += len(c["pts"])
    assert LK_REQUIRED <= seen, sorted(LK_REQUIRED - seen)
    assert npts > 3000


def test_round_half_even_decides_a_weight():
    """The constructed halves really are ties, to both sides: cvRound takes 8190.5 down and 0.5 down to 0, 8189.5 up."""
    w = R._weights(np.float32(0.5), np.float32(3 / 16384.0))
    assert w[4] and w[:4] == (8190, 8190, 2, 2)          # 8190.5, 8190.5, 1.5 -> 8190, 8190, 2; the remainder
    w = R._weights(np.float32(0.5), np.float32(1 / 16384.0))
    assert w[4] and w[:4] == (8192, 8192, 0, 0)          # 8191.5, 8191.5, 0.5
    w = R._weights(np.float32(5 / 16384.0), np.float32(0.5))
    assert w[4] and w[:4] == (8190, 2, 8190, 2)          # 8189.5 -> 8190, 2.5 -> 2


def fb_cases(orc, synth):
    out = []
    for (w, h, ux, uy, seed), win, ml, crit, maxc in (((320, 240, 300, -170, 5), (21, 21), 3, CRIT_DEFAULT, 120),
                                                     ((320, 240, 600, 420, 7), (35, 35), 4, CRIT_REF, 80),
                                                     ((200, 150, -330, 90, 3), (9, 13), 2, (1, 7, 0), 100)):
        a, b = synth.frame(w, h, 0, 0, seed), synth.frame(w, h, ux, uy, seed)
        pts = R.good_features(a, maxc, 0.01, 7, None, 5).reshape(-1, 2)
        out.append((a, b, pts, win, ml, crit))
    return out


FB_FLOAT = ("p1", "p0r", "err_fwd", "err_bwd", "dist")
FB_INT = ("st_fwd", "st_bwd", "valid")


def test_track_fb_on_detected_corners(orc, synth):
    for a, b, pts, win, ml, crit in fb_cases(orc, synth):
        assert same(pts.reshape(-1, 1, 2), orc.good_features(a, len(pts), 0.01, 7, None, 5))
        r = R.track_fb(a, b, pts, win, ml, crit)
        g = orc.track_fb(a, b, pts, win, ml, crit)
        for k in FB_FLOAT + FB_INT:
            assert same(g[k], r[k]), (win, k)
        assert r["valid"].mean() > 0.8


# ------------------------------------------------------------------------------------------ corners
def ties_frame():
    """test_corner_ties_and_plateaus: a periodic frame, every corner has the same response."""
    yy, xx = np.mgrid[0:240, 0:320]
    return (((xx // 8) + (yy // 8)) % 2 * 200 + 20).astype(np.uint8)


def ramp_frame():
    return (np.add.outer(np.arange(200), 2 * np.arange(300)) % 256).astype(np.uint8)


def eig_frames(synth):
    rng = np.random.RandomState(12)
    flat = synth.frame(131, 77, 5, 9, 31)
    flat[20:60, 30:100] = 93                                  # exact zeros inside
    out = [synth.frame(320, 240, 17, 4242, 7), flat, ties_frame()[:96, :128].copy(), ramp_frame()[:64, :80].copy()]
    out += [rng.randint(0, 256, s).astype(np.uint8) for s in ((9, 13), (64, 3), (3, 3), (1, 70), (2, 5), (3, 4))]
    out.append(np.full((20, 30), 255, np.uint8))
    return out


BLOCK_SIZES = (2, 3, 5, 7, 10)


def test_min_eig_map_bit_for_bit(orc, synth):
    for img in eig_frames(synth):
        for bs in BLOCK_SIZES:
            assert same(orc.min_eig_map(img, bs), R.min_eig_map(img, bs)), (img.shape, bs)


def corner_cases(synth):
    """(tag, img, mask, maxCorners, qualityLevel, minDistance, blockSize)."""
    rng = np.random.RandomState(99)
    cases = []
    tex = synth.frame(320, 240, 0, 0, 4321)
    for bs in BLOCK_SIZES:
        for md in (0, 0.5, 1, 2.5, 3.5, 10, 25):
            cases.append(("textured", tex, None, 0 if md != 10 else 150, 0.01, md, bs))
    mask = np.zeros_like(tex)
    mask[40:200, 60:300] = 255
    mask[100:130, 150:200] = 0
    rmask = (rng.randint(0, 4, tex.shape) > 0).astype(np.uint8) * 255
    for m, bs, md in ((mask, 10, 10), (mask, 3, 2.5), (rmask, 5, 3.5), (rmask, 7, 0), (np.zeros_like(tex), 3, 5)):
        cases.append(("masked", tex, m, 0, 0.007, md, bs))
    flat = tex.copy()
    flat[60:180, 80:260] = 93
    cases.append(("flat patch", flat, None, 0, 0.01, 4, 3))
    cases.append(("flat patch", flat, None, 0, 0.01, 10, 10))
    cases.append(("constant frame", np.full((50, 60), 7, np.uint8), None, 10, 0.01, 5, 3))
    ties = ties_frame()
    for md in (0, 1, 4, 10):
        cases.append(("ties", ties, None, 0, 0.05, md, 3))
    for maxc in (1, 7, 64, 65, 500):                          # the cut falls inside the run of equal responses
        cases.append(("ties cut", ties, None, maxc, 0.05, 4, 3))
    cases.append(("ties cut, no distance", ties, None, 33, 0.05, 0, 5))
    ramp = ramp_frame()
    for md, bs in ((0, 3), (1, 5), (3.5, 10), (25, 7)):
        cases.append(("ramp with plateaus", ramp, None, 0, 0.05, md, bs))
    for k, shape in enumerate(((3, 3), (4, 7), (9, 13), (64, 3), (3, 64), (3, 4), (58, 59), (31, 100))):
        img = rng.randint(0, 256, shape).astype(np.uint8)
        cases.append(("noise %dx%d" % shape, img, None, 0, 0.01, (1, 2.5, 10)[k % 3], BLOCK_SIZES[k % 5]))
        cases.append(("noise %dx%d" % shape, img, None, 5, 0.3, 0, BLOCK_SIZES[(k + 2) % 5]))
    return cases


CORNER_REQUIRED = {"tie", "reject_adjacent_cell", "reject_own_cell", "border_refused", "maxcorners_stop"}


def test_good_features_lists_equal_in_order_and_every_rule_reached(orc, synth):
    """The oracle's corner list against the restatement's -- same corners, same order, None where there is none -- over
    corner_cases, and the restatement's trace shows a tie decided by address, a candidate refused by a neighbour found in
    an adjacent cell (and one in its own), a local maximum on the 1-px frame border refused, and a maxCorners stop."""
    seen = set()
    for tag, img, mask, maxc, q, md, bs in corner_cases(synth):
        trace = []
        want = R.good_features(img, maxc, q, md, mask, bs, trace=trace)
        got = orc.good_features(img, maxc, q, md, mask, bs)
        what = (tag, img.shape, maxc, q, md, bs)
        assert (got is None) == (want is None), what
        if want is not None:
            assert same(got, want), what
        seen |= set(trace)
        if tag.startswith("ties") and md >= 1 and want is not None and maxc == 0:
            assert "tie" in trace and len(want) > 100
    assert CORNER_REQUIRED <= seen, sorted(CORNER_REQUIRED - seen)
    # frames without an interior: no corner, whatever the response
    rng = np.random.RandomState(3)
    for shape in ((1, 70), (2, 5), (70, 2), (1, 1)):
        img = rng.randint(0, 256, shape).astype(np.uint8)
        assert R.good_features(img, 0, 0.01, 1, None, 3) is None and orc.good_features(img, 0, 0.01, 1, None, 3) is None


def test_dilating_the_raw_map_instead_of_the_thresholded_one_cannot_show(synth):
    """A.7 dilates the map AFTER threshold(TOZERO).  Taking the 3 x 3 maximum over the raw map instead is not an error
    an input can expose, so no case of corner_cases is aimed at it: a candidate v passed v > thresh >= 0, every
    neighbour the threshold zeroed was <= thresh < v, so both maxima equal v or exceed it together.  Shown here on the
    maps of the corner cases rather than only claimed."""
    for tag, img, mask, maxc, q, md, bs in corner_cases(synth):
        eig = R.min_eig_map(img, bs)
        ok = np.ones(eig.shape, bool) if mask is None else mask != 0
        thresh = np.float32((float(eig[ok].max()) if ok.any() else 0.0) * q)
        assert thresh >= 0
        t = np.where(eig > thresh, eig, np.float32(0))
        h, w = eig.shape

        def dilate(m):
            big = np.full((h + 2, w + 2), -np.inf, np.float32)
            big[1:-1, 1:-1] = m
            return np.max([big[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0)

        assert np.array_equal((t != 0) & (t == dilate(t)), (t != 0) & (t == dilate(eig))), (tag, img.shape, bs)


def test_tie_break_is_by_higher_address():
    """Four equal corners of a symmetric frame, no minimum distance: the order is from the last raster address down."""
    p = R.good_features(ties_frame(), 0, 0.05, 0, None, 3).reshape(-1, 2)
    addr = p[:, 1].astype(np.int64) * 320 + p[:, 0].astype(np.int64)
    eig = R.min_eig_map(ties_frame(), 3)[p[:, 1].astype(int), p[:, 0].astype(int)]
    runs = np.nonzero(np.diff(eig) == 0)[0]
    assert len(runs) > 100 and np.all(np.diff(addr)[runs] < 0)


# ------------------------------------------------------------------------------------------ the s1 loop
def loop_cases(synth):
    frames, _ = synth.sequence(160, 120, 7, seed=77, max_step_px=2.5)
    mask = np.zeros((120, 160), np.uint8)
    mask[8:112, 10:150] = 255
    fp = dict(maxCorners=60, qualityLevel=0.01, minDistance=7, blockSize=5)
    lk = dict(winSize=(21, 21), maxLevel=2, criteria=CRIT_REF)
    return frames, mask, fp, lk


def same_segments(got, ref):
    assert len(got) == len(ref) and len(ref) >= 2
    for (gf, gt, gq), (rf, rt, rq) in zip(got, ref):
        assert gf == rf and len(gt) == len(rt) > 20
        assert same(np.asarray(gt, np.float32), np.asarray(rt, np.float32))
        assert same(np.asarray(gq, np.float32), np.asarray(rq, np.float32))


def test_reference_loop_on_oracle_equals_loop_on_restatement(orc, synth):
    frames, mask, fp, lk = loop_cases(synth)
    for track_len in (1, 3):
        ref = run_reference_loop(frames, track_len, fp, lk, mask=mask, cv=R.RestatementCv)
        got = run_reference_loop(frames, track_len, fp, lk, mask=mask, cv=OracleCv(orc))
        same_segments(got, ref)
