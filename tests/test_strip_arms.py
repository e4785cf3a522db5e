"""Every arm of the strip corner kernel on frames just large enough to hold it (tests/strip_arm_frames.py).

CPU first: on each new rounding frame box_sum_frames.running_map -- another legal double summation -- stays within the derived
bound of the exact reference and differs from the term-by-term restatement in at most 1 % of the pixels, so holding the
kernel to both asks nothing a correct summation cannot give (test_box_sums_host.py does the same for its frames).

GPU: the map within the bound of the exact reference and at most 1 % of pixels not the restatement's; corner lists the
restatement's, in order (they run the arm that tests nothing per pixel: no mask, no map), and the maximum that arm publishes
(icelk_detect_max_key) the key of the restatement's maximum; dots on the wave seams, a frame flat in its lower half, an
all-flat frame (maximum +0), stripes (maximum +0 over ordinary radicands) and dots on stripes bit for bit as the generic
kernel (ICELK_GENERIC_CORNERS=1): maps, lists and the published maximum.  Which of these frames reach the square root's band
and which only sqrtf is said in strip_arm_frames.py."""
import numpy as np
import pytest

import box_sum_frames as B
import np_restatement as R
import strip_arm_frames as S
from test_restatement_oracle import same

SELECTIONS = [(0, 0.01, 0), (0, 0.007, 4), (50, 0.01, 4), (0, 1e-4, 0)]


def test_frames_hold_every_arm():
    for bs in B.FUSED:
        c = B.strip_cfg(bs)
        assert 3 * c["TW"] < S.W <= 4 * c["TW"] and 2 * c["SH"] < S.H <= 3 * c["SH"], bs
        # strips 0 .. 2 in x have all their output columns inside the frame, strip 3 is narrower; strip 1 in y rolls
        assert [(k + 1) * c["TW"] <= S.W for k in range(4)] == [True, True, True, False], bs
        xs = [k * c["TW"] - 1 - bs // 2 for k in range(4)]
        ys = [k * c["SH"] - 1 - bs // 2 for k in range(3)]
        assert [y - 1 >= 0 and y + c["NROWS"] <= S.H - 1 for y in ys] == [False, True, False], bs
        assert all(xs[1] + 1 <= x < xs[1] + c["NT"] for x in S.seam_columns(bs)), bs
    c = B.strip_cfg(10)
    assert 247 <= c["TW"] + 2 and 248 > c["TW"] and 40 < c["SH"]


@pytest.mark.parametrize("label,bs", S.CASES)
def test_running_sums_stay_within_the_bound_and_the_share(label, bs):
    r = S.references(label, bs)
    ne = r["running"].view(np.uint32) != r["term"].view(np.uint32)
    ok = ~ne | B.within_bound(r["running"], r["img"], bs, r["exact"], r["bound"])
    assert ok.all(), (label, bs, int((~ok).sum()))
    assert ne.sum() <= 0.01 * ne.size, (label, bs, int(ne.sum()))
    assert B.within_bound(r["term"], r["img"], bs, r["exact"], r["bound"]).all(), (label, bs)


def test_signed_extremes_of_the_bits_give_the_largest_ordered_key():
    """The row phase that tests nothing per pixel keeps, instead of a key per pixel, the largest and the smallest of the
    values' bits as signed integers: the largest if it is >= 0, else the smallest, has the largest ordered_key -- for
    every mix of signs, -0 against +0 included (k_corners.hip, strip_body)."""
    def key(bits):
        bits = np.asarray(bits, np.uint32)
        return np.where(bits & 0x80000000, ~bits, bits | 0x80000000).astype(np.uint32)
    rng = np.random.RandomState(7)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-38, -1e-38, 1.0, -1.0, 3e-19, -3e-19], np.float32)
    for trial in range(4000):
        n = rng.randint(1, 9)
        v = np.where(rng.rand(n) < 0.5, rng.choice(special, n), (rng.randn(n) * 10.0 ** rng.randint(-30, 3)).astype(np.float32))
        if trial % 4 == 0:
            v = -np.abs(v)                                   # nothing above -0
        v = v.astype(np.float32)
        b = v.view(np.int32)
        pick = b.max() if b.max() >= 0 else b.min()
        assert key(np.array([pick], np.int32).view(np.uint32))[0] == key(v.view(np.uint32)).max(), v


def _context(monkeypatch, generic=False):
    from iceberg_tracking_code_amd import Context
    if generic:
        monkeypatch.setenv("ICELK_GENERIC_CORNERS", "1")
    return Context(S.W, S.H, n_slots=1, max_pts=1 << 16)


@pytest.mark.gpu
def test_map_and_lists_on_rounding_frames(monkeypatch):
    c = _context(monkeypatch)
    try:
        for label, bs in S.CASES:
            r = S.references(label, bs)
            c.upload_gray(0, r["img"])
            got = c.min_eig_map(0, bs)
            ne = got.view(np.uint32) != r["term"].view(np.uint32)
            worst = float((np.abs(got.astype(np.float64) - r["exact"].astype(np.float64)) / r["bound"]).max())
            print("strip arms: %-10s bs %2d  %4d of %6d pixels not identical, worst |eig - exact| / bound %.3g"
                  % (label, bs, ne.sum(), ne.size, worst))
            assert B.within_bound(got, r["img"], bs, r["exact"], r["bound"]).all(), (label, bs)
            assert ne.sum() <= 0.01 * ne.size, (label, bs, int(ne.sum()))
            for maxc, q, md in SELECTIONS:
                want = R.good_features(r["img"], maxc, q, md, None, bs)
                got_list = c.good_features(0, maxc, q, md, False, bs)
                # the maximum of the whole map: the strip kernel's differs from the restatement's only where a pixel does,
                # and the largest value of these frames is not among those few (asserted: the two maps agree there)
                assert got.max() == r["term"].max(), (label, bs)
                assert c.detect_max_key() == S.ordered_key(got.max()) == S.ordered_key(r["term"].max()), (label, bs, maxc, q, md)
                assert (got_list is None) == (want is None), (label, bs, maxc, q, md)
                if want is not None:
                    assert same(got_list, want), (label, bs, maxc, q, md)
    finally:
        c.close()


def _exact_frames():
    out = [("flat", bs, S.flat()) for bs in B.FUSED]
    out += [("dots", bs, S.dots(bs)) for bs in B.FUSED]
    out += [("half-flat", bs, S.half_flat(bs)) for bs in B.FUSED]
    out += [("stripes", bs, S.stripes()) for bs in B.FUSED]
    out += [("stripes-dots", bs, S.stripes_dots(bs)) for bs in B.FUSED]
    return out


@pytest.mark.gpu
def test_exact_frames_are_the_generic_kernels_bit_for_bit(monkeypatch):
    """Flat ground has radicand 0 (the wave takes sqrtf), the dots sit on the seams between the waves of a workgroup, the
    stripes have ordinary radicands everywhere and a maximum of +0; every box sum of these frames is exact, so no order of
    addition can show.  The published maximum is read back after the detection that tests nothing per pixel."""
    frames = _exact_frames()
    results = []
    for generic in (False, True):
        c = _context(monkeypatch, generic)
        try:
            res = []
            for what, bs, img in frames:
                c.upload_gray(0, img)
                lists = [c.good_features(0, maxc, q, md, False, bs) for maxc, q, md in SELECTIONS]
                key = c.detect_max_key()
                res.append((c.min_eig_map(0, bs), lists, key, c.detect_max_key()))
            results.append(res)
        finally:
            c.close()
    for (what, bs, img), (m_strip, l_strip, k_strip, km_strip), (m_gen, l_gen, k_gen, km_gen) in zip(frames, *results):
        assert np.array_equal(m_strip.view(np.uint32), m_gen.view(np.uint32)), (what, bs)
        # after the detection and after the map (the arm with per-pixel tests): the generic kernel's, and the key of the map's
        # maximum -- 0x80000000, the key of +0, on the flat frame and on the stripes
        assert k_strip == k_gen == km_strip == km_gen == S.ordered_key(m_gen.max()), (what, bs, hex(k_strip), hex(k_gen))
        if what in ("flat", "stripes"):
            assert k_strip == 0x80000000 and not m_strip.any() and not np.signbit(m_strip).any(), (what, bs)
        for a, b, sel in zip(l_strip, l_gen, SELECTIONS):
            assert (a is None) == (b is None), (what, bs, sel)
            if a is not None:
                assert same(a, b), (what, bs, sel)
        if what in ("flat", "stripes"):
            assert not m_strip.any() and all(a is None for a in l_strip), bs
        else:
            assert all(a is not None and len(a) >= 6 for a in l_strip[:1]), (what, bs)
            want = R.good_features(img, *SELECTIONS[0][:3], None, bs)
            assert same(l_strip[0], want), (what, bs)
