"""The Harris detector on the frames the smaller-eigenvalue response is already tested on: box sums that round, every arm of
the strip kernel, ties and plateaus, binary content, and a mask that keeps nothing but a constant band (both detectors).

tests/test_gpu_harris.py holds k_harris_strip<3|5|7|10> and the Harris argument of k_min_eig on blob frames alone: fine-noise
ground, no two equal responses, one small ramp with a negative maximum.  Here:

  a  box_sum_frames.FRAMES + RESIDUE_FRAMES      the strip kernel's map is the restatement's or within harris_box_sums.harris_bound
                                                 of the exact reference; the any-blockSize kernel's is the restatement's
  b  strip_arm_frames                            FRESH, rolling and the row phase that tests nothing per pixel; a negative masked
                                                 maximum published by that phase
  c  ties_frame, ramp_frame, 0/255 families      thousands of equal responses: the order among equals is by address
  d  RESIDUE_FRAMES under a mask of the band     the restatement lists nothing: the term-by-term map is exactly 0 there

Every test first asserts on the restatement the property it aims at, so it cannot pass vacuously.  Lists are compared bit
for bit, order included, through good_features (the host's tail) and through seg_detect + seg_read (k_tail.hip), on the strip
kernel and on the any-blockSize kernel (ICELK_GENERIC_CORNERS=1, read at every call).  The references and the bound are held
on the CPU alone in tests/test_harris_box_sums_host.py.
"""
import contextlib

import numpy as np
import pytest

import box_sum_frames as B
import extreme_frames as xf
import harris_box_sums as HB
import harris_restatement as H
import np_restatement as R
import strip_arm_frames as S
from test_gpu_box_sums import SELECTIONS
from test_restatement_oracle import ramp_frame, same, ties_frame

pytestmark = pytest.mark.gpu

GENERIC = "ICELK_GENERIC_CORNERS"
SWITCHES = (None, GENERIC)
KS = HB.KS
ALL = B.FRAMES + B.RESIDUE_FRAMES
BLOCK_SIZES = B.FUSED + (4,)


@pytest.fixture(scope="module")
def ectx():
    """a context of this file's own: one slot, as tests/test_gpu_box_sums.py opens it, wide enough for the arm frames"""
    from iceberg_tracking_code_amd import Context
    c = Context(S.W, 240, n_slots=1, max_pts=1 << 16)
    yield c
    c.close()


@contextlib.contextmanager
def kernel(monkeypatch, switch):
    if switch:
        monkeypatch.setenv(switch, "1")
    try:
        yield
    finally:
        if switch:
            monkeypatch.delenv(switch)


def differ(a, b):
    return a.view(np.uint32) != b.view(np.uint32)


def response_map(c, bs, k):
    return c.min_eig_map(0, bs) if k is None else c.harris_map(0, bs, k)


def detect(c, sel, use_mask, bs, k):
    """one selection through both tails -> (list of good_features, its candidate count, its published key, list of seg_detect)"""
    maxc, q, md = sel
    kw = dict(useHarrisDetector=k is not None, k=0.04 if k is None else k)
    got = c.good_features(0, maxc, q, md, use_mask, bs, **kw)
    cand, key = c.detect_stats()["candidates"], c.detect_max_key()
    n = c.seg_detect(0, maxc, q, md, use_mask, bs, **kw)
    seg = None
    if n:
        seg = np.ascontiguousarray(c.seg_read()[0][:, 0, :]).reshape(-1, 1, 2)
        assert len(seg) == n
    return got, cand, key, seg


def lists_are(c, monkeypatch, want, sel, use_mask, bs, k, what, no_candidates=False, switches=SWITCHES):
    """both kernels, both tails: `want` bit for bit and in order, or nothing where it is None; -> the published keys.
    no_candidates: the masked maximum is <= 0, so the candidate stage itself must have listed nothing"""
    keys = []
    for switch in switches:
        with kernel(monkeypatch, switch):
            got, cand, key, seg = detect(c, sel, use_mask, bs, k)
        for name, lst in (("good_features", got), ("seg_detect", seg)):
            assert (lst is None) == (want is None), (what, switch, name, sel, None if lst is None else len(lst))
            if want is not None:
                assert same(lst, want), (what, switch, name, sel, len(lst), len(want))
        if no_candidates:
            assert want is None and cand == 0, (what, switch, sel, cand)
        keys.append(key)
    return keys


def held_to_the_bound(got, m, residue, what):
    """(a)'s conditions on the strip kernel's map; m: harris_box_sums' references at one k; -> (not identical, worst ratio)"""
    ne = differ(got, m["term"])
    worst = float((np.abs(got.astype(np.float64) - m["exact"].astype(np.float64)) / m["bound"]).max())
    ok = ~ne | HB.within_bound(got, m["exact"], m["bound"])
    assert ok.all(), (what, int((~ok).sum()), worst)
    if residue:
        assert np.all(m["term"][ne] == 0) and np.all(got[ne] <= 0), (what, int(ne.sum()), float(got[ne].max()))
    else:
        assert ne.sum() <= 0.01 * ne.size, (what, int(ne.sum()))
    return int(ne.sum()), worst


# ---------------------------------------------------------------------------------------------- a. rounding box sums
_lists = {}


def expected_lists(key, resp):
    """H.select over SELECTIONS on one restatement map, computed once per session"""
    if key not in _lists:
        _lists[key] = [H.select(resp, maxc, q, md) for maxc, q, md in SELECTIONS]
    return _lists[key]


@pytest.mark.parametrize("switch", SWITCHES, ids=["strip", "generic"])
def test_harris_map_on_rounding_box_sums(ectx, monkeypatch, switch):
    lines = both_signs = 0
    for entry in ALL:
        r = HB.references(entry)
        ectx.upload_gray(0, r["img"])
        for k in KS:
            m, what = r[k], (B.tag(entry), k, switch)
            assert (m["term"] > 0).mean() > 0.2, what
            both_signs += bool((m["term"] < 0).mean() > 0.01)
            with kernel(monkeypatch, switch):
                got = ectx.harris_map(0, r["bs"], k)
            ne = differ(got, m["term"])
            worst = float((np.abs(got.astype(np.float64) - m["exact"].astype(np.float64)) / m["bound"]).max())
            print("harris box sums: %-28s k %.2f %-8s %4d of %5d pixels not identical, worst |R - exact| / bound %.3g"
                  % (B.tag(entry), k, "generic" if switch else "strip", ne.sum(), ne.size, worst))
            lines += 1
            if switch:
                assert not ne.any(), (what, int(ne.sum()))
            else:
                held_to_the_bound(got, m, entry in B.RESIDUE_FRAMES, what)
    assert lines == len(ALL) * len(KS) and both_signs >= lines // 2, both_signs          # the cancelling form has both signs


@pytest.mark.parametrize("k", KS)
def test_harris_corner_lists_on_rounding_box_sums(ectx, monkeypatch, k):
    nonempty = 0
    for entry in ALL:
        r = HB.references(entry)
        ectx.upload_gray(0, r["img"])
        for sel, want in zip(SELECTIONS, expected_lists((B.tag(entry), k), r[k]["term"])):
            lists_are(ectx, monkeypatch, want, sel, False, r["bs"], k, (B.tag(entry), k))
            nonempty += want is not None and len(want) >= 5
    assert nonempty == len(ALL) * len(SELECTIONS)


# ---------------------------------------------------------------------------------------------- b. every arm
WIDE_FLOOR = {3: 2180, 5: 1671, 7: 1395, 10: 1084}       # wide-pm1 at k 0.04, qualityLevel 0.01, minDistance 0


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("label,bs", S.CASES, ids=["%s-bs%d" % c for c in S.CASES])
def test_arm_rounding_frames(ectx, monkeypatch, label, bs, k):
    r = HB.arm_references(label, bs)
    m, what = r[k], (label, bs, k)
    assert (m["term"] > 0).mean() > 0.5, what
    ectx.upload_gray(0, r["img"])
    with kernel(monkeypatch, GENERIC):
        assert same(ectx.harris_map(0, bs, k), m["term"]), what
    got = ectx.harris_map(0, bs, k)
    n, worst = held_to_the_bound(got, m, False, what)
    print("harris strip arms: %-10s bs %2d k %.2f  %4d of %6d pixels not identical, worst |R - exact| / bound %.3g"
          % (label, bs, k, n, got.size, worst))
    want_key = S.ordered_key(m["term"].max())
    for sel, want in zip(SELECTIONS, expected_lists(("arm", label, bs, k), m["term"])):
        if label == "wide-pm1" and k == 0.04 and sel == (0, 0.01, 0):
            assert len(want) >= WIDE_FLOOR[bs], (what, len(want))
        # no mask, no map: the strips inside the frame run the row phase that tests nothing per pixel
        keys = lists_are(ectx, monkeypatch, want, sel, False, bs, k, what)
        assert keys == [want_key, want_key], (what, sel, [hex(v) for v in keys], hex(want_key))


EXACT = [(name, bs) for name in ("flat", "dots", "half-flat", "stripes", "stripes-dots") for bs in B.FUSED]
EXACT_SELECTIONS = [(0, 0.01, 0), (0, 0.007, 4), (50, 0.01, 4)]
# restatement, k 0.04, qualityLevel 0.01, minDistance 0: (corners, tied pairs)
EXACT_FLOOR = {("dots", 10): (678, 666), ("dots", 3): (12, 5), ("stripes-dots", 3): (25, 7)}


def exact_frame(name, bs):
    return {"flat": lambda: S.flat(), "dots": lambda: S.dots(bs), "half-flat": lambda: S.half_flat(bs),
            "stripes": lambda: S.stripes(), "stripes-dots": lambda: S.stripes_dots(bs)}[name]()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name,bs", EXACT, ids=["%s-bs%d" % c for c in EXACT])
def test_arm_exact_frames_bit_for_bit(ectx, monkeypatch, name, bs, k):
    """Every box sum of these frames is exact, so no order of addition can show: map, lists and the published maximum are
    the restatement's on both kernels.  The stripes have dy = 0 everywhere: det = 0 and R = -kf t t < 0 in every pixel, so the
    strips inside the frame publish a NEGATIVE maximum from the row phase that keeps signed extremes in place of keys."""
    img = exact_frame(name, bs)
    term, what = H.harris_map(img, bs, k), (name, bs, k)
    negative = name == "stripes" or (name, bs) == ("stripes-dots", 10)
    if negative:
        assert term.max() < 0, what
    if name == "flat":
        assert not term.any() and not np.signbit(term).any()
    if (name, bs) in EXACT_FLOOR and k == 0.04:
        corners, tied = EXACT_FLOOR[(name, bs)]
        assert len(H.select(term, 0, 0.01, 0)) >= corners and H.ties(term, 0.01) >= tied, what
    ectx.upload_gray(0, img)
    maps = []
    for switch in SWITCHES:
        with kernel(monkeypatch, switch):
            maps.append(ectx.harris_map(0, bs, k))
        assert same(maps[-1], term), (what, switch, int(differ(maps[-1], term).sum()))
    want_key = S.ordered_key(term.max())
    for sel in EXACT_SELECTIONS:
        want = H.select(term, *sel)
        keys = lists_are(ectx, monkeypatch, want, sel, False, bs, k, what, no_candidates=bool(term.max() <= 0))
        assert keys == [want_key, want_key], (what, sel, [hex(v) for v in keys], hex(want_key))
        if negative:
            assert want is None and want_key < 0x80000000, what
    if name == "flat":
        assert want_key == 0x80000000 and not any(np.signbit(v).any() for v in maps), what


# ---------------------------------------------------------------------------------------------- c. ties, plateaus, 0/255
TIE_FRAMES = ("ties", "ramp", "blocks2", "blocks3", "mondrian", "stripes")
CUTS = (1, 7, 64, 65, 500)          # corner_cases' "ties cut": maxCorners inside a run of equal responses, at (0.05, 4)
# restatement, k 0.04: (frame, blockSize) -> (selection, corners at least, tied pairs at qualityLevel of the selection at least)
TIE_FLOOR = {("ties", 3): ((0, 0.05, 4), 1131, 4523), ("ties", 5): ((0, 0.05, 4), 2262, 18095),
             ("ramp", 3): ((0, 0.05, 4), 3, 2), ("ramp", 5): ((0, 0.05, 4), 5, 3),
             ("blocks2", 3): ((0, 0.01, 5), 1713, 5922), ("blocks2", 10): ((0, 0.01, 5), 1383, 452),
             ("blocks3", 3): ((0, 0.01, 5), 1658, 1), ("blocks3", 10): ((0, 0.01, 5), 1558, 1),
             ("stripes", 3): ((0, 0.01, 5), 216, 1), ("stripes", 10): ((0, 0.01, 5), 17, 1),
             ("mondrian", 5): ((0, 0.01, 5), 1309, 1)}
_tie_frames = {}


def tie_frame(name):
    if name not in _tie_frames:
        img = ties_frame() if name == "ties" else ramp_frame() if name == "ramp" else xf.FAMILIES[name](320, 240, 2)[0]
        img = np.ascontiguousarray(img)
        img.setflags(write=False)
        _tie_frames[name] = img
    return _tie_frames[name]


def block_mask(h, w, seed):
    rng = np.random.RandomState(seed)
    return np.kron(rng.randint(0, 4, ((h + 7) // 8, (w + 7) // 8)) > 0, np.ones((8, 8)))[:h, :w].astype(np.uint8) * 255


def test_strip_geometry_of_the_tie_frames():
    """at every fused blockSize one strip lies wholly inside each frame and takes the fast row phase, and a narrower one lies
    beside it (csrc/k_corners.hip StripCfg, restated in box_sum_frames.strip_cfg)"""
    for name in TIE_FRAMES:
        h, w = tie_frame(name).shape
        assert (h, w) in ((240, 320), (200, 300))
        for bs in B.FUSED:
            c, an = B.strip_cfg(bs), bs // 2
            nx, ny = (w + c["TW"] - 1) // c["TW"], (h + c["SH"] - 1) // c["SH"]
            inside = [(bx, by) for bx in range(nx) for by in range(ny)
                      if (bx + 1) * c["TW"] <= w and by * c["SH"] - 1 - an - 1 >= 0 and by * c["SH"] - 1 - an + c["NROWS"] <= h - 1]
            assert len(inside) >= 1 and nx == 2 and w % c["TW"] and all(bx == 0 for bx, _ in inside), (name, bs)


def test_a_maxcorners_cut_is_a_prefix_of_the_uncut_list():
    """what lets test_ties_plateaus_and_binary_content take the cuts from one selection: H.select stops at maxCorners"""
    resp = H.harris_map(tie_frame("ties"), 3, 0.04)
    whole = H.select(resp, 0, 0.05, 4)
    for maxc in CUTS:
        assert same(H.select(resp, maxc, 0.05, 4), whole[:maxc])


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("bs", BLOCK_SIZES)
@pytest.mark.parametrize("name", TIE_FRAMES)
def test_ties_plateaus_and_binary_content(ectx, monkeypatch, name, bs, k):
    img = tie_frame(name)
    resp, what = H.harris_map(img, bs, k), (name, bs, k)
    if k == 0.04:
        assert H.ties(resp, 0.01) > 0, what
    if (name, bs) in TIE_FLOOR and k == 0.04:
        sel, corners, tied = TIE_FLOOR[(name, bs)]
        assert len(H.select(resp, *sel)) >= corners and H.ties(resp, sel[1]) >= tied, what
    ectx.upload_gray(0, img)
    for switch in SWITCHES:
        with kernel(monkeypatch, switch):
            assert same(ectx.harris_map(0, bs, k), resp), (what, switch)       # the sums of these frames are exact
    whole = H.select(resp, 0, 0.05, 4)
    lists_are(ectx, monkeypatch, whole, (0, 0.05, 4), False, bs, k, what)
    for maxc in CUTS:
        lists_are(ectx, monkeypatch, None if whole is None else whole[:maxc], (maxc, 0.05, 4), False, bs, k, what)
    for sel in ((0, 0.01, 0), (0, 0.01, 5)):
        lists_are(ectx, monkeypatch, H.select(resp, *sel), sel, False, bs, k, what)
    mask = block_mask(*img.shape, seed=bs)
    ectx.set_mask(mask)
    lists_are(ectx, monkeypatch, H.select(resp, 0, 0.05, 4, mask), (0, 0.05, 4), True, bs, k, what)


# ---------------------------------------------------------------------------------------------- d. mask of a constant band
BAND_SELECTIONS = [(0, q, md) for q in (0.01, 0.007) for md in (0, 4)]


def restated(img, term, sel, mask, bs, k):
    """the restatement's list: np_restatement's own for the smaller eigenvalue, harris_restatement.select on the Harris map"""
    return R.good_features(img, *sel, mask, bs) if k is None else H.select(term, *sel, mask=mask)


@pytest.mark.parametrize("k", (None,) + KS, ids=["shi-tomasi", "harris-0.04", "harris-0.15"])
@pytest.mark.parametrize("entry", B.RESIDUE_FRAMES, ids=[B.tag(e) for e in B.RESIDUE_FRAMES])
def test_mask_of_a_constant_band_lists_nothing(ectx, monkeypatch, entry, k):
    """The mask keeps the pixels whose term-by-term response is exactly 0: the band below the texture.  The restatement's
    masked maximum is 0, so it lists nothing.  Under that mask the strip kernel's only non-zero values are the residues its
    running sums carry out of the texture, and their sign decides whether it lists corners."""
    img, bs = B.build(entry), entry[2]
    term = B.references(entry)["term"] if k is None else HB.references(entry)[k]["term"]
    mask = (term == 0).astype(np.uint8) * 255
    what = (B.tag(entry), k)
    assert 0.3 <= (mask != 0).mean() <= 0.9, (what, float((mask != 0).mean()))
    ectx.upload_gray(0, img)
    got = response_map(ectx, bs, k)
    under = got[mask != 0]
    print("band mask: %-20s %-11s %4d of %5d masked pixels not 0 in the strip kernel's map, %d above 0, largest %.3g, smallest %.3g"
          % (B.tag(entry), "shi-tomasi" if k is None else "harris %.2f" % k, (under != 0).sum(), under.size, (under > 0).sum(),
             under.max(), under.min()))
    ectx.set_mask(mask)
    for sel in BAND_SELECTIONS:
        assert restated(img, term, sel, mask, bs, k) is None, (what, sel)
        lists_are(ectx, monkeypatch, None, sel, True, bs, k, what, no_candidates=True)
        # the same upload without the mask: the restatement's list, so a fault above is the mask's and not the map's
        whole = restated(img, term, sel, None, bs, k)
        assert whole is not None and len(whole) >= 5, (what, sel)
        lists_are(ectx, monkeypatch, whole, sel, False, bs, k, what)
