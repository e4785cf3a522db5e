"""The Harris response on the frames of tests/box_sum_frames.py and tests/strip_arm_frames.py, and the bound of
tests/harris_box_sums.py, on references alone (CPU).

What is shown here, before any kernel is asked anything: harris_of_sums is the restatement's response behind its sums; the
derived Harris bound holds for two legal orders of double addition and does not hold for a wrong term or a misplaced window;
the orders disagree in few pixels; and over an exactly constant band a running sum's residue gives a Harris value <= 0 where
the term-by-term map has 0.  tests/test_gpu_harris_edges.py then holds the kernels to the same.
"""
import numpy as np
import pytest

import box_sum_frames as B
import harris_box_sums as HB
import harris_restatement as H
import strip_arm_frames as S
from test_restatement_oracle import same

ALL = B.FRAMES + B.RESIDUE_FRAMES
IDS = [B.tag(e) for e in ALL]
ARM_IDS = ["%s-bs%d" % c for c in S.CASES]
QUALITY, MIN_DISTANCE = (0.01, 0.007), (0, 4)


def differ(a, b):
    return a.view(np.uint32) != b.view(np.uint32)


def test_every_frame_and_both_k_are_covered():
    assert len(ALL) == 41 and len(set(IDS)) == 41 and HB.KS == (0.04, 0.15)
    assert {bs for _, bs in S.CASES} == set(B.FUSED)


def test_dropped_sums_is_exact_sums_with_a_term_dropped():
    entry = B.FRAMES[7]
    img, bs = B.build(entry), entry[2]
    sums = B.exact_sums(img, bs)
    for y, x, j in ((0, 0, 0), (5, 47, 48), (17, 20, 24), (img.shape[0] - 1, 3, 13)):
        got, want = HB.dropped_sums(img, bs, sums, y, x, j), B.exact_sums(img, bs, drop=(y, x, j))
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert any(a[y, x] != s[y, x] for a, s in zip(got, sums))


def held(r, k):
    """The assertions every frame is held to at one k; r: HB.references / HB.arm_references."""
    img, bs, sums = r["img"], r["bs"], r["sums"]
    m = r[k]
    exact, bnd = m["exact"], m["bound"]
    # the restated response behind the restatement's own sums is the restatement's map
    assert same(HB.harris_of_sums(*B.rows_first_sums(img, bs), k)[0], m["term"])
    for tail in (0, 1):
        assert same(HB.harris_of_sums(*B.rows_first_sums(img, bs), k, tail)[0], H.harris_map(img, bs, k, tail))
    for name in ("term", "running"):
        ok = HB.within_bound(m[name], exact, bnd)
        assert ok.all(), (name, int((~ok).sum()), float((np.abs(m[name].astype(np.float64) - exact) / bnd).max()))
    # planted: at the strongest pixel of the map, the window's largest term (dx*dx + dy*dy) dropped from all three sums ...
    y, x = (int(v) for v in np.unravel_index(int(np.argmax(exact)), exact.shape))
    xx, _, yy = B.products(img, bs)
    by, bx = B.window_index(img.shape[0], bs), B.window_index(img.shape[1], bs)
    j = int(np.argmax([float(xx[by[i][y], bx[n][x]]) + float(yy[by[i][y], bx[n][x]]) for i in range(bs) for n in range(bs)]))
    wrong = HB.harris_of_sums(*HB.dropped_sums(img, bs, sums, y, x, j), k)[0]
    assert not same(wrong, exact)
    bad = ~HB.within_bound(wrong, exact, bnd)
    assert bad.sum() == 1 and bad[y, x]
    # ... and every window one row too low
    assert not HB.within_bound(HB.exact_harris_map(img, bs, k, shift_rows=1), exact, bnd).all()


@pytest.mark.parametrize("k", HB.KS)
@pytest.mark.parametrize("entry", ALL, ids=IDS)
def test_bound_holds_for_two_orders_and_breaks_for_planted_errors(entry, k):
    held(HB.references(entry), k)


@pytest.mark.parametrize("k", HB.KS)
@pytest.mark.parametrize("case", S.CASES, ids=ARM_IDS)
def test_bound_holds_and_breaks_on_the_arm_frames(case, k):
    held(HB.arm_references(*case), k)


@pytest.mark.parametrize("k", HB.KS)
@pytest.mark.parametrize("entry", B.FRAMES, ids=IDS[:len(B.FRAMES)])
def test_orders_disagree_in_few_pixels(entry, k):
    m = HB.references(entry)[k]
    n = int(differ(m["running"], m["term"]).sum())
    assert n <= 0.01 * m["term"].size, n


@pytest.mark.parametrize("k", HB.KS)
@pytest.mark.parametrize("case", S.CASES, ids=ARM_IDS)
def test_orders_disagree_in_few_pixels_of_the_arm_frames(case, k):
    m = HB.arm_references(*case)[k]
    n = int(differ(m["running"], m["term"]).sum())
    assert n <= 0.01 * m["term"].size, n


@pytest.mark.parametrize("k", HB.KS)
@pytest.mark.parametrize("entry", B.RESIDUE_FRAMES, ids=IDS[len(B.FRAMES):])
def test_a_constant_bands_residue_gives_a_response_that_is_not_positive(entry, k):
    """Below the texture a = S dx^2 is exactly 0 in every order (its terms are exact), so R = -fl(bb) - fl(fl(kf c) c) of
    whatever residues b and c carry: never above zero.  Every pixel where the running map is not the term-by-term one reads 0
    there and a value <= 0 here, inside the bound."""
    m = HB.references(entry)[k]
    ne = differ(m["running"], m["term"])
    assert ne.any()
    assert np.all(m["term"][ne] == 0) and np.all(m["exact"][ne] == 0) and np.all(m["running"][ne] <= 0)
    assert HB.within_bound(m["running"], m["exact"], m["bound"])[ne].all()


@pytest.mark.parametrize("entry", ALL, ids=IDS)
def test_corner_lists_of_the_running_sum_map_are_the_restatements(entry):
    r = HB.references(entry)
    for k in HB.KS:
        m = r[k]
        for q in QUALITY:
            for md in MIN_DISTANCE:
                a, b = H.select(m["running"], 0, q, md), H.select(m["term"], 0, q, md)
                assert (a is None) == (b is None), (k, q, md)
                if a is not None:
                    assert same(a, b), (k, q, md)


def test_print_worst_ratios(capsys):
    """not an assertion beyond the bound's own: the figures DESIGN.md quotes for the CPU references"""
    worst = {k: 0.0 for k in HB.KS}
    most = 0
    for entry in ALL:
        r = HB.references(entry)
        for k in HB.KS:
            m = r[k]
            for name in ("term", "running"):
                worst[k] = max(worst[k], float((np.abs(m[name].astype(np.float64) - m["exact"]) / m["bound"]).max()))
            if entry in B.FRAMES:
                most = max(most, int(differ(m["running"], m["term"]).sum()))
    with capsys.disabled():
        print("\nharris box sums (CPU references): worst |R - exact| / bound %s, most differing pixels on FRAMES %d"
              % (", ".join("k %.2f: %.3g" % kv for kv in sorted(worst.items())), most))
    assert max(worst.values()) <= 1.0
