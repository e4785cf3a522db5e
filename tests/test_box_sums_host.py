"""The frames of tests/box_sum_frames.py and the bound of DESIGN.md section 4.2, on references alone (CPU).

What is shown here, before any kernel is asked anything: the frames really tell summation orders apart; the two
term-by-term statements (oracle, np_restatement) still agree bit for bit on them; the derived bound holds for two legal
orders of double addition and does not hold for a wrong term or a misplaced window; and the orders disagree in few pixels.
tests/test_gpu_box_sums.py then holds the kernels to the same bound.
"""
import os
import re

import numpy as np
import pytest

import box_sum_frames as B
import np_restatement as R
from test_restatement_oracle import same

ALL = B.FRAMES + B.RESIDUE_FRAMES
IDS = [B.tag(e) for e in ALL]
QUALITY, MIN_DISTANCE, MAX_CORNERS = (0.01, 0.007), (0, 4), (0, 50)

refs = B.references


def test_frame_list_covers_every_fused_block_size_and_every_extension():
    for bs in B.FUSED:
        assert sum(1 for e in B.FRAMES if e[2] == bs and e[4]) >= 2, bs
    shapes = {B.tag(e): B.build(e).shape for e in B.FRAMES}
    for e in B.FRAMES:
        h, w = shapes[B.tag(e)]
        assert h >= e[2] + 2 and w >= 48
    assert any(B.build(e).shape[1] > B.strip_cfg(e[2])["TW"] for e in B.FRAMES if e[2] == 10)       # a strip seam in x
    assert any(B.build(e).shape[0] > B.strip_cfg(e[2])["SH"] for e in B.FRAMES if e[2] == 10)       # ... and in y
    assert any(e[3].get("above") for e in B.FRAMES)
    assert len(set(IDS)) == len(IDS)


def test_strip_constants_are_those_of_the_kernel_source():
    """chain_length takes N from StripCfg: the restated constants are read back out of k_corners.hip."""
    src = open(os.path.join(os.path.dirname(__file__), "..", "iceberg_tracking_code_amd", "csrc", "k_corners.hip")).read()
    body = src[src.index("struct StripCfg {"):]
    body = body[:body.index("};")]
    for pattern in (r"NT = 256;", r"EW = NT - \(BS - 1\);", r"TW = EW - 2;", r"\bR = 4;", r"UNROLL = BS \* R / gcd_c\(BS, R\);",
                    r"EH = \(64 / UNROLL\) \* UNROLL;", r"SH = EH - 2;", r"NROWS = EH \+ BS - 1;", r"RX = 4;"):
        assert re.search(pattern, body), pattern
    assert [B.strip_cfg(bs)["SH"] for bs in B.FUSED] == [58, 58, 54, 58]
    assert [B.strip_cfg(bs)["TW"] for bs in B.FUSED] == [252, 250, 248, 245]
    assert [B.strip_cfg(bs)["NROWS"] for bs in B.FUSED] == [62, 64, 62, 69]
    # (bs - 1) + 2 EH + (bs - 1) + 2 (RX - 1)
    assert [B.chain_length(bs) for bs in B.FUSED] == [130, 134, 130, 144]


@pytest.mark.parametrize("entry", ALL, ids=IDS)
def test_products_are_the_restatements_and_some_window_is_inexact(entry):
    """The planes restated in box_sum_frames are the restatement's (their rows-first sums give its map bit for bit); and in
    at least one window of the frame the sequential double sum is not the exact sum: the frame can tell orders apart."""
    r = refs(entry)
    img, bs = r["img"], r["bs"]
    assert same(B.eig_of_sums(*B.rows_first_sums(img, bs))[0], r["term"])
    exact, seq = B.exact_sums(img, bs), B.sequential_sums(img, bs)
    inexact = np.any([e != s for e, s in zip(exact, seq)], axis=0)
    assert inexact.any()
    differs = not same(r["running"], r["term"])
    assert differs == entry[4]


def test_exact_sums_are_exact_where_a_double_can_show_it():
    """exact_sums against math.fsum (correctly rounded) at sampled windows, every plane."""
    import math
    entry = B.FRAMES[7]
    img, bs = B.build(entry), entry[2]
    h, w = img.shape
    by, bx = B.window_index(h, bs), B.window_index(w, bs)
    rng = np.random.RandomState(0)
    for p, s in zip(B.products(img, bs), B.exact_sums(img, bs)):
        for y, x in zip(rng.randint(0, h, 200), rng.randint(0, w, 200)):
            terms = [float(p[by[i][y], bx[j][x]]) for i in range(bs) for j in range(bs)]
            assert s[y, x] == math.fsum(terms)


@pytest.mark.parametrize("entry", ALL, ids=IDS)
def test_restatement_and_oracle_agree_bit_for_bit(orc, entry):
    """They share the term-by-term order, so rounding or not they must agree: the map and the corner lists, at every fused
    blockSize and at the unfused 4."""
    img = refs(entry)["img"]
    for bs in (3, 4, 5, 7, 10):
        assert same(orc.min_eig_map(img, bs), R.min_eig_map(img, bs)), bs
        for q in QUALITY:
            for md in MIN_DISTANCE:
                for maxc in MAX_CORNERS:
                    a, b = orc.good_features(img, maxc, q, md, None, bs), R.good_features(img, maxc, q, md, None, bs)
                    assert (a is None) == (b is None), (bs, q, md, maxc)
                    if a is not None:
                        assert same(a, b), (bs, q, md, maxc)


@pytest.mark.parametrize("entry", ALL, ids=IDS)
def test_bound_holds_for_two_orders_and_breaks_for_planted_errors(entry):
    r = refs(entry)
    img, bs, exact, bnd = r["img"], r["bs"], r["exact"], r["bound"]
    for name in ("term", "running"):
        ok = B.within_bound(r[name], img, bs, exact, bnd)
        assert ok.all(), (name, int((~ok).sum()))
    # planted: at the strongest pixel of the map, the window's largest term (dx*dx + dy*dy) dropped from all three sums ...
    y, x = (int(v) for v in np.unravel_index(int(np.argmax(exact)), exact.shape))
    xx, _, yy = B.products(img, bs)
    by, bx = B.window_index(img.shape[0], bs), B.window_index(img.shape[1], bs)
    k = int(np.argmax([float(xx[by[i][y], bx[j][x]]) + float(yy[by[i][y], bx[j][x]]) for i in range(bs) for j in range(bs)]))
    wrong = B.exact_map(img, bs, drop=(y, x, k))
    assert not same(wrong, exact)
    bad = ~B.within_bound(wrong, img, bs, exact, bnd)
    assert bad.sum() == 1 and bad[y, x]
    # ... and every window one row too low
    assert not B.within_bound(B.exact_map(img, bs, shift_rows=1), img, bs, exact, bnd).all()


@pytest.mark.parametrize("entry", B.FRAMES, ids=IDS[:len(B.FRAMES)])
def test_orders_disagree_in_few_pixels(entry):
    r = refs(entry)
    n = int((r["running"].view(np.uint32) != r["term"].view(np.uint32)).sum())
    assert n <= 0.01 * r["term"].size, n


def test_a_constant_band_keeps_a_running_sums_residue():
    """RESIDUE_FRAMES: below the texture the exact map is 0 and so is the term-by-term one; the running sum reads a residue
    of the texture's rounding in more than 1 % of the pixels, each far inside the bound."""
    for entry in B.RESIDUE_FRAMES:
        r = refs(entry)
        ne = r["running"].view(np.uint32) != r["term"].view(np.uint32)
        assert ne.sum() > 0.01 * ne.size
        assert np.all(r["term"][ne] == 0) and np.all(r["exact"][ne] == 0)
        assert np.abs(r["running"][ne]).max() < 1e-17 < r["bound"].min()
