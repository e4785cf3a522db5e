"""The detector kernels on frames where double addition of the box sums rounds (tests/box_sum_frames.py).

The generic kernel adds term by term like the oracle and the restatement: bit for bit, no exception.  The strip kernel
(and the two-pass form, whose map is the strip kernel's and whose candidates get their value from sums of its own order)
adds in another order: every pixel is either bit-identical to the restatement or within the derived bound of DESIGN.md
section 4.2 of the exact reference, and on frames whose band keeps feeding terms at most 1 % of the pixels are not
identical.  The differences sit many orders of magnitude below qualityLevel * max, so every corner list is the restatement's.
The references and the bound are checked on the CPU alone in tests/test_box_sums_host.py.
"""
import numpy as np
import pytest

import box_sum_frames as B
import np_restatement as R
from test_restatement_oracle import same

pytestmark = pytest.mark.gpu

DETECTOR_SWITCHES = [None, "ICELK_TWO_PASS_CORNERS", "ICELK_GENERIC_CORNERS"]
ALL = B.FRAMES + B.RESIDUE_FRAMES
SELECTIONS = [(maxc, q, md) for q in (0.01, 0.007) for md in (0, 4) for maxc in (0, 50)]

_lists = {}


def expected_lists(entry):
    """The restatement's corner lists of one frame over SELECTIONS, computed once per session."""
    key = B.tag(entry)
    if key not in _lists:
        r = B.references(entry)
        _lists[key] = [R.good_features(r["img"], maxc, q, md, None, r["bs"]) for maxc, q, md in SELECTIONS]
    return _lists[key]


def context(switch, monkeypatch):
    from iceberg_tracking_code_amd import Context
    if switch:
        monkeypatch.setenv(switch, "1")
    return Context(320, 240, n_slots=1, max_pts=1 << 16)


def test_frames_cross_a_strip_seam_in_x_and_in_y():
    for bs in B.FUSED:
        cfg = B.strip_cfg(bs)
        shapes = [B.build(e).shape for e in B.FRAMES if e[2] == bs]
        assert any(w > cfg["TW"] for _, w in shapes) and any(h > cfg["SH"] for h, _ in shapes), bs


@pytest.mark.parametrize("switch", DETECTOR_SWITCHES)
def test_min_eig_map_on_rounding_box_sums(switch, monkeypatch):
    c = context(switch, monkeypatch)
    counts = []
    try:
        for entry in ALL:
            r = B.references(entry)
            c.upload_gray(0, r["img"])
            got = c.min_eig_map(0, r["bs"])
            ne = got.view(np.uint32) != r["term"].view(np.uint32)
            worst = float((np.abs(got.astype(np.float64) - r["exact"].astype(np.float64)) / r["bound"]).max())
            counts.append((B.tag(entry), int(ne.sum()), ne.size, worst))
            print("box sums: %-28s %-24s %4d of %5d pixels not identical, worst |eig - exact| / bound %.3g"
                  % (B.tag(entry), switch or "strip", ne.sum(), ne.size, worst))
            if switch == "ICELK_GENERIC_CORNERS":
                assert not ne.any(), (B.tag(entry), int(ne.sum()))
                continue
            ok = ~ne | B.within_bound(got, r["img"], r["bs"], r["exact"], r["bound"])
            assert ok.all(), (B.tag(entry), switch, int((~ok).sum()))
            if entry in B.FRAMES:
                assert ne.sum() <= 0.01 * ne.size, (B.tag(entry), switch, int(ne.sum()))
    finally:
        c.close()
    assert len(counts) == len(ALL)


@pytest.mark.parametrize("switch", DETECTOR_SWITCHES)
def test_corner_lists_on_rounding_box_sums(switch, monkeypatch):
    """icelk_good_features (the host's tail) and icelk_seg_detect + icelk_seg_read (the default tail): the restatement's
    list, in order, at qualityLevel 0.01 / 0.007, minDistance 0 / 4, maxCorners 0 / 50."""
    c = context(switch, monkeypatch)
    try:
        for entry in ALL:
            r = B.references(entry)
            c.upload_gray(0, r["img"])
            for (maxc, q, md), want in zip(SELECTIONS, expected_lists(entry)):
                what = (B.tag(entry), switch, maxc, q, md)
                got = c.good_features(0, maxc, q, md, False, r["bs"])
                assert (got is None) == (want is None), what
                if want is not None:
                    assert same(got, want), what
                n = c.seg_detect(0, maxc, q, md, False, r["bs"])
                assert n == (0 if want is None else len(want)), what
                if n:
                    tracks, _ = c.seg_read()
                    assert same(np.ascontiguousarray(tracks[:, 0, :]), want.reshape(-1, 2)), what
    finally:
        c.close()
