"""What travels with a handed-over template (k_lk_fast.hip, TmplIO) and what does not: the 2x2 matrix travels, the level's
verdict -- the minEig test against the pair's own threshold, the D test, 1/D -- is reached anew by the pair that takes
the template.  (Round 9 built the verdict's hand-over and took it out again: DESIGN.md 4.1.  These tests were written for
it and hold either way; they pin what a hand-over of the verdict would have to keep.)  On small frames whose contrast
falls from full to nothing in patches -- so that features fail at a coarse level only, at level 0, or nowhere -- the
segment loop with the hand-over equals, bit for bit, the loop without it (ICELK_NO_TEMPLATE_REUSE) and the reference
loop on the oracle, also where a pair brings another minEigThreshold than the pair that left the templates.

(The segment calls of the C ABI carry no flags: a pair with ICELK_FLAG_MIN_EIGENVALS cannot follow one without through
them; icelk_pyrlk, where the flag can be set, takes no templates.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 96, 80
CRIT = (3, 30, 0.01)
# contrast of the 24 x 20 patches, row by row: full texture, fading texture, flat
CONTRAST = [1.0, 0.3, 0.08, 0.0,
            0.04, 1.0, 0.02, 0.15,
            0.0, 0.06, 1.0, 0.03,
            0.5, 0.0, 0.1, 1.0]


def _frames(n, seed=7):
    from iceberg_tracking_code_amd import synth
    c = np.zeros((H, W), np.float32)
    for k, v in enumerate(CONTRAST):
        c[(k // 4) * 20:(k // 4 + 1) * 20, (k % 4) * 24:(k % 4 + 1) * 24] = v
    out = []
    for i in range(n):
        t = synth.frame(W, H, 90 * i, -70 * i, seed).astype(np.float32)
        out.append(np.clip(np.rint(128.0 + (t - 128.0) * c), 0, 255).astype(np.uint8))
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _oracle_pairs(orc, frames, p0, lk, thresholds):
    """The reference loop's pairs (s1:323-333) on the oracle with one minEigThreshold per pair: tracks and qualities of
    the survivors, and the backward status of every pair."""
    tracks = p0.reshape(-1, 1, 2).astype(np.float32)
    quality = np.zeros((len(tracks), 0), np.float32)
    st_b = []
    for i, thr in enumerate(thresholds):
        r = orc.track_fb(frames[i], frames[i + 1], tracks[:, -1], minEigThreshold=thr, **lk)
        keep = r["valid"].astype(bool)
        st_b.append((r["st_fwd"].copy(), r["st_bwd"].copy(), keep))
        tracks = np.concatenate([tracks, r["p1"].reshape(-1, 1, 2)], 1)[keep]
        quality = np.concatenate([quality, r["dist"].reshape(-1, 1)], 1)[keep]
    return tracks, quality, st_b


def _gpu_pairs(frames, lk, thresholds, hint):
    from iceberg_tracking_code_amd import Context
    ctx = Context(W, H, n_slots=len(frames), max_pts=4096)
    try:
        for i, f in enumerate(frames):
            ctx.upload_gray(i, f)
        ctx.seg_track_len_hint(hint)
        n = ctx.seg_detect(0, 0, 1e-4, 3, False, 3)
        p0, _ = ctx.seg_read()
        for i, thr in enumerate(thresholds):
            ctx.seg_track(i, i + 1, minEigThreshold=thr, **lk)
        tracks, quality = ctx.seg_read()
        return n, p0, tracks, quality, ctx.seg_template_stats()
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def frames():
    return _frames(4)


@pytest.mark.parametrize("win", [(21, 21), (15, 15)])
@pytest.mark.parametrize("levels", [2, 3])
@pytest.mark.parametrize("track_len", [2, 3])
def test_verdict_hand_over_changes_nothing(orc, monkeypatch, frames, win, levels, track_len):
    lk = dict(winSize=win, maxLevel=levels - 1, criteria=CRIT)
    thresholds = [1e-3] * track_len
    n, p0, ta, qa, (taken, left) = _gpu_pairs(frames, lk, thresholds, track_len)
    monkeypatch.setenv("ICELK_NO_TEMPLATE_REUSE", "1")
    nb, p0b, tb, qb, off = _gpu_pairs(frames, lk, thresholds, track_len)
    monkeypatch.delenv("ICELK_NO_TEMPLATE_REUSE")
    rt, rq, st = _oracle_pairs(orc, frames, p0, lk, thresholds)
    assert n == nb > 100 and off == (0, 0) and taken == track_len - 1 and left == track_len - 1
    assert np.array_equal(_bits(p0), _bits(p0b))
    assert ta.shape == tb.shape == rt.shape and len(ta) > 30
    assert np.array_equal(_bits(ta), _bits(tb)) and np.array_equal(_bits(qa), _bits(qb))
    assert np.array_equal(_bits(ta), _bits(rt)) and np.array_equal(_bits(qa), _bits(rq))
    # the content does what it is for: in a pair whose forward pass takes templates, survivors of the pair before fail at
    # level 0 (status 0) and others pass
    fwd = st[1][0]
    assert 0 < int((fwd == 0).sum()) < len(fwd)


@pytest.mark.parametrize("win", [(21, 21), (15, 15)])
@pytest.mark.parametrize("thresholds", [(1e-4, 2e-3, 1e-4), (2e-3, 1e-4, 2e-3)])
def test_another_threshold_is_judged_anew(orc, monkeypatch, frames, win, thresholds):
    """Pair to pair the minEigThreshold changes: a verdict reached under the other threshold must not be used."""
    lk = dict(winSize=win, maxLevel=2, criteria=CRIT)
    thresholds = list(thresholds)
    n, p0, ta, qa, (taken, left) = _gpu_pairs(frames, lk, thresholds, 3)
    monkeypatch.setenv("ICELK_NO_TEMPLATE_REUSE", "1")
    _, _, tb, qb, _ = _gpu_pairs(frames, lk, thresholds, 3)
    monkeypatch.delenv("ICELK_NO_TEMPLATE_REUSE")
    rt, rq, st = _oracle_pairs(orc, frames, p0, lk, thresholds)
    assert taken == 2 and left == 2
    assert ta.shape == tb.shape == rt.shape and len(ta) > 10
    assert np.array_equal(_bits(ta), _bits(tb)) and np.array_equal(_bits(qa), _bits(qb))
    assert np.array_equal(_bits(ta), _bits(rt)) and np.array_equal(_bits(qa), _bits(rq))
    # the change of threshold matters on this content: with the first pair's threshold kept, the second pair ends otherwise
    kept, _, _ = _oracle_pairs(orc, frames, p0, lk, [thresholds[0]] * 3)
    assert kept.shape != rt.shape or not np.array_equal(_bits(kept), _bits(rt))
