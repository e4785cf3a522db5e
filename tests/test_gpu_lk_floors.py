"""The tracker's origin floors (k_lk_fast.hip: floor_uni through csrc/lk_uniform_math.h) against the oracle on 64x48 frames, for
the four tuned windows, on points whose floor is where a conversion can go wrong: exact integers, the float just below an
integer, tiny negative values, the frame's corners, a window width outside the frame on each side, +-2^30, +-inf and
NaN -- as they are (level 0 sees them) and times 2^level, so that every level of the pyramid sees them after the scaling
of p0.  Forward pass with its residual error (the floor of the error's origin) and forward+backward."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 64, 48
CRIT = (3, 30, 0.01)
WINDOWS = [(15, 15), (21, 21), (31, 31), (35, 35)]


def _points(win, levels):
    ww, wh = win
    hx, hy = (ww - 1) * 0.5, (wh - 1) * 0.5
    below = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))
    xs = [0.0, 1.0, 17.0, 40.0, W - 1.0,                                    # exact integers (window origin: integer or .5)
          hx, hx + 3.0, below(hx + 3.0), below(17.0), below(1.0),           # origin an exact integer / just below one
          -1e-30, -1e-38, -1e-42, -0.0, 1e-42, below(0.0),                   # tiny negative values (and a subnormal)
          hx - 1e-6, below(hx),                                              # origin a tiny negative value
          -float(ww), -float(ww) - 1.0, below(-float(ww) + hx), W + float(ww), W - 1.0 + float(ww), W + hx,
          2.0 ** 30, -2.0 ** 30, np.inf, -np.inf, np.nan]
    ys = [0.0, 1.0, 11.0, 30.0, H - 1.0,
          hy, hy + 3.0, below(hy + 3.0), below(11.0), below(1.0),
          -1e-30, -1e-38, -1e-42, -0.0, 1e-42, below(0.0),
          hy - 1e-6, below(hy),
          -float(wh), -float(wh) - 1.0, below(-float(wh) + hy), H + float(wh), H - 1.0 + float(wh), H + hy,
          2.0 ** 30, -2.0 ** 30, np.inf, -np.inf, np.nan]
    base = []
    for i, x in enumerate(xs):
        base.append((x, ys[i]))                       # the same kind in both coordinates
        base.append((x, 20.0 + 0.25 * (i % 4)))       # the kind in x, y inside
        base.append((24.0 + 0.25 * (i % 4), ys[i]))   # the kind in y, x inside
    corners = [(0.0, 0.0), (W - 1.0, 0.0), (0.0, H - 1.0), (W - 1.0, H - 1.0), (W - 0.5, H - 0.5), (-0.5, -0.5)]
    p = np.array(base + corners, np.float32)
    # ... and the same kinds as level l sees them: p * 2^l scales back to p exactly there
    with np.errstate(over="ignore", invalid="ignore"):
        return np.concatenate([p * np.float32(2.0 ** l) for l in range(levels)])


@pytest.fixture(scope="module")
def pair():
    from iceberg_tracking_code_amd import Context, synth
    f0, f1 = synth.frame(W, H, 0, 0, 3), synth.frame(W, H, 200, -120, 3)
    c = Context(W, H, n_slots=2, max_pts=4096)
    c.upload_gray(0, f0)
    c.upload_gray(1, f1)
    yield c, f0, f1
    c.close()


def _same(a, b, what, nan_is_nan=False):
    """Bit for bit.  nan_is_nan: a NaN equals a NaN whatever its sign and payload -- for the forward-backward distance of a
    +-inf point alone, |inf - inf|: the subtraction MAKES a NaN there, x86 and the device make different ones, and hypotf
    hands on what it is given (a NaN that came in with a point is carried bit for bit, and is compared that way)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        if nan_is_nan:
            assert np.array_equal(np.isnan(a), np.isnan(b)), what
            a, b = np.where(np.isnan(a), np.float32(0), a), np.where(np.isnan(b), np.float32(0), b)
        a, b = a.view(np.uint32), b.view(np.uint32)
    bad = np.flatnonzero((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(1))
    assert len(bad) == 0, "%s: rows %s differ: %s / %s" % (what, bad[:10].tolist(), a[bad[:4]].tolist(), b[bad[:4]].tolist())


@pytest.mark.parametrize("win", WINDOWS)
def test_floors_at_every_level(pair, orc, win):
    ctx, f0, f1 = pair
    levels = orc.pyramid_levels(W, H, win, 3) + 1
    pts = _points(win, levels)
    assert len(pts) < 4096
    got = ctx.pyrlk(0, 1, pts, None, win, 3, CRIT)
    ref = orc.pyrlk(f0, f1, pts, None, win, 3, CRIT)
    for g, r, what in zip(got, ref, ("nextPts", "status", "err")):
        _same(g, r, "%s %s" % (win, what))
    st = ref[1].ravel()
    assert 0.2 * len(pts) < st.sum() < 0.9 * len(pts)      # tracked and rejected points both
    fb = ctx.track_fb(0, 1, pts, win, 3, CRIT)
    rb = orc.track_fb(f0, f1, pts, win, 3, CRIT)
    for k in ("p1", "p0r", "st_fwd", "st_bwd", "err_fwd", "err_bwd", "dist", "valid"):
        _same(fb[k], rb[k], "%s %s" % (win, k), nan_is_nan=k == "dist")
