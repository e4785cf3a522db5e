"""The segment picture, the part that needs no GPU: the host statement of the rasteriser
(icelk_plot_overlay_host: csrc/plot_raster.h on the CPU) against the numpy restatement, byte for byte; the font against
the glyphs written out in tests/plot_restatement.py; the tables; what is refused; and the restatement against the
reference's own matplotlib calls, within two pixels."""
import ctypes as C

import numpy as np
import pytest

import plot_cases as pc
import plot_restatement as R


@pytest.mark.parametrize("vertices", pc.VERTICES)
@pytest.mark.parametrize("w,h,width", pc.SHAPES)
def test_host_statement_equals_the_restatement(w, h, width, vertices):
    from iceberg_tracking_code_amd import plot_overlay_host
    gray, tracks, stamp, want = pc.case(w, h, width, vertices)
    got = plot_overlay_host(gray, tracks, width, stamp)
    assert got.shape == want.shape and np.array_equal(got, want)
    # the cases do what they are there for
    lines, dots = R.counts(gray.shape, tracks, width)
    assert lines.max() > 0 and dots.max() > 31
    if width >= w:
        assert np.array_equal(R.background(gray, *R.size(w, h, width)), gray)
    if stamp:
        assert (want == R.STAMP_COLOUR).all(axis=2).any()


def test_the_stamp_runs_off_the_right_edge():
    w, h, width = pc.SHAPES[0]
    wo, ho = R.size(w, h, width)
    stamp = pc.STAMPS[2]
    assert (3 * wo) // 100 + 6 * len(stamp) > wo
    assert R.stamp_mask(stamp, wo, ho)[:, -1].any() or R.stamp_mask(stamp, wo, ho)[:, -2].any()


def test_tracks_left_out_whole_and_empty_table():
    from iceberg_tracking_code_amd import plot_overlay_host
    gray = pc.frame(64, 48)
    bare = plot_overlay_host(gray, np.zeros((0, 2, 2), np.float32), 24)
    assert np.array_equal(bare, np.repeat(R.background(gray, 24, 18)[..., None], 3, axis=2))
    for bad in (np.nan, np.inf, 2.0 ** 20, -(2.0 ** 20)):
        t = np.array([[[5, 5], [40, 30], [bad, 20]]], np.float32)
        assert np.array_equal(plot_overlay_host(gray, t, 24), bare), bad
    t = np.array([[[5, 5], [40, 30], [2.0 ** 20 - 1, 20]]], np.float32)
    assert not np.array_equal(plot_overlay_host(gray, t, 24), bare)


def test_font_is_the_one_written_out():
    from iceberg_tracking_code_amd import _lib, plot_glyph
    from iceberg_tracking_code_amd.plot import STAMP_CHARACTERS
    assert sorted(R.GLYPHS) == sorted(STAMP_CHARACTERS)
    for ch, rows in R.GLYPHS.items():
        assert plot_glyph(ch) == rows, ch
    lib = _lib.load()
    rows = (C.c_uint8 * 7)(*([0xAA] * 7))
    for ch in range(256):
        if chr(ch) not in R.GLYPHS:
            assert lib.icelk_plot_glyph(ch, rows) == _lib.EARG
    assert list(rows) == [0xAA] * 7


def test_tables():
    assert R.TL[0] == R.TD[0] == 65536
    assert R.TL[23] == 1 and R.TL[24:] == [0] * 8
    assert R.TD[12] == 1 and R.TD[13:] == [0] * 19
    # the library's tables are the restatement's: a pixel under k lines / k dots on black and on white shows TL[k] / TD[k]
    from iceberg_tracking_code_amd import plot_overlay_host
    for level in (0, 255):
        gray = np.full((8, 64), level, np.uint8)
        for k in (1, 2, 5, 23, 24, 31, 40):
            t = np.tile(np.array([[[2.0, 3.0], [30.0, 3.0]]], np.float32), (k, 1, 1))
            rgb = plot_overlay_host(gray, t, 64)
            n = min(k, 31)
            v1 = (level * R.TL[n] + 32768) >> 16
            assert rgb[3, 10, 1] == v1                                       # k lines
            assert rgb[3, 10, 0] == (level * R.TL[n] + 255 * (65536 - R.TL[n]) + 32768) >> 16
            assert rgb[3, 29, 1] == (v1 * R.TD[n] + 32768) >> 16             # k lines under k dots
            assert rgb[3, 30, 1] == (level * R.TD[n] + 32768) >> 16          # k dots
            assert (rgb[6, 10] == level).all()
    # the line's last column is 29: 256 c + 128 < Xb leaves the end point's own pixel to the dot
    lines, dots = R.counts((8, 64), np.array([[[2.0, 3.0], [30.0, 3.0]]], np.float32), 64)
    assert lines[3, 2:30].tolist() == [1] * 28 and lines[3, 30] == 0 and dots[3, 29:32].tolist() == [1, 1, 1]


def test_bad_arguments_write_nothing():
    from iceberg_tracking_code_amd import _lib
    lib = _lib.load()
    gray = pc.frame(64, 48)
    t = np.array([[[5, 5], [40, 30]]], np.float32)
    rgb = np.full((48, 64, 3), 0x5A, np.uint8)

    def call(width=24, stamp=b"12:30", tracks=t, vertices=2, w=64, h=48):
        return lib.icelk_plot_overlay_host(gray.ctypes.data_as(_lib.u8p), w, h, 64, tracks.ctypes.data_as(_lib.f32p), len(tracks), vertices,
                                           width, stamp, rgb.ctypes.data_as(_lib.u8p), 64 * 3)
    assert call() == _lib.OK
    rgb[:] = 0x5A
    assert call(stamp=b"12h30") == _lib.EARG                     # a character without a glyph
    assert call(stamp=b"1" * 49) == _lib.EARG
    assert call(width=7) == _lib.EARG
    assert call(vertices=0) == _lib.EARG and call(vertices=18) == _lib.EARG
    assert call(w=0) == _lib.EARG and call(h=70000) == _lib.EARG
    assert (rgb == 0x5A).all()
    assert call(stamp=b"1" * 48) == _lib.OK
    ow, oh = C.c_int(-1), C.c_int(-1)
    assert lib.icelk_plot_size(64, 48, 7, C.byref(ow), C.byref(oh)) == _lib.EARG and (ow.value, oh.value) == (-1, -1)
    assert lib.icelk_plot_size(64, 48, 8, C.byref(ow), C.byref(oh)) == _lib.OK and (ow.value, oh.value) == (8, 6)
    # quality belongs to the device calls, which check it (and width and stamp) before anything is enqueued:
    # tests/test_gpu_plot.py has 0 and 101 on a live handle.  Without a handle the calls refuse everything, untouched buffers
    n = C.c_uint64(77)
    for q in (0, 101, 90):
        assert lib.icelk_plot_tracks(None, 0, t.ctypes.data_as(_lib.f32p), 1, 2, 24, b"", q, None, 0, None, 0, C.byref(n)) == _lib.EARG
        assert lib.icelk_seg_plot(None, 0, 0, 24, b"", q, None, 0, None, 0, C.byref(n), None) == _lib.EARG
    assert n.value == 77
    from iceberg_tracking_code_amd import plot_overlay_host
    with pytest.raises(ValueError):
        plot_overlay_host(gray, t, 24, "12h30")
    with pytest.raises(ValueError):
        plot_overlay_host(gray, t, 7)


def test_names():
    from iceberg_tracking_code_amd import plot_name, plot_stamp
    assert plot_name("/a/plots", "/x/y/20190714-123005.jpg", 2, 60) == "/a/plots/20190714-123005_120sec.jpg"
    assert plot_stamp("/x/y/20190714-123005.jpg", 2, 60) == "20190714-123005 120/60"
    assert all(ch in R.GLYPHS for ch in plot_stamp("20190714-123005.jpg", 16, 3600))


# ---- the restatement against the reference's own drawing calls -----------------------------------------------------
def _isolated_tracks():
    """12 tracks on a 480 x 320 frame, each at least 12 px long, at least 16 px apart from each other"""
    rng = np.random.default_rng(5)
    T = []
    for k in range(12):
        cx, cy = 60 + 120 * (k % 4), 55 + 105 * (k // 4)        # a 4 x 3 lattice of cells 120 x 105
        a = rng.uniform(0, 2 * np.pi)
        r = rng.uniform(8, 20)                                  # half length: 16 .. 40 px long
        p = (cx - r * np.cos(a), cy - r * np.sin(a))
        q = (cx + r * np.cos(a), cy + r * np.sin(a))
        m = (cx + rng.uniform(-1, 1), cy + rng.uniform(-1, 1))
        T.append([p, m, q])
    T = np.array(T, np.float32)
    for i in range(12):
        assert np.hypot(*(T[i, -1] - T[i, 0])) >= 12
        for j in range(i):
            d = np.hypot(*(T[i][:, None, :] - T[j][None, :, :]).reshape(-1, 2).T)
            assert d.min() >= 16 + 40                            # vertices that far apart: the chords are 16 px apart at least
    return T


def _within(a, b, r):
    """every pixel of a lies within r (Chebyshev) of a pixel of b"""
    grown = np.zeros_like(b)
    H, W = b.shape
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            grown[max(0, dy):H + min(0, dy), max(0, dx):W + min(0, dx)] |= b[max(0, -dy):H + min(0, -dy), max(0, -dx):W + min(0, -dx)]
    return not (a & ~grown).any()


def test_restatement_against_the_reference_drawing_calls():
    """imshow + LineCollection(color='red', alpha=0.4) + plot('.', ms=2.5, alpha=0.6) of s1:410-420 on an axes that fills
    a 240 x 160 Agg canvas, against the restatement's marks at width 240: each within 2 pixels of the other."""
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import matplotlib.collections as mc
    import matplotlib.pyplot as plt
    W, H, wo, ho = 480, 320, 240, 160
    gray = np.full((H, W), 128, np.uint8)
    tracks = _isolated_tracks()
    assert R.size(W, H, wo) == (wo, ho)
    fig = plt.figure(figsize=(wo / 80.0, ho / 80.0), dpi=80)
    try:
        ax = fig.add_axes([0, 0, 1, 1])
        ax.imshow(gray, cmap="gray", vmin=0, vmax=255)
        ax.add_collection(mc.LineCollection(tracks, color="red", alpha=0.4))
        endpoints = np.float32([tr[-1] for tr in tracks]).reshape(-1, 2)
        ax.plot(endpoints[:, 0], endpoints[:, 1], ".", color="red", ms=2.5, alpha=0.6)
        ax.set_xlim([0, W])
        ax.set_ylim([H, 0])
        ax.set_aspect("auto")
        ax.axis("off")
        fig.canvas.draw()
        canvas = np.asarray(fig.canvas.buffer_rgba()).astype(np.int64)
    finally:
        plt.close(fig)
    assert canvas.shape[:2] == (ho, wo)
    theirs = canvas[..., 0] - canvas[..., 1] >= 40
    ours = R.marks(gray.shape, tracks, wo)
    assert theirs.sum() > 12 * 6 and ours.sum() > 12 * 6
    assert _within(theirs, ours, 2), "the reference marks a pixel more than 2 px from ours"
    assert _within(ours, theirs, 2), "we mark a pixel more than 2 px from the reference's"
