"""CPU: the velocity map's host statement (icelk_map_overlay_host: csrc/map_raster.h on the CPU) against the numpy
restatement, byte for byte; what the ABI refuses; the font; the colour table and the index rule against matplotlib; the
arrow scaling against the reference's; the strings, names and corner choice against the reference's expressions; and the
content against matplotlib's own quiver within the distance DESIGN.md 7.7 derives.  No GPU."""
import ctypes as C
import datetime as dt
import os
import re
import sys

import numpy as np
import pytest

import map_cases as mc
import map_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("width,views,variant", mc.CASES)
def test_host_statement_equals_restatement(width, views, variant):
    from iceberg_tracking_code_amd import map_overlay_host
    pic, want = mc.case(width, views, variant)
    got = map_overlay_host(pic)
    assert got.shape == want.shape == ((3 * width) // 4, width, 3)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=2))[:5]


def test_the_cases_hold_what_they_claim():
    """the shared pictures do exercise the rules' edges: every code of the base layer, thickness 1, 2 and 7, the head's cap,
    stacked arrows, arrows left out"""
    seen_thick = set()
    for variant in range(3):
        pic, want = mc.case(160, 2, variant)
        base, top, count = R.planes(pic)
        assert set(np.unique(base)) == {0, 1, 2, 3}
        for panel in pic["panels"]:
            view, lim = panel["view"], panel["limits"]
            w = R.arrow_width(view, lim, panel["width"])
            seen_thick.add(min(7, max(1, (w + 128) >> 8)))
            a = panel["arrows"]
            hits = [R.arrow_hits(view, lim, panel["width"], panel["pivot"], arrow) for arrow in a]
            assert len(hits[12]) == 1 and len(hits[13]) == 1                      # shorter than a pixel, zero length
            assert all(len(hits[k]) == 0 for k in (17, 18, 19, 20, 21, 22, 23))   # outside, NaN, inf, 2^20, beyond
            assert len(hits[15]) > 0 and len(hits[16]) > 0                        # partly outside
            assert [len(h) > 0 for h in hits[27:]] == [True, True, True, True, False, False, False, True]   # the speeds
            x0, y0 = view[:2]
            stacked = set(hits[24]) & set(hits[25]) & set(hits[26])
            assert stacked and all(top[y0 + q, x0 + p] == 27 and count[y0 + q, x0 + p] >= 3 for p, q in stacked)
    assert seen_thick == {1, 2, 7}
    # the cap: a 100 m (10 pixel) wide arrow 69 pixels long has a head of 48 pixels, not 50
    view, lim = (0, 0, 400, 300), (mc.X0, mc.X0 + 4000.0, mc.Y0, mc.Y0 + 3000.0)
    head = [h for h in R.arrow_hits(view, lim, 100.0, "tail", (mc.X0 + 500.0, mc.Y0 + 1500.0, 690.0, 0.0, 0.1)) if abs(h[1] - 150) > 4]
    assert min(p for p, _ in head) == 50 + 69 - 48 and max(abs(q - 150) for _, q in head) in (14, 15)


def test_stacked_arrows_blend_as_stated():
    """alpha 1: the painter's result; alpha 0.75: the top colour at the stacked opacity"""
    from iceberg_tracking_code_amd import map_overlay_host
    lim = (0.0, 640.0, 0.0, 480.0)
    arrows = np.array([(100.0, 100.0, 300.0, 0.0, s) for s in (0.1, 0.4, 0.2)])
    for alpha, n_hits in ((1.0, 3), (0.75, 3)):
        pic = dict(width=64, height=48, table=mc.table(), panels=[dict(view=(0, 0, 64, 48), limits=lim, arrows=arrows, width=10.0, alpha=alpha)])
        rgb = map_overlay_host(pic)
        assert np.array_equal(rgb, R.render(pic))
        over = mc.table()[R.colour_index(0.2, 0.5)].astype(float)
        want = 255 + (over - 255) * (1 - (1 - alpha) ** n_hits)
        assert np.abs(rgb[38, 20].astype(float) - want).max() <= 0.51


def _desc(pic):
    from iceberg_tracking_code_amd import map_descriptor
    return map_descriptor(pic)


def _host_rc(d):
    from iceberg_tracking_code_amd import _lib
    rgb = np.full((d.height if 0 < d.height < 4096 else 1, max(d.width, 1) if d.width < 4096 else 1, 3), 0xAA, np.uint8)
    rc = _lib.load().icelk_map_overlay_host(C.byref(d), None, None, 0, rgb.ctypes.data_as(_lib.u8p), rgb.strides[0])
    assert rc == _lib.OK or (rgb == 0xAA).all()          # a refused picture writes nothing
    return rc


def test_what_the_abi_refuses():
    from iceberg_tracking_code_amd import _lib, map_overlay_host
    pic, _ = mc.case(64, 2, 0)
    d, keep = _desc(pic)
    assert _host_rc(d) == _lib.OK
    cams = np.tile(np.array([[mc.X0 + 10.0, mc.Y0 + 10.0]]), (9, 1))

    def refused(change, code=_lib.EARG):
        d, keep = _desc(pic)
        hold = change(d)
        assert _host_rc(d) == code, change
        del hold
    for n in (8, 9):
        d, keep = _desc(pic)
        d.panel[1].cameras, d.panel[1].n_cameras = cams.ctypes.data, n
        assert _host_rc(d) == (_lib.OK if n == 8 else _lib.EARG)
    d, keep = _desc(pic)
    assert d.n_texts == 16
    d.n_texts = 17
    assert _host_rc(d) == _lib.EARG
    for bad in (b"12h30_x", b"50%", b"a" * 49, b"\xe2\x88\x92"):
        d, keep = _desc(pic)
        d.text[3].text = bad
        assert _host_rc(d) == _lib.EARG, bad
    refused(lambda d: setattr(d, "width", 63))
    refused(lambda d: setattr(d, "height", 0))
    refused(lambda d: setattr(d, "n_panels", 0))
    refused(lambda d: setattr(d, "n_panels", 3))
    refused(lambda d: setattr(d, "table", None))
    refused(lambda d: setattr(d.panel[0], "w", 0))
    refused(lambda d: setattr(d.panel[0], "x0", -1))
    refused(lambda d: setattr(d.panel[1], "w", d.panel[1].w + 13))          # past the picture's right edge
    refused(lambda d: setattr(d.panel[1], "h", d.height))
    refused(lambda d: setattr(d.panel[1], "x0", d.panel[0].x0 + 3))         # overlapping views
    refused(lambda d: setattr(d.panel[0], "bar_x0", d.width - 3))
    refused(lambda d: setattr(d.panel[0], "xmax", d.panel[0].xmin))
    refused(lambda d: setattr(d.panel[0], "ymin", float("nan")))
    refused(lambda d: setattr(d.panel[0], "pivot", 2))
    refused(lambda d: setattr(d.panel[0], "width", 0.0))
    refused(lambda d: setattr(d.panel[0], "alpha", 0.0))
    refused(lambda d: setattr(d.panel[0], "alpha", 1.5))
    refused(lambda d: setattr(d.panel[0], "vmax", float("inf")))
    refused(lambda d: setattr(d.panel[0], "n_arrows", -1))
    refused(lambda d: setattr(d.panel[0], "arrows", None))
    refused(lambda d: setattr(d.panel[0], "n_cells", (1 << 24) + 1))
    refused(lambda d: setattr(d.panel[0], "outline", None))
    refused(lambda d: setattr(d.text[0], "px", (1 << 20) + 1))
    refused(lambda d: setattr(d.panel[0], "resident", 1), _lib.ESTATE)      # resident arrows, and none given
    rgb = np.zeros((48, 64, 3), np.uint8)
    assert _lib.load().icelk_map_overlay_host(None, None, None, 0, rgb.ctypes.data_as(_lib.u8p), 192) == _lib.EARG
    d, keep = _desc(pic)
    assert _lib.load().icelk_map_overlay_host(C.byref(d), None, None, 0, None, 192) == _lib.EARG
    assert _lib.load().icelk_map_overlay_host(C.byref(d), None, None, 0, rgb.ctypes.data_as(_lib.u8p), 191) == _lib.EARG
    # the Python layer
    with pytest.raises(ValueError):
        map_overlay_host(dict(pic, texts=pic["texts"] + [(0, 0, "x")]))
    with pytest.raises(ValueError):
        map_overlay_host(dict(pic, texts=[(0, 0, "50%")]))
    with pytest.raises(ValueError):
        map_overlay_host(dict(pic, width=63))
    with pytest.raises(_lib.IcelkError):
        map_overlay_host(dict(pic, panels=[dict(pic["panels"][0], resident=True)]))


def test_resident_arrows_and_groups_on_the_host():
    from iceberg_tracking_code_amd import map_overlay_host
    pic, _ = mc.case(96, 1, 0)
    a = pic["panels"][0]["arrows"]
    group = (np.arange(len(a)) % 3).astype(np.int32)
    for g in (-1, 0, 1, 2):
        p = dict(pic, panels=[dict({k: v for k, v in pic["panels"][0].items() if k != "arrows"}, resident=True, group=g)])
        got = map_overlay_host(p, a, group)
        assert np.array_equal(got, R.render(p, a, group)), g
        if g >= 0:      # the picture of a group is the picture of its arrows alone but for the painter's order, which the index keeps
            sub = dict(pic, panels=[dict(pic["panels"][0], arrows=a[group == g])])
            assert np.array_equal(got, map_overlay_host(sub))
    assert np.array_equal(map_overlay_host(dict(pic, panels=[dict(pic["panels"][0], resident=True, group=-1)]), a), mc.case(96, 1, 0)[1])


def test_letter_glyphs_equal_the_drawings():
    from iceberg_tracking_code_amd import _lib, map_glyph, plot_glyph
    from iceberg_tracking_code_amd.velocity_map import MAP_CHARACTERS
    assert set(MAP_CHARACTERS.upper()) == set(R.GLYPHS) and len(R.GLYPHS) == 44
    for ch in MAP_CHARACTERS:
        assert map_glyph(ch) == R.GLYPHS[ch.upper()], ch
    for ch in "0123456789-:./ ":
        assert map_glyph(ch) == plot_glyph(ch)
    drawn = [tuple(v) for v in R.GLYPHS.values()]
    assert len(set(drawn)) == len(drawn)                                    # no two characters look alike
    rows = (C.c_uint8 * 7)()
    for ch in "_%#äµ\0":
        assert _lib.load().icelk_map_glyph(ord(ch), rows) == _lib.EARG
    assert _lib.load().icelk_map_glyph(ord("A"), None) == _lib.EARG
    # the segment picture's glyph set has not grown
    for ch in "Aa,()":
        assert _lib.load().icelk_plot_glyph(ord(ch), rows) == _lib.EARG, ch


SPEEDS = (0.0, float(np.nextafter(0.5, 0)), 0.5, 0.7, 1e-9, 0.25, 0.4999, 0.001953125, 0.49804687499999994, 123.0)


def test_colour_table_and_index_rule_against_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    from matplotlib.colors import Normalize
    from iceberg_tracking_code_amd import gist_rainbow_table
    cmap = matplotlib.colormaps["gist_rainbow"]
    table = gist_rainbow_table()
    assert table.shape == (256, 3) and table.dtype == np.uint8
    assert np.array_equal(table, cmap(np.arange(256), bytes=True)[:, :3])
    for vmax in (0.5, 0.3, 2.0):
        norm = Normalize(0, vmax)
        for s in SPEEDS + tuple(np.linspace(0, vmax, 1031)):
            assert tuple(table[R.colour_index(s, vmax)]) == tuple(cmap(norm(s), bytes=True)[:3]), (s, vmax)


def test_index_rule_of_the_library():
    """the library's index (seen through a one-arrow picture and a table whose entries differ) is the restatement's"""
    from iceberg_tracking_code_amd import map_overlay_host
    for s in SPEEDS:
        pic = dict(width=64, height=8, table=mc.table(), panels=[dict(view=(0, 0, 64, 8), limits=(0, 64, 0, 8), arrows=[(5.0, 4.5, 40.0, 0.0, s)],
                                                                      width=1.0, vmax=0.5)])
        assert tuple(map_overlay_host(pic)[3, 10]) == tuple(mc.table()[R.colour_index(s, 0.5)]), s


def _reference_dir():
    """where the golden generators read the reference from, if it is there"""
    text = open(os.path.join(ROOT, "tests", "golden", "make_ref_functions_golden.py")).read()
    path = re.search(r'^REF = "(.*)"', text, flags=re.M).group(1)
    return path if os.path.exists(os.path.join(path, "imports", "tracking_misc.py")) else None


def test_scaled_arrows_equal_the_reference():
    from iceberg_tracking_code_amd import scaled_arrows

    def restated(u, v, exponent=0.5, factor=250):       # imports/tracking_misc.py:61-74
        angles = np.arctan2(v, u)
        speed_scaled = (np.hypot(u, v) ** 0.5) * factor
        return [np.cos(angles) * speed_scaled, np.sin(angles) * speed_scaled]
    fns = [restated]
    ref = _reference_dir()
    if ref:
        sys.path.insert(0, ref)
        try:
            import imports.tracking_misc as trm
            fns.append(trm.scale_arrows)
        finally:
            sys.path.remove(ref)
    rng = np.random.default_rng(3)
    u, v = rng.normal(0, 0.2, 4000), rng.normal(0, 0.2, 4000)
    u[:6], v[:6] = (0, 0, 1e-300, -0.3, 0.3, np.nan), (0, 0.25, 0, 0, -0.3, 0.1)
    for fn in fns:
        for kw in (dict(), dict(exponent=0.2, factor=100)):
            for a, b in zip(scaled_arrows(u, v, **kw), fn(u, v, **kw)):
                assert a.dtype == np.float64 and np.array_equal(a.view(np.int64), np.asarray(b).view(np.int64))
        for a, b in zip(scaled_arrows(list(u[:9]), list(v[:9])), fn(list(u[:9]), list(v[:9]))):     # s3 passes lists
            assert np.array_equal(a.view(np.int64), np.asarray(b).view(np.int64))
    # the quirk: the exponent is ignored
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(scaled_arrows(u, v, exponent=0.2), scaled_arrows(u, v, exponent=0.9)))


def test_strings_names_and_corner_choice():
    from iceberg_tracking_code_amd import map_layout, map_name, map_strings, map_texts, map_view
    from iceberg_tracking_code_amd.velocity_map import map_corner_right
    day = dt.datetime(2019, 7, 24)
    start_datetime, end_datetime = day + dt.timedelta(hours=9.5), day + dt.timedelta(hours=10.0)
    min_time, max_time = dt.datetime(2019, 7, 24, 8, 30), dt.datetime(2019, 7, 24, 20, 0)
    grid_size, target_path = 250, "plots"
    for cam_with_tracks in (["UAS7"], ["UAS7", "UAS8", "cam_3"]):
        for time_window in (0.5, 24.0):
            # s3:522-536, 630-637 as they stand
            datestring = 'Date: {}'.format(day.strftime('%Y-%m-%d'))
            if time_window == 24.0:
                timestring = 'Time: ' + min_time.strftime('%H:%M') + '-' + max_time.strftime('%H:%M') + ' UTC'
                plotname = os.path.join(target_path, '{}-{}.png'.format(min_time.strftime('%Y%m%d_%H%M'), max_time.strftime('%H%M')))
            else:
                timestring = 'Time: ' + start_datetime.strftime('%H:%M') + '-' + end_datetime.strftime('%H:%M') + ' UTC'
                plotname = os.path.join(target_path, '{}-{}.png'.format(start_datetime.strftime('%Y%m%d_%H%M'), end_datetime.strftime('%H%M')))
            gridstring = 'Grid spacing: {} m'.format(grid_size)
            if len(cam_with_tracks) == 1:
                camstring = 'Camera: {}'.format(str(cam_with_tracks)[1:-1].replace("'", ''))
            else:
                camstring = 'Cameras: {}'.format(str(cam_with_tracks)[1:-1].replace("'", ''))
            assert map_strings(day, start_datetime, end_datetime, cam_with_tracks, grid_size, time_window, min_time, max_time) == \
                [datestring, timestring, camstring, gridstring]
            assert map_name(target_path, start_datetime, end_datetime, time_window, min_time, max_time) == plotname[:-4] + ".jpg"
    assert map_name("p", start_datetime, end_datetime) == os.path.join("p", "20190724_0930-1000.jpg")
    # the limits (s3:488-489, 662-663)
    fjord = dict(x=np.array([512345.6, 518000.2, 515000.0]), y=np.array([7455000.9, 7459123.4, 7457000.0]))
    x_coords, y_coords = fjord['x'], fjord['y']
    assert map_view(fjord, 1) == (int(np.min(x_coords)-500), int(np.max(x_coords)+300), int(np.min(y_coords)-300), int(np.max(y_coords)+300))
    assert map_view(fjord, 2) == (int(np.min(x_coords)-3000), int(np.max(x_coords)+300), int(np.min(y_coords)-300), int(np.max(y_coords)+300))
    # the corner test (s3:562, s3:778), as the reference has it
    min_x, max_x = 511845, 518300
    for xcord, ycord in ((512000.0, 7455000.0), (512000.0, 518000.0), (513000.0, 518000.0), (512345.0, 517800.0), (512345.1, 517800.0)):
        assert map_corner_right(xcord, ycord, (min_x, max_x, 0, 0)) == bool(xcord- min_x <= 500 and max_x - ycord  <= 500)
    # the layout in integers, and where the texts go
    limits = map_view(fjord, 1)
    for width, panels in ((1400, 1), (1400, 2), (64, 1), (64, 2), (333, 2)):
        L = map_layout(limits, width, panels)
        assert L["width"] == width and len(L["views"]) == panels and L["scale"] == max(1, width // 400)
        for v in L["views"]:
            assert v["h"] == max(1, (2 * v["w"] * (limits[3] - limits[2]) + (limits[1] - limits[0])) // (2 * (limits[1] - limits[0])))
            assert 0 <= v["x0"] and v["x0"] + v["w"] <= v["bar_x0"] and v["bar_x0"] + v["bar_w"] <= v["right"] <= width
            assert 0 <= v["y0"] and v["y0"] + v["h"] <= L["height"]
        assert all(a["right"] <= b["x0"] for a, b in zip(L["views"], L["views"][1:]))
    with pytest.raises(ValueError):
        map_layout(limits, 63)
    L = map_layout(limits, 1400, 1)
    strings = ["Date: 2019-07-24", "Time: 09:30-10:00 UTC", "Cameras: UAS7, UAS8", "Grid spacing: 250 m"]
    v = L["views"][0]
    left = map_texts(L, limits, strings, [(515000.0, 7456000.0)], (515000.0, 7456000.0, "Cameras"), 0.5, 1)
    assert [t for _, _, t in left] == strings + ["Cameras", "0.5", "0.0", "Speed (m/s)"]
    assert all(px == v["x0"] + (2 * v["w"]) // 100 for px, _, _ in left[:4]) and [py for _, py, _ in left[:4]] == \
        [v["y0"] + (20 * v["h"]) // 100 + 27 * n for n in range(4)]
    right = map_texts(L, limits, strings, [(512000.0, 518100.0)], (512000.0, 518100.0, "Camera"), 0.5, 1)
    assert all(px + 18 * len(t) == v["x0"] + v["w"] - (2 * v["w"]) // 100 for px, _, t in right[:4])
    assert [t for _, _, t in right[4:]] == ["0.5", "0.0", "Speed (m/s)"]      # that camera is 2^20 pixels off the map: no label
    both = map_texts(L, limits, strings, [(515000.0, 7456000.0), (512000.0, 518100.0)], (515000.0, 7456000.0, "Cameras"), 0.5, 1)
    assert len(both) == 12                                                    # one map: every camera picks its corner
    two = map_texts(map_layout(map_view(fjord, 2), 1400, 2), map_view(fjord, 2), strings, [(515000.0, 7456000.0), (512000.0, 518100.0)],
                    (515000.0, 7456000.0, "Cameras"), 0.5, 2)
    assert len(two) == 16 and sum(t == "Cameras" for _, _, t in two) == 2


# ---- content against the reference's own calls ---------------------------------------------------------------------------
# a canvas pixel with ink lies within D pixels (Chebyshev) of a pixel the rules mark, and the other way
# round.  Per axis, for an arrow w pixels wide (here 3 and 4, heads of 5 w <= the arrow's length, so neither side shortens
# the head): 0.5 (a canvas pixel with any coverage: its centre is within half a pixel of the shape) + 0.5 (a marked pixel
# stands for its centre: the line's sample is within half a pixel of the shaft's axis) + 0.75 (the thickness is w rounded
# and centred to within half a pixel) + w (1 - 1 / sqrt 2) / 2 = 0.59 (thickened along the minor axis, not across the
# shaft) = 2.34 on the shaft; 0.5 + 0.5 + 0.31 w = 2.24 at the head, whose back is straight where matplotlib's is swept
# (3 : 5 : 4.5: the notch 0.5 w in front of the barbs).  Distances between pixels are whole numbers: D = 2.
D = 2


def _far(a, b, d):
    """pixels of a farther than d (Chebyshev) from every pixel of b"""
    grown = np.zeros_like(b)
    ys, xs = np.nonzero(b)
    for dy in range(-d, d + 1):
        for dx in range(-d, d + 1):
            yy, xx = ys + dy, xs + dx
            ok = (yy >= 0) & (yy < b.shape[0]) & (xx >= 0) & (xx < b.shape[1])
            grown[yy[ok], xx[ok]] = True
    return a & ~grown


@pytest.mark.parametrize("pivot,mpl_pivot", (("tail", "tail"), ("mid", "mid")))
@pytest.mark.parametrize("width", (30.0, 40.0))
def test_content_against_matplotlib_quiver(pivot, mpl_pivot, width):
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from iceberg_tracking_code_amd import gist_rainbow_table, map_overlay_host
    vw, vh, m, vmax = 400, 300, 10.0, 0.5
    limits = (mc.X0, mc.X0 + m * vw, mc.Y0, mc.Y0 + m * vh)
    arrows = []
    for k in range(12):      # a lattice of isolated arrows 22 .. 59 pixels long: the four axis directions, then the octants
        ang = k * np.pi / 2 if k < 4 else 2 * np.pi * (k / 12.0) + 0.1 * (k % 3 == 1)
        length = m * (22 + 3.4 * k)
        arrows.append((limits[0] + m * (50 + 100 * (k % 4)) + 0.3 * k, limits[2] + m * (50 + 100 * (k // 4)) - 0.7 * k, length * np.cos(ang),
                       length * np.sin(ang), vmax * (k + 0.5) / 12))
    a = np.array(arrows)
    fig = plt.figure(figsize=(vw / 100.0, vh / 100.0), dpi=100, facecolor="w")
    try:
        ax = fig.add_axes([0, 0, 1, 1])
        ax.axis("off")
        ax.set_xlim(limits[0], limits[1])
        ax.set_ylim(limits[2], limits[3])
        ax.quiver(a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4], clim=[0.0, vmax], pivot=mpl_pivot, cmap="gist_rainbow", units="x", scale=1,
                  width=width, alpha=1)
        fig.canvas.draw()
        canvas = np.asarray(fig.canvas.buffer_rgba())[..., :3].copy()
    finally:
        plt.close(fig)
    assert canvas.shape == (vh, vw, 3)
    pic = dict(width=vw, height=vh, table=gist_rainbow_table(), panels=[dict(view=(0, 0, vw, vh), limits=limits, arrows=a, pivot=pivot, width=width,
                                                                              vmax=vmax)])
    mine = map_overlay_host(pic)
    assert np.array_equal(mine, R.render(pic))
    ink, marked = (canvas != 255).any(axis=2), (mine != 255).any(axis=2)
    assert marked.sum() > 12 * 22 * 3 and ink.sum() > 12 * 22 * 3
    print("ink %d marked %d; beyond %d: %d / %d" % (ink.sum(), marked.sum(), D, _far(ink, marked, D).sum(), _far(marked, ink, D).sum()))
    assert not _far(ink, marked, D).any() and not _far(marked, ink, D).any()
    # the colour at the centre of every shaft is the table's entry of the rule's index, in both.  Ours holds the table's
    # bytes (matplotlib's bytes=True: the entry times 255, truncated); the canvas holds the same entry as Agg makes bytes of
    # a float colour (times 255, rounded), so it is compared with that entry rounded: the same index, at most 1 apart
    table = gist_rainbow_table()
    entries = matplotlib.colormaps["gist_rainbow"](np.arange(256))[:, :3]
    for x, y, dx, dy, speed in a:
        f = (0.3 if pivot == "tail" else -0.2)                              # a point of the shaft well behind the head
        X, Y = R.fixed((0, 0, vw, vh), limits, x + f * dx, y + f * dy)
        idx = R.colour_index(speed, vmax)
        assert tuple(mine[Y >> 8, X >> 8]) == tuple(table[idx])
        assert tuple(canvas[Y >> 8, X >> 8]) == tuple(np.floor(entries[idx] * 255 + 0.5).astype(np.uint8))
        assert np.abs(canvas[Y >> 8, X >> 8].astype(int) - table[idx]).max() <= 1
