"""GPU: the velocity map written as a PNG file (icelk_map_draw_png: the drawing of icelk_map_draw / _insets, then the PNG
writer of csrc/k_png.hip on the resident R G B).  The file decodes with Pillow to exactly the pixels the
call hands back, which are the host rasteriser's; its bytes are the host statement's of those pixels; the JPEG calls
around it are undisturbed; and the day driver's `plot_format="png"` writes the reference's names."""
import io
import os

import numpy as np
import pytest
from PIL import Image

import day_grid_golden as G
import map_cases as mc
import thumb_cases as tc

pytestmark = pytest.mark.gpu


def _decode(data):
    im = Image.open(io.BytesIO(data))
    assert im.format == "PNG" and im.mode == "RGB"
    return np.asarray(im)


def _bare(insets):
    return [{k: v for k, v in q.items() if k != "pixels"} for q in insets]


@pytest.mark.parametrize("width,views,variant", [(64, 1, 0), (96, 2, 1), (160, 2, 2)])
def test_map_png_holds_exactly_the_rasterised_pixels(ctx, width, views, variant):
    from iceberg_tracking_code_amd import encode_png_host, map_overlay_host
    pic, want = mc.case(width, views, variant)
    before = ctx.map_draw(pic)
    data, rgb = ctx.map_draw(dict(pic, quality=3), want_rgb=True, format="png")       # the quality plays no part
    assert np.array_equal(rgb, want) and np.array_equal(rgb, map_overlay_host(pic))
    assert np.array_equal(_decode(data), rgb)
    assert data == encode_png_host(rgb)
    assert ctx.map_draw(pic, format="png") == data                                    # without the R G B
    assert ctx.map_draw(pic) == before                                                # the JPEG right after
    with pytest.raises(ValueError):
        ctx.map_draw(pic, format="gif")


@pytest.mark.parametrize("width,views", [(64, 2), (160, 1)])
def test_map_png_with_insets(ctx, width, views):
    from iceberg_tracking_code_amd import encode_png_host, map_overlay_host
    pic, _ = mc.case(width, views, 0)
    ctx.map_inset_release()
    try:
        for name in ("corners", "overlap"):
            insets = tc.inset_cases(width, pic["height"])[name]
            for q in insets:
                ctx.map_inset_set(q["index"], q["pixels"])
            full = dict(pic, insets=_bare(insets))
            before = ctx.map_draw(full)
            data, rgb = ctx.map_draw(full, want_rgb=True, format="png")
            assert np.array_equal(rgb, map_overlay_host(dict(pic, insets=insets))), name
            assert np.array_equal(_decode(data), rgb) and data == encode_png_host(rgb), name
            assert ctx.map_draw(full) == before
    finally:
        ctx.map_inset_release()


def test_map_png_with_resident_arrows(ctx):
    from iceberg_tracking_code_amd import encode_png_host, map_overlay_host
    pic, _ = mc.case(96, 1, 0)
    arrows = pic["panels"][0]["arrows"]
    group = (np.arange(len(arrows)) % 3).astype(np.int32)
    ctx.map_arrows_set(arrows, group)
    try:
        for g in (-1, 1):
            p = dict(pic, panels=[dict({k: v for k, v in pic["panels"][0].items() if k != "arrows"}, resident=True, group=g)])
            before = ctx.map_draw(p)
            data, rgb = ctx.map_draw(p, want_rgb=True, format="png")
            assert np.array_equal(rgb, map_overlay_host(p, arrows, group)), g
            assert np.array_equal(_decode(data), rgb) and data == encode_png_host(rgb), g
            assert ctx.map_draw(p) == before
    finally:
        ctx.map_arrows_release()


def test_day_driver_writes_png_maps(ctx, tmp_path, monkeypatch):
    from iceberg_tracking_code_amd import Context, utm_to_gridded_utm
    z = G.load()
    G.build_tree(z, str(tmp_path / "in"))
    camnames, schedule, drifts, fjord, day, grid_size, thr = G.args(z)
    cameras = [dict(camera=c, start_day=20190701, end_day=20190831, easting=float(fjord["x"].min() + 300.0 + 700.0 * k),
                    northing=float(fjord["y"].min() + 150.0 + 500.0 * k)) for k, c in enumerate(camnames) if c != "camD"]
    pixels = []
    draw = Context.map_draw

    def recording(self, picture, want_rgb=False, format="jpeg"):
        data, rgb = draw(self, picture, want_rgb=True, format=format)
        pixels.append(rgb)
        return data
    monkeypatch.setattr(Context, "map_draw", recording)

    def run(name, **kw):
        (tmp_path / name).mkdir()
        got = utm_to_gridded_utm(camnames, str(tmp_path / "in"), "utm", str(tmp_path / name), schedule, drifts, fjord, day, 0.5, grid_size, thr, ctx=ctx,
                                 plots=str(tmp_path / (name + "_plots")), plot_switch=2, speedthreshold_cbar=0.3, cameras=cameras, out_width=240, **kw)
        return got, sorted(os.listdir(str(tmp_path / (name + "_plots"))))
    got_jpg, jpgs = run("jpg")
    jpg_pixels, pixels = pixels, []
    got_png, pngs = run("png", plot_format="png")
    assert [n for n, _ in got_png] == [n for n, _ in got_jpg] and len(got_png) == 10
    assert pngs == sorted(n.split("_30min")[0] + ".png" for n, _ in got_png)            # the reference's names, and no .jpg
    assert jpgs == [n[:-4] + ".jpg" for n in pngs]
    assert len(jpg_pixels) == len(pixels) == 10
    for name, want in zip([n.split("_30min")[0] + ".png" for n, _ in got_png], jpg_pixels):
        with open(str(tmp_path / "png_plots" / name), "rb") as f:
            assert np.array_equal(_decode(f.read()), want), name
    with pytest.raises(ValueError):
        run("bad", plot_format="gif")
