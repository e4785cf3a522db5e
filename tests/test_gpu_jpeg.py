"""GPU: the device half of the JPEG ingest path (k_jpeg.hip behind icelk_jpeg_decode_rgb / icelk_upload_jpeg) against
Pillow -- every pixel equal --, against the existing upload_bgr path, and through track_image_sequence."""
import datetime as dt
import os

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as jc

pytestmark = pytest.mark.gpu

BIG = (531, 397)    # 67 x 50 blocks: several workgroups of the inverse DCT, tile boundaries of both kernels in x and y


def _equal_pillow(ctx, label, data):
    from iceberg_tracking_code_amd import decode_jpeg
    want = jc.pil_decode(data)
    got = decode_jpeg(data, ctx=ctx)
    assert got.shape == want.shape and got.dtype == np.uint8, label
    assert np.array_equal(got, want), (label, int(np.count_nonzero(got != want)))


def test_decode_equals_pillow_on_the_matrix(ctx):
    cases = jc.matrix(min_width=3)
    assert len(cases) > 250
    for label, data in cases:
        _equal_pillow(ctx, label, data)


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_decode_equals_pillow_across_workgroups(ctx, sub):
    _equal_pillow(ctx, "photo s%d" % sub, jc.encode(jc.photo(*BIG, 21), quality=85, subsampling=sub))
    # hard edges + full-range noise at quality 100: the clamps of the inverse DCT and of the colour conversion both work
    data = jc.encode(jc.edges(*BIG), quality=100, subsampling=sub)
    px = jc.pil_decode(data)
    assert (px == 0).any() and (px == 255).any()
    _equal_pillow(ctx, "edges s%d" % sub, data)


def test_decode_gray_file_and_narrow_chroma_planes(ctx):
    _equal_pillow(ctx, "gray", jc.encode(jc.photo(*BIG, 22, channels=1), quality=80))
    # chroma planes of 2 samples' width are replicated, not filtered; 3 samples is the narrowest filtered plane
    for w in (3, 4, 5, 6):
        for sub in (1, 2):
            _equal_pillow(ctx, "%dx9 s%d" % (w, sub), jc.encode(jc.photo(w, 9, 23), quality=90, subsampling=sub))


@pytest.fixture(scope="module")
def upload_files():
    out = {}
    for (w, h) in ((64, 48), BIG):
        for sub in (2, 0) + ((1,) if (w, h) == BIG else ()):
            data = jc.encode(jc.photo(w, h, 24), quality=90, subsampling=sub)
            out[(w, h, sub)] = (data, jc.pil_decode(data))
    return out


@pytest.mark.parametrize("variant", [3, 4])
@pytest.mark.parametrize("crop", [None, (0, 0, 0, 0), (5, 3, 7, 2), (16, 16, 16, 16)])
def test_upload_jpeg_equals_upload_bgr(ctx, upload_files, variant, crop):
    from iceberg_tracking_code_amd import read_jpeg
    for key, (data, pixels) in upload_files.items():
        ctx.upload_bgr(0, pixels, variant, crop)
        want = ctx.download_level(0, 0)
        ctx.upload_jpeg(1, read_jpeg(data), variant, crop)
        got = ctx.download_level(1, 0)
        assert got.shape == want.shape, (key, got.shape, want.shape)
        assert np.array_equal(got, want), (key, int(np.count_nonzero(got != want)))


def test_upload_jpeg_rejects_what_upload_bgr_rejects(ctx):
    from iceberg_tracking_code_amd import read_jpeg
    j = read_jpeg(jc.encode(jc.photo(64, 48, 25), quality=90))
    with pytest.raises(ValueError):
        ctx.upload_jpeg(0, j, 4, (32, 0, 32, 0))          # nothing left
    with pytest.raises(ValueError):
        ctx.upload_jpeg(0, j, 4, (-1, 0, 0, 0))
    with pytest.raises(ValueError):
        ctx.upload_jpeg(0, read_jpeg(jc.encode(jc.photo(64, 48, 25, channels=1))), 4)   # one component
    bad = read_jpeg(jc.encode(jc.photo(64, 48, 25), quality=90))
    bad.info.blocks_x[1] += 1                               # a descriptor that contradicts the image size
    with pytest.raises(ValueError):
        ctx.upload_jpeg(0, bad, 4)
    ctx.upload_jpeg(0, j, 4)                                # the handle is fine afterwards
    assert ctx.download_level(0, 0).shape == (48, 64)


def test_sequence_with_device_decoder_equals_pil_decoder(synth, tmp_path):
    """a folder like the one of test_gpu_sequence.py, one photo saved progressive (it goes through PIL)"""
    from iceberg_tracking_code_amd import UnsupportedJpeg, read_jpeg, track_image_sequence
    w, h, n, T, dts = 720, 540, 9, 2, 60
    grays, _ = synth.sequence(w, h, n, seed=31, max_step_px=2.0)
    src = tmp_path / "photos"
    src.mkdir()
    t0 = dt.datetime(2019, 7, 24, 10, 0, 0)
    names = []
    for k, g in enumerate(grays):
        rgb = np.stack([g, np.roll(g, 1, 1), np.roll(g, 1, 0)], 2)
        p = src / ((t0 + dt.timedelta(seconds=k * dts)).strftime("%Y%m%d-%H%M%S") + ".jpg")
        Image.fromarray(rgb).save(p, quality=95, progressive=(k == 3))
        names.append(str(p))
    with pytest.raises(UnsupportedJpeg):
        read_jpeg(names[3])
    crop = (24, 60, 16, 8)
    poly = [(40, 80), (700, 70), (690, 520), (300, 470), (50, 530)]
    fp = dict(maxCorners=400, qualityLevel=0.007, minDistance=10, blockSize=10)
    lk = dict(winSize=(21, 21), maxLevel=3, criteria=(3, 30, 0.01))
    res = {}
    for decoder in ("pil", "device"):
        dst = tmp_path / decoder
        dst.mkdir()
        res[decoder] = (track_image_sequence(names, str(dst), T, dts, crop=crop, mask_polygon=(poly, crop[0], crop[1]),
                                             feature_params=fp, lk_params=lk, decode_threads=3, decoder=decoder), dst)
    (a, da), (b, db) = res["pil"], res["device"]
    assert len(a) == len(b) == 4
    assert sorted(os.listdir(da)) == sorted(os.listdir(db)) and len(os.listdir(da)) == 4
    for (pa, ta, qa), (pb, tb, qb) in zip(a, b):
        assert os.path.basename(pa) == os.path.basename(pb) and len(ta) > 100
        assert np.array_equal(ta, tb) and np.array_equal(qa, qb)
        za, zb = np.load(pa, allow_pickle=False), np.load(pb, allow_pickle=False)
        assert np.array_equal(za["tracks"], zb["tracks"]) and np.array_equal(za["trackquality"], zb["trackquality"])
