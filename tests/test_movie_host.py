"""The host side of the movie: the scaler's host statement against Pillow's `resize(..., Image.BICUBIC)` and
against an independent numpy restatement (tests/movie_restatement.py), byte for byte; the size rule against a table
worked out by hand; a frame against Pillow's resize-then-save; the container against a RIFF walker written here from the
layout in DESIGN.md.  No GPU."""
import io
import struct

import numpy as np
import pytest
from PIL import Image

import movie_restatement as R
from iceberg_tracking_code_amd import movie as M


def _pillow(rgb, size):
    return np.asarray(Image.fromarray(rgb).resize(size, Image.BICUBIC))


@pytest.mark.parametrize("fill", R.FILLS)
@pytest.mark.parametrize("src,dst", R.CASES, ids=["%dx%d-%dx%d" % (s + d) for s, d in R.CASES])
def test_resize_host_is_pillow_and_restatement(src, dst, fill):
    rgb = R.pixels(src, fill)
    got = M.resize_host(rgb, dst)
    assert got.shape == (dst[1], dst[0], 3) and got.dtype == np.uint8
    assert np.array_equal(got, _pillow(rgb, dst))
    assert np.array_equal(got, R.resize(rgb, dst))
    if fill == "extremes" and dst[0] > src[0] >= 37:          # an enlargement of many 0 / 255 edges: the overshoot clips at both ends
        assert got.min() == 0 and got.max() == 255


def test_resize_host_with_a_row_stride_that_is_no_multiple_of_four():
    wide = R.pixels((39, 23), "random")                        # rows of 117 bytes
    view = wide[:, :37]
    assert view.strides[0] == 117 and view.strides[0] % 4 and not view.flags["C_CONTIGUOUS"]
    assert np.array_equal(M.resize_host(view, (64, 48)), _pillow(np.ascontiguousarray(view), (64, 48)))


def test_resize_host_refuses_what_it_cannot_hold():
    with pytest.raises(ValueError):
        M.resize_host(np.zeros((4, 4, 3), np.uint8), (0, 4))
    with pytest.raises(ValueError):
        M.resize_host(np.zeros((4, 4, 3), np.uint8), (4, 16385))
    with pytest.raises(ValueError):
        M.resize_host(np.zeros((4, 4), np.uint8), (4, 4))


def test_movie_size_table():
    # mh = max(16, (mw h div w + 8) div 16 * 16), by hand:
    assert M.movie_size(1200, 800) == (2000, 1328)             # 2000 * 800 div 1200 = 1333; 1341 div 16 = 83; 83 * 16
    assert M.movie_size(1400, 933) == (2000, 1328)             # 1866000 div 1400 = 1332; 1340 div 16 = 83
    assert M.movie_size(3, 1000) == (2000, 666672)             # 2000000 div 3 = 666666; 666674 div 16 = 41667; plain arithmetic
    assert M.movie_size(3, 1000, 48) == (48, 16000)            # 48000 div 3 = 16000, a multiple of 16
    assert M.movie_size(1000, 3) == (2000, 16)                 # 6000 div 1000 = 6; 14 div 16 = 0 -> 16
    assert M.movie_size(1200, 800, 0) == (1200, 800)           # the picture's own width; 800 = 50 * 16
    assert M.movie_size(1400, 933, -5) == (1400, 928)          # 933 + 8 = 941; 941 div 16 = 58; 58 * 16
    assert M.movie_size(1200, 800, 2000) == R.movie_size(1200, 800, 2000)
    with pytest.raises(ValueError):
        M.movie_size(0, 10)
    with pytest.raises(ValueError):
        M.movie_size(10, 10, 16385)


@pytest.mark.parametrize("quality", [75, 90])
def test_frame_host_is_pillows_resize_then_save(quality):
    rgb = R.pixels((37, 23), "random", seed=3)
    want = io.BytesIO()
    Image.fromarray(rgb).resize((64, 48), Image.BICUBIC).save(want, "JPEG", quality=quality)
    assert M.frame_host(rgb, (64, 48), quality) == want.getvalue()


# ---- the container -------------------------------------------------------------------------------------------------
def _chunks(data, pos, end):
    """[(fourcc, body offset, length)] of the chunks in data[pos:end], every one inside it, padded to an even length"""
    out = []
    while pos < end:
        assert pos + 8 <= end
        tag, n = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        assert pos + 8 + n <= end, tag
        out.append((tag, pos + 8, n))
        pos += 8 + n + (n & 1)
    assert pos == end
    return out


def _three_frames():
    frames = [M.frame_host(R.pixels((37, 23), "random", seed=s), (48, 32), 90) for s in (0, 2, 3)]
    assert {len(f) & 1 for f in frames} == {0, 1}, [len(f) for f in frames]   # an odd and an even length among them
    return frames


def test_container_layout(tmp_path):
    frames = _three_frames()
    path = tmp_path / "m.avi"
    with M.MovieWriter(path, fps=8, width=48) as mv:
        mv.add_rgb(R.pixels((37, 23), "random", seed=0))      # movie_size(37, 23, 48) = (48, 32)
        assert mv.size == (48, 32)
        for f in frames[1:]:
            mv.add_jpeg(f)
    data = path.read_bytes()
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack_from("<I", data, 4)[0] == len(data) - 8
    top = _chunks(data, 12, len(data))
    assert [t for t, _, _ in top] == [b"LIST", b"LIST", b"idx1"]
    (_, hdrl, hdrl_n), (_, movi, movi_n), (_, idx, idx_n) = top
    assert data[hdrl:hdrl + 4] == b"hdrl" and data[movi:movi + 4] == b"movi"
    head = _chunks(data, hdrl + 4, hdrl + hdrl_n)
    assert [t for t, _, _ in head] == [b"avih", b"LIST"] and head[0][2] == 56
    largest = max(len(f) for f in frames)
    avih = struct.unpack_from("<14I", data, head[0][1])
    assert avih[0] == 125000 and avih[2] == 0 and avih[3] == 0x10 and avih[4] == 3 and avih[5] == 0 and avih[6] == 1
    assert avih[7] == largest and avih[8:10] == (48, 32) and avih[10:] == (0, 0, 0, 0)
    assert avih[1] == -(-sum(len(f) for f in frames) * 8 // 3)                  # bytes a second, rounded up
    assert data[head[1][1]:head[1][1] + 4] == b"strl"
    strl = _chunks(data, head[1][1] + 4, head[1][1] + head[1][2])
    assert [(t, n) for t, _, n in strl] == [(b"strh", 56), (b"strf", 40)]
    at = strl[0][1]
    assert data[at:at + 8] == b"vidsMJPG"
    flags, prio, lang, initial, scale, rate, start, length, suggested, quality, sample = struct.unpack_from("<IHHIIIIIIII", data, at + 8)
    assert (flags, prio, lang, initial, scale, rate, start, length, suggested, quality, sample) == (0, 0, 0, 0, 1, 8, 0, 3, largest, 0xFFFFFFFF, 0)
    assert struct.unpack_from("<4H", data, at + 48) == (0, 0, 48, 32)
    size, w, h, planes, bits, comp, image, xp, yp, used, important = struct.unpack_from("<IiiHH4sIiiII", data, strl[1][1])
    assert (size, w, h, planes, bits, comp, image, xp, yp, used, important) == (40, 48, 32, 1, 24, b"MJPG", 3 * 48 * 32, 0, 0, 0, 0)
    body = _chunks(data, movi + 4, movi + movi_n)
    assert [t for t, _, _ in body] == [b"00dc"] * 3 and [n for _, _, n in body] == [len(f) for f in frames]
    assert idx_n == 16 * 3
    for k, (_, at, n) in enumerate(body):
        assert data[at:at + n] == frames[k]
        if n & 1:
            assert data[at + n] == 0                                            # the padding byte
        tag, flags, off, ln = struct.unpack_from("<4sIII", data, idx + 16 * k)
        assert (tag, flags, ln) == (b"00dc", 0x10, n) and movi + off == at - 8  # counted from the 'movi' fourcc
        want = np.asarray(Image.open(io.BytesIO(frames[k])).convert("RGB"))
        got = np.asarray(Image.open(io.BytesIO(data[at:at + n])).convert("RGB"))
        assert got.shape == (32, 48, 3) and np.array_equal(got, want)
    # Pillow decodes a frame to what it decodes the frame alone to; and the first frame is the picture's
    assert frames[0] == M.frame_host(R.pixels((37, 23), "random", seed=0), (48, 32), 90)


def test_read_avi_gives_the_frames_back(tmp_path):
    frames = _three_frames()
    path = tmp_path / "m.avi"
    mv = M.MovieWriter(path, fps=5)
    for f in frames:
        mv.add_jpeg(f)
    assert mv.frames == 3
    mv.close()
    mv.close()                                                                  # a second close does nothing
    got = M.read_avi(path)
    assert got["fps"] == 5 and (got["width"], got["height"]) == (48, 32) and got["frames"] == frames
    with pytest.raises(ValueError):
        mv.add_jpeg(frames[0])                                                  # closed


def test_no_frames_no_file(tmp_path):
    path = tmp_path / "empty.avi"
    with M.MovieWriter(path):
        pass
    assert not path.exists()


def test_add_jpeg_refuses_another_size(tmp_path):
    frames = _three_frames()
    other = M.frame_host(R.pixels((37, 23), "random"), (64, 48), 90)
    with M.MovieWriter(tmp_path / "m.avi") as mv:
        mv.add_jpeg(frames[0])
        with pytest.raises(ValueError):
            mv.add_jpeg(other)
        with pytest.raises(ValueError):
            mv.add_jpeg(b"not a jpeg")
        assert mv.frames == 1
    assert M.jpeg_size(other) == (64, 48)


def test_a_movie_past_the_limit_is_refused(tmp_path, monkeypatch):
    frames = _three_frames()
    monkeypatch.setattr(M, "MAX_FILE", 232 + 2 * (8 + 16) + sum(len(f) + (len(f) & 1) for f in frames[:2]) + 8)
    with M.MovieWriter(tmp_path / "m.avi") as mv:
        mv.add_jpeg(frames[0])
        mv.add_jpeg(frames[1])                                                  # exactly at the limit
        with pytest.raises(M.MovieTooLarge):
            mv.add_jpeg(frames[2])
    assert M.read_avi(tmp_path / "m.avi")["frames"] == frames[:2]


def test_drivers_refuse_a_movie_without_plots(tmp_path):
    import datetime as dt
    from iceberg_tracking_code_amd import track_image_sequence, utm_to_gridded_utm, utm_to_gridded_utm_days
    with pytest.raises(ValueError, match="movie needs plots"):
        track_image_sequence(["a.jpg"], str(tmp_path), 2, 10, movie=True)
    with pytest.raises(ValueError, match="movie needs plots"):
        utm_to_gridded_utm([], "", "", str(tmp_path), [], [], {}, dt.datetime(2020, 1, 1), 1.0, 250.0, 1, movie=True)
    with pytest.raises(ValueError, match="movie needs plots"):
        utm_to_gridded_utm_days([], [], "", "", str(tmp_path), [], [], {}, 1.0, 250.0, 1, movie=True)
