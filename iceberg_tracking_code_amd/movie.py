"""The movie of the pictures: what the reference makes of a day's segment pictures (s1_lucaskanade_tracking.py:452-473,
'tracks_oblique_<track_len * track_len_sec>sec.avi') and of a run's window maps (s3_utm_to_gridded_utm.py:194-215,
'velocities_utm_<minutes>min.avi') with imports/timelapse.sh: 8 frames per second, scaled to 2000 pixels wide.

The reference's codec (mencoder's msmpeg4v2) is not reproduced.  The file here is a Motion-JPEG AVI: every frame a baseline
JPEG, byte for byte `Image.fromarray(rgb).resize(size, Image.BICUBIC).save(f, "JPEG", quality=quality)` of the picture's
R G B, scaled and coded on the device from the pixels the picture writer left there (`Context.picture_frame`; the rule is
csrc/resize.h).  Here are the host-only parts: the size rule, the host statement of the scaler and of a
frame, the container's writer and a reader for it.

The container (AVI 1.0, no OpenDML; every number little-endian):

    'RIFF' size 'AVI '
      'LIST' size 'hdrl'
        'avih' 56   dwMicroSecPerFrame = 1000000 // fps, dwMaxBytesPerSec, 0, dwFlags = AVIF_HASINDEX (0x10), dwTotalFrames, 0,
                    dwStreams = 1, dwSuggestedBufferSize = the largest chunk, dwWidth, dwHeight, 0 0 0 0
        'LIST' size 'strl'
          'strh' 56 'vids' 'MJPG', 0, 0, 0, dwScale = 1, dwRate = fps, 0, dwLength = frames, dwSuggestedBufferSize,
                    dwQuality = 0xffffffff, dwSampleSize = 0, rcFrame = 0 0 width height (16 bits each)
          'strf' 40 BITMAPINFOHEADER: 40, width, height, planes 1, 24 bits, 'MJPG', biSizeImage = 3 width height, 0 0 0 0
      'LIST' size 'movi'
        '00dc' length, the JPEG file, a zero byte where the length is odd        (one per frame)
      'idx1' 16 frames
        '00dc', AVIIF_KEYFRAME (0x10), the chunk's offset counted from the 'movi' fourcc, its length   (one per frame)
"""
import ctypes as C
import os
import struct

import numpy as np

from . import _lib
from .jpeg import _rgb3, resave_bytes

MOVIE_FPS = 8          # imports/timelapse.sh is called with '8'
MOVIE_WIDTH = 2000     # ... and with dim1 = 2000, dim2 = -10
MOVIE_QUALITY = 90
MAX_FILE = (1 << 31) - (1 << 20)
_HEADER = 12 + 12 + (8 + 56) + 12 + (8 + 56) + (8 + 40)   # up to the 'LIST' of movi
AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10


def tracks_movie_name(track_len, track_len_sec):
    """'tracks_oblique_<track_len * track_len_sec>sec.avi' (s1:465)"""
    return "tracks_oblique_{}sec.avi".format(track_len * track_len_sec)


def velocities_movie_name(time_window):
    """'velocities_utm_<minutes>min.avi' (s3:211)"""
    return "velocities_utm_{}min.avi".format(int(time_window * 60.0))


def movie_size(w, h, width=MOVIE_WIDTH):
    """(mw, mh) of the movie of w x h pictures asked for `width` pixels wide (icelk_movie_size): mw = width, mh keeps the
    proportions, rounded to the nearest multiple of 16 and at least 16 -- mencoder's scale=W:-10.  width <= 0: the picture's
    own width."""
    mw, mh = C.c_int(0), C.c_int(0)
    if _lib.load().icelk_movie_size(int(w), int(h), int(width), C.byref(mw), C.byref(mh)) != _lib.OK:
        raise ValueError("a picture with a side outside 1 .. 16384, or a movie wider than 16384")
    return mw.value, mh.value


def resize_host(rgb, size):
    """H x W x 3 uint8 -> its (oh, ow, 3) resampling to size = (ow, oh) by the code the device's tables come from, on the CPU
    (icelk_resize_host): Pillow's `Image.fromarray(rgb).resize(size, Image.BICUBIC)`, byte for byte.  No GPU is needed."""
    a = _rgb3(rgb)
    ow, oh = (int(v) for v in size)
    out = np.empty((max(oh, 1), max(ow, 1), 3), np.uint8)
    rc = _lib.load().icelk_resize_host(a.ctypes.data_as(_lib.u8p), a.shape[1], a.shape[0], a.strides[0], ow, oh,
                                       out.ctypes.data_as(_lib.u8p), out.strides[0])
    if rc == _lib.ENOMEM:
        raise MemoryError("icelk_resize_host")
    if rc != _lib.OK:
        raise ValueError("icelk_resize_host: a side outside 1 .. 16384")
    return out


def frame_host(rgb, size, quality=MOVIE_QUALITY):
    """The movie frame of a picture on the host: `resize_host`, then the host statement of the JPEG writer
    (`jpeg.resave_bytes`) -- the bytes `Context.picture_frame` returns for the same picture."""
    return resave_bytes(resize_host(rgb, size), quality)


def jpeg_size(data):
    """(width, height) of a JPEG file's frame header, or None"""
    data, pos = bytes(data), 2
    if data[:2] != b"\xff\xd8":
        return None
    while pos + 4 <= len(data) and data[pos] == 0xFF:
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        n = data[pos + 2] << 8 | data[pos + 3]
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return (data[pos + 7] << 8 | data[pos + 8], data[pos + 5] << 8 | data[pos + 6]) if pos + 9 <= len(data) else None
        if n < 2 or m == 0xDA:
            return None
        pos += 2 + n
    return None


class MovieTooLarge(RuntimeError):
    """The next frame would take the file past 2^31 - 2^20 bytes: an AVI 1.0 file holds no more (there is no OpenDML here)."""


class MovieWriter:
    """A Motion-JPEG AVI written frame by frame (the layout is this module's docstring).

        with MovieWriter(path) as movie:
            ...draw a picture on ctx...
            movie.add_picture(ctx)

    The first frame fixes the movie's size: `movie_size` of the picture at `width`, or the size of the first `add_jpeg`
    frame.  Frames go to the file as they come; the counts, the largest chunk and the index are written by `close`.  A movie
    without frames writes no file."""

    def __init__(self, path, fps=MOVIE_FPS, width=MOVIE_WIDTH, quality=MOVIE_QUALITY):
        if int(fps) < 1 or not 1 <= int(quality) <= 100:
            raise ValueError("fps below 1 or a JPEG quality outside 1 .. 100")
        self.path, self.fps, self.width, self.quality = str(path), int(fps), int(width), int(quality)
        self.size = None
        self.frames = 0
        self._f = None
        self._index = []       # (offset from the 'movi' fourcc, length)
        self._closed = False

    # -- frames -----------------------------------------------------------------------------------
    def _size_for(self, w, h):
        if self.size is None:
            self.size = movie_size(w, h, self.width)
        return self.size

    def add_picture(self, ctx):
        """The frame of `ctx`'s most recent picture, resized and coded on the device (`Context.picture_frame`)."""
        size = self._size_for(*ctx.picture_size())
        self._append(ctx.picture_frame(size, self.quality))

    def add_rgb(self, rgb, ctx=None):
        """A frame of the caller's own H x W x 3 uint8 picture: resized and coded on the host, or with a Context on the
        device (`Context.resize_rgb`, `Context.jpeg_resave_bytes`); the bytes are the same."""
        a = _rgb3(rgb)
        size = self._size_for(a.shape[1], a.shape[0])
        if ctx is None:
            self._append(frame_host(a, size, self.quality))
        else:
            self._append(resave_bytes(ctx.resize_rgb(a, size), self.quality, ctx=ctx))

    def add_jpeg(self, data):
        """A ready frame: the bytes of a JPEG file of the movie's size (ValueError otherwise; the first frame sets it)."""
        data = bytes(data)
        size = jpeg_size(data)
        if size is None:
            raise ValueError("not a JPEG file with a frame header")
        if self.size is None:
            self.size = size
        if tuple(size) != tuple(self.size):
            raise ValueError("a frame of %d x %d in a movie of %d x %d" % (size + tuple(self.size)))
        self._append(data)

    def _append(self, data):
        if self._closed:
            raise ValueError("the movie is closed")
        if self._f is None:
            self._f = open(self.path, "wb")
            self._f.write(self._header())
        at = self._f.tell()
        padded = len(data) + (len(data) & 1)
        if at + 8 + padded + 8 + 16 * (self.frames + 1) > MAX_FILE:
            raise MovieTooLarge("%s: frame %d would take the file past %d bytes" % (self.path, self.frames, MAX_FILE))
        self._f.write(b"00dc" + struct.pack("<I", len(data)) + data + b"\0" * (len(data) & 1))
        self._index.append((at - (_HEADER + 8), len(data)))
        self.frames += 1

    # -- the container ----------------------------------------------------------------------------
    def _header(self, movi_bytes=0):
        """Everything up to the first frame, for what is known so far; `close` writes it again with the final numbers"""
        w, h = self.size
        n = self.frames
        largest = max([ln for _, ln in self._index], default=0)
        total = sum(ln for _, ln in self._index)
        per_sec = 0 if n == 0 else (total * self.fps + n - 1) // n
        avih = struct.pack("<14I", 1000000 // self.fps, per_sec, 0, AVIF_HASINDEX, n, 0, 1, largest, w, h, 0, 0, 0, 0)
        strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, 1, self.fps, 0, n, largest, 0xFFFFFFFF, 0, 0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", 3 * w * h, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        idx = 8 + 16 * n
        riff = 4 + 8 + len(hdrl) + 8 + 4 + movi_bytes + idx
        head = b"RIFF" + struct.pack("<I", riff) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl
        head += b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"
        assert len(head) == _HEADER + 12
        return head

    def close(self):
        """Finishes the file: the index behind the frames, the final numbers into the headers.  Without frames: nothing."""
        if self._closed:
            return
        self._closed = True
        if self._f is None:
            return
        try:
            end = self._f.tell()
            self._f.write(b"idx1" + struct.pack("<I", 16 * self.frames))
            self._f.write(b"".join(b"00dc" + struct.pack("<III", AVIIF_KEYFRAME, off, ln) for off, ln in self._index))
            self._f.seek(0)
            self._f.write(self._header(end - (_HEADER + 12)))
        finally:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def open_movie(movie, directory, name):
    """The `movie=` keyword of the drivers -> (MovieWriter, whether the driver owns and closes it): True writes `name` into
    `directory`, a path that file, a MovieWriter is used as it is and left open."""
    if isinstance(movie, MovieWriter):
        return movie, False
    if movie is True:
        return MovieWriter(os.path.join(str(directory), name)), True
    if isinstance(movie, (str, os.PathLike)):
        return MovieWriter(movie), True
    raise ValueError("movie is None, True, a path or a MovieWriter")


def read_avi(path):
    """dict(fps, width, height, frames=[bytes]) of a Motion-JPEG AVI as `MovieWriter` writes them: the '00dc' chunks of the
    'movi' list in file order, each without its padding."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError("%s: not an AVI file" % path)
    out = dict(fps=None, width=None, height=None, frames=[])

    def walk(pos, end):
        while pos + 8 <= end:
            tag, n = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
            body = pos + 8
            if tag == b"LIST":
                if data[body:body + 4] == b"movi":
                    frames(body + 4, body + n)
                else:
                    walk(body + 4, body + n)
            elif tag == b"strh":
                scale, rate = struct.unpack_from("<II", data, body + 20)
                out["fps"] = rate / scale if rate % scale else rate // scale
            elif tag == b"strf":
                out["width"], out["height"] = struct.unpack_from("<ii", data, body + 4)
            pos = body + n + (n & 1)

    def frames(pos, end):
        while pos + 8 <= end:
            tag, n = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
            if tag == b"00dc":
                out["frames"].append(data[pos + 8:pos + 8 + n])
            pos += 8 + n + (n & 1)

    walk(12, min(len(data), 8 + struct.unpack_from("<I", data, 4)[0]))
    return out
