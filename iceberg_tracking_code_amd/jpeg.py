"""JPEG ingest with the pixel work on the device.

The host reads a baseline JPEG's headers and Huffman-decodes its scan into quantised DCT coefficients (`read_jpeg`:
csrc/abi_jpeg.hip, no GPU needed, the GIL is released, so a thread pool decodes files side by side); the device
dequantises, inverse-transforms, upsamples chroma and converts colour (csrc/k_jpeg.hip) -- into a tracker slot as a
cropped gray frame (`Context.upload_jpeg`, `SegmentTracker.push_jpeg`) or back to the host as pixels (`decode_jpeg`).
Pixels equal Pillow's (libjpeg's default decoder) bit for bit.

The reference's lossy re-save of the crop (s1:272: every photo is cropped with Pillow and saved again as JPEG, and the
loop tracks on those files) without the file: `resave_tables`, `resave_coefficients` (host) and `resave_rgb` (device)
give the tables, coefficients and pixels of `Image.fromarray(rgb).save(f, "JPEG", quality=...)`, bit for bit; the
uploads take it as `resave=` (`Context.upload_bgr` ...).

Taken: baseline (SOF0), 8 bit, Huffman coded, one interleaved scan, gray or YCbCr with 4:4:4 / 4:2:2 / 4:2:0 sampling,
restart markers, width >= 3.  Every other valid file raises `UnsupportedJpeg` -- the caller decodes it another way.
"""
import ctypes as C

import numpy as np

from . import _lib


class UnsupportedJpeg(ValueError):
    """A valid JPEG file of a kind the device decoder does not take (progressive, arithmetic coding, 12 bit, CMYK, other
    sampling factors, several scans, ...)."""


class JpegCoefficients:
    """What `read_jpeg` returns: `info` (the icelk_jpeg_info_t: size, sampling, quantisation tables, coefficient layout)
    and `coef`, the int16 coefficients in that layout."""

    def __init__(self, info, coef):
        self.info, self.coef = info, coef

    @property
    def coef_ptr(self):
        return C.c_void_p(self.coef.ctypes.data)

    @property
    def width(self):
        return self.info.width

    @property
    def height(self):
        return self.info.height

    @property
    def ncomp(self):
        return self.info.ncomp

    def blocks(self, c):
        """component c as (blocks_y, blocks_x, 8, 8) int16, natural order, not dequantised (a view)"""
        i = self.info
        n = i.blocks_x[c] * i.blocks_y[c] * 64
        return self.coef[i.coef_offset[c]:i.coef_offset[c] + n].reshape(i.blocks_y[c], i.blocks_x[c], 8, 8)

    def quant(self, c):
        return np.array(self.info.quant[c], np.uint16).reshape(8, 8)


def _check(rc, what):
    if rc == _lib.OK:
        return
    if rc == _lib.EUNSUP:
        raise UnsupportedJpeg("%s: a JPEG file of a kind the device decoder does not take" % what)
    if rc == _lib.ENOMEM:
        raise MemoryError(what)
    raise ValueError("%s: not a JPEG file, or a damaged one (icelk error %d)" % (what, rc))


def _stats_dict(st):
    """an icelk_jpeg_huff_stats_t as `Context.jpeg_huff_stats` returns it"""
    return {k: int(getattr(st, k)) for k, _ in st._fields_ if k != "reserved"}


def describe_jpeg(data):
    """The icelk_jpeg_info_t of a file given as bytes."""
    data = bytes(data)
    info = _lib.JpegInfo()
    _check(_lib.load().icelk_jpeg_describe(data, len(data), C.byref(info)), "icelk_jpeg_describe")
    return info


def read_jpeg(path_or_bytes, out=None):
    """The host stage: a path or the file's bytes -> JpegCoefficients.  `out`: an int16 array to decode into (e.g. a view
    of pinned memory from `Context.host_alloc`); it is used when it is large enough, else a new array is made."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    lib = _lib.load()
    info = _lib.JpegInfo()
    _check(lib.icelk_jpeg_describe(data, len(data), C.byref(info)), "icelk_jpeg_describe")
    n = int(info.coef_count)
    if out is not None and out.dtype == np.int16 and out.ndim == 1 and out.size >= n and out.flags.c_contiguous:
        coef = out[:n]
    else:
        coef = np.empty(n, np.int16)
    _check(lib.icelk_jpeg_read_coefficients(data, len(data), C.c_void_p(coef.ctypes.data), n), "icelk_jpeg_read_coefficients")
    return JpegCoefficients(info, coef)


def read_jpeg_lanes(data, subseq_bits=512, max_hops=256, max_rounds=8):
    """`read_jpeg` by the algorithm of the device's Huffman decoder (csrc/jpeg_lanes.h), run lane by lane on the CPU:
    (JpegCoefficients, statistics as `Context.jpeg_huff_stats` gives them).  No GPU needed; for tests and measurements."""
    data = bytes(data)
    lib = _lib.load()
    info = _lib.JpegInfo()
    _check(lib.icelk_jpeg_describe(data, len(data), C.byref(info)), "icelk_jpeg_describe")
    coef = np.empty(int(info.coef_count), np.int16)
    st = _lib.JpegHuffStats()
    _check(lib.icelk_jpeg_read_coefficients_lanes(data, len(data), C.c_void_p(coef.ctypes.data), coef.size, int(subseq_bits),
                                                  int(max_hops), int(max_rounds), C.byref(st)),
           "icelk_jpeg_read_coefficients_lanes")
    return JpegCoefficients(info, coef), _stats_dict(st)


def decode_jpeg(data, ctx=None, huffman="host"):
    """A path, the file's bytes or a JpegCoefficients -> H x W x 3 (R G B) or H x W uint8 array, the pixels
    np.array(PIL.Image.open(...)) gives, computed on the device.  `ctx`: a Context to run on (default: the one of the
    cv2-shaped functions, api.default_context).  huffman="device": the scan is Huffman-decoded on the device too
    (a path or bytes only)."""
    if huffman not in ("host", "device"):
        raise ValueError('huffman must be "host" or "device"')
    if huffman == "device":
        if isinstance(data, JpegCoefficients):
            raise ValueError('huffman="device" takes a path or the file\'s bytes')
        if not isinstance(data, (bytes, bytearray, memoryview)):
            with open(data, "rb") as f:
                data = f.read()
        data = bytes(data)
        if ctx is None:
            from .api import default_context
            info = describe_jpeg(data)
            ctx = default_context(info.width, info.height)
        return ctx.jpeg_decode_rgb_file(data)
    j = data if isinstance(data, JpegCoefficients) else read_jpeg(data)
    if ctx is None:
        from .api import default_context
        ctx = default_context(j.width, j.height)
    return ctx.jpeg_decode_rgb(j)


# ---- thumbnails: the inset photographs of the velocity map (csrc/thumb_raster.h) --------------------------
def _box2(box):
    bw, bh = (int(v) for v in box)
    return bw, bh


def thumbnail_size(width, height, box):
    """(tw, th): a width x height image fitted into box = (box_w, box_h), proportions kept, never enlarged
    (icelk_thumb_size)."""
    bw, bh = _box2(box)
    tw, th = C.c_int(0), C.c_int(0)
    if _lib.load().icelk_thumb_size(int(width), int(height), bw, bh, C.byref(tw), C.byref(th)) != _lib.OK:
        raise ValueError("an image outside 1 .. 65535 or a box outside 1 .. 16384 pixels a side")
    return tw.value, th.value


def thumbnail_host(image, size):
    """H x W or H x W x 3 uint8 -> its (th, tw, 3) thumbnail of size = (tw, th), every channel the exact area average, by the
    code the device runs, on the CPU (icelk_thumb_host).  No GPU is needed."""
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("expected an HxW or HxWx3 uint8 image")
    channels = 1 if a.ndim == 2 else a.shape[2]
    if a.strides[-1] != 1 or (a.ndim == 3 and a.strides[1] != channels) or a.strides[0] < channels * a.shape[1]:
        a = np.ascontiguousarray(a)
    tw, th = (int(v) for v in size)
    out = np.empty((max(th, 1), max(tw, 1), 3), np.uint8)
    rc = _lib.load().icelk_thumb_host(a.ctypes.data_as(_lib.u8p), a.shape[1], a.shape[0], channels, a.strides[0], tw, th,
                                      out.ctypes.data_as(_lib.u8p), out.strides[0])
    if rc == _lib.ENOMEM:
        raise MemoryError("icelk_thumb_host")
    if rc != _lib.OK:
        raise ValueError("icelk_thumb_host: a thumbnail larger than the image or smaller than one pixel")
    return out


def thumbnail(data_or_path, box, ctx=None):
    """A path or the bytes of a JPEG file -> its (th, tw, 3) uint8 thumbnail fitted into box = (box_w, box_h): decoded and
    reduced on the device (icelk_jpeg_thumb_file), equal to `thumbnail_host(np.asarray(Image.open(f).convert("RGB")),
    thumbnail_size(...))`.  `ctx`: as `decode_jpeg`.  Files the device decoder does not take raise `UnsupportedJpeg`."""
    if not isinstance(data_or_path, (bytes, bytearray, memoryview)):
        with open(data_or_path, "rb") as f:
            data_or_path = f.read()
    data = bytes(data_or_path)
    info = describe_jpeg(data)
    size = thumbnail_size(info.width, info.height, box)
    if ctx is None:
        from .api import default_context
        ctx = default_context(info.width, info.height)
    return ctx.jpeg_thumb_file(data, size)


# ---- the reference's re-save of the crop -----------------------------------------------------------------------------
REFERENCE_RESAVE_QUALITY = 75   # Pillow's default: `img_crop.save(outpath)` names none (camtools.py:64-104)


def resave_quality(resave):
    """The `resave=` keyword of the uploads and drivers -> a JPEG quality, or None for no re-save: None, "reference"
    (Pillow's default, 75, what the reference's crop pool writes) or an int in 1 .. 100."""
    if resave is None:
        return None
    if resave == "reference":
        return REFERENCE_RESAVE_QUALITY
    if isinstance(resave, (bool, str)) or int(resave) != resave or not 1 <= int(resave) <= 100:
        raise ValueError('resave must be None, "reference" or a JPEG quality in 1 .. 100')
    return int(resave)


def _rgb3(rgb):
    a = np.asarray(rgb)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("expected HxWx3 uint8 image")
    if a.strides[2] != 1 or a.strides[1] != 3 or a.strides[0] < 3 * a.shape[1]:
        a = np.ascontiguousarray(a)
    return a


def resave_tables(quality=75):
    """(luma, chroma): the 8 x 8 uint16 quantisation tables, natural order, of the file Pillow writes at `quality`."""
    quality = resave_quality(quality)
    luma, chroma = np.empty((8, 8), np.uint16), np.empty((8, 8), np.uint16)
    _check(_lib.load().icelk_jpeg_resave_tables(quality, C.c_void_p(luma.ctypes.data), C.c_void_p(chroma.ctypes.data)),
           "icelk_jpeg_resave_tables")
    return luma, chroma


def resave_coefficients(rgb, quality=75):
    """H x W x 3 (R G B) uint8 -> what `read_jpeg` returns for the file `Image.fromarray(rgb).save(f, "JPEG",
    quality=quality)` writes, computed on the host without writing it (csrc/jpeg_fwd.h): a JpegCoefficients that
    `Context.upload_jpeg` and `decode_jpeg` take as they take a file's."""
    a, quality = _rgb3(rgb), resave_quality(quality)
    lib = _lib.load()
    info = _lib.JpegInfo()
    args = (a.ctypes.data_as(_lib.u8p), a.shape[1], a.shape[0], a.strides[0], quality, C.byref(info))
    _check(lib.icelk_jpeg_resave_coefficients_host(*args, None, 0), "icelk_jpeg_resave_coefficients_host")
    coef = np.empty(int(info.coef_count), np.int16)
    _check(lib.icelk_jpeg_resave_coefficients_host(*args, C.c_void_p(coef.ctypes.data), coef.size), "icelk_jpeg_resave_coefficients_host")
    return JpegCoefficients(info, coef)


def resave_rgb(rgb, quality=75, ctx=None):
    """H x W x 3 (R G B) uint8 -> the pixels np.array(Image.open(f)) gives after `Image.fromarray(rgb).save(f, "JPEG",
    quality=quality)`, computed on the device (csrc/k_jpeg_fwd.hip, then the decoder's kernels).  `ctx`: as `decode_jpeg`."""
    a, quality = _rgb3(rgb), resave_quality(quality)
    if ctx is None:
        from .api import default_context
        ctx = default_context(a.shape[1], a.shape[0])
    return ctx.jpeg_resave_rgb(a, quality)


# ---- the re-saved crop as a file ---------------------------------------------------------------------------------------
def _encode_error(rc, what, message=""):
    """The exception of a writer call that returned `rc`, with the code in its `code` attribute: ValueError (ICELK_EARG: a
    coefficient the standard tables have no code for, or a descriptor the writer does not take), UnsupportedJpeg (restart
    intervals, a third quantisation table), IcelkError (ICELK_ECAP: more blocks than 32-bit bit offsets take; ...)."""
    text = "%s: icelk error %d%s" % (what, rc, ": " + message if message else "")
    e = {_lib.EARG: ValueError, _lib.EUNSUP: UnsupportedJpeg, _lib.ENOMEM: MemoryError}.get(rc, _lib.IcelkError)(text)
    e.code = rc
    return e


def _encode_call(call, guess, what, handle=None):
    """call(out, capacity, byref(len)) -> rc, into a buffer of `guess` bytes and, when the call says it takes more, into one
    of that size"""
    n, cap = C.c_uint64(0), int(guess)
    for _ in range(2):
        buf = np.empty(cap, np.uint8)
        rc = call(C.c_void_p(buf.ctypes.data), cap, C.byref(n))
        if rc == _lib.OK:
            return buf[:n.value].tobytes()
        if rc != _lib.ECAP or n.value <= cap:
            break
        cap = n.value
    msg = _lib.load().icelk_last_error(handle) if handle is not None else None
    raise _encode_error(rc, what, msg.decode() if msg else "")


def _comment_args(comment):
    if comment is None:
        return None, 0
    comment = bytes(comment)
    return comment, len(comment)


def source_comment(data):
    """The comment Pillow reports for a JPEG file given as bytes (`Image.open(f).info.get("comment")`): the body of the
    last COM segment in front of the scan, or None.  `crop().save()` carries it over into the re-saved crop, so the
    writers below take it as `comment=`."""
    data = bytes(data)
    found, pos = None, 2
    if data[:2] != b"\xff\xd8":
        return None
    while pos + 4 <= len(data) and data[pos] == 0xFF:
        m = data[pos + 1]
        if m == 0xFF:                                      # a fill byte
            pos += 1
            continue
        n = data[pos + 2] << 8 | data[pos + 3]
        if n < 2 or pos + 2 + n > len(data):
            break
        if m == 0xFE:
            found = data[pos + 4:pos + 2 + n]
        if m == 0xDA:
            break
        pos += 2 + n
    return found


def encode_header(info, comment=None):
    """SOI up to the end of the SOS segment of the file `encode_jpeg` writes for a descriptor (host)."""
    com, ncom = _comment_args(comment)
    lib = _lib.load()
    return _encode_call(lambda out, cap, n: lib.icelk_jpeg_encode_header(C.byref(info), com, ncom, out, cap, n), 1024 + ncom,
                        "icelk_jpeg_encode_header")


def encode_jpeg(coefficients, comment=None, ctx=None):
    """A JpegCoefficients -> the bytes of the baseline JPEG file libjpeg writes for them at its defaults (the Huffman tables
    of T.81 Annex K, no restart intervals, JFIF 1.01 without a density; csrc/jpeg_enc.h): `encode_jpeg(read_jpeg(f)) == f`
    for a file Pillow wrote without optimize=True.  Without `ctx` the scan is coded on the host, with a Context on the
    device (csrc/k_jpeg_enc.hip); the bytes are the same.  `comment`: the body of a COM segment, or None."""
    j = coefficients
    coef = np.ascontiguousarray(j.coef, np.int16)
    if coef.size < int(j.info.coef_count):
        raise ValueError("fewer coefficients than the descriptor counts")
    com, ncom = _comment_args(comment)
    ptr, guess = C.c_void_p(coef.ctypes.data), 4096 + ncom + coef.size
    if ctx is not None:
        return ctx.jpeg_encode(j.info, ptr, com, ncom, guess)
    lib = _lib.load()
    return _encode_call(lambda out, cap, n: lib.icelk_jpeg_encode_coefficients_host(C.byref(j.info), ptr, com, ncom, out, cap, n), guess,
                        "icelk_jpeg_encode_coefficients_host")


def resave_bytes(rgb, quality=75, comment=None, ctx=None):
    """H x W x 3 (R G B) uint8 -> the bytes `Image.fromarray(rgb).save(f, "JPEG", quality=quality)` writes, byte for byte.
    Without `ctx` on the host (csrc/jpeg_fwd.h, csrc/jpeg_enc.h); with a Context forward transform and entropy coder run
    on the device and only the file comes back (width >= 3 there).  `comment`: what Pillow carries over from the source of a
    crop (`source_comment`), or None."""
    a, quality = _rgb3(rgb), resave_quality(quality)
    com, ncom = _comment_args(comment)
    if ctx is not None:
        return ctx.jpeg_resave_bytes(a, quality, comment)
    lib = _lib.load()
    args = (a.ctypes.data_as(_lib.u8p), a.shape[1], a.shape[0], a.strides[0], quality, com, ncom)
    return _encode_call(lambda out, cap, n: lib.icelk_jpeg_resave_file_host(*args, out, cap, n), 4096 + ncom + a.shape[0] * a.shape[1],
                        "icelk_jpeg_resave_file_host")
