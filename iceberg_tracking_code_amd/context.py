"""Context: one GPU handle (icelk_t) with numpy-facing methods.

This is the host side of the hot path: everything here is argument marshalling around the C ABI of
include/icelk.h.  One Context per process per GPU (see DESIGN.md "Multi-GPU").
"""
import contextlib
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, f32p, u8p
from .plot import PLOT_QUALITY, PLOT_WIDTH, _stamp_arg, _tracks3, plot_size
from .velocity_map import _resident_args, map_descriptor, map_inset_array
from .orthophoto import FORMATS as ORTHO_FORMATS, _source_array, _source_bytes, opts_struct, raster_struct
from . import stabilize as _stab
from .jpeg import (UnsupportedJpeg, _comment_args, _encode_call, _rgb3, _stats_dict, describe_jpeg, resave_coefficients,
                   resave_quality, thumbnail_host, thumbnail_size)

TERM_CRITERIA_COUNT = 1
TERM_CRITERIA_MAX_ITER = 1
TERM_CRITERIA_EPS = 2
OPTFLOW_USE_INITIAL_FLOW = 4
OPTFLOW_LK_GET_MIN_EIGENVALS = 8
GRAY_CV3 = 3
GRAY_CV4 = 4
LK_GENERIC_KERNEL = 0x100
LK_MULTI_PER_WAVE = 0x200
FB_HYPOT = 0
FB_SQRT = 1

DEFAULT_CRITERIA = (TERM_CRITERIA_COUNT | TERM_CRITERIA_EPS, 30, 0.01)


def _u8(a):
    return a.ctypes.data_as(u8p)


def _f32(a):
    return a.ctypes.data_as(f32p)


def _gray2d(img, name="image"):
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError("%s must be a 2-D uint8 array (got %s %s)" % (name, a.dtype, a.shape))
    if a.strides[1] != 1 or a.strides[0] < a.shape[1]:
        a = np.ascontiguousarray(a)
    return a


def _crop4(crop):
    """(left, top, right, bottom) pixels to drop as four ints; None: nothing is dropped"""
    return (0, 0, 0, 0) if crop is None else tuple(int(v) for v in crop)


def _criteria(criteria):
    t, cnt, eps = criteria
    return int(t), int(cnt), float(eps)


# bytes first offered for a file of each kind (`_file_call`); a map's PNG is about 1.6 x its JPEG (profiles/png_map.txt)
FIRST_GUESSES = {"crop": 1 << 16, "resave": 1 << 16, "plot": 1 << 18, "map_jpeg": 1 << 18, "map_png": 1 << 18}
FRAME_FIRST_GUESS = 1 << 19   # ... and for a movie frame (`Context.picture_frame`)
ORTHO_FIRST_GUESS = 1 << 18   # ... and for an orthophoto (`Context.ortho_write`)


def _file_call(guesses, key, call, what, handle=None, extra=0):
    """A call that fills a file buffer: call(out, capacity, byref(len)) -> rc is offered guesses[key] + extra bytes, then what
    it says it takes (`_encode_call`); the next file of its kind is about as large: a quarter more is remembered for it."""
    data = _encode_call(call, guesses[key] + extra, what, handle)
    guesses[key] = max(1 << 16, len(data) + len(data) // 4)
    return data


def _rgb_out(want, width, height):
    """The optional R G B output of a picture call: (array or None, pointer or None, row stride)"""
    if not want:
        return None, None, 0
    rgb = np.empty((height, width, 3), np.uint8)
    return rgb, _u8(rgb), rgb.strides[0]


class Context:
    """Owns the device memory of `n_slots` resident frames (+ pyramids) and all point buffers."""

    def __init__(self, max_w, max_h, n_slots=3, max_pts=1 << 18, device=0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.max_w, self.max_h, self.n_slots, self.max_pts, self.device = max_w, max_h, n_slots, max_pts, device
        check(self._lib.icelk_create(device, max_w, max_h, n_slots, max_pts, C.byref(self._h)), None)
        self._guesses = dict(FIRST_GUESSES)
        self._ortho_size = None   # (width, height) of the mosaic `ortho_begin` began

    # -- lifetime -----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.icelk_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ck(self, rc):
        check(rc, self._h)

    def set_stream(self, stream_ptr):
        """Run on an existing HIP stream (e.g. torch.cuda.current_stream().cuda_stream)."""
        self._ck(self._lib.icelk_set_stream(self._h, C.c_void_p(stream_ptr or 0)))

    def sync(self):
        self._ck(self._lib.icelk_sync(self._h))

    def set_lk_kernel(self, which):
        """0 = default, LK_GENERIC_KERNEL or LK_MULTI_PER_WAVE: the three tracker kernels give identical results."""
        self._ck(self._lib.icelk_set_lk_kernel(self._h, int(which)))

    def set_variant(self, name, value):
        """A named build-dependent variant of OpenCV's arithmetic: "lk_sums" 0|1|2, "sobel_fma" 0..3, "eig_fma" 0|1
        (icelk_set_variant; 0 = default).  The oracle has the same switches (oracle.set_variant).  "lk_wide_sums" 1 is a
        testing aid: the tuned tracker kernels take their 64-bit wave sums everywhere; no result changes."""
        self._ck(self._lib.icelk_set_variant(self._h, name.encode(), int(value)))

    def set_fb_distance(self, form):
        """FB_HYPOT (np.hypot on float32, s1:330; default) or FB_SQRT ((dx**2+dy**2)**0.5, s0_1:99)."""
        self._ck(self._lib.icelk_set_fb_distance(self._h, int(form)))

    # -- ingest -------------------------------------------------------------------------------
    def upload_gray(self, slot, img):
        a = _gray2d(img)
        self._ck(self._lib.icelk_upload_gray(self._h, slot, _u8(a), a.shape[1], a.shape[0], a.strides[0]))

    def upload_bgr(self, slot, img, variant=GRAY_CV4, crop=None, resave=None):
        """3-channel frame -> gray in `slot` (s1:310-311).  `crop` = (left, top, right, bottom) pixels to drop, the
        box `Camera.crop_image` cuts (camtools.py:213-231): only the kept region crosses PCIe, straight out of the
        decoded frame.  `resave`: None -- pixel values are those of the frame -- or "reference" / a JPEG quality: the
        reference's lossy re-save of the crop (s1:272) is reproduced on the device, for a frame in R G B order, and the slot
        holds what `upload_bgr(slot, np.array(Image.open(re-saved crop)), variant)` leaves (icelk_upload_bgr_resave)."""
        a = _rgb3(img)                    # rows are dense; the row pitch of a cropped view is fine as it is
        if crop is not None:
            left, top, right, bottom = _crop4(crop)
            if min(left, top, right, bottom) < 0 or left + right >= a.shape[1] or top + bottom >= a.shape[0]:
                raise ValueError("crop box leaves no image")
            a = a[top:a.shape[0] - bottom, left:a.shape[1] - right]
        quality = resave_quality(resave)
        if quality is not None:
            self._ck(self._lib.icelk_upload_bgr_resave(self._h, slot, _u8(a), a.shape[1], a.shape[0], a.strides[0], variant, quality))
            return
        self._ck(self._lib.icelk_upload_bgr(self._h, slot, _u8(a), a.shape[1], a.shape[0], a.strides[0], variant))

    def upload_jpeg(self, slot, jpeg, variant=GRAY_CV4, crop=None, resave=None):
        """A file read by `jpeg.read_jpeg` -> gray in `slot`, exactly what `upload_bgr(slot, np.array(Image.open(f)),
        variant, crop, resave)` leaves there: inverse DCT, chroma upsampling, colour conversion, crop and gray run on the
        device (icelk_upload_jpeg); only the blocks the crop needs are transformed.  `resave`: as `upload_bgr`
        (icelk_upload_jpeg_resave)."""
        left, top, right, bottom = _crop4(crop)
        quality = resave_quality(resave)
        if quality is not None:
            self._ck(self._lib.icelk_upload_jpeg_resave(self._h, slot, C.byref(jpeg.info), jpeg.coef_ptr, variant, left, top,
                                                        right, bottom, quality))
            return
        self._ck(self._lib.icelk_upload_jpeg(self._h, slot, C.byref(jpeg.info), jpeg.coef_ptr, variant, left, top, right,
                                             bottom))

    def jpeg_decode_rgb(self, jpeg):
        """The decoded image of a file read by `jpeg.read_jpeg`: H x W x 3 (R G B) or H x W uint8, equal to Pillow's."""
        i = jpeg.info
        out = np.empty((i.height, i.width, 3) if i.ncomp == 3 else (i.height, i.width), np.uint8)
        self._ck(self._lib.icelk_jpeg_decode_rgb(self._h, C.byref(i), jpeg.coef_ptr, _u8(out), out.strides[0]))
        return out

    # -- JPEG files with the Huffman decoding on the device too (csrc/k_jpeg_huff.hip) ---------------
    def _ck_jpeg(self, rc):
        if rc == _lib.EUNSUP:
            raise UnsupportedJpeg("a JPEG file of a kind the device decoder does not take")
        self._ck(rc)

    def upload_jpeg_file(self, slot, data, variant=GRAY_CV4, crop=None, resave=None):
        """The bytes of a JPEG file -> gray in `slot`, as `upload_jpeg(slot, read_jpeg(data), variant, crop, resave)`
        leaves it: the scan is Huffman-decoded on the device as well (icelk_upload_jpeg_file), the coefficients never
        visit the host.  The same files are taken as by `read_jpeg`; others raise `UnsupportedJpeg`.  `resave`: as
        `upload_bgr` (icelk_upload_jpeg_file_resave)."""
        data = bytes(data)
        left, top, right, bottom = _crop4(crop)
        quality = resave_quality(resave)
        if quality is not None:
            self._ck_jpeg(self._lib.icelk_upload_jpeg_file_resave(self._h, slot, data, len(data), variant, left, top, right,
                                                                  bottom, quality))
            return
        self._ck_jpeg(self._lib.icelk_upload_jpeg_file(self._h, slot, data, len(data), variant, left, top, right, bottom))

    def upload_jpeg_file_async(self, slot, data, variant=GRAY_CV4, crop=None, resave=None, crop_file=False):
        """`upload_jpeg_file` ahead of the frame: the host's share and the errors it can see now, every device phase
        enqueued on a decode stream beside the tracker, no wait (icelk_upload_jpeg_file_async).  `data` is copied by the
        library and free when the call returns.  The slot holds no usable frame before `jpeg_async_finish(slot)` has
        returned -- or `jpeg_async_poll(slot)` says 1.  `resave`: as `upload_bgr`; the re-save is part of the enqueued
        job (icelk_upload_jpeg_file_async_resave).  `crop_file` (needs `resave`): the job also codes the crop's file,
        which `jpeg_async_finish_file(slot)` returns."""
        if isinstance(data, bytearray):
            buf = (C.c_char * len(data)).from_buffer(data)   # as it is: the library takes its own copy
        else:
            buf = data = bytes(data)
        left, top, right, bottom = _crop4(crop)
        quality = resave_quality(resave)
        if quality is None:
            if crop_file:
                raise ValueError("crop_file needs resave=: the file is the re-saved crop's")
            self._ck_jpeg(self._lib.icelk_upload_jpeg_file_async(self._h, slot, buf, len(data), variant, left, top, right, bottom))
            return
        self._ck_jpeg(self._lib.icelk_upload_jpeg_file_async_resave(self._h, slot, buf, len(data), variant, left, top, right, bottom,
                                                                    quality, 1 if crop_file else 0))

    def jpeg_async_poll(self, slot):
        """0: the slot's file is in flight, 1: decoded, 2: the host decoder has to take it (`jpeg_async_finish` does).
        A look at pinned memory; never blocks."""
        state = C.c_int(0)
        self._ck(self._lib.icelk_jpeg_async_poll(self._h, slot, C.byref(state)))
        return state.value

    def jpeg_async_finish(self, slot):
        """Waits for the verdict on the slot's file, has the host decoder take it where the device's bounds or the stream
        ask for that, and returns that file's statistics (the keys of `jpeg_huff_stats`).  Raises as `upload_jpeg_file`
        does; the slot then holds no frame."""
        st = _lib.JpegHuffStats()
        self._ck_jpeg(self._lib.icelk_jpeg_async_finish(self._h, slot, C.byref(st)))
        return _stats_dict(st)

    def jpeg_async_finish_file(self, slot, comment=None):
        """`jpeg_async_finish` for a file started with `resave=` and `crop_file=True`; returns (the bytes of the file
        Pillow's `Image.open(f).crop(box).save(out)` writes, a dictionary as `jpeg_crop_finish` returns).  `comment`: the
        source's comment (`jpeg.source_comment`) or None.  The job is gone afterwards, also when the call raises -- with one
        exception: a file started without `crop_file=True` (IcelkError, ICELK_ESTATE) stays in flight, nothing of it has
        been waited for, and `jpeg_async_finish(slot)` is still to be called."""
        return self._finish_file(lambda *args: self._lib.icelk_jpeg_async_finish_file(self._h, slot, *args), "icelk_jpeg_async_finish_file",
                                 comment, lambda: self._lib.icelk_jpeg_async_finish(self._h, slot, None))

    def _finish_file(self, call, what, comment, drop):
        """call(comment, its length, out, capacity, byref(len), byref(stats)) -> rc; (the file's bytes, the statistics).
        drop(): the library keeps a job whose file did not fit (ICELK_ECAP); this ends it here"""
        com, ncom = _comment_args(comment)
        st = _lib.JpegCropStats()
        try:
            data = _file_call(self._guesses, "crop", lambda out, cap, n: call(com, ncom, out, cap, n, C.byref(st)), what, self._h, ncom)
        except _lib.IcelkError as e:
            if getattr(e, "code", None) == _lib.ECAP:
                drop()
            raise
        stats = _stats_dict(st.huff)
        stats.update(route=_lib.JPEG_CROP_ROUTES[st.route], blocks=int(st.blocks), budget=int(st.budget), stream_len=int(st.stream_len))
        return data, stats

    def jpeg_crop_fwd_device_coefficients(self, data, crop=None, quality=75):
        """The coefficients of the file Pillow's `Image.open(f).crop(box).save(out, quality=quality)` writes, as the fused
        crop-and-forward kernel makes them from the decoded planes (icelk_jpeg_crop_fwd_device_coefficients), for tests."""
        data = bytes(data)
        left, top, right, bottom = _crop4(crop)
        i = describe_jpeg(data)
        w, h = i.width - left - right, i.height - top - bottom
        if w < 1 or h < 1:
            raise ValueError("crop box leaves no image")
        count = 384 * ((w + 15) // 16) * ((h + 15) // 16)    # 4 luma and 2 chroma blocks per MCU
        coef = np.empty(count, np.int16)
        self._ck_jpeg(self._lib.icelk_jpeg_crop_fwd_device_coefficients(self._h, data, len(data), left, top, right, bottom, int(quality),
                                                                        C.c_void_p(coef.ctypes.data), coef.size))
        return coef

    # -- the crop step on its own: decode, crop, re-save and encode in one enqueued piece (csrc/abi_jpeg_crop.hip on csrc/abi_jpeg_job.hip) --
    def jpeg_crop_config(self, stream_bytes_per_block=48):
        """Bytes of stuffed scan per block (1 .. 416) that a crop job started from now on may take on the device; a scan
        that takes more is coded again at `jpeg_crop_finish` with host-read sizes (route "over-budget"), same bytes."""
        self._ck(self._lib.icelk_jpeg_crop_config(self._h, int(stream_bytes_per_block)))

    def jpeg_crop_start(self, data, crop=None, quality=75):
        """Starts the reference's crop step for one photo given as bytes -- Huffman decoding, inverse DCT, the crop box,
        the re-save at `quality` ("reference" or 1 .. 100) and the entropy coder, enqueued on a decode stream without a wait
        (icelk_jpeg_crop_start) -- and returns its ticket.  No frame slot is touched and the handle's max_w x max_h bound
        nothing.  `data` is copied by the library.  Raises as `upload_jpeg_file(resave=)` does; no ticket is taken then."""
        quality = resave_quality(quality)
        if quality is None:
            raise ValueError('quality must be "reference" or a JPEG quality in 1 .. 100')
        if isinstance(data, bytearray):
            buf = (C.c_char * len(data)).from_buffer(data)
        else:
            buf = data = bytes(data)
        left, top, right, bottom = _crop4(crop)
        ticket = C.c_int(0)
        self._ck_jpeg(self._lib.icelk_jpeg_crop_start(self._h, buf, len(data), left, top, right, bottom, quality, C.byref(ticket)))
        return ticket.value

    def jpeg_crop_poll(self, ticket):
        """0: the job is in flight, 1: its file is coded on the device, 2: `jpeg_crop_finish` has host work to do (the host
        decoder, or a scan over the budget).  A look at pinned memory; never blocks."""
        state = C.c_int(0)
        self._ck(self._lib.icelk_jpeg_crop_poll(self._h, int(ticket), C.byref(state)))
        return state.value

    def jpeg_crop_finish(self, ticket, comment=None):
        """Waits for the job and returns (the bytes of the file Pillow's `Image.open(f).crop(box).save(out)` writes, a
        dictionary: the keys of `jpeg_huff_stats` for the source file, "route" -- "device", "host-huffman" or
        "over-budget" --, "blocks", "budget" and "stream_len").  `comment`: the source's comment (`jpeg.source_comment`),
        which Pillow carries over, or None.  The ticket is gone afterwards, also when the call raises."""
        return self._finish_file(lambda *args: self._lib.icelk_jpeg_crop_finish(self._h, int(ticket), *args), "icelk_jpeg_crop_finish",
                                 comment, lambda: self._lib.icelk_jpeg_crop_cancel(self._h, int(ticket)))

    def jpeg_crop_cancel(self, ticket):
        """Waits for what the job has enqueued and drops the ticket."""
        self._ck(self._lib.icelk_jpeg_crop_cancel(self._h, int(ticket)))

    def jpeg_decode_rgb_file(self, data):
        """The decoded image of a JPEG file given as bytes, Huffman decoding included on the device."""
        data = bytes(data)
        i = describe_jpeg(data)
        out = np.empty((i.height, i.width, 3) if i.ncomp == 3 else (i.height, i.width), np.uint8)
        self._ck_jpeg(self._lib.icelk_jpeg_decode_rgb_file(self._h, data, len(data), _u8(out), out.strides[0]))
        return out

    def jpeg_thumb_file(self, data, size):
        """The (th, tw, 3) thumbnail of size = (tw, th) of a JPEG file given as bytes: decoded on the device as
        `jpeg_decode_rgb_file` decodes it and reduced there from the component planes, every channel the exact area average
        (icelk_jpeg_thumb_file; `jpeg.thumbnail_size` gives the size of a box).  Equal to `jpeg.thumbnail_host` of Pillow's
        pixels."""
        data = bytes(data)
        tw, th = (int(v) for v in size)
        out = np.empty((max(th, 1), max(tw, 1), 3), np.uint8)
        self._ck_jpeg(self._lib.icelk_jpeg_thumb_file(self._h, data, len(data), tw, th, _u8(out), out.strides[0]))
        return out

    def jpeg_resave_rgb(self, rgb, quality=75):
        """H x W x 3 (R G B) uint8 -> the pixels of the image saved as JPEG at `quality` and opened again (`jpeg.resave_rgb`)."""
        a = np.ascontiguousarray(_rgb3(rgb))
        out = np.empty(a.shape, np.uint8)
        self._ck(self._lib.icelk_jpeg_resave_rgb(self._h, _u8(a), a.shape[1], a.shape[0], a.strides[0], int(quality), _u8(out),
                                                 out.strides[0]))
        return out

    def jpeg_resave_file(self, comment=None):
        """The bytes of the JPEG file of the handle's most recent re-save (an upload with `resave=`, `jpeg_resave_rgb`,
        `jpeg_resave_device_coefficients`): what Pillow's `crop.save(path)` writes for that crop, entropy-coded on the device
        from the coefficients the re-save left there (icelk_jpeg_resave_encode).  No slot is touched.  `comment`: the
        source's comment (`jpeg.source_comment`), which Pillow carries over, or None.  IcelkError (code ICELK_ESTATE) when
        the handle has never re-saved."""
        com, ncom = _comment_args(comment)
        return _file_call(self._guesses, "resave", lambda out, cap, n: self._lib.icelk_jpeg_resave_encode(self._h, com, ncom, out, cap, n),
                          "icelk_jpeg_resave_encode", self._h, ncom)

    def jpeg_encode(self, info, coef_ptr, comment, comment_len, guess):
        """`jpeg.encode_jpeg` on the device (icelk_jpeg_encode_coefficients)."""
        return _encode_call(lambda out, cap, n: self._lib.icelk_jpeg_encode_coefficients(self._h, C.byref(info), coef_ptr, comment,
                                                                                         comment_len, out, cap, n), guess,
                            "icelk_jpeg_encode_coefficients", self._h)

    def jpeg_resave_bytes(self, rgb, quality=75, comment=None):
        """`jpeg.resave_bytes` on the device: forward transform (the coefficients come back too; this is the form for
        tests and single images -- the uploads with `resave=` followed by `jpeg_resave_file` move only the file)."""
        a = np.ascontiguousarray(rgb)
        info = _lib.JpegInfo()
        args = (_u8(a), a.shape[1], a.shape[0], a.strides[0], int(quality))
        self._ck(self._lib.icelk_jpeg_resave_coefficients_host(*args, C.byref(info), None, 0))
        coef = np.empty(int(info.coef_count), np.int16)
        self._ck(self._lib.icelk_jpeg_resave_device_coefficients(self._h, *args, C.c_void_p(coef.ctypes.data), coef.size))
        return self.jpeg_resave_file(comment)

    def jpeg_resave_device_coefficients(self, rgb, quality=75):
        """The coefficients `jpeg.resave_coefficients(rgb, quality).coef` as the device's forward kernel makes them, for tests."""
        a = np.ascontiguousarray(rgb)
        coef = np.empty(resave_coefficients(a, quality).coef.size, np.int16)
        self._ck(self._lib.icelk_jpeg_resave_device_coefficients(self._h, _u8(a), a.shape[1], a.shape[0], a.strides[0], int(quality),
                                                                 C.c_void_p(coef.ctypes.data), coef.size))
        return coef

    def jpeg_device_coefficients(self, data):
        """The quantised DCT coefficients of a JPEG file as the device decodes them (`read_jpeg(data).coef`), for tests."""
        data = bytes(data)
        coef = np.empty(int(describe_jpeg(data).coef_count), np.int16)
        self._ck_jpeg(self._lib.icelk_jpeg_device_coefficients(self._h, data, len(data), C.c_void_p(coef.ctypes.data), coef.size))
        return coef

    def jpeg_huff_config(self, subseq_bits=512, max_hops=256, max_rounds=8):
        """Bits per decoder lane (a multiple of 32) and the work bound of the device's Huffman decoder: a file that needs
        more is decoded by the host decoder inside the same call (`jpeg_huff_stats()["fallback"]` says so)."""
        self._ck(self._lib.icelk_jpeg_huff_config(self._h, int(subseq_bits), int(max_hops), int(max_rounds)))

    def jpeg_huff_stats(self):
        """Of the file decoded last: segments, subsequences, rounds, max_hops, total_hops, lanes_in_step, spanning_blocks,
        fallback (0: none, 1: work bound, 2: a stream that contradicts itself, 3: size)."""
        st = _lib.JpegHuffStats()
        self._ck(self._lib.icelk_jpeg_huff_stats(self._h, C.byref(st)))
        return _stats_dict(st)

    def set_gray_device(self, slot, dev_ptr, w, h, stride):
        self._ck(self._lib.icelk_set_gray_device(self._h, slot, C.c_void_p(dev_ptr), w, h, stride))

    def cvt_bgr_device(self, slot, dev_ptr, w, h, stride, variant=GRAY_CV4):
        self._ck(self._lib.icelk_cvt_bgr_device(self._h, slot, C.c_void_p(dev_ptr), w, h, stride, variant))

    def upload_gray_async(self, slot, pinned_ptr, w, h, stride):
        self._ck(self._lib.icelk_upload_gray_async(self._h, slot, C.c_void_p(pinned_ptr), w, h, stride))

    def host_alloc(self, nbytes):
        """Pinned host memory for `upload_gray_async` (address as int); release with `host_free`."""
        p = C.c_void_p()
        self._ck(self._lib.icelk_host_alloc(C.byref(p), int(nbytes)))
        return p.value

    def host_free(self, ptr):
        self._ck(self._lib.icelk_host_free(C.c_void_p(ptr)))

    def synth_frame(self, slot, w, h, ux=0, uy=0, seed=1234, affine=None):
        """Procedural frame on the device (bit-identical to synth.frame); `affine` = (ax, bx, ay, by) in 2^-20 px/px."""
        if affine is None:
            self._ck(self._lib.icelk_synth_frame(self._h, slot, w, h, int(ux), int(uy), int(seed)))
            return
        a = (C.c_int32 * 4)(*[int(v) for v in affine])
        self._ck(self._lib.icelk_synth_frame_affine(self._h, slot, w, h, int(ux), int(uy), int(seed), a))

    def drop_pyramid(self, slot):
        self._ck(self._lib.icelk_drop_pyramid(self._h, slot))

    def download_level(self, slot, level=0):
        w, h = C.c_int(0), C.c_int(0)
        self._ck(self._lib.icelk_download_level(self._h, slot, level, None, 0, C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value), np.uint8)
        self._ck(self._lib.icelk_download_level(self._h, slot, level, _u8(out), w.value, C.byref(w), C.byref(h)))
        return out

    def build_pyramid(self, slot, winSize=(21, 21), maxLevel=3):
        n = C.c_int(0)
        self._ck(self._lib.icelk_build_pyramid(self._h, slot, winSize[0], winSize[1], maxLevel, C.byref(n)))
        return n.value

    # -- tracker ------------------------------------------------------------------------------
    def pyrlk(self, prev_slot, next_slot, prev_pts, next_pts=None, winSize=(21, 21), maxLevel=3,
              criteria=DEFAULT_CRITERIA, flags=0, minEigThreshold=1e-4):
        p0 = np.ascontiguousarray(prev_pts, dtype=np.float32).reshape(-1, 2)
        n = p0.shape[0]
        if flags & OPTFLOW_USE_INITIAL_FLOW:
            if next_pts is None:
                raise ValueError("OPTFLOW_USE_INITIAL_FLOW needs nextPts")
            p1 = np.ascontiguousarray(next_pts, dtype=np.float32).reshape(-1, 2).copy()
            if p1.shape[0] != n:
                raise ValueError("nextPts and prevPts differ in length")
        else:
            p1 = np.zeros((n, 2), np.float32)
        st = np.zeros(n, np.uint8)
        er = np.zeros(n, np.float32)
        t, cnt, eps = _criteria(criteria)
        self._ck(self._lib.icelk_pyrlk(self._h, prev_slot, next_slot, _f32(p0), _f32(p1), _u8(st), _f32(er), n,
                                       winSize[0], winSize[1], maxLevel, t, cnt, eps, flags, minEigThreshold))
        return p1.reshape(-1, 1, 2), st.reshape(-1, 1), er.reshape(-1, 1)

    def track_fb(self, slot0, slot1, p0, winSize=(21, 21), maxLevel=3, criteria=DEFAULT_CRITERIA,
                 minEigThreshold=1e-4, fb_threshold=1.0):
        p0 = np.ascontiguousarray(p0, dtype=np.float32).reshape(-1, 2)
        n = p0.shape[0]
        out = dict(p1=np.zeros((n, 2), np.float32), p0r=np.zeros((n, 2), np.float32),
                   st_fwd=np.zeros(n, np.uint8), st_bwd=np.zeros(n, np.uint8),
                   err_fwd=np.zeros(n, np.float32), err_bwd=np.zeros(n, np.float32),
                   dist=np.zeros(n, np.float32), valid=np.zeros(n, np.uint8))
        t, cnt, eps = _criteria(criteria)
        self._ck(self._lib.icelk_track_fb(self._h, slot0, slot1, _f32(p0), n, winSize[0], winSize[1], maxLevel, t,
                                          cnt, eps, minEigThreshold, fb_threshold, _f32(out["p1"]),
                                          _f32(out["p0r"]), _u8(out["st_fwd"]), _u8(out["st_bwd"]),
                                          _f32(out["err_fwd"]), _f32(out["err_bwd"]), _f32(out["dist"]),
                                          _u8(out["valid"])))
        return out

    def fb_filter(self, p0, p0r, fb_threshold=1.0):
        """(dist, valid) of s1:329-333 for given p0 / p0r, computed by the tracker's own device function."""
        a = np.ascontiguousarray(p0, dtype=np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(p0r, dtype=np.float32).reshape(-1, 2)
        if a.shape != b.shape:
            raise ValueError("p0 and p0r differ in length")
        n = a.shape[0]
        dist, valid = np.zeros(n, np.float32), np.zeros(n, np.uint8)
        self._ck(self._lib.icelk_fb_filter(self._h, _f32(a), _f32(b), n, float(fb_threshold), _f32(dist), _u8(valid)))
        return dist, valid

    # -- detector -----------------------------------------------------------------------------
    def set_mask(self, mask):
        if mask is None:
            self._ck(self._lib.icelk_set_mask(self._h, None, 0, 0, 0))
            return
        m = _gray2d(mask, "mask")
        self._ck(self._lib.icelk_set_mask(self._h, _u8(m), m.shape[1], m.shape[0], m.strides[0]))

    def set_mask_polygon(self, poly, crop_left, crop_top, w, h):
        """The mask of s1:285-291 rasterised on the device from `maskpoly` (camtools.py:184-211)."""
        p = np.ascontiguousarray(poly, dtype=np.float64).reshape(-1, 2)
        self._ck(self._lib.icelk_set_mask_polygon(self._h, p.ctypes.data_as(_lib.f64p), len(p), float(crop_left),
                                                  float(crop_top), int(w), int(h)))

    def download_mask(self):
        w, h = C.c_int(0), C.c_int(0)
        self._ck(self._lib.icelk_download_mask(self._h, None, 0, C.byref(w), C.byref(h)))
        m = np.empty((h.value, w.value), np.uint8)
        self._ck(self._lib.icelk_download_mask(self._h, _u8(m), w.value, C.byref(w), C.byref(h)))
        return m

    def min_eig_map(self, slot, blockSize=3):
        lvl = self.download_level(slot, 0)
        out = np.empty(lvl.shape, np.float32)
        self._ck(self._lib.icelk_min_eig_map(self._h, slot, blockSize, _f32(out), out.shape[1]))
        return out

    def harris_map(self, slot, blockSize=3, k=0.04):
        """cv2.cornerHarris(frame, blockSize, 3, k) of the slot (icelk_harris_map).  k is this call's own: the detector
        setting of the handle is neither read nor changed."""
        lvl = self.download_level(slot, 0)
        out = np.empty(lvl.shape, np.float32)
        self._ck(self._lib.icelk_harris_map(self._h, slot, int(blockSize), float(k), _f32(out), out.shape[1]))
        return out

    # -- which response the detector ranks by ---------------------------------------------------
    def set_detector(self, harris=False, k=0.04):
        """cv2.goodFeaturesToTrack's useHarrisDetector / k for every detection enqueued from now on (icelk_set_detector).
        harris=False: the smaller eigenvalue (Shi-Tomasi, the default; k is kept and not read).  A detection in flight,
        and candidates prepared ahead, keep the detector they were enqueued under."""
        self._ck(self._lib.icelk_set_detector(self._h, 1 if harris else 0, float(k)))

    def get_detector(self):
        """(harris, k) as set_detector left them."""
        kind, k = C.c_int(0), C.c_double(0)
        self._ck(self._lib.icelk_get_detector(self._h, C.byref(kind), C.byref(k)))
        return bool(kind.value), k.value

    @contextlib.contextmanager
    def _detector_for_call(self, useHarrisDetector, k):
        """The keyword arguments useHarrisDetector / k of the detector calls.  None (the default): the call runs under
        set_detector's setting.  True / False: the Harris response with this k / the smaller eigenvalue for the candidate
        stage the call enqueues -- the library snapshots the setting there -- and the handle's own setting is back when the
        call returns."""
        if useHarrisDetector is None:
            yield
            return
        before = self.get_detector()
        self.set_detector(bool(useHarrisDetector), k if useHarrisDetector else before[1])
        try:
            yield
        finally:
            self.set_detector(*before)

    def good_features(self, slot, maxCorners, qualityLevel, minDistance, use_mask=False, blockSize=3,
                      useHarrisDetector=None, k=0.04):
        cap = self.max_pts if maxCorners <= 0 else min(int(maxCorners), self.max_pts)
        out = np.empty((max(cap, 1), 2), np.float32)
        n = C.c_int(0)
        with self._detector_for_call(useHarrisDetector, k):
            self._ck(self._lib.icelk_good_features(self._h, slot, 1 if use_mask else 0, int(maxCorners),
                                                   float(qualityLevel), float(minDistance), int(blockSize), _f32(out), cap,
                                                   C.byref(n)))
        if n.value == 0:
            return None
        return out[:n.value].reshape(-1, 1, 2).copy()

    def detect_fast_stats(self, w, h):
        out = (C.c_longlong * 8)()
        self._ck(self._lib.icelk_detect_fast_stats(self._h, int(w), int(h), out))
        return dict(tiles=out[0], listed=out[1], whole_tiles=out[2], ties=out[3], max_listed=out[4], max_overflow_tiles=out[5],
                    longest_list=out[6], evaluated=out[7])

    def detect_max_key(self):
        """The masked maximum of the eigenvalue map as the latest detection published it: its order-preserving key."""
        k = C.c_uint(0)
        self._ck(self._lib.icelk_detect_max_key(self._h, C.byref(k)))
        return k.value

    def detect_stats(self):
        a, b = C.c_int(0), C.c_int(0)
        self._ck(self._lib.icelk_detect_stats(self._h, C.byref(a), C.byref(b)))
        return dict(candidates=a.value, accepted=b.value)

    # -- device-resident segment state ----------------------------------------------------------
    def seg_detect(self, slot, maxCorners, qualityLevel, minDistance, use_mask=False, blockSize=3,
                   useHarrisDetector=None, k=0.04):
        n = C.c_int(0)
        with self._detector_for_call(useHarrisDetector, k):
            self._ck(self._lib.icelk_seg_detect(self._h, slot, 1 if use_mask else 0, int(maxCorners), float(qualityLevel),
                                                float(minDistance), int(blockSize), C.byref(n)))
        return n.value

    def build_pyramid_ahead(self, slot, winSize=(21, 21), maxLevel=3):
        self._ck(self._lib.icelk_build_pyramid_ahead(self._h, slot, winSize[0], winSize[1], maxLevel))

    def seg_detect_prepare(self, slot, use_mask=False, blockSize=3, useHarrisDetector=None, k=0.04):
        with self._detector_for_call(useHarrisDetector, k):
            self._ck(self._lib.icelk_seg_detect_prepare(self._h, slot, 1 if use_mask else 0, int(blockSize)))

    def seg_detect_begin(self, slot, maxCorners, qualityLevel, minDistance, use_mask=False, blockSize=3,
                         useHarrisDetector=None, k=0.04):
        with self._detector_for_call(useHarrisDetector, k):
            self._ck(self._lib.icelk_seg_detect_begin(self._h, slot, 1 if use_mask else 0, int(maxCorners),
                                                      float(qualityLevel), float(minDistance), int(blockSize)))

    def seg_detect_finish(self, maxCorners):
        n = C.c_int(0)
        self._ck(self._lib.icelk_seg_detect_finish(self._h, int(maxCorners), C.byref(n)))
        return n.value

    def seg_detect_stage(self, maxCorners):
        n = C.c_int(0)
        self._ck(self._lib.icelk_seg_detect_stage(self._h, int(maxCorners), C.byref(n)))
        return n.value

    def seg_detect_stage_try(self, maxCorners):
        """icelk_seg_detect_stage_try: the corner count once the oldest detection in flight is through, else None (no wait)."""
        n, done = C.c_int(0), C.c_int(0)
        self._ck(self._lib.icelk_seg_detect_stage_try(self._h, int(maxCorners), C.byref(n), C.byref(done)))
        return n.value if done.value else None

    def seg_detect_cancel(self):
        """Abandon detections begun / prepared / staged ahead and never used (icelk_seg_detect_cancel)."""
        self._ck(self._lib.icelk_seg_detect_cancel(self._h))

    def seg_switch(self):
        self._ck(self._lib.icelk_seg_switch(self._h))

    def seg_track(self, slot_prev, slot_next, winSize=(21, 21), maxLevel=3, criteria=DEFAULT_CRITERIA,
                  minEigThreshold=1e-4, fb_threshold=1.0, wait=True):
        t, cnt, eps = _criteria(criteria)
        if wait:
            n = C.c_int(0)
            self._ck(self._lib.icelk_seg_track(self._h, slot_prev, slot_next, winSize[0], winSize[1], maxLevel, t, cnt,
                                               eps, minEigThreshold, fb_threshold, C.byref(n)))
            return n.value
        self._ck(self._lib.icelk_seg_track_async(self._h, slot_prev, slot_next, winSize[0], winSize[1], maxLevel, t,
                                                 cnt, eps, minEigThreshold, fb_threshold))
        return None

    def seg_track_defer(self, slot_prev, slot_next, winSize=(21, 21), maxLevel=3, criteria=DEFAULT_CRITERIA,
                        minEigThreshold=1e-4, fb_threshold=1.0):
        """The last pair of a segment: nothing is launched, the pair goes out together with the first pair of the next
        segment (one tracker launch for both) -- see icelk_seg_track_defer in include/icelk.h."""
        t, cnt, eps = _criteria(criteria)
        self._ck(self._lib.icelk_seg_track_defer(self._h, slot_prev, slot_next, winSize[0], winSize[1], maxLevel, t,
                                                 cnt, eps, minEigThreshold, fb_threshold))

    def seg_flush(self):
        self._ck(self._lib.icelk_seg_flush(self._h))

    def seg_template_stats(self):
        """(pairs whose forward pass took the templates of the pair before, pairs that left templates) -- diagnostics."""
        out = (C.c_longlong * 2)()
        self._ck(self._lib.icelk_seg_template_stats(self._h, out))
        return int(out[0]), int(out[1])

    def seg_template_info(self):
        """(bytes of one template table, tracks it has room for, state: 0 in use / 1 switched off / 2 allocation failed)."""
        by, rows, st = C.c_longlong(0), C.c_longlong(0), C.c_int(0)
        self._ck(self._lib.icelk_seg_template_info(self._h, C.byref(by), C.byref(rows), C.byref(st)))
        return int(by.value), int(rows.value), int(st.value)

    def seg_tail_stats(self):
        """(segments staged by the device-driven detection tail, segments staged by the host's tail) -- diagnostics."""
        out = (C.c_longlong * 2)()
        self._ck(self._lib.icelk_seg_tail_stats(self._h, out))
        return int(out[0]), int(out[1])

    def seg_track_len_hint(self, track_len):
        """Pairs per segment of the driving loop (0: unknown); lets the last pair of a segment skip leaving templates for a
        successor that never comes (icelk_seg_track_len_hint).  Results do not depend on it."""
        self._ck(self._lib.icelk_seg_track_len_hint(self._h, int(track_len)))

    def seg_live(self):
        n, tot = C.c_int(0), C.c_int64(0)
        self._ck(self._lib.icelk_seg_live(self._h, C.byref(n), C.byref(tot)))
        return n.value, tot.value

    def seg_archive(self, dev_tracks_ptr, dev_quality_ptr, dev_count_ptr, cap_rows, closed=False):
        """Gather the current segment's surviving tracks (`closed`: those of the segment the latest switch closed) into
        device memory of the caller (no wait); returns the vertex count the rows have."""
        nv = C.c_int(0)
        fn = self._lib.icelk_seg_archive_closed if closed else self._lib.icelk_seg_archive
        self._ck(fn(self._h, C.c_void_p(dev_tracks_ptr), C.c_void_p(dev_quality_ptr or 0),
                                             C.c_void_p(dev_count_ptr), int(cap_rows), C.byref(nv)))
        return nv.value

    def seg_read(self, closed=False):
        """(tracks (n, V, 2) f32, trackquality (n, V-1) f32): what np.savez stores at s1:394-395.  `closed`: of the
        segment the latest switch closed instead of the current one."""
        n, nv = C.c_int(0), C.c_int(0)
        fn = self._lib.icelk_seg_read_closed if closed else self._lib.icelk_seg_read
        self._ck(fn(self._h, None, None, 0, 0, C.byref(n), C.byref(nv)))
        tracks = np.zeros((n.value, nv.value, 2), np.float32)
        quality = np.zeros((n.value, max(nv.value - 1, 0)), np.float32)
        if n.value:
            self._ck(fn(self._h, _f32(tracks), _f32(quality), n.value, nv.value, C.byref(n),
                                              C.byref(nv)))
        return tracks, quality

    # -- camera shake fitted to land anchors (stabilize.py) ---------------------
    def stab_set_anchor_mask(self, anchor_mask):
        """The anchor mask of `seg_stabilize` (non-zero = static ground): uploaded once, resident until replaced or released
        (None).  icelk_stab_set_anchor_mask."""
        _stab.set_anchor_mask(self, anchor_mask)

    def seg_stabilize(self, closed=False, **params):
        """`seg_read` with the stabilisation in between (icelk_seg_stab_read): the segment's rows are flagged from the
        resident anchor mask, the camera's motion is fitted to the anchors and every row is corrected, on the device.
        Returns the dict of `stabilize.stabilize_tracks` plus `trackquality`.  IcelkError (ICELK_ESTATE) without a mask."""
        return _stab.seg_stabilize(self, closed, **params)

    # -- the picture of a segment (s1:397-434) --------------------------------------------------
    def _plot_call(self, slot, width, want_rgb, call, what):
        """call(rgb pointer, rgb stride, out, capacity, byref(len)) -> rc; the file's bytes, with the R G B if asked for"""
        w, h = C.c_int(0), C.c_int(0)
        if want_rgb:
            self._ck(self._lib.icelk_download_level(self._h, int(slot), 0, None, 0, C.byref(w), C.byref(h)))
        rgb, rgb_ptr, stride = _rgb_out(want_rgb, *(plot_size(w.value, h.value, width) if want_rgb else (0, 0)))
        data = _file_call(self._guesses, "plot", lambda out, cap, n: call(rgb_ptr, stride, out, cap, n), what, self._h)
        return (data, rgb) if want_rgb else data

    def plot_tracks(self, slot, tracks, width=PLOT_WIDTH, stamp="", quality=PLOT_QUALITY, want_rgb=False):
        """The picture of the frame in `slot` with `tracks` (n, vertices, 2) drawn on it -- red lines, a red dot at every
        track's end, `stamp` in a corner -- `width` pixels wide, as the bytes of a JPEG file (icelk_plot_tracks; the rules
        are DESIGN.md 7.6).  Rasterised and coded on the device; the file is what `Image.fromarray(rgb).save(f, "JPEG",
        quality=quality)` writes for the picture's R G B.  want_rgb: (bytes, that R G B (Ho, Wo, 3) uint8), for tests.
        IcelkError (code ICELK_ESTATE) for an empty slot."""
        t = _tracks3(tracks)
        text = _stamp_arg(stamp)
        return self._plot_call(slot, width, want_rgb, lambda rgb, stride, out, cap, n: self._lib.icelk_plot_tracks(
            self._h, int(slot), _f32(t), t.shape[0], t.shape[1], int(width), text, int(quality), rgb, stride, out, cap, n), "icelk_plot_tracks")

    def seg_plot(self, slot, closed=False, width=PLOT_WIDTH, stamp="", quality=PLOT_QUALITY, want_rgb=False):
        """`plot_tracks` with the surviving tracks of the current segment (`closed`: of the segment the latest switch
        closed), gathered on the device: no track data crosses PCIe (icelk_seg_plot)."""
        text = _stamp_arg(stamp)
        return self._plot_call(slot, width, want_rgb, lambda rgb, stride, out, cap, n: self._lib.icelk_seg_plot(
            self._h, int(slot), int(bool(closed)), int(width), text, int(quality), rgb, stride, out, cap, n, None), "icelk_seg_plot")

    # -- the velocity map of a gridded window (s3:449-465) ---------------------------------------
    def map_arrows_set(self, arrows, group=None):
        """A day's arrows (n, 5) x, y, dx, dy, speed and, if given, the group (the window, say) of each, copied to the
        device, where they stay until the next set, `map_arrows_release` or `close` (icelk_map_arrows_set): a panel with
        resident=True draws them, all or one group."""
        a, g, _, n = _resident_args(np.zeros((0, 5)) if arrows is None else arrows, group)
        self._ck(self._lib.icelk_map_arrows_set(self._h, a.ctypes.data_as(_lib.f64p), None if g is None else g.ctypes.data_as(_lib.i32p), n))

    def map_arrows_release(self):
        self._ck(self._lib.icelk_map_arrows_release(self._h))

    def map_inset_set(self, index, source, box=None):
        """Resident inset `index` (0 .. 7) of the maps' pictures, until the next set of that index, `map_inset_release` or
        `close`; returns its (tw, th).  `source`: the bytes of a JPEG file -- decoded and reduced on the device to fit
        box = (box_w, box_h) (icelk_map_inset_set_file); a file the device decoder does not take is opened with Pillow and
        reduced with `jpeg.thumbnail_host` -- or an H x W (x 3) uint8 array, reduced on the host to fit `box` (None: taken as
        it is) and uploaded (icelk_map_inset_set_pixels)."""
        if isinstance(source, (bytes, bytearray, memoryview)):
            data = bytes(source)
            if box is None:
                raise ValueError("a JPEG file needs a box to be fitted into")
            try:
                info = describe_jpeg(data)
                size = thumbnail_size(info.width, info.height, box)
                self._ck_jpeg(self._lib.icelk_map_inset_set_file(self._h, int(index), data, len(data), size[0], size[1]))
                return size
            except UnsupportedJpeg:
                import io
                from PIL import Image
                source = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        a = np.asarray(source)
        if box is not None:
            a = thumbnail_host(a, thumbnail_size(a.shape[1], a.shape[0], box))
        a = _rgb3(a if a.ndim == 3 else np.repeat(a[..., None], 3, axis=2))
        self._ck(self._lib.icelk_map_inset_set_pixels(self._h, int(index), _u8(a), a.shape[1], a.shape[0], a.strides[0]))
        return a.shape[1], a.shape[0]

    def map_inset_release(self):
        self._ck(self._lib.icelk_map_inset_release(self._h))

    def png_encode(self, rgb):
        """H x W x 3 uint8 -> the bytes of the PNG file `png.encode_png_host(rgb)` returns, with the row filters, the deflate
        block and the Adler-32 made on the device (icelk_png_encode_rgb): pixels up, file down."""
        a = _rgb3(rgb)
        args = (_u8(a), a.shape[1], a.shape[0], a.strides[0])
        from .png import png_bound
        return _encode_call(lambda out, cap, n: self._lib.icelk_png_encode_rgb(self._h, *args, out, cap, n), png_bound(a.shape[1], a.shape[0]),
                            "icelk_png_encode_rgb", self._h)

    def map_draw(self, picture, want_rgb=False, format="jpeg"):
        """The picture a dict of velocity_map describes (`velocity_map.map_picture` makes one of a window), as the bytes of a
        JPEG file (icelk_map_draw; the rules are DESIGN.md 7.7) or, with format="png", of a PNG file that decodes to exactly
        the picture's R G B (icelk_map_draw_png, DESIGN.md 7.9: the quality is ignored, everything else below holds).  With picture["insets"] = [dict(index=, at=(x0, y0),
        label=(px, py, text) | None)] the resident thumbnails of `map_inset_set` are pasted in, each with its label
        (icelk_map_draw_insets); without the key, or with an empty list, the call is icelk_map_draw's.  Rasterised and coded on the device; the file is what
        `Image.fromarray(rgb).save(f, "JPEG", quality=quality)` writes for the picture's R G B.  want_rgb: (bytes, that
        R G B (height, width, 3) uint8), for tests.  IcelkError (code ICELK_ESTATE) when a panel draws the resident arrows
        and none are set."""
        if format not in ("jpeg", "png"):
            raise ValueError("format is 'jpeg' or 'png'")
        d, keep = map_descriptor(picture)
        rgb, rgb_ptr, stride = _rgb_out(want_rgb, max(d.width, 1), max(d.height, 1))
        insets, n_insets = map_inset_array(picture["insets"]) if picture.get("insets") else (None, 0)
        if format == "png":
            fn, what, head = self._lib.icelk_map_draw_png, "icelk_map_draw_png", (insets, n_insets)
        elif n_insets:
            fn, what, head = self._lib.icelk_map_draw_insets, "icelk_map_draw_insets", (insets, n_insets)
        else:
            fn, what, head = self._lib.icelk_map_draw, "icelk_map_draw", ()
        data = _file_call(self._guesses, "map_" + format, lambda out, cap, n: fn(self._h, C.byref(d), *head, rgb_ptr, stride, out, cap, n),
                          what, self._h)
        del keep   # what the descriptor points into: alive until the call has returned
        return (data, rgb) if want_rgb else data

    # -- the movie of the pictures (s1:452-473, s3:194-215) -------------------------------------
    def resize_rgb(self, rgb, size):
        """H x W x 3 uint8 -> its (oh, ow, 3) resampling to size = (ow, oh), larger or smaller, on the device
        (icelk_resize_rgb): pixels up, pixels down.  Equal to `movie.resize_host`, that is to Pillow's
        `Image.fromarray(rgb).resize(size, Image.BICUBIC)`."""
        a = _rgb3(rgb)
        ow, oh = (int(v) for v in size)
        out = np.empty((max(oh, 1), max(ow, 1), 3), np.uint8)
        self._ck(self._lib.icelk_resize_rgb(self._h, _u8(a), a.shape[1], a.shape[0], a.strides[0], ow, oh, _u8(out), out.strides[0]))
        return out

    def picture_size(self):
        """(width, height) of the handle's most recent picture (`plot_tracks`, `seg_plot`, `map_draw`); IcelkError (code
        ICELK_ESTATE) when it has drawn none."""
        w, h = C.c_int(0), C.c_int(0)
        self._ck(self._lib.icelk_picture_size(self._h, C.byref(w), C.byref(h)))
        return w.value, h.value

    def picture_frame(self, size, quality=90, want_rgb=False):
        """The movie frame of the handle's most recent picture: its R G B, still on the device, resized to size = (ow, oh)
        and coded there, as the bytes of a JPEG file (icelk_picture_frame) -- what
        `Image.fromarray(rgb).resize(size, Image.BICUBIC).save(f, "JPEG", quality=quality)` writes for the picture's R G B.
        want_rgb: (bytes, the frame's R G B (oh, ow, 3) uint8), for tests.  IcelkError (code ICELK_ESTATE) when the handle
        has drawn no picture."""
        ow, oh = (int(v) for v in size)
        rgb, rgb_ptr, stride = _rgb_out(want_rgb, max(ow, 1), max(oh, 1))
        self._guesses.setdefault("frame", FRAME_FIRST_GUESS)
        data = _file_call(self._guesses, "frame", lambda out, cap, n: self._lib.icelk_picture_frame(
            self._h, ow, oh, int(quality), rgb_ptr, stride, out, cap, n), "icelk_picture_frame", self._h)
        return (data, rgb) if want_rgb else data

    # -- the orthophoto --------------------------------------------------------
    def ortho_begin(self, raster, max_range=0.0, sampling="bilinear", fill=(255, 255, 255)):
        """Begins a mosaic on `raster` (a dict of `orthophoto.ortho_raster`, or (x0, y0, res, width, height)): every pixel
        the fill colour, seen by no camera (icelk_ortho_begin).  One mosaic is in progress per Context, in the picture
        writer's R G B: drawing another kind of picture ends it."""
        r, o = raster_struct(raster), opts_struct(max_range, sampling, fill)
        self._ck(self._lib.icelk_ortho_begin(self._h, C.byref(r), C.byref(o)))
        self._ortho_size = (r.width, r.height)

    def ortho_add(self, camera, index, source):
        """Adds a camera's photograph to the mosaic under `index` (0 .. 254): where the camera sees a pixel from nearer
        than every camera added so far, the pixel takes its sample (k_ortho_add).  `source`: the bytes of a JPEG file or a
        path to one (decoded on the device; `UnsupportedJpeg` for a file its decoder refuses), an (h, w) or (h, w, 3) uint8
        array, or ("slot", k)."""
        cam = camera.struct()
        if isinstance(source, tuple) and len(source) == 2 and source[0] == "slot":
            self._ck(self._lib.icelk_ortho_add_slot(self._h, C.byref(cam), int(index), int(source[1])))
            return
        a = _source_array(source)
        if a is not None:
            self._ck(self._lib.icelk_ortho_add_pixels(self._h, C.byref(cam), int(index), a.ctypes.data, a.shape[1], a.shape[0],
                                                      1 if a.ndim == 2 else 3, a.strides[0]))
            return
        data = _source_bytes(source)
        if data is None:
            raise ValueError("a source is JPEG bytes, a path, a uint8 array or ('slot', k)")
        self._ck_jpeg(self._lib.icelk_ortho_add_jpeg_file(self._h, C.byref(cam), int(index), data, len(data)))

    def ortho_write(self, format=None, quality=90):
        """The mosaic as dict(rgb (height, width, 3) uint8, cover (height, width) uint8, file): `file` the bytes of a PNG
        ("png": exactly the pixels) or of a JPEG ("jpeg": what `Image.fromarray(rgb).save(f, "JPEG", quality=quality)`
        writes), coded on the device by the picture writer (icelk_ortho_write); None with format=None.  The mosaic stays:
        further cameras can be added and it can be written again."""
        if format is not None and format not in ORTHO_FORMATS:
            raise ValueError("format is None, 'jpeg' or 'png'")
        if self._ortho_size is None:
            raise _lib.IcelkError("icelk error %d: no orthophoto has been begun (ortho_begin)" % _lib.ESTATE)
        w, h = self._ortho_size
        rgb, cover = np.empty((h, w, 3), np.uint8), np.empty((h, w), np.uint8)

        def call(out, cap, n):
            return self._lib.icelk_ortho_write(self._h, ORTHO_FORMATS[format or "png"], int(quality), _u8(rgb), rgb.strides[0],
                                               _u8(cover), cover.strides[0], out, cap, n)
        if format is None:
            # no file wanted: none is offered room, and "it takes *len bytes" is the expected answer
            n = C.c_uint64(0)
            rc = call(None, 0, C.byref(n))
            if rc != _lib.ECAP:
                self._ck(rc)
            return dict(rgb=rgb, cover=cover, file=None)
        self._guesses.setdefault("ortho_" + format, ORTHO_FIRST_GUESS)
        data = _file_call(self._guesses, "ortho_" + format, call, "icelk_ortho_write", self._h)
        return dict(rgb=rgb, cover=cover, file=data)

    # -- measurement ----------------------------------------------------------------------------
    def prof_enable(self, on=True):
        """on: False / True (every kernel) / 2 (tracker launches only: the other streams carry no event records)."""
        self._ck(self._lib.icelk_prof_enable(self._h, int(on)))

    def prof_reset(self):
        self._ck(self._lib.icelk_prof_reset(self._h))

    def prof_iterations(self):
        """(forward, backward) LK iteration counts per feature of the latest tracker call made while profiling was on;
        tracks that were already dead are left out."""
        n = C.c_int(0)
        self._ck(self._lib.icelk_prof_iterations(self._h, None, 0, C.byref(n)))
        buf = np.zeros(max(n.value, 1), np.uint32)
        if n.value:
            self._ck(self._lib.icelk_prof_iterations(self._h, buf.ctypes.data_as(C.POINTER(C.c_uint32)), n.value,
                                                     C.byref(n)))
        buf = buf[:n.value]
        buf = buf[buf != 0xffffffff]
        return (buf & 0xffff).astype(np.int64), (buf >> 16).astype(np.int64)

    def stream_probe_info(self):
        """Which hardware queues the side streams of this handle landed on (icelk_stream_probe_info)."""
        picks = (C.c_int * 4)()
        q, lim = C.c_double(0), C.c_double(0)
        self._ck(self._lib.icelk_stream_probe_info(self._h, picks, C.byref(q), C.byref(lim)))
        return dict(detection=picks[0], candidates=picks[1], pyramid=picks[2], tail=picks[3], quickest=q.value,
                    limit=lim.value, probed=picks[0] >= 0)

    def prof_table(self):
        out = {}
        for k in range(self._lib.icelk_prof_count()):
            n, ms = C.c_int(0), C.c_double(0)
            self._ck(self._lib.icelk_prof_get(self._h, k, C.byref(n), C.byref(ms)))
            if n.value:
                out[self._lib.icelk_prof_name(k).decode()] = dict(launches=n.value, total_ms=ms.value,
                                                                  avg_us=1e3 * ms.value / n.value)
        return out
