"""The reference's crop step on its own: `cam.crop_image_parallel(imagelist, targetworkspace)` (camtools.py:64-104,
237-258, called at s1:272) opens every photo, crops it and saves it again as a JPEG into the day's target folder, which
the tracker, s3's plots and the movies then read.  `crop_image_sequence` writes that folder, byte for byte, with the
work on the device: a photo is one crop job (`Context.jpeg_crop_start` / `jpeg_crop_finish`, csrc/abi_jpeg_crop.hip on csrc/abi_jpeg_job.hip) --
Huffman decoding, inverse DCT, the crop box, the lossy re-save and the entropy coder enqueued in one piece, the coder's
sizes left on the device -- and only the finished file comes back.

The folder can then be tracked as often as wanted, the reference's way and on the fast driver:

    cropped = [p for p, _, _ in crop_image_sequence(photos, target, crop=box)]
    track_image_sequence(cropped, out, ..., decoder="device", huffman="device", pipeline=True,
                         mask_polygon=(poly, box[0], box[1]))

The cropped files are baseline, 4:2:0, with the standard Huffman tables: exactly what the device decoder takes, and
opening one gives the re-saved pixels bit for bit -- what `track_image_sequence(photos, crop=box, resave="reference")`
tracks on.
"""
import os
import threading
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .jpeg import REFERENCE_RESAVE_QUALITY, describe_jpeg, resave_bytes, resave_quality, source_comment

_TRUNCATED_LOCK = threading.Lock()   # PIL.ImageFile.LOAD_TRUNCATED_IMAGES is one flag for the whole process


def _crop_box(size, crop):
    """Pillow's box of `img.crop` for (left, top, right, bottom) pixels to drop (camtools.py:77-80)"""
    left, top, right, bottom = (0, 0, 0, 0) if crop is None else (int(v) for v in crop)
    width, height = size
    return left, top, width - right, height - bottom


def pil_crop_image(path, crop):
    """The `"pil"` route's open-and-crop: `Image.open(path).crop(box)`, loaded.  A file Pillow refuses as truncated is
    opened once more with truncated loading allowed, as camtools.py:83-104 does; the process-wide flag is set for that
    load only, under a lock, and restored afterwards -- a load that another thread runs beside it without this function
    sees the flag set for that while.  An error of the file system (no such file, no permission: an OSError with an
    errno) is not Pillow's complaint about the data and is raised as it is."""
    from PIL import Image, ImageFile

    def load():
        im = Image.open(path)
        im = im.crop(_crop_box(im.size, crop))            # loads the photo; the crop keeps its `info` (the comment)
        im.load()
        return im
    try:
        return load()
    except OSError as e:
        if e.errno is not None:                           # the file system's, not Pillow's "image file is truncated"
            raise
        with _TRUNCATED_LOCK:
            before = ImageFile.LOAD_TRUNCATED_IMAGES
            ImageFile.LOAD_TRUNCATED_IMAGES = True
            try:
                return load()
            finally:
                ImageFile.LOAD_TRUNCATED_IMAGES = before


def pil_crop_file(path, crop, quality, ctx=None):
    """One photo by the `"pil"` route: Pillow decodes and crops (`pil_crop_image`), `jpeg.resave_bytes` writes the crop's
    file -- on the device with a Context, on the host without; the bytes are the same.  A photo that is not R G B (one
    component, CMYK) is saved by Pillow itself, as the reference does: the writer here makes three-component files."""
    im = pil_crop_image(path, crop)
    if im.mode != "RGB":
        import io
        f = io.BytesIO()
        im.save(f, "JPEG", quality=quality)
        return f.getvalue()
    rgb = np.array(im)
    if ctx is not None and rgb.shape[1] < 3:              # the device's forward kernel takes widths from 3
        ctx = None
    return resave_bytes(rgb, quality, im.info.get("comment"), ctx)


def _read(path):
    """What a reader thread makes of one photo: (its bytes or None, its comment).  None: the device decoder does not take
    the file (progressive, CMYK, one component, unparsable, ...) and PIL will."""
    with open(path, "rb") as f:
        data = f.read()
    try:
        if describe_jpeg(data).ncomp == 3:
            return data, source_comment(data)
    except ValueError:                                    # UnsupportedJpeg is one
        pass
    return None, None


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def crop_image_sequence(imagelist, target_dir, crop=None, quality="reference", device=0, read_threads=4, write_threads=2,
                        in_flight=4, ctx=None):
    """Writes `target_dir/<basename>` for every photo of `imagelist`: byte for byte the file
    `Image.open(p).crop(box).save(out)` writes (crop_image_standalone of the reference), the source's comment carried
    over.  Returns [(path written, its bytes, route)] in list order.

    crop           (left, top, right, bottom) of the calibration workbook (camtools.py:147-150) or None
    quality        "reference" (Pillow's default, 75: the reference names none) or 1 .. 100
    read_threads   threads that only read files (and look at their headers)
    write_threads  threads that write the finished files: no file is written on the thread that talks to the device
    in_flight      crop jobs started before the oldest one is finished; each owns a working set on the device
    ctx            a Context to run on (it is left open); default: one of its own on `device`, closed at the end
    route          "device": coded on the device without a host wait; "host-huffman": the host's Huffman decoder took the
                   file; "over-budget": the coded scan was larger than `Context.jpeg_crop_config` allows and was coded
                   again with host-read sizes; "pil": a file the device decoder does not take, or a crop less than 3
                   pixels wide, went through PIL, that file only
    The reference's log file of photos that failed is not written: a photo that PIL cannot open either raises."""
    quality = resave_quality(quality)
    if quality is None:
        raise ValueError('quality must be "reference" or a JPEG quality in 1 .. 100')
    read_threads, write_threads, in_flight = int(read_threads), int(write_threads), int(in_flight)
    if in_flight < 1 or read_threads < 1 or write_threads < 1:
        raise ValueError("in_flight, read_threads and write_threads must be at least 1")
    imagelist = [str(p) for p in imagelist]
    if not imagelist:
        return []
    os.makedirs(target_dir, exist_ok=True)
    own = ctx is None
    if own:
        from .context import Context
        ctx = Context(64, 64, n_slots=2, max_pts=64, device=device)   # crop jobs use no slot and no point buffer
    out = [None] * len(imagelist)
    ahead = read_threads + in_flight
    tickets = deque()                                     # (index, ticket or None, comment) in list order
    open_tickets = set()
    try:
        with ThreadPoolExecutor(max_workers=read_threads) as readers, ThreadPoolExecutor(max_workers=write_threads) as writers:
            reads = deque(readers.submit(_read, p) for p in imagelist[:ahead])
            writes = []
            pending = deque()                             # writes handed over and not yet waited for: a few files at most

            def finish_oldest():
                k, ticket, comment = tickets.popleft()
                if ticket is None:
                    data, route = pil_crop_file(imagelist[k], crop, quality, ctx), "pil"
                else:
                    open_tickets.discard(ticket)
                    try:
                        data, stats = ctx.jpeg_crop_finish(ticket, comment)
                        route = stats["route"]
                    except ValueError:                    # what only the decoder sees of a damaged file: PIL has the word
                        data, route = pil_crop_file(imagelist[k], crop, quality, ctx), "pil"
                path = os.path.join(target_dir, os.path.basename(imagelist[k]))
                while len(pending) > write_threads + 2:   # a slow disk holds the device back, not the folder's bytes in memory
                    pending.popleft().result()
                pending.append(writers.submit(_write, path, data))
                writes.append((k, path, route, pending[-1]))

            for k in range(len(imagelist)):
                data, comment = reads.popleft().result()
                if k + ahead < len(imagelist):
                    reads.append(readers.submit(_read, imagelist[k + ahead]))
                ticket = None
                if data is not None:
                    try:
                        ticket = ctx.jpeg_crop_start(data, crop, quality)
                        open_tickets.add(ticket)
                    except ValueError:                    # unsupported, damaged, or a crop too narrow: PIL has the word
                        ticket = None
                tickets.append((k, ticket, comment))
                if len(tickets) >= in_flight:
                    finish_oldest()
            while tickets:
                finish_oldest()
            for k, path, route, done in writes:
                out[k] = (path, done.result(), route)
    finally:
        for ticket in open_tickets:
            try:
                ctx.jpeg_crop_cancel(ticket)
            except Exception:                             # noqa: BLE001 -- the first error is the one to report
                pass
        if own:
            ctx.close()
    return out


__all__ = ["crop_image_sequence", "pil_crop_file", "pil_crop_image", "REFERENCE_RESAVE_QUALITY"]
