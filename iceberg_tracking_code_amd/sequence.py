"""One folder of time-lapse photographs -> track files: the body of `lucaskanade_tracking` in the reference
(s1_lucaskanade_tracking.py:234-450) with the frame loop on the GPU.

What the reference does per day folder: crop every photo with PIL and save it again as JPEG (s1:272,
camtools.py:64-104), list the cropped copies, build the fjord mask (s1:285-294), then for every `start` offset walk
the list: decode (s1:310), cvtColor (s1:311), track / filter / extend (s1:313-359), at every `track_len`-th frame
check the time gaps and save the segment (s1:362-395), detect new corners (s1:437-448).

Here: a small thread pool decodes ahead on the host -- the real end-to-end bound, far slower than the GPU step.  With
`decoder="pil"` (default) it decodes whole photos with PIL and the crop box is cut during the upload of the decoded
frame (`Context.upload_bgr(crop=...)`); with `decoder="device"` the pool only Huffman-decodes (`jpeg.read_jpeg`) and
the device does the inverse DCT, chroma upsampling, colour conversion, crop and gray (`Context.upload_jpeg`), giving
the same pixels; files the device decoder does not take go through PIL one by one.  With `huffman="device"` on top
the pool only reads the files and the device Huffman-decodes them as well (`Context.upload_jpeg_file`); with
`pipeline=True` on top of that the files are decoded ahead of their frame, beside the tracker steps of the frames in
front of them (`SegmentTracker.prefetch_jpeg`).  Either way
pixel values are those of the original photo unless `resave` asks for the reference's lossy re-save of the crop, which
then runs on the device between crop and gray conversion (csrc/k_jpeg_fwd.hip; with `pipeline=True` as part of the job
that decodes the file ahead, `resave_ahead=True`); gray conversion, detection,
tracking, filtering and the track table are the device-resident loop of `SegmentTracker`; the mask is rasterised on
the device from the polygon (`icelk_set_mask_polygon`) or uploaded.  Output files carry the reference's names and
arrays.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .movie import open_movie, tracks_movie_name
from .plot import PLOT_QUALITY, PLOT_WIDTH, plot_name, plot_stamp
from .tracker import REF_FEATURE_PARAMS, REF_LK_PARAMS, SegmentTracker, npz_name, save_tracks, segment_time_ok


def _load(path, kind, with_comment):
    """What a pool thread makes of one photo.  kind "pixels": `np.array(Image.open(path))` (s1:310; RGB order, cvtColor is
    asked for BGR2GRAY).  "coefficients" (decoder="device"): the host stage only, `jpeg.read_jpeg`.  "bytes"
    (huffman="device" on top): the file as it is, its headers looked at.  A file the device decoder does not take
    (progressive, CMYK, gray, ...) or cannot parse is decoded by PIL instead -- that file only; PIL then also is the one to
    complain about a broken file.  with_comment: (frame, the photo's comment), Pillow's `im.info.get("comment")`, which
    `crop().save()` carries into the crop's file."""
    if kind != "pixels":
        from .jpeg import describe_jpeg, read_jpeg, source_comment
        try:
            with open(path, "rb") as f:
                data = f.read()
            frame = read_jpeg(data) if kind == "coefficients" else data
            if (frame.ncomp if kind == "coefficients" else describe_jpeg(data).ncomp) == 3:
                return (frame, source_comment(data)) if with_comment else frame
        except ValueError:                                # UnsupportedJpeg is one
            pass
    from PIL import Image
    im = Image.open(path)
    return (np.array(im), im.info.get("comment")) if with_comment else np.array(im)


def _image_size(path, decoder):
    if decoder == "device":
        from .jpeg import describe_jpeg
        try:
            with open(path, "rb") as f:
                info = describe_jpeg(f.read())
            return info.width, info.height
        except ValueError:
            pass
    first = _load(path, "pixels", False)
    return first.shape[1], first.shape[0]


# frame slots of the pipelined driver: previous and current frame plus the files decoded ahead
PIPELINE_SLOTS = 6


def track_image_sequence(imagelist, target_dir, track_len, track_len_sec, startlist=(0,), crop=None, mask=None,
                         mask_polygon=None, feature_params=None, lk_params=None, decode_threads=4, decode_ahead=6,
                         gray_variant=4, device=0, on_segment=None, save=True, decoder="pil", huffman="host", pipeline=False,
                         n_slots=PIPELINE_SLOTS, resave=None, save_crops=None, plots=None, plot_width=PLOT_WIDTH,
                         plot_quality=PLOT_QUALITY, resave_ahead=False, movie=None, anchor_mask=None, stabilize=None):
    """Track one day's photos.  Returns [(npz path, tracks (n, T+1, 2) f32, trackquality (n, T) f32)] of the
    segments that pass the time-gap rule, in order.

    imagelist      sorted photo paths named '%Y%m%d-%H%M%S.jpg' (s1:264)
    crop           (left, top, right, bottom) of the calibration workbook (camtools.py:147-150) or None
    mask           H x W uint8 array (255 = detect here), or
    mask_polygon   (maskpoly, cropleft, croptop): rasterised on the device as s1:285-291 / camtools.py:184-211 do
    feature_params cv2.goodFeaturesToTrack's keywords (default: the reference's, s1:240-244); `useHarrisDetector` (False)
                   and `k` (0.04) are among them and go with every detection, those prepared ahead included
    startlist      offsets into the list, each walked separately (s1:304)
    on_segment     optional callback(npz path, tracks, trackquality), e.g. a projection step
    decoder        "pil": photos are decoded on the host; "device": only their Huffman decoding is (see above) -- same
                   outputs, supported files and the per-file fallback are listed in INTEGRATION.md
    huffman        with decoder="device": "host" (the pool threads Huffman-decode) or "device" (they only read the file
                   and its headers; the scan is decoded on the device, `Context.upload_jpeg_file`) -- same outputs
    pipeline       with decoder="device", huffman="device": up to n_slots - 2 files are decoded ahead of their frame on
                   streams of their own (`SegmentTracker.prefetch_jpeg` / `push_prefetched`) -- same outputs
    n_slots        frame slots of the pipelined driver, at least 5
    resave         None: pixel values are those of the photos.  "reference": the tracker sees what the reference's tracker
                   sees, the crop saved by Pillow as a new JPEG (quality 75, s1:272) and opened again -- reproduced on the
                   device, no file is written; an int: that quality.  With pipeline=True only together with resave_ahead=True.
                   A file the device decoder
                   does not take goes through PIL, that file only, and is re-saved on the device all the same.  The
                   two-pass route gets the same tracks with pipeline=True: `crop.crop_image_sequence` writes the re-saved
                   crops first, and this function then runs on those files with no crop and no resave
    save_crops     with resave: a directory that receives `<basename of the photo>` for every photo ingested, the file the
                   reference's crop step writes into its target folder (`Image.open(p).crop(box).save(out)`, the source's
                   comment carried over), entropy-coded on the device (csrc/k_jpeg_enc.hip) right after the upload and
                   written on the calling thread once the photo's step is enqueued; once per photo, however many entries
                   of startlist visit it.  With pipeline=True only together with resave_ahead=True.  The tracks do not
                   change
    resave_ahead   with pipeline=True and resave: the re-save -- and with save_crops the coding of the crop's file -- is part
                   of the job that decodes a photo ahead of its frame (`SegmentTracker.prefetch_jpeg(resave=...)`,
                   icelk_upload_jpeg_file_async_resave): one pass over the photos gives the reference's tracks and its crop
                   folder.  Same outputs as pipeline=False with the same options
    plots          a directory (created) that receives, for every segment that passes the time-gap rule, the picture the
                   reference draws of it (s1:397-434): the segment's last frame `plot_width` pixels wide, its tracks as red
                   lines, their ends as red dots, '<last photo> <track_len * track_len_sec>/<track_len_sec>' in a corner --
                   rasterised and coded on the device (`SegmentTracker.plot_closed`) as
                   '<basename of the segment's last photo>_<track_len * track_len_sec>sec.jpg', the reference's name
                   (s1:429) with .jpg for .png, at JPEG quality `plot_quality`.  With every decoder / huffman / pipeline /
                   resave / save_crops combination; the returned list and the .npz files do not change.  None: nothing
                   of it runs and nothing is allocated
    movie          with plots: the movie the reference makes of the day's pictures (s1:452-473), a Motion-JPEG AVI at 8
                   frames per second and 2000 pixels wide.  Every picture written also becomes a frame, in the order
                   written, scaled and coded on the device from the pixels the picture left there (`movie.MovieWriter`,
                   DESIGN.md 7.11).  True: 'tracks_oblique_<track_len * track_len_sec>sec.avi', the reference's name, in
                   `plots`; a path: that file; a `MovieWriter`: frames are added to it and it is left open.  Without a
                   picture no file is written.  The pictures, the returned list and the .npz files do not change.  None:
                   nothing of it runs
    anchor_mask, stabilize   the opt-in stabilising stage (stabilize.py): `anchor_mask` is an H x W array of
                   the cropped frame, non-zero = static ground; `stabilize` is True or a dict of `stabilize_tracks`'
                   keywords and needs `anchor_mask`.  The camera's motion since a segment's first frame is fitted to the
                   tracks that start under the anchor mask, and every track is mapped back through it on the device
                   (`SegmentTracker(anchor_mask=, stabilize=)`).  `tracks` / `trackquality` are then saved, handed to
                   on_segment and returned WITHOUT the anchor rows, in the coordinates of the segment's first frame, so
                   that land points never reach s2; the file also holds `anchor_tracks`, `anchor_trackquality` (the anchor
                   rows, corrected like the rest) and, per vertex after the first, `camera_motion` (a, b, tx, ty),
                   `camera_inliers`, `camera_rms` and `camera_status`.  With every decoder / pipeline / resave / plots
                   combination; the segment picture keeps drawing the raw tracks, anchors included.  A detector mask becomes
                   mask OR anchor mask, and the detector's quality threshold is relative to the maximum over the joined
                   mask: the water corners can therefore differ from a run without anchors.  None: nothing of it runs
                   or is allocated, and every file is what it was
    """
    if decoder not in ("pil", "device"):
        raise ValueError('decoder must be "pil" or "device"')
    if huffman not in ("host", "device"):
        raise ValueError('huffman must be "host" or "device"')
    if huffman == "device" and decoder != "device":
        raise ValueError('huffman="device" needs decoder="device"')
    if pipeline and (decoder != "device" or huffman != "device"):
        raise ValueError('pipeline=True needs decoder="device" and huffman="device"')
    from .jpeg import resave_quality
    resave = resave_quality(resave)
    if resave_ahead and not (pipeline and resave is not None):
        raise ValueError("resave_ahead=True needs pipeline=True and resave")
    if pipeline and resave is not None and not resave_ahead:
        raise ValueError("resave is not available with pipeline=True (unless resave_ahead=True)")
    if save_crops is not None and resave is None:
        raise ValueError("save_crops needs resave: the files written are the re-saved crops")
    if save_crops is not None and pipeline and not resave_ahead:
        raise ValueError("save_crops is not available with pipeline=True (unless resave_ahead=True)")
    if pipeline and int(n_slots) < 5:
        raise ValueError("n_slots must be at least 5")
    if movie is not None and plots is None:
        raise ValueError("movie needs plots: its frames are the pictures")
    imagelist = [str(p) for p in imagelist]
    out = []
    if len(imagelist) <= track_len:                       # s1:267
        return out
    fp = dict(REF_FEATURE_PARAMS if feature_params is None else feature_params)
    lk = dict(REF_LK_PARAMS if lk_params is None else lk_params)
    w, h = _image_size(imagelist[0], decoder)
    if crop is not None:
        left, top, right, bottom = (int(v) for v in crop)
        w, h = w - left - right, h - top - bottom
    kind = ("bytes" if huffman == "device" else "coefficients") if decoder == "device" else "pixels"

    def load(path):
        return _load(path, kind, save_crops is not None)
    if save_crops is not None:
        os.makedirs(save_crops, exist_ok=True)
    if plots is not None:
        os.makedirs(plots, exist_ok=True)
    written = set()                                       # photos whose crop has been written
    trk = None
    film, film_own = (None, False) if movie is None else open_movie(movie, plots, tracks_movie_name(track_len, track_len_sec))
    try:
        with ThreadPoolExecutor(max_workers=max(1, int(decode_threads))) as pool:
            for start in startlist:
                names = imagelist[start:]
                if trk is not None:
                    trk.close()
                # a fresh loop state per start offset (the reference carries the last frame of the previous pass
                # into the first step of the next one; nothing is saved from that pair, s1:362-363)
                trk = SegmentTracker(w, h, track_len, feature_params=fp, lk_params=lk, mask=mask,
                                     mask_polygon=mask_polygon, device=device, n_slots=int(n_slots) if pipeline else 3,
                                     anchor_mask=anchor_mask, stabilize=stabilize)
                pending = [pool.submit(load, p) for p in names[:decode_ahead]]
                fed = 0                                   # pipeline=True: frames handed to the tracker's prefetch queue
                ahead_kw = {}                             # ... and the options each of those in flight was handed with
                for counter in range(len(names)):
                    if pipeline:
                        # previous and current frame stay resident, every other slot holds a frame on its way
                        while fed < len(names) and fed - counter < trk.n_slots - 2:
                            frame = pending.pop(0).result()
                            if fed + decode_ahead < len(names):
                                pending.append(pool.submit(load, names[fed + decode_ahead]))
                            kw = dict(variant=gray_variant, crop=crop)
                            if resave_ahead:
                                kw.update(resave=resave)
                            if save_crops is not None:
                                frame, comment = frame
                                if names[fed] not in written:
                                    kw.update(crop_file=os.path.join(save_crops, os.path.basename(names[fed])), comment=comment)
                                    written.add(names[fed])
                            ahead_kw[fed] = kw
                            if isinstance(frame, bytes):
                                try:
                                    trk.prefetch_jpeg(frame, **kw)
                                except ValueError:        # what the host sees of an unsupported or damaged file ...
                                    trk.prefetch_bgr(_load(names[fed], "pixels", False), **kw)
                            else:
                                trk.prefetch_bgr(frame, **kw)
                            fed += 1
                        try:
                            seg = trk.push_prefetched()
                        except ValueError:                # ... and what only the decoder sees: PIL has the word
                            trk.replace_prefetched_bgr(_load(names[counter], "pixels", False), **ahead_kw[counter])
                            seg = trk.push_prefetched()
                        del ahead_kw[counter]
                    else:
                        frame = pending.pop(0).result()
                        if counter + decode_ahead < len(names):
                            pending.append(pool.submit(load, names[counter + decode_ahead]))
                        kw = dict(variant=gray_variant, crop=crop, resave=resave)
                        if save_crops is not None:
                            frame, comment = frame
                            if names[counter] not in written:
                                kw.update(crop_file=os.path.join(save_crops, os.path.basename(names[counter])), comment=comment)
                        if isinstance(frame, bytes):
                            try:
                                seg = trk.push_jpeg(frame, **kw)
                            except ValueError:            # unsupported or damaged, that file only: PIL has the word
                                seg = trk.push_bgr(_load(names[counter], "pixels", False), **kw)
                        elif isinstance(frame, np.ndarray):
                            seg = trk.push_bgr(frame, **kw)
                        else:
                            seg = trk.push_jpeg(frame, **kw)
                        written.add(names[counter])
                    if seg is None:
                        continue
                    seg_first, tracks, quality = seg
                    seg_names = names[seg_first:seg_first + track_len + 1]
                    if not segment_time_ok(seg_names, track_len_sec):        # s1:364-390
                        continue
                    npz = os.path.join(target_dir, npz_name(os.path.basename(seg_names[0]), track_len, track_len_sec))
                    more = {}
                    if trk.stabilize is not None:
                        st = trk.last_stabilization
                        land = st["anchors"]
                        more = dict(anchor_tracks=tracks[land], anchor_trackquality=quality[land], camera_motion=st["motion"],
                                    camera_inliers=st["inliers"], camera_rms=st["rms"], camera_status=st["status"])
                        tracks, quality = tracks[~land], quality[~land]
                    if save:
                        save_tracks(npz, tracks, quality, **more)
                    if plots is not None:
                        with open(plot_name(plots, seg_names[-1], track_len, track_len_sec), "wb") as f:
                            f.write(trk.plot_closed(plot_width, plot_stamp(seg_names[-1], track_len, track_len_sec), plot_quality))
                        if film is not None:
                            film.add_picture(trk.ctx)
                    if on_segment is not None:
                        on_segment(npz, tracks, quality)
                    out.append((npz, tracks, quality))
    finally:
        if trk is not None:
            trk.close()
        if film_own:
            film.close()
    return out
