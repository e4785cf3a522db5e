"""Host-side mirror of the reference's tracking loops, driving the HIP library.

`SegmentTracker` is the loop of s1_lucaskanade_tracking.py:304-450 (s0_1_test_lucaskanade_tracking.py:77-181) with
the state resident on the GPU (slots, pyramids, live points, track table): one pyramid build per frame instead of
the four OpenCV does, one fused forward+backward launch per pair, nothing crossing PCIe except the finished
segment.  The list-of-lists form of the same loop, written against cv2-shaped functions, is test harness and
lives in tests/reference_loops.py.

Also here: the `.npz` wire format consumed by s2_cam_to_utm.py:177,197-198,233-234.
"""
import datetime as dt
import os
from contextlib import suppress
from itertools import takewhile

import numpy as np

from .context import Context, TERM_CRITERIA_COUNT, TERM_CRITERIA_EPS
from .plot import PLOT_QUALITY, PLOT_WIDTH

# parameter literals of the reference (s1:240-248, s0_1:37-45)
REF_FEATURE_PARAMS = dict(maxCorners=50000000, qualityLevel=0.007, minDistance=10, blockSize=10)
REF_LK_PARAMS = dict(winSize=(35, 35), maxLevel=4, criteria=(TERM_CRITERIA_EPS | TERM_CRITERIA_COUNT, 25, 0.03))
REF_FB_THRESHOLD = 1.0   # `valid = dist < 1` (s1:333), `self.distthreshold = 1.0` (s0_1:51)


def npz_name(first_image_path, track_len, track_len_sec):
    """'<%Y%m%d-%H%M%S>_{T*dt}sec_at_{dt}sec_tracks.npz' next to the image (s1:394)."""
    return "{}_{}sec_at_{}sec_tracks.npz".format(str(first_image_path).split(".")[0], track_len * track_len_sec,
                                                 track_len_sec)


def segment_time_ok(names, track_len_sec):
    """The +-2 s gap rule of s1:364-388 over the file names of one segment's frames."""
    times = [dt.datetime.strptime(os.path.basename(str(n)), "%Y%m%d-%H%M%S.jpg") for n in names]
    for a, b in zip(times[:-1], times[1:]):
        if (b - a).seconds not in (track_len_sec - 2, track_len_sec - 1, track_len_sec, track_len_sec + 1,
                                   track_len_sec + 2):
            return False
    return True


def save_tracks(npzname, tracks, trackquality, **more):
    """np.savez(npzname, tracks=tracks, trackquality=trackquality) (s1:395).  `more`: further arrays of the same file (the
    stabilising stage's: sequence.track_image_sequence)."""
    np.savez(npzname, tracks=tracks, trackquality=trackquality, **more)


class _Ahead:
    """A frame whose upload was started ahead of its push: its slot, whether its JPEG file is still to be finished, and the
    crop file asked for -- path, comment and, once they are there, its bytes: without them (`abort()`) nothing is written."""
    __slots__ = ("slot", "in_flight", "crop_file", "comment", "data")

    def __init__(self, slot, in_flight=False, crop_file=None, comment=None):
        self.slot, self.in_flight, self.crop_file, self.comment, self.data = slot, in_flight, crop_file, comment, None


class SegmentTracker:
    """Device-resident form of the s1 loop.  Feed frames one at a time; finished segments come back as
    (first_frame_index, tracks (n, T+1, 2) f32, trackquality (n, T) f32) -- the np.savez payload.

    Frames are given as host arrays (`push`), as device pointers (`push_device`) or generated on the
    device (`push_synth`).  Three slots rotate: previous frame, current frame, and one being uploaded.

    feature_params are cv2.goodFeaturesToTrack's: maxCorners, qualityLevel, minDistance, blockSize and, optional,
    useHarrisDetector (default False: Shi-Tomasi) and k (default 0.04; read with the Harris detector only).  They go with
    every detection the tracker starts or prepares ahead.

    anchor_mask, stabilize: the opt-in stabilising stage (stabilize.py).  `anchor_mask` is an H x W array,
    non-zero = static ground; `stabilize` is True for the default parameters or a dict of `stabilize_tracks`' keywords, and
    needs `anchor_mask`.  The tracks that start under the anchor mask are the anchors: the camera's motion since the segment's
    first frame is fitted to them and every track is mapped back through it, so the segment a push returns -- the same
    3-tuple, anchors included, all rows corrected -- is in the coordinates of its first frame (`Context.seg_stabilize` in
    place of `seg_read`); `last_stabilization` holds the rest of that call's dict (`anchors`, `motion`, `inliers`, `rms`,
    `status`, `rounds_used`, `n_anchors`).  Where a detector mask is in use it becomes mask OR anchor mask, so that corners
    are found on the anchors' ground (a `mask_polygon` is rasterised, downloaded once, joined on the host and set again).
    The detector's quality threshold is relative to the maximum response over the joined mask: the water corners can
    therefore differ from a run without anchors.  Without `stabilize` nothing of this runs or is allocated.
    """

    def __init__(self, width, height, track_len, feature_params=None, lk_params=None, mask=None, max_pts=1 << 18,
                 device=0, fb_threshold=REF_FB_THRESHOLD, ctx=None, n_slots=3, lookahead=True, mask_polygon=None,
                 pair_launch=True, anchor_mask=None, stabilize=None):
        self.track_len = int(track_len)
        if self.track_len < 1 or self.track_len > 16:
            raise ValueError("track_len must be in 1..16")
        self.fp = dict(REF_FEATURE_PARAMS if feature_params is None else feature_params)
        self.lk = dict(REF_LK_PARAMS if lk_params is None else lk_params)
        self.fb_threshold = float(fb_threshold)
        self.w, self.h = width, height
        self.stabilize, self.last_stabilization = self._stabilize_arg(stabilize, anchor_mask, width, height), None
        self.ctx = ctx if ctx is not None else Context(width, height, n_slots=n_slots, max_pts=max_pts, device=device)
        self.n_slots = self.ctx.n_slots
        self.ctx.seg_track_len_hint(track_len)    # the last pair of a segment leaves no templates behind
        self.use_mask = mask is not None or mask_polygon is not None
        if mask_polygon is not None:
            # (maskpoly, cropleft, croptop): the mask of s1:285-291 rasterised on the device (camtools.py:184-211)
            poly, crop_left, crop_top = mask_polygon
            self.ctx.set_mask_polygon(poly, crop_left, crop_top, width, height)
            if self.stabilize is not None:
                self.ctx.set_mask(self._joined(self.ctx.download_mask(), anchor_mask))
        elif mask is not None:
            self.ctx.set_mask(mask if self.stabilize is None else self._joined(mask, anchor_mask))
        if self.stabilize is not None:
            self.ctx.stab_set_anchor_mask(anchor_mask)
        self.counter = 0          # frames consumed
        self.cur = -1             # slot of the newest frame
        self.seg_first = 0
        self.active = False
        self.n_detected = 0
        self._queue = []          # frames whose upload was started ahead of time, in the order they will be pushed
        self.lookahead = bool(lookahead)
        self.pair_launch = bool(pair_launch) and self.lookahead   # see `_step`: joint launch across a segment change
        # how many steps ahead of a detection frame its min-distance stage / its corner candidates may start (`_step`)
        self.begin_ahead, self.prepare_ahead, self.stage_lag = 4, 6, 2
        self.stage_nowait = True  # the host round trip of a detection is taken without waiting (icelk_seg_detect_stage_try)
        # the step (counted back from the detection frame) at whose end the host WAITS for a detection's counts if they have
        # not come by themselves.  0: never before the frame itself -- the tail of a detection runs on the device without the
        # host (k_tail.hip), so adopting it is a look at pinned memory, done right before the switch.  1: at the end of step
        # d-1, as long as the tail needed the host (ICELK_HOST_TAIL=1: it had to be enqueued a step before it was needed)
        self.stage_block_at = 1 if os.environ.get("ICELK_HOST_TAIL") else 0
        self._resident = False    # inside push_slot
        # callable(first_frame, closed) invoked once per finished segment, when all its pairs have been launched: e.g.
        # ctx.seg_archive(..., closed=closed).  closed=False: the segment is still the current one (the switch follows);
        # closed=True: the switch has happened (its last pair went out in a joint launch, see `_step`)
        self.on_close = None
        self._advanced = None     # the slot announced for the next frame, when the joint launch of this step took its pair
        self._reset_ahead()
        self.pairs_launched = 0   # frame pairs handed to the tracker kernels so far (a joint launch carries two)
        self._closed_now = False  # the latest step closed a segment: `plot_closed` may draw it on that step's frame

    @staticmethod
    def _stabilize_arg(stabilize, anchor_mask, width, height):
        """The stabilising stage's parameters as a dict, None when it is off.  Refused before a handle is made."""
        if stabilize is None or stabilize is False:
            if anchor_mask is not None:
                raise ValueError("anchor_mask is read by the stabilising stage alone: pass stabilize=True or its parameters")
            return None
        if anchor_mask is None:
            raise ValueError("stabilize needs anchor_mask")
        if np.shape(anchor_mask) != (height, width):
            raise ValueError("anchor_mask must be %d x %d like the frames, not %r" % (height, width, np.shape(anchor_mask)))
        from .stabilize import params_struct
        params = {} if stabilize is True else dict(stabilize)
        params_struct(**params)                   # unknown keywords and values no struct can hold raise here
        return params

    @staticmethod
    def _joined(mask, anchor_mask):
        """The detector's mask with the anchors' ground added: 255 where either is non-zero."""
        if np.shape(mask) != np.shape(anchor_mask):
            raise ValueError("mask and anchor_mask differ in size")
        return np.where((np.asarray(mask) != 0) | (np.asarray(anchor_mask) != 0), 255, 0).astype(np.uint8)

    def _read_segment(self):
        """What a push returns of the finished (still current) segment: read as it is, or through the stabilising stage."""
        if self.stabilize is None:
            return self.ctx.seg_read()
        r = self.ctx.seg_stabilize(**self.stabilize)
        tracks, quality = r.pop("tracks"), r.pop("trackquality")
        self.last_stabilization = r
        return tracks, quality

    def _reset_ahead(self):
        """Nothing is under way for the frames after `counter - 1`."""
        self._det_queue = []      # detections in flight, oldest first: (frame counter, step at which it was begun)
        # latest frame whose detection has been begun / whose corner candidates have been prepared ahead
        self._begun_upto = self._prep_upto = self.counter - 1
        self._staged = None       # (detection frame, corners): a new segment waits in the spare set for the switch
        self._pyr_ahead = set()   # slots whose pyramid was enqueued ahead of their step

    # -- frame sources --------------------------------------------------------------------------
    def _next_slot(self):
        if self._queue:
            raise RuntimeError("prefetched frames are pending; consume them with push_prefetched()")
        return (self.cur + 1) % self.n_slots

    def push(self, frame_gray, wait=True):
        s = self._next_slot()
        self.ctx.upload_gray(s, frame_gray)
        return self._step(s, wait)

    @staticmethod
    def _check_crop(crop_file, resave):
        if crop_file is not None and resave is None:
            raise ValueError("crop_file needs resave: the file written is the re-saved crop")

    @staticmethod
    def _write_crop(crop_file, data):
        """Written on the calling thread once the step is enqueued: the device tracks meanwhile.  No bytes, no file."""
        if data is not None:
            with open(crop_file, "wb") as f:
                f.write(data)

    def _push_upload(self, upload, frame, wait, variant, crop, resave, crop_file, comment):
        """The body of `push_bgr` and `push_jpeg`: `upload` is the Context method that fills the slot."""
        self._check_crop(crop_file, resave)
        s = self._next_slot()
        upload(s, frame, variant, crop, resave)
        # the re-saved crop's file, taken before the step is enqueued: the call's synchronisations wait for the upload alone
        data = None if crop_file is None else self.ctx.jpeg_resave_file(comment)
        seg = self._step(s, wait)
        self._write_crop(crop_file, data)
        return seg

    def push_bgr(self, frame, wait=True, variant=4, crop=None, resave=None, crop_file=None, comment=None):
        """`crop` = (left, top, right, bottom): the box of camtools.py:213-231, cut during the upload.  `resave`: None,
        "reference" or a JPEG quality -- the reference's lossy re-save of the crop, reproduced on the device
        (`Context.upload_bgr`).  `crop_file`: with `resave`, a path to write that re-saved crop to, the file the
        reference's `img_crop.save(outpath)` writes: coded after the upload, written once the step is enqueued; `comment`: the source photo's comment, which
        Pillow carries into that file (`jpeg.source_comment`, or `im.info.get("comment")`)."""
        return self._push_upload(self.ctx.upload_bgr, frame, wait, variant, crop, resave, crop_file, comment)

    def push_jpeg(self, jpeg, wait=True, variant=4, crop=None, resave=None, crop_file=None, comment=None):
        """A frame as `jpeg.read_jpeg` returns it (quantised DCT coefficients): decoded, cropped and turned to gray on
        the device; the step is the one `push_bgr` makes with the file's decoded pixels.  The file's `bytes` instead: the
        Huffman decoding runs on the device as well (`Context.upload_jpeg_file`).  `resave`, `crop_file`, `comment`: as
        `push_bgr`."""
        upload = self.ctx.upload_jpeg_file if isinstance(jpeg, (bytes, bytearray, memoryview)) else self.ctx.upload_jpeg
        return self._push_upload(upload, jpeg, wait, variant, crop, resave, crop_file, comment)

    def push_device(self, dev_ptr, stride, wait=True):
        s = self._next_slot()
        self.ctx.set_gray_device(s, dev_ptr, self.w, self.h, stride)
        return self._step(s, wait)

    def push_pinned(self, pinned_ptr, stride, wait=True):
        s = self._next_slot()
        self.ctx.upload_gray_async(s, pinned_ptr, self.w, self.h, stride)
        return self._step(s, wait)

    def prefetch_pinned(self, pinned_ptr, stride):
        """Start the upload of a FUTURE frame from pinned host memory (BASELINE.json configs[2]: hipMemcpyAsync
        double buffering).  Frames are consumed in prefetch order by `push_prefetched`; with n_slots slots at
        most n_slots - 2 uploads may be in flight (previous and current frame stay resident)."""
        s = self._next_prefetch_slot()
        self.ctx.upload_gray_async(s, pinned_ptr, self.w, self.h, stride)
        self._queue.append(_Ahead(s))

    @property
    def prefetched(self):
        """The slots of the frames prefetched and not yet pushed, in their order."""
        return [q.slot for q in self._queue]

    def _next_prefetch_slot(self):
        if len(self._queue) >= self.n_slots - 2:
            raise RuntimeError("too many frames in flight for %d slots" % self.n_slots)
        last = self._queue[-1].slot if self._queue else self.cur
        return (last + 1) % self.n_slots

    def prefetch_jpeg(self, data, variant=4, crop=None, resave=None, crop_file=None, comment=None):
        """Start the decoding of a FUTURE frame from the bytes of its JPEG file (`Context.upload_jpeg_file_async`): it
        runs on the device beside the steps of the frames in front of it.  Slots, order and the n_slots - 2 limit are
        `prefetch_pinned`'s.  What the host can see of a bad file raises here (ValueError), and no slot is taken; the
        rest comes out of `push_prefetched`.  `resave`, `crop_file`, `comment`: as `push_bgr` -- the re-save and, with
        `crop_file`, the coding of the crop's file are part of the enqueued job; `push_prefetched` writes the file."""
        self._check_crop(crop_file, resave)
        s = self._next_prefetch_slot()
        self.ctx.upload_jpeg_file_async(s, data, variant, crop, resave, crop_file is not None)
        self._queue.append(_Ahead(s, True, crop_file, comment))

    def _upload_bgr_ahead(self, q, frame, variant, crop, resave, crop_file, comment):
        """The synchronous `upload_bgr(resave=)` into the slot of q.  The crop's file is taken at once -- the handle's "most
        recent re-save" is overwritten by the next one -- and its bytes are held until the frame is pushed."""
        self._check_crop(crop_file, resave)
        q.data = None
        self.ctx.upload_bgr(q.slot, frame, variant, crop, resave)
        if crop_file is not None:
            q.crop_file, q.comment, q.data = crop_file, comment, self.ctx.jpeg_resave_file(comment)

    def prefetch_bgr(self, frame, variant=4, crop=None, resave=None, crop_file=None, comment=None):
        """A host-decoded frame into the next prefetch slot (a plain `upload_bgr`): the file of a folder that the device
        decoder does not take, between files that it does.  `resave`, `crop_file`, `comment`: as `push_bgr`."""
        q = _Ahead(self._next_prefetch_slot())
        self._upload_bgr_ahead(q, frame, variant, crop, resave, crop_file, comment)
        self._queue.append(q)

    def replace_prefetched_bgr(self, frame, variant=4, crop=None, resave=None, crop_file=None, comment=None):
        """After `push_prefetched` has raised for the JPEG file at the head of the queue: fill its slot from the
        host-decoded frame instead; `push_prefetched` may then be called again.  `resave`, `crop_file`, `comment`: as
        `push_bgr`."""
        if not self._queue:
            raise RuntimeError("no prefetched frame")
        if self._queue[0].in_flight:
            raise RuntimeError("the frame at the head of the queue has not failed")
        self._upload_bgr_ahead(self._queue[0], frame, variant, crop, resave, crop_file, comment)

    def push_prefetched(self, wait=True):
        if not self._queue:
            raise RuntimeError("no prefetched frame")
        q = self._queue[0]
        if q.in_flight:
            # the verdict on the file, the host decoder if it is asked for.  A file that raises leaves the queue as it is
            # and its slot empty, with no bytes for a crop file (`replace_prefetched_bgr`)
            q.in_flight = False
            if q.crop_file is None:
                self.ctx.jpeg_async_finish(q.slot)
            else:
                q.data = self.ctx.jpeg_async_finish_file(q.slot, q.comment)[0]
        self._queue.pop(0)
        # nothing is built or detected ahead on a frame whose verdict is still out: the list ends in front of it
        ahead = takewhile(lambda a: not a.in_flight or self.ctx.jpeg_async_poll(a.slot) == 1, self._queue[:self.MAX_AHEAD])
        seg = self._step(q.slot, wait, *[a.slot for a in ahead])
        self._write_crop(q.crop_file, q.data)  # once the step is enqueued, as `_push_upload`
        return seg

    def push_slot(self, slot, wait=True, *ahead):
        """Use a frame that already sits in `slot` (level 0 resident in HBM); its pyramid is rebuilt.
        `ahead`: the slots where the following frames already sit, nearest first, up to MAX_AHEAD of them (see `_step`);
        None ends the list."""
        if slot not in self._pyr_ahead:
            self.ctx.drop_pyramid(slot)
        self._resident = True
        try:
            return self._step(slot, wait, *ahead)
        finally:
            self._resident = False

    def push_synth(self, ux, uy, seed=1234, wait=True):
        s = self._next_slot()
        self.ctx.synth_frame(s, self.w, self.h, ux, uy, seed)
        return self._step(s, wait)

    # -- the loop body (s1:313-450) -------------------------------------------------------------
    def _detect_begin(self, slot):
        self.ctx.seg_detect_begin(slot, self.fp["maxCorners"], self.fp["qualityLevel"], self.fp["minDistance"],
                                  self.use_mask, self.fp.get("blockSize", 3), **self._detector_kw())

    def _detector_kw(self):
        """feature_params' useHarrisDetector / k as the keywords of the detector calls.  Parameters that do not name the
        detector give none: the calls are then the very ones they were, under the handle's own setting (Shi-Tomasi unless
        Context.set_detector said otherwise)"""
        if "useHarrisDetector" not in self.fp:
            return {}
        return dict(useHarrisDetector=bool(self.fp["useHarrisDetector"]), k=float(self.fp.get("k", 0.04)))

    MAX_AHEAD = 6

    def _step(self, slot, wait, *ahead_slots):
        """One pass of the loop body.  `ahead_slots`: slots of the FOLLOWING frames (nearest first, up to six) when they
        are already on their way to the device (prefetched uploads, resident ring).  The detector needs nothing but its
        own frame, so the work for a coming detection frame d is spread over the steps before it and runs beside their
        tracker launches, each part as early as the frame's slot is known and the buffers it needs are free:
          d-6  corner candidates (`seg_detect_prepare`: a spare candidate buffer, own stream)
          d-4  min-distance stage (`seg_detect_begin`) -- two detections may be in flight
          d-2  the one host round trip of a detection, the sort and the new segment's initialisation in the spare set
               of segment buffers (`seg_detect_stage`): it waits for kernels that were issued two steps -- with
               track_len 2 a whole tracker launch -- earlier, and the min-distance stage of the NEXT detection is on
               the device already, so the host never stands in a loop with the detector's kernels
          d    the switch (no GPU work, no wait).
        With less lookahead the same calls move later (a stage one step after its begin at the least); with none,
        everything happens at d.

        Joint launch: the last pair of the closing segment, (d-1, d), and the first pair of the new one, (d, d+1), are
        independent (s1:362 / s1:440).  When frame d+1 is already on the device and nothing has to be read at d, step d
        holds the first back (`seg_track_defer`), switches, and tracks (d, d+1) at once: both pairs go to the device as
        ONE tracker launch and step d+1 has no pair left to launch.  Results are those of the serial order in every
        case."""
        self._closed_now = False
        c = self.counter
        detect = c % self.track_len == 0
        ahead = self.lookahead and self.track_len >= 2
        known = ahead_slots[:self.MAX_AHEAD] + (None,)                   # None ends the list
        slot_of = dict(enumerate((slot,) + known[:known.index(None)]))   # frame c + k sits in slot_of[k]
        self._pyr_ahead.discard(slot)
        staged_now = detect and self._adopt_staged(c, ahead)
        if detect and not staged_now:
            self._begin_unstarted(c, slot)
        joint = self._launch_pair(c, slot, slot_of.get(1), detect and staged_now and not wait)
        if self.lookahead:
            self._pyramids_ahead(slot, slot_of.get(1), slot_of.get(2) if self.pair_launch else None)
        out = self._change_segment(c, wait, staged_now) if detect and not joint else None
        if ahead:
            self._work_ahead(c, slot_of)
        self._closed_now = detect and c > 0
        self.cur, self.counter = slot, c + 1
        return out

    def _adopt_staged(self, c, ahead):
        """Phase 1, at a detection frame c.  If its detection was begun steps ago and its tail has run on the device, adopt it
        now (waits only if the device is behind).  Returns whether the segment of frame c waits in the spare set."""
        q = self._det_queue
        if self._staged is None and ahead and q and q[0][0] == c and q[0][1] < c:
            self._staged = (c, self.ctx.seg_detect_stage(self.fp["maxCorners"]))
            q.pop(0)
        return self._staged is not None and self._staged[0] == c

    def _begin_unstarted(self, c, slot):
        """Phase 2, at a detection frame c with nothing staged.  If nothing was started ahead for it, start it now, on its own
        stream, beside the tracker launch of phase 3 (the reference does them back to back, s1:323-326 then s1:437)."""
        if not (self._det_queue and self._det_queue[0][0] == c):
            self._detect_begin(slot)
            self._det_queue.append((c, c))
            self._begun_upto = c

    def _enter_segment(self, c, n_detected):
        """The segment that starts at frame c is the current one: the bookkeeping of a joint and of a plain change."""
        self.n_detected, self._staged, self.seg_first, self.active = n_detected, None, c, True

    def _launch_pair(self, c, slot, next_slot, may_join):
        """Phase 3: the pair (previous frame, this frame) goes to the tracker, unless it went out with the launch of the step
        before -- on the strength of the slot that was announced for this frame then.  Where a staged segment starts here and
        nothing is read (`may_join`) and the next frame's slot is known: the joint launch of `_step`, and True."""
        if self._advanced is not None:
            if slot != self._advanced:
                raise RuntimeError("frame pushed in slot %d, but slot %d was announced for it one step ago (its pair has "
                                   "been launched already)" % (slot, self._advanced))
            self._advanced = None
        elif self.active:
            lk_tail = (self.lk["winSize"], self.lk["maxLevel"], self.lk["criteria"], self.lk.get("minEigThreshold", 1e-4),
                       self.fb_threshold)
            if may_join and self.pair_launch and next_slot is not None and c > 0:
                self.ctx.seg_track_defer(self.cur, slot, *lk_tail)
                self.ctx.seg_switch()
                self.ctx.seg_track(slot, next_slot, *lk_tail, wait=False)
                self.pairs_launched += 2
                self._advanced = next_slot
                if self.on_close is not None:
                    self.on_close(self.seg_first, True)
                self._enter_segment(c, self._staged[1])
                return True
            self.ctx.seg_track(self.cur, slot, *lk_tail, wait=False)
            self.pairs_launched += 1
        return False

    def _pyramids_ahead(self, slot, next_slot, next2_slot):
        """Phase 4: pyramids of the following frames, on the copy stream, in the shadow of the tracker launch of phase 3
        (two ahead when a joint launch may need frame c+2 at step c+1; not the frame that launch has just tracked into)."""
        for s_k in (next_slot, next2_slot):
            if s_k is None or s_k in self._pyr_ahead or s_k in (slot, self.cur, self._advanced):
                continue
            if self._resident:
                self.ctx.drop_pyramid(s_k)   # a resident ring is rebuilt on every visit
            self.ctx.build_pyramid_ahead(s_k, self.lk["winSize"], self.lk["maxLevel"])
            self._pyr_ahead.add(s_k)

    def _change_segment(self, c, wait, staged_now):
        """Phase 5, at a detection frame c whose pair went out plain.  The finished segment is handed over (`on_close`; read
        for the push to return if the caller waits); then the switch, or else the end of frame c's detection, the oldest."""
        if c > 0 and self.on_close is not None:
            self.on_close(self.seg_first, False)
        out = (self.seg_first, *self._read_segment()) if c > 0 and wait else None
        if staged_now:
            self.ctx.seg_switch()
            self._enter_segment(c, self._staged[1])
        else:
            self._enter_segment(c, self.ctx.seg_detect_finish(self.fp["maxCorners"]))
            self._det_queue.pop(0)
        return out

    def _work_ahead(self, c, slot_of):
        """Phase 6, in this order.  Stage: the host round trip of the oldest detection in flight, and the new segment into
        the spare set (behind this step's switch, if there was one: the spare set is the one after the current) -- once its
        kernels have had `stage_lag` steps, or when its frame is next; without waiting while there is a later step to do
        it at, the segment is needed at step d.  (Waiting only at d itself was measured too: the tail of the detection --
        sort, corner list, the new segment's tables -- then starts when the tracker launch already needs it: C3 3 820 ->
        3 290 pairs/s.)  Begin: the next detection frame not begun yet, up to `begin_ahead` steps ahead, two in flight at
        most.  Prepare: the detection frame after the one begun last, once its slot is known (six steps ahead at most) and
        the candidates prepared before have been adopted by their seg_detect_begin."""
        T = self.track_len
        if self._det_queue and self._staged is None:
            d, begun = self._det_queue[0]
            if d > c and begun < c and (c - begun >= self.stage_lag or d - c <= 1):
                wait = d - c <= self.stage_block_at or not self.stage_nowait
                n_new = (self.ctx.seg_detect_stage if wait else self.ctx.seg_detect_stage_try)(self.fp["maxCorners"])
                if n_new is not None:
                    self._staged = (d, n_new)
                    self._det_queue.pop(0)
        d = max(self._begun_upto, c) // T * T + T
        if len(self._det_queue) < 2 and 1 <= d - c <= self.begin_ahead and slot_of.get(d - c) is not None:
            self._detect_begin(slot_of[d - c])
            self._det_queue.append((d, c))
            self._begun_upto = d
        d = max(self._begun_upto, self._prep_upto, c) // T * T + T
        if self._prep_upto <= self._begun_upto and 1 <= d - c <= self.prepare_ahead and slot_of.get(d - c) is not None:
            self.ctx.seg_detect_prepare(slot_of[d - c], self.use_mask, self.fp.get("blockSize", 3), **self._detector_kw())
            self._prep_upto = d

    def plot_closed(self, width=PLOT_WIDTH, stamp="", quality=PLOT_QUALITY):
        """The picture of the segment the latest push closed (the one it returned), drawn on the frame of that push -- the
        segment's last frame -- as the bytes of a JPEG file: `Context.seg_plot(self.cur, closed=True, ...)`, the tracks
        gathered on the device.  RuntimeError when the latest push closed no segment."""
        if not self._closed_now:
            raise RuntimeError("no segment has been closed by the latest push")
        return self.ctx.seg_plot(self.cur, True, width, stamp, quality)

    def flush(self):
        """Nothing of a pushed frame is held back across steps any more; kept so that callers can mark the end of a
        sequence (a pair waiting inside the library -- icelk_seg_track_defer used directly -- goes out)."""
        self.ctx.seg_flush()

    def live(self):
        return self.ctx.seg_live()

    def abort(self):
        """End (or interrupt) a sequence whose announced frames will not all be pushed: a pair held back inside the library
        goes out, detections begun / prepared / staged ahead for frames that never came are abandoned
        (icelk_seg_detect_cancel).  The current segment stays readable; the handle's one-call detector forms work again,
        and pushing may continue -- the next detection frame then starts its detection when it arrives.  Returns the
        number of frames consumed so far."""
        self.ctx.seg_flush()
        self.ctx.seg_detect_cancel()
        for s in sorted(q.slot for q in self._queue if q.in_flight):
            with suppress(ValueError):    # JPEG files in flight are dropped: finished for their working set's sake,
                self.ctx.jpeg_async_finish(s)   # whatever they end as
        for q in self._queue:     # the frames stay queued in their slots; no crop file of theirs is written
            q.in_flight, q.data = False, None
        if self._advanced is not None:
            # a joint launch has already tracked the pair into the frame announced for the next step (it sat in its slot):
            # that frame counts as consumed -- it is never a detection frame (track_len >= 2 wherever pairs are joined)
            self.cur, self.counter, self._advanced = self._advanced, self.counter + 1, None
        self._reset_ahead()
        return self.counter

    def close(self):
        self.ctx.close()
