"""`SegmentTracker` against a recording stand-in for `Context`: what the host half of the hot path asks of the device,
call by call, with no device and no library.

A scenario is a plain function over parameters that drives a tracker as a caller would and returns one trace: every
`Context` call in order (`[name, argument, ...]`), and between them the `on_close` hook, the value every push
returned, every change in the listing of the crop directory and every exception that left a tracker method.
`SCENARIOS` maps a readable key to (function, parameters); `run(key, env)` replays one.  The traces of the tree as
it stood when the schedule was last changed on purpose are `tests/golden/tracker_traces.json.gz`
(`tests/golden/make_tracker_traces.py`); `tests/test_tracker_schedule.py` compares.
"""
import itertools
import json
import os
import tempfile

import numpy as np

from iceberg_tracking_code_amd.tracker import SegmentTracker

RAISED = object()    # what `Trace.call` returns in place of a result when the call raised


def render(x):
    """The one rule by which an argument enters a trace."""
    def plain(v):
        return v is None or isinstance(v, (bool, int, float, str)) or (isinstance(v, tuple) and all(map(plain, v)))
    if isinstance(x, (bytes, bytearray, memoryview)):
        return "bytes:%d" % len(x)
    return repr(x) if plain(x) else type(x).__name__


class Trace:
    def __init__(self, crop_dir=None):
        self.entries = []
        self.crop_dir = crop_dir
        self.listing = []

    def look(self):
        """The crop directory, whenever it is not what it was at the last look."""
        if self.crop_dir is not None:
            now = sorted(os.listdir(self.crop_dir))
            if now != self.listing:
                self.listing = now
                self.entries.append(["crop_dir"] + now)

    def add(self, entry):
        self.look()
        self.entries.append(entry)

    def call(self, fn, *a, **k):
        """A tracker method as a driver calls it: what it raises goes into the trace and the scenario goes on."""
        try:
            return fn(*a, **k)
        except Exception as e:
            self.add(["raises", type(e).__name__, str(e)])
            return RAISED

    def push(self, fn, *a, **k):
        seg = self.call(fn, *a, **k)
        if seg is not RAISED:
            self.add(["returns", None if seg is None else seg[0]])
            self.look()
        return seg

    def crop_files(self):
        self.look()
        for name in self.listing:
            with open(os.path.join(self.crop_dir, name), "rb") as f:
                self.entries.append(["crop_file", name, f.read().decode("latin-1")])

    def done(self):
        return json.loads(json.dumps(self.entries))


class Recorder:
    """Answers every attribute but `n_slots` with a function that records its call and gives the scripted answer.
    `frame` is set by the scenario to the frame it is about to hand over: a JPEG job remembers the frame it carries."""

    def __init__(self, trace, n_slots, tries=(), polls=(), bad=(), refused=()):
        self.n_slots = n_slots
        self._trace = trace
        self._tries, self._polls = list(tries), list(polls)
        self._bad, self._refused = set(bad), set(refused)
        self._count = 100
        self._job_frame = {}
        self.frame = None

    def _answer(self, name, a):
        if name == "seg_detect_stage_try" and self._tries and not self._tries.pop(0):
            return None
        if name in ("seg_detect_stage", "seg_detect_finish", "seg_detect_stage_try"):
            self._count += 1
            return self._count
        if name == "seg_read":
            return np.zeros((1, 3, 2), np.float32), np.zeros((1, 2), np.float32)
        if name == "seg_live":
            return 1, 2
        if name == "jpeg_async_poll":
            return self._polls.pop(0) if self._polls else 1
        if name == "upload_jpeg_file_async":
            if self.frame in self._refused:
                raise ValueError("frame %d refused at start" % self.frame)
            self._job_frame[a[0]] = self.frame
        if name in ("jpeg_async_finish", "jpeg_async_finish_file"):
            frame = self._job_frame.pop(a[0], None)
            if frame in self._bad:
                self._bad.discard(frame)
                raise ValueError("frame %d bad at finish" % frame)
            return (b"file of slot %d" % a[0], {}) if name == "jpeg_async_finish_file" else None
        if name == "jpeg_resave_file":
            return b"resaved, comment " + render(a[0]).encode()
        return None

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def f(*a, **k):
            self._trace.add([name] + [render(x) for x in a] + ["%s=%s" % (n, render(k[n])) for n in sorted(k)])
            return self._answer(name, a)
        return f


def _tracker(trace, *a, **k):
    trk = trace.call(SegmentTracker, *a, **k)
    if trk is not RAISED:
        trk.on_close = lambda first, closed: trace.add(["on_close", first, closed])
    return trk


# -- resident ring (`push_slot`) ----------------------------------------------------------------------------------
RING_FRAMES, RING_SLOTS = 14, 8
TRIES = {"ready": (), "F": (False,), "FFTF": (False, False, True, False)}


def ring(T, lookahead, pair, ann, wait, tries, variant=None, sched=None):
    trace = Trace()
    ctx = Recorder(trace, RING_SLOTS, tries=TRIES[tries])
    trk = _tracker(trace, 64, 48, T, ctx=ctx, lookahead=lookahead, pair_launch=pair)
    if sched is not None:
        trk.begin_ahead, trk.prepare_ahead, trk.stage_lag, trk.stage_nowait = sched
    aborts = {4, 7} if variant == "abort" else set()
    wrong = variant == "wrong_slot"
    i = 0
    while i < RING_FRAMES:
        ahead = [(i + k) % RING_SLOTS for k in range(1, ann + 1)] if i + 1 < RING_FRAMES else []
        if variant == "none_mid" and ahead:
            ahead.insert(ann // 2, None)
        before = trk.pairs_launched
        trace.push(trk.push_slot, i % RING_SLOTS, wait, *ahead)
        joint = trk.pairs_launched - before == 2
        if variant == "plot_closed":
            trace.call(trk.plot_closed, 320, "stamp %d" % i, 80)
        i += 1
        if i - 1 in aborts:
            i = trace.call(trk.abort)            # a pair launched ahead has consumed its frame
            trace.add(["abort returns", i])
        elif wrong and joint and i < RING_FRAMES:
            wrong = False                        # once: the frame in another slot than the one just announced for it
            trace.push(trk.push_slot, (i + 3) % RING_SLOTS, wait)
    trace.call(trk.flush)
    return trace.done()


# -- prefetch queue -----------------------------------------------------------------------------------------------
QUEUE_FRAMES = 12
POLLS = {"1": (), "0010110": (0, 0, 1, 0, 1, 1, 0)}


def _crop_kw(crop_dir, crops, k):
    kw = dict(crop=(1, 2, 3, 4))
    if crops == "all" or (crops == "but5" and k != 5):
        # a trace shows the length of a comment: one length per frame
        kw.update(resave=75, crop_file=os.path.join(crop_dir, "%02d.jpg" % k), comment=b"c" * (k + 1))
    return kw


def queue(T, n_slots, polls, bad, refused, crops, abort, wait, pinned=False):
    with tempfile.TemporaryDirectory() as crop_dir:
        trace = Trace(crop_dir)
        ctx = Recorder(trace, n_slots, polls=POLLS[polls], bad=bad, refused=refused)
        trk = _tracker(trace, 64, 48, T, ctx=ctx, n_slots=n_slots)
        fed = c = 0
        feeding = True
        while c < fed or (feeding and fed < QUEUE_FRAMES):
            while feeding and fed < QUEUE_FRAMES and fed - c < n_slots - 2:
                kw = _crop_kw(crop_dir, crops, fed)
                ctx.frame = fed
                if pinned:
                    trace.call(trk.prefetch_pinned, 4096 + fed, 64)
                elif fed % 5 == 3 or trace.call(trk.prefetch_jpeg, b"x" * fed, **kw) is RAISED:
                    trace.call(trk.prefetch_bgr, "frame %d" % fed, **kw)    # as the folder driver: the host's decoder
                fed += 1
            if trace.push(trk.push_prefetched, wait=wait) is RAISED:
                ctx.frame = c
                trace.call(trk.replace_prefetched_bgr, "host-decoded frame %d" % c, **_crop_kw(crop_dir, crops, c))
                trace.push(trk.push_prefetched, wait=wait)
            if abort and c == 7:
                trace.add(["abort returns", trace.call(trk.abort)])
                feeding = False                  # what is still queued is pushed, nothing more
            c += 1
        trace.call(trk.flush)
        trace.crop_files()
        return trace.done()


def queue_refusals():
    with tempfile.TemporaryDirectory() as crop_dir:
        trace = Trace(crop_dir)
        path = os.path.join(crop_dir, "crop.jpg")
        ctx = Recorder(trace, 5, bad={0})
        trk = _tracker(trace, 64, 48, 2, ctx=ctx, n_slots=5)
        trace.call(trk.replace_prefetched_bgr, "frame")                     # empty queue
        trace.call(trk.replace_prefetched_bgr, "frame", crop_file=path)     # ... which is said first
        trace.call(trk.push_prefetched)
        for form in (trk.push_bgr, trk.prefetch_bgr):                       # crop_file without resave
            trace.call(form, "frame", crop_file=path, comment=b"c")
        trace.call(trk.prefetch_jpeg, b"file", crop_file=path)
        for k in range(3):
            ctx.frame = k
            trace.call(trk.prefetch_jpeg, b"x" * k, resave="reference")
        trace.call(trk.prefetch_pinned, 4096, 64)                           # one more than n_slots - 2
        trace.call(trk.prefetch_bgr, "frame")
        trace.call(trk.prefetch_bgr, "frame", crop_file=path)
        trace.call(trk.prefetch_jpeg, b"file")
        trace.call(trk.prefetch_jpeg, b"file", crop_file=path)
        for form in (trk.push, trk.push_bgr, trk.push_jpeg):               # while frames are queued
            trace.call(form, "frame")
        for form in (trk.push_device, trk.push_pinned, trk.push_synth):
            trace.call(form, 4096, 64)
        trace.call(trk.replace_prefetched_bgr, "frame")                     # the head has not failed
        trace.push(trk.push_prefetched)                                     # ... now it has
        trace.call(trk.replace_prefetched_bgr, "frame", crop_file=path)
        trace.call(trk.replace_prefetched_bgr, "frame", resave=90, crop_file=path, comment=b"c")
        trace.call(trk.replace_prefetched_bgr, "frame")                     # twice: the second one holds, without a file
        for _ in range(4):
            trace.push(trk.push_prefetched)
        trace.crop_files()
        return trace.done()


# -- plain sources ------------------------------------------------------------------------------------------------
SOURCES = ("push", "push_bgr", "push_jpeg_bytes", "push_jpeg_coefficients", "push_device", "push_pinned", "push_synth")


def plain(source, mask, crops):
    with tempfile.TemporaryDirectory() as crop_dir:
        trace = Trace(crop_dir)
        kw = {"mask": dict(mask=np.ones((48, 64), np.uint8)),
              "polygon": dict(mask_polygon=([(1, 1), (60, 1), (30, 40)], 3, 4)), "none": {}}[mask]
        trk = _tracker(trace, 64, 48, 2, ctx=Recorder(trace, 3), **kw)
        trk.on_close = None
        for k in range(5):
            ckw = _crop_kw(crop_dir, crops, k)
            if source == "push":
                trace.push(trk.push, "gray %d" % k)
            elif source == "push_bgr":
                trace.push(trk.push_bgr, "bgr %d" % k, **ckw)
            elif source == "push_jpeg_bytes":
                trace.push(trk.push_jpeg, b"j" * k, True, 2, **ckw)
            elif source == "push_jpeg_coefficients":
                trace.push(trk.push_jpeg, {"frame": k}, **ckw)
            elif source == "push_synth":
                trace.push(trk.push_synth, 0.5 * k, -0.25 * k, seed=k)
            else:
                trace.push(getattr(trk, source), 4096 + k, 64)
        trace.call(trk.flush)
        trace.add(["live returns"] + list(trace.call(trk.live)))
        trace.call(trk.close)
        trace.crop_files()
        return trace.done()


def bad_track_len(T):
    trace = Trace()
    _tracker(trace, 64, 48, T, ctx=Recorder(trace, 3))
    return trace.done()


# -- the catalogue ------------------------------------------------------------------------------------------------
def _key(family, **p):
    def short(v):
        if isinstance(v, tuple):
            return ",".join(map(str, v)) or "-"
        return {True: "1", False: "0"}[v] if isinstance(v, bool) else str(v)
    return family + "".join("/%s=%s" % (n, short(v)) for n, v in p.items())


def _scenarios():
    out = {}

    def add(family, fn, env=None, **p):
        out[_key(family, **p)] = (fn, p, env or {})

    for T, la, pair, ann, wait, tries in itertools.product((1, 2, 3, 5), (False, True), (False, True), (0, 1, 2, 6),
                                                           (False, True), tuple(TRIES)):
        add("ring", ring, T=T, lookahead=la, pair=pair, ann=ann, wait=wait, tries=tries)
    for T, ann, pair, tries in itertools.product((2, 3), (2, 6), (False, True), ("ready", "F")):
        base = dict(T=T, lookahead=True, pair=pair, ann=ann, wait=False, tries=tries)
        add("ring", ring, env={"ICELK_HOST_TAIL": "1"}, **base, variant="host_tail")
        for variant in ("none_mid", "abort", "plot_closed") + (("wrong_slot",) if pair else ()):
            add("ring", ring, **base, variant=variant)
        for sched in ((2, 4, 1, True), (4, 6, 2, False)):
            add("ring", ring, **base, sched=sched)
    for T, n_slots, polls, bad, refused, crops, abort, wait in itertools.product(
            (2, 3), (5, 6), tuple(POLLS), ((), (2,)), ((), (4,)), ("none", "all", "but5"), (False, True), (False, True)):
        add("queue", queue, T=T, n_slots=n_slots, polls=polls, bad=bad, refused=refused, crops=crops, abort=abort,
            wait=wait)
    add("queue", queue, T=2, n_slots=5, polls="0010110", bad=(), refused=(), crops="none", abort=False, wait=False,
        pinned=True)
    add("queue/refusals", queue_refusals)
    for source, mask in itertools.product(SOURCES, ("none", "mask", "polygon")):
        add("plain", plain, source=source, mask=mask, crops="none")
    for source in ("push_bgr", "push_jpeg_bytes", "push_jpeg_coefficients"):
        add("plain", plain, source=source, mask="none", crops="but5")
    for T in (0, 17):
        add("plain/bad_track_len", bad_track_len, T=T)
    return out


SCENARIOS = _scenarios()


def run(key, env):
    """Replay one scenario.  `env`: something with pytest's `monkeypatch.setenv` / `delenv` (the tracker reads
    ICELK_HOST_TAIL when it is made)."""
    fn, params, variables = SCENARIOS[key]
    env.delenv("ICELK_HOST_TAIL", raising=False)
    for name, value in variables.items():
        env.setenv(name, value)
    try:
        return fn(**params)
    finally:
        for name in variables:
            env.delenv(name, raising=False)
