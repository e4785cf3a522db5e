"""What the stabilising stage costs per segment (profiles/stabilize.txt is one run's output).

Two segments of three vertices (track_len 2) tracked on procedural frames: 10 000 rows on 4000 x 3000 (the C2
configuration of bench.py) and the uncapped detector on 3456 x 2304 (REF, about 40 000 rows); the anchor mask is the left
tenth of the frame, so about a tenth of the rows are anchors.  On the finished segment three read-outs alternate within one
run, each after WARM warm-up rounds:
    seg_stabilize                              gather, flags, fit and correction on the device, one read-out
    seg_read                                   the plain read-out
    seg_read + stabilize_tracks_host           the plain read-out and the host statement of the same rules
Every call ends in a wait for the device, so the time between two device events recorded around it (on an otherwise idle
stream of the host framework) is the call's duration on the device's clock; without the framework the host clock is used
and the output says so.  The per-kernel times are not taken here: they come from one separate
`rocprofv3 --kernel-trace --stats` run of this script with --once, which does a single seg_stabilize per configuration.
Needs an MI355X.

    python tools/stabilize_bench.py [output file] [--once]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from iceberg_tracking_code_amd import Context, stabilize_tracks_host

args = [a for a in sys.argv[1:] if not a.startswith("--")]
ONCE = "--once" in sys.argv
out = open(args[0], "w") if args else None
REPEATS, WARM = (1, 0) if ONCE else (30, 5)
PERIOD_US = 289.0    # two frames of the C2 loop
CONFIGS = (("C2", 4000, 3000, 10000, (21, 21), 3, (3, 30, 0.01)), ("REF", 3456, 2304, 50000000, (35, 35), 4, (3, 25, 0.03)))
DETECT = dict(qualityLevel=0.007, minDistance=10, blockSize=10)


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


try:
    import torch
    EVENTS = torch.cuda.is_available()
except ImportError:
    EVENTS = False


def timed(call):
    """(microseconds, result) of a call that has waited for the device when it returns"""
    if EVENTS:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        result = call()
        b.record()
        b.synchronize()
        return 1e3 * a.elapsed_time(b), result
    t = time.perf_counter()
    result = call()
    return 1e6 * (time.perf_counter() - t), result


def med(v):
    return "median %8.1f us (min %8.1f, max %8.1f) of %d" % (statistics.median(v), min(v), max(v), len(v))


say("clock: " + ("device events around each synchronised call" if EVENTS else "host clock around each synchronised call"))
for name, w, h, max_corners, win, max_level, criteria in CONFIGS:
    ctx = Context(w, h, n_slots=3, max_pts=1 << 18)
    for slot, (ux, uy) in enumerate(((0, 0), (296, -168), (-832, 640))):
        ctx.synth_frame(slot, w, h, ux, uy, 1234)
    n0 = ctx.seg_detect(0, max_corners, DETECT["qualityLevel"], DETECT["minDistance"], False, DETECT["blockSize"])
    ctx.seg_track(0, 1, win, max_level, criteria)
    ctx.seg_track(1, 2, win, max_level, criteria)
    mask = np.zeros((h, w), np.uint8)
    mask[:, :w // 10] = 255
    ctx.stab_set_anchor_mask(mask)

    def host_route():
        tracks, quality = ctx.seg_read()
        x0, y0 = np.floor(tracks[:, 0, 0].astype(np.float64) + 0.5), np.floor(tracks[:, 0, 1].astype(np.float64) + 0.5)
        return stabilize_tracks_host(tracks, x0 < w // 10)

    routes = (("seg_stabilize", ctx.seg_stabilize), ("seg_read", ctx.seg_read), ("seg_read + stabilize_tracks_host", host_route))
    times = {r: [] for r, _ in routes}
    last = {}
    for i in range(WARM + REPEATS):
        for r, call in routes if not ONCE else routes[:1]:
            us, last[r] = timed(call)
            if i >= WARM:
                times[r].append(us)
    dev = last["seg_stabilize"]
    say("%s: %d x %d, %d corners, %d rows after two pairs, %d anchors, V = 3; inliers %s, status %s, rounds %s"
        % (name, w, h, n0, len(dev["tracks"]), dev["n_anchors"], dev["inliers"].tolist(), dev["status"].tolist(), dev["rounds_used"].tolist()))
    if not ONCE:
        host = last["seg_read + stabilize_tracks_host"]
        say("  device equals the host statement: %s" % all(np.array_equal(dev[k].view(np.uint8), host[k].view(np.uint8))
                                                            for k in ("tracks", "motion", "rms", "inliers", "status")))
        for r, _ in routes:
            say("  %-34s %s" % (r, med(times[r])))
        added = statistics.median(times["seg_stabilize"]) - statistics.median(times["seg_read"])
        say("  added per segment by the stage: %.1f us, %.0f %% of the %.0f us period of two frames" % (added, 100.0 * added / PERIOD_US, PERIOD_US))
    ctx.close()
say("done")
