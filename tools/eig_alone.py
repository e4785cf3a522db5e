"""The strip corner kernel alone (candidates prepared ahead, nothing beside them), per block size, from the handle's profile.

    python tools/eig_alone.py [--harris] [--k K] [--size WxH] [--block-sizes 10 3 5 7] [--reps 6] [--rounds 3]

--harris times both responses in ONE process and session, alternating (k_eig_strip, k_harris_strip, k_eig_strip, ...), so
that the two ranges come from one box in one state: C2 is --size 4000x3000 --block-sizes 3, REF --size 3456x2304
--block-sizes 10.  One JSON line per (block size, detector) at the end."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iceberg_tracking_code_amd import Context

ap = argparse.ArgumentParser()
ap.add_argument("--harris", action="store_true")
ap.add_argument("--k", type=float, default=0.04)
ap.add_argument("--size", default="4000x3000")
ap.add_argument("--block-sizes", type=int, nargs="*", default=[10, 3, 5, 7])
ap.add_argument("--reps", type=int, default=6)
ap.add_argument("--rounds", type=int, default=None)
args = ap.parse_args()
w, h = (int(v) for v in args.size.split("x"))
rounds = args.rounds if args.rounds is not None else (3 if args.harris else 1)
ctx = Context(w, h, n_slots=2, max_pts=1 << 16)
ctx.synth_frame(0, w, h, 10, -20, 1234)
ctx.seg_detect(0, 10000, 0.007, 10, False, 10)    # prepared candidates are cut at the quality level of the latest detection


def alone(bs, harris):
    kw = dict(useHarrisDetector=harris, k=args.k)
    ctx.seg_detect_prepare(0, False, bs, **kw); ctx.sync()
    ctx.prof_reset(); ctx.prof_enable(True)
    for _ in range(args.reps):
        ctx.synth_frame(0, w, h, 10, -20, 1234)    # new generation: the prepared candidates are stale
        ctx.seg_detect_prepare(0, False, bs, **kw)
    ctx.sync(); ctx.prof_enable(False)
    return ctx.prof_table()["corner_candidates"]["avg_us"]


out = []
for bs in args.block_sizes:
    times = {False: [], True: []}
    for _ in range(rounds):
        for harris in ((False, True) if args.harris else (False,)):
            times[harris].append(alone(bs, harris))
    for harris, name in ((False, "min_eig"), (True, "harris")):
        if times[harris]:
            t = times[harris]
            print("blockSize", bs, name, "corner kernel alone: %s us (mean of %d launches each)"
                  % (", ".join("%.1f" % v for v in t), args.reps))
            out.append(dict(size=args.size, block_size=bs, detector=name, k=args.k if harris else None, reps=args.reps,
                            avg_us=[round(v, 2) for v in t], min_us=round(min(t), 2), max_us=round(max(t), 2)))
ctx.close()
for o in out:
    print(json.dumps(o))
