#!/usr/bin/env python3
"""What the device JPEG ingest path costs and gains, on 4000x3000 4:2:0 photos of the procedural texture.

    python tools/jpeg_ingest.py host   [--out profiles/jpeg_ingest_host.txt]      any CPU, no GPU needed
    python tools/jpeg_ingest.py device [--out profiles/jpeg_ingest_device.txt]    MI355X: HIP-event times of the two kernels
    python tools/jpeg_ingest.py e2e [--frames 24] [--threads 16] [--out ...]      MI355X: track_image_sequence, both decoders
    python tools/jpeg_ingest.py huffman [--out profiles/jpeg_huffman_device.txt]  MI355X: Huffman decoding on the device
    python tools/jpeg_ingest.py huffman-loop                                      MI355X: the calls for a kernel trace
    python tools/jpeg_ingest.py e2e-huffman [--frames 24] [--threads 16]          MI355X: huffman="host" against "device"
    python tools/jpeg_ingest.py e2e-pipeline [--frames 24] [--threads 16]         MI355X: pipeline=False against True
    python tools/jpeg_ingest.py pipeline-loop [--frames 24]                       MI355X: pipelined runs for a kernel trace
    python tools/jpeg_ingest.py resave [--frames 24] [--out profiles/jpeg_resave.txt]  MI355X: the reference's re-save of the crop
    python tools/jpeg_ingest.py resave-file [--frames 24] [--out profiles/jpeg_resave_file.txt]  MI355X: ... written as files
    python tools/jpeg_ingest.py crop-folder [--frames 96] [--out profiles/jpeg_crop_folder.txt]  MI355X: the crop step on its own
    python tools/jpeg_ingest.py crop-folder-loop [--frames 24]                    MI355X: the calls for a kernel trace
    python tools/jpeg_ingest.py resave-fused [--out profiles/jpeg_resave_pipeline.txt]      MI355X: the fused kernel against the pair
    python tools/jpeg_ingest.py resave-pipeline [--frames 96] [--out ...]         MI355X: one pass against two (appends to the file)

host    one thread, best of 5: `read_jpeg` (Huffman decoding into coefficients) against `np.array(Image.open(...))` (what
        the "pil" decoder does per photo), and Pillow's own 1/8-scale draft decode -- entropy decoding plus a DC-only
        transform, the yardstick for a tuned entropy decoder -- at quality 75 and 95.
device  `Context.upload_jpeg` with profiling on: average HIP-event time of k_jpeg_idct and k_jpeg_out against the bytes
        each has to move, and the host-clock time of the whole call (upload of the coefficients included).
e2e     photos per second of the folder driver with decoder="pil" and decoder="device", same folder, same threads,
        the two alternating.
huffman `Context.upload_jpeg_file` (Huffman decoding on the device too) at quality 75 and 95: the cost of icelk_jpeg_index
        on one host thread, then for subsequence lengths 256 .. 4096 the whole call by the host clock (it ends in a
        synchronise) with rounds, mean and maximum hops, against `read_jpeg` + `upload_jpeg`.
huffman-loop   20 calls of `upload_jpeg_file` per quality at the default subsequence length and nothing else: run it under
        `rocprofv3 --kernel-trace --stats --` for the per-kernel times.
e2e-huffman    the folder driver with decoder="device": huffman="host" against huffman="device", alternating.
e2e-pipeline   the folder driver with decoder="device", huffman="device": pipeline=False (the yardstick) against
        pipeline=True, alternating, three runs each behind one untimed run, tracks compared in every run; then
        pipeline=True over n_slots 5 / 6 / 8, one decode stream against two, normal against high priority
        (ICELK_JPEG_ASYNC_STREAMS / ICELK_JPEG_ASYNC_PRIO), and where a photo's time goes by the host clock.
resave  `Context.upload_bgr(resave="reference")` on a 4000x3000 crop with profiling on: average HIP-event time of k_jpeg_fwd
        (the forward half of the re-save) against its algorithmic bytes, and of k_jpeg_idct and k_jpeg_out on the re-saved
        coefficients; the three uploads by the host clock with and without the re-save; then photos per second of the
        folder driver with resave=None against resave="reference", alternating, three runs each.
resave-file    the re-saved crop as a file (`Context.jpeg_resave_file`, csrc/k_jpeg_enc.hip) at quality 75 and 95: first the
        yardstick, the reference's own step `Image.open -> crop -> save` per photo on one thread and on a pool of 16
        processes (host only, before the GPU is touched); then 20 calls with profiling on: HIP-event time of every encoder
        kernel against the bytes it moves, the whole call by the host clock split into kernels, the rest (two
        synchronisations, the copy to the host, the header) and the file write; then photos per second of the folder
        driver with resave="reference", without and with save_crops, alternating, three runs each.
crop-folder    the crop step on its own (`crop_image_sequence`, csrc/abi_jpeg_crop.hip on csrc/abi_jpeg_job.hip) on the folder of resave-file: the same
        yardstick first (one thread, a pool of 16 processes forked before the GPU is touched); then, alternating behind
        untimed runs, three runs each of (a) the synchronous way to the same folder -- `upload_jpeg_file(resave=)`,
        `jpeg_resave_file()` and the write, photo by photo on the calling thread -- and (b) `crop_image_sequence`; every
        file of (b) is compared with Pillow's before a rate counts; then where a photo's time goes in (b), one job at a time.
crop-folder-loop   two runs of `crop_image_sequence` and nothing else, for `rocprofv3 --kernel-trace --stats --`.
resave-fused   k_jpeg_crop_fwd (the crop box of the planes straight to the re-saved coefficients) against k_jpeg_out in its
        R G B form followed by k_jpeg_fwd, summed, on the same 4000x3000 crop: HIP events around each kernel, 20 launches
        each per run, the two alternating, three runs behind an untimed one.  The pair is a crop job's (its kernel ids
        are its own), the fused kernel goes through its test entry.
resave-pipeline    the folder of crop-folder, photos per second of (a) one pass, `pipeline=True, resave_ahead=True`, without
        and with save_crops, (b) the two-pass route -- `crop_image_sequence`, then a pipelined run on its files, both
        timed -- and (c) `pipeline=False, resave=`; alternating, three runs each behind untimed ones; tracks and crop
        files are checked equal (the files against Pillow's) before a rate counts.
pipeline-loop  one plain and two pipelined runs of the same folder and nothing else, for `rocprofv3 --kernel-trace --stats --`.
"""
import argparse
import datetime as dt
import io
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from PIL import Image  # noqa: E402

W, H = 4000, 3000


def photo(k=0):
    """the procedural texture of synth.py as a colour photo (the three channels are shifted copies)"""
    from iceberg_tracking_code_amd import synth
    g = synth.frame(W, H, 300 * k, -200 * k)
    return np.stack([g, np.roll(g, 3, 1), np.roll(g, 2, 0)], 2)


def encode(img, quality):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=quality, subsampling=2)
    return b.getvalue()


def best_ms(f, n=5):
    best = None
    for _ in range(n):
        t = time.perf_counter()
        f()
        el = time.perf_counter() - t
        best = el if best is None else min(best, el)
    return 1e3 * best


def host(out):
    from iceberg_tracking_code_amd import read_jpeg
    img = photo()
    print("host stage, one thread, best of 5, %dx%d 4:2:0, procedural texture" % (W, H), file=out)
    print("quality  file MB  PIL decode ms  read_jpeg ms  PIL/read_jpeg  draft(1/8) ms  read_jpeg/draft", file=out)
    for q in (75, 95):
        data = encode(img, q)

        def draft():
            im = Image.open(io.BytesIO(data))
            im.draft("RGB", (W // 8, H // 8))
            im.load()
        pil = best_ms(lambda: np.array(Image.open(io.BytesIO(data))))
        rd = best_ms(lambda: read_jpeg(data))
        dr = best_ms(draft)
        print("%7d  %7.2f  %13.1f  %12.1f  %13.2f  %13.1f  %15.2f" % (q, len(data) / 1e6, pil, rd, pil / rd, dr, rd / dr), file=out)


def device(out):
    from iceberg_tracking_code_amd import Context, read_jpeg
    j = read_jpeg(encode(photo(), 90))
    i = j.info
    coef_b = 2 * int(i.coef_count)
    plane_b = sum(i.blocks_x[c] * i.blocks_y[c] * 64 for c in range(3))
    gray_b = W * H
    ctx = Context(W, H, n_slots=2, max_pts=64)
    try:
        for _ in range(3):
            ctx.upload_jpeg(0, j, 4)
        ctx.prof_reset()
        ctx.prof_enable(True)
        n = 20
        t = time.perf_counter()
        for _ in range(n):
            ctx.upload_jpeg(0, j, 4)
        call_ms = 1e3 * (time.perf_counter() - t) / n
        ctx.prof_enable(False)
        tab = ctx.prof_table()
    finally:
        ctx.close()
    idct, outk = tab["jpeg_idct"]["avg_us"], tab["jpeg_out"]["avg_us"]
    print("device stage, %dx%d 4:2:0, %d uploads, HIP events around each kernel" % (W, H, n), file=out)
    print("k_jpeg_idct  %8.1f us  reads %.1f MB of coefficients, writes %.1f MB of planes: %.2f TB/s" %
          (idct, coef_b / 1e6, plane_b / 1e6, (coef_b + plane_b) / idct / 1e6), file=out)
    print("k_jpeg_out   %8.1f us  reads %.1f MB of planes, writes %.1f MB of gray: %.2f TB/s" %
          (outk, plane_b / 1e6, gray_b / 1e6, (plane_b + gray_b) / outk / 1e6), file=out)
    need = (coef_b + gray_b) / 8e12 * 1e6
    trip = 2 * plane_b / 8e12 * 1e6
    print("algorithmic bytes (coefficients in + gray out, %.1f MB) at 8 TB/s: %.1f us; the planes' round trip through HBM "
          "(%.1f MB) another %.1f us" % ((coef_b + gray_b) / 1e6, need, 2 * plane_b / 1e6, trip), file=out)
    print("both kernels %.1f us: %.1f %% of the algorithmic bound, %.1f %% of the bound with the round trip" %
          (idct + outk, 100 * need / (idct + outk), 100 * (need + trip) / (idct + outk)), file=out)
    print("whole upload_jpeg call by the host clock (pageable coefficients across PCIe, both kernels, synchronise): %.2f ms"
          % call_ms, file=out)


def mean_ms(f, n=10, warm=2):
    for _ in range(warm):
        f()
    t = time.perf_counter()
    for _ in range(n):
        f()
    return 1e3 * (time.perf_counter() - t) / n


def huffman(out):
    import ctypes as C
    from iceberg_tracking_code_amd import Context, _lib, read_jpeg
    lib = _lib.load()
    files = [(q, k, encode(photo(k), q)) for q in (75, 95) for k in (0, 1)]
    print("Huffman decoding on the device, %dx%d 4:2:0, procedural texture, two photos per quality" % (W, H), file=out)
    print("icelk_jpeg_index (headers, memchr for the markers, tables), one host thread, best of 5:", file=out)
    for q, k, data in files:
        info, scan = _lib.JpegInfo(), _lib.JpegScan()
        tables = (C.c_uint8 * _lib.JPEG_TABLE_BYTES)()
        ms = best_ms(lambda: lib.icelk_jpeg_index(data, len(data), C.byref(info), C.byref(scan), None, None, 0, tables))
        print("  quality %d photo %d: %.2f MB, %.3f ms (%.1f GB/s)" % (q, k, len(data) / 1e6, ms, len(data) / ms / 1e6), file=out)
    ctx = Context(W, H, n_slots=2, max_pts=64)
    try:
        print("whole call by the host clock, mean of 10, ending in a synchronise:", file=out)
        print("quality photo  read_jpeg ms  upload_jpeg ms | S: upload_jpeg_file ms, compressed GB/s, lanes, rounds, mean hops, max hops, "
              "lanes in step, fallback", file=out)
        for q, k, data in files:
            j = read_jpeg(data)
            rd = best_ms(lambda: read_jpeg(data), 3)
            up = mean_ms(lambda: ctx.upload_jpeg(0, j, 4))
            ctx.upload_jpeg(0, j, 4)
            want = ctx.download_level(0, 0)
            print("%7d %5d  %12.2f  %14.2f" % (q, k, rd, up), file=out)
            for S in (256, 512, 1024, 2048, 4096):
                ctx.jpeg_huff_config(S, 256, 255)
                ms = mean_ms(lambda: ctx.upload_jpeg_file(1, data, 4))
                st = ctx.jpeg_huff_stats()
                same = np.array_equal(ctx.download_level(1, 0), want) and np.array_equal(ctx.jpeg_device_coefficients(data), j.coef)
                print("    S %4d: %7.3f ms  %6.2f GB/s  %6d lanes  %2d rounds  mean %5.2f  max %3d  in step %5d  fallback %d  %s" %
                      (S, ms, len(data) / ms / 1e6, st["subsequences"], st["rounds"], st["total_hops"] / st["subsequences"],
                       st["max_hops"], st["lanes_in_step"], st["fallback"], "equal" if same else "DIFFERENT"), file=out)
                out.flush()
    finally:
        ctx.close()


def huffman_loop():
    from iceberg_tracking_code_amd import Context
    ctx = Context(W, H, n_slots=2, max_pts=64)
    try:
        for q in (75, 95):
            data = encode(photo(), q)
            for _ in range(20):
                ctx.upload_jpeg_file(0, data, 4)
            print("quality %d: %.2f MB, %s" % (q, len(data) / 1e6, ctx.jpeg_huff_stats()))
    finally:
        ctx.close()


def e2e(out, n, threads, compare="decoder"):
    from iceberg_tracking_code_amd import track_image_sequence
    tmp = tempfile.mkdtemp(prefix="icelk_jpeg_")
    t0 = dt.datetime(2019, 7, 24, 10, 0, 0)
    names = []
    for k in range(n):
        p = os.path.join(tmp, (t0 + dt.timedelta(seconds=60 * k)).strftime("%Y%m%d-%H%M%S") + ".jpg")
        with open(p, "wb") as f:
            f.write(encode(photo(k), 90))
        names.append(p)
    size = sum(os.path.getsize(p) for p in names) / n / 1e6
    fp = dict(maxCorners=10000, qualityLevel=0.007, minDistance=10, blockSize=10)
    lk = dict(winSize=(21, 21), maxLevel=3, criteria=(3, 30, 0.01))
    print("folder driver, %d photos of %dx%d 4:2:0 quality 90 (%.1f MB each), decode_threads %d, %d usable cores" %
          (n, W, H, size, threads, len(os.sched_getaffinity(0))), file=out)
    # the two sides of the comparison: the decoders, or, with decoder="device", where the Huffman decoding runs
    word = "decoder" if compare == "decoder" else "huffman"
    sides = ("pil", "device") if compare == "decoder" else ("host", "device")
    res = {sides[0]: [], sides[1]: []}
    ref = None
    for rep in range(3):
        for side in sides:
            kw = dict(decoder=side) if compare == "decoder" else dict(decoder="device", huffman=side)
            t = time.perf_counter()
            got = track_image_sequence(names, tmp, 2, 60, feature_params=fp, lk_params=lk, decode_threads=threads,
                                       decode_ahead=max(6, 2 * threads), save=False, **kw)
            res[side].append(n / (time.perf_counter() - t))
            if ref is None:
                ref = got
            same = len(got) == len(ref) and all(np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(got, ref))
            if not same:
                raise SystemExit("%s %s: tracks differ from the first run" % (word, side))
    for side in sides:
        print('%s="%s": %s photos/s (runs in order)' %
              (word, side, ", ".join("%.1f" % v for v in res[side])), file=out)
    print("ratio of the best runs: %.2f; %d segments, tracks equal in every run" %
          (max(res[sides[1]]) / max(res[sides[0]]), len(ref)), file=out)
    for p in names:
        os.remove(p)
    os.rmdir(tmp)


def folder(n):
    """n photos as the e2e modes use them -> (directory, paths)"""
    tmp = tempfile.mkdtemp(prefix="icelk_jpeg_")
    t0 = dt.datetime(2019, 7, 24, 10, 0, 0)
    names = []
    for k in range(n):
        p = os.path.join(tmp, (t0 + dt.timedelta(seconds=60 * k)).strftime("%Y%m%d-%H%M%S") + ".jpg")
        with open(p, "wb") as f:
            f.write(encode(photo(k), 90))
        names.append(p)
    return tmp, names


PIPE_FP = dict(maxCorners=10000, qualityLevel=0.007, minDistance=10, blockSize=10)
PIPE_LK = dict(winSize=(21, 21), maxLevel=3, criteria=(3, 30, 0.01))


def run_folder(names, tmp, threads, **kw):
    """one run of the folder driver with the device decoder -> (photos/s, segments)"""
    from iceberg_tracking_code_amd import track_image_sequence
    t = time.perf_counter()
    got = track_image_sequence(names, tmp, 2, 60, feature_params=PIPE_FP, lk_params=PIPE_LK, decode_threads=threads,
                               decode_ahead=max(6, 2 * threads), save=False, decoder="device", huffman="device", **kw)
    return len(names) / (time.perf_counter() - t), got


def same_tracks(got, ref):
    return len(got) == len(ref) and all(np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(got, ref))


class Stopwatch:
    """host-clock time spent inside the named callables of one run (class attributes are wrapped and put back)"""

    def __init__(self, targets):
        self.targets, self.total, self.calls, self.saved = targets, {}, {}, []

    def __enter__(self):
        import threading
        lock = threading.Lock()
        for label, (owner, attr) in self.targets.items():
            f = getattr(owner, attr)
            self.saved.append((owner, attr, f))
            self.total[label], self.calls[label] = 0.0, 0

            def timed(*a, _f=f, _label=label, **kw):
                t = time.perf_counter()
                try:
                    return _f(*a, **kw)
                finally:
                    el = time.perf_counter() - t
                    with lock:
                        self.total[_label] += el
                        self.calls[_label] += 1
            setattr(owner, attr, timed)
        return self

    def __exit__(self, *exc):
        for owner, attr, f in self.saved:
            setattr(owner, attr, f)


def pipeline(out, n, threads):
    from iceberg_tracking_code_amd import context, sequence, tracker
    tmp, names = folder(n)
    size = sum(os.path.getsize(p) for p in names) / n / 1e6
    print("folder driver, decoder=\"device\", huffman=\"device\": %d photos of %dx%d 4:2:0 quality 90 (%.1f MB each), "
          "decode_threads %d, %d usable cores" % (n, W, H, size, threads, len(os.sched_getaffinity(0))), file=out)
    for v in ("ICELK_JPEG_ASYNC_STREAMS", "ICELK_JPEG_ASYNC_PRIO"):
        os.environ.pop(v, None)
    _, ref = run_folder(names, tmp, threads)                 # untimed: cold files, code objects, clocks
    res = {False: [], True: []}
    for rep in range(3):
        for pipe in (False, True):
            rate, got = run_folder(names, tmp, threads, pipeline=pipe)
            if not same_tracks(got, ref):
                raise SystemExit("pipeline=%s: tracks differ from the first run" % pipe)
            res[pipe].append(rate)
    for pipe in (False, True):
        print("pipeline=%s: %s photos/s (runs in order)" % (pipe, ", ".join("%.1f" % v for v in res[pipe])), file=out)
    lo, hi = min(res[False]), max(res[False])
    print("ratio of the medians: %.2f (of the best runs: %.2f); spread of pipeline=False: %.1f%% of its median; %d segments, "
          "tracks equal in every run" % (sorted(res[True])[1] / sorted(res[False])[1], max(res[True]) / max(res[False]),
                                         100 * (hi - lo) / sorted(res[False])[1], len(ref)), file=out)
    print("pipeline=True by slots, decode streams and their priority (three runs each, in order):", file=out)
    for prio in ("normal", "high"):
        for streams in (1, 2):
            for slots in (5, 6, 8):
                os.environ["ICELK_JPEG_ASYNC_STREAMS"], os.environ["ICELK_JPEG_ASYNC_PRIO"] = str(streams), prio
                rates = []
                for rep in range(3):
                    rate, got = run_folder(names, tmp, threads, pipeline=True, n_slots=slots)
                    if not same_tracks(got, ref):
                        raise SystemExit("n_slots %d, %d streams, %s: tracks differ" % (slots, streams, prio))
                    rates.append(rate)
                print("  n_slots %d, %d stream%s, %-6s  %s" % (slots, streams, " " if streams == 1 else "s", prio,
                                                             ", ".join("%.1f" % v for v in rates)), file=out)
    for v in ("ICELK_JPEG_ASYNC_STREAMS", "ICELK_JPEG_ASYNC_PRIO"):
        os.environ.pop(v, None)
    # where a photo's time goes (defaults).  The file reads run on the pool's threads beside the loop; the other three
    # are the loop's own thread, one after the other
    targets = {"file read + headers (pool threads)": (sequence, "_load"),
               "start: index, pinned copy, enqueue": (context.Context, "upload_jpeg_file_async"),
               "finish: wait for the verdict": (context.Context, "jpeg_async_finish"),
               "tracker step": (tracker.SegmentTracker, "_step")}
    with Stopwatch(targets) as sw:
        rate, got = run_folder(names, tmp, threads, pipeline=True)
    print("one more pipelined run under a stopwatch: %.1f photos/s = %.2f ms per photo, of which by the host clock" %
          (rate, 1e3 / rate), file=out)
    for label in targets:
        print("  %-36s %6.2f ms per photo (%d calls)" % (label, 1e3 * sw.total[label] / n, sw.calls[label]), file=out)
    targets = {"file read + headers (pool threads)": (sequence, "_load"),
               "upload_jpeg_file (decode, 3 host waits)": (context.Context, "upload_jpeg_file"),
               "tracker step": (tracker.SegmentTracker, "_step")}
    with Stopwatch(targets) as sw:
        rate, got = run_folder(names, tmp, threads, pipeline=False)
    print("and a plain one: %.1f photos/s = %.2f ms per photo" % (rate, 1e3 / rate), file=out)
    for label in targets:
        print("  %-36s %6.2f ms per photo (%d calls)" % (label, 1e3 * sw.total[label] / n, sw.calls[label]), file=out)
    for p in names:
        os.remove(p)
    os.rmdir(tmp)


def resave(out, n, threads):
    from iceberg_tracking_code_amd import Context, read_jpeg, resave_rgb
    img = photo()
    data = encode(img, 90)
    j = read_jpeg(data)
    i = j.info
    rgb_b, coef_b = 3 * W * H, 2 * int(i.coef_count)
    plane_b = sum(i.blocks_x[c] * i.blocks_y[c] * 64 for c in range(3))
    ctx = Context(W, H, n_slots=2, max_pts=64)
    try:
        same = np.array_equal(resave_rgb(img, ctx=ctx), np.array(Image.open(io.BytesIO(encode_default(img)))))
        for _ in range(3):
            ctx.upload_bgr(0, img, 4, resave="reference")
        ctx.prof_reset()
        ctx.prof_enable(True)
        reps = 20
        for _ in range(reps):
            ctx.upload_bgr(0, img, 4, resave="reference")
        ctx.prof_enable(False)
        tab = ctx.prof_table()
        calls = []
        for label, f in (("upload_bgr", lambda **kw: ctx.upload_bgr(0, img, 4, **kw)), ("upload_jpeg", lambda **kw: ctx.upload_jpeg(0, j, 4, **kw)),
                         ("upload_jpeg_file", lambda **kw: ctx.upload_jpeg_file(0, data, 4, **kw))):
            calls.append((label, mean_ms(lambda: f()), mean_ms(lambda: f(resave="reference"))))
    finally:
        ctx.close()
    fwd, idct, outk = (tab[k]["avg_us"] for k in ("jpeg_fwd", "jpeg_idct", "jpeg_out"))
    print("the reference's re-save of the crop on the device, %dx%d crop, quality 75, %d uploads (upload_bgr), HIP events around "
          "each kernel; pixels %s Pillow's" % (W, H, reps, "equal" if same else "DIFFER FROM"), file=out)
    print("k_jpeg_fwd   %8.1f us  reads %.1f MB of RGB, writes %.1f MB of coefficients: %.2f TB/s; those bytes at 8 TB/s: %.1f us" %
          (fwd, rgb_b / 1e6, coef_b / 1e6, (rgb_b + coef_b) / fwd / 1e6, (rgb_b + coef_b) / 8e12 * 1e6), file=out)
    print("k_jpeg_idct  %8.1f us  reads %.1f MB of coefficients, writes %.1f MB of planes: %.2f TB/s" %
          (idct, coef_b / 1e6, plane_b / 1e6, (coef_b + plane_b) / idct / 1e6), file=out)
    print("k_jpeg_out   %8.1f us  reads %.1f MB of planes, writes %.1f MB of gray: %.2f TB/s" %
          (outk, plane_b / 1e6, W * H / 1e6, (plane_b + W * H) / outk / 1e6), file=out)
    print("forward kernel / (k_jpeg_idct + k_jpeg_out): %.2f" % (fwd / (idct + outk)), file=out)
    print("whole call by the host clock, mean of 10, ending in a synchronise: resave=None, resave=\"reference\"", file=out)
    for label, a, b in calls:
        print("  %-17s %7.2f ms  %7.2f ms  (+%.2f ms)" % (label, a, b, b - a), file=out)
    out.flush()
    tmp, names = folder(n)
    print("folder driver, decoder=\"device\", huffman=\"device\": %d photos of %dx%d 4:2:0 quality 90, decode_threads %d, %d usable cores" %
          (n, W, H, threads, len(os.sched_getaffinity(0))), file=out)
    run_folder(names, tmp, threads)                          # untimed: cold files, code objects, clocks
    res, segs = {None: [], "reference": []}, {}
    for rep_ in range(3):
        for side in (None, "reference"):
            rate, got = run_folder(names, tmp, threads, resave=side)
            if side in segs and not same_tracks(got, segs[side]):
                raise SystemExit("resave=%s: tracks differ between runs" % side)
            segs[side] = got
            res[side].append(rate)
    for side in (None, "reference"):
        print("resave=%s: %s photos/s (runs in order)" % (repr(side), ", ".join("%.1f" % v for v in res[side])), file=out)
    print("ratio of the medians: %.2f; %d segments; tracks equal between the two: %s (they are not meant to be)" %
          (sorted(res["reference"])[1] / sorted(res[None])[1], len(segs[None]), same_tracks(segs[None], segs["reference"])), file=out)
    for p in names:
        os.remove(p)
    os.rmdir(tmp)


def _reference_step(args):
    """camtools.py:64-104 for one photo: open, crop (the whole frame here), save at Pillow's defaults"""
    src, dst = args
    im = Image.open(src)
    w, h = im.size
    im.crop((0, 0, w, h)).save(dst)
    return os.path.getsize(dst)


def resave_file(out, n, threads):
    import multiprocessing as mp
    tmp, names = folder(n)
    crops = os.path.join(tmp, "crops")
    os.makedirs(crops)
    jobs = [(p, os.path.join(crops, os.path.basename(p))) for p in names]
    print("the re-saved crop as a file, %d photos of %dx%d 4:2:0 quality 90, %d usable cores" % (n, W, H, len(os.sched_getaffinity(0))), file=out)
    print("yardstick, the reference's step on the host (Image.open -> crop -> save, quality 75), photos/s, three runs each:", file=out)
    _reference_step(jobs[0])                                 # untimed
    one = []
    for _ in range(3):
        t = time.perf_counter()
        for j in jobs:
            _reference_step(j)
        one.append(n / (time.perf_counter() - t))
    print("  one thread:          %s" % ", ".join("%.1f" % v for v in one), file=out)
    with mp.get_context("fork").Pool(16) as pool:            # before this process touches the GPU
        pool.map(_reference_step, jobs)
        many = []
        for _ in range(3):
            t = time.perf_counter()
            pool.map(_reference_step, jobs)
            many.append(n / (time.perf_counter() - t))
    print("  pool of 16 processes: %s" % ", ".join("%.1f" % v for v in many), file=out)
    out.flush()

    from iceberg_tracking_code_amd import Context
    img = photo()
    kernels = ("jpeg_enc_count", "jpeg_enc_scan", "jpeg_enc_pack", "jpeg_enc_ff", "jpeg_enc_stuff")
    ctx = Context(W, H, n_slots=2, max_pts=64)
    try:
        for q in (75, 95):
            want = io.BytesIO()
            Image.fromarray(img).save(want, "JPEG", quality=q)
            want = want.getvalue()
            blocks = 6 * ((W + 15) // 16) * ((H + 15) // 16)
            coef_b = 128 * blocks
            for _ in range(3):
                ctx.upload_bgr(0, img, 4, resave=q)
                got = ctx.jpeg_resave_file()
            ctx.prof_reset()
            ctx.prof_enable(True)
            reps, call, write = 20, [], []
            for _ in range(reps):
                ctx.upload_bgr(0, img, 4, resave=q)
                t = time.perf_counter()
                got = ctx.jpeg_resave_file()
                call.append(time.perf_counter() - t)
                t = time.perf_counter()
                with open(os.path.join(crops, "one.jpg"), "wb") as f:
                    f.write(got)
                write.append(time.perf_counter() - t)
            ctx.prof_enable(False)
            tab = ctx.prof_table()
            stream = len(got) - (got.index(b"\xff\xda") + 14) - 2   # header and EOI aside
            packed = stream - got.count(b"\xff\x00")
            moved = {"jpeg_enc_count": (coef_b, 2 * blocks), "jpeg_enc_scan": (4 * (blocks // 64), 4 * (blocks // 64)),
                     "jpeg_enc_pack": (coef_b + 2 * blocks, packed), "jpeg_enc_ff": (packed, 4 * (packed // 16384 + 1)),
                     "jpeg_enc_stuff": (packed, stream)}
            print("quality %d: file %.2f MB, %s Pillow's; %d blocks; %d calls, HIP events around each kernel (scan runs twice per "
                  "call: the bytes are the first's)" % (q, len(got) / 1e6, "equals" if got == want else "DIFFERS FROM", blocks, reps), file=out)
            total = 0.0
            for k in kernels:
                us, launches = tab[k]["avg_us"], tab[k]["launches"]
                total += us * launches / reps
                rd, wr = moved[k]
                print("  k_%-15s %7.1f us  reads %8.3f MB, writes %8.3f MB: %6.3f TB/s, %5.2f %% of 8 TB/s" %
                      (k, us, rd / 1e6, wr / 1e6, (rd + wr) / us / 1e6, 100 * (rd + wr) / us / 1e6 / 8), file=out)
            call, write = sorted(call), sorted(write)
            print("  jpeg_resave_file() by the host clock, median of %d (min .. max): %.3f ms (%.3f .. %.3f); kernels %.3f ms; the rest "
                  "(two synchronisations, %.2f MB to the host, header, bytes object) %.3f ms; file write %.3f ms (%.3f .. %.3f)" %
                  (reps, 1e3 * call[reps // 2], 1e3 * call[0], 1e3 * call[-1], total / 1e3, len(got) / 1e6, 1e3 * call[reps // 2] - total / 1e3,
                   1e3 * write[reps // 2], 1e3 * write[0], 1e3 * write[-1]), file=out)
            out.flush()
    finally:
        ctx.close()
    print("folder driver, decoder=\"device\", huffman=\"device\", resave=\"reference\", decode_threads %d: photos/s (runs in order)" % threads,
          file=out)
    run_folder(names, tmp, threads, resave="reference")      # untimed: cold files, code objects, clocks
    run_folder(names, tmp, threads, resave="reference", save_crops=crops)   # ... and the writer's buffers
    res, segs = {False: [], True: []}, {}
    for rep_ in range(3):
        for side in (False, True):
            kw = dict(save_crops=crops) if side else {}
            rate, got = run_folder(names, tmp, threads, resave="reference", **kw)
            if segs and not same_tracks(got, segs[0]):
                raise SystemExit("save_crops=%s: tracks differ" % side)
            segs[0] = got
            res[side].append(rate)
    print("  without save_crops: %s" % ", ".join("%.1f" % v for v in res[False]), file=out)
    print("  with save_crops:    %s" % ", ".join("%.1f" % v for v in res[True]), file=out)
    print("  ratio of the medians: %.2f; tracks equal in every run; against the yardstick's medians: %.2f x one thread, %.2f x "
          "the pool of 16 (the driver also decodes, re-saves, detects and tracks)" %
          (sorted(res[True])[1] / sorted(res[False])[1], sorted(res[True])[1] / sorted(one)[1], sorted(res[True])[1] / sorted(many)[1]), file=out)
    for f in os.listdir(crops):
        os.remove(os.path.join(crops, f))
    os.rmdir(crops)
    for p in names:
        os.remove(p)
    os.rmdir(tmp)


def _median(v):
    return sorted(v)[len(v) // 2]


def _remove_tree(tmp, dirs, names):
    for d in dirs:
        if not os.path.isdir(d):
            continue
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
        os.rmdir(d)
    for p in names:
        os.remove(p)
    os.rmdir(tmp)


def crop_folder(out, n):
    import multiprocessing as mp
    tmp, names = folder(n)
    dirs = [os.path.join(tmp, d) for d in ("crops_pillow", "crops_a", "crops_b")]
    for d in dirs:
        os.makedirs(d)
    pillow_dir, a_dir, b_dir = dirs
    try:                                                     # the tree goes whatever happens: 96 photos of 12 MP
        jobs = [(p, os.path.join(pillow_dir, os.path.basename(p))) for p in names]
        print("the crop step on its own, %d photos of %dx%d 4:2:0 quality 90, %d usable cores" % (n, W, H, len(os.sched_getaffinity(0))), file=out)
        print("yardstick, the reference's step on the host (Image.open -> crop -> save, quality 75), photos/s, three runs each:", file=out)
        _reference_step(jobs[0])                                 # untimed
        one = []
        for _ in range(3):
            t = time.perf_counter()
            for j in jobs:
                _reference_step(j)
            one.append(n / (time.perf_counter() - t))
        print("  one thread:           %s" % ", ".join("%.1f" % v for v in one), file=out)
        with mp.get_context("fork").Pool(16) as pool:            # before this process touches the GPU
            pool.map(_reference_step, jobs)
            many = []
            for _ in range(3):
                t = time.perf_counter()
                pool.map(_reference_step, jobs)
                many.append(n / (time.perf_counter() - t))
        print("  pool of 16 processes: %s" % ", ".join("%.1f" % v for v in many), file=out)
        out.flush()

        from iceberg_tracking_code_amd import Context, crop_image_sequence, source_comment
        ctx = Context(W, H, n_slots=2, max_pts=64)

        def run_a():
            """the synchronous way, everything on the calling thread"""
            t = time.perf_counter()
            for p in names:
                with open(p, "rb") as f:
                    data = f.read()
                ctx.upload_jpeg_file(0, data, 4, None, resave="reference")
                got = ctx.jpeg_resave_file(source_comment(data))
                with open(os.path.join(a_dir, os.path.basename(p)), "wb") as f:
                    f.write(got)
            return n / (time.perf_counter() - t)

        def run_b():
            t = time.perf_counter()
            done = crop_image_sequence(names, b_dir, ctx=ctx)
            return n / (time.perf_counter() - t), done

        try:
            run_a()                                              # untimed: cold files, code objects, clocks, the jobs' buffers
            _, done = run_b()
            routes = {}
            for (path, nbytes, route), (_, want) in zip(done, jobs):
                routes[route] = routes.get(route, 0) + 1
                for mine in (path, os.path.join(a_dir, os.path.basename(path))):
                    with open(mine, "rb") as f, open(want, "rb") as g:
                        if f.read() != g.read():
                            raise SystemExit("%s differs from Pillow's file" % mine)
            print("all %d files of (a) and of (b) equal Pillow's; routes of (b): %s" % (n, routes), file=out)
            res = {"a": [], "b": []}
            for _ in range(3):
                res["a"].append(run_a())
                res["b"].append(run_b()[0])
            print("(a) upload_jpeg_file(resave=) + jpeg_resave_file() + write, calling thread, photos/s (runs in order): %s" %
                  ", ".join("%.1f" % v for v in res["a"]), file=out)
            print("(b) crop_image_sequence, 4 readers, 2 writers, 4 in flight, photos/s:                               %s" %
                  ", ".join("%.1f" % v for v in res["b"]), file=out)
            ma, mb, mo, mm = (_median(v) for v in (res["a"], res["b"], one, many))

            def verdict(x, y):
                return "no difference (below the 10 %% spread between runs)" if abs(x / y - 1) < 0.10 else "%.2f x" % (x / y)
            print("medians: (a) %.1f, (b) %.1f, one thread %.1f, pool of 16 %.1f; (b) against (a): %s; (b) against the pool: %s" %
                  (ma, mb, mo, mm, verdict(mb, ma), verdict(mb, mm)), file=out)
            # where a photo's time goes in (b): one job at a time, by the host clock
            parts = {k: [] for k in ("read", "start", "device", "finish", "write")}
            for p in names:
                t0 = time.perf_counter()
                with open(p, "rb") as f:
                    data = f.read()
                comment = source_comment(data)
                t1 = time.perf_counter()
                ticket = ctx.jpeg_crop_start(data, None, 75)
                t2 = time.perf_counter()
                while ctx.jpeg_crop_poll(ticket) == 0:
                    pass
                t3 = time.perf_counter()
                got, _ = ctx.jpeg_crop_finish(ticket, comment)
                t4 = time.perf_counter()
                with open(os.path.join(b_dir, os.path.basename(p)), "wb") as f:
                    f.write(got)
                t5 = time.perf_counter()
                for k, v in zip(("read", "start", "device", "finish", "write"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
                    parts[k].append(1e3 * v)
            print("one job at a time, median ms per photo: " + ", ".join("%s %.3f" % (k, _median(v)) for k, v in parts.items()) +
                  " (start: index, lanes, the copy into pinned memory, the enqueue; device: polling until the verdict; finish: the copy "
                  "of the scan, header, bytes object)", file=out)
        finally:
            ctx.close()
    finally:
        _remove_tree(tmp, dirs, names)


def resave_fused(out):
    from iceberg_tracking_code_amd import Context
    data = encode(photo(), 90)
    reps = 20
    ctx = Context(W, H, n_slots=2, max_pts=64)
    try:
        def pair():
            for _ in range(reps):
                ctx.jpeg_crop_finish(ctx.jpeg_crop_start(data, None, 75))

        def fused():
            for _ in range(reps):
                ctx.jpeg_crop_fwd_device_coefficients(data)

        def timed(f, keys):
            ctx.prof_reset()
            ctx.prof_enable(True)
            f()
            ctx.prof_enable(False)
            tab = ctx.prof_table()
            assert all(tab[k]["launches"] == reps for k in keys), tab
            return [tab[k]["avg_us"] for k in keys]
        pair()
        fused()                                                  # untimed
        rows = []
        for _ in range(3):
            rgb, fwd = timed(pair, ("jpeg_crop_rgb", "jpeg_fwd"))
            (one,) = timed(fused, ("jpeg_crop_fwd",))
            rows.append((rgb, fwd, one))
    finally:
        ctx.close()
    print("the fused crop-and-forward kernel against the pair it replaces, %dx%d crop of a 4:2:0 photo, quality 75, HIP events, "
          "%d launches per run, us per launch (runs in order)" % (W, H, reps), file=out)
    print("run  k_jpeg_out<rgb>  k_jpeg_fwd    pair  k_jpeg_crop_fwd  fused / pair", file=out)
    for k, (rgb, fwd, one) in enumerate(rows):
        print("%3d  %15.1f  %10.1f  %6.1f  %15.1f  %12.2f" % (k, rgb, fwd, rgb + fwd, one, one / (rgb + fwd)), file=out)
    pairs, ones = [r[0] + r[1] for r in rows], [r[2] for r in rows]
    spread = max(max(pairs) - min(pairs), max(ones) - min(ones))
    diff = _median(ones) - _median(pairs)
    print("medians: pair %.1f us, fused %.1f us; spread between runs %.1f us; fused - pair %+.1f us: %s" %
          (_median(pairs), _median(ones), spread, diff,
           "SLOWER than the pair by more than the spread" if diff > spread else "not slower than the pair by more than the spread"), file=out)
    print("derived, not timed: the pair writes and reads %.1f MB of R G B per photo (%.1f MB of traffic) in a buffer of %.1f MB per "
          "job in flight; the fused kernel has neither" % (3 * W * H / 1e6, 6 * W * H / 1e6, 3 * W * H / 1e6), file=out)


def resave_pipeline(out, n, threads):
    from iceberg_tracking_code_amd import crop_image_sequence
    tmp, names = folder(n)
    dirs = [os.path.join(tmp, d) for d in ("crops_pillow", "crops_one_pass", "crops_two_pass")]
    for d in dirs:
        os.makedirs(d)
    pillow_dir, one_dir, two_dir = dirs
    try:
        for p in names:
            _reference_step((p, os.path.join(pillow_dir, os.path.basename(p))))

        def check_files(d):
            for p in names:
                with open(os.path.join(d, os.path.basename(p)), "rb") as f, open(os.path.join(pillow_dir, os.path.basename(p)), "rb") as g:
                    if f.read() != g.read():
                        raise SystemExit("%s: %s differs from Pillow's file" % (d, os.path.basename(p)))

        def one_pass(save):
            rate, got = run_folder(names, tmp, threads, pipeline=True, resave_ahead=True, resave="reference", save_crops=one_dir if save else None)
            if save:
                check_files(one_dir)
            return rate, got

        def two_pass():
            t = time.perf_counter()
            done = crop_image_sequence(names, two_dir)
            got = run_folder([p for p, _, _ in done], tmp, threads, pipeline=True)[1]
            rate = n / (time.perf_counter() - t)
            check_files(two_dir)
            return rate, got

        def serial():
            return run_folder(names, tmp, threads, resave="reference")
        routes = (("(a) one pass, resave_ahead=True", lambda: one_pass(False)), ("(a) ... with save_crops", lambda: one_pass(True)),
                  ("(b) two passes, crop pass included", two_pass), ("(c) pipeline=False, resave=", serial))
        ref = None
        for label, f in routes:                                  # untimed: cold files, code objects, clocks, the jobs' buffers
            got = f()[1]
            ref = got if ref is None else ref
            if not same_tracks(got, ref):
                raise SystemExit("%s: tracks differ from the first route's" % label)
        res = {label: [] for label, _ in routes}
        for _ in range(3):
            for label, f in routes:
                rate, got = f()
                if not same_tracks(got, ref):
                    raise SystemExit("%s: tracks differ" % label)
                res[label].append(rate)
        print("", file=out)
        print("the reference's tracks from a folder of %d photos of %dx%d 4:2:0 quality 90, decode_threads %d, %d usable cores; photos/s "
              "(runs in order), tracks equal on every route, crop files equal Pillow's" % (n, W, H, threads, len(os.sched_getaffinity(0))), file=out)
        for label, _ in routes:
            print("  %-36s %s   median %.1f" % (label, ", ".join("%.1f" % v for v in res[label]), _median(res[label])), file=out)
        a, a_save, b, c = (_median(res[label]) for label, _ in routes)
        print("(a) / (b): %.2f, with save_crops %.2f; (a) / (c): %.2f" % (a / b, a_save / b, a / c), file=out)
    finally:
        _remove_tree(tmp, dirs, names)


def crop_folder_loop(n):
    from iceberg_tracking_code_amd import crop_image_sequence
    tmp, names = folder(n)
    d = os.path.join(tmp, "crops")
    os.makedirs(d)
    try:
        for rep in range(2):
            t = time.perf_counter()
            done = crop_image_sequence(names, d)
            print("crop_image_sequence: %.1f photos/s, routes %s" % (n / (time.perf_counter() - t), sorted({r for _, _, r in done})))
    finally:
        _remove_tree(tmp, [d], names)


def encode_default(img):
    """Pillow's defaults, as the reference's crop pool saves"""
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG")
    return b.getvalue()


def pipeline_loop(n):
    tmp, names = folder(n)
    _, ref = run_folder(names, tmp, 16)
    for rep in range(2):
        rate, got = run_folder(names, tmp, 16, pipeline=True)
        print("pipeline=True: %.1f photos/s, tracks %s" % (rate, "equal" if same_tracks(got, ref) else "DIFFER"))
    for p in names:
        os.remove(p)
    os.rmdir(tmp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("host", "device", "e2e", "huffman", "huffman-loop", "e2e-huffman", "e2e-pipeline",
                                         "pipeline-loop", "resave", "resave-file", "crop-folder", "crop-folder-loop", "resave-fused",
                                         "resave-pipeline"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=None)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    if a.frames is None:
        a.frames = 96 if a.mode in ("crop-folder", "resave-pipeline") else 24
    if a.mode == "huffman-loop":
        return huffman_loop()
    if a.mode == "pipeline-loop":
        return pipeline_loop(a.frames)
    if a.mode == "crop-folder-loop":
        return crop_folder_loop(a.frames)
    name = {"resave-fused": "jpeg_resave_pipeline", "resave-pipeline": "jpeg_resave_pipeline", "resave": "jpeg_resave", "resave-file": "jpeg_resave_file", "crop-folder": "jpeg_crop_folder", "huffman": "jpeg_huffman_device", "e2e-huffman": "jpeg_huffman_e2e", "e2e-pipeline": "jpeg_pipeline_e2e"}.get(
        a.mode, "jpeg_ingest_%s" % a.mode)
    path = a.out or os.path.join(ROOT, "profiles", name + ".txt")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a" if a.mode == "resave-pipeline" else "w") as out:
        if a.mode == "resave-fused":
            resave_fused(out)
        elif a.mode == "resave-pipeline":
            resave_pipeline(out, a.frames, min(a.threads, 16))
        elif a.mode == "host":
            host(out)
        elif a.mode == "device":
            device(out)
        elif a.mode == "huffman":
            huffman(out)
        elif a.mode == "e2e-huffman":
            e2e(out, a.frames, min(a.threads, 16), compare="huffman")
        elif a.mode == "resave":
            resave(out, a.frames, min(a.threads, 16))
        elif a.mode == "resave-file":
            resave_file(out, a.frames, min(a.threads, 16))
        elif a.mode == "crop-folder":
            crop_folder(out, a.frames)
        elif a.mode == "e2e-pipeline":
            pipeline(out, a.frames, min(a.threads, 16))
        else:
            e2e(out, a.frames, min(a.threads, 16))
    sys.stdout.write(open(path).read())


if __name__ == "__main__":
    main()
