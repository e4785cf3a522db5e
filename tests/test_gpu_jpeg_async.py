"""GPU: JPEG files decoded ahead of their frame (csrc/abi_jpeg_async.hip on csrc/abi_jpeg_job.hip, k_jpeg_huff_verdict) against the synchronous
call on the same bytes under the same `jpeg_huff_config`: one file, several in flight and their working sets reused,
the caller's buffer, damaged and unsupported files, the tracker fed by `prefetch_jpeg`, the pipelined folder driver;
the verdict kernel on the edges of its bounds (the round a file settles in, more than 64 rounds, the longest chain)
against the CPU statement of the lanes as well, and the calls that may come between a start and its finish.
Every comparison is exact; which files fall back to the host decoder is never written down here, the synchronous call
and the CPU statement say it."""
import datetime as dt
import io
import os
import time

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_streams as js
from test_gpu_jpeg_streams import UPLOADS

pytestmark = pytest.mark.gpu

DEADLINE = 20.0   # seconds a verdict may take before a test gives up polling


@pytest.fixture()
def hctx(ctx):
    """the session's context with the decoder's defaults, whatever a test sets"""
    ctx.jpeg_huff_config()
    yield ctx
    ctx.jpeg_huff_config()


def _photo(sampling):
    return jc.encode(jc.photo(120, 88, 21), quality=85, subsampling=sampling)


def _poll_until_there(ctx, slot):
    t0 = time.monotonic()
    while True:
        state = ctx.jpeg_async_poll(slot)
        if state != 0:
            return state
        assert time.monotonic() - t0 < DEADLINE, "no verdict within %g s" % DEADLINE


def _sync(ctx, slot, data, variant=4, crop=None):
    """(pixels, statistics) the synchronous call leaves"""
    ctx.upload_jpeg_file(slot, data, variant, crop)
    return ctx.download_level(slot, 0), ctx.jpeg_huff_stats()


def _compare_stats(label, got, want):
    if want["fallback"] == 0:
        assert got == want, (label, got, want)
    else:
        assert got["fallback"] == want["fallback"], (label, got, want)


@pytest.mark.parametrize("crop", [None, (5, 3, 7, 2)])
@pytest.mark.parametrize("S", (32, 512))
def test_one_file(hctx, S, crop):
    """Where the synchronous call fell back only `fallback` is compared: behind a work bound the asynchronous chain keeps
    launching the rounds the synchronous call stops at, so hop totals and round counts may differ there."""
    hctx.jpeg_huff_config(S)
    files = [(label, js.stream(label).data) for label in UPLOADS] + [("photo 120x88 s%d" % s, _photo(s)) for s in (0, 1, 2)]
    for label, data in files:
        for variant in (3, 4):
            want, st_want = _sync(hctx, 1, data, variant, crop)
            hctx.upload_jpeg_file_async(0, data, variant, crop)
            state = _poll_until_there(hctx, 0)
            st = hctx.jpeg_async_finish(0)
            assert hctx.jpeg_async_poll(0) in (1, 2), label
            assert (state == 1) == (st["fallback"] == 0), (label, state, st)
            got = hctx.download_level(0, 0)
            assert got.shape == want.shape, (label, got.shape, want.shape)
            assert np.array_equal(got, want), (label, S, variant, int(np.count_nonzero(got != want)))
            _compare_stats((label, S, variant), st, st_want)
            assert hctx.jpeg_huff_stats() == st_want, label      # still "the latest synchronous file"


def test_several_in_flight():
    """four files of different sizes and samplings started back to back, finished out of order; then once more with the
    files moved on by one slot, so that every working set is reused by a file of another size"""
    from iceberg_tracking_code_amd import Context
    files = [("big-interval b 444 528x512", js.stream("big-interval b 444 528x512").data), ("photo 120x88 420", _photo(2)),
             ("ri-1 420 256x256", js.stream("ri-1 420 256x256").data),
             ("flat black 420 736x736", js.stream("flat black 420 736x736").data)]
    with Context(1024, 768, n_slots=6, max_pts=1 << 12) as ctx:
        ctx.jpeg_huff_config(32)
        want = [_sync(ctx, 4, data) for _, data in files]
        fallbacks = [st["fallback"] for _, st in want]
        print(dict(zip((label for label, _ in files), fallbacks)))
        assert any(f == 0 for f in fallbacks) and any(f != 0 for f in fallbacks), fallbacks
        for shift in (0, 1):
            in_slot = [(k + shift) % 4 for k in range(4)]      # the file slot k gets
            for k in range(4):
                ctx.upload_jpeg_file_async(k, files[in_slot[k]][1])
            stats = {}
            for k in (2, 0, 3, 1):
                stats[k] = ctx.jpeg_async_finish(k)
            for k in range(4):
                label, (px, st_want) = files[in_slot[k]][0], want[in_slot[k]]
                got = ctx.download_level(k, 0)
                assert got.shape == px.shape and np.array_equal(got, px), (label, shift, k)
                _compare_stats((label, shift, k), stats[k], st_want)
        ctx.sync()


def test_the_callers_buffer_is_free(hctx):
    decoded, falls_back = _photo(2), js.stream("flat black 420 736x736").data
    hctx.jpeg_huff_config(32)
    seen = set()
    for data in (decoded, falls_back):
        want, st_want = _sync(hctx, 1, data)
        buf = bytearray(data)
        hctx.upload_jpeg_file_async(0, buf)
        buf[:] = bytes(len(buf))
        st = hctx.jpeg_async_finish(0)
        assert np.array_equal(hctx.download_level(0, 0), want)
        _compare_stats(len(data), st, st_want)
        seen.add(st["fallback"] != 0)
    assert seen == {False, True}      # one on the device, one by the host decoder from the library's copy


def _outcome(fn):
    """("ok", pixels) or ("raised", exception class)"""
    try:
        return "ok", fn()
    except Exception as e:      # noqa: BLE001 -- the class is what is compared
        return "raised", type(e)


def _async_whole(ctx, slot, data):
    ctx.upload_jpeg_file_async(slot, data)
    ctx.jpeg_async_finish(slot)
    return ctx.download_level(slot, 0)


def _damaged():
    photo = _photo(2)
    sos = photo.index(b"\xff\xda")
    begin, end = sos + 2 + int.from_bytes(photo[sos + 2:sos + 4], "big"), photo.rindex(b"\xff\xd9")
    flipped = bytearray(photo)
    rng = np.random.default_rng(77)
    for _ in range(100):
        flipped[int(rng.integers(begin, end))] ^= int(rng.integers(1, 256))
    return photo, [("truncated", photo[:len(photo) // 2]), ("100 bytes flipped", bytes(flipped))]


@pytest.mark.parametrize("S", (32, 512))
def test_damaged_files(hctx, S):
    """wherever the error surfaces, start or finish, it is the synchronous call's; afterwards the slot takes a frame and
    the next file is right"""
    hctx.jpeg_huff_config(S)
    photo, cases = _damaged()
    good, _ = _sync(hctx, 1, photo)
    frame = jc.photo(64, 48, 3)
    for label, data in cases:
        kind_want, want = _outcome(lambda: _sync(hctx, 1, data)[0])
        kind, got = _outcome(lambda: _async_whole(hctx, 0, data))
        print(label, S, kind_want, want if kind_want == "raised" else "")
        assert kind == kind_want, (label, kind, got, kind_want, want)
        if kind == "raised":
            assert got is want, (label, got, want)
        else:
            assert np.array_equal(got, want), label
        hctx.upload_bgr(0, frame)
        hctx.upload_bgr(1, frame)
        assert np.array_equal(hctx.download_level(0, 0), hctx.download_level(1, 0))
        assert np.array_equal(_async_whole(hctx, 0, photo), good), label


def test_unsupported_file_and_busy_slot(hctx):
    from PIL import Image
    from iceberg_tracking_code_amd import IcelkError, UnsupportedJpeg
    buf = io.BytesIO()
    Image.fromarray(jc.photo(40, 30, 3)).save(buf, "JPEG", progressive=True)
    with pytest.raises(UnsupportedJpeg):
        hctx.upload_jpeg_file_async(0, buf.getvalue())
    photo, other = _photo(2), _photo(0)
    want, _ = _sync(hctx, 1, photo)
    hctx.upload_jpeg_file_async(0, photo)
    with pytest.raises(IcelkError, match="-5"):
        hctx.upload_jpeg_file_async(0, other)
    with pytest.raises(IcelkError, match="-5"):
        hctx.upload_bgr(0, jc.photo(64, 48, 3))          # no other upload takes the slot from the file either
    hctx.jpeg_async_finish(0)
    assert np.array_equal(hctx.download_level(0, 0), want)
    with pytest.raises(IcelkError, match="-5"):
        hctx.jpeg_async_finish(0)                          # nothing in flight any more


# ---- the tracker ---------------------------------------------------------------------------------------------------------
TRACKER_BOUNDS = dict(subseq_bits=32, max_hops=160, max_rounds=8)
FP = dict(maxCorners=200, qualityLevel=0.007, minDistance=10, blockSize=10)
LK = dict(winSize=(21, 21), maxLevel=2, criteria=(3, 30, 0.01))


def _rgb(g):
    return np.stack([g, np.roll(g, 1, 1), np.roll(g, 1, 0)], 2)


def _pil_bytes(rgb, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", **kw)
    return buf.getvalue()


@pytest.fixture(scope="module")
def tracker_case(synth):
    """Eleven frames as bytes, frame 4 black, and what a tracker fed by `push_jpeg` makes of them.  The black frame of an
    encoder is the easiest of all files for the lanes (it decodes under any bound), so the fallback inside the pipeline
    comes from the work bound instead: at 160 hops some of the noise frames decode on the device and some do not --
    which, the synchronous run says."""
    from iceberg_tracking_code_amd import SegmentTracker
    grays, _ = synth.sequence(320, 240, 11, seed=31, max_step_px=2.0)
    files = [_pil_bytes(np.zeros((240, 320, 3), np.uint8) if k == 4 else _rgb(g), quality=95) for k, g in enumerate(grays)]
    trk = SegmentTracker(320, 240, 2, FP, LK, max_pts=4096)
    trk.ctx.jpeg_huff_config(**TRACKER_BOUNDS)
    want, fallbacks = [], []
    for data in files:
        seg = trk.push_jpeg(data)
        fallbacks.append(trk.ctx.jpeg_huff_stats()["fallback"])
        if seg is not None:
            want.append(seg)
    trk.close()
    print("fallbacks of the frames:", fallbacks)
    assert any(f == 0 for f in fallbacks) and any(f != 0 for f in fallbacks), fallbacks
    assert len(want) == 5 and sum(len(t) for _, t, _ in want) > 300
    return files, want


def _same_segments(got, want):
    assert [g[0] for g in got] == [w[0] for w in want]
    for (_, ta, qa), (_, tb, qb) in zip(got, want):
        assert ta.shape == tb.shape and np.array_equal(ta, tb) and np.array_equal(qa, qb)


@pytest.mark.parametrize("n_slots,use_on_close", [(5, False), (4, False), (5, True)])
def test_tracker_fed_by_prefetch_jpeg(tracker_case, n_slots, use_on_close):
    """n_slots - 2 files kept ahead: three with five slots, two with four, where a slot is refilled while the frame before
    it is still being tracked; once with the segments collected through on_close and no wait at all"""
    from iceberg_tracking_code_amd import SegmentTracker
    files, want = tracker_case
    trk = SegmentTracker(320, 240, 2, FP, LK, max_pts=4096, n_slots=n_slots)
    ctx = trk.ctx
    ctx.jpeg_huff_config(**TRACKER_BOUNDS)
    got = []
    if use_on_close:
        trk.on_close = lambda first, closed: got.append((first,) + ctx.seg_read(closed=closed))
    fed = 0
    for k in range(len(files)):
        while fed < len(files) and fed - k < n_slots - 2:
            trk.prefetch_jpeg(files[fed])
            fed += 1
        seg = trk.push_prefetched(wait=not use_on_close)
        if seg is not None:
            got.append(seg)
    trk.flush()
    ctx.sync()
    trk.close()
    _same_segments(got, want)


def test_failed_file_is_replaced_and_abort_drops_jobs(tracker_case):
    from PIL import Image
    from iceberg_tracking_code_amd import SegmentTracker
    files, want = tracker_case
    trk = SegmentTracker(320, 240, 2, FP, LK, max_pts=4096, n_slots=5)
    trk.ctx.jpeg_huff_config(**TRACKER_BOUNDS)
    got = []
    for k in range(4):
        # frame 1 arrives as a file cut in the scan: of the photo's size it is not, but it never gets that far
        data = files[k][:len(files[k]) // 2] if k == 1 else files[k]
        try:
            trk.prefetch_jpeg(data)
            seg = None
            try:
                seg = trk.push_prefetched()
            except ValueError:
                assert k == 1
                trk.replace_prefetched_bgr(np.array(Image.open(io.BytesIO(files[k]))))
                seg = trk.push_prefetched()
        except ValueError:
            assert k == 1                                   # the host saw it at the start: no slot was taken
            trk.prefetch_bgr(np.array(Image.open(io.BytesIO(files[k]))))
            seg = trk.push_prefetched()
        if seg is not None:
            got.append(seg)
    _same_segments(got, want[:1])
    trk.prefetch_jpeg(files[4])
    trk.prefetch_jpeg(files[5])
    assert trk.abort() == 4
    for s in (trk.prefetched[0], trk.prefetched[1]):
        trk.ctx.upload_bgr(s, np.zeros((240, 320, 3), np.uint8))     # the slots are nobody's any more
    trk.close()


# ---- the folder driver ---------------------------------------------------------------------------------------------------
def test_pipelined_folder_equals_the_plain_drivers(synth, tmp_path):
    """nine 720x540 photos, one saved progressive (PIL takes that file in every driver) and one black"""
    from iceberg_tracking_code_amd import track_image_sequence
    w, h, n, T, dts = 720, 540, 9, 2, 60
    grays, _ = synth.sequence(w, h, n, seed=31, max_step_px=2.0)
    src = tmp_path / "photos"
    src.mkdir()
    t0 = dt.datetime(2019, 7, 24, 10, 0, 0)
    names = []
    for k, g in enumerate(grays):
        t = t0 + dt.timedelta(seconds=k * dts + (30 if k == 5 else 0))
        p = src / (t.strftime("%Y%m%d-%H%M%S") + ".jpg")
        rgb = np.zeros((h, w, 3), np.uint8) if k == 6 else _rgb(g)
        p.write_bytes(_pil_bytes(rgb, quality=95, progressive=(k == 3)))
        names.append(str(p))
    crop = (24, 60, 16, 8)
    poly = [(40, 80), (700, 70), (690, 520), (300, 470), (50, 530)]
    fp = dict(maxCorners=400, qualityLevel=0.007, minDistance=10, blockSize=10)
    lk = dict(winSize=(21, 21), maxLevel=3, criteria=(3, 30, 0.01))
    runs = {}
    for name, kw in (("pipeline", dict(decoder="device", huffman="device", pipeline=True)),
                     ("device", dict(decoder="device", huffman="device")), ("pil", dict(decoder="pil"))):
        dst = tmp_path / name
        dst.mkdir()
        runs[name] = (track_image_sequence(names, str(dst), T, dts, startlist=(0, 1), crop=crop, mask_polygon=(poly, crop[0], crop[1]),
                                           feature_params=fp, lk_params=lk, decode_threads=3, **kw), sorted(os.listdir(dst)))
    got, got_files = runs["pipeline"]
    assert len(got) >= 4 and sum(len(t) for _, t, _ in got) > 300
    for other in ("device", "pil"):
        ref, ref_files = runs[other]
        assert got_files == ref_files, other
        assert [os.path.basename(p) for p, _, _ in got] == [os.path.basename(p) for p, _, _ in ref], other
        for (_, ta, qa), (_, tb, qb) in zip(got, ref):
            assert ta.shape == tb.shape and np.array_equal(ta, tb) and np.array_equal(qa, qb), other


# ---- the edges of the verdict, and the calls between start and finish -------------------------------------------------------
# No round count, hop count or fallback is written down below: the CPU statement of the lanes (`read_jpeg_lanes` under the
# same three parameters) and the synchronous call say them, and the asynchronous file has to agree with both.
GENEROUS = dict(max_hops=256, max_rounds=255)


def _bgr_gray(ctx, slot, key, rgb):
    """what `upload_bgr` makes of a file's Pillow pixels: right without any decoder of this project; once per file"""
    if key not in _bgr_gray.cache:
        ctx.upload_bgr(slot, rgb)
        _bgr_gray.cache[key] = ctx.download_level(slot, 0)
    return _bgr_gray.cache[key]


_bgr_gray.cache = {}


def _pillow_of(label):
    """the decoded pixels of a catalogue stream an 8-bit encoder can make, else None"""
    return js.pillow(label) if js.stream(label).tier == "pixels" else None


def _three_way(ctx, label, data, S, max_hops, max_rounds, rgb=None, slots=(0, 1, 2)):
    """The file under one configuration by the asynchronous call, the synchronous call and the CPU statement: `fallback`
    always agrees, every field where nothing fell back, pixels always; against `upload_bgr(rgb)` too where the file's
    pixels are Pillow's business.  Returns the CPU statement's fallback."""
    from iceberg_tracking_code_amd import read_jpeg_lanes
    a, s, b = slots
    ctx.jpeg_huff_config(S, max_hops, max_rounds)
    _, cpu = read_jpeg_lanes(data, S, max_hops, max_rounds)
    want, st_sync = _sync(ctx, s, data)
    ctx.upload_jpeg_file_async(a, data)
    st = ctx.jpeg_async_finish(a)
    got = ctx.download_level(a, 0)
    what = (label, S, max_hops, max_rounds)
    print(what, "cpu", cpu, "sync", st_sync, "async", st)
    assert st["fallback"] == st_sync["fallback"] == cpu["fallback"], (what, st, st_sync, cpu)
    if cpu["fallback"] == 0:
        assert st == cpu and st_sync == cpu, (what, st, st_sync, cpu)
    assert got.shape == want.shape and np.array_equal(got, want), (what, int(np.count_nonzero(got != want)))
    if rgb is not None:
        assert np.array_equal(got, _bgr_gray(ctx, b, label, rgb)), what
    return cpu["fallback"]


ROUND_FILES = ("flat black 420 531x397", "out-of-range 1023 q1 420 48x48", "flat black 420 736x736", "big-interval b 444 528x512")


def test_round_bound(hctx):
    """max_rounds one below, at and one above the rounds a file needs: the verdict kernel's `first_quiet <= max_rounds`"""
    from iceberg_tracking_code_amd import read_jpeg_lanes
    needs = {}
    for label in ROUND_FILES:
        data = js.stream(label).data
        _, st = read_jpeg_lanes(data, 32, **GENEROUS)
        R = needs[label] = st["rounds"]
        assert st["fallback"] == 0 and 2 <= R < 255, (label, st)
        outcome = {m: _three_way(hctx, label, data, 32, 256, m, _pillow_of(label)) for m in (R - 1, R, R + 1, 255)}
        assert outcome[R - 1] != 0 and outcome[R] == 0 and outcome[R + 1] == 0 and outcome[255] == 0, (label, R, outcome)
    print("rounds needed:", needs)
    assert any(R >= 4 for R in needs.values()) and any(R >= 16 for R in needs.values()), needs


def test_more_than_64_rounds():
    """a black 2112 x 2112 frame: 69 groups of lanes that hand their state on one group per round, so the verdict kernel's
    64 threads find the first quiet round in the second pass of their loop"""
    from iceberg_tracking_code_amd import Context, read_jpeg_lanes
    data = jc.encode(np.zeros((2112, 2112, 3), np.uint8), quality=85, subsampling=2)
    _, st = read_jpeg_lanes(data, 32, **GENEROUS)
    R = st["rounds"]
    print("2112x2112 black: %d bytes, %d lanes, R = %d" % (len(data), st["subsequences"], R))
    assert st["fallback"] == 0 and 64 < R < 255, st
    rgb = jc.pil_decode(data)
    with Context(2112, 2112, n_slots=3, max_pts=1 << 12) as ctx:
        outcome = {m: _three_way(ctx, "black 2112x2112", data, 32, 256, m, rgb) for m in (R - 1, R, 255)}
        ctx.sync()
    assert outcome[R - 1] != 0 and outcome[R] == 0 and outcome[255] == 0, (R, outcome)


def test_hop_bound(hctx):
    """max_hops around the longest chain of a file: the work bound of a chain, `hops >= max_hops`, as the verdict sees it"""
    from iceberg_tracking_code_amd import read_jpeg_lanes
    files = [("photo 120x88 420", _photo(2), jc.pil_decode(_photo(2)))]
    files += [(label, js.stream(label).data, _pillow_of(label)) for label in ("ri-edges ri-uneven", "ri-edges fill-rst")]
    longest = {}
    for label, data, rgb in files:
        _, st = read_jpeg_lanes(data, 32, **GENEROUS)
        M = longest[label] = st["max_hops"]
        assert st["fallback"] == 0 and 2 <= M < 255 and 1 < st["rounds"] <= 8, (label, st)
        outcome = {m: _three_way(hctx, label, data, 32, m, 8, rgb) for m in (M - 1, M, M + 1, M + 2)}
        assert outcome[M - 1] != 0 and outcome[M] != 0 and outcome[M + 1] == 0 and outcome[M + 2] == 0, (label, M, outcome)
    print("longest chains:", longest)


def _right(ctx, slot, free_slot, label, px, rgb):
    """the slot holds `px`, which is also what Pillow's pixels give"""
    got = ctx.download_level(slot, 0)
    assert got.shape == px.shape and np.array_equal(got, px), label
    assert np.array_equal(got, _bgr_gray(ctx, free_slot, label, rgb)), label


def test_between_start_and_finish():
    """a configuration change and a synchronous file between the start and the finish of asynchronous ones: every file is
    decoded under the configuration at its start, in its own working set"""
    from iceberg_tracking_code_amd import Context
    c1, c2 = (32, 256, 8), (512, 256, 8)
    A = ("photo 120x88 420", _photo(2), jc.pil_decode(_photo(2)))
    B = ("flat black 420 736x736", js.stream("flat black 420 736x736").data, js.pillow("flat black 420 736x736"))
    Cf = ("big-interval b 444 528x512", js.stream("big-interval b 444 528x512").data, js.pillow("big-interval b 444 528x512"))
    with Context(1024, 768, n_slots=6, max_pts=1 << 12) as ctx:
        want = {}
        for name, f, cfg in (("A1", A, c1), ("B1", B, c1), ("A2", A, c2), ("C2", Cf, c2)):
            ctx.jpeg_huff_config(*cfg)
            want[name] = _sync(ctx, 4, f[1])
        print({name: st["fallback"] for name, (_, st) in want.items()})
        assert sorted([want["A1"][1]["fallback"] != 0, want["B1"][1]["fallback"] != 0]) == [False, True], want
        ctx.jpeg_huff_config(*c1)
        ctx.upload_jpeg_file_async(0, A[1])
        ctx.upload_jpeg_file_async(2, B[1])
        ctx.jpeg_huff_config(*c2)
        ctx.upload_jpeg_file(1, Cf[1])
        ctx.upload_jpeg_file_async(3, A[1])
        stats = {k: ctx.jpeg_async_finish(k) for k in (3, 2, 0)}
        assert ctx.jpeg_huff_stats() == want["C2"][1]
        for slot, name, f in ((0, "A1", A), (2, "B1", B), (1, "C2", Cf), (3, "A2", A)):
            _right(ctx, slot, 5, f[0], want[name][0], f[2])
            if slot != 1:
                _compare_stats((name, slot), stats[slot], want[name][1])
        ctx.sync()


def test_sync_and_close_with_files_in_flight():
    from iceberg_tracking_code_amd import Context
    files = [("photo 120x88 420", _photo(2), jc.pil_decode(_photo(2)))]
    files += [(label, js.stream(label).data, js.pillow(label)) for label in ("flat black 420 736x736", "ri-1 420 256x256")]
    with Context(1024, 768, n_slots=6, max_pts=1 << 12) as ctx:
        ctx.jpeg_huff_config(32)
        want = [_sync(ctx, 4, data) for _, data, _ in files]
        for k, (_, data, _) in enumerate(files):
            ctx.upload_jpeg_file_async(k, data)
        ctx.sync()
        states = [ctx.jpeg_async_poll(k) for k in range(3)]       # one look each: the decode streams are the handle's
        assert all(s in (1, 2) for s in states), states
        for k, (label, _, rgb) in enumerate(files):
            st = ctx.jpeg_async_finish(k)
            assert (states[k] == 1) == (st["fallback"] == 0), (label, states[k], st)
            _compare_stats(label, st, want[k][1])
            _right(ctx, k, 5, label, want[k][0], rgb)
        for k, (_, data, _) in enumerate(files):
            ctx.upload_jpeg_file_async(k, data)
        # nobody finishes these: close() waits for them
    with Context(1024, 768, n_slots=3, max_pts=1 << 12) as ctx:
        ctx.jpeg_huff_config(32)
        for label, data, rgb in files:
            px, _ = _sync(ctx, 1, data)
            assert np.array_equal(_async_whole(ctx, 0, data), px), label
            _right(ctx, 0, 2, label, px, rgb)
        ctx.sync()


def test_start_calls_that_fail_late(hctx):
    """errors that a start call finds after the host's share (index and lanes) is done leave no job owning the slot; with
    another file in flight beside them"""
    from iceberg_tracking_code_amd import IcelkError
    photo, rgb = _photo(2), jc.pil_decode(_photo(2))
    other, other_rgb = js.stream("ri-1 420 256x256").data, js.pillow("ri-1 420 256x256")
    good, _ = _sync(hctx, 1, photo)
    beside, st_beside = _sync(hctx, 1, other)
    frame = jc.photo(64, 48, 3)
    hctx.upload_bgr(1, frame)
    frame_gray = hctx.download_level(1, 0)
    cases = [("larger than the context", js.stream("big-interval c 420 1056x1024 ri4100").data, None),
             ("one component", js.stream("big-interval a gray 1032x512").data, None),
             ("a crop that leaves less than nothing", photo, (70, 0, 60, 0))]
    hctx.upload_jpeg_file_async(2, other)
    for label, data, crop in cases:
        kind_want, want = _outcome(lambda: hctx.upload_jpeg_file(1, data, 4, crop))
        kind, got = _outcome(lambda: hctx.upload_jpeg_file_async(0, data, 4, crop))
        print(label, kind_want, want, kind, got)
        assert kind_want == "raised" and kind == "raised" and got is want, (label, kind, got, kind_want, want)
        hctx.upload_bgr(0, frame)                                     # no job was left owning the slot
        assert np.array_equal(hctx.download_level(0, 0), frame_gray), label
        with pytest.raises(IcelkError, match="-5"):
            hctx.jpeg_async_finish(0)
        assert np.array_equal(_async_whole(hctx, 0, photo), good), label
    st = hctx.jpeg_async_finish(2)
    _compare_stats("beside", st, st_beside)
    _right(hctx, 2, 1, "ri-1 420 256x256", beside, other_rgb)
    _right(hctx, 0, 1, "photo 120x88 420", good, rgb)
