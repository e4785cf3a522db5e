"""The tuned tracker's same-cell arm (k_lk_fast.hip: an iteration whose window origin has the pixel cell of the iteration
before it keeps that iteration's widened tile rows) against the oracle, bit for bit, on small frames of smooth texture.

Every case first shows ON THE CPU, from tests/np_restatement.py alone, that its inputs reach the arm it is named for at
least 20 times: the restatement's `_floor` is wrapped so that every origin it floors lands, with the trace's notes, in one
stream of events, and `arms` walks that stream with the kernel's tile rule (staged at the first origin of a level pass
with kLkTileMargin pixels around it, restaged when an origin leaves it).  Only then is the kernel run."""
import numpy as np
import pytest

import np_restatement as npr

pytestmark = pytest.mark.gpu

CRIT = (3, 30, 0.01)
R = 1                        # kLkTileMargin (csrc/icelk_internal.h)
KEYS_FB = ("p1", "p0r", "st_fwd", "st_bwd", "err_fwd", "err_bwd", "dist", "valid")
EXITS = ("zero_iter", "outside_first", "outside_iter", "eps", "oscillation", "count")


# ---------------------------------------------------------------------------------------------- frames
def texture(w, h, seed, radius=3):
    """Blurred noise (three box passes each way ~ a Gaussian), stretched to the full grey range."""
    rng = np.random.default_rng(seed)
    a = rng.random((h + 6 * radius, w + 6 * radius))
    k = 2 * radius + 1
    for _ in range(3):
        c = np.cumsum(np.pad(a, ((0, 0), (1, 0))), 1)
        a = (c[:, k:] - c[:, :-k]) / k
        c = np.cumsum(np.pad(a, ((1, 0), (0, 0))), 0)
        a = (c[k:] - c[:-k]) / k
    a = a[:h, :w]
    return np.ascontiguousarray(np.clip(np.rint((a - a.min()) / (a.max() - a.min()) * 255.0), 0, 255).astype(np.uint8))


def shifted_pair(w, h, seed, dx, dy, radius=3):
    """Two crops of one canvas: the content of the second frame is the first's moved by (dx, dy) whole pixels."""
    m = 8
    big = texture(w + 2 * m, h + 2 * m, seed, radius)
    return (np.ascontiguousarray(big[m:m + h, m:m + w]), np.ascontiguousarray(big[m - dy:m - dy + h, m - dx:m - dx + w]))


def interior_points(w, h, n, seed, border=24):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(border, w - border, n), rng.uniform(border, h - border, n)], 1).astype(np.float32)


# ---------------------------------------------------------------------------------------------- arms, on the CPU
class _Events(list):
    """The `trace` list of np_restatement.pyrlk; the wrapped _floor appends to it as well."""


def restatement_events(f0, f1, pts, win, level):
    ev = _Events()
    inner = npr._floor

    def floor(v):
        i = inner(v)
        ev.append(("floor", i))
        return i

    npr._floor = floor
    try:
        res = npr.track_fb(f0, f1, pts, win, level, CRIT, trace=ev)
    finally:
        npr._floor = inner
    return res, ev


def arms(ev, win):
    """Counts of what the kernel's iteration loop does with each origin the restatement floored."""
    pitch = ((win[0] + 1 + 2 * R + 2) // 4 + 1) * 4          # Cfg::JPD * 4
    n = dict.fromkeys(("iterations", "first", "same", "move_x", "move_y", "move_xy", "restage", "same_after_restage",
                       "restage_same_jb_vertical", "restage_same_jb_x4", "aba", "exit_after_same", "outside_after_same",
                       "level_shares_cell", "first_at_cell_0_0"), 0)
    state, pend, cells, kinds, tile, last_cell_of_pass, point = "T", [], [], [], None, None, None
    for e in ev:
        if e[0] == "floor":
            pend.append(e[1])
            if len(pend) < 2:
                continue
            cell, pend = tuple(pend), []
            if state == "T":
                state, cells, kinds, tile = "ITER", [], [], None
            elif state == "ERR":
                state = "T"
            else:
                n["iterations"] += 1
                if not cells:
                    kind = "first"
                    tile = (cell[0] - R, cell[1] - R)          # staged with the level, at this origin
                    if cell == last_cell_of_pass:
                        n["level_shares_cell"] += 1
                    if cell == (0, 0):
                        n["first_at_cell_0_0"] += 1
                elif cell == cells[-1]:
                    kind = "same"
                    if kinds[-1] == "restage":
                        n["same_after_restage"] += 1
                else:
                    dx, dy = cell[0] - cells[-1][0], cell[1] - cells[-1][1]
                    if 0 <= cell[0] - tile[0] <= 2 * R and 0 <= cell[1] - tile[1] <= 2 * R:
                        kind = "move_xy" if dx and dy else ("move_x" if dx else "move_y")
                    else:
                        kind = "restage"
                        jb0 = (cells[-1][1] - tile[1]) * pitch + (tile[0] & 3) + cells[-1][0] - tile[0]
                        tile = (cell[0] - R, cell[1] - R)
                        if jb0 == R * pitch + (tile[0] & 3) + R:
                            if dx == 0:
                                n["restage_same_jb_vertical"] += 1
                            elif dx % 4 == 0:
                                n["restage_same_jb_x4"] += 1
                    if len(cells) >= 2 and cell == cells[-2]:
                        n["aba"] += 1
                n[kind] += 1
                cells.append(cell)
                kinds.append(kind)
            continue
        i, level, tag = e
        if i != point:
            point, last_cell_of_pass = i, None
        if tag in ("outside", "mineig", "det"):
            state = "T"
        elif tag in EXITS:
            # the last origin floored belongs to the iteration that left the level
            if len(kinds) >= 2 and kinds[-2] == "same":
                n["exit_after_same"] += 1
                if tag == "outside_iter":
                    n["outside_after_same"] += 1
            last_cell_of_pass = cells[-1] if cells else None
            state = "ERR" if level == 0 and tag not in ("outside_first", "outside_iter") else "T"
    return n


# ---------------------------------------------------------------------------------------------- the kernel
@pytest.fixture(scope="module")
def gctx():
    from iceberg_tracking_code_amd import Context
    c = Context(320, 240, n_slots=2, max_pts=4096)
    yield c
    c.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_fb(got, ref, tag):
    for k in KEYS_FB:
        assert np.array_equal(_bits(got[k]).ravel(), _bits(ref[k]).ravel()), (tag, k)


def _kernel_equals_oracle(gctx, orc, f0, f1, pts, win, level, tag):
    assert f0.shape == (240, 320) and len(pts) <= 500
    gctx.upload_gray(0, f0)
    gctx.upload_gray(1, f1)
    ref = orc.track_fb(f0, f1, pts, win, level, CRIT)
    _same_fb(gctx.track_fb(0, 1, pts, win, level, CRIT), ref, tag)
    return ref


# name -> (shift of the second frame's content, maxLevel, blur radius, contrast of the second frame, the arms it is named for)
W, H, NPTS = 320, 240, 400
SCENES = {
    # a step of about a pixel, then the estimate settles inside one cell: the common arm
    "same_cell": ((1, 1), 0, 3, 1.0, ("same",)),
    # two pixels each way: the estimate crosses cells in x, in y and in both under one staged tile
    "cell_changes": ((2, -2), 1, 3, 1.0, ("move_x", "move_y", "move_xy", "same", "exit_after_same")),
    # further than the tile's margin at the finest level: restaged, then iterated in place
    "leaves_tile": ((4, 3), 0, 4, 1.0, ("restage", "same_after_restage")),
    # the same, straight down: the restaged tile has the byte offset the old one had
    "leaves_tile_vertical": ((0, 4), 0, 4, 1.0, ("restage_same_jb_vertical", "same_after_restage")),
    # ... and four columns along
    "leaves_tile_x4": ((5, 0), 0, 5, 1.0, ("restage_same_jb_x4", "same_after_restage")),
    # A -> B -> A: a second frame of higher contrast makes every step overshoot, and points at whole pixels put the
    # answer's window origin on a cell boundary, which the estimate then crosses back and forth
    "a_b_a": ((1, 0), 0, 3, 1.7, ("aba", "same")),
}


def scene(name):
    k = list(SCENES).index(name)
    shift, level, radius, gain, _ = SCENES[name]
    f0, f1 = shifted_pair(W, H, 100 + k, shift[0], shift[1], radius)
    pts = interior_points(W, H, NPTS, 7 + k)
    if gain != 1.0:
        f1 = np.ascontiguousarray(np.clip(np.rint((f1.astype(np.float64) - 128.0) * gain + 128.0), 0, 255).astype(np.uint8))
        jitter = np.random.default_rng(k).uniform(-0.04, 0.04, pts.shape)
        pts = (np.rint(pts) + jitter).astype(np.float32)
    return f0, f1, pts, level


@pytest.fixture(scope="module")
def scenes():
    return {name: scene(name) for name in SCENES}


@pytest.mark.parametrize("win", [(21, 21), (15, 15)])
@pytest.mark.parametrize("name", list(SCENES))
def test_arms_of_the_iteration(gctx, orc, scenes, name, win):
    f0, f1, pts, level = scenes[name]
    res, ev = restatement_events(f0, f1, pts, win, level)
    n = arms(ev, win)
    print(name, win, n)
    for arm in SCENES[name][4]:
        assert n[arm] >= 20, (name, win, arm, n)
    ref = _kernel_equals_oracle(gctx, orc, f0, f1, pts, win, level, (name, win))
    _same_fb(res, ref, (name, win, "restatement"))
    assert ref["valid"].sum() > len(pts) // 4


def corner_case():
    f0, f1 = shifted_pair(W, H, 300, 0, 0)
    # the second frame: the first with a little noise, so that there is something to iterate on
    noise = np.random.default_rng(5).integers(-6, 7, f1.shape)
    f1 = np.ascontiguousarray(np.clip(f1.astype(np.int64) + noise, 0, 255).astype(np.uint8))
    off = np.array([(x, y) for y in (0.0, 0.4, 0.9, 1.3, 1.75, 2.0) for x in (0.0, 0.3, 0.8, 1.2, 1.6, 2.0)], np.float32)
    return f0, f1, np.concatenate([off, np.float32([W - 1, H - 1]) - off])


def edge_case():
    f0, _ = shifted_pair(W, H, 500, 0, 0, 4)
    # the second frame: columns pulled to the right by an amount that grows towards the right edge
    x = np.arange(W, dtype=np.float64)
    src = np.clip(np.rint(x - 0.9 * np.clip((x - 200) / 20.0, 0, None) ** 1.5), 0, W - 1).astype(np.intp)
    f1 = np.ascontiguousarray(f0[:, src])
    rng = np.random.default_rng(3)
    return f0, f1, np.stack([rng.uniform(W - 16, W - 1, 300), rng.uniform(30, H - 30, 300)], 1).astype(np.float32)


@pytest.mark.parametrize("win", [(21, 21), (15, 15)])
def test_frame_corners_share_the_cell_from_level_to_level(gctx, orc, win):
    """Points within 2 px of (0, 0) and of the far corner, four levels: near (0, 0) the window origin is -(win - 1) / 2 at
    every level, so a level's first iteration has the cell of the last one of the level above (it must fetch all the same),
    and every tile goes through the reflecting loader."""
    f0, f1, pts = corner_case()
    res, ev = restatement_events(f0, f1, pts, win, 3)
    n = arms(ev, win)
    print(win, n)
    assert n["level_shares_cell"] >= 20 and n["same"] >= 20, n
    ref = _kernel_equals_oracle(gctx, orc, f0, f1, pts, win, 3, ("corners", win))
    _same_fb(res, ref, ("corners", win, "restatement"))
    assert ref["st_fwd"].sum() >= 20


@pytest.mark.parametrize("win", [(21, 21), (15, 15)])
def test_points_no_cell_can_hold(gctx, orc, win):
    """NaN, +-inf, +-2^29, +-2^31 in either coordinate (their floors are the ints a marker for "no cell yet" could have been:
    INT_MAX, INT_MIN, -2^29), and points whose first origin floors to (0, 0), the value the cell starts from: the first
    iteration of a level takes the full arm whatever the cell, origin test included."""
    f0, f1 = shifted_pair(W, H, 400, 1, 0)
    hx, hy = (win[0] - 1) * 0.5, (win[1] - 1) * 0.5
    wild = [np.nan, np.inf, -np.inf, 2.0 ** 29, -2.0 ** 29, 2.0 ** 31, -2.0 ** 31, -2.0 ** 29 + hx, 2.0 ** 31 - 128]
    pts = [(v, 100.25) for v in wild] + [(150.5, v) for v in wild] + [(v, v) for v in wild]
    pts += [(hx + fx, hy + fy) for fx in (0.0, 0.25, 0.9) for fy in (0.0, 0.5, 0.9)]
    pts = np.array(pts, np.float32)
    gctx.upload_gray(0, f0)
    gctx.upload_gray(1, f1)
    for level in (0, 3):
        got = gctx.pyrlk(0, 1, pts, None, win, level, CRIT)
        ref = orc.pyrlk(f0, f1, pts, None, win, level, CRIT)
        for g, r, what in zip(got, ref, ("nextPts", "status", "err")):
            assert np.array_equal(_bits(g).ravel(), _bits(r).ravel()), (win, level, what)
        st = ref[1].ravel()
        assert st[:3 * len(wild)].sum() == 0 and st[3 * len(wild):].sum() == 9, st
        fb, rb = gctx.track_fb(0, 1, pts, win, level, CRIT), orc.track_fb(f0, f1, pts, win, level, CRIT)
        for k in KEYS_FB:
            if k == "dist":      # |inf - inf| makes a NaN, and x86 and the device make different ones (test_gpu_lk_floors.py)
                assert np.array_equal(np.isnan(fb[k]), np.isnan(rb[k])), (win, level, k)
                keep = ~np.isnan(rb[k])
                assert np.array_equal(_bits(fb[k])[keep], _bits(rb[k])[keep]), (win, level, k)
            else:
                assert np.array_equal(_bits(fb[k]).ravel(), _bits(rb[k]).ravel()), (win, level, k)


def test_first_origin_at_cell_0_0_is_reached():
    """The CPU half of the (0, 0) points above: their first iteration does floor to the cell the kernel's cell starts from."""
    f0, f1 = shifted_pair(W, H, 400, 1, 0)
    pts = np.array([(10.0 + fx, 10.0 + fy) for fx in (0.0, 0.25, 0.9) for fy in (0.0, 0.5, 0.9)] * 3, np.float32)
    _, ev = restatement_events(f0, f1, pts, (21, 21), 0)
    n = arms(ev, (21, 21))
    assert n["first_at_cell_0_0"] >= 20, n


def test_leaving_the_level_after_a_same_cell_iteration(gctx, orc):
    """A level left in an iteration that follows a same-cell one, by every way out: eps, oscillation and the count as in
    test_arms_of_the_iteration's cases, and -- content pulled towards the right edge, points beside that edge -- the search
    window leaving the level (the origin test the same-cell arm skips must still run for the cell that fails it)."""
    f0, f1, pts = edge_case()
    res, ev = restatement_events(f0, f1, pts, (21, 21), 0)
    n = arms(ev, (21, 21))
    print(n)
    assert n["exit_after_same"] >= 20 and n["outside_after_same"] >= 10, n
    ref = _kernel_equals_oracle(gctx, orc, f0, f1, pts, (21, 21), 0, "leaves level")
    _same_fb(res, ref, "leaves level, restatement")


def test_segments_hand_over_and_joint_launch(orc):
    """Two segments of two pairs through SegmentTracker: the hand-over pass (stored templates) and the joint launch of two
    pairs run the iteration loop with the kept pairs.  Against the reference loop on the oracle."""
    from iceberg_tracking_code_amd import Context, SegmentTracker
    from reference_loops import OracleCv, run_reference_loop
    m = 12
    big = texture(W + 2 * m, H + 2 * m, 600, 3)
    frames = [np.ascontiguousarray(big[m - k:m - k + H, m + 2 * k:m + 2 * k + W]) for k in range(5)]
    fp = dict(maxCorners=300, qualityLevel=0.005, minDistance=6, blockSize=5)
    lk = dict(winSize=(21, 21), maxLevel=3, criteria=CRIT)
    ref = run_reference_loop(frames, 2, fp, lk, cv=OracleCv(orc))
    assert len(ref) == 2 and len(ref[0][1]) > 100
    ctx = Context(W, H, n_slots=len(frames), max_pts=4096)
    try:
        for i, f in enumerate(frames):
            ctx.upload_gray(i, f)
        trk = SegmentTracker(W, H, 2, fp, lk, ctx=ctx)
        got = []
        trk.on_close = lambda first, closed: got.append((first,) + ctx.seg_read(closed=closed))
        ctx.prof_enable(True)
        for i in range(len(frames)):
            trk.push_slot(i, False, *[i + k if i + k < len(frames) else None for k in range(1, 7)])
        trk.flush()
        ctx.sync()
        assert ctx.prof_table().get("lk_fb_pair", {}).get("launches", 0) >= 1
    finally:
        ctx.close()
    assert len(got) == 2
    for (gf, gt, gq), (rf, rt, rq) in zip(got, ref):
        rt = np.asarray(rt, np.float32).reshape(len(rt), -1, 2)
        rq = np.asarray(rq, np.float32).reshape(len(rq), -1)
        assert gf == rf and gt.shape == rt.shape
        assert np.array_equal(_bits(gt), _bits(rt)) and np.array_equal(_bits(gq), _bits(rq))


@pytest.mark.parametrize("form", ["31x31", "35x35", "lk_sums", "lk_wide_sums"])
def test_forms_that_keep_the_full_arm(gctx, orc, scenes, form):
    """The windows with several segments per lane and the named sum variants fetch and widen in every iteration, as before."""
    f0, f1, pts, _ = scenes["cell_changes"]
    win = {"31x31": (31, 31), "35x35": (35, 35)}.get(form, (21, 21))
    gctx.upload_gray(0, f0)
    gctx.upload_gray(1, f1)
    if form in ("lk_sums", "lk_wide_sums"):
        gctx.set_variant(form, 1)
    try:
        got = gctx.track_fb(0, 1, pts, win, 2, CRIT)
    finally:
        if form in ("lk_sums", "lk_wide_sums"):
            gctx.set_variant(form, 0)
    if form == "lk_sums":
        with orc.variants(lk_sums=1):
            ref = orc.track_fb(f0, f1, pts, win, 2, CRIT)
    else:
        ref = orc.track_fb(f0, f1, pts, win, 2, CRIT)
    _same_fb(got, ref, form)
    assert ref["valid"].sum() > len(pts) // 4
