"""The tuned tracker's pair chain (lk_common.h, "two guarded sums as one chain": b1 and b2 of an iteration, a11 and a22 of a
template reduced in ONE register through v_permlane32_swap_b32, totals in lanes 31 and 63).

1. tests/sum_chain_main.hip, a program of its own, runs the helpers on the device one wave per case against 64-bit sums
   of the host: a value in a single lane (every lane, either input), every lane at the guard's limits, a few thousand
   random vectors inside the guard.  Built here, run as a child under a time limit.
2. The kernels against the oracle, bit for bit, through track_fb on frames of 160 x 120 with 12 interior points, at
   maxLevel 0 and 1 and all four tuned windows, on scenes where a mix-up of the two sums, or of the wave's halves, shows.
   Every case first shows ON THE CPU (tests/np_restatement.py, its `_bilinear` wrapped; the lane layout of Cfg<WW, WH>
   restated below) that it does what it is named for: at least 20 iterations whose lane partials pass the guard and whose
   two totals differ -- a case that never reaches the narrow arm, or cannot tell the sums apart, fails instead of passing.
3. One segment case: two segments through SegmentTracker (joint launch, template hand-over) against the reference loop."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import extreme_frames as xf
import np_restatement as npr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "sum_chain_main.hip")
CSRC = os.path.join(ROOT, "iceberg_tracking_code_amd", "csrc")

CRIT = (3, 30, 0.01)
W, H, NPTS = 160, 120, 12
WINDOWS = [(15, 15), (21, 21), (31, 31), (35, 35)]
KEYS_FB = ("p1", "p0r", "st_fwd", "st_bwd", "valid")
GUARD_BIAS, GUARD = 1 << 25, 1 << 26           # kSumGuardBias, kSumGuard
# cases of sum_chain_main.hip: single lanes (64 lanes x 2 inputs) of 2^25 - 1 and of -2^25, four constant pairs, 3000 random
# vectors signed; single lanes of 2^26 - 1, three constant pairs, 3000 random vectors unsigned; 2 inputs x 4 values per case
N_SIGNED, N_UNSIGNED = 2 * 128 + 4 + 3000, 128 + 3 + 3000
N_VALUES = 8 * (N_SIGNED + N_UNSIGNED)


def test_pair_chain_on_the_device(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    exe = str(tmp_path / "sum_chain_main")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I" + CSRC,
                    SOURCE, "-o", exe], check=True, timeout=300)
    run = subprocess.run(["timeout", "-k", "10", "60", exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"sum chain: (\d+) signed cases, (\d+) unsigned cases, (\d+) values, mismatches (\d+)", run.stdout)
    assert m, run.stdout
    assert [int(g) for g in m.groups()] == [N_SIGNED, N_UNSIGNED, N_VALUES, 0], run.stdout


# ---------------------------------------------------------------------------------------------- the lanes, on the CPU
def pick_seg(ww, wh):
    """Cfg<WW, WH>::S (lk_fast_tiles.h, pick_seg): the segment length of least cost, the smallest on a tie."""
    best, best_cost = 8, 1 << 30
    for s in range(5, 9):
        nseg = (ww + s - 1) // s
        cost = ((nseg * wh + 63) // 64) * (s + 3)
        if cost < best_cost:
            best, best_cost = s, cost
    return best


def lane_partials(px, win):
    """The 64 lane partials of a window's per-pixel products: task t = row t // NSEG, pixels (t % NSEG) * S .. + S - 1 of it,
    in lane t % 64 (k_lk_fast.hip, "this lane's row segments")."""
    ww, wh = win
    s = pick_seg(ww, wh)
    nseg = (ww + s - 1) // s
    px = np.asarray(px, np.int64).reshape(wh, ww)
    lanes = np.zeros(64, np.int64)
    for t in range(nseg * wh):
        row, col = t // nseg, (t % nseg) * s
        lanes[t % 64] += px[row, col:col + s].sum()
    return lanes


def signed_guard(*lanes):
    return all(bool((((np.asarray(v, np.int64) + GUARD_BIAS) & 0xffffffff) < GUARD).all()) for v in lanes)


class Probe(list):
    """The `trace` list of np_restatement.pyrlk, with npr._bilinear wrapped around it: per template the lane partials of
    a11, a12, a22, per iteration those of b1 and b2 (an iteration = a step length noted in the trace)."""

    def __init__(self, win):
        super().__init__()
        self.win = win
        self.last9 = self.Iw = self.Ix = self.Iy = None
        self.prev14 = False
        self.templates, self.iterations = [], []

    def bilinear(self, inner, patch, wt, shift):
        v = inner(patch, wt, shift)
        if shift == npr.W_BITS:
            if self.prev14:
                self.Iy = v
                lp = [lane_partials(p, self.win) for p in (self.Ix * self.Ix, self.Ix * self.Iy, self.Iy * self.Iy)]
                narrow = bool(((lp[0] | lp[2]) < GUARD).all()) and signed_guard(lp[1])
                self.templates.append(dict(narrow=narrow, lanes=lp, totals=[int(x.sum()) for x in lp]))
            else:
                self.Ix, self.Iw = v, self.last9
            self.prev14 = not self.prev14
        else:
            self.last9 = v
        return v

    def append(self, e):
        super().append(e)
        if isinstance(e[2], float):
            diff = self.last9 - self.Iw
            l1, l2 = lane_partials(diff * self.Ix, self.win), lane_partials(diff * self.Iy, self.win)
            self.iterations.append(dict(narrow=signed_guard(l1, l2), lanes=(l1, l2), totals=(int(l1.sum()), int(l2.sum()))))


def probe(f0, f1, pts, win, level):
    p = Probe(win)
    inner = npr._bilinear
    npr._bilinear = lambda patch, wt, shift: p.bilinear(inner, patch, wt, shift)
    try:
        res = npr.track_fb(f0, f1, pts, win, level, CRIT, trace=p)
    finally:
        npr._bilinear = inner
    return res, p


# ---------------------------------------------------------------------------------------------- frames
def texture(w, h, seed, rx=2, ry=2):
    """Blurred noise (three box passes each way, radii rx and ry), stretched to half the grey range around 128."""
    rng = np.random.default_rng(seed)
    a = rng.random((h + 6 * ry, w + 6 * rx))
    for _ in range(3):
        k = 2 * rx + 1
        c = np.cumsum(np.pad(a, ((0, 0), (1, 0))), 1)
        a = (c[:, k:] - c[:, :-k]) / k
        k = 2 * ry + 1
        c = np.cumsum(np.pad(a, ((1, 0), (0, 0))), 0)
        a = (c[k:] - c[:-k]) / k
    a = a[:h, :w]
    return np.ascontiguousarray(np.clip(np.rint(64.0 + (a - a.min()) / (a.max() - a.min()) * 128.0), 0, 255).astype(np.uint8))


def shifted_pair(seed, dx, dy, rx=2, ry=2):
    m = 4
    big = texture(W + 2 * m, H + 2 * m, seed, rx, ry)
    return (np.ascontiguousarray(big[m:m + H, m:m + W]), np.ascontiguousarray(big[m - dy:m - dy + H, m - dx:m - dx + W]))


def banded_pair(seed, y0, y1):
    """Texture in the rows y0 .. y1 - 1 alone, flat grey elsewhere, moved one pixel in x."""
    f0, f1 = shifted_pair(seed, 1, 0)
    f0, f1 = f0.copy(), f1.copy()
    for f in (f0, f1):
        f[:y0] = 128
        f[y1:] = 128
    return f0, f1


def grid_points(seed, y=None, border=26):
    rng = np.random.default_rng(seed)
    xs = rng.uniform(border, W - border, NPTS)
    ys = rng.uniform(border, H - border, NPTS) if y is None else np.full(NPTS, y) + rng.uniform(0.0, 0.9, NPTS)
    return np.stack([xs, ys], 1).astype(np.float32)


BAND = (20, 60)            # rows of texture in the half-window scenes


def scene(name, win):
    wh = win[1]
    if name == "stretched_x":         # smooth along x: gradients in y dominate, sum a22 > 2 sum a11
        return shifted_pair(11, 1, 1, rx=5, ry=1) + (grid_points(1),)
    if name == "stretched_y":
        return shifted_pair(12, 1, 1, rx=1, ry=5) + (grid_points(2),)
    if name == "shift_x":
        return shifted_pair(13, 1, 0) + (grid_points(3),)
    if name == "shift_y":
        return shifted_pair(14, 0, 1) + (grid_points(4),)
    if name == "top_half":            # the window's rows 0 .. wh // 2 - 3 end with the band, the rest is flat
        return banded_pair(15, *BAND) + (grid_points(5, y=BAND[1] + 2 + (wh - 1) // 2 - (wh // 2 - 2)),)
    if name == "bottom_half":         # the band starts at the window's row wh // 2 + 3
        return banded_pair(16, BAND[1], BAND[1] + 40) + (grid_points(6, y=BAND[1] - 4 - (wh // 2 + 3) + (wh - 1) // 2 + 1),)
    if name == "limits":              # test_gpu_sum_width.py's family that splits the waves between the two arms
        I, J = xf.stretched(W, H, 9, k=8)[:2]
        return I, J, grid_points(7)
    raise KeyError(name)


SCENES = ("stretched_x", "stretched_y", "shift_x", "shift_y", "top_half", "bottom_half", "limits")


def claims(name, win, p):
    """What the case is named for, shown on the lane partials the restatement produced."""
    it = [i for i in p.iterations if i["narrow"] and i["totals"][0] != i["totals"][1]]
    tm = [t for t in p.templates if t["narrow"]]
    assert len(it) >= 20, (name, win, "iterations in the narrow arm whose totals differ", len(it), len(p.iterations))
    assert len(tm) >= 8 and all(t["totals"][0] != t["totals"][2] for t in tm), (name, win, len(tm))
    if name == "stretched_x":
        n = sum(t["totals"][2] > 2 * t["totals"][0] for t in tm)
        assert n >= 20, (name, win, n, len(tm))
    if name == "stretched_y":
        n = sum(t["totals"][0] > 2 * t["totals"][2] for t in tm)
        assert n >= 20, (name, win, n, len(tm))
    if name == "shift_x":
        n = sum(abs(i["totals"][0]) > 2 * abs(i["totals"][1]) for i in it)
        assert n >= 20, (name, win, n)
    if name == "shift_y":
        n = sum(abs(i["totals"][1]) > 2 * abs(i["totals"][0]) for i in it)
        assert n >= 20, (name, win, n)
    if name in ("top_half", "bottom_half") and win in ((15, 15), (21, 21)):
        # one segment per lane: the lanes run down the window, so one half of the wave carries the whole sum
        idle = slice(32, 64) if name == "top_half" else slice(0, 32)
        busy = slice(0, 32) if name == "top_half" else slice(32, 64)
        n = sum(not i["lanes"][0][idle].any() and not i["lanes"][1][idle].any() and
                bool(i["lanes"][0][busy].any()) and bool(i["lanes"][1][busy].any()) for i in it)
        assert n >= 20, (name, win, n, len(it))
        n = sum(not t["lanes"][0][idle].any() and not t["lanes"][2][idle].any() and t["totals"][0] > 0 and t["totals"][2] > 0
                for t in tm)
        assert n >= 8, (name, win, n, len(tm))
    if name == "limits":
        wide = sum(not i["narrow"] for i in p.iterations)
        print(name, win, "iterations in the wide arm:", wide, "of", len(p.iterations))


# ---------------------------------------------------------------------------------------------- the kernel
@pytest.fixture(scope="module")
def gctx():
    from iceberg_tracking_code_amd import Context
    c = Context(W, H, n_slots=2, max_pts=4096)
    yield c
    c.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_fb(got, ref, tag):
    for k in KEYS_FB:
        assert np.array_equal(_bits(got[k]).ravel(), _bits(ref[k]).ravel()), (tag, k)


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("win", WINDOWS)
@pytest.mark.parametrize("name", SCENES)
def test_kernel_against_oracle(gctx, orc, name, win, level):
    f0, f1, pts = scene(name, win)
    assert f0.shape == (H, W) and 8 <= len(pts) <= 16
    res, p = probe(f0, f1, pts, win, level)
    print(name, win, level, "iterations", len(p.iterations), "narrow", sum(i["narrow"] for i in p.iterations),
          "templates", len(p.templates), "narrow", sum(t["narrow"] for t in p.templates))
    claims(name, win, p)
    gctx.upload_gray(0, f0)
    gctx.upload_gray(1, f1)
    ref = orc.track_fb(f0, f1, pts, win, level, CRIT)
    _same_fb(res, ref, (name, win, level, "restatement"))
    for wide in ((0, 1) if name == "limits" else (0,)):
        gctx.set_variant("lk_wide_sums", wide)
        try:
            got = gctx.track_fb(0, 1, pts, win, level, CRIT)
        finally:
            gctx.set_variant("lk_wide_sums", 0)
        _same_fb(got, ref, (name, win, level, wide))
    assert ref["valid"].sum() >= len(pts) // 2 or name == "limits"


def test_segments_joint_launch_and_hand_over(orc):
    """Two segments of two pairs through SegmentTracker on 160 x 120 frames: the joint launch of two pairs and the pass that
    takes stored templates (no template sums of its own) beside the pass that builds them, against the list-of-lists loop
    on the oracle."""
    from iceberg_tracking_code_amd import Context, SegmentTracker
    from reference_loops import OracleCv, run_reference_loop
    m = 8
    big = texture(W + 2 * m, H + 2 * m, 21)
    frames = [np.ascontiguousarray(big[m - k:m - k + H, m + k:m + k + W]) for k in range(5)]
    fp = dict(maxCorners=60, qualityLevel=0.005, minDistance=6, blockSize=5)
    lk = dict(winSize=(21, 21), maxLevel=1, criteria=CRIT)
    ref = run_reference_loop(frames, 2, fp, lk, cv=OracleCv(orc))
    assert len(ref) == 2 and len(ref[0][1]) >= 8
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
