"""The catalogue the stabilisation is checked on (test_stab_host.py on the CPU, test_gpu_stab.py on the device): seeded,
small tables with planted camera motions.  A case is (name, tracks (n, V, 2) float32, flags (n,) bool, params, info); info
says what was planted: `clean` (rows that carry the planted motion and nothing else), `shift` (V - 1, 2) where the motion is
a pure translation.

Frame 3456 x 2304.  Vertex 0 of every row sits on integer pixels, anchors on the left third of the frame; the planted motion
of vertex k is a roll about the frame's centre plus a shift, or a shift by whole 1/256 px; outliers are anchors displaced by
5-25 px.  The table lengths and anchor counts are those at which np.sum changes strategy (below 8 terms, 8 accumulators, the
128-term leaves, the halves aligned to 8, the 8192-term chunks) and at which the kernels' loops wrap (64, 256)."""
import functools

import numpy as np

W, H = 3456, 2304
MODELS = ("translation", "similarity")


def _table(rng, n, n_a, V):
    """n rows on integer pixels, the first-flagged n_a of them (spread over the table, in row order) on the left third"""
    flags = np.zeros(n, bool)
    flags[np.sort(rng.choice(n, size=min(n_a, n), replace=False))] = True
    x0 = np.where(flags, rng.integers(8, W // 3, n), rng.integers(8, W - 8, n)).astype(np.float64)
    y0 = rng.integers(8, H - 8, n).astype(np.float64)
    return x0, y0, flags


def _move(x0, y0, V, rolls, shifts):
    """vertex k = vertex 0 rolled by rolls[k - 1] about the centre and shifted by shifts[k - 1], in doubles"""
    t = np.zeros((len(x0), V, 2))
    t[:, 0, 0], t[:, 0, 1] = x0, y0
    for k in range(1, V):
        c, s = np.cos(rolls[k - 1]), np.sin(rolls[k - 1])
        dx, dy = x0 - W / 2, y0 - H / 2
        t[:, k, 0] = c * dx - s * dy + W / 2 + shifts[k - 1][0]
        t[:, k, 1] = s * dx + c * dy + H / 2 + shifts[k - 1][1]
    return t


def _outliers(rng, t, flags, fraction):
    """a fraction of the anchors displaced by 5-25 px in a random direction, a new one at every vertex; returns the clean rows"""
    a = np.flatnonzero(flags)
    bad = a[rng.random(len(a)) < fraction]
    for k in range(1, t.shape[1]):
        r, phi = rng.uniform(5, 25, len(bad)), rng.uniform(0, 2 * np.pi, len(bad))
        t[bad, k, 0] += r * np.cos(phi)
        t[bad, k, 1] += r * np.sin(phi)
    clean = np.ones(len(t), bool)
    clean[bad] = False
    return clean


def _rolls(rng, V):
    return rng.uniform(0.002, 0.012, V - 1) * rng.choice([-1, 1], V - 1), rng.uniform(-6, 6, (V - 1, 2))


def dyadic(seed, n, n_a, V, outliers=0.0):
    """a translation by whole 1/256 px: every coordinate and every sum is exact"""
    rng = np.random.default_rng(seed)
    x0, y0, flags = _table(rng, n, n_a, V)
    shift = rng.integers(-1500, 1500, (V - 1, 2)) / 256.0
    t = _move(x0, y0, V, np.zeros(V - 1), shift)
    clean = np.ones(n, bool)
    if outliers:
        a = np.flatnonzero(flags)
        bad = a[rng.random(len(a)) < outliers]
        for k in range(1, V):
            t[bad, k] += rng.choice([-1, 1], (len(bad), 2)) * rng.integers(5 * 256, 18 * 256, (len(bad), 2)) / 256.0
        clean[bad] = False
    return t.astype(np.float32), flags, dict(clean=clean, shift=shift)


def roll(seed, n, n_a, V, noise=0.0, outliers=0.4):
    rng = np.random.default_rng(seed)
    x0, y0, flags = _table(rng, n, n_a, V)
    t = _move(x0, y0, V, *_rolls(rng, V))
    clean = _outliers(rng, t, flags, outliers)
    if noise:
        t[:, 1:] += rng.uniform(-noise, noise, t[:, 1:].shape)
    return t.astype(np.float32), flags, dict(clean=clean)


@functools.lru_cache(maxsize=None)
def catalogue():
    cases = []

    def add(name, made, both=True, **params):
        t, flags, info = made
        for model in (MODELS if both else (params.pop("model"),)):
            cases.append(("%s-%s" % (name, model), t, flags, dict(params, model=model), info))

    # table lengths, with every vertex count
    for i, n in enumerate((1, 2, 63, 64, 65, 255, 256, 257, 1000)):
        V = (2, 3, 5, 17)[i % 4]
        add("n%d-V%d" % (n, V), roll(100 + n, n, max(n // 2, min(n, 12)), V, noise=0.3, outliers=0.2))
    add("n257-V17-dyadic", dyadic(99, 257, 90, 17))
    # anchor counts at which np.sum changes strategy; even and odd counts, the noise makes the middle terms distinct
    for n_a in (0, 9, 10, 11, 127, 128, 129, 136, 257):
        add("na%d" % n_a, roll(200 + n_a, 1000, n_a, 3, noise=0.3, outliers=0.2))
    big_rng = np.random.default_rng(7)
    big, _, _ = roll(300, 20000, 20000, 3, noise=0.3, outliers=0.2)     # ONE table of 20 000 rows, all on the left third
    for n_a in (1025, 8192, 8193, 16400):
        flags = np.zeros(20000, bool)
        flags[np.sort(big_rng.choice(20000, size=n_a, replace=False))] = True
        add("big-na%d" % n_a, (big, flags, {}))
    # planted motions
    x0, y0, flags = _table(np.random.default_rng(1), 1000, 300, 4)
    add("identity", (_move(x0, y0, 4, np.zeros(3), np.zeros((3, 2))).astype(np.float32), flags, dict(clean=np.ones(1000, bool), shift=np.zeros((3, 2)))))
    add("dyadic", dyadic(2, 1000, 300, 4, outliers=0.1))
    add("roll", roll(3, 1000, 300, 4))
    add("roll-noisy", roll(4, 1000, 300, 4, noise=0.3))
    # anchor displacements uniform in +-50 px: nothing to fit
    rng = np.random.default_rng(5)
    t = _move(x0, y0, 4, np.zeros(3), np.zeros((3, 2)))
    t[np.ix_(flags, [1, 2, 3])] += rng.uniform(-50, 50, (int(flags.sum()), 3, 2))
    add("scatter", (t.astype(np.float32), flags, {}))
    # all anchors on one point: no spread to fit a roll to
    t, f, info = dyadic(6, 1000, 300, 4)
    t[f] = t[f] - t[f, :1] + np.float32([700, 900])     # every anchor starts at (700, 900) and keeps its (exact) displacement
    add("one-point", (t, f, info), both=False, model="similarity")
    add("rounds1", roll(4, 1000, 300, 4, noise=0.3), both=False, model="similarity", rounds=1)
    # an anchor at exactly `threshold` from an exact model, under a start gate of the same size: inside by the <=
    t, f, info = dyadic(8, 200, 64, 3)
    first = np.flatnonzero(f)[0]
    t[first, 1:, 0] += np.float32(1.0)
    add("at-threshold", (t, f, dict(info, edge=first)), threshold=1.0, start_gate=1.0)
    # a NaN in an anchor row (the row is no anchor) and in a plain row (it passes through the arithmetic)
    t, f, info = roll(9, 1000, 300, 4, noise=0.3)
    t = t.copy()
    t[np.flatnonzero(f)[3], 2, 1] = np.nan
    t[np.flatnonzero(~f)[5], 1, 0] = np.nan
    t[np.flatnonzero(~f)[6], 0, 0] = np.inf
    add("nan", (t, f, {}))
    return tuple(cases)


def names():
    return [c[0] for c in catalogue()]


def case(name):
    return next(c for c in catalogue() if c[0] == name)
