"""The Harris response on box sums whose double addition rounds: references and a derived bound -- TEST HARNESS.

tests/box_sum_frames.py tells orders of double addition apart on the smaller-eigenvalue map.  The Harris response of
tests/harris_restatement.py is formed from the same three sums and cancels in float32 -- R = fl(ac) - fl(bb) - fl(fl(kf t) t)
with t = fl(a + c) -- so one float32 ulp of a sum can be many ulps of R, and the bound of box_sum_frames.bound (derived for
(a + c) - sqrt(...)) says nothing about it.  This module restates the response on sums that are handed in, builds the
high-precision reference and a second legal order from box_sum_frames, and derives a bound of its own.

  harris_of_sums(s0, s1, s2, k, tail=0)   the float32 forms of harris_restatement.harris_map on three double planes -> R, a, b, c
  exact_harris_map(img, bs, k)            ... on box_sum_frames.exact_sums: the high-precision reference
  running_harris_map(img, bs, k)          ... on box_sum_frames.running_sums: another legal double summation, NOT the kernel
  dropped_sums(img, bs, sums, y, x, j)    exact_sums(drop=(y, x, j)) without forming every window again
  harris_bound(img, bs, k)                the derived bound, no margin
  references(entry) / arm_references(label, bs)
                                          per chosen frame, once per session and read-only

Numpy and the standard library only; nothing compiled, not the oracle, not the package.
"""
import numpy as np

import box_sum_frames as B
import harris_restatement as H
import strip_arm_frames as S

F = np.float32
KS = (0.04, 0.15)


def harris_of_sums(s0, s1, s2, k, tail=0):
    """harris_restatement.harris_map behind its box sums: a, b, c = (float)S, not halved; every operation rounded to float32."""
    a, b, c = (np.asarray(s, np.float64).astype(np.float32) for s in (s0, s1, s2))
    t = a + c
    det = a * c - b * b
    assert t.dtype == np.float32 and det.dtype == np.float32
    if tail:
        t64 = t.astype(np.float64)
        r = (det.astype(np.float64) - (float(k) * t64) * t64).astype(np.float32)
    else:
        r = det - (F(k) * t) * t
    assert r.dtype == np.float32
    return r, a, b, c


def exact_harris_map(img, bs, k, tail=0, **planted):
    return harris_of_sums(*B.exact_sums(img, bs, **planted), k, tail)[0]


def running_harris_map(img, bs, k, tail=0):
    return harris_of_sums(*B.running_sums(img, bs), k, tail)[0]


def dropped_sums(img, bs, sums, y, x, j):
    """`sums` (box_sum_frames.exact_sums(img, bs)) with the j-th term (row-major) left out of the window of pixel (y, x):
    what exact_sums(img, bs, drop=(y, x, j)) returns -- only that pixel changes, and its window is summed again in integers."""
    h, w = np.asarray(img).shape
    by, bx = B.window_index(h, bs), B.window_index(w, bs)
    rows, cols = [int(r[y]) for r in by], [int(c[x]) for c in bx]
    out = []
    for p, s in zip(B.products(img, bs), sums):
        z = B._as_integers(p[np.ix_(rows, cols)]).ravel()
        s = s.copy()
        s[y, x] = (sum(int(v) for v in z) - int(z[j])) / (1 << B.SHIFT)       # int / int: one rounding, to double
        out.append(s)
    return out


# ---------------------------------------------------------------------------------------------- the bound
def _step32(x):
    """the float32 grid step at a magnitude, as a double"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def harris_bound(img, bs, k, n=None, sums=None):
    """Per pixel, a, b, c, t from the exact reference, kf = (float)k, d = N 2^-53 Smax as in box_sum_frames.bound:

        e_x = d + ulp32(|x| + d)                         x in a, b, c: two roundings to float32 of sums at most d apart
        e_t = e_a + e_c + ulp32(|a + c| + e_a + e_c)     the two roundings of a + c
        P   = |c| e_a + |a| e_c + e_a e_c + (2 |b| + e_b) e_b + kf (2 |t| + e_t) e_t          how far ac - bb - kf t t can move
        bound = P + 6 ulp32(max(|ac|, bb, kf t t) + P)   six float32 roundings in each of the two evaluations, half a step each

    No margin; DESIGN.md section 4.2 has the derivation."""
    n = B.chain_length(bs) if n is None else n
    sums = B.exact_sums(img, bs) if sums is None else sums
    kf = float(F(k))
    _, a, b, c = harris_of_sums(*sums, k)
    t = (a + c).astype(np.float64)
    a, b, c = (np.abs(v.astype(np.float64)) for v in (a, b, c))
    smax = float(int(bs) ** 2) * max(float(np.abs(p).max()) for p in B.products(img, bs))
    d = n * 2.0 ** -53 * smax
    ea, eb, ec = (d + _step32(v + d) for v in (a, b, c))
    et = ea + ec + _step32(np.abs(t) + ea + ec)
    moved = c * ea + a * ec + ea * ec + (2.0 * b + eb) * eb + kf * (2.0 * np.abs(t) + et) * et
    largest = np.maximum(np.maximum(a * c, b * b), kf * t * t)
    return moved + 6.0 * _step32(largest + moved)


def within_bound(got, ref, bnd):
    return np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) <= bnd


# ---------------------------------------------------------------------------------------------- references, computed once
_references = {}


def _frozen(r):
    for v in r.values():
        for u in (v if isinstance(v, (list, tuple)) else [v]):
            if isinstance(u, np.ndarray):
                u.setflags(write=False)
    return r


def _build(key, img, bs):
    """img, bs, sums (exact), and per k of KS: exact, bound, term (harris_restatement.harris_map), running."""
    if key not in _references:
        sums = B.exact_sums(img, bs)
        running = B.running_sums(img, bs)
        r = dict(img=img, bs=bs, sums=sums)
        for k in KS:
            r[k] = _frozen(dict(exact=harris_of_sums(*sums, k)[0], bound=harris_bound(img, bs, k, sums=sums),
                                term=H.harris_map(img, bs, k), running=harris_of_sums(*running, k)[0]))
        _references[key] = _frozen(r)
    return _references[key]


def references(entry):
    """one of box_sum_frames.FRAMES + RESIDUE_FRAMES at its own blockSize"""
    return _build(B.tag(entry), B.build(entry), entry[2])


def arm_references(label, bs):
    """one of strip_arm_frames.CASES"""
    _, seed, kind, w, h, _ = next(e for e in S.ROUNDING if e[0] == label)
    key = "arm-%s-bs%d" % (label, bs)
    if key not in _references:
        _build(key, S.rounding(seed, kind, w, h), bs)
    return _references[key]
