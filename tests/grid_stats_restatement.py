"""The three per-cell rules of csrc/grid_stats.h written a second time, in numpy and plain Python, by the text of the
rules and not by the header's code: no radix select, no keys -- a sort.  The sums are np_restatement-free on purpose:
np.sum over a contiguous float64 array IS the chunked pairwise sum the header restates, so this file leans on numpy
for that one step only and spells out everything else one rounding at a time.

    std(a)     m = np.sum(a) / n; d = (a - m) * (a - m); sqrt(np.sum(d) / (n - 1)); n == 1 gives 0.0 / 0 = NaN
    median(a)  NaN when a term is NaN; s = sorted terms; odd n: (0.0 + s[n // 2]) / 1.0;
               even n: ((0.0 + s[n // 2 - 1]) + s[n // 2]) / 2.0
    mad(a)     median(|a - median(a)|)
An empty cell has NaN in all three."""
import numpy as np

F = np.float64


def std(a):
    a = np.ascontiguousarray(a, F)
    n = len(a)
    if n == 0:
        return F(np.nan)
    with np.errstate(all="ignore"):
        m = np.sum(a) / F(n)
        d = a - m
        d = d * d
        return np.sqrt(np.sum(d) / F(n - 1))


def median(a):
    a = np.ascontiguousarray(a, F)
    n = len(a)
    if n == 0 or np.isnan(a).any():
        return F(np.nan)
    s = sorted(float(x) for x in a)            # Python's sort: +-0.0 compare equal, and their order does not show below
    with np.errstate(all="ignore"):
        if n % 2:
            return (F(0.0) + F(s[n // 2])) / F(1.0)
        return ((F(0.0) + F(s[n // 2 - 1])) + F(s[n // 2])) / F(2.0)


def mad(a):
    a = np.ascontiguousarray(a, F)
    if len(a) == 0:
        return F(np.nan)
    with np.errstate(all="ignore"):
        return median(np.abs(a - median(a)))


def cell_stats(a):
    return std(a), median(a), mad(a)


def numpy_stats(a):
    """numpy itself: the yardstick."""
    a = np.ascontiguousarray(a, F)
    if len(a) == 0:
        return F(np.nan), F(np.nan), F(np.nan)
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return np.std(a, ddof=1), np.median(a), np.median(np.abs(a - np.median(a)))
