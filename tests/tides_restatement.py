"""The per-cell harmonic fit restated in numpy, written from the rule's text, not from csrc/tides.h.

Every loop over windows, terms and chunks is explicit; the cells of a cube are carried along as the one array axis, each
operation on it a single correctly rounded float64 operation per cell (no dot, no sum, no fused multiply-add), and "this cell
skips this window" is a np.where that keeps the old value.  The library's host statement must agree with this bit for bit.

The rule: window t is a sample of a cell iff u and v are finite and count >= min_count.  With B the basis table, the sums
A[i][j] = sum B[t][i] * B[t][j] (j <= i), ru[i] = sum B[t][i] * u[t], rv, su = sum u[t], sv run over the cell's samples in
chunks of 256 windows: ascending within a chunk onto +0.0, the chunk totals ascending onto +0.0.  n < max(min_samples, m) is
status 1.  Otherwise Cholesky row by row, subtractions in ascending k, status 2 when a pivot s fails s > 2^-30 * A[j][j];
otherwise L y = r forwards and L^T c = y backwards.  Second pass: pred = c[0] * B[t][0] + c[1] * B[t][1] + ..., res = u -
pred, ss_res = sum res * res, ss_tot = sum (u - su / n)^2, chunked alike; rms = sqrt(ss_res / (n - m)), NaN for n == m;
explained = 1 - ss_res / ss_tot.  Everything is NaN for status != 0."""
import numpy as np

CHUNK = 256
PIVOT_TOL = 2.0 ** -30
RESULT_KEYS = ("coef_u", "coef_v", "rms_u", "rms_v", "explained_u", "explained_v", "n", "first", "last", "status", "residual_u",
               "residual_v")


def chunked_sum(nt, take, term):
    """sum over t of term(t) where take[t], per cell, in the rule's order"""
    total = np.zeros(take.shape[1])
    for c0 in range(0, nt, CHUNK):
        part = np.zeros(take.shape[1])
        for t in range(c0, min(nt, c0 + CHUNK)):
            part = np.where(take[t], part + term(t), part)
        total = total + part
    return total


def restate(u, v, count, basis, min_count=1, min_samples=None):
    """u, v, count (windows, cells), basis (windows, m) -> the dict of tides.fit_arrays_host with the residual cubes"""
    u, v, count, B = (np.asarray(a, np.float64) for a in (u, v, count, basis))
    nt, nc = u.shape
    m = B.shape[1]
    min_samples = m if min_samples is None else min_samples
    with np.errstate(all="ignore"):
        take = np.isfinite(u) & np.isfinite(v) & (count >= np.float64(min_count))
        n = take.sum(axis=0).astype(np.int32)
        some = n > 0
        first = np.where(some, np.argmax(take, axis=0), -1).astype(np.int32)
        last = np.where(some, nt - 1 - np.argmax(take[::-1], axis=0), -1).astype(np.int32)
        A = {(i, j): chunked_sum(nt, take, lambda t: B[t, i] * B[t, j]) for i in range(m) for j in range(i + 1)}
        r = {"u": [chunked_sum(nt, take, lambda t: B[t, i] * u[t]) for i in range(m)],
             "v": [chunked_sum(nt, take, lambda t: B[t, i] * v[t]) for i in range(m)]}
        mean = {"u": chunked_sum(nt, take, lambda t: u[t]) / n.astype(np.float64),
                "v": chunked_sum(nt, take, lambda t: v[t]) / n.astype(np.float64)}
        status = np.where(n < max(min_samples, m), 1, 0).astype(np.int32)
        L = {}
        for i in range(m):
            for j in range(i + 1):
                s = A[i, j]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                if j < i:
                    L[i, j] = s / L[j, j]
                else:
                    status = np.where((status == 0) & ~(s > PIVOT_TOL * A[j, j]), 2, status).astype(np.int32)
                    L[i, i] = np.sqrt(s)
        ok = status == 0
        out = dict(n=n, first=first, last=last, status=status)
        for comp, x in (("u", u), ("v", v)):
            y = []
            for i in range(m):
                s = r[comp][i]
                for k in range(i):
                    s = s - L[i, k] * y[k]
                y.append(s / L[i, i])
            c = [None] * m
            for i in range(m - 1, -1, -1):
                s = y[i]
                for k in range(i + 1, m):
                    s = s - L[k, i] * c[k]
                c[i] = s / L[i, i]
            c = [np.where(ok, q, np.nan) for q in c]
            res = np.full((nt, nc), np.nan)
            for t in range(nt):
                pred = c[0] * B[t, 0]
                for j in range(1, m):
                    pred = pred + c[j] * B[t, j]
                res[t] = np.where(take[t] & ok, x[t] - pred, np.nan)
            fitted = take & ok
            ss_res = chunked_sum(nt, fitted, lambda t: res[t] * res[t])
            ss_tot = chunked_sum(nt, fitted, lambda t: (x[t] - mean[comp]) * (x[t] - mean[comp]))
            rms = np.where(n == m, np.nan, np.sqrt(ss_res / (n - m).astype(np.float64)))
            out["coef_" + comp] = np.stack(c, axis=1)
            out["rms_" + comp] = np.where(ok, rms, np.nan)
            out["explained_" + comp] = np.where(ok, 1.0 - ss_res / ss_tot, np.nan)
            out["residual_" + comp] = res
    return out


def same_bits(a, b, keys=RESULT_KEYS):
    """None when two result dicts agree -- shapes, dtypes and bits, a NaN matching any NaN --, else the first key that differs"""
    for k in keys:
        p, q = np.asarray(a[k]), np.asarray(b[k])
        if p.shape != q.shape or p.dtype != q.dtype:
            return k
        if p.dtype.kind == "f":
            nan = np.isnan(p)
            if not np.array_equal(nan, np.isnan(q)) or p[~nan].tobytes() != q[~nan].tobytes():
                return k
        elif p.tobytes() != q.tobytes():
            return k
    return None
