"""The stabilisation's rules (csrc/stab.h) restated in numpy, written from the rules and not from the C++:
every sum is literally np.sum(wf * ...), the start shift literally np.median.  test_stab_host.py holds the library's host
statement to this bit for bit, test_gpu_stab.py the kernels to the host statement."""
import numpy as np

TOO_FEW, LOST, DEGENERATE, NOT_CONVERGED = 1, 2, 4, 8


def anchor_flags(tracks, mask):
    t = np.asarray(tracks, np.float32)
    m = np.asarray(mask)
    x0, y0 = t[:, 0, 0].astype(np.float64), t[:, 0, 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        fx, fy = np.floor(x0 + 0.5), np.floor(y0 + 0.5)
        inside = (fx >= 0) & (fx < m.shape[1]) & (fy >= 0) & (fy < m.shape[0])
    flags = np.zeros(len(t), bool)
    ix, iy = fx[inside].astype(np.int64), fy[inside].astype(np.int64)
    flags[inside] = m[iy, ix] != 0
    return flags


def _inliers(m, g, x, y, X, Y):
    a, b, tx, ty = m
    ex = X - ((a * x - b * y) + tx)
    ey = Y - ((b * x + a * y) + ty)
    r2 = ex * ex + ey * ey
    return r2 <= g * g, r2


def _fit(w, model, min_spread, x, y, X, Y):
    wf = w.astype(np.float64)
    n_in = np.sum(wf)
    translation = (np.float64(1.0), np.float64(0.0), np.sum(wf * (X - x)) / n_in, np.sum(wf * (Y - y)) / n_in)
    if model == "translation":
        return translation, False
    mx, my, mX, mY = np.sum(wf * x) / n_in, np.sum(wf * y) / n_in, np.sum(wf * X) / n_in, np.sum(wf * Y) / n_in
    xc, yc, Xc, Yc = x - mx, y - my, X - mX, Y - mY
    D = np.sum(wf * (xc * xc + yc * yc))
    if not D >= n_in * min_spread * min_spread:
        return translation, True
    a = np.sum(wf * (xc * Xc + yc * Yc)) / D
    b = np.sum(wf * (xc * Yc - yc * Xc)) / D
    return (a, b, mX - (a * mx - b * my), mY - (b * mx + a * my)), False


def stabilize(tracks, flags, model="translation", threshold=1.0, start_gate=8.0, rounds=8, min_anchors=10, min_spread=64.0):
    t = np.asarray(tracks, np.float32)
    n, V, _ = t.shape
    threshold, start_gate, min_spread = np.float64(threshold), np.float64(start_gate), np.float64(min_spread)
    A = np.flatnonzero((np.asarray(flags).reshape(-1) != 0) & np.isfinite(t).reshape(n, -1).all(axis=1))
    x, y = t[A, 0, 0].astype(np.float64), t[A, 0, 1].astype(np.float64)
    out = t.copy()
    motion, inliers, rms = np.zeros((V - 1, 4)), np.zeros(V - 1, np.int32), np.full(V - 1, np.nan)
    status, rounds_used = np.zeros(V - 1, np.int32), np.zeros(V - 1, np.int32)
    with np.errstate(all="ignore"):
        for k in range(1, V):
            motion[k - 1] = (1.0, 0.0, 0.0, 0.0)
            if len(A) < min_anchors:
                status[k - 1] = TOO_FEW
                continue
            X, Y = t[A, k, 0].astype(np.float64), t[A, k, 1].astype(np.float64)
            m = (np.float64(1.0), np.float64(0.0), np.median(X - x), np.median(Y - y))
            g = max(threshold, start_gate)
            w, _ = _inliers(m, g, x, y, X, Y)
            lost = converged = degenerate = False
            used = 0
            for r in range(1, rounds + 1):
                if np.count_nonzero(w) < min_anchors:
                    lost = True
                    break
                m, degenerate = _fit(w, model, min_spread, x, y, X, Y)
                used = r
                g2 = max(threshold, g / 2)
                w2, _ = _inliers(m, g2, x, y, X, Y)
                converged = bool(np.array_equal(w2, w) and g2 == g)
                w, g = w2, g2
                if converged:
                    break
            if np.count_nonzero(w) < min_anchors:
                lost = True
            inliers[k - 1], rounds_used[k - 1] = np.count_nonzero(w), used
            status[k - 1] = (LOST if lost else 0) | (DEGENERATE if degenerate else 0) | (NOT_CONVERGED if not converged and used == rounds else 0)
            if lost:
                continue
            wf = w.astype(np.float64)
            _, r2 = _inliers(m, g, x, y, X, Y)
            rms[k - 1] = np.sqrt(np.sum(wf * r2) / np.sum(wf))
            motion[k - 1] = m
            a, b, tx, ty = m
            det = a * a + b * b
            Xa, Ya = t[:, k, 0].astype(np.float64) - tx, t[:, k, 1].astype(np.float64) - ty
            xs, ys = (a * Xa + b * Ya) / det, (a * Ya - b * Xa) / det
            # a NaN's sign and payload are not IEEE's to say: THE quiet NaN stands for every one of them
            out[:, k, 0] = np.where(np.isnan(xs), np.float32(np.nan), xs.astype(np.float32))
            out[:, k, 1] = np.where(np.isnan(ys), np.float32(np.nan), ys.astype(np.float32))
    return dict(tracks=out, motion=motion, inliers=inliers, rms=rms, status=status, rounds_used=rounds_used, n_anchors=len(A))
