"""The thumbnail rule and the inset paste restated in numpy, independently of csrc/thumb_raster.h: integer
overlap matrices, one matrix product per axis, Python integers for the size rule; no call into the library.

    size(W, H, box) -> (tw, th)
    weights(ns, no) -> (no, ns) int64: the overlap of output cell i with source cell x on an axis scaled by no
    reduce(image, (tw, th)) -> (th, tw, 3) uint8
    paste(rgb, insets) -> rgb with every inset's thumbnail and label drawn in order; insets as a picture dict carries them,
                          each with pixels=
"""
import numpy as np

import map_restatement as R


def size(W, H, box):
    bw, bh = box
    tw = min(bw, W)
    th = max(1, (2 * tw * H + W) // (2 * W))
    if th > bh:
        th = min(bh, H)
        tw = min(bw, max(1, (2 * th * W + H) // (2 * H)))
    return tw, th


def weights(ns, no):
    """output cell i covers [i ns, (i + 1) ns), source cell x covers [x no, (x + 1) no)"""
    i = np.arange(no, dtype=np.int64)[:, None]
    x = np.arange(ns, dtype=np.int64)[None, :]
    return np.clip(np.minimum((i + 1) * ns, (x + 1) * no) - np.maximum(i * ns, x * no), 0, None)


def reduce(image, size_):
    a = np.asarray(image)
    if a.ndim == 2:
        a = a[..., None]
    H, W = a.shape[:2]
    tw, th = size_
    Ay, Ax = weights(H, th), weights(W, tw)
    out = np.empty((th, tw, a.shape[2]), np.int64)
    for c in range(a.shape[2]):
        s = Ay @ a[..., c].astype(np.int64) @ Ax.T
        out[..., c] = (s + (W * H) // 2) // (W * H)
    out = out.astype(np.uint8)
    return np.repeat(out, 3, axis=2) if out.shape[2] == 1 else out


def paste(rgb, insets):
    out = np.array(rgb, np.uint8)
    H, W = out.shape[:2]
    for q in insets:
        px = np.asarray(q["pixels"], np.uint8)
        x0, y0 = q["at"]
        out[y0:y0 + px.shape[0], x0:x0 + px.shape[1]] = px
        if q.get("label") is not None:
            out[R.text_mask([tuple(q["label"])], W, H)] = 0
    return out
