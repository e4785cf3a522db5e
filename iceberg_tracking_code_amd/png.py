"""The PNG writer: an 8-bit R G B picture as the file the reference's `plt.savefig(...png)` stands for (s3:630-637), with
the pixels exact.  The file is the signature, IHDR (8 bits, colour type 2, no interlace), one IDAT and IEND; IDAT holds a
zlib stream of one fixed-Huffman deflate block over the filtered rows (csrc/png_enc.h).  Here are the host
calls, which need no GPU: the host statement of the whole file, the filtered rows, and the size bound.  On the device the
same file, byte for byte, comes from `Context.png_encode(rgb)` and, for a window's map, from
`Context.map_draw(picture, format="png")`."""
import ctypes as C

import numpy as np

from . import _lib
from .jpeg import _encode_call, _rgb3

PNG_SEGMENT = 4096      # bytes of the filtered stream per greedy parse (png::kSegment)
PNG_MAX_SIDE = 16384


def png_bound(w, h):
    """The largest file the coder writes for a w x h picture: 9 bits per filtered byte and the fixed parts
    (icelk_png_bound).  ValueError outside 1 <= w, h <= 16384, h (1 + 3 w) <= 2^28."""
    n = C.c_uint64(0)
    _lib.check(_lib.load().icelk_png_bound(int(w), int(h), C.byref(n)))
    return n.value


def png_filter_host(rgb):
    """H x W x 3 uint8 -> the filtered rows, H (1 + 3 W) bytes: per row the filter type, then the filtered bytes
    (icelk_png_filter_host)."""
    a = _rgb3(rgb)
    out = np.empty(a.shape[0] * (1 + 3 * a.shape[1]), np.uint8)
    _lib.check(_lib.load().icelk_png_filter_host(a.ctypes.data_as(_lib.u8p), a.shape[1], a.shape[0], a.strides[0], out.ctypes.data_as(_lib.u8p)))
    return out.tobytes()


def encode_png_host(rgb):
    """H x W x 3 uint8 -> the bytes of the PNG file, by the host statement of the coder (icelk_png_encode_host):
    `np.asarray(Image.open(file))` is `rgb` again, and `Context.png_encode(rgb)` returns the same bytes."""
    a = _rgb3(rgb)
    lib = _lib.load()
    args = (a.ctypes.data_as(_lib.u8p), a.shape[1], a.shape[0], a.strides[0])
    # a buffer of the bound: the coder runs once (numpy touches none of it)
    return _encode_call(lambda out, cap, n: lib.icelk_png_encode_host(*args, out, cap, n), png_bound(a.shape[1], a.shape[0]), "icelk_png_encode_host")
