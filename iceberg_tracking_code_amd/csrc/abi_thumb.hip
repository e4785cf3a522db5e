// abi_thumb.hip -- the inset photographs of the velocity map (s3:593-626, s3:788-829): a camera's photo reduced to a
// thumbnail on the device, and the resident set of thumbnails icelk_map_draw_insets (abi_map.hip) pastes into a picture.
//
//   host    icelk_thumb_size, icelk_thumb_host: thumb_raster.h on the CPU; no handle, re-entrant
//   device  icelk_jpeg_thumb_file: the synchronous ingest route (jpeg_huff_device -> jpeg_planes(..., on_device),
//           abi_jpeg_ingest.hip: the same files, the same error codes, the host's Huffman decoder inside the call), then
//           k_jpeg_thumb (k_thumb.hip) from the component planes into the decoder's R G B buffer, and that to the caller.
//           icelk_map_inset_set_file: the same into an allocation of the thumbnail's own, which becomes resident inset
//           `index`; icelk_map_inset_set_pixels uploads a ready one; icelk_map_inset_release.  Every call waits for the
//           device; a thumbnail that is replaced or released is freed after that wait.
//
// Bounds, load by load and store by store.  The planes are jpeg_plane_layout's for the whole image (left = top = right =
// bottom = 0): plane k holds blocks_y[k] 8 rows of pitch[k] = blocks_x[k] 8 bytes, the image's W x H luma samples and
// cw x ch chroma samples at its top-left.  tw <= W and th <= H are checked against the file's own header before the launch.
//   k_jpeg_thumb   grid (ceil(tw / per), th): output row j = blockIdx.y < th, pixels i_first .. i_last <= tw - 1.
//       loads      through rgbpx::rgb4 / load4 only (jpeg_rgb.h): luma row y in first_source(j) .. last_source(j) <= H - 1,
//                  columns x4 .. x4 + 3 with x4 < xe <= last_source(tw - 1) + 1 = W: one dword where x4 + 3 < W, else byte by
//                  byte with the column clamped to W - 1.  Chroma: the window chroma4 names for (x4, y), every column
//                  clamped to 0 .. cw - 1 by load4 and the rows y (modes 0, 1, 3: ch = H), y / 2 <= ch - 1 (modes 2, 4:
//                  ch = ceil(H / 2)) and the far row clamped to 0 .. ch - 1.  A one-component file loads luma alone
//       LDS        col[quarter][c][4 lane .. 4 lane + 3], quarter < 4, lane < 64, rows of 256 words; read at x - base with
//                  base <= x <= base + 255 and x < xe, where every quarter's lane of x has stored
//       stores     the byte(s) of pair (i, c) at dst + j pitch + 3 i + c, i <= i_last <= tw - 1, c < 3, j < th,
//                  pitch >= 3 tw: inside the th pitch bytes of dst
//   k_map_inset    threads t < bw bh over the rectangle inset_box clips to [0, Wo) x [0, Ho): three byte stores at
//                  rgb + 3 (py Wo + px) < 3 Wo Ho, the size picture_grow gives c->picture.d_rgb.  Loads: the thumbnail at
//                  (dy, dx), 0 <= dx < w, 0 <= dy < h, of an allocation of h 3 w bytes; the label's glyph indices g[cell],
//                  cell < n <= 48, in the kernel's own argument
#include "icelk_ctx.h"

namespace icelk {

void map_insets_free(Ctx* c)
{
    Ctx::Map& M = c->map;
    for (int k = 0; k < thumb::kMaxInsets; k++) {
        if (M.d_inset[k]) hipFree(M.d_inset[k]);   // waits for everything that may still read it
        M.d_inset[k] = nullptr, M.inset_w[k] = M.inset_h[k] = 0;
    }
}

namespace {

// the thumbnail `fresh` (tw x th, rows 3 tw bytes apart) takes the place of resident inset `index`
void adopt_inset(Ctx* c, int index, uint8_t* fresh, int tw, int th)
{
    Ctx::Map& M = c->map;
    if (M.d_inset[index]) hipFree(M.d_inset[index]);
    M.d_inset[index] = fresh, M.inset_w[index] = tw, M.inset_h[index] = th;
}

// The file decoded to planes on the compute stream and k_jpeg_thumb enqueued behind them.  to_host: into the decoder's
// R G B buffer, *d_out says where; else into a new allocation the caller owns (*d_out), freed here after an error.
int thumb_of_file(Ctx* c, const uint8_t* data, uint64_t len, int tw, int th, bool to_host, uint8_t** d_out)
{
    *d_out = nullptr;
    icelk_jpeg_info_t I;
    if (int rc = jpeg_huff_device(c, data, len, &I)) return rc;
    if (tw < 1 || th < 1 || tw > I.width || th > I.height) FAIL(c, ICELK_EARG, "a thumbnail larger than the image, or smaller than one pixel");
    JpegOutArgs O{};
    if (int rc = jpeg_planes(c, &I, nullptr, 0, 0, 0, 0, &O, true)) return rc;
    const size_t bytes = 3 * (size_t)tw * th;
    uint8_t* dst = nullptr;
    if (to_host) {
        if (int rc = grow(c, &c->jpeg.d_rgb, &c->jpeg.rgb_cap, bytes)) return rc;
        dst = c->jpeg.d_rgb;
    } else if (int rc = dmalloc(c, &dst, bytes)) {
        return rc;
    }
    O.dst = dst;
    O.dst_pitch = 3 * tw;
    {
        ProfScope p(c, K_JPEG_THUMB);
        launch_jpeg_thumb(c->stream, O, I.ncomp, tw, th);
    }
    int rc = check_launch(c, "jpeg_thumb");
    if (rc && !to_host) hipFree(dst);
    if (rc) return rc;
    *d_out = dst;
    return ICELK_OK;
}

}  // namespace

}  // namespace icelk

using namespace icelk;

extern "C" {

int icelk_thumb_size(int w, int h_, int box_w, int box_h, int* tw, int* th)
{
    if (!tw || !th || !thumb::size(w, h_, box_w, box_h, tw, th)) return ICELK_EARG;
    return ICELK_OK;
}

int icelk_thumb_host(const uint8_t* img, int w, int h_, int channels, int stride, int tw, int th, uint8_t* out_rgb, int out_stride)
{
    if (!img || !out_rgb || (channels != 1 && channels != 3) || w < 1 || w > thumb::kMaxSource || h_ < 1 || h_ > thumb::kMaxSource) return ICELK_EARG;
    if (tw < 1 || tw > w || th < 1 || th > h_ || (long long)stride < (long long)w * channels || (long long)out_stride < 3LL * tw) return ICELK_EARG;
    try {
        thumb::reduce_host(img, w, h_, channels, (size_t)stride, tw, th, out_rgb, (size_t)out_stride);
    } catch (...) {
        return ICELK_ENOMEM;
    }
    return ICELK_OK;
}

int icelk_jpeg_thumb_file(icelk_t* h, const uint8_t* data, uint64_t len, int tw, int th, uint8_t* out_rgb, int stride)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!out_rgb) FAIL(c, ICELK_EARG, "null output image");
    if ((long long)stride < 3LL * tw) FAIL(c, ICELK_EARG, "stride smaller than a row of the thumbnail");
    HIPCHK(c, hipSetDevice(c->device));
    uint8_t* d = nullptr;
    if (int rc = thumb_of_file(c, data, len, tw, th, true, &d)) return rc;
    HIPCHK(c, hipMemcpy2DAsync(out_rgb, (size_t)stride, d, 3 * (size_t)tw, 3 * (size_t)tw, (size_t)th, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

int icelk_map_inset_set_file(icelk_t* h, int index, const uint8_t* data, uint64_t len, int tw, int th)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (index < 0 || index >= thumb::kMaxInsets) FAIL(c, ICELK_EARG, "an inset index outside 0 .. 7");
    if (tw > thumb::kMaxBox || th > thumb::kMaxBox) FAIL(c, ICELK_EARG, "a thumbnail of more than 16384 pixels a side");
    HIPCHK(c, hipSetDevice(c->device));
    uint8_t* d = nullptr;
    if (int rc = thumb_of_file(c, data, len, tw, th, false, &d)) return rc;
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) hipFree(d);
    HIPCHK(c, e);
    adopt_inset(c, index, d, tw, th);
    return ICELK_OK;
}

int icelk_map_inset_set_pixels(icelk_t* h, int index, const uint8_t* rgb, int tw, int th, int stride)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (index < 0 || index >= thumb::kMaxInsets) FAIL(c, ICELK_EARG, "an inset index outside 0 .. 7");
    if (!rgb || tw < 1 || tw > thumb::kMaxBox || th < 1 || th > thumb::kMaxBox || stride < 3 * tw)
        FAIL(c, ICELK_EARG, "a null thumbnail, a side outside 1 .. 16384, or a stride smaller than a row");
    HIPCHK(c, hipSetDevice(c->device));
    uint8_t* d = nullptr;
    if (int rc = dmalloc(c, &d, 3 * (size_t)tw * th)) return rc;
    const hipError_t e = hipMemcpy2D(d, 3 * (size_t)tw, rgb, (size_t)stride, 3 * (size_t)tw, (size_t)th, hipMemcpyHostToDevice);
    if (e != hipSuccess) hipFree(d);
    HIPCHK(c, e);
    adopt_inset(c, index, d, tw, th);
    return ICELK_OK;
}

int icelk_map_inset_release(icelk_t* h)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    map_insets_free(c);
    return ICELK_OK;
}

}  // extern "C"
