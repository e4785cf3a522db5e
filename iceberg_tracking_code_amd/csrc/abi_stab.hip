// abi_stab.hip -- camera shake fitted to land anchors.  The rules are stab.h, the kernels k_stab.hip's.
//
//   host    icelk_stab_tracks_host, icelk_stab_anchor_flags_host: stab.h on the CPU; no handle, re-entrant
//   device  icelk_stab_tracks: the caller's table into the handle's read-out buffer (as icelk_project_tracks), the caller's
//           flags up, the five kernels, table and results down, one wait.  icelk_seg_stab_read: seg_gather_counted leaves
//           the table in the same buffer and its row count ON THE DEVICE, where the kernels read it (their grids are sized
//           for the segment's corners); the flags come from the resident anchor mask; then table, quality, flags, results
//           and the count come down behind ONE wait -- the caller's rows are copied, and a count above them is ICELK_ECAP
//           after the fact.  The sizing call (tracks NULL) is icelk_seg_read's and waits for the count
// The scratch is allocated at first use for max_pts rows and freed with the handle; the order keys of the start medians and
// the inlier bytes are a stretch per vertex and grow with the vertices seen.  Bounds: k_stab.hip's header states them;
// n <= max_pts and 2 <= V <= 17 are checked here before every launch.
#include <vector>

#include "icelk_ctx.h"

namespace icelk {

void stab_destroy(Ctx* c)
{
    Ctx::Stab& S = c->stab;
    for (void* p : {(void*)S.d_mask, (void*)S.d_flags, (void*)S.d_anchor, (void*)S.d_w, (void*)S.d_idx, (void*)S.d_keys, (void*)S.d_med,
                    (void*)S.d_out})
        if (p) hipFree(p);
    S = Ctx::Stab{};
}

namespace {

struct Results {   // the caller's per-vertex arrays
    double* motion;
    int32_t* inliers;
    double* rms;
    int32_t *status, *rounds_used;
    int* n_anchors;
    bool complete() const { return motion && inliers && rms && status && rounds_used; }
};

void deliver(const stab::VertexResult* R, int V, int n_a, const Results& out)
{
    for (int k = 0; k < V - 1; k++) {
        out.motion[4 * k] = R[k].m.a, out.motion[4 * k + 1] = R[k].m.b, out.motion[4 * k + 2] = R[k].m.tx, out.motion[4 * k + 3] = R[k].m.ty;
        out.inliers[k] = R[k].inliers, out.rms[k] = R[k].rms, out.status[k] = R[k].status, out.rounds_used[k] = R[k].rounds_used;
    }
    if (out.n_anchors) *out.n_anchors = n_a;
}

int stab_grow(Ctx* c, int V)
{
    Ctx::Stab& S = c->stab;
    const size_t rows = (size_t)std::max(c->max_pts, 1);
    if (!S.ready) {
        if (int rc = dmalloc(c, &S.d_flags, rows)) return rc;
        if (int rc = dmalloc(c, &S.d_anchor, rows)) return rc;
        if (int rc = dmalloc(c, &S.d_idx, rows)) return rc;
        if (int rc = dmalloc(c, &S.d_med, (size_t)2 * (kMaxVert - 1))) return rc;
        if (int rc = dmalloc(c, &S.d_out, 1)) return rc;
        S.ready = true;
    }
    if (int rc = grow(c, &S.d_keys, &S.keys_cap, rows * 2 * (size_t)(V - 1))) return rc;
    return grow(c, &S.d_w, &S.w_cap, rows * (size_t)(V - 1));
}

// the five kernels over the n x V table in d_out_tracks (n_ptr: at most n rows, counted on the device); in_flags: d_flags holds
// the caller's flags (else the mask gives them)
int stab_on(Ctx* c, int n, const int* n_ptr, int V, const icelk_stab_params_t& P, bool in_flags)
{
    Ctx::Stab& S = c->stab;
    StabArgs A{};
    A.tracks = c->d_out_tracks, A.n = n, A.n_ptr = n_ptr, A.V = V;
    A.in_flags = in_flags ? S.d_flags : nullptr;
    A.mask = S.d_mask, A.mask_w = S.mask_w, A.mask_h = S.mask_h;
    A.flags = S.d_flags, A.anchor = S.d_anchor, A.idx = S.d_idx, A.n_a = &S.d_out->n_a;
    A.keys = S.d_keys, A.w = S.d_w, A.stride = (size_t)std::max(c->max_pts, 1), A.med = S.d_med, A.res = S.d_out->res, A.P = P;
    for (int step = 0; step < STAB_STEPS; step++) {
        {
            ProfScope p(c, K_STAB_FLAGS + step);
            launch_stab_step(c->stream, A, step);
        }
        if (int rc = check_launch(c, "stab")) return rc;
    }
    return ICELK_OK;
}

bool shape_ok(int n, int V) { return n >= 0 && V >= 2 && V <= stab::kMaxVert; }

}  // namespace

}  // namespace icelk

using namespace icelk;

extern "C" {

int icelk_stab_tracks_host(const float* tracks, const uint8_t* flags, int n, int n_vertices, const icelk_stab_params_t* params_or_null,
                           float* out_tracks, double* motion, int32_t* inliers, double* rms, int32_t* status, int32_t* rounds_used,
                           int* n_anchors)
{
    const Results out{motion, inliers, rms, status, rounds_used, n_anchors};
    if (!shape_ok(n, n_vertices) || !out.complete() || (n > 0 && (!tracks || !flags || !out_tracks))) return ICELK_EARG;
    const icelk_stab_params_t P = params_or_null ? *params_or_null : stab::default_params();
    if (!stab::params_ok(P)) return ICELK_EARG;
    std::vector<int> idx((size_t)n + 1);
    std::vector<uint8_t> w((size_t)n + 1);
    stab::VertexResult R[stab::kMaxVert - 1];
    const int n_a = stab::run_host(tracks, flags, n, n_vertices, P, idx.data(), w.data(), out_tracks, R);
    deliver(R, n_vertices, n_a, out);
    return ICELK_OK;
}

int icelk_stab_anchor_flags_host(const float* tracks, int n, int n_vertices, const uint8_t* mask, int w, int h_, int stride, uint8_t* flags)
{
    if (n < 0 || n_vertices < 1 || !mask || w < 1 || h_ < 1 || stride < w || (n > 0 && (!tracks || !flags))) return ICELK_EARG;
    stab::flags_host(tracks, n, n_vertices, mask, w, h_, (size_t)stride, flags);
    return ICELK_OK;
}

int icelk_stab_tracks(icelk_t* h, const float* tracks, const uint8_t* flags, int n, int n_vertices, const icelk_stab_params_t* params_or_null,
                      float* out_tracks, double* motion, int32_t* inliers, double* rms, int32_t* status, int32_t* rounds_used,
                      int* n_anchors)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    const Results out{motion, inliers, rms, status, rounds_used, n_anchors};
    if (!shape_ok(n, n_vertices) || !out.complete() || (n > 0 && (!tracks || !flags || !out_tracks)))
        FAIL(c, ICELK_EARG, "a null pointer, n < 0 or vertices outside 2 .. 17");
    const icelk_stab_params_t P = params_or_null ? *params_or_null : stab::default_params();
    if (!stab::params_ok(P)) FAIL(c, ICELK_EARG, "a stabilisation parameter outside its range");
    if (n > c->max_pts) FAIL(c, ICELK_ECAP, "more tracks than max_pts of icelk_create");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = stab_grow(c, n_vertices)) return rc;
    Ctx::Stab& S = c->stab;
    const size_t floats = (size_t)n * n_vertices * 2;
    if (n > 0) {
        HIPCHK(c, copy_n(c->d_out_tracks, tracks, floats, kH2D, c->stream));
        HIPCHK(c, copy_n(S.d_flags, flags, (size_t)n, kH2D, c->stream));
    }
    if (int rc = stab_on(c, n, nullptr, n_vertices, P, true)) return rc;
    StabOut O;
    if (n > 0) HIPCHK(c, copy_n(out_tracks, c->d_out_tracks, floats, kD2H, c->stream));
    HIPCHK(c, copy_n(&O, S.d_out, 1, kD2H, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    deliver(O.res, n_vertices, O.n_a, out);
    return ICELK_OK;
}

int icelk_stab_set_anchor_mask(icelk_t* h, const uint8_t* host_mask, int w, int h_, int stride)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    Ctx::Stab& S = c->stab;
    HIPCHK(c, hipSetDevice(c->device));
    if (!host_mask) {
        if (S.d_mask) HIPCHK(c, hipFree(S.d_mask));   // waits for whatever still reads it
        S.d_mask = nullptr, S.mask_w = S.mask_h = 0;
        return ICELK_OK;
    }
    if (w < 1 || h_ < 1 || w > c->max_w || h_ > c->max_h || stride < w) FAIL(c, ICELK_EARG, "an anchor mask larger than the handle's frames, or a stride below its width");
    if (S.d_mask) HIPCHK(c, hipFree(S.d_mask));
    S.d_mask = nullptr, S.mask_w = S.mask_h = 0;
    if (int rc = dmalloc(c, &S.d_mask, (size_t)w * h_)) return rc;
    HIPCHK(c, hipMemcpy2DAsync(S.d_mask, (size_t)w, host_mask, (size_t)stride, (size_t)w, (size_t)h_, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // the caller's mask has been read
    S.mask_w = w, S.mask_h = h_;
    return ICELK_OK;
}

int icelk_seg_stab_read(icelk_t* h, int closed, const icelk_stab_params_t* params_or_null, float* tracks, float* quality, uint8_t* flags,
                        int cap, int max_vertices, int* out_n, int* out_vertices, double* motion, int32_t* inliers, double* rms,
                        int32_t* status, int32_t* rounds_used, int* n_anchors)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    Ctx::Stab& S = c->stab;
    const icelk_stab_params_t P = params_or_null ? *params_or_null : stab::default_params();
    if (!stab::params_ok(P)) FAIL(c, ICELK_EARG, "a stabilisation parameter outside its range");
    if (!S.d_mask) FAIL(c, ICELK_ESTATE, "no anchor mask has been set (icelk_stab_set_anchor_mask)");
    HIPCHK(c, hipSetDevice(c->device));
    if (!tracks) {   // sizing, as icelk_seg_read: the count costs a wait of its own
        return closed ? icelk_seg_read_closed(h, nullptr, nullptr, 0, 0, out_n, out_vertices) : icelk_seg_read(h, nullptr, nullptr, 0, 0, out_n, out_vertices);
    }
    const Results out{motion, inliers, rms, status, rounds_used, n_anchors};
    if (!out.complete() || cap < 0) FAIL(c, ICELK_EARG, "null result arrays");
    if (int rc = stab_grow(c, 2)) return rc;   // the row numbers and counts; the per-vertex stretches once the vertices are known
    // the gather counts the rows on the device and every kernel behind it reads the count there: no host look until the end
    int* d_n = &S.d_out->n;
    int upper = 0, nv = 0;
    if (int rc = seg_gather_counted(c, closed != 0, d_n, &upper, &nv)) return rc;
    if (out_vertices) *out_vertices = nv;
    if (nv > max_vertices) FAIL(c, ICELK_ECAP, "host track buffers too small");
    if (nv < 2) FAIL(c, ICELK_ESTATE, "the segment has no pair yet: nothing to stabilise");
    if (int rc = stab_grow(c, nv)) return rc;
    if (int rc = stab_on(c, upper, d_n, nv, P, false)) return rc;
    StabOut O;
    const int rows = std::min(cap, upper);   // the caller's rows: all of the table's, or *out_n says that they were too few
    if (rows > 0) {
        HIPCHK(c, hipMemcpy2DAsync(tracks, sizeof(float) * 2 * max_vertices, c->d_out_tracks, sizeof(float) * 2 * nv, sizeof(float) * 2 * nv, rows,
                                   hipMemcpyDeviceToHost, c->stream));
        if (quality)
            HIPCHK(c, hipMemcpy2DAsync(quality, sizeof(float) * (max_vertices - 1), c->d_out_quality, sizeof(float) * (nv - 1),
                                       sizeof(float) * (nv - 1), rows, hipMemcpyDeviceToHost, c->stream));
        if (flags) HIPCHK(c, copy_n(flags, S.d_flags, (size_t)rows, kD2H, c->stream));
    }
    HIPCHK(c, copy_n(&O, S.d_out, 1, kD2H, c->stream));   // the results, the anchors and the rows in one copy
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (out_n) *out_n = O.n;
    if (O.n > cap) FAIL(c, ICELK_ECAP, "host track buffers too small");
    deliver(O.res, nv, O.n_a, out);
    return ICELK_OK;
}

}  // extern "C"
