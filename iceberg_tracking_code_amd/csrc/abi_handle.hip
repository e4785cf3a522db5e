// abi_handle.hip -- the handle: create / destroy, the stream-placement probe, switches, sync, the profiling table.
#include <dlfcn.h>

#include <chrono>

#include "icelk_ctx.h"

namespace icelk {

static const char* kKernelNames[K_COUNT_] = {
    "bgr2gray", "pyrdown", "lk", "lk_fb", "corner_candidates", "min_distance", "sort_emit",
    "project_tracks", "synth", "lk_fb_pair", "jpeg_idct", "jpeg_out", "jpeg_huff", "jpeg_fwd",
    "jpeg_enc_count", "jpeg_enc_scan", "jpeg_enc_pack", "jpeg_enc_ff", "jpeg_enc_stuff",
    "jpeg_enc_pack_budget", "jpeg_enc_ff_budget", "jpeg_enc_stuff_budget", "jpeg_crop_rgb", "jpeg_crop_verdict", "jpeg_crop_fwd",
    "plot_background", "plot_clear", "plot_scatter", "plot_resolve",
    "map_clear", "map_cells", "map_polyline", "map_arrows", "map_resolve",
    "jpeg_thumb", "map_inset",
    "png_filter", "png_parse", "png_scan", "png_pack", "png_adler",
    "resize_rows", "resize_cols",
    "grid_segments", "grid_std", "grid_select",
    "ortho_fill", "ortho_add",
    "validate_assign", "validate_pools", "validate_judge",
    "stab_flags", "stab_compact", "stab_median", "stab_rounds", "stab_apply",
    "boxes_assign", "boxes_day_assign", "grid_day_assign",
};

std::string g_create_err;
std::mutex g_mu;

Roctx::Roctx()
{
    if (!getenv("ICELK_ROCTX")) return;
    void* lib = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return;
    push = reinterpret_cast<int (*)(const char*)>(dlsym(lib, "roctxRangePushA"));
    pop = reinterpret_cast<int (*)()>(dlsym(lib, "roctxRangePop"));
    if (!push || !pop) push = nullptr;
}

Roctx& roctx()
{
    static Roctx r;
    return r;
}

void prof_drain(Ctx* c)
{
    for (auto& e : c->evts) {
        hipEventSynchronize(e.b);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
            c->prof_ms[e.id] += ms;
            c->prof_launches[e.id] += 1;
        }
        c->evt_pool.push_back(e);   // reused by later scopes, destroyed with the handle
    }
    c->evts.clear();
}

// the detection chain is ~20 short kernels; a high-priority queue keeps each of them from waiting behind
// the thousands of pending workgroups of the tracker launch it overlaps with
hipError_t create_priority_stream(hipStream_t* s)
{
    int least = 0, greatest = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e != hipSuccess) return e;
    return hipStreamCreateWithPriority(s, hipStreamNonBlocking, greatest);
}

// ---- which hardware queue a side stream lands on matters --------------------------------------------------------------
// The runtime backs every HIP stream with a hardware queue, and the queues sit on a handful of dispatch pipes.  A pipe
// works on one dispatch at a time: while the tracker launch -- ten thousand workgroups, most of them waiting for a wave
// slot for most of the launch -- occupies its pipe, a kernel of ANOTHER queue on the same pipe is not even looked at
// until the last tracker workgroup has gone out.  Which pipe a new stream gets depends on how many queues the process
// has created before (the host framework's included), so it cannot be written down: it is measured.  Eight candidate
// high-priority streams are created; a probe fills the device from stream A with workgroups that idle for ~25 us each
// (~200 us in all) and times a one-wave kernel on stream B beside it -- it comes back after a few microseconds, or
// together with the filler.  The detection stream must not be held up by the compute stream; the candidates stream
// (one long kernel per detection) must not hold up the detection stream; the pyramid stream must be held up by neither
// the compute nor the candidates stream.  Measured on C2: 5 050 pairs/s with the three on pipes of their own, 4 000
// with the candidates stream behind the tracker's pipe.
__global__ void k_probe_idle(unsigned ticks)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz
    for (int guard = 0; guard < 200000; guard++) {
        if (__builtin_amdgcn_s_memrealtime() - t0 >= ticks) break;
        __builtin_amdgcn_s_sleep(8);
    }
}

__global__ void k_probe_tick(unsigned* out)
{
    if (out) *out = 1u;
}

// fraction of the filler's duration (on `busy`) after which a one-wave kernel on `side` completed: ~0.1 when the two
// queues are served independently, ~1 when `side` waits for the filler's dispatch
static double probe_pair(hipStream_t busy, hipStream_t side, hipEvent_t e_busy, hipEvent_t e_side)
{
    using clk = std::chrono::steady_clock;
    hipStreamSynchronize(busy);
    hipStreamSynchronize(side);
    const auto t0 = clk::now();
    hipLaunchKernelGGL(k_probe_idle, dim3(65536), dim3(64), 0, busy, 2500u);
    hipEventRecord(e_busy, busy);
    hipLaunchKernelGGL(k_probe_tick, dim3(1), dim3(64), 0, side, (unsigned*)nullptr);
    hipEventRecord(e_side, side);
    hipEventSynchronize(e_side);
    const auto t1 = clk::now();
    hipEventSynchronize(e_busy);
    const auto t2 = clk::now();
    const double whole = std::chrono::duration<double>(t2 - t0).count();
    const double frac = whole > 0 ? std::chrono::duration<double>(t1 - t0).count() / whole : 1.0;
    if (getenv("ICELK_STREAM_PROBE_LOG"))
        fprintf(stderr, "icelk probe: busy %p side %p: side done after %.2f of %.0f us\n", (void*)busy, (void*)side, frac, 1e6 * whole);
    return frac;
}

static hipError_t create_side_streams(Ctx* c)
{
    constexpr int NC = 8;
    hipStream_t cand[NC] = {nullptr};
    hipEvent_t ea = nullptr, eb = nullptr;
    hipError_t r = hipEventCreateWithFlags(&ea, hipEventDisableTiming);
    if (r == hipSuccess) r = hipEventCreateWithFlags(&eb, hipEventDisableTiming);
    for (int i = 0; i < NC && r == hipSuccess; i++) r = create_priority_stream(&cand[i]);
    if (r == hipSuccess) {
        probe_pair(c->own_stream, cand[0], ea, eb);   // code object load, clocks
        // every candidate beside the compute stream, twice; "held up" = clearly later than the quickest one
        double beside[NC], quickest = 1.0;
        for (int i = 0; i < NC; i++) {
            beside[i] = std::min(probe_pair(c->own_stream, cand[i], ea, eb), probe_pair(c->own_stream, cand[i], ea, eb));
            quickest = std::min(quickest, beside[i]);
        }
        const double limit = std::max(1.6 * quickest, quickest + 0.12);
        bool used[NC] = {false};
        auto pick = [&](auto ok) {
            for (int i = 0; i < NC; i++)
                if (!used[i] && beside[i] <= limit && ok(cand[i])) { used[i] = true; return i; }
            for (int i = 0; i < NC; i++)        // nothing passes (fewer pipes than assumed): the least held up of the rest
                if (!used[i]) { used[i] = true; return i; }
            return 0;
        };
        const int d = pick([&](hipStream_t) { return true; });
        c->det_stream = cand[d];
        const int e = pick([&](hipStream_t s) { return probe_pair(s, c->det_stream, ea, eb) <= limit; });
        c->eig_stream = cand[e];
        const int q = pick([&](hipStream_t s) { return probe_pair(c->eig_stream, s, ea, eb) <= limit; });
        c->pyr_stream = cand[q];
        const int t = pick([&](hipStream_t s) { return probe_pair(c->eig_stream, s, ea, eb) <= limit; });
        c->tail_stream = cand[t];
        c->side_pick[0] = d;
        c->side_pick[1] = e;
        c->side_pick[2] = q;
        c->side_pick[3] = t;
        c->probe_limit = limit;
        c->probe_quickest = quickest;
        if (getenv("ICELK_STREAM_PROBE_LOG"))
            fprintf(stderr, "icelk probe: detection = candidate %d, candidates stream = %d, pyramid = %d (limit %.2f)\n", d, e, q, limit);
        for (int i = 0; i < NC; i++)
            if (!used[i]) hipStreamDestroy(cand[i]);
    } else {
        for (auto s : cand)
            if (s) hipStreamDestroy(s);
    }
    if (ea) hipEventDestroy(ea);
    if (eb) hipEventDestroy(eb);
    return r;
}

static void destroy_ctx(Ctx* c)
{
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    jpeg_async_destroy(c);   // before the slots go: files in flight write into them
    jpeg_resave_destroy(c);
    jpeg_enc_destroy(c);
    plot_destroy(c);
    map_destroy(c);
    ortho_destroy(c);
    stab_destroy(c);
    picture_destroy(c);
    png_destroy(c);
    movie_destroy(c);
    prof_drain(c);
    for (auto& e : c->evt_pool) {
        hipEventDestroy(e.a);
        hipEventDestroy(e.b);
    }
    if (c->d_stamps) {
        std::vector<unsigned long long> hs(3 * c->stamps_cap);
        if (hipMemcpy(hs.data(), c->d_stamps, hs.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            if (FILE* f = fopen(c->stamps_path.c_str(), "wb")) {
                fwrite(hs.data(), 8, hs.size(), f);
                fclose(f);
            }
        }
        hipFree(c->d_stamps);
    }
    if (c->d_iters) hipFree(c->d_iters);
    for (void* b : c->tmpl.buf)
        if (b) hipFree(b);
    for (auto& s : c->slots) {
        if (s.base) hipFree(s.base);
        if (s.ready) hipEventDestroy(s.ready);
        if (s.frame_ev) hipEventDestroy(s.frame_ev);
        if (s.used_own) hipEventDestroy(s.used_own);
        if (s.det_used) hipEventDestroy(s.det_used);
        if (s.eig_used) hipEventDestroy(s.eig_used);
    }
    if (c->det_stream) hipStreamSynchronize(c->det_stream);
    if (c->eig_stream) hipStreamSynchronize(c->eig_stream);
    if (c->det_done) hipEventDestroy(c->det_done);
    if (c->corners_free) hipEventDestroy(c->corners_free);
    if (c->det_stream) hipStreamDestroy(c->det_stream);
    if (c->eig_stream) hipStreamDestroy(c->eig_stream);
    for (auto& b : c->sb) {
        if (b.used_own) hipEventDestroy(b.used_own);
        if (b.ready) hipEventDestroy(b.ready);
    }
    for (auto& e : c->launch_ev)
        if (e) hipEventDestroy(e);
    for (auto& e : c->eo) free_eig_out(e);
    for (auto& S : c->dset) free_det_set(S);
    if (c->h_seg) hipHostFree(c->h_seg);
    void* ptrs[] = {c->d_bgr, c->d_mask, c->d_p0, c->d_p1, c->d_p0r, c->d_err_f, c->d_err_b, c->d_dist, c->d_corners,
                    c->d_st_f, c->d_st_b, c->d_valid, c->dset[0].D.eig, c->d_tracked,
                    c->d_out_tracks, c->d_out_quality, c->post.d_proj, c->post.d_keep, c->post.d_cube_u, c->post.d_cube_v,
                    c->post.d_cube_count, c->calib.d_shore, c->calib.d_water, c->jpeg.d_rgb};
    jpeg_dec_free(c->jpeg.sync);
    for (void* p : ptrs)
        if (p) hipFree(p);
    for (auto& S : c->sb) {
        void* sp[] = {S.live, S.alive, S.order, S.order_border, S.tracks, S.quality};
        for (void* p : sp)
            if (p) hipFree(p);
    }
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    for (auto q : c->copy_hi)
        if (q) {
            hipStreamSynchronize(q);
            hipStreamDestroy(q);
        }
    if (c->pyr_stream) {
        hipStreamSynchronize(c->pyr_stream);
        hipStreamDestroy(c->pyr_stream);
    }
    if (c->tail_stream) {
        hipStreamSynchronize(c->tail_stream);
        hipStreamDestroy(c->tail_stream);
    }
    delete c;
}

}  // namespace icelk

using namespace icelk;

extern "C" {

int icelk_version(void) { return 100; }

const char* icelk_last_error(icelk_t* h)
{
    if (!h) return g_create_err.c_str();
    return C(h)->err.c_str();
}

int icelk_create(int device, int max_w, int max_h, int n_slots, int max_pts, icelk_t** out)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (!out || max_w <= 0 || max_h <= 0 || max_w > 65535 || max_h > 65535 || n_slots <= 0 || max_pts <= 0) {
        g_create_err = "icelk_create: bad argument";
        return ICELK_EARG;
    }
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) {
        g_create_err = std::string("icelk_create: no HIP device (") + hipGetErrorString(e) + ")";
        return ICELK_EHIP;
    }
    if (device < 0 || device >= ndev) {
        g_create_err = "icelk_create: device index out of range";
        return ICELK_EARG;
    }
    e = hipSetDevice(device);
    if (e != hipSuccess) {
        g_create_err = std::string("hipSetDevice: ") + hipGetErrorString(e);
        return ICELK_EHIP;
    }
    Ctx* c = new Ctx();
    c->device = device;
    c->max_w = max_w;
    c->max_h = max_h;
    c->n_slots = n_slots;
    c->max_pts = max_pts;
    int rc = ICELK_OK;
    auto fail = [&](int code) {
        g_create_err = c->err;
        destroy_ctx(c);
        return code;
    };
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
        create_side_streams(c) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&c->h_seg), 64, hipHostMallocMapped) != hipSuccess ||
        hipEventCreateWithFlags(&c->det_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->corners_free, hipEventDisableTiming) != hipSuccess) {
        c->err = "hipStreamCreate failed";
        return fail(ICELK_EHIP);
    }
    c->stream = c->own_stream;
    c->slots.resize(n_slots);
    const size_t sb = slot_bytes(max_w, max_h);
    for (auto& s : c->slots) {
        if ((rc = dmalloc(c, &s.base, sb))) return fail(rc);
        s.bytes = sb;
        if (hipEventCreateWithFlags(&s.ready, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s.frame_ev, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s.used_own, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s.det_used, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s.eig_used, hipEventDisableTiming) != hipSuccess) {
            c->err = "hipEventCreate failed";
            return fail(ICELK_EHIP);
        }
        s.used = s.used_own;
        layout_levels(s, max_w, max_h);
        if (!layout_ok(s)) {
            c->err = "slot layout violates the dword-access invariant (internal)";
            return fail(ICELK_ECAP);
        }
    }
    for (auto& S : c->sb) {
        if (hipEventCreateWithFlags(&S.used_own, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&S.ready, hipEventDisableTiming) != hipSuccess) {
            c->err = "hipEventCreate failed";
            return fail(ICELK_EHIP);
        }
        S.used = S.used_own;
    }
    for (auto& e : c->launch_ev)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            c->err = "hipEventCreate failed";
            return fail(ICELK_EHIP);
        }
    const size_t npx = (size_t)max_w * max_h;
    c->bgr_pitch = align_up(3 * max_w, kPitchAlign);
    c->mask_pitch = align_up(max_w, kPitchAlign);
    const size_t np = (size_t)max_pts;
    const int cand_cap = (int)std::min<size_t>(candidate_capacity(max_w, max_h), (size_t)1 << 30);
    c->ncell_cap = npx + 1;
    if ((rc = dmalloc(c, &c->d_bgr, (size_t)c->bgr_pitch * max_h)) || (rc = dmalloc(c, &c->d_mask, (size_t)c->mask_pitch * max_h)) ||
        (rc = dmalloc(c, &c->d_p0, 2 * np)) || (rc = dmalloc(c, &c->d_p1, 2 * np)) || (rc = dmalloc(c, &c->d_p0r, 2 * np)) ||
        (rc = dmalloc(c, &c->d_err_f, np)) || (rc = dmalloc(c, &c->d_err_b, np)) || (rc = dmalloc(c, &c->d_dist, np)) ||
        (rc = dmalloc(c, &c->d_corners, 2 * np)) || (rc = dmalloc(c, &c->d_st_f, np)) || (rc = dmalloc(c, &c->d_st_b, np)) ||
        (rc = dmalloc(c, &c->d_valid, np)) || (rc = dmalloc(c, &c->dset[0].D.eig, npx)) || (rc = dmalloc(c, &c->d_tracked, 64)) ||
        (rc = dmalloc(c, &c->d_out_tracks, np * kMaxVert * 2)) || (rc = dmalloc(c, &c->d_out_quality, np * (kMaxVert - 1))))
        return fail(rc);
    for (auto& S : c->sb)
        if ((rc = dmalloc(c, &S.live, 2 * np)) || (rc = dmalloc(c, &S.alive, np)) || (rc = dmalloc(c, &S.order, np)) ||
            (rc = dmalloc(c, &S.order_border, 1)) || (rc = dmalloc(c, &S.tracks, np * kMaxVert * 2)) ||
            (rc = dmalloc(c, &S.quality, np * (kMaxVert - 1))))
            return fail(rc);
    c->use_order = getenv("ICELK_NO_ORDER") == nullptr;
    c->pyr_per_level = getenv("ICELK_PYR_PER_LEVEL") != nullptr;
    c->tmpl.off = getenv("ICELK_NO_TEMPLATE_REUSE") != nullptr;
    if (const char* tb = getenv("ICELK_TEMPLATE_BUDGET_MB")) c->tmpl.budget = (size_t)std::max(atoll(tb), 0LL) << 20;
    c->host_tail = getenv("ICELK_HOST_TAIL") != nullptr;
    if (const char* fs = getenv("ICELK_TAIL_FORCE_STATUS")) c->tail_force_status = std::min(std::max(atoi(fs), 0), 4);
    if ((rc = dmalloc(c, &c->d_iters, (size_t)max_pts))) return fail(rc);
    if (const char* sp = getenv("ICELK_LK_STAMPS")) {
        c->stamps_path = sp;
        c->stamps_cap = (size_t)max_pts + 8;
        if ((rc = dmalloc(c, &c->d_stamps, 3 * c->stamps_cap))) return fail(rc);
    }
    if (const char* k = getenv("ICELK_LK_KERNEL")) {   // A/B measurements: "generic" | "multi" (default: one feature per wave)
        if (!strcmp(k, "generic")) c->lk_kernel_flags = ICELK_FLAG_GENERIC_KERNEL;
        else if (!strcmp(k, "multi")) c->lk_kernel_flags = ICELK_FLAG_MULTI_PER_WAVE;
    }
    // three candidate buffers and two detector sets (everything a detection in flight owns; the full-frame eigenvalue
    // map of icelk_min_eig_map is shared)
    for (auto& e : c->eo)
        if ((rc = alloc_eig_out(c, e, cand_cap))) return fail(rc);
    for (int k = 0; k < 2; k++) {
        Ctx::DetSet& S = c->dset[k];
        S.D.eig = c->dset[0].D.eig;
        if ((rc = alloc_det_set(c, S, cand_cap))) return fail(rc);
        activate_eig_out(c, S, k);
    }
    if (hipMemset(c->d_tracked, 0, 64 * 8) != hipSuccess) {
        c->err = "hipMemset failed";
        return fail(ICELK_EHIP);
    }
    // The host's tail (detect_finish) sorts with rocPRIM, and the first launch of its kernels in a process costs the host
    // ~8 ms (the code object of k_sort.hip is loaded then).  With the device-driven tail that first time was some
    // detection in the MIDDLE of a run -- the first one the device handed back -- and a 64-pair batch lasted 26 ms instead
    // of 17 (profiles/r04_c3_stall.txt).  Paid here instead: 64 keys through the sort, once per handle.
    DetectScratch& D0 = c->dset[0].D;
    if (hipMemsetAsync(D0.acc, 0, 64 * sizeof(unsigned long long), c->tail_stream) != hipSuccess) {
        c->err = "hipMemset failed";
        return fail(ICELK_EHIP);
    }
    sort_keys_desc(c->tail_stream, D0, D0.acc, D0.acc_sorted, 64);
    if (hipStreamSynchronize(c->tail_stream) != hipSuccess) {
        c->err = "warm-up sort failed";
        return fail(ICELK_EHIP);
    }
    *out = reinterpret_cast<icelk_t*>(c);
    return ICELK_OK;
}

int icelk_destroy(icelk_t* h)
{
    if (!h) return ICELK_EARG;
    destroy_ctx(C(h));
    return ICELK_OK;
}

int icelk_set_stream(icelk_t* h, void* hip_stream)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
    return ICELK_OK;
}

int icelk_sync(icelk_t* h)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    int rcf = flush_deferred(c);   // a pair waiting for a partner counts as issued work
    if (rcf) return rcf;
    // every stream of the handle: uploads / JPEG files decoded ahead / pyramids built ahead, candidate kernels of a prepared detection
    // (icelk_seg_detect_prepare), the min-distance / sort / emit stage, tracker launches
    for (auto q : c->copy_hi)
        if (q) HIPCHK(c, hipStreamSynchronize(q));
    if (int rcj = jpeg_async_sync(c)) return rcj;
    HIPCHK(c, hipStreamSynchronize(c->pyr_stream));
    HIPCHK(c, hipStreamSynchronize(c->eig_stream));
    HIPCHK(c, hipStreamSynchronize(c->det_stream));
    HIPCHK(c, hipStreamSynchronize(c->tail_stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

int icelk_set_lk_kernel(icelk_t* h, int which)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (which != 0 && which != ICELK_FLAG_GENERIC_KERNEL && which != ICELK_FLAG_MULTI_PER_WAVE)
        FAIL(c, ICELK_EARG, "bad kernel selector");
    c->lk_kernel_flags = which;
    return ICELK_OK;
}

int icelk_set_variant(icelk_t* h, const char* name, int value)
{
    if (!h || !name) return ICELK_EARG;
    Ctx* c = C(h);
    if (!strcmp(name, "lk_sums") && value >= 0 && value <= 2) c->lk_sum_mode = value;
    else if (!strcmp(name, "lk_wide_sums") && (value == 0 || value == 1)) c->lk_wide_sums = value;
    else if (!strcmp(name, "sobel_fma") && value >= 0 && value <= 3) c->corner_variant = (c->corner_variant & 4) | value;
    else if (!strcmp(name, "eig_fma") && (value == 0 || value == 1)) c->corner_variant = (c->corner_variant & 3) | (value << 2);
    else if (!strcmp(name, "harris_tail") && (value == 0 || value == 1)) c->harris_tail = value;
    else FAIL(c, ICELK_EARG, "unknown variant / value");
    for (auto& e : c->eo) e.valid = false;     // candidates prepared under another variant are not adopted
    return ICELK_OK;
}

int icelk_set_fb_distance(icelk_t* h, int form)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (form != ICELK_FB_HYPOT && form != ICELK_FB_SQRT) FAIL(c, ICELK_EARG, "bad forward-backward distance form");
    c->fb_dist_form = form;
    return ICELK_OK;
}

// ---- measurement -------------------------------------------------------------------------------
int icelk_prof_enable(icelk_t* h, int on)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!on) prof_drain(c);
    c->prof = on != 0;
    c->prof_tracker_only = on == 2;
    return ICELK_OK;
}

int icelk_prof_reset(icelk_t* h)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    prof_drain(c);
    for (int i = 0; i < K_COUNT_; i++) {
        c->prof_launches[i] = 0;
        c->prof_ms[i] = 0;
    }
    return ICELK_OK;
}

int icelk_prof_iterations(icelk_t* h, uint32_t* host_out, int cap, int* out_n)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    if (!out_n || cap < 0 || (cap > 0 && !host_out)) FAIL(c, ICELK_EARG, "bad output buffer");
    *out_n = c->iters_n;
    if (host_out && cap > 0 && c->iters_n > 0) {
        const int n = c->iters_n < cap ? c->iters_n : cap;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(host_out, c->d_iters, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
    }
    return ICELK_OK;
}

int icelk_stream_probe_info(icelk_t* h, int* picks, double* quickest, double* limit)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (picks)
        for (int k = 0; k < 4; k++) picks[k] = c->side_pick[k];
    if (quickest) *quickest = c->probe_quickest;
    if (limit) *limit = c->probe_limit;
    return ICELK_OK;
}

int icelk_prof_count(void) { return K_COUNT_; }

const char* icelk_prof_name(int kernel_id)
{
    if (kernel_id < 0 || kernel_id >= K_COUNT_) return "";
    return kKernelNames[kernel_id];
}

int icelk_prof_get(icelk_t* h, int kernel_id, int* launches, double* total_ms)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (kernel_id < 0 || kernel_id >= K_COUNT_) FAIL(c, ICELK_EARG, "bad kernel id");
    prof_drain(c);
    if (launches) *launches = c->prof_launches[kernel_id];
    if (total_ms) *total_ms = c->prof_ms[kernel_id];
    return ICELK_OK;
}

}  // extern "C"
