// zr_accum.cpp — the accumulator side of the C ABI (include/zr_capi.h): a frame in batches of samples whose lane sums stay on the device (zr_accum),
// adaptive sampling on top of them (§12), the queries of what an accumulator holds, and render_batched, the accumulator zr_render makes for an oversized frame.
#include "zr_frame.h"

namespace zr_host {
namespace {

// What a zr_accum holds.  The lane sums live in d_partial ([pixel][channel][lane], zr_launch.h: ACCUM_DOUBLES_PER_PIXEL), pixel k being the k-th of the plan's
// pixels in tile order (d_pixels) whichever way the pipeline's own list runs.
struct AccumState {
    zr_ctx* ctx = nullptr; int device = 0;
    Plan plan;
    DevBuf<double> d_partial; DevBuf<uint32_t> d_pixels; uint32_t n_pix = 0;
    int first = 0, done = 0;
    int route = 2;                 // zr_counters::path of the batches so far: which one-shot kernel's pairing the resolve follows
    uint32_t direct = 0;           // bound to the direct-light integrator (zr_accum_set_direct): 0x80000000 | its flags; create to destroy, resets included
    bool bound = false;            // a batch has been added since create / reset: later ones must bring the same camera, seed and scene
    zr_camera cam{}; uint64_t seed = 0; const zr_scene* scene = nullptr; uint64_t scene_epoch = 0;   // (the scene as refitted so often: zr_scene_refit)
    // adaptive sampling (zr_render_adaptive), allocated by its first run: the sample count per pixel, the active list and its slot index
    // (two of each: a pass compacts one into the other), the flags per list position and the compaction's block counts and totals
    bool adaptive = false;         // an adaptive pass has completed since create / reset: the counts are per pixel (d_count) and `done` is the largest
    DevBuf<int32_t> d_count; DevBuf<uint32_t> d_list[2], d_slot[2], d_flag, d_block_active, d_block_at_max, d_totals;
    static zr_camera key_of(zr_camera c) { c.samples_per_pixel = 0; return c; }   // the camera as the binding compares it: its sample count is ignored here
    void bind(const zr_camera& c, uint64_t sd, const zr_scene* s) { if (!bound) { bound = true; cam = key_of(c); seed = sd; scene = s; scene_epoch = s->epoch; } }   // by the first samples added
    size_t sums() const { return (size_t)n_pix * zr::ACCUM_DOUBLES_PER_PIXEL; }
    size_t device_bytes() const {
        return sums() * sizeof(double) + (size_t)n_pix * sizeof(uint32_t) + d_count.n * sizeof(int32_t) +
               (d_list[0].n + d_list[1].n + d_slot[0].n + d_slot[1].n + d_flag.n + d_block_active.n + d_block_at_max.n + d_totals.n) * sizeof(uint32_t);
    }
};

// the storage of an accumulator of a.plan: the pixel list and the lane sums, which accum_zero clears; idle: a stream to synchronise before the sums are allocated
int accum_storage(AccumState& a, zr_ctx* c, const hipStream_t* idle) {
    const std::vector<uint32_t> pix = plan_pixels(a.plan);
    a.ctx = c; a.device = c->device; a.n_pix = (uint32_t)pix.size();   // (sides of at most ST_MAX_FRAME_SIDE: fewer than 2^32 pixels)
    if (int rc = a.d_pixels.upload(pix)) return rc;
    if (idle) HIP_OK(hipStreamSynchronize(*idle));
    if (a.d_partial.alloc(a.sums()) != ZR_OK) return fail(ZR_E_NOMEM, "no device memory for the lane sums of %u pixels (%zu bytes)", a.n_pix, a.sums() * sizeof(double));
    return ZR_OK;
}

// Nothing held.  whole_device: zeroed on the null stream and the device synchronised (the context's streams do not wait for the null stream); else in `stream`'s order.
int accum_zero(AccumState& a, hipStream_t stream, bool whole_device) {
    const size_t bytes = std::max<size_t>(a.sums() * sizeof(double), 64);
    if (whole_device) { HIP_OK(hipMemset(a.d_partial.p, 0, bytes)); HIP_OK(hipDeviceSynchronize()); }
    else HIP_OK(hipMemsetAsync(a.d_partial.p, 0, bytes, stream));
    a.done = 0; a.bound = false; a.adaptive = false;
    return ZR_OK;
}

// The samples [sample0, sample0 + n) of n_pix listed pixels as per-sample radiance in zr_ctx::d_partial ([pixel][n][3]), by the route zr_render takes for this scene and
// camera.  job: plan, camera, environment, seed, stream, count and keep_going as the caller left them.  `pixels` is what the pixel-group route renders; the pipeline
// renders job.d_list when that is set (the same list) and otherwise the plan's cached list, *flipped then saying that it ran in the reverse of the plan's order
// (list_runs_reversed).  Nothing but d_partial and the counters is written: the caller adds the samples to its sums, or drops them.
int render_batch_samples(zr_ctx* c, const zr_scene* s, FrameJob& job, const uint32_t* pixels, uint32_t n_pix, int sample0, int n, HostTimer& timer, bool* flipped) {
    job.dc.spp = n; job.sample0 = (uint32_t)sample0; job.d_out = nullptr; job.d_out2 = nullptr; job.progress = nullptr; job.rows_done = nullptr;
    *flipped = false;
    if (job.keep_going && *job.keep_going == 0) return fail(ZR_E_CANCELLED, "batch cancelled before it began");
    const uint64_t units = (uint64_t)n_pix * (uint64_t)n;
    if (job.direct) return render_direct_samples(c, s, job, pixels, n_pix, sample0, n, timer);   // the one place a direct accumulator's batches leave the plain routes
    if (fits_stream(c, s, job.plan, job.dc, 1, 0)) {
        if (units > zr::ST_MAX_UNITS) return fail(ZR_E_NOMEM, "a batch of %d samples is %llu work units, the pipeline numbers 2^32 - 1 per run: ask for fewer samples", n, (unsigned long long)units);
        *flipped = !job.d_list && list_runs_reversed();
        return render_stream(c, s, job);
    }
    // the pixel-group route: the batch's per-sample radiance
    if (units > (1ull << 37)) return fail(ZR_E_NOMEM, "a batch of %d samples is %llu samples of radiance: ask for fewer", n, (unsigned long long)units);
    if (c->d_partial.n < units * 3) {
        HIP_OK(hipStreamSynchronize(job.stream));
        if (c->d_partial.alloc(units * 3) != ZR_OK) return fail(ZR_E_NOMEM, "no device memory for the per-sample radiance buffer (%zu bytes): ask for fewer samples", (size_t)units * 3 * sizeof(double));
    }
    c->last_path = 0;
    if (c->pending.size() > 4096) { int rr = resolve_times(c); if (rr) return rr; }
    c->render_id++; c->last_stream = job.stream; c->last_counted = job.count;
    timer.begin(job.stream, 1);
    HIP_OK(zr::launch_render_samples(s->ds, job.dc, job.de, job.seed, pixels, n_pix, (uint32_t)sample0, (uint32_t)n, c->d_partial.p, c->d_ctr.p, job.count, job.stream));
    timer.end(job.stream, 1);
    if (job.keep_going) {
        HIP_OK(hipStreamSynchronize(job.stream));
        if (*job.keep_going == 0) return fail(ZR_E_CANCELLED, "batch cancelled");
    }
    return ZR_OK;
}

// One batch: the samples [sample0, sample0 + n) of every pixel of the accumulator by the route zr_render takes for this scene and camera, added to the lane sums.
// The batch is rendered whole before the sums are touched: on any failure — ZR_E_CANCELLED, ZR_E_NOMEM (this many samples do not fit the route in one run) — they
// are as they were.
int accumulate_batch(zr_ctx* c, const zr_scene* s, FrameJob& job, AccumState& a, int sample0, int n) {
    c->last_rounds = 0;
    HIP_OK(hipMemsetAsync(c->d_ctr.p, 0, zr::CTR_BLOCK * sizeof(unsigned long long), job.stream));
    if (a.n_pix == 0) return ZR_OK;
    HostTimer timer(c);
    bool flipped = false;
    int rc = render_batch_samples(c, s, job, a.d_pixels.p, a.n_pix, sample0, n, timer, &flipped);
    if (rc) return rc;
    timer.begin(job.stream, 3);
    HIP_OK(zr::launch_accumulate(c->d_partial.p, a.n_pix, (uint32_t)n, (uint32_t)sample0, flipped, a.d_partial.p, job.stream));
    timer.end(job.stream, 3);
    if ((rc = timer.status())) return rc;
    HIP_OK(hipStreamSynchronize(job.stream));
    a.route = c->last_path;
    return ZR_OK;
}

// the mean of the samples held, into the accumulator's pixels of the device frame d_out, with the pairing of the kernel that rendered them (zr_stream.hip: accum_resolve)
int accum_resolve_into(const AccumState& a, double* d_out, hipStream_t stream) {
    // per-pixel counts are all at least 64, where lanes_for gives 64
    if (a.adaptive) HIP_OK(zr::launch_accum_resolve_counts(a.d_partial.p, a.d_pixels.p, a.d_count.p, a.n_pix, a.plan.W, a.route == 0 ? 64 : 1, d_out, stream));
    else HIP_OK(zr::launch_accum_resolve(a.d_partial.p, a.d_pixels.p, a.n_pix, a.plan.W, a.done, a.route == 0 ? lanes_for(a.done) : 1, d_out, stream));
    return ZR_OK;
}
// A query kernel's launch as zr_get_kernel_times sees it under ZR_TIMELOG_KIND=4 (the variance and the robust resolve: profiles/robust_resolve.txt compares them).
// It belongs to no render (render_id 0: renders count from 1, and RunTotals::finish adopts only later ids): zr_counters' kernel times stay the renders' own.
struct QueryTimer {
    HostTimer t; hipStream_t stream;
    QueryTimer(zr_ctx* c, hipStream_t stream) : t(c), stream(stream) { if (c->pending.size() > 4096) (void)resolve_times(c); t.begin(stream, 4); }
    ~QueryTimer() { const size_t n = t.c->pending.size(); t.end(stream, 4); if (t.c->pending.size() > n) t.c->pending.back().render_id = 0; }
};
int accum_variance_into(const AccumState& a, double* d_out, hipStream_t stream) {
    QueryTimer timer(a.ctx, stream);
    HIP_OK(zr::launch_accum_variance(a.d_partial.p, a.d_pixels.p, a.adaptive ? a.d_count.p : nullptr, a.done, a.n_pix, a.plan.W, d_out, stream));
    return ZR_OK;
}
// the robust colour, the variance of that mean and the trim (either may be null) into the accumulator's pixels of device frames (zr_robust.hip)
int accum_robust_into(const AccumState& a, const zr_robust_params& rp, double* d_out, double* d_var, int32_t* d_trim, hipStream_t stream) {
    QueryTimer timer(a.ctx, stream);
    HIP_OK(zr::launch_accum_resolve_robust(a.d_partial.p, a.d_pixels.p, a.adaptive ? a.d_count.p : nullptr, a.done, a.n_pix, a.plan.W, rp.mode, rp.trim, rp.strength,
                                           d_out, d_var, d_trim, stream));
    return ZR_OK;
}
// zr_robust_params as both robust entries check them, before any device call
int check_robust_params(const zr_robust_params* rp) {
    if (rp->mode != ZR_ROBUST_GINI && rp->mode != ZR_ROBUST_FIXED) return fail(ZR_E_INVALID, "mode = %d is neither ZR_ROBUST_GINI (0) nor ZR_ROBUST_FIXED (1)", rp->mode);
    if (rp->trim < 0 || rp->trim > 31) return fail(ZR_E_INVALID, "trim = %d outside 0..31", rp->trim);
    if (!(rp->strength >= 0) || !std::isfinite(rp->strength)) return fail(ZR_E_INVALID, "strength %g is negative or not finite", rp->strength);
    return ZR_OK;
}
int accum_halves_into(const AccumState& a, double* d_out_a, double* d_out_b, hipStream_t stream) {
    HIP_OK(zr::launch_accum_halves(a.d_partial.p, a.d_pixels.p, a.adaptive ? a.d_count.p : nullptr, a.done, a.n_pix, a.plan.W, d_out_a, d_out_b, stream));
    return ZR_OK;
}

// One render made of several runs (render_batched's batches, an adaptive run's passes) as zr_get_counters sees it: counters and rounds summed, one render's launch times
struct RunTotals {
    zr_ctx* c; bool count; uint64_t id0, rounds = 0; unsigned long long totals[zr::CTR_WORDS] = {0};
    RunTotals(zr_ctx* c, bool count) : c(c), count(count), id0(c->render_id) {}
    int add_run() {   // a run has completed and its stream is idle
        unsigned long long h[zr::CTR_WORDS] = {0};
        if (count) HIP_OK(hipMemcpy(h, c->d_ctr.p, sizeof h, hipMemcpyDeviceToHost));
        for (int w = 0; w < zr::CTR_WORDS; w++) totals[w] += h[w];
        rounds += c->last_rounds;
        return ZR_OK;
    }
    int finish(hipStream_t stream) {   // leaves the stream idle
        for (auto& p : c->pending) if (p.render_id > id0) p.render_id = c->render_id;
        if (count) HIP_OK(hipMemcpyAsync(c->d_ctr.p, totals, sizeof totals, hipMemcpyHostToDevice, stream));
        HIP_OK(hipStreamSynchronize(stream));
        c->last_counted = count; c->last_rounds = rounds;
        return ZR_OK;
    }
};

// What zr_render_accumulate and zr_render_adaptive check after their null tests, in the pinned order (tests/test_accum_validation.py).  n: the fewest samples the
// call adds (the adaptive entry has checked its min_samples); end: one past the last sample it may reach
int accum_call_ready(const zr_ctx* c, const zr_scene* s, const zr_camera* cam, uint64_t seed, const AccumState& st, const char* entry, int n, long long end) {
    if (st.ctx != c) return fail(ZR_E_INVALID, "accumulator belongs to another context");
    if (n < 1) return fail(ZR_E_INVALID, "a batch has at least one sample (%d asked for)", n);
    if (int rc = scene_ready(c, s, entry)) return rc;
    const int W = cam->image_width < 1 ? 1 : cam->image_width, H = cam->image_height < 1 ? 1 : cam->image_height;
    if (W != st.plan.W || H != st.plan.H) return fail(ZR_E_INVALID, "camera of %d x %d px, accumulator of %d x %d", W, H, st.plan.W, st.plan.H);
    const zr_camera key = AccumState::key_of(*cam);
    if (st.bound && (std::memcmp(&key, &st.cam, sizeof key) != 0 || seed != st.seed || s != st.scene || s->epoch != st.scene_epoch))
        return fail(ZR_E_INVALID, "camera, seed or scene differ from the first batch's: zr_accum_reset starts a new frame");
    if (end > 0x7FFFFFFFll) return fail(ZR_E_INVALID, "sample range beyond 2^31");
    if (st.adaptive) return fail(ZR_E_STATE, "the accumulator holds an adaptive run's per-pixel counts: zr_accum_reset starts a new frame");
    return ZR_OK;
}

// what the queries of an accumulator's contents share: something has been rendered; for `what` (the noise estimate, the variance), the same count in every lane
int query_ready(const AccumState& st, const char* entry) {
    return st.done == 0 ? fail(ZR_E_STATE, "zr_render_accumulate or zr_render_adaptive must precede %s", entry) : ZR_OK;
}
int whole_lanes(const AccumState& st, const char* what) {
    return !st.adaptive && st.done % 64 != 0 ? fail(ZR_E_STATE, "the accumulator holds %d samples per pixel, not a multiple of 64: %s is not defined", st.done, what) : ZR_OK;
}
int variance_ready(const AccumState& st, const char* entry) {   // zr_accum_variance, zr_accum_denoise: zr_accum_error's state rules
    int rc = query_ready(st, entry);
    return rc ? rc : whole_lanes(st, "the variance");
}

// What zr_accum_denoise, zr_accum_denoise_nlm and zr_accum_temporal share once their arguments have passed.  whole_frame: `entry` `does` whole frames only;
// device_frames: what the entry works on, made on the context's stream — d_a the mean, or with d_b the two halves, and d_v the variance of the mean (a
// whole-frame plan: the kernels write every pixel of the frames)
int whole_frame(const AccumState& st, const char* entry, const char* does) {
    return st.plan.whole() ? ZR_OK : fail(ZR_E_INVALID, "%s %s whole frames: the accumulator was made with a region", entry, does);
}
int device_frames(const AccumState& st, DevBuf<double>& d_a, DevBuf<double>* d_b, DevBuf<double>& d_v) {
    HIP_OK(hipSetDevice(st.device));
    const size_t n = st.plan.npx() * 3;
    const hipStream_t stream = st.ctx->stream;
    int rc;
    if ((rc = d_a.alloc(n)) || (d_b && (rc = d_b->alloc(n))) || (rc = d_v.alloc(n))) return rc;
    if ((rc = d_b ? accum_halves_into(st, d_a.p, d_b->p, stream) : accum_resolve_into(st, d_a.p, stream))) return rc;
    return accum_variance_into(st, d_v.p, stream);
}

// a frame-shaped query (the mean, the variance): `into` runs on the null stream into a device frame of which only the plan's pixels are written, and only they are copied out
int query_frame(const AccumState& st, int (*into)(const AccumState&, double*, hipStream_t), double* out) {
    HIP_OK(hipSetDevice(st.device));
    DevBuf<double> d_frame;
    int rc = d_frame.alloc(st.plan.npx() * 3);
    if (rc || (rc = into(st, d_frame.p, nullptr))) return rc;
    HIP_OK(hipStreamSynchronize(nullptr));
    std::vector<double> staging;
    return copy_region(st.plan, d_frame.p, out, staging);
}

// per-slot values -> the plan's pixels of a W*H array
template <class T>
void scatter_to_frame(const Plan& plan, const std::vector<T>& per_slot, T* out) {
    const std::vector<uint32_t> pix = plan_pixels(plan);
    for (size_t k = 0; k < pix.size(); k++) out[(size_t)(pix[k] >> 16) * plan.W + (pix[k] & 0xFFFFu)] = per_slot[k];
}

}  // namespace

// A frame whose only misfit is its size — more work units than one run numbers, or no memory for 24 bytes of samples[] per unit — rendered through the pipeline in
// batches of samples with an accumulator of its own.  Same image bit for bit (the lane sums do not know where the batches were cut), counters are the frame's totals.
// Batches are equal, a multiple of 64 samples where possible, at most `n_max` samples; a batch that meets ZR_E_NOMEM is retried at half the size.  ZR_E_NOMEM from here:
// not even small batches fit (or the lane sums themselves do not): the caller falls back to the pixel-group kernel.
int render_batched(zr_ctx* c, const zr_scene* s, const FrameJob& frame, int n_max) {
    const int spp = frame.dc.spp;
    AccumState a;
    a.plan = frame.plan;
    int rc = accum_storage(a, c, &frame.stream);
    if (rc || (rc = accum_zero(a, frame.stream, false))) return rc;
    n_max = std::max(1, std::min(n_max, spp));
    const int n_batches = (spp + n_max - 1) / n_max;
    int n = (spp + n_batches - 1) / n_batches;
    if (n >= 64) n = (n + 63) / 64 * 64 <= n_max ? (n + 63) / 64 * 64 : std::max(n_max / 64 * 64, 1);
    FrameJob job = frame;
    RunTotals runs(c, frame.count);
    bool cancelled = false;
    while (a.done < spp) {
        const int nb = std::min(n, spp - a.done);
        rc = accumulate_batch(c, s, job, a, a.done, nb);
        if (rc == ZR_E_NOMEM && nb > 1) {
            n = nb / 2 >= 64 ? nb / 2 / 64 * 64 : nb / 2;
            std::fprintf(stderr, "[zr] %s: retrying with batches of %d samples\n", zr_host::last_error(), n);
            continue;
        }
        if (rc == ZR_E_CANCELLED) { cancelled = true; break; }
        if (rc || (rc = runs.add_run())) return rc;
        a.done += nb;
        if (a.done < spp) {
            const double f = (double)a.done / spp;
            if (frame.rows_done) { const int r = std::min(frame.plan.H - 1, (int)(f * frame.plan.H)); if (r > *frame.rows_done) *frame.rows_done = r; }
            if (frame.progress) {   // the preview between batches is the exact image of the samples done
                const bool wants = frame.d_out && frame.progress->wants_frame();
                if (wants) { if ((rc = accum_resolve_into(a, frame.d_out, frame.stream))) return rc; HIP_OK(hipStreamSynchronize(frame.stream)); }
                frame.progress->report(f, wants);
            }
            if (frame.keep_going && *frame.keep_going == 0) { cancelled = true; break; }
        }
    }
    if ((a.done > 0 && frame.d_out && (rc = accum_resolve_into(a, frame.d_out, frame.stream))) || (rc = runs.finish(frame.stream))) return rc;
    if (cancelled) return fail(ZR_E_CANCELLED, "render cancelled after %d of %d samples per pixel", a.done, spp);
    return ZR_OK;
}

}  // namespace zr_host

struct zr_accum { AccumState st; };

extern "C" {

zr_accum* zr_accum_create(zr_ctx* c, int width, int height, const zr_region* region) {
    if (!c) { fail(ZR_E_INVALID, "null argument"); return nullptr; }
    if (width < 1 || height < 1) { fail(ZR_E_INVALID, "accumulator size %d x %d not supported", width, height); return nullptr; }
    if (hipSetDevice(c->device) != hipSuccess) { fail(ZR_E_DEVICE, "hipSetDevice(%d) failed", c->device); return nullptr; }
    zr_camera shape{}; shape.image_width = width; shape.image_height = height;
    std::unique_ptr<zr_accum> a(new zr_accum);
    Plan& plan = a->st.plan;
    if (make_plan(shape, region, plan)) return nullptr;
    if (plan.W > zr::ST_MAX_FRAME_SIDE || plan.H > zr::ST_MAX_FRAME_SIDE) { fail(ZR_E_INVALID, "an accumulator's frame may be at most %d pixels a side", zr::ST_MAX_FRAME_SIDE); return nullptr; }
    if (accum_storage(a->st, c, nullptr) || accum_zero(a->st, nullptr, true)) return nullptr;
    return a.release();
}

void zr_accum_destroy(zr_accum* a) {
    if (!a) return;
    (void)hipSetDevice(a->st.device);
    delete a;
}

int zr_accum_reset(zr_accum* a, int first_sample) {
    if (!a) return fail(ZR_E_INVALID, "null argument");
    if (first_sample < 0) return fail(ZR_E_INVALID, "first sample %d below zero", first_sample);
    HIP_OK(hipSetDevice(a->st.device));
    if (int rc = accum_zero(a->st, nullptr, true)) return rc;
    a->st.first = first_sample;
    return ZR_OK;
}

int zr_render_accumulate(zr_ctx* c, const zr_scene* s, const zr_camera* cam, const zr_env* env, uint64_t seed, zr_accum* a, int n_samples,
                         int collect_counters, volatile const uint8_t* keep_going) {
    if (!c || !s || !cam || !env || !a) return fail(ZR_E_INVALID, "null argument");
    AccumState& st = a->st;
    FrameJob job; job.count = collect_counters != 0; job.keep_going = keep_going; job.direct = st.direct;
    int rc = accum_call_ready(c, s, cam, seed, st, "zr_render_accumulate", n_samples, (long long)st.first + st.done + n_samples);
    if (rc || (rc = prepare_frame(c, s, cam, env, seed, nullptr, job, &st.plan)) || (rc = accumulate_batch(c, s, job, st, st.first + st.done, n_samples))) return rc;
    st.done += n_samples;
    st.bind(*cam, seed, s);
    return ZR_OK;
}

int zr_accum_resolve_device(zr_accum* a, void* d_out_rgb, void* hip_stream) {
    if (!a || !d_out_rgb) return fail(ZR_E_INVALID, "null argument");
    if (a->st.done == 0) return fail(ZR_E_STATE, "zr_render_accumulate must precede zr_accum_resolve");
    HIP_OK(hipSetDevice(a->st.device));
    if (int rc = accum_resolve_into(a->st, (double*)d_out_rgb, (hipStream_t)hip_stream)) return rc;
    HIP_OK(hipStreamSynchronize((hipStream_t)hip_stream));
    return ZR_OK;
}

int zr_accum_resolve(zr_accum* a, double* out_rgb) {
    if (!a || !out_rgb) return fail(ZR_E_INVALID, "null argument");
    if (a->st.done == 0) return fail(ZR_E_STATE, "zr_render_accumulate must precede zr_accum_resolve");
    return query_frame(a->st, accum_resolve_into, out_rgb);
}

int zr_accum_variance(zr_accum* a, double* out_var) {
    if (!a || !out_var) return fail(ZR_E_INVALID, "null argument");
    int rc = variance_ready(a->st, "zr_accum_variance");
    return rc ? rc : query_frame(a->st, accum_variance_into, out_var);
}

int zr_accum_halves(zr_accum* a, double* out_a, double* out_b) {
    if (!a || !out_a || !out_b) return fail(ZR_E_INVALID, "null argument");
    const AccumState& st = a->st;
    int rc = variance_ready(st, "zr_accum_halves");
    if (rc) return rc;
    HIP_OK(hipSetDevice(st.device));
    DevBuf<double> d_a, d_b;
    if ((rc = d_a.alloc(st.plan.npx() * 3)) || (rc = d_b.alloc(st.plan.npx() * 3)) || (rc = accum_halves_into(st, d_a.p, d_b.p, nullptr))) return rc;
    HIP_OK(hipStreamSynchronize(nullptr));
    std::vector<double> staging;   // only the plan's pixels are copied out
    return (rc = copy_region(st.plan, d_a.p, out_a, staging)) ? rc : copy_region(st.plan, d_b.p, out_b, staging);
}

// ---- the firefly-robust resolve ---------------------------------------------------------------------------------------------------------------

int zr_accum_resolve_robust(zr_accum* a, const zr_robust_params* rp, double* out_rgb, double* out_variance, int32_t* out_trim) {
    if (!rp) return fail(ZR_E_INVALID, "null argument: params");
    int rc = check_robust_params(rp);   // the parameters first: they need no device and no other argument
    if (rc) return rc;
    if (!a) return fail(ZR_E_INVALID, "null argument: accumulator");
    if (!out_rgb) return fail(ZR_E_INVALID, "null argument: out_rgb");
    const AccumState& st = a->st;
    if ((rc = variance_ready(st, "zr_accum_resolve_robust"))) return rc;
    HIP_OK(hipSetDevice(st.device));
    // device frames of which only the plan's pixels are written, and only they are copied out
    const size_t npx = st.plan.npx();
    DevBuf<double> d_c, d_v; DevBuf<int32_t> d_t;
    if ((rc = d_c.alloc(npx * 3)) || (out_variance && (rc = d_v.alloc(npx * 3))) || (out_trim && (rc = d_t.alloc(npx)))) return rc;
    if ((rc = accum_robust_into(st, *rp, d_c.p, out_variance ? d_v.p : nullptr, out_trim ? d_t.p : nullptr, nullptr))) return rc;
    HIP_OK(hipStreamSynchronize(nullptr));
    std::vector<double> staging;
    if ((rc = copy_region(st.plan, d_c.p, out_rgb, staging)) || (out_variance && (rc = copy_region(st.plan, d_v.p, out_variance, staging)))) return rc;
    if (out_trim && st.n_pix) {
        std::vector<int32_t> h(npx);
        HIP_OK(hipMemcpy(h.data(), d_t.p, npx * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (uint32_t pk : plan_pixels(st.plan)) { const size_t o = (size_t)(pk >> 16) * st.plan.W + (pk & 0xFFFFu); out_trim[o] = h[o]; }
    }
    return ZR_OK;
}

int zr_kat_resolve_robust(zr_ctx* c, const zr_robust_params* rp, const double* lane_sums, const int32_t* counts, size_t n_pix, double* out_rgb,
                          double* out_variance, int32_t* out_trim) {
    if (!rp) return fail(ZR_E_INVALID, "null argument: params");
    int rc = check_robust_params(rp);
    if (rc) return rc;
    if (!c) return fail(ZR_E_INVALID, "null argument: context");
    if (!lane_sums) return fail(ZR_E_INVALID, "null argument: lane_sums");
    if (!counts) return fail(ZR_E_INVALID, "null argument: counts");
    if (!out_rgb) return fail(ZR_E_INVALID, "null argument: out_rgb");
    if (n_pix > 0x7FFFFFFFu) return fail(ZR_E_INVALID, "n_pix = %zu beyond 2^31", n_pix);
    for (size_t k = 0; k < n_pix; k++)
        if (counts[k] < 64 || counts[k] % 64 != 0) return fail(ZR_E_INVALID, "counts[%zu] = %d is not a positive multiple of 64", k, counts[k]);
    if (n_pix == 0) return ZR_OK;
    HIP_OK(hipSetDevice(c->device));
    DevBuf<double> d_s, d_c, d_v; DevBuf<int32_t> d_n, d_t;
    if ((rc = d_s.upload(lane_sums, n_pix * zr::ACCUM_DOUBLES_PER_PIXEL)) || (rc = d_n.upload(counts, n_pix)) || (rc = d_c.alloc(n_pix * 3)) ||
        (out_variance && (rc = d_v.alloc(n_pix * 3))) || (out_trim && (rc = d_t.alloc(n_pix)))) return rc;
    HIP_OK(zr::launch_accum_resolve_robust(d_s.p, nullptr, d_n.p, 0, (uint32_t)n_pix, 0, rp->mode, rp->trim, rp->strength, d_c.p, out_variance ? d_v.p : nullptr,
                                           out_trim ? d_t.p : nullptr, nullptr));
    HIP_OK(hipStreamSynchronize(nullptr));
    HIP_OK(hipMemcpy(out_rgb, d_c.p, n_pix * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_variance) HIP_OK(hipMemcpy(out_variance, d_v.p, n_pix * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_trim) HIP_OK(hipMemcpy(out_trim, d_t.p, n_pix * sizeof(int32_t), hipMemcpyDeviceToHost));
    return ZR_OK;
}

// ---- direct light sampling (the integrator itself: zr_direct.cpp, zr_direct.hip) -----------------------------------------------------------------

int zr_accum_set_direct(zr_accum* a, const zr_direct_params* dp) {
    if (dp) { if (int rc = check_direct_params(dp)) return rc; }   // the parameters first: they need no device and no other argument
    if (!a) return fail(ZR_E_INVALID, "null argument: accumulator");
    if (a->st.done != 0) return fail(ZR_E_STATE, "the accumulator holds %d samples per pixel: zr_accum_set_direct binds an integrator to an empty one (zr_accum_reset)", a->st.done);
    a->st.direct = dp ? (0x80000000u | dp->flags | (a->st.direct & kDirectEnv)) : 0u;   // (unbinding clears zr_accum_set_direct_env's switch, rebinding keeps it)
    return ZR_OK;
}

int zr_accum_set_direct_env(zr_accum* a, int on) {
    if (!a) return fail(ZR_E_INVALID, "null argument: accumulator");
    if (a->st.done != 0) return fail(ZR_E_STATE, "the accumulator holds %d samples per pixel: zr_accum_set_direct_env needs an empty one (zr_accum_reset)", a->st.done);
    if (!a->st.direct) return fail(ZR_E_STATE, "no direct-light integrator is bound to the accumulator: zr_accum_set_direct comes first");
    a->st.direct = on ? (a->st.direct | kDirectEnv) : (a->st.direct & ~kDirectEnv);
    return ZR_OK;
}

int zr_accum_get_direct_env(const zr_accum* a, int* on) {
    if (!a) return fail(ZR_E_INVALID, "null argument: accumulator");
    if (!on) return fail(ZR_E_INVALID, "null argument: on");
    *on = (a->st.direct & kDirectEnv) ? 1 : 0;
    return ZR_OK;
}

int zr_accum_get_direct(const zr_accum* a, zr_direct_params* out) {
    if (!a) return fail(ZR_E_INVALID, "null argument: accumulator");
    if (!out) return fail(ZR_E_INVALID, "null argument: out");
    out->flags = a->st.direct & (ZR_DIRECT_EMITTERS | ZR_DIRECT_SUN); out->pad_ = a->st.direct ? 1u : 0u;   // pad_: 1 while an integrator is bound (flags may be 0)
    return ZR_OK;
}

int zr_accum_state(const zr_accum* a, int64_t out[4]) {
    if (!a || !out) return fail(ZR_E_INVALID, "null argument");
    out[0] = a->st.first; out[1] = a->st.done; out[2] = (int64_t)a->st.n_pix; out[3] = (int64_t)a->st.device_bytes();
    return ZR_OK;
}

// ---- adaptive sampling ----------------------------------------------------------------------------------------------------------------------

int zr_render_adaptive(zr_ctx* c, const zr_scene* s, const zr_camera* cam, const zr_env* env, uint64_t seed, zr_accum* a, const zr_adaptive_params* p,
                       int collect_counters, volatile const uint8_t* keep_going, zr_adaptive_stats* out) {
    if (out) std::memset(out, 0, sizeof *out);   // whatever happens below, `out` holds the statistics of the passes that completed
    if (!p) return fail(ZR_E_INVALID, "null argument");
    // the parameters first: they need no device and no other argument
    const int counts[3] = {p->min_samples, p->max_samples, p->step_samples};
    const char* names[3] = {"min_samples", "max_samples", "step_samples"};
    for (int k = 0; k < 3; k++)
        if (counts[k] < 64 || counts[k] % 64 != 0) return fail(ZR_E_INVALID, "%s = %d is not a positive multiple of 64", names[k], counts[k]);
    if (p->max_samples < p->min_samples) return fail(ZR_E_INVALID, "max_samples %d below min_samples %d", p->max_samples, p->min_samples);
    if (!(p->threshold >= 0) || !std::isfinite(p->threshold)) return fail(ZR_E_INVALID, "threshold %g is negative or not finite", p->threshold);
    if (!(p->dark_floor >= 0) || !std::isfinite(p->dark_floor)) return fail(ZR_E_INVALID, "dark_floor %g is negative or not finite", p->dark_floor);
    if (!c || !s || !cam || !env || !a) return fail(ZR_E_INVALID, "null argument");
    AccumState& st = a->st;
    int rc = accum_call_ready(c, s, cam, seed, st, "zr_render_adaptive", p->min_samples, (long long)st.first + p->max_samples);
    if (rc || (rc = whole_lanes(st, "the noise estimate"))) return rc;
    if (st.done > p->min_samples) return fail(ZR_E_STATE, "the accumulator holds %d samples per pixel, more than min_samples = %d", st.done, p->min_samples);
    FrameJob job; job.count = collect_counters != 0; job.keep_going = keep_going; job.direct = st.direct;
    if ((rc = prepare_frame(c, s, cam, env, seed, nullptr, job, &st.plan))) return rc;
    c->last_rounds = 0;
    HIP_OK(hipMemsetAsync(c->d_ctr.p, 0, zr::CTR_BLOCK * sizeof(unsigned long long), job.stream));
    if (st.n_pix == 0) return ZR_OK;
    // the run's buffers, and the first list: every pixel, in the order the pipeline's own list has (upload_pixel_list: bottom-up shortens the drain)
    const size_t n_blocks = ((size_t)st.n_pix + 255) / 256;
    if ((rc = st.d_count.alloc(st.n_pix)) || (rc = st.d_flag.alloc(st.n_pix)) || (rc = st.d_block_active.alloc(n_blocks)) || (rc = st.d_block_at_max.alloc(n_blocks)) ||
        (rc = st.d_totals.alloc(2))) return rc;
    for (int k = 0; k < 2; k++) if ((rc = st.d_list[k].alloc(st.n_pix)) || (rc = st.d_slot[k].alloc(st.n_pix))) return rc;
    std::vector<uint32_t> pix = plan_pixels(st.plan), slot(pix.size());
    for (size_t k = 0; k < slot.size(); k++) slot[k] = (uint32_t)k;
    if (list_runs_reversed()) { std::reverse(pix.begin(), pix.end()); std::reverse(slot.begin(), slot.end()); }
    HIP_OK(hipMemcpy(st.d_list[0].p, pix.data(), pix.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(st.d_slot[0].p, slot.data(), slot.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_OK(hipDeviceSynchronize());   // the context's streams do not wait for the null stream
    // counts lie in {min + j * step}: the last of them at or below max_samples is where a pixel that is still noisy stops
    const int last_count = p->min_samples + (p->max_samples - p->min_samples) / p->step_samples * p->step_samples;
    zr_adaptive_stats stats{};
    RunTotals runs(c, job.count);
    uint32_t n_active = st.n_pix;
    int cur = 0, count_now = st.done, stop = ZR_OK;
    std::string stop_msg;
    while (n_active > 0) {
        const int target = stats.passes == 0 ? p->min_samples : count_now + p->step_samples;
        const int n = target - count_now;
        if (keep_going && *keep_going == 0) { stop = ZR_E_CANCELLED; stop_msg = "adaptive render cancelled after " + std::to_string(stats.passes) + " passes"; break; }
        HostTimer timer(c);
        if (n > 0) {   // (0: the accumulator came with min_samples already; pass 0 is then the estimate alone)
            job.d_list = st.d_list[cur].p; job.n_list = n_active;
            HIP_OK(hipMemsetAsync(c->d_ctr.p, 0, zr::CTR_BLOCK * sizeof(unsigned long long), job.stream));
            bool flipped = false;
            rc = render_batch_samples(c, s, job, st.d_list[cur].p, n_active, st.first + count_now, n, timer, &flipped);
            if (rc) {   // the pass is discarded whole; the accumulator is as the pass before left it
                stop = rc; stop_msg = zr_host::last_error();
                if (rc == ZR_E_NOMEM) stop_msg += " (adaptive pass " + std::to_string(stats.passes) + ": lower step_samples" + (stats.passes == 0 ? " / min_samples)" : ")");
                break;
            }
        }
        timer.begin(job.stream, 3);
        HIP_OK(zr::launch_adaptive_accumulate(c->d_partial.p, st.d_slot[cur].p, n_active, (uint32_t)n, (uint32_t)(st.first + count_now), st.d_partial.p, st.d_count.p,
                                              st.d_flag.p, target, last_count, p->threshold, p->dark_floor, job.stream));
        HIP_OK(zr::launch_adaptive_compact(st.d_flag.p, n_active, st.d_list[cur].p, st.d_slot[cur].p, st.d_list[cur ^ 1].p, st.d_slot[cur ^ 1].p, st.d_block_active.p,
                                           st.d_block_at_max.p, st.d_totals.p, job.stream));
        timer.end(job.stream, 3);
        if ((rc = timer.status())) return rc;
        uint32_t h_totals[2] = {0, 0};   // the read-back of a pass: how many pixels go on, how many max_samples stopped (a counting run also reads the counter block)
        HIP_OK(hipMemcpyAsync(h_totals, st.d_totals.p, sizeof h_totals, hipMemcpyDeviceToHost, job.stream));
        HIP_OK(hipStreamSynchronize(job.stream));
        if (n > 0) {
            st.route = c->last_path;
            if ((rc = runs.add_run())) return rc;
        }
        st.adaptive = true; st.done = target; count_now = target;
        st.bind(*cam, seed, s);
        stats.passes++; stats.samples += (uint64_t)n_active * (uint64_t)n; stats.stopped_at_max += h_totals[1];
        stats.stopped_by_threshold += n_active - h_totals[0] - h_totals[1];
        n_active = h_totals[0]; cur ^= 1;
        if (out) *out = stats;
    }
    if ((rc = runs.finish(job.stream))) return rc;
    if (stop != ZR_OK) return fail(stop, "%s", stop_msg.c_str());
    return ZR_OK;
}

int zr_accum_error(zr_accum* a, double dark_floor, double* out) {
    if (!a || !out) return fail(ZR_E_INVALID, "null argument");
    if (!(dark_floor >= 0) || !std::isfinite(dark_floor)) return fail(ZR_E_INVALID, "dark_floor %g is negative or not finite", dark_floor);
    AccumState& st = a->st;
    int rc = query_ready(st, "zr_accum_error");
    if (rc || (rc = whole_lanes(st, "the noise estimate"))) return rc;
    HIP_OK(hipSetDevice(st.device));
    DevBuf<double> d_err;
    if ((rc = d_err.alloc(st.n_pix))) return rc;
    HIP_OK(zr::launch_accum_error(st.d_partial.p, st.adaptive ? st.d_count.p : nullptr, st.done, st.n_pix, dark_floor, d_err.p, nullptr));
    HIP_OK(hipStreamSynchronize(nullptr));
    std::vector<double> h(st.n_pix);
    if (st.n_pix) HIP_OK(hipMemcpy(h.data(), d_err.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    scatter_to_frame(st.plan, h, out);
    return ZR_OK;
}

int zr_accum_sample_counts(zr_accum* a, int32_t* out) {
    if (!a || !out) return fail(ZR_E_INVALID, "null argument");
    AccumState& st = a->st;
    int rc = query_ready(st, "zr_accum_sample_counts");
    if (rc) return rc;
    std::vector<int32_t> h(st.n_pix, (int32_t)st.done);
    if (st.adaptive && st.n_pix) {
        HIP_OK(hipSetDevice(st.device));
        HIP_OK(hipMemcpy(h.data(), st.d_count.p, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    scatter_to_frame(st.plan, h, out);
    return ZR_OK;
}

int64_t zr_accum_lane_sums(zr_accum* a, double* out, size_t cap_doubles) {
    if (!a || (!out && cap_doubles != 0)) return fail(ZR_E_INVALID, "null argument");
    AccumState& st = a->st;
    int rc = query_ready(st, "zr_accum_lane_sums");
    if (rc) return rc;
    const size_t n = st.sums();
    if (!out) return (int64_t)n;
    if (cap_doubles < n) return fail(ZR_E_INVALID, "room for %zu doubles, the lane sums are %zu", cap_doubles, n);
    HIP_OK(hipSetDevice(st.device));
    if (n) HIP_OK(hipMemcpy(out, st.d_partial.p, n * sizeof(double), hipMemcpyDeviceToHost));
    return (int64_t)n;
}

// variance-guided denoising of what an accumulator holds (the filter itself: zr_image.cpp)
int zr_accum_denoise(zr_accum* a, const zr_denoise_guided_params* dp, const double* albedo, const double* normal, const double* zdepth, double* out,
                     double* out_variance) {
    if (!a || !dp || !albedo || !normal || !out) return fail(ZR_E_INVALID, "null argument");
    int rc = check_guided_params(dp);
    if (rc) return rc;
    AccumState& st = a->st;
    DevBuf<double> d_c, d_v;
    if ((rc = whole_frame(st, "zr_accum_denoise", "filters")) || (rc = variance_ready(st, "zr_accum_denoise")) || (rc = device_frames(st, d_c, nullptr, d_v))) return rc;
    return denoise_guided_device(st.ctx, dp, d_c, d_v, albedo, normal, zdepth, st.plan.W, st.plan.H, out, out_variance);
}

// non-local-means denoising of what an accumulator holds (the filter itself: zr_image.cpp)
int zr_accum_denoise_nlm(zr_accum* a, const zr_denoise_nlm_params* dp, const double* albedo, const double* normal, double* out, double* out_error) {
    if (!dp) return fail(ZR_E_INVALID, "null argument");
    int rc = check_nlm_params(dp);   // the parameters first: they need no device and no other argument
    if (rc) return rc;
    if (!a || !albedo || !normal || !out) return fail(ZR_E_INVALID, "null argument");
    AccumState& st = a->st;
    DevBuf<double> d_a, d_b, d_v;
    if ((rc = whole_frame(st, "zr_accum_denoise_nlm", "filters")) || (rc = variance_ready(st, "zr_accum_denoise_nlm")) || (rc = device_frames(st, d_a, &d_b, d_v))) return rc;
    return denoise_nlm_device(st.ctx, dp, d_a, d_b, d_v, albedo, normal, st.plan.W, st.plan.H, out, out_error);
}

// what an accumulator holds taken into a history (the reprojection itself: zr_temporal.cpp)
int zr_accum_temporal(zr_accum* a, zr_temporal* t, const zr_temporal_params* p, const zr_scene* s, const zr_camera* cam, uint64_t seed, double* out_color,
                      double* out_variance, int32_t* out_history) {
    if (!p) return fail(ZR_E_INVALID, "null argument");
    int rc = check_temporal_params(p);   // the parameters first: they need no device and no other argument
    if (rc) return rc;
    if (!a || !t || !s || !cam) return fail(ZR_E_INVALID, "null argument");
    AccumState& st = a->st;
    if ((rc = whole_frame(st, "zr_accum_temporal", "takes")) || (rc = temporal_call_ready(t, st.ctx, s, cam, "zr_accum_temporal")) ||
        (rc = variance_ready(st, "zr_accum_temporal"))) return rc;
    int64_t shape[4];
    (void)zr_temporal_state(t, shape);
    if (shape[0] != st.plan.W || shape[1] != st.plan.H) return fail(ZR_E_INVALID, "accumulator of %d x %d px, history of %d x %d", st.plan.W, st.plan.H, (int)shape[0], (int)shape[1]);
    DevBuf<double> d_c, d_v;
    if ((rc = device_frames(st, d_c, nullptr, d_v))) return rc;
    return temporal_accumulate_device(t, p, s, cam, seed, d_c.p, d_v.p, out_color, out_variance, out_history);
}

}  // extern "C"
