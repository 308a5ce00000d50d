// zr_render.cpp — the render side of the C ABI (include/zr_capi.h).  Every render entry point describes its frame once (FrameJob, filled and validated by prepare_frame;
// the region arithmetic lives on Plan: zr_frame.h) and hands it to a driver: enqueue_render (the streaming pipeline where the frame fits it, else the pixel-group kernel),
// render_stream (the pipeline's round loop or the fused small-scene kernel) or the AOV / split-pass / BVH-debug launches.  Also here: counters, known-answer entry points.
#include "zr_frame.h"

namespace zr_host {
namespace {   // this unit's own; what zr_accum.cpp and zr_image.cpp call too follows below

// tiles per launch of the paths that render tile lists (the pixel-group kernel, the BVH debug view): one launch per frame unless the caller polls
// (cancellation, progress), which needs batch boundaries
size_t batch_tiles(bool interactive) { return (size_t)std::max(1, (int)env_double("ZR_BATCH_TILES", interactive ? 256 : (double)(1 << 30))); }

// camera::initialize, camera.hpp:358-399
void make_camera(const zr_camera& c, zr::DCamera& d) {
    int W = c.image_width < 1 ? 1 : c.image_width, H = c.image_height < 1 ? 1 : c.image_height;
    double aspect = double(W) / H;
    H3 center = h3(c.lookfrom), lookat = h3(c.lookat), vup = h3(c.vup);
    double theta = c.vfov * kPi / 180.0;
    double h = std::tan(theta / 2);
    double vh = 2 * h * c.focus_dist;
    double vw = vh * aspect;
    H3 w = unit(center - lookat);
    H3 u = unit(cross(vup, w));
    H3 v = cross(w, u);
    H3 vu = vw * u;
    H3 vv = vh * -v;
    H3 du = vu / W;
    H3 dv = vv / H;
    H3 ul = center - (c.focus_dist * w) - vu / 2 - vv / 2;
    H3 p00 = ul + 0.5 * (du + dv);
    double rad = c.focus_dist * std::tan((c.defocus_angle / 2) * kPi / 180.0);
    st3(d.center, center); st3(d.pixel00, p00); st3(d.du, du); st3(d.dv, dv);
    st3(d.disk_u, u * rad); st3(d.disk_v, v * rad);
    d.W = W; d.H = H; d.spp = c.samples_per_pixel < 1 ? 1 : c.samples_per_pixel; d.max_depth = c.max_depth;
    d.defocus = !(c.defocus_angle <= 0) ? 1 : 0;
    d.pad_ = 0;
}

// ray-independent part of get_background_color, camera.hpp:832-834, 844-858, 874-895, 914-918
void make_env(const zr_env& e, zr::DEnv& d) {
    std::memset(&d, 0, sizeof d);
    d.mode = e.mode; d.hdr_tex = e.hdr_texture; d.intensity = e.intensity;
    H3 bg = h3(e.background_color) * e.intensity;
    st3(d.solid, bg);
    d.cy = std::cos(e.hdri_rotation); d.sy = std::sin(e.hdri_rotation);
    d.cp = std::cos(e.hdri_tilt); d.sp = std::sin(e.hdri_tilt);
    d.cr = std::cos(e.hdri_roll); d.sr = std::sin(e.hdri_roll);
    H3 sun = unit(h3(e.sun_direction));
    double sh = sun.y;
    double ah = sh - 0.05;
    double sky_exposure = clampd(ah * 8.0 + 1.4, 0.0, 1.0);
    double day = clampd(ah * 10.0 + 1.1, 0.0, 1.0);
    double sunset_i = clampd(1.0 - std::fabs(ah + 0.05) * 30.0, 0.0, 1.0);
    double sunset = (ah > -0.1) ? sunset_i : 0.0;
    if (sh < 0) sunset *= (sh * 10.0 + 1.0);
    sunset = clampd(sunset, 0.0, 1.0);
    H3 zen = H3{0.01, 0.03, 0.1} * (1.0 - day) + H3{0.2, 0.5, 1.0} * day;
    H3 hor = H3{0.05, 0.02, 0.01} * (1.0 - day) + H3{0.6, 0.8, 1.0} * day;
    hor = hor * (1.0 - sunset) + H3{1.0, 0.35, 0.1} * sunset;
    st3(d.sun, sun); st3(d.horizon, hor); st3(d.zenith, zen);
    d.sky_scale = e.intensity * 1.5; d.sky_exposure = sky_exposure;
    d.sun_thr = 1.0 - (e.sun_size * 0.001);
    d.sun_on = ah > -0.1 ? 1 : 0;
    H3 scol = h3(e.sun_color) * (1.0 - sunset) + H3{1.0, 0.3, 0.1} * sunset;
    double vis = clampd(sh * 5.0 + 1.0, 0.0, 1.0);
    st3(d.sun_add, (scol * e.sun_intensity) * vis);
}

// tiles [first, first + count) of the uploaded tile list, for one launch of a tile-list kernel
zr::WorkDesc work_desc(const Plan& p, const int32_t* d_tiles, size_t first, size_t count, int lanes) {
    zr::WorkDesc wd;
    wd.tiles = d_tiles + first; wd.n_tiles = (int32_t)count; wd.tile_size = p.ts; wd.tiles_x = p.tiles_x;
    wd.x0 = p.x0; wd.y0 = p.y0; wd.x1 = p.x1; wd.y1 = p.y1;
    wd.lanes_per_pixel = lanes;
    return wd;
}

// a zeroed device frame for an output the caller asked for
int zeroed_frame(DevBuf<double>& d, const double* out, const Plan& p, hipStream_t stream) {
    if (!out) return ZR_OK;
    int rc = d.alloc(p.npx() * 3);
    if (rc) return rc;
    HIP_OK(hipMemsetAsync(d.p, 0, p.npx() * 3 * sizeof(double), stream));
    return ZR_OK;
}

int check_env(const zr::DEnv& de, const zr_scene* s) {
    if (de.mode > ZR_ENV_SOLID_COLOR) return fail(ZR_E_INVALID, "unknown environment mode %u", de.mode);
    if (de.mode == ZR_ENV_HDR_MAP && de.hdr_tex != ZR_NO_TEXTURE && de.hdr_tex >= s->textures.size()) return fail(ZR_E_INVALID, "environment texture id out of range");
    return ZR_OK;
}

// spill slabs of the EXTEND traversal stack, sized for the deepest tree this context has met (never below 36 levels, the
// fixed size of round 1): one slab per resident wave and sub-pool
int ensure_stack_slabs(zr_ctx* c, const zr_scene* s) {
    const uint32_t need = std::max<uint32_t>(36u, zr::stream_overflow_levels(s->stack_demand));
    if (need <= c->st_ovf_levels && c->d_st_overflow.p) return ZR_OK;
    HIP_OK(hipDeviceSynchronize());
    c->d_st_overflow.release();
    int rc = c->d_st_overflow.alloc(ST_MAX_POOLS * zr::stream_overflow_bytes(c->st_blocks, need));
    if (rc) { c->st_ovf_levels = 0; return rc; }
    c->st_ovf_levels = need;
    return ZR_OK;
}

// ---- variant 2: the streaming wavefront pipeline (zr_stream.hip), in the steps of render_stream below -------------------------------------------------

// the plan's pixels as the pipeline's pixel list, uploaded when the plan differs from the cached list's
int upload_pixel_list(zr_ctx* c, const Plan& plan) {
    // Work units are handed out in pixel-list order, and when they run out the frame DRAINS: the paths still alive need up to
    // max_depth more rounds, each with fewer rays than the chip wants (10 rounds = 16 ms of a 415 ms cfg3 frame, 10 of the
    // 60 ms of a rank's 1/8 share).  The drain is as long as the paths started last, so the list runs BOTTOM-UP: the top
    // of a frame is where the sky is, and a sky sample ends in one round.  The image does not depend on the order (every
    // sample is written once and reduced in a fixed order).
    const bool reversed = list_runs_reversed();
    std::vector<int32_t> key = {plan.W, plan.H, plan.ts, plan.x0, plan.y0, plan.x1, plan.y1, (int32_t)plan.tiles.size(),
                                plan.tiles.empty() ? -1 : plan.tiles.front(), plan.tiles.empty() ? -1 : plan.tiles.back(),
                                (int32_t)reversed};
    if (key == c->pix_key && c->d_pixels.p) return ZR_OK;
    std::vector<uint32_t> pix = plan_pixels(plan);
    if (reversed) std::reverse(pix.begin(), pix.end());
    int rc = c->d_pixels.upload(pix);
    if (rc == ZR_OK) c->pix_key = key;
    return rc;
}

// A world of a handful of objects is rendered by the FUSED kernel (zr_stream.hip: fused_render): every object tested per
// segment, the path in registers, no tree, no slot pool.  Testing all objects costs time in proportion to their number, the
// pipeline about the same per segment whatever the scene: the switch-over is ZR_FUSED_MAX objects.  A caller that polls
// (cancellation, lines_rendered, live preview) gets the frame in sixteen launches with the poll between them; the split passes
// stay on the pipeline.
int render_fused(zr_ctx* c, const zr_scene* s, const zr::StreamJob& sj) {
    if (c->fused_blocks == 0) c->fused_blocks = zr::fused_blocks();
    HostTimer timer(c);
    int parts = 1;
    zr::StreamHooks hooks = sj.hooks; hooks.timer = &timer; hooks.done_out = &parts;
    hipError_t fe = zr::fused_render_frame(s->ds, sj.frame, sj.ctx, c->fused_blocks, s->leaf_level <= 1 ? 1 : 2, s->fused, hooks);
    if (fe != hipSuccess) return fail(ZR_E_DEVICE, "fused small-scene kernel failed: %s", hipGetErrorString(fe));
    c->last_rounds = (uint64_t)(parts < 0 ? -parts : parts); c->last_path = 3;
    HIP_OK(hipStreamSynchronize(sj.ctx.streams[0]));
    if (parts < 0) return fail(ZR_E_CANCELLED, "render cancelled after %d of 16 parts", -parts);
    return ZR_OK;
}

// The slot pool of a frame of `units` work units: large enough to fill the chip every round, small enough that the frame takes dozens of rounds (a
// rank that owns 1/8 of the tiles must not degenerate into one shrinking batch).  Grows zr_ctx::d_pool when this frame needs more than it holds.
int size_slot_pool(zr_ctx* c, uint64_t units, uint32_t spp, bool lean_pair, hipStream_t stream, zr::StreamPool& pool) {
    const bool affine = env_double("ZR_STREAM_AFFINE", 0) != 0;   // measured: -18 % L2 requests, -14 % misses, frame time +1 % (profiles/r3_affine_ab.txt): off
    uint32_t P = 0, unit_chunk = 0, drain_slots = 0;
    size_t drain_at = 0;
    for (uint32_t cap = c->st_slots;; cap /= 2) {
        P = cap / 64 * 64;
        // slots = units / 8 where the lean kernels run as two sub-pools (cfg2: 93.2 ms at 8, 98.9 at 4, 115 at 2), units / 3 for one pool of the general builds, whose
        // launches are worth making larger (demo: 128.1 ms at 8, 126.0 at 4, 125.1 at 3: profiles/r4_experiments_ab.txt)
        uint64_t want = std::max<uint64_t>(units / (uint64_t)std::max(1.0, env_double("ZR_STREAM_UNITS_PER_SLOT", lean_pair ? 8 : 3)), 1u << 20);
        want = want / 64 * 64;
        if (want < P) P = (uint32_t)want;
        if (units < P) P = (uint32_t)((units + 63) / 64 * 64);
        // XCD-affine hand-out of the work units (zr_stream.hip: st_unit_of): chunks of `unit_chunk` units — by default the samples of
        // 1024 consecutive pixels of the tile-ordered list, i.e. one 32 x 32 tile — belong to one shard, hence to one XCD's L2
        unit_chunk = 0;
        if (affine) {
            const uint32_t round = 64u * 256u;   // a pool is whole rounds of ST_SHARDS SHADE blocks
            P = std::max<uint32_t>(round, P / round * round);
            if (units < P) P = (uint32_t)((units + round - 1) / round * round);
            uint64_t G = (uint64_t)std::max(1.0, env_double("ZR_STREAM_CHUNK_PX", 1024)) * spp;
            G = std::min<uint64_t>(G, units / (64u * 8u));   // every shard gets at least eight chunks (small frames: smaller chunks)
            unit_chunk = (uint32_t)std::max<uint64_t>(256, std::min<uint64_t>(G, 1u << 30));
        }
        // the slot pool, its sub-pools' rounding, and behind them the small pool the survivors of a frame's drain are moved to
        // (zr_stream.hip: stream_compact).  Sized for the P this frame uses and only ever grown: a 64 x 64 test frame or a one-ray
        // device_hit() does not reserve the 13.7 GB a 1080p frame at 512 spp wants ("Device memory")
        drain_slots = P / 16 / 256 * 256 + 256;
        drain_at = zr::stream_pool_bytes(P) + 65536 * ST_MAX_POOLS;
        const size_t pool_need = drain_at + zr::stream_pool_bytes(drain_slots);
        if (c->d_pool.n >= pool_need) break;
        HIP_OK(hipStreamSynchronize(stream));
        if (c->d_pool.alloc(pool_need) == ZR_OK) break;
        // a pool that cannot be had is retried at half the size: the frame takes more rounds, the image is the same
        if (cap <= (1u << 20)) return fail(ZR_E_NOMEM, "no device memory for a slot pool of %u paths (%zu bytes)", P, pool_need);
        std::fprintf(stderr, "[zr] no device memory for a pool of %u path slots (%zu bytes): retrying with half\n", P, pool_need);
    }
    const bool use_drain = env_double("ZR_STREAM_DRAIN_POOL", 1) != 0;
    pool = zr::StreamPool{c->d_pool.p, P, use_drain ? (void*)(c->d_pool.p + drain_at) : nullptr, drain_slots, unit_chunk};
    return ZR_OK;
}

// the buffers of the reflection / refraction split (mode 1 / 2), grown as the frame needs
int split_buffers(zr_ctx* c, uint64_t units, int mode, hipStream_t stream, zr::StreamSplit& split) {
    int rc;
    if (c->d_kend.n < units * 2) { if ((rc = c->d_kend.alloc(units * 2))) return rc; }
    if (c->d_cls.n < units) { if ((rc = c->d_cls.alloc(units))) return rc; }
    if (mode == 2) HIP_OK(hipMemsetAsync(c->d_cls.p, 0, units, stream));
    const size_t cp = ((size_t)c->st_slots / 256 + ST_MAX_POOLS + 1) * 4;
    if (c->d_cpart.n < cp) { if ((rc = c->d_cpart.alloc(cp))) return rc; }
    split = zr::StreamSplit{mode, c->d_kend.p, c->d_cls.p, c->d_cpart.p};
    return ZR_OK;
}

// The sky pre-pass of a pipeline frame (zr_sky.hip): the listed pixels whose every camera ray provably sees only the environment are written to job.d_out here, the
// others are compacted, in list order, into zr_ctx::d_walk_pixels; *n_walk (host) says how many those are.  The cached list (d_pixels, pix_key) is left alone.
// One 4-byte device-to-host copy and a stream synchronisation.
int sky_prepass(zr_ctx* c, const zr_scene* s, const FrameJob& job, const uint32_t* pixels, uint32_t n_pix, uint32_t* n_walk) {
    int rc;
    const size_t n_blocks = ((size_t)n_pix + 255) / 256;
    if (c->d_sky_flag.n < n_pix && (rc = c->d_sky_flag.alloc(n_pix))) return rc;
    if (c->d_walk_pixels.n < n_pix && (rc = c->d_walk_pixels.alloc(n_pix))) return rc;
    if (c->d_sky_blocks.n < n_blocks && (rc = c->d_sky_blocks.alloc(n_blocks))) return rc;
    if (!c->d_n_walk.p && (rc = c->d_n_walk.alloc(1))) return rc;
    HostTimer timer(c);
    timer.begin(job.stream, 0);
    HIP_OK(zr::launch_sky_prepass(s->ds, job.dc, job.de, job.seed, pixels, n_pix, (uint32_t)job.dc.spp, job.sample0, job.d_out, c->d_sky_flag.p, c->d_sky_blocks.p,
                                  c->d_walk_pixels.p, c->d_n_walk.p, job.stream));
    timer.end(job.stream, 0);
    if ((rc = timer.status())) return rc;
    HIP_OK(hipMemcpyAsync(c->h_active, c->d_n_walk.p, sizeof(uint32_t), hipMemcpyDeviceToHost, job.stream));   // (pinned; the round loop's copies come later)
    HIP_OK(hipStreamSynchronize(job.stream));
    *n_walk = c->h_active[0];
    if (*n_walk > n_pix) return fail(ZR_E_DEVICE, "the sky pre-pass kept %u of %u pixels", *n_walk, n_pix);
    return ZR_OK;
}

// work units one run of the pipeline may have: the packing limit, or less (ZR_STREAM_BATCH_UNITS: a development switch that makes a small frame render in batches)
uint64_t stream_unit_limit() { return (uint64_t)std::min((double)zr::ST_MAX_UNITS, std::max(1.0, env_double("ZR_STREAM_BATCH_UNITS", (double)zr::ST_MAX_UNITS))); }

// ---- the tile-list paths ------------------------------------------------------------------------------------------------------------------------------

// The batch loop of the two interactive tile-list callers (the pixel-group path of enqueue_render, zr_render_bvh_debug): the uploaded tile list in batches of
// batch_tiles(), `launch(first, count)` for each.  A caller that polls gets keep_going looked at before every batch and, after it, the stream synchronised
// (progress / cancellation need the batch to have finished: camera.hpp:441,548-552) and `report_rows(last tile of the batch, is it the last batch)` run.
template <class Launch, class ReportRows>
int run_tile_batches(const FrameJob& job, Launch launch, ReportRows report_rows) {
    const std::vector<int32_t>& tiles = job.plan.tiles;
    const size_t batch = batch_tiles(job.interactive());
    const size_t n_batches = (tiles.size() + batch - 1) / batch;
    for (size_t b = 0; b < n_batches; b++) {
        if (job.keep_going && *job.keep_going == 0) {
            HIP_OK(hipStreamSynchronize(job.stream));
            return fail(ZR_E_CANCELLED, "render cancelled after %zu of %zu batches", b, n_batches);
        }
        const size_t end = std::min(tiles.size(), (b + 1) * batch);
        int rc = launch(b * batch, end - b * batch);
        if (rc) return rc;
        if (job.interactive()) {
            HIP_OK(hipStreamSynchronize(job.stream));
            if (job.rows_done) report_rows(tiles[end - 1], b + 1 == n_batches);
        }
    }
    return ZR_OK;
}

// Renders the job through the streaming pipeline where the frame fits it and the device has the memory, else through the pixel-group kernel.  (Left alone, as they
// change what a frame submits: the tile list is uploaded for every frame although only the pixel-group path reads it; the counter block is cleared here and in render_stream.)
int enqueue_render(zr_ctx* c, const zr_scene* s, const FrameJob& job) {
    const Plan& plan = job.plan;
    c->last_rounds = 0;
    int rc = c->d_tiles.upload(plan.tiles);
    if (rc) return rc;
    HIP_OK(hipMemsetAsync(c->d_ctr.p, 0, zr::CTR_BLOCK * sizeof(unsigned long long), job.stream));
    const uint64_t units = plan.units(job.dc.spp), unit_limit = stream_unit_limit();
    if (fits_stream(c, s, plan, job.dc, 1, 0)) {   // everything but the frame's size fits the pipeline
        const uint64_t n_pix = units / (uint64_t)job.dc.spp;
        int r2 = ZR_E_NOMEM, n_max = job.dc.spp / 2;
        if (units <= unit_limit || job.dc.spp == 1) r2 = render_stream(c, s, job);
        else n_max = (int)std::min<uint64_t>(unit_limit / std::max<uint64_t>(n_pix, 1), (uint64_t)job.dc.spp);
        // too many work units for one run, or no memory for one run's buffers (24 bytes per primary sample + the slot pool) beside what else lives on the
        // device: the same frame in batches of samples (render_batched)
        if (r2 == ZR_E_NOMEM && job.dc.spp > 1) r2 = render_batched(c, s, job, n_max);
        if (job.rows_done && r2 == ZR_OK) *job.rows_done = plan.H;
        if (r2 != ZR_E_NOMEM) return r2;
        // not even in batches: the pixel-group kernel below needs neither buffer
        std::fprintf(stderr, "[zr] %s: rendering this frame with the pixel-group kernel (same results, slower)\n", zr_host::last_error());
        HIP_OK(hipMemsetAsync(c->d_ctr.p, 0, zr::CTR_BLOCK * sizeof(unsigned long long), job.stream));
    } else if (c->variant == 2 && !c->warned_fallback) {   // said once per context: the frame is rendered, by the slower kernel
        c->warned_fallback = true;
        std::fprintf(stderr, "[zr] frame outside the streaming pipeline's packing limits (max_depth %d > %d, %d x %d px > %d, or a scene with more than 2^24 "
                             "primitives of a kind; a frame of more than 2^32 work units is no longer one of them, it renders in sample batches): rendered by the "
                             "pixel-group kernel — same results, several times slower\n",
                     job.dc.max_depth, zr::ST_MAX_BOUNCES, plan.W, plan.H, zr::ST_MAX_FRAME_SIDE);
    }
    c->last_path = 0;
    if (c->pending.size() > 4096) { int rr = resolve_times(c); if (rr) return rr; }
    c->render_id++; c->last_stream = job.stream; c->last_counted = job.count;
    HostTimer timer(c);
    // rows_done after a batch: the rows ABOVE the tile row of the batch's last tile.  (zr_render_bvh_debug counts that tile row in, which is what a batch has
    // finished when it ends a tile row; the two rules differ by one tile row and are both kept as they were.)
    return run_tile_batches(job,
        [&](size_t first, size_t count) -> int {
            timer.begin(job.stream, 1);
            HIP_OK(zr::launch_render(s->ds, job.dc, job.de, job.seed, work_desc(plan, c->d_tiles.p, first, count, lanes_for(job.dc.spp)), job.d_out, c->d_ctr.p, job.count, job.stream));
            timer.end(job.stream, 1);
            return timer.status();
        },
        [&](int last_tile, bool) {
            const int rows = std::min(plan.H, (last_tile / plan.tiles_x) * plan.ts);
            if (rows > *job.rows_done) *job.rows_done = rows;
        });
}

int check_debug_params(const zr_bvh_debug_params* dp) {
    if (!dp) return fail(ZR_E_INVALID, "null argument");
    if (dp->level < -1) return fail(ZR_E_INVALID, "BVH debug level %d below -1", dp->level);
    if (!(dp->thickness > 0.0f) || !std::isfinite(dp->thickness)) return fail(ZR_E_INVALID, "BVH debug thickness must be a positive finite number");
    return ZR_OK;
}

// The end of a frame entry that polls, `rrc` being its driver's answer: a cancelled render still delivers what it rendered (`copy`), then reports the cancellation.
template <class Copy>
int deliver(zr_ctx* c, int rrc, Copy copy, volatile int* rows_done, int H) {
    if (rrc != ZR_OK && rrc != ZR_E_CANCELLED) return rrc;
    std::string cancel_msg = zr_host::last_error();
    HIP_OK(hipStreamSynchronize(c->stream));
    if (int rc = copy()) return rc;
    if (rrc == ZR_E_CANCELLED) return fail(rrc, "%s", cancel_msg.c_str());
    if (rows_done) *rows_done = H;  // camera.hpp:576-578
    return ZR_OK;
}

// The device half of a trace or known-answer entry: `in` uploaded, `launch(d_in, d_out)` on the context's stream, its n_out results back on the host.
template <class In, class Out, class Launch>
int run_on_device(zr_ctx* c, const In* in, size_t n_in, Out* out, size_t n_out, Launch launch) {
    HIP_OK(hipSetDevice(c->device));
    DevBuf<In> d_in; DevBuf<Out> d_out;
    int rc;
    if ((rc = d_in.upload(in, n_in)) || (rc = d_out.alloc(n_out))) return rc;
    HIP_OK(launch(d_in.p, d_out.p));
    HIP_OK(hipStreamSynchronize(c->stream));
    HIP_OK(hipMemcpy(out, d_out.p, n_out * sizeof(Out), hipMemcpyDeviceToHost));
    return ZR_OK;
}

}  // namespace

// lanes of a wave that share a pixel in the tile-list kernels: the largest power of two <= n samples, at most 64
int lanes_for(int n) { int lanes = 64; while (lanes > n) lanes >>= 1; return lanes; }

int make_plan(const zr_camera& cam, const zr_region* region, Plan& p) {
    p.W = cam.image_width < 1 ? 1 : cam.image_width;
    p.H = cam.image_height < 1 ? 1 : cam.image_height;
    p.ts = 32; int mod = 1, rem = 0, skew = 0;
    p.x0 = 0; p.y0 = 0; p.x1 = p.W; p.y1 = p.H;
    if (region) {
        if (region->tile_size > 0) p.ts = region->tile_size;
        if (region->tile_mod > 1) { mod = region->tile_mod; rem = region->tile_rem; skew = region->tile_skew; }
        if (region->w > 0 && region->h > 0) { p.x0 = region->x0; p.y0 = region->y0; p.x1 = region->x0 + region->w; p.y1 = region->y0 + region->h; }
    }
    if (p.x0 < 0 || p.y0 < 0 || p.x1 > p.W || p.y1 > p.H || rem < 0 || rem >= mod || skew < 0 || p.ts > 1024)
        return fail(ZR_E_INVALID, "region outside the %dx%d frame or bad tile parameters", p.W, p.H);
    p.tiles_x = (p.W + p.ts - 1) / p.ts; p.tiles_y = (p.H + p.ts - 1) / p.ts;
    p.tiles.clear();
    for (int ty = p.y0 / p.ts; ty <= (p.y1 - 1) / p.ts; ty++)
        for (int tx = p.x0 / p.ts; tx <= (p.x1 - 1) / p.ts; tx++) {
            int t = ty * p.tiles_x + tx;
            const int part = skew > 0 ? (int)(((long long)tx + (long long)skew * ty) % mod) : t % mod;   // zr_region::tile_skew
            if (part == rem) p.tiles.push_back(t);
        }
    return ZR_OK;
}

// the plan's pixels of the device frame -> the caller's frame, through `scratch`; no other pixel of `out` is touched (null: an output the caller did not ask for)
int copy_region(const Plan& p, const double* d_frame, double* out, std::vector<double>& scratch) {
    if (!out) return ZR_OK;
    scratch.resize(p.npx() * 3);
    HIP_OK(hipMemcpy(scratch.data(), d_frame, scratch.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int32_t t : p.tiles) {
        const TileRect r = p.clip(t);
        for (int y = r.ya; y < r.yb; y++)
            if (r.xb > r.xa) std::memcpy(out + ((size_t)y * p.W + r.xa) * 3, scratch.data() + ((size_t)y * p.W + r.xa) * 3, (size_t)(r.xb - r.xa) * 3 * sizeof(double));
    }
    return ZR_OK;
}

// the scene half of an entry point's argument preamble (the null tests differ per entry and stay there)
int scene_ready(const zr_ctx* c, const zr_scene* s, const char* entry, bool any_context) {
    if (!s->committed) return fail(ZR_E_STATE, "zr_scene_commit must precede %s", entry);
    if (s->stale) return fail(ZR_E_STATE, "scene updated but not refitted: zr_scene_refit must precede %s", entry);
    if (!any_context && s->ctx != c) return fail(ZR_E_INVALID, "scene belongs to another context");
    return ZR_OK;
}

// the shared validation, in the order every entry has had it: region and tile parameters (`plan`: an accumulator's own, in place of the one `region` describes), then the
// environment (`env` is null for the AOV passes, which have none)
int prepare_frame(zr_ctx* c, const zr_scene* s, const zr_camera* cam, const zr_env* env, uint64_t seed, const zr_region* region, FrameJob& job, const Plan* plan) {
    HIP_OK(hipSetDevice(c->device));
    if (plan) job.plan = *plan;
    else if (int rc = make_plan(*cam, region, job.plan)) return rc;
    make_camera(*cam, job.dc);
    if (env) { make_env(*env, job.de); if (int rc = check_env(job.de, s)) return rc; }
    job.seed = seed; job.stream = c->stream;
    return ZR_OK;
}

// Does the frame fit the streaming pipeline's packing (zr_launch.h: ST_MAX_*)?  Otherwise the pixel-group kernels render it: slower, same results.
// depth_factor: paths per sample (the split passes trace two and count both in the bounce byte); units: the caller's count of work units
bool fits_stream(const zr_ctx* c, const zr_scene* s, const Plan& plan, const zr::DCamera& dc, int depth_factor, uint64_t units) {
    return c->variant == 2 && s->quad_ok /* ST_MAX_LEAF_PRIMS */ && depth_factor * dc.max_depth <= zr::ST_MAX_BOUNCES && units <= zr::ST_MAX_UNITS &&
           plan.W <= zr::ST_MAX_FRAME_SIDE && plan.H <= zr::ST_MAX_FRAME_SIDE;
}

int resolve_times(zr_ctx* c) {
    if (c->pending.empty()) return ZR_OK;
    bool fresh = false;
    for (auto& p : c->pending) {
        HIP_OK(hipEventSynchronize(p.b));
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, p.a, p.b));
        if (p.kind == c->log_kind) c->log.push_back(ms);  // default: the dominant kernel's launches (render_* / stream_extend)
        if (p.render_id == c->render_id) {
            if (!fresh) { c->last_render_ms = 0; c->last_extend_ms = 0; c->last_shade_ms = 0; fresh = true; }
            c->last_render_ms += ms;
            if (p.kind == 1) c->last_extend_ms += ms;
            if (p.kind == 2) c->last_shade_ms += ms;
        }
        c->pool.push_back(p.a); c->pool.push_back(p.b);
    }
    c->pending.clear();
    if (c->log.size() > (1u << 20)) c->log.erase(c->log.begin(), c->log.begin() + (c->log.size() - (1u << 20)));
    return ZR_OK;
}

// the plan's pixels in tile order, x | y << 16 (ST_MAX_FRAME_SIDE)
std::vector<uint32_t> plan_pixels(const Plan& plan) {
    std::vector<uint32_t> pix;
    pix.reserve((size_t)plan.tiles.size() * plan.ts * plan.ts);
    for (int32_t t : plan.tiles) {
        const TileRect r = plan.clip(t);
        for (int y = r.ya; y < r.yb; y++) for (int x = r.xa; x < r.xb; x++) pix.push_back((uint32_t)x | ((uint32_t)y << 16));
    }
    return pix;
}

// the one reader of the switch: upload_pixel_list, and in zr_accum.cpp whoever pairs a list position with a pixel (render_batch_samples, an adaptive run's first list)
bool list_runs_reversed() { return env_double("ZR_STREAM_BOTTOM_UP", 1) != 0; }

// Renders job.plan into job.d_out through the pipeline or, for a small world, the fused kernel.  The frame must fit the pipeline (fits_stream: both callers ask
// first).  Synchronises the stream internally (the round loop needs the active-slot count), so zr_render_device returns with the frame complete.
// mode 0: the render; 1 / 2: beauty pass and replay pass of the reflection / refraction split (zr_stream.hip, stream_shade)
int render_stream(zr_ctx* c, const zr_scene* s, const FrameJob& job, int mode) {
    int rc = ZR_OK;
    // the caller's own list leaves the cached one (zr_ctx::d_pixels, pix_key) alone: a later render of the plan gets the plan's list
    if (!job.d_list && (rc = upload_pixel_list(c, job.plan))) return rc;
    const uint32_t* pixels = job.d_list ? job.d_list : c->d_pixels.p;
    uint32_t n_pix = job.d_list ? job.n_list : (uint32_t)c->d_pixels.n;
    const uint32_t spp = (uint32_t)job.dc.spp;
    if (c->pending.size() > 65536) { int rr = resolve_times(c); if (rr) return rr; }
    c->render_id++; c->last_stream = job.stream; c->last_counted = job.count; c->last_rounds = 0; c->last_drain_round = 0; c->last_sub_pools = 0;
    c->last_shade_launches[0] = c->last_shade_launches[1] = 0;
    HIP_OK(hipMemsetAsync(c->d_ctr.p, 0, zr::CTR_BLOCK * sizeof(unsigned long long), job.stream));
    if (n_pix == 0) return ZR_OK;
    uint64_t units = (uint64_t)n_pix * spp;   // one work unit per primary sample
    // per-sample radiance first: without it this pipeline cannot run at all (the caller falls back to the pixel-group kernel)
    size_t samples_n = (size_t)units * 3;
    if (c->d_partial.n < samples_n) {
        HIP_OK(hipStreamSynchronize(job.stream));
        if (c->d_partial.alloc(samples_n) != ZR_OK) return fail(ZR_E_NOMEM, "no device memory for the per-sample radiance buffer (%zu bytes)", samples_n * sizeof(double));
    }
    hipStream_t streams[ST_MAX_POOLS];
    streams[0] = job.stream;
    for (int k = 1; k < ST_MAX_POOLS; k++) streams[k] = c->sub[k];
    const bool fused = mode == 0 && s->fused_ok && s->leaf_level <= 2 && s->leaf_objects > 0 && (double)s->leaf_objects <= env_double("ZR_FUSED_MAX", ZR_FUSED_OBJECTS) &&
                       env_double("ZR_FUSED", 1) != 0;
    // A frame that the pipeline reduces into d_out from the plan's own list first loses its sky pixels (sky_prepass): they never become work units.  Not the counting
    // render (the instrument: every unit goes through the pipeline), not a batch of an accumulator (d_out == nullptr, its own list), not the split passes.
    if (mode == 0 && !fused && job.d_out && !job.d_list && !job.count && s->ds.shade_escape && env_double("ZR_SKY_PREPASS", 1) != 0) {
        uint32_t n_walk = n_pix;
        if ((rc = sky_prepass(c, s, job, pixels, n_pix, &n_walk))) return rc;
        c->presolved = n_pix - n_walk; c->presolved_render = c->render_id;
        if (n_walk < n_pix) { pixels = c->d_walk_pixels.p; n_pix = n_walk; units = (uint64_t)n_pix * spp; samples_n = (size_t)units * 3; }
        if (n_pix == 0) { c->last_path = 2; return ZR_OK; }   // (the stream is idle: sky_prepass synchronised it)
    }
    zr::StreamJob sj{};
    sj.frame = zr::StreamFrame{&job.dc, &job.de, job.seed, spp, n_pix, pixels, c->d_partial.p, job.d_out, job.d_out2, job.count, job.sample0};
    sj.ctx = zr::StreamContext{c->d_ctl.p, nullptr, 0, c->st_blocks, c->d_ctr.p, streams, 1, c->st_event, c->h_active, c->h_polls, c->poll_events};
    sj.hooks = zr::StreamHooks{nullptr, job.keep_going, job.progress, nullptr};
    const bool polled = job.keep_going || job.progress;   // a cancelled frame / a preview reduces what exists: the samples start at zero
    if (fused) {
        if (polled) HIP_OK(hipMemsetAsync(c->d_partial.p, 0, samples_n * sizeof(double), job.stream));
        return render_fused(c, s, sj);
    }
    c->last_path = 2;
    if ((rc = ensure_stack_slabs(c, s))) return rc;
    sj.ctx.overflow = c->d_st_overflow.p; sj.ctx.ovf_levels = c->st_ovf_levels;
    // Two sub-pools, a fraction of a round apart on two streams, let one pool's SHADE run beside the other's EXTEND.  Until round 3 that paid on a rank's share only
    // (the whole frame: 366.6 against 365.7 ms): SHADE needed 124 registers and found no room beside EXTEND's waves.  The lean builds of both kernels use 80
    // (zr_stream.hip), a SIMD holds three waves of each, and a whole cfg3 frame gains 3.5 % with 64 Mi slots, 5.4 % with 128 Mi (profiles/r4_experiments_ab.txt); the
    // general builds (demo: 128 + 117 registers) do not fit beside each other and lose 2 %: one pool for those
    const bool lean_pair = s->leaf_level == 0 && s->ds.shade_lean != 0 && mode == 0;
    if ((rc = size_slot_pool(c, units, spp, lean_pair, job.stream, sj.pool))) return rc;
    if (polled) HIP_OK(hipMemsetAsync(c->d_partial.p, 0, samples_n * sizeof(double), job.stream));
    sj.split.mode = mode;
    if (mode != 0 && (rc = split_buffers(c, units, mode, job.stream, sj.split))) return rc;
    const bool sharded = job.plan.tiles.size() < (size_t)job.plan.tiles_x * job.plan.tiles_y;
    sj.ctx.n_pools = c->st_pools > 0 ? c->st_pools : ((sharded || lean_pair) ? 2 : 1);
    HostTimer timer(c);
    int rounds = 0, drain[2] = {0, 0}, shade_launches[2] = {0, 0};
    sj.hooks.timer = &timer; sj.hooks.done_out = &rounds; sj.hooks.drain_out = drain; sj.hooks.shade_out = shade_launches;
    hipError_t e = zr::stream_render(s->ds, sj, s->leaf_level);
    if (e != hipSuccess) return fail(ZR_E_DEVICE, "streaming pipeline failed: %s", hipGetErrorString(e));
    c->last_rounds = (uint64_t)(rounds < 0 ? -rounds : rounds); c->last_drain_round = drain[0]; c->last_sub_pools = drain[1];
    c->last_shade_launches[0] = shade_launches[0]; c->last_shade_launches[1] = shade_launches[1];
    HIP_OK(hipStreamSynchronize(job.stream));
    if (rounds < 0) return fail(ZR_E_CANCELLED, "render cancelled after %d rounds", -rounds);
    return ZR_OK;
}

void camera_frame(const zr_camera& cam, zr::DCamera& dc) { make_camera(cam, dc); }
int env_frame(const zr_env& env, const zr_scene* s, zr::DEnv& de) { make_env(env, de); return check_env(de, s); }

// world.hit(r, interval(tmin, tmax), rec) for n rays that are on the device already: what zr_trace does once its rays are uploaded, and where the geometry
// buffer's centre rays enter (zr_temporal.cpp).  The context's stream is idle on return.
int trace_device(zr_ctx* c, const zr_scene* s, const double* d_rays, size_t n, double tmin, double tmax, uint64_t seed, uint64_t pixel, uint32_t bounce,
                 zr_hit* d_hits, uint2* d_ki) {
    // Two engines answer the same question: the pair-BVH walk of variants 0/1 and — for the render interval
    // [0.001, inf) — the EXTEND kernel of the streaming pipeline.  ZR_TRACE_ENGINE=pairs|extend picks one (tests run
    // both); by default the engine of the active render variant is used.
    const char* eng = std::getenv("ZR_TRACE_ENGINE");
    const bool can_extend = c->variant == 2 && s->quad_ok && tmin == 0.001 && tmax == HUGE_VAL && n < (1u << 30);
    if (eng && std::strcmp(eng, "extend") == 0 && !can_extend)
        return fail(ZR_E_INVALID, "ZR_TRACE_ENGINE=extend needs ZR_KERNEL=2, tmin = 0.001, tmax = inf and a scene within the 4-wide tree's limits");
    if (can_extend && !(eng && std::strcmp(eng, "pairs") == 0)) {
        DevBuf<unsigned char> pool;
        int rc;
        if ((rc = ensure_stack_slabs(c, s))) return rc;
        if ((rc = pool.alloc(zr::stream_pool_bytes((uint32_t)n) + 65536))) return rc;
        HIP_OK(hipMemsetAsync(c->d_ctr.p, 0, zr::CTR_BLOCK * sizeof(unsigned long long), c->stream));
        const zr::StreamContext ctx{c->d_ctl.p, c->d_st_overflow.p, c->st_ovf_levels, c->st_blocks, c->d_ctr.p, &c->stream, 1, c->st_event, c->h_active};
        HIP_OK(zr::stream_trace(s->ds, d_rays, (uint32_t)n, seed, pixel, bounce, d_hits, d_ki, pool.p, ctx, s->leaf_level));
        HIP_OK(hipStreamSynchronize(c->stream));
        unsigned int capped = 0;
        HIP_OK(hipMemcpy(&capped, c->d_ctl.p + zr::CTL_CAPPED, sizeof capped, hipMemcpyDeviceToHost));
        if (capped) return fail(ZR_E_DEVICE, "EXTEND hit its iteration cap on %u wave(s)", capped);
    } else {
        HIP_OK(zr::launch_trace(s->ds, d_rays, n, tmin, tmax, seed, pixel, bounce, d_hits, d_ki, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
    }
    return ZR_OK;
}

}  // namespace zr_host

extern "C" {

int zr_render_device(zr_ctx* c, const zr_scene* s, const zr_camera* cam, const zr_env* env, uint64_t seed, const zr_region* region,
                     int collect_counters, void* d_out_rgb, void* hip_stream) {
    if (!c || !s || !cam || !env || !d_out_rgb) return fail(ZR_E_INVALID, "null argument");
    int rc = scene_ready(c, s, "zr_render");
    if (rc) return rc;
    FrameJob job;
    if ((rc = prepare_frame(c, s, cam, env, seed, region, job))) return rc;
    // default stream requested: use the legacy null stream so that callers' stream-ordered work (torch) sees it
    job.stream = (hipStream_t)hip_stream;
    job.count = collect_counters != 0; job.d_out = (double*)d_out_rgb;
    return enqueue_render(c, s, job);
}

int zr_render(zr_ctx* c, const zr_scene* s, const zr_camera* cam, const zr_env* env, uint64_t seed, const zr_region* region,
              int collect_counters, double* out_rgb, volatile const uint8_t* keep_going, volatile int* rows_done) {
    if (!c || !s || !cam || !env || !out_rgb) return fail(ZR_E_INVALID, "null argument");
    int rc = scene_ready(c, s, "zr_render");
    if (rc) return rc;
    FrameJob job;
    if ((rc = prepare_frame(c, s, cam, env, seed, region, job))) return rc;
    const Plan& plan = job.plan;
    if ((rc = c->d_out.alloc(plan.npx() * 3))) return rc;
    HIP_OK(hipMemsetAsync(c->d_out.p, 0, plan.npx() * 3 * sizeof(double), c->stream));
    if (rows_done) *rows_done = 0;
    // a whole frame goes straight into the caller's buffer; a region through a staging copy (only its pixels may be touched)
    std::vector<double> staging;
    auto copy_out = [&]() -> int {
        if (!plan.whole()) return copy_region(plan, c->d_out.p, out_rgb, staging);
        HIP_OK(hipMemcpy(out_rgb, c->d_out.p, plan.npx() * 3 * sizeof(double), hipMemcpyDeviceToHost));
        return ZR_OK;
    };
    // Progress as the reference's callers see it: lines_rendered advances while the frame renders (camera.hpp:548-552) and the
    // GUI reads render_accumulator mid-render (main.cpp:1576).  The pipeline finishes samples all over the frame rather than
    // row by row, so `rows_done` = H x the finished fraction of the samples (H only at the very end), and a few times per second
    // out_rgb receives the mean of the samples finished so far (every pixel brightens towards its final value).
    struct Preview : zr::StreamProgress {
        volatile int* rows; int H; double last = 0; std::function<int()> copy; double period;
        static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
        bool wants_frame() override { return now() - last >= period; }
        void report(double f, bool reduced) override {
            const int r = std::min(H - 1, std::max(0, (int)(f * H)));
            if (r > *rows) *rows = r;
            if (reduced) { (void)copy(); last = now(); }
        }
    } preview;
    preview.rows = rows_done; preview.H = plan.H; preview.copy = copy_out; preview.period = env_double("ZR_PREVIEW_PERIOD_S", 0.2); preview.last = Preview::now();
    job.count = collect_counters != 0; job.d_out = c->d_out.p;
    job.keep_going = keep_going; job.rows_done = rows_done; job.progress = rows_done ? &preview : nullptr;
    return deliver(c, enqueue_render(c, s, job), copy_out, rows_done, plan.H);
}

int zr_render_aov(zr_ctx* c, const zr_scene* s, const zr_camera* cam, uint64_t seed, const zr_region* region, const zr_aov_params* ap,
                  double* out_albedo, double* out_normal, double* out_zdepth) {
    if (!c || !s || !cam || !ap) return fail(ZR_E_INVALID, "null argument");
    int rc = scene_ready(c, s, "zr_render_aov");
    if (rc) return rc;
    if (!out_albedo && !out_normal && !out_zdepth) return ZR_OK;
    FrameJob job;
    if ((rc = prepare_frame(c, s, cam, nullptr, seed, region, job))) return rc;
    // camera basis u, v, w exactly as camera::initialize builds it (camera.hpp:380-382)
    H3 w = unit(h3(cam->lookfrom) - h3(cam->lookat));
    H3 u = unit(cross(h3(cam->vup), w));
    H3 v = cross(w, u);
    double uvw[9] = {u.x, u.y, u.z, v.x, v.y, v.z, w.x, w.y, w.z};
    const int spp = job.dc.spp;
    const int aux_sample = std::min(std::max(spp / 8, 64), 1024);   // std::clamp(spp / 8, 64, 1024), camera.hpp:433
    const int aux = std::min(aux_sample, spp);                      // camera.hpp:535
    const Plan& plan = job.plan;
    DevBuf<double> d_a, d_n, d_z;
    if ((rc = zeroed_frame(d_a, out_albedo, plan, c->stream)) || (rc = zeroed_frame(d_n, out_normal, plan, c->stream)) || (rc = zeroed_frame(d_z, out_zdepth, plan, c->stream))) return rc;
    if ((rc = c->d_tiles.upload(plan.tiles))) return rc;
    const zr::WorkDesc wd = work_desc(plan, c->d_tiles.p, 0, plan.tiles.size(), lanes_for(aux));
    HIP_OK(zr::launch_aov(s->ds, job.dc, seed, wd, aux, ap->z_depth_max_dist, uvw, d_a.p, d_n.p, d_z.p, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    std::vector<double> staging;
    if ((rc = copy_region(plan, d_a.p, out_albedo, staging)) || (rc = copy_region(plan, d_n.p, out_normal, staging)) || (rc = copy_region(plan, d_z.p, out_zdepth, staging))) return rc;
    return ZR_OK;
}

int zr_render_passes(zr_ctx* c, const zr_scene* s, const zr_camera* cam, const zr_env* env, uint64_t seed, const zr_region* region,
                     double* out_beauty, double* out_reflection, double* out_refraction) {
    if (!c || !s || !cam || !env) return fail(ZR_E_INVALID, "null argument");
    int rc = scene_ready(c, s, "zr_render_passes");
    if (rc) return rc;
    if (!out_beauty && !out_reflection && !out_refraction) return ZR_OK;
    FrameJob job;
    if ((rc = prepare_frame(c, s, cam, env, seed, region, job))) return rc;
    const Plan& plan = job.plan;
    DevBuf<double> d_b, d_r, d_f;
    if ((rc = zeroed_frame(d_b, out_beauty, plan, c->stream)) || (rc = zeroed_frame(d_r, out_reflection, plan, c->stream)) || (rc = zeroed_frame(d_f, out_refraction, plan, c->stream))) return rc;
    if ((rc = c->d_tiles.upload(plan.tiles))) return rc;
    // Historical, kept: this entry counts whole tiles, not the clipped region as zr_render does (Plan::units).  The counts differ by less than a tile's width
    // of pixels per edge, so they only pick different paths for a frame that close to 2^32 units — and both paths render the same frame.
    const uint64_t tile_units = (uint64_t)plan.tiles.size() * plan.ts * plan.ts * (uint64_t)job.dc.spp;
    if (fits_stream(c, s, plan, job.dc, 2, tile_units) && env_double("ZR_PASSES_STREAM", 1) != 0) {
        // two runs of the streaming pipeline: the beauty pass records where every sample's stream stopped, the replay pass traces
        // the camera ray again and runs the second path from there (stream_shade MODE 1 / 2)
        unsigned long long ha[zr::CTR_WORDS], hb[zr::CTR_WORDS];
        job.d_out = d_b.p;
        if ((rc = render_stream(c, s, job, 1))) return rc;
        HIP_OK(hipMemcpy(ha, c->d_ctr.p, sizeof ha, hipMemcpyDeviceToHost));
        job.d_out = d_r.p; job.d_out2 = d_f.p;
        if ((rc = render_stream(c, s, job, 2))) return rc;
        c->last_path = 2;
        HIP_OK(hipMemcpy(hb, c->d_ctr.p, sizeof hb, hipMemcpyDeviceToHost));
        // counted by SHADE in both passes (EXTEND runs uninstrumented): samples, segments, hits, draws
        unsigned long long h[zr::CTR_WORDS] = {0};
        h[zr::CTR_SAMPLES] = (unsigned long long)c->d_pixels.n * (unsigned long long)job.dc.spp;   // every sample of the region, once
        for (int w : {zr::CTR_SEGMENTS, zr::CTR_HITS, zr::CTR_DRAWS}) h[w] = ha[w] + hb[w];
        HIP_OK(hipMemcpy(c->d_ctr.p, h, sizeof h, hipMemcpyHostToDevice));
        c->last_counted = true;
    } else {
        c->render_id++; c->last_counted = true; c->last_rounds = 0; c->last_path = 0;
        HIP_OK(hipMemsetAsync(c->d_ctr.p, 0, zr::CTR_BLOCK * sizeof(unsigned long long), c->stream));
        const zr::WorkDesc wd = work_desc(plan, c->d_tiles.p, 0, plan.tiles.size(), lanes_for(job.dc.spp));
        HIP_OK(zr::launch_passes(s->ds, job.dc, job.de, seed, wd, d_b.p, d_r.p, d_f.p, c->d_ctr.p, c->stream));
    }
    HIP_OK(hipStreamSynchronize(c->stream));
    std::vector<double> staging;
    if ((rc = copy_region(plan, d_b.p, out_beauty, staging)) || (rc = copy_region(plan, d_r.p, out_reflection, staging)) || (rc = copy_region(plan, d_f.p, out_refraction, staging))) return rc;
    return ZR_OK;
}

int zr_render_bvh_debug(zr_ctx* c, const zr_scene* s, const zr_camera* cam, const zr_env* env, uint64_t seed, const zr_region* region,
                        const zr_bvh_debug_params* dp, double* out_rgb, volatile const uint8_t* keep_going, volatile int* rows_done) {
    if (!c || !s || !cam || !env || !out_rgb) return fail(ZR_E_INVALID, "null argument");
    int rc = check_debug_params(dp);
    if (rc || (rc = scene_ready(c, s, "zr_render_bvh_debug"))) return rc;
    FrameJob job;
    if ((rc = prepare_frame(c, s, cam, env, seed, region, job))) return rc;
    const Plan& plan = job.plan;
    if ((rc = c->d_out.alloc(plan.npx() * 3))) return rc;
    HIP_OK(hipMemsetAsync(c->d_out.p, 0, plan.npx() * 3 * sizeof(double), c->stream));
    if (rows_done) *rows_done = 0;
    if ((rc = c->d_tiles.upload(plan.tiles))) return rc;
    job.d_out = c->d_out.p; job.keep_going = keep_going; job.rows_done = rows_done;
    // rows_done after a batch: the rows down to the lower edge of the tile row of the batch's last tile, the whole frame after the last batch.  (The pixel-group
    // path of enqueue_render reports one tile row less, the rows above that tile row; both rules are kept as they were.)
    int rrc = run_tile_batches(job,
        [&](size_t first, size_t count) -> int {
            HIP_OK(zr::launch_bvh_debug(s->ds, job.dc, job.de, seed, work_desc(plan, c->d_tiles.p, first, count, 1), dp->level, dp->thickness, c->d_out.p, c->stream));
            return ZR_OK;
        },
        [&](int last_tile, bool last_batch) {
            const int rows = std::min(plan.H, (last_tile / plan.tiles_x + 1) * plan.ts);
            if (rows > *rows_done) *rows_done = last_batch ? plan.H : rows;
        });
    std::vector<double> staging;
    return deliver(c, rrc, [&]() { return copy_region(plan, c->d_out.p, out_rgb, staging); }, rows_done, plan.H);
}

int zr_trace_bvh_debug(zr_ctx* c, const zr_scene* s, const zr_bvh_debug_params* dp, const double* rays6, size_t n, double tmin, uint64_t seed,
                       uint64_t pixel, uint32_t bounce, zr_bvh_debug_hit* out) {
    if (!c || !s || (n && (!rays6 || !out))) return fail(ZR_E_INVALID, "null argument");
    int rc = check_debug_params(dp);
    if (rc || (rc = scene_ready(c, s, "zr_trace_bvh_debug"))) return rc;
    if (n == 0) return ZR_OK;
    return run_on_device(c, rays6, n * 6, out, n, [&](const double* d_rays, zr_bvh_debug_hit* d_out) {
        return zr::launch_trace_bvh_debug(s->ds, d_rays, n, tmin, seed, pixel, bounce, dp->level, dp->thickness, d_out, c->stream); });
}

int zr_trace_paths(zr_ctx* c, const zr_scene* s, const zr_camera* cam, uint64_t seed, const int32_t* requests, int n, int max_segments, double* out) {
    if (!c || !s || !cam || (n > 0 && (!requests || !out))) return fail(ZR_E_INVALID, "null argument");
    if (int rc0 = scene_ready(c, s, "zr_trace_paths", true)) return rc0;   // a scene of any context is accepted here, unlike everywhere else: kept as it has always been
    if (n <= 0 || max_segments <= 0) return ZR_OK;
    static_assert(ZR_PATH_RECORD == ZR_PATH_REC, "record size");
    zr::DCamera dc; make_camera(*cam, dc);
    for (int k = 0; k < n; k++)
        if (requests[3 * k] < 0 || requests[3 * k] >= dc.W || requests[3 * k + 1] < 0 || requests[3 * k + 1] >= dc.H || requests[3 * k + 2] < 0)
            return fail(ZR_E_INVALID, "path request %d outside the frame", k);
    return run_on_device(c, requests, (size_t)n * 3, out, (size_t)n * max_segments * ZR_PATH_RECORD, [&](const int32_t* d_req, double* d_out) {
        return zr::launch_path_records(s->ds, dc, seed, d_req, n, max_segments, d_out, c->stream); });
}

int zr_get_counters(zr_ctx* c, zr_counters* out) {
    if (!c || !out) return fail(ZR_E_INVALID, "null argument");
    HIP_OK(hipSetDevice(c->device));
    int rc = resolve_times(c);
    if (rc) return rc;
    std::memset(out, 0, sizeof *out);
    out->kernel_ms = c->last_render_ms;
    out->extend_ms = c->last_extend_ms; out->shade_ms = c->last_shade_ms; out->rounds = c->last_rounds; out->path = (uint64_t)c->last_path;
    unsigned long long h[zr::CTR_WORDS];
    HIP_OK(hipMemcpy(h, c->d_ctr.p, sizeof h, hipMemcpyDeviceToHost));
    if (c->last_counted || env_double("ZR_RAW_COUNTERS", 0) != 0) {
        out->primary_samples = h[zr::CTR_SAMPLES]; out->segments = h[zr::CTR_SEGMENTS]; out->nodes_tested = h[zr::CTR_NODES]; out->spheres_tested = h[zr::CTR_SPHERES];
        out->triangles_tested = h[zr::CTR_TRIANGLES]; out->cubes_tested = h[zr::CTR_CUBES]; out->media_tested = h[zr::CTR_MEDIA]; out->hits = h[zr::CTR_HITS];
        out->rng_draws = h[zr::CTR_DRAWS]; out->escaped = h[zr::CTR_ESCAPED];
        out->node_execs = h[zr::CTR_NODE_EXECS]; out->node_lanes = h[zr::CTR_NODE_LANES]; out->leaf_execs = h[zr::CTR_LEAF_EXECS]; out->leaf_lanes = h[zr::CTR_LEAF_LANES];
        out->shade_execs = h[zr::CTR_SHADE_EXECS]; out->shade_lanes = h[zr::CTR_SHADE_LANES];   // shade_lanes: the counting lean SHADE's slots; otherwise a ZR_WAVE_PROFILE build's (zr_launch.h)
    }
    if (std::getenv("ZR_LANE_HISTOGRAM")) {   // development aid (a -DZR_WAVE_PROFILE build fills them): EXTEND's iterations per phase by ready lanes, 8 buckets of 8 lanes
        unsigned long long hh[zr::CTR_HIST_WORDS];
        HIP_OK(hipMemcpy(hh, c->d_ctr.p + zr::CTR_HIST, sizeof hh, hipMemcpyDeviceToHost));
        const char* names[3] = {"NODE", "LEAF", "FETCH"};
        for (int ph = 0; ph < 3; ph++) {
            unsigned long long tot = 0;
            for (int b = 0; b < 8; b++) tot += hh[ph * 8 + b];
            std::fprintf(stderr, "[zr] %-5s iterations by ready lanes (1-8 ... 57-64):", names[ph]);
            for (int b = 0; b < 8; b++) std::fprintf(stderr, " %5.1f%%", tot ? 100.0 * (double)hh[ph * 8 + b] / (double)tot : 0.0);
            std::fprintf(stderr, "   of %llu\n", tot);
        }
    }
    return ZR_OK;
}

int zr_last_round_loop(zr_ctx* c, int* drain_round, int* sub_pools) {
    if (!c) return fail(ZR_E_INVALID, "null argument");
    if (drain_round) *drain_round = c->last_drain_round;
    if (sub_pools) *sub_pools = c->last_sub_pools;
    return ZR_OK;
}

int zr_last_shade_builds(zr_ctx* c, int* in_place, int* sorted) {
    if (!c) return fail(ZR_E_INVALID, "null argument");
    if (in_place) *in_place = c->last_shade_launches[0];
    if (sorted) *sorted = c->last_shade_launches[1];
    return ZR_OK;
}

int zr_last_extend_fetches(zr_ctx* c, uint64_t* checked, uint64_t* skipped) {
    if (!c) return fail(ZR_E_INVALID, "null argument");
    HIP_OK(hipSetDevice(c->device));
    unsigned long long h[2] = {0, 0};
    static_assert(zr::CTR_FETCH_SKIPPED == zr::CTR_FETCH_CHECKED + 1, "read as a pair");
    if (c->last_counted) {
        HIP_OK(hipStreamSynchronize(c->stream));
        HIP_OK(hipMemcpy(h, c->d_ctr.p + zr::CTR_FETCH_CHECKED, sizeof h, hipMemcpyDeviceToHost));
    }
    if (checked) *checked = h[0];
    if (skipped) *skipped = h[1];
    return ZR_OK;
}

uint64_t zr_last_presolved_pixels(zr_ctx* c) {
    return c && c->presolved_render == c->render_id ? c->presolved : 0;
}

int zr_get_kernel_times(zr_ctx* c, float* ms, int cap) {
    if (!c) return fail(ZR_E_INVALID, "null argument");
    HIP_OK(hipSetDevice(c->device));
    int rc = resolve_times(c);
    if (rc) return rc;
    int total = (int)c->log.size();
    int n = std::min(total, std::max(cap, 0));
    for (int k = 0; k < n; k++) ms[k] = c->log[c->log.size() - n + k];
    c->log.clear();
    return total;
}

int zr_trace(zr_ctx* c, const zr_scene* s, const double* rays6, size_t n, double tmin, double tmax, uint64_t seed, uint64_t pixel,
             uint32_t bounce, zr_hit* out) {
    if (!c || !s || (n && (!rays6 || !out))) return fail(ZR_E_INVALID, "null argument");
    if (int rc0 = scene_ready(c, s, "zr_trace", true)) return rc0;   // a scene of any context is accepted here, unlike everywhere else: kept as it has always been
    HIP_OK(hipSetDevice(c->device));
    DevBuf<double> d_rays; DevBuf<zr_hit> d_hits;
    std::vector<double> r(rays6, rays6 + n * 6);
    int rc;
    if ((rc = d_rays.upload(r))) return rc;
    if ((rc = d_hits.alloc(n))) return rc;
    if ((rc = trace_device(c, s, d_rays.p, n, tmin, tmax, seed, pixel, bounce, d_hits.p))) return rc;
    if (n) HIP_OK(hipMemcpy(out, d_hits.p, n * sizeof(zr_hit), hipMemcpyDeviceToHost));
    return ZR_OK;
}

int zr_kat_scatter(zr_ctx* c, const zr_scene* s, const double* rays6, const zr_hit* recs, const uint64_t* keys, const uint64_t* first_draw,
                   size_t n, zr_scatter_out* out) {
    if (!c || !s || (n && (!rays6 || !recs || !keys || !out))) return fail(ZR_E_INVALID, "null argument");
    if (int rc0 = scene_ready(c, s, "zr_kat_scatter")) return rc0;
    if (n == 0) return ZR_OK;
    HIP_OK(hipSetDevice(c->device));
    DevBuf<double> d_rays; DevBuf<zr_hit> d_recs; DevBuf<uint64_t> d_keys, d_first; DevBuf<zr_scatter_out> d_out;
    int rc;
    if ((rc = d_rays.upload(std::vector<double>(rays6, rays6 + n * 6))) || (rc = d_recs.upload(std::vector<zr_hit>(recs, recs + n))) ||
        (rc = d_keys.upload(std::vector<uint64_t>(keys, keys + n))) || (rc = d_out.alloc(n))) return rc;
    if (first_draw && (rc = d_first.upload(std::vector<uint64_t>(first_draw, first_draw + n)))) return rc;
    HIP_OK(zr::launch_kat_scatter(s->ds, d_rays.p, d_recs.p, d_keys.p, first_draw ? d_first.p : nullptr, n, d_out.p, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    HIP_OK(hipMemcpy(out, d_out.p, n * sizeof(zr_scatter_out), hipMemcpyDeviceToHost));
    return ZR_OK;
}

int zr_kat_shade_lean(zr_ctx* c, const zr_scene* s, const double* rays6, const uint64_t* keys, const uint64_t* first_draw, size_t n, zr_hit* out_hits,
                      zr_scatter_out* out) {
    if (!c || !s || (n && (!rays6 || !keys || !out_hits || !out))) return fail(ZR_E_INVALID, "null argument");
    if (int rc0 = scene_ready(c, s, "zr_kat_shade_lean")) return rc0;
    if (!s->ds.shade_lean) return fail(ZR_E_STATE, "zr_kat_shade_lean: the scene did not commit with SHADE's lean build (kernels: shade_lean = 0)");
    if (n == 0) return ZR_OK;
    HIP_OK(hipSetDevice(c->device));
    DevBuf<double> d_rays; DevBuf<uint64_t> d_keys, d_first; DevBuf<zr_hit> d_hits; DevBuf<zr_scatter_out> d_out;
    int rc;
    if ((rc = d_rays.upload(std::vector<double>(rays6, rays6 + n * 6))) || (rc = d_keys.upload(std::vector<uint64_t>(keys, keys + n))) ||
        (rc = d_hits.alloc(n)) || (rc = d_out.alloc(n))) return rc;
    if (first_draw && (rc = d_first.upload(std::vector<uint64_t>(first_draw, first_draw + n)))) return rc;
    HIP_OK(zr::launch_kat_shade_lean(s->ds, d_rays.p, d_keys.p, first_draw ? d_first.p : nullptr, n, d_hits.p, d_out.p, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    HIP_OK(hipMemcpy(out_hits, d_hits.p, n * sizeof(zr_hit), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out, d_out.p, n * sizeof(zr_scatter_out), hipMemcpyDeviceToHost));
    return ZR_OK;
}

int zr_kat_texture(zr_ctx* c, const zr_scene* s, uint32_t texture_id, const double* uvp5, size_t n, double* out_rgb) {
    if (!c || !s || (n && (!uvp5 || !out_rgb))) return fail(ZR_E_INVALID, "null argument");
    if (int rc0 = scene_ready(c, s, "zr_kat_texture")) return rc0;
    if (texture_id >= s->textures.size()) return fail(ZR_E_INVALID, "texture id %u out of range", texture_id);
    if (n == 0) return ZR_OK;
    return run_on_device(c, uvp5, n * 5, out_rgb, n * 3, [&](const double* d_in, double* d_out) { return zr::launch_kat_texture(s->ds, texture_id, d_in, n, d_out, c->stream); });
}

int zr_kat_background(zr_ctx* c, const zr_scene* s, const zr_env* env, const double* dirs3, size_t n, double* out_rgb) {
    if (!c || !s || !env || (n && (!dirs3 || !out_rgb))) return fail(ZR_E_INVALID, "null argument");
    if (int rc0 = scene_ready(c, s, "zr_kat_background")) return rc0;
    zr::DEnv de; make_env(*env, de);
    if (int rc0 = check_env(de, s)) return rc0;
    if (n == 0) return ZR_OK;
    return run_on_device(c, dirs3, n * 3, out_rgb, n * 3, [&](const double* d_in, double* d_out) { return zr::launch_kat_background(s->ds, de, d_in, n, d_out, c->stream); });
}

int zr_kat_camera_rays(zr_ctx* c, const zr_camera* cam, uint64_t seed, const int32_t* requests3, size_t n, double* out7) {
    if (!c || !cam || (n && (!requests3 || !out7))) return fail(ZR_E_INVALID, "null argument");
    if (n == 0) return ZR_OK;
    zr::DCamera dc; make_camera(*cam, dc);
    for (size_t k = 0; k < n; k++)
        if (requests3[3 * k] < 0 || requests3[3 * k] >= dc.W || requests3[3 * k + 1] < 0 || requests3[3 * k + 1] >= dc.H || requests3[3 * k + 2] < 0)
            return fail(ZR_E_INVALID, "camera-ray request %zu outside the frame", k);
    return run_on_device(c, requests3, n * 3, out7, n * 7, [&](const int32_t* d_req, double* d_out) { return zr::launch_kat_camera_rays(dc, seed, d_req, n, d_out, c->stream); });
}

}  // extern "C"
