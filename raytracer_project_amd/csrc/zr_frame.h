// zr_frame.h — what zr_render.cpp, zr_accum.cpp and zr_image.cpp share: Plan, FrameJob, HostTimer, and the functions one of them calls in another (declarations only)
#pragma once
#include "zr_host_internal.h"

namespace zr_host {

struct TileRect { int xa, xb, ya, yb; };   // the pixels [xa, xb) x [ya, yb); xb <= xa or yb <= ya: none
// which pixels a call renders: the frame, its tile grid, the region rectangle and the tiles of this part (zr_region)
struct Plan {
    int W, H, ts, tiles_x, tiles_y, x0, y0, x1, y1;
    std::vector<int32_t> tiles;
    size_t npx() const { return (size_t)W * H; }
    bool whole() const { return tiles.size() == (size_t)tiles_x * tiles_y && x0 == 0 && y0 == 0 && x1 == W && y1 == H; }
    // tile t's pixels that lie in the region
    TileRect clip(int32_t t) const {
        const int tx = (t % tiles_x) * ts, ty = (t / tiles_x) * ts;
        return {std::max(tx, x0), std::min(tx + ts, x1), std::max(ty, y0), std::min(ty + ts, y1)};
    }
    // work units of the streaming pipeline: one per primary sample of the plan's pixels
    uint64_t units(int spp) const {
        uint64_t n = 0;
        for (int32_t t : tiles) {
            const TileRect r = clip(t);
            if (r.xb > r.xa && r.yb > r.ya) n += (uint64_t)(r.xb - r.xa) * (r.yb - r.ya) * (uint64_t)spp;
        }
        return n;
    }
};

// One frame job: what every render entry works out before it launches, and what its driver needs.  prepare_frame fills the first line, the entry the rest.
struct FrameJob {
    Plan plan; zr::DCamera dc; zr::DEnv de{}; uint64_t seed = 0; hipStream_t stream = nullptr;
    bool count = false;                               // zr_counters wanted
    uint32_t sample0 = 0;                             // a batch of a progressive render: dc.spp samples from this one on (render_stream; 0 = the whole frame)
    double* d_out = nullptr; double* d_out2 = nullptr;   // device frames (d_out2: the refraction frame of the split's replay pass)
    volatile const uint8_t* keep_going = nullptr; volatile int* rows_done = nullptr;
    zr::StreamProgress* progress = nullptr;
    uint32_t direct = 0;                              // an accumulator bound to the direct-light integrator (zr_accum_set_direct): 0x80000000 | its flags (| kDirectEnv)
    const uint32_t* d_list = nullptr; uint32_t n_list = 0;   // a device pixel list of the caller's (an adaptive pass: the active pixels) instead of the plan's cached one
    bool interactive() const { return keep_going || rows_done; }   // the caller polls: the tile-list paths need batch boundaries
};

// records a pair of HIP events around a launch into zr_ctx::pending (resolve_times turns them into milliseconds); the one recycler of zr_ctx::pool
struct HostTimer : zr::StreamTimer {
    zr_ctx* c; hipEvent_t cur_a = nullptr; hipError_t err = hipSuccess;
    explicit HostTimer(zr_ctx* c) : c(c) {}
    hipEvent_t get() {
        if (!c->pool.empty()) { hipEvent_t e = c->pool.back(); c->pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        if ((err = hipEventCreate(&e)) != hipSuccess) return nullptr;
        return e;
    }
    void begin(hipStream_t st, int) override { cur_a = get(); if (cur_a) (void)hipEventRecord(cur_a, st); }
    void end(hipStream_t st, int kind) override {
        hipEvent_t b = get();
        if (!cur_a || !b) return;
        (void)hipEventRecord(b, st);
        zr_ctx::Pending pe{}; pe.a = cur_a; pe.b = b; pe.render_id = c->render_id; pe.kind = kind;
        c->pending.push_back(pe);
        cur_a = nullptr;
    }
    size_t logged() override { return c->pending.size(); }
    void drop_from(size_t n) override {
        for (size_t i = n; i < c->pending.size(); i++) { c->pool.push_back(c->pending[i].a); c->pool.push_back(c->pending[i].b); }
        if (n < c->pending.size()) c->pending.resize(n);
    }
    int status() const { return err == hipSuccess ? ZR_OK : fail(ZR_E_DEVICE, "hipEventCreate(&e) failed: %s", hipGetErrorString(err)); }
};

int make_plan(const zr_camera& cam, const zr_region* region, Plan& p);
std::vector<uint32_t> plan_pixels(const Plan& plan);   // the plan's pixels in tile order, x | y << 16 (ST_MAX_FRAME_SIDE)
bool list_runs_reversed();                             // does the pipeline's own pixel list run in the reverse of plan_pixels' order?
int lanes_for(int n);
int copy_region(const Plan& p, const double* d_frame, double* out, std::vector<double>& scratch);
int scene_ready(const zr_ctx* c, const zr_scene* s, const char* entry, bool any_context = false);
int prepare_frame(zr_ctx* c, const zr_scene* s, const zr_camera* cam, const zr_env* env, uint64_t seed, const zr_region* region, FrameJob& job,
                  const Plan* plan = nullptr);
int resolve_times(zr_ctx* c);
bool fits_stream(const zr_ctx* c, const zr_scene* s, const Plan& plan, const zr::DCamera& dc, int depth_factor, uint64_t units);
int render_stream(zr_ctx* c, const zr_scene* s, const FrameJob& job, int mode = 0);
// the above: zr_render.cpp; zr_accum.cpp (enqueue_render calls it) and zr_image.cpp (zr_accum_denoise calls them):
int render_batched(zr_ctx* c, const zr_scene* s, const FrameJob& frame, int n_max);
int denoise_guided_device(zr_ctx* c, const zr_denoise_guided_params* dp, DevBuf<double>& d_c, DevBuf<double>& d_v, const double* albedo, const double* normal,
                          const double* zdepth, int W, int H, double* out, double* out_variance);
int check_guided_params(const zr_denoise_guided_params* dp);
// likewise for the non-local-means filter: d_a / d_b hold the two halves and receive out / out_error, d_v holds the variance of the full mean
int denoise_nlm_device(zr_ctx* c, const zr_denoise_nlm_params* dp, DevBuf<double>& d_a, DevBuf<double>& d_b, DevBuf<double>& d_v, const double* albedo,
                       const double* normal, int W, int H, double* out, double* out_error);
int check_nlm_params(const zr_denoise_nlm_params* dp);
// zr_render.cpp, for zr_temporal.cpp: camera::initialize's frame, and zr_trace's body for rays that are on the device already
void camera_frame(const zr_camera& cam, zr::DCamera& dc);
int trace_device(zr_ctx* c, const zr_scene* s, const double* d_rays, size_t n, double tmin, double tmax, uint64_t seed, uint64_t pixel, uint32_t bounce,
                 zr_hit* d_hits, uint2* d_ki = nullptr /* per ray the (kind, index) both engines hold where they fill zr_hit; all ones on a miss */);
// zr_render.cpp, for zr_direct.cpp: the ray-independent environment of make_env, checked against the scene's textures
int env_frame(const zr_env& env, const zr_scene* s, zr::DEnv& de);
// zr_direct.cpp, for zr_accum.cpp (render_batch_samples calls it): a batch of a direct-light accumulator — render_batch_samples' pixel-group branch
// with the direct kernel; builds the scene's light table on first use
int check_direct_params(const zr_direct_params* dp);
// ... and DESIGN §21: kDirectEnv in FrameJob::direct / AccumState::direct asks for the environment map to be sampled too (zr_accum_set_direct_env)
const uint32_t kDirectEnv = 0x40000000u;
int render_direct_samples(zr_ctx* c, const zr_scene* s, FrameJob& job, const uint32_t* pixels, uint32_t n_pix, int sample0, int n, HostTimer& timer);
// zr_temporal.cpp, for zr_accum.cpp (zr_accum_temporal calls them): the parameter check, what a call checks before any device work (its null tests aside),
// and one frame taken from device memory (d_color / d_variance: W*H*3 doubles, complete on the context's stream)
int check_temporal_params(const zr_temporal_params* p);
int temporal_call_ready(const zr_temporal* t, const zr_ctx* c, const zr_scene* s, const zr_camera* cam, const char* entry);
int temporal_accumulate_device(zr_temporal* t, const zr_temporal_params* p, const zr_scene* s, const zr_camera* cam, uint64_t seed, const double* d_color,
                               const double* d_variance, double* out_color, double* out_variance, int32_t* out_history);

}  // namespace zr_host
