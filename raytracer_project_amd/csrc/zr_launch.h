// zr_launch.h — host-visible launch interface of zr_kernels.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/zr_capi.h"
#include "zr_round_polls.h"

#define ZR_BLOCK 256

namespace zr {

struct DScene;
struct DCamera;
struct DEnv;

// The context's counter block (zr_ctx::d_ctr, `gctr` in the kernels): CTR_BLOCK 64-bit words, cleared before every render.  zr_get_counters hands the
// first CTR_WORDS of them out as zr_counters; an instrumented render (count != 0) fills words 0-12, 14 (lean SHADE) and 15.
enum { CTR_SAMPLES = 0, CTR_SEGMENTS = 1, CTR_NODES = 2, CTR_SPHERES = 3, CTR_TRIANGLES = 4, CTR_CUBES = 5, CTR_MEDIA = 6, CTR_HITS = 7, CTR_DRAWS = 8,
       CTR_NODE_EXECS = 9, CTR_NODE_LANES = 10, CTR_LEAF_EXECS = 11, CTR_LEAF_LANES = 12,   // EXTEND's iterations per phase and the lanes they ran with
       CTR_SHADE_EXECS = 13, CTR_SHADE_LANES = 14,   // zr_counters::shade_execs / shade_lanes.  shade_execs: no kernel of the product build writes it (zero).  shade_lanes:
                                                     // the counting lean SHADE adds the slots it shaded, i.e. the segments EXTEND handed it; other builds leave it zero; see below
       CTR_ESCAPED = 15,                             // segments lean SHADE finished itself (ray_escapes); they are part of CTR_SEGMENTS
       CTR_WORDS = 16,
       CTR_HIST = 16, CTR_HIST_WORDS = 24,           // ZR_WAVE_PROFILE build only: EXTEND's per-phase lane histograms, [phase][8 buckets of 8 lanes]
       CTR_FETCH_CHECKED = 40, CTR_FETCH_SKIPPED = 41,   // the counting lean EXTEND: slots it fetched with / without testing their meta word (zr_last_extend_fetches)
       CTR_DIRECT_SHADOW = 42, CTR_DIRECT_VISIBLE = 43, CTR_DIRECT_SUN = 44,   // the counting direct-light kernel (zr_direct.hip): shadow queries, those that saw their sample, sun queries among them (zr_get_direct_stats)
       CTR_DIRECT_ENV = 45, CTR_DIRECT_ENV_VISIBLE = 46,   // ... queries towards the environment map among them, and those that saw it (zr_get_direct_env_stats)
       CTR_BLOCK = 48 };
// A -DZR_WAVE_PROFILE build (scripts/wave_profile.sh) runs uninstrumented renders and REUSES words of the block for EXTEND's wave statistics, read back
// through the zr_counters fields of the words' product meaning (ZR_RAW_COUNTERS=1, scripts/wave_profile.py): phase p = 0 NODE, 1 LEAF, 2 FETCH
enum { CTR_PROF_EXECS = 1, CTR_PROF_LANES = 2,   // + 2 * p: iterations of phase p, lanes they ran with (words 1-6)
       CTR_PROF_WAVE_TICKS = 13,                 // sum of wave lifetimes in 10 ns ticks (read as shade_execs)
       CTR_PROF_WAVES = 14 };                    // waves launched (read as shade_lanes)

// which pixels one launch covers: the tiles `tiles[0..n_tiles)` (row-major tile ids), clipped to the
// rectangle [x0,x1) x [y0,y1)
struct WorkDesc {
    const int32_t* tiles;
    int32_t n_tiles, tile_size, tiles_x;
    int32_t x0, y0, x1, y1;
    int32_t lanes_per_pixel;
};

hipError_t launch_render(const DScene& sc, const DCamera& cam, const DEnv& env, uint64_t seed, const WorkDesc& wd, double* out,
                         unsigned long long* gctr, bool count, hipStream_t stream);
// variant 2: streaming wavefront pipeline (zr_stream.hip)
struct StreamTimer {  // host-provided HIP-event recorder; kind: 0 init, 1 extend, 2 shade, 3 reduce
    virtual void begin(hipStream_t, int kind) = 0;
    virtual void end(hipStream_t, int kind) = 0;
    virtual size_t logged() { return 0; }      // launches recorded so far
    virtual void drop_from(size_t) {}          // forget the launches recorded after the first `logged()` ones (the rounds queued behind the one that emptied the pools)
    virtual ~StreamTimer() = default;
};
// host-provided progress sink of the round loop (camera::lines_rendered and the live preview of camera.hpp:548-552 / main.cpp:1576):
// after every host synchronisation of the loop, report() gets the fraction of the frame's samples that are finished;
// when wants_frame() said yes just before, `out` holds the mean of the samples finished so far (partial sums / spp)
struct StreamProgress {
    virtual bool wants_frame() = 0;
    virtual void report(double finished_fraction, bool frame_reduced) = 0;
    virtual ~StreamProgress() = default;
};
#define ST_MAX_POOLS 8   /* sub-pools of the slot pool, one HIP stream each */
enum { CTL_CAPPED = 2 };   // control block (zr_ctx::d_ctl; the rest of its layout: zr_stream.hip, CTL_*): EXTEND waves that hit their iteration cap
uint32_t stream_overflow_levels(uint32_t stack_demand);
size_t stream_overflow_bytes(int blocks, uint32_t levels);
size_t stream_ctl_words();
int stream_extend_blocks();
size_t stream_pool_bytes(uint32_t P);
// Packing limits of the pipeline.  A frame or scene beyond one of them is rendered by the pixel-group kernel (zr_render.cpp: fits_stream).
constexpr int ST_MAX_BOUNCES = 250;               // the bounce counter is 8 bits of a slot's flag word (zr_stream.hip: SF_MA)
constexpr uint64_t ST_MAX_UNITS = 0xFFFFFFFFull;   // work units (one per primary sample) are numbered in 32 bits (SF_MB)
constexpr int ST_MAX_FRAME_SIDE = 65535;           // a pixel of the pixel list is x | y << 16
constexpr uint32_t ST_MAX_LEAF_PRIMS = 1u << 24;   // a leaf reference is 24 bits of index + 4 of count (zr_scene::quad_ok, decided at the commit)
// One run of the pipeline, grouped by what the arguments are for.  Pointers are device memory unless they say otherwise; the hooks may all be null.
struct StreamFrame {     // what is rendered: one work unit per primary sample of the n_pix listed pixels (x | y << 16)
    const DCamera* cam; const DEnv* env; uint64_t seed; uint32_t spp, n_pix; const uint32_t* pixels;
    double* samples;     // per-sample radiance, 3 doubles per unit
    double *out, *out2;  // the frame the samples are reduced into (null: none wanted) and, in mode 2, the refraction frame
    bool count;          // the instrumented builds (zr_counters)
    uint32_t sample0 = 0;   // the run renders samples [sample0, sample0 + spp) of every pixel (a batch of a progressive render; 0: the whole frame)
};
struct StreamPool {      // the frame's slot pool; the small pool the survivors of its drain are moved to (null: not used); chunk of the XCD-affine hand-out (0: striped)
    void* slots; uint32_t P; void* drain; uint32_t drain_slots, unit_chunk;
};
struct StreamContext {   // what the context owns (zr_ctx): control block, EXTEND's spill slabs and persistent grid, counter block (CTR_*), streams, pinned copy of ctl (of which a frame with a progress sink fills the unit counters' block), poll ring
    unsigned int* ctl; void* overflow; uint32_t ovf_levels; int extend_blocks; unsigned long long* gctr;
    hipStream_t* streams; int n_pools;   // streams[0] is the caller's stream, the others are internal; n_pools: sub-pools wanted
    hipEvent_t event; unsigned int* h_active;
    // the round loop's polls (zr_round_polls.h): pinned [POLL_RING][ST_MAX_POOLS][POLL_WORDS] words that the device writes, and one event (no timing) per sub-pool and
    // ring slot, [POLL_RING][ST_MAX_POOLS].  The round loop learns what the device did from them alone: stream_render answers a null ring with
    // hipErrorInvalidValue.  stream_trace does not poll: null there
    unsigned int* h_polls = nullptr; hipEvent_t* poll_events = nullptr;
};
struct StreamSplit { int mode; void* kend; void* cls; unsigned long long* cpart; };   // mode 0: the render; 1 / 2: the passes of the reflection / refraction split, with their buffers
struct StreamHooks {     // the host's view into the loop
    StreamTimer* timer; volatile const uint8_t* keep_going /* host memory, polled between rounds: 0 cancels */; StreamProgress* progress;
    int* done_out;       // rounds run (stream_render: up to and including the one that emptied the pools) or parts launched (fused_render_frame); negative: cancelled after that many
    int* drain_out = nullptr;   // stream_render: the round after which the survivors moved to the drain pool (0: they never did); [1]: the sub-pools the frame began with
    int* shade_out = nullptr;   // stream_render: SHADE launches enqueued, [0] of the in-place lean build, [1] of every sorted build (the rounds queued behind the emptying one included)
};
struct StreamJob { StreamFrame frame; StreamPool pool; StreamContext ctx; StreamSplit split; StreamHooks hooks; };
// leaf_level: the EXTEND build the scene needs (zr_scene::leaf_level)
hipError_t stream_render(const DScene& sc, const StreamJob& job, int leaf_level);
// The objects of a small world as the fused kernel wants them: IN THE KERNEL ARGUMENTS.  The kernarg segment is read with scalar
// loads, so an object's record reaches every lane of a wave through SGPRs — no vector memory instruction, no VGPRs per lane for
// data that is the same in all of them (reading the records through the scene's pointers, the compiler issued 255 vector loads
// in the loop and spilled; the pointers come out of a struct, so it cannot prove the addresses uniform and read-only).
// rec: sphere cx cy cz r | triangle 9 vertices | cube 6 | placed cube 16 (ZR_PCUBE_STRIDE) | plain medium: boundary (sphere 4 / cube 6), [6] = -1/density,
// [7] = id bits, [8] = boundary type bits.
#define ZR_FUSED_OBJECTS 16
struct FusedObjs {
    uint32_t n, pad_;
    uint32_t kind[ZR_FUSED_OBJECTS];    // leaf kind (ZR_PRIM_* / ZR_KIND_PCUBE); media here are plain ones only
    uint32_t index[ZR_FUSED_OBJECTS];   // index in that kind's array (what a hit reports)
    double rec[ZR_FUSED_OBJECTS][16];   // (a placed cube's record is the longest: ZR_PCUBE_STRIDE)
};
int fused_blocks();
// uses of `ctx`: ctl, gctr, streams[0].  level: 1 = no wrapped objects and only plain media, 2 = everything but placements
hipError_t fused_render_frame(const DScene& sc, const StreamFrame& frame, const StreamContext& ctx, int blocks, int level, const FusedObjs& objs, const StreamHooks& hooks);
// Progressive accumulation (zr_accum, zr_stream.hip): `partial` holds 64 lane sums x 3 channels per pixel ([pixel][channel][lane], 192 doubles).
// launch_accumulate adds a batch of per-sample radiance ([n_pix][n][3], the samples sample0 ... sample0 + n - 1) to it: sample s goes to lane s % 64, in increasing s
// (flip: the batch's pixel list ran in the reverse of the accumulator's order).  launch_accum_resolve writes the mean of the `done` samples held into
// the listed pixels of `out` (frame width W); asc_lanes: 1 = stream_reduce's butterfly, L = lanes_for(done) the pixel-group kernel's.
constexpr size_t ACCUM_DOUBLES_PER_PIXEL = 192;
hipError_t launch_accumulate(const double* samples, uint32_t n_pix, uint32_t n, uint32_t sample0, bool flip, double* partial, hipStream_t stream);
hipError_t launch_accum_resolve(const double* partial, const uint32_t* pixels, uint32_t n_pix, int W, int done, int asc_lanes, double* out, hipStream_t stream);
// the pixel-group kernel's arithmetic for one batch: samples [sample0, sample0 + n) of the listed pixels, written as per-sample radiance ([n_pix][n][3]) for launch_accumulate
hipError_t launch_render_samples(const DScene& sc, const DCamera& cam, const DEnv& env, uint64_t seed, const uint32_t* pixels, uint32_t n_pix, uint32_t sample0,
                                 uint32_t n, double* samples, unsigned long long* gctr, bool count, hipStream_t stream);
// Adaptive sampling (zr_render_adaptive, zr_adaptive.hip).  launch_adaptive_accumulate: one pass's samples ([n_list][n][3]) of the active list onto the lane sums of
// the slots slot[i], then the noise estimate of the updated sums: count[slot] = new_count, flag[i] = 1 goes on / 2 noisy at max_samples / 0 converged.
// launch_adaptive_compact: the positions with flag 1, in order, into pixels_out / slot_out; totals (device) = {active, at max}; block_active / block_at_max: scratch of
// ceil(n_list / 256) words each.  launch_accum_error: the estimate of every slot (count: per slot, or null for uniform_count).  launch_accum_resolve_counts:
// launch_accum_resolve with 1.0 / count[pixel].
hipError_t launch_adaptive_accumulate(const double* samples, const uint32_t* slot, uint32_t n_list, uint32_t n, uint32_t sample0, double* partial, int32_t* count,
                                      uint32_t* flag, int new_count, int max_samples, double threshold, double dark_floor, hipStream_t stream);
hipError_t launch_adaptive_compact(const uint32_t* flag, uint32_t n_list, const uint32_t* pixels_in, const uint32_t* slot_in, uint32_t* pixels_out,
                                   uint32_t* slot_out, uint32_t* block_active, uint32_t* block_at_max, uint32_t* totals, hipStream_t stream);
hipError_t launch_accum_error(const double* partial, const int32_t* count, int uniform_count, uint32_t n_pix, double dark_floor, double* err, hipStream_t stream);
hipError_t launch_accum_resolve_counts(const double* partial, const uint32_t* pixels, const int32_t* count, uint32_t n_pix, int W, int asc_lanes, double* out,
                                       hipStream_t stream);
// the per-channel variance of every slot's mean into the listed pixels of `out` (frame width W, 3 doubles a pixel; count as launch_accum_error's)
hipError_t launch_accum_variance(const double* partial, const uint32_t* pixels, const int32_t* count, int uniform_count, uint32_t n_pix, int W, double* out,
                                 hipStream_t stream);
// the two half images of every slot (the even lanes' mean, the odd lanes' mean) into the listed pixels of out_a / out_b (as launch_accum_variance)
hipError_t launch_accum_halves(const double* partial, const uint32_t* pixels, const int32_t* count, int uniform_count, uint32_t n_pix, int W, double* out_a,
                               double* out_b, hipStream_t stream);
// The firefly-robust resolve (zr_accum_resolve_robust, zr_robust.hip): the Gini-trimmed mean of every slot's lane sums, the variance of that mean and the trim,
// into the listed pixels of out / out_var (3 doubles a pixel) / out_trim (one int32) of a frame W wide.  pixels null: slot i goes to element i
// (zr_kat_resolve_robust).  out_var / out_trim may be null; count as launch_accum_error's; mode / trim / strength: zr_robust_params, checked by the caller.
hipError_t launch_accum_resolve_robust(const double* partial, const uint32_t* pixels, const int32_t* count, int uniform_count, uint32_t n_pix, int W, int mode,
                                       int trim, double strength, double* out, double* out_var, int32_t* out_trim, hipStream_t stream);
// The sky pre-pass (zr_sky.hip): of the n_pix listed pixels, those whose every camera ray of the samples [sample0, sample0 + spp) provably sees only the
// environment get their mean written to `out` (stream_reduce's value, bit for bit); the others go, in list order, to walk[0 .. *n_walk).  Device scratch:
// flag and walk n_pix words, block_count ceil(n_pix / 256) words, n_walk one word.  ZR_SKY_SIEVE=1 puts a one-ray sieve in front (same flags, frame and list).
hipError_t launch_sky_prepass(const DScene& sc, const DCamera& cam, const DEnv& env, uint64_t seed, const uint32_t* pixels, uint32_t n_pix, uint32_t spp,
                              uint32_t sample0, double* out, uint32_t* flag, uint32_t* block_count, uint32_t* walk, uint32_t* n_walk, hipStream_t stream);
// closest hits of n rays in [0.001, inf) through the EXTEND kernel on ctx.streams[0]; `pool` holds stream_pool_bytes(round_up(n, 64)) bytes.  d_out_ki (may be null):
// per ray the (kind, index) of the leaf primitive that answered, as closest_hit names it (a placed group: ZR_KIND_INSTANCE | instance << 8, the triangle); all ones on a miss
hipError_t stream_trace(const DScene& sc, const double* d_rays, uint32_t n, uint64_t seed, uint64_t pixel, uint32_t bounce, zr_hit* d_out, uint2* d_out_ki, void* pool,
                        const StreamContext& ctx, int leaf_level);
hipError_t launch_aov(const DScene& sc, const DCamera& cam, uint64_t seed, const WorkDesc& wd, int aux, double zmax, const double* uvw9,
                      double* out_albedo, double* out_normal, double* out_zdepth, hipStream_t stream);
hipError_t launch_passes(const DScene& sc, const DCamera& cam, const DEnv& env, uint64_t seed, const WorkDesc& wd, double* out_beauty,
                         double* out_reflection, double* out_refraction, unsigned long long* gctr, hipStream_t stream);
hipError_t launch_post(const double* d_frame, int W, int H, const zr_post_params& pp, int is_data_pass, int apply_gamma, double ev, double* d_tmp0,
                       double* d_tmp1, double* d_tmp2, uint8_t* d_out, hipStream_t stream);
hipError_t launch_analyze(const double* d_frame, size_t n, double* d_part_log, float* d_part_max, int* d_hist, hipStream_t stream);
hipError_t launch_sharpen(const double* d_in, double* d_out, int W, int H, double amount, hipStream_t stream);
hipError_t launch_denoise(const double* d_color, const double* d_albedo, const double* d_normal, const double* d_zdepth, int W, int H,
                          const zr_denoise_params& dp, float4* d_col0, float4* d_col1, float4* d_g0, float4* d_g1, double* d_out,
                          hipStream_t stream);
// the variance-guided form (zr_denoise_guided): d_variance W*H*3 doubles; d_var0 / d_var1 W*H float4 scratch beside the colour's; d_out_var (may be null, may
// be d_variance) receives the filtered variance
hipError_t launch_denoise_guided(const double* d_color, const double* d_variance, const double* d_albedo, const double* d_normal, const double* d_zdepth, int W,
                                 int H, const zr_denoise_guided_params& dp, float4* d_col0, float4* d_col1, float4* d_var0, float4* d_var1, float4* d_g0,
                                 float4* d_g1, double* d_out, double* d_out_var, hipStream_t stream);
// the dual-buffer non-local-means filter (zr_nlm.hip): halves, variance and guides W*H*3 doubles; d_ua .. d_g1 W*H float4 scratch; d_out may be
// d_half_a, d_out_error may be null or d_half_b
hipError_t launch_denoise_nlm(const double* d_half_a, const double* d_half_b, const double* d_variance, const double* d_albedo, const double* d_normal, int W, int H,
                              const zr_denoise_nlm_params& dp, float4* d_ua, float4* d_ub, float4* d_vh, float4* d_vs, float4* d_g0, float4* d_g1, double* d_out,
                              double* d_out_error, hipStream_t stream);
// Temporal accumulation (zr_temporal.hip).  A view is a camera as the reprojection needs it: centre, the first pixel's centre, the unit backward
// axis w, the inverse of the pixel grid (a = du / (du . du), b = dv / (dv . dv): exact because du is perpendicular to dv) and the focus distance.
struct TemporalView { double center[3], pixel00[3], w[3], a[3], b[3], f; };
// one half of a history: the geometry planes of a frame (position / normal 3 doubles a pixel, material id) and the blended colour, variance and history length
struct TemporalPlanes { double* pos; double* nrm; uint32_t* mat; double* col; double* var; int32_t* len; };
hipError_t launch_gbuffer_rays(const DCamera& cam, double* d_rays, hipStream_t stream);
hipError_t launch_gbuffer_pack(const zr_hit* d_hits, const double* d_rays, size_t n, double* d_pos, double* d_nrm, double* d_t, uint32_t* d_mat, hipStream_t stream);
// the motion of the refit between the history's frame and this one: this frame's (kind, index) plane as trace_device writes it, one word per leaf
// primitive of the world's tree at leaf_base[kind] + index (a slot among `records`, ZR_MOTION_STATIC or ZR_MOTION_CUT), the records of 21 doubles
struct TemporalMotion { const uint2* ki; const uint32_t* leaf_word; const double* records; uint32_t leaf_base[8]; uint32_t n_leaves, n_slots; };
hipError_t launch_temporal_reproject(int W, int H, const TemporalView& cur, const TemporalView& prev, bool have_prev, const zr_temporal_params& tp,
                                     const double* d_color, const double* d_variance, const TemporalPlanes& now, const TemporalPlanes& before,
                                     const TemporalMotion* motion /* null: no motion */, hipStream_t stream);
hipError_t launch_gbuffer_entries(const TemporalMotion& mv, const uint32_t* d_leaf_entry, size_t n, uint32_t* d_out, hipStream_t stream);
hipError_t launch_bvh_debug(const DScene& sc, const DCamera& cam, const DEnv& env, uint64_t seed, const WorkDesc& wd, int level, float thickness, double* out,
                            hipStream_t stream);
hipError_t launch_trace_bvh_debug(const DScene& sc, const double* rays, size_t n, double tmin, uint64_t seed, uint64_t pixel, uint32_t bounce, int level,
                                  float thickness, zr_bvh_debug_hit* out, hipStream_t stream);
#define ZR_PATH_REC 17
hipError_t launch_path_records(const DScene& sc, const DCamera& cam, uint64_t seed, const int32_t* req, int n_req, int max_seg, double* out,
                               hipStream_t stream);
hipError_t launch_kat_scatter(const DScene& sc, const double* rays, const zr_hit* recs, const uint64_t* keys, const uint64_t* first_draw, size_t n,
                              zr_scatter_out* out, hipStream_t stream);
hipError_t launch_kat_shade_lean(const DScene& sc, const double* rays, const uint64_t* keys, const uint64_t* first_draw, size_t n, zr_hit* out_hit,
                                 zr_scatter_out* out, hipStream_t stream);
hipError_t launch_kat_texture(const DScene& sc, uint32_t tex, const double* uvp, size_t n, double* out, hipStream_t stream);
hipError_t launch_kat_background(const DScene& sc, const DEnv& env, const double* dirs, size_t n, double* out, hipStream_t stream);
hipError_t launch_kat_camera_rays(const DCamera& cam, uint64_t seed, const int32_t* req, size_t n, double* out, hipStream_t stream);
hipError_t launch_trace(const DScene& sc, const double* rays, size_t n, double tmin, double tmax, uint64_t seed, uint64_t pixel,
                        uint32_t bounce, zr_hit* out, uint2* out_ki /* may be null: as stream_trace's */, hipStream_t stream);

}  // namespace zr
