// zr_host_internal.h — what the host-side translation units of libzr_hip.so share (round 4: zr_host.cpp was one 2 482-line file):
//   zr_host.cpp    context life cycle, error string, small C-ABI entry points
//   zr_commit.cpp  scene setters, the commit plan, zr_scene_commit through the host builder or the device builder (zr_flatten.h: validation, the plan, the
//                  flattener and the host builder's CPU half — no HIP, built on zr_scene_input.h: the world as given)
//   zr_update.cpp  moving worlds: zr_scene_update_* on the host copy, zr_scene_refit and its state (zr_update.h: the rules, no HIP; zr_refit.h / .hip: the device side)
//   zr_scene_query.cpp  what a committed scene answers: statistics, kernel builds, traversal stack, builder, zr_scene_tree_boxes
//   zr_render.cpp  camera frame / sky constants, the frame job every render entry prepares (tile plan, validation) and its drivers (streaming pipeline, fused
//                  kernel, pixel-group kernel), AOV / split passes, BVH debug view, counters, known-answer entry points
//   zr_accum.cpp   the accumulator (zr_accum): a frame in batches of samples, adaptive sampling, the queries of what it holds, render_batched
//   zr_direct.cpp  direct light sampling: the scene's light table, the batch driver of a direct accumulator, zr_render_direct, its known-answer entries
//   zr_envlight.cpp  ... and of the HDR environment map: the environment table, zr_render_direct_env, its dump and known-answer entries
//   zr_image.cpp   the image-space entry points, which need no scene: post stack, the two denoisers, sharpening, frame analysis
//                  (these three share zr_frame.h: Plan, FrameJob, HostTimer and the drivers one of them calls in another)
// Plain C++ (host compiler, -ffp-contract=off so that the camera frame and the sky constants are computed with exactly the reference's operation order,
// camera.hpp:358-399, 874-895,914); the kernels live in the .hip files.  There is deliberately no CPU rendering path in this library: without a HIP device
// zr_create() fails and says so.
#pragma once
#include <hip/hip_runtime_api.h>

#include "zr_build.h"
#include "zr_scene_input.h"
#include "zr_launch.h"

#define HIP_OK(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) return fail(ZR_E_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_));       \
    } while (0)

namespace zr_host {

const double kPi = 3.14159265358979323846;

struct H3 { double x, y, z; };
inline H3 h3(const double* p) { return H3{p[0], p[1], p[2]}; }
inline H3 operator+(H3 a, H3 b) { return H3{a.x + b.x, a.y + b.y, a.z + b.z}; }
inline H3 operator-(H3 a, H3 b) { return H3{a.x - b.x, a.y - b.y, a.z - b.z}; }
inline H3 operator-(H3 a) { return H3{-a.x, -a.y, -a.z}; }
inline H3 operator*(double t, H3 v) { return H3{t * v.x, t * v.y, t * v.z}; }
inline H3 operator*(H3 v, double t) { return t * v; }
inline H3 operator/(H3 v, double t) { return (1 / t) * v; }  // vec3.hpp:149-151
inline H3 cross(H3 a, H3 b) { return H3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double len(H3 a) { return std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
inline H3 unit(H3 v) { double l = len(v); if (l < 1e-8) return H3{0, 0, 0}; return v / l; }
inline void st3(double* d, H3 v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; }
inline double clampd(double v, double lo, double hi) { return v < lo ? lo : (hi < v ? hi : v); }

template <class T>
struct DevBuf {
    T* p = nullptr; size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
    ~DevBuf() { release(); }
    void release() { if (p) { (void)hipFree(p); p = nullptr; n = 0; } }
    int upload(const std::vector<T>& v) { return upload(v.data(), v.size()); }
    int upload(const zr::RawArray<T>& v) { return upload(v.data(), v.size()); }
    int upload(const T* src, size_t count) {
        release();
        n = count;
        size_t bytes = std::max<size_t>(sizeof(T) * count, 64);  // never a null device pointer
        HIP_OK(hipMalloc((void**)&p, bytes));
        if (count) HIP_OK(hipMemcpy(p, src, sizeof(T) * count, hipMemcpyHostToDevice));
        return ZR_OK;
    }
    int alloc(size_t count) {
        if (count == n && p) return ZR_OK;
        release();
        if (hipMalloc((void**)&p, std::max<size_t>(sizeof(T) * count, 64)) != hipSuccess) {
            p = nullptr; (void)hipGetLastError();
            return fail(ZR_E_DEVICE, "out of device memory (%zu bytes requested)", sizeof(T) * count);
        }
        n = count;
        return ZR_OK;
    }
};

}  // namespace zr_host
using namespace zr_host;

struct zr_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t sub[ST_MAX_POOLS] = {};   // internal streams of the streaming pipeline's sub-pools 1..K-1 (sub[0] unused)
    DevBuf<unsigned long long> d_ctr;
    DevBuf<double> d_out;
    DevBuf<int32_t> d_tiles;
    bool warned_fallback = false;         // the notice about a frame beyond the streaming pipeline's limits has been printed
    int variant = 2;                      // 2 streaming wavefront pipeline (default); 0 pixel-group megakernel (the fallback for frames beyond the pipeline's packing limits)
    // variant 2: slot pool and per-frame buffers
    DevBuf<unsigned char> d_pool;
    DevBuf<uint32_t> d_pixels;
    DevBuf<double> d_partial;
    // the sky pre-pass (zr_sky.hip): flag per list position, the compaction's block counts, the pixels the pipeline walks, their number; grown as frames need
    DevBuf<uint32_t> d_sky_flag, d_sky_blocks, d_walk_pixels, d_n_walk;
    uint64_t presolved = 0, presolved_render = 0;   // pixels the pre-pass resolved in render `presolved_render` (zr_last_presolved_pixels)
    DevBuf<uint32_t> d_kend;              // reflection / refraction split: (draws, segments) of every unit's beauty path
    DevBuf<unsigned char> d_cls;           // ... and the class of its second path
    DevBuf<unsigned long long> d_cpart;    // ... and the per-block counters of the two passes
    DevBuf<unsigned int> d_ctl;
    DevBuf<unsigned char> d_st_overflow;
    uint32_t st_ovf_levels = 0;           // levels per lane the spill slabs of d_st_overflow hold
    int st_blocks = 0;
    int fused_blocks = 0;                 // persistent grid of the fused small-scene kernel (0: not asked yet)
    uint32_t st_slots = 0;
    int st_pools = -1;                    // sub-pools staggered on separate streams: 1 = one pool, -1 = auto
    hipEvent_t st_event = nullptr;
    unsigned int* h_active = nullptr;     // pinned
    unsigned int* h_polls = nullptr;      // pinned: the round loop's poll ring (zr_round_polls.h), written by the device
    hipEvent_t poll_events[zr::POLL_RING * ST_MAX_POOLS] = {};   // ... and the event behind each of its slots
    int last_drain_round = 0, last_sub_pools = 0;   // of the last pipeline frame: the loop round after which the survivors moved to the drain pool (0: never), sub-pools it began with
    int last_shade_launches[2] = {0, 0};            // of the last pipeline frame: SHADE launches of the in-place lean build / of the sorted builds (zr_last_shade_builds)
    std::vector<int32_t> pix_key;         // plan the cached pixel list was built for
    uint64_t last_rounds = 0;
    int last_path = 0;                    // zr_counters::path of the last render
    double last_extend_ms = 0, last_shade_ms = 0;
    // device timing of render-kernel launches: HIP events recorded on the stream the kernel is launched on
    struct Pending { hipEvent_t a, b; uint64_t render_id; int kind; };
    std::vector<hipEvent_t> pool;     // recycled events
    std::vector<Pending> pending;     // launches not yet resolved to milliseconds
    std::vector<float> log;           // resolved launch times since the last zr_get_kernel_times (oldest first)
    int log_kind = 1;                 // ZR_TIMELOG_KIND: which kernel zr_get_kernel_times reports (1 extend/render, 2 shade)
    uint64_t render_id = 0;
    double last_render_ms = 0;        // sum over the launches of the most recent render call
    hipStream_t last_stream = nullptr;
    bool last_counted = false;
    uint64_t direct_slots = 0, direct_objects = 0;   // the light table of the last direct-light batch (zr_get_direct_stats)
    uint64_t direct_render = 0;                      // ... and the render it was (render_id): the counter block holds its shadow-query counts while no other render followed
    // memory a commit frees off the caller's clock (staging arrays, the device builder's arena): at most one such thread is outstanding, and zr_destroy joins it —
    // a detached thread could still be inside hipFree while the process tears the HIP runtime down
    std::mutex trash_m;
    std::thread trash;
    template <class F> void free_later(F&& f) {
        std::lock_guard<std::mutex> lk(trash_m);
        if (trash.joinable()) trash.join();
        try { trash = std::thread(std::forward<F>(f)); } catch (...) { f(); }
    }
    void drain_trash() { std::lock_guard<std::mutex> lk(trash_m); if (trash.joinable()) trash.join(); }
};

struct RefitState;   // zr_update.cpp
namespace zr_host { struct LightCache; }   // zr_direct.cpp
namespace zr_host { struct EnvLightCache; }   // zr_envlight.cpp

struct zr_scene : SceneInput {   // the world as given (host side), then what the commit made of it
    zr_ctx* ctx = nullptr;
    int device = 0;               // the context's device ordinal, kept here so that zr_scene_destroy needs no live context (a scene may outlive its context)
    bool borrowed = false;        // the geometry arrays are the caller's (released after the commit)
    bool released = false;        // ... and have been released: the scene cannot be committed again without new input
    unsigned reset_mask = 0;      // ... which geometry arrays have been given again since (SET_* bits, zr_commit.cpp: GEOMETRY_SET)
    // device
    bool committed = false;
    DevBuf<zr::NodePair> d_nodes;
    DevBuf<zr::NodeQ> d_quads;
    bool quad_ok = true;          // leaf references fit the EXTEND kernel's 32-bit stack entries
    DevBuf<double> d_spheres, d_tri_v, d_tri_s, d_cubes, d_pcubes;
    DevBuf<uint32_t> d_sphere_mat, d_cube_mat, d_pcube_mat;
    DevBuf<zr::DMedium> d_media;
    DevBuf<zr::DWrapped> d_wrapped;
    DevBuf<zr::DInstance> d_insts;
    DevBuf<zr_xform_op> d_ops;
    DevBuf<zr_material> d_mats;
    DevBuf<zr_texture> d_texs;
    DevBuf<unsigned char> d_texels;
    zr::DScene ds{};
    int leaf_level = 2;           // EXTEND build: 0 bare triangles / spheres only, 1 + bare and placed cubes and unwrapped media, 2 everything
    uint32_t stack_demand = 0;    // worst-case entries on an EXTEND lane's traversal stack (Flattener::stack_demand)
    size_t leaf_objects = 0;      // leaf objects of the world's tree (all kinds): small worlds render through the fused kernel
    zr::FusedObjs fused{};        // ... their records, for the kernel arguments (finish_commit)
    bool fused_ok = false;
    uint64_t stats[4] = {0, 0, 0, 0};
    const char* builder = "";   // which builder made the committed tree (zr_scene_builder)
    std::vector<uint32_t> leaf_src[8];   // per leaf kind, in that kind's array order: a leaf primitive's index in the caller's arrays (zr_scene_tree_boxes);
                                         // 0xFFFFFFFF for the primitives inside media and wrapper chains
    // ---- moving worlds (zr_update.cpp: zr_scene_update_*, zr_scene_refit).  What the commit keeps for them — only of a scene it may bake again, i.e. one
    // whose arrays were copied — and the state of the updates since
    std::vector<zr_object> plan_objs;    // the commit plan's world list ...
    std::vector<uint8_t> plan_code;      // ... its classification per entry (leaf kind | baked << 4): an update must not change it
    bool plan_bake = true;               // ... and the knob it was made with (BuildKnobs::bake)
    uint32_t plan_cnt[8] = {};           // leaf objects per kind
    std::vector<zr::BuildBox> group_box; // per zr_group: the box of its triangles in their own space, as the builder that made the tree computed it
    bool stale = false;                  // an update changed the host copy of the world and no refit has followed: nothing may read the device scene
    uint64_t epoch = 0;                  // refits applied to this commit
    uint64_t serial = 0;                 // of this commit among all commits of the process (an epoch alone restarts at 0): what a tracking zr_temporal remembers
    mutable std::shared_ptr<zr_host::LightCache> lights;   // the light table of (serial, epoch), built by the first direct-light render that needs it
    mutable std::shared_ptr<zr_host::EnvLightCache> env_light;   // the environment table of (serial, a texture), built by the first use that needs it; refits keep it
    std::shared_ptr<RefitState> refit;   // reverse indices, leaf boxes, the trees' schedule, device buffers: made by the first update or refit after a commit, dropped by the next
};

// The motion table of a scene's last refit as the temporal stage reads it on the device (zr_update.cpp): the step epoch - 1 -> epoch.
// leaf_word[leaf_base[kind] + index] = a slot among `records` (21 doubles each), ZR_MOTION_STATIC or ZR_MOTION_CUT.  All null for a scene no refit state exists for.
struct MotionView { const uint32_t* leaf_word = nullptr; const double* records = nullptr; uint32_t leaf_base[8] = {}; uint32_t n_leaves = 0, n_slots = 0; };
MotionView scene_motion_view(const zr_scene* s);
// per leaf primitive of the world's tree (leaf_base[kind] + index) its world-list entry, on the device; builds the host half of the refit state if there is none
int scene_leaf_entries(zr_scene* s, const uint32_t** d_leaf_entry, MotionView* view);

// the small world's objects as the fused kernel's arguments (zr_launch.h: FusedObjs), read back from the device arrays: by a commit and again by a refit
int refresh_fused_objects(zr_scene* s);

struct CommitSummary {   // what the shared end of a commit needs to know about the tree either builder produced (counts and array sizes: the CommitPlan's)
    zr::NodeF root{}; bool quant_ok = true;
    size_t n_pairs = 0, n_quads = 0, kept_closed = 0;
    bool plain_media = true;   // every medium's boundary is an unwrapped sphere or cube
    uint32_t stack_demand = 0; int quad_depth = 0, max_depth = 0;
    const char* builder = "";
};
