// zr_temporal.cpp — temporal accumulation on the host side (include/zr_capi.h): the geometry buffer of a camera (zr_render_gbuffer), the history of a
// frame (zr_temporal) and one frame taken into it (zr_temporal_accumulate; zr_accum_temporal in zr_accum.cpp enters at temporal_accumulate_device).  The kernels:
// zr_temporal.hip.
#include "zr_frame.h"

namespace zr_host {
namespace {

// the camera as the reprojection sees it, from the quantities camera::initialize derives (camera_frame) and its backward axis w (camera.hpp:380)
void make_view(const zr_camera& cam, const zr::DCamera& dc, zr::TemporalView& v) {
    const H3 w = unit(h3(cam.lookfrom) - h3(cam.lookat));
    const double uu = (dc.du[0] * dc.du[0] + dc.du[1] * dc.du[1]) + dc.du[2] * dc.du[2];
    const double vv = (dc.dv[0] * dc.dv[0] + dc.dv[1] * dc.dv[1]) + dc.dv[2] * dc.dv[2];
    st3(v.w, w);
    for (int k = 0; k < 3; k++) { v.center[k] = dc.center[k]; v.pixel00[k] = dc.pixel00[k]; v.a[k] = dc.du[k] / uu; v.b[k] = dc.dv[k] / vv; }
    v.f = cam.focus_dist;
}
bool view_finite(const zr::TemporalView& v) {
    const double* d = v.center;   // 16 doubles in a row
    for (int k = 0; k < 16; k++) if (!std::isfinite(d[k])) return false;
    return true;
}
static_assert(sizeof(zr::TemporalView) == 16 * sizeof(double), "a view is 16 doubles");

// The centre rays of `dc` through zr_trace's route into d_hits (npx records), the rays left in d_rays (npx * 6 doubles).  The context's stream is idle on return.
int gbuffer_device(zr_ctx* c, const zr_scene* s, const zr::DCamera& dc, uint64_t seed, double* d_rays, zr_hit* d_hits, uint2* d_ki = nullptr) {
    HIP_OK(zr::launch_gbuffer_rays(dc, d_rays, c->stream));
    return trace_device(c, s, d_rays, (size_t)dc.W * dc.H, 0.001, HUGE_VAL, seed, ZR_GBUFFER_STREAM, 0, d_hits, d_ki);
}

template <class T>
int copy_out(T* out, const T* d, size_t n) {
    if (out && n) HIP_OK(hipMemcpy(out, d, n * sizeof(T), hipMemcpyDeviceToHost));
    return ZR_OK;
}

}  // namespace
}  // namespace zr_host

// Two halves: `cur` holds the history the next frame reprojects from (valid when frames > 0), the other one receives that frame.
struct zr_temporal {
    zr_ctx* ctx = nullptr; int device = 0;
    int W = 0, H = 0;
    int64_t frames = 0;
    int cur = 0;
    zr::TemporalView view{};   // of the frame in half `cur`
    struct Half { DevBuf<double> pos, nrm, col, var; DevBuf<uint32_t> mat; DevBuf<int32_t> len; } half[2];
    DevBuf<double> d_rays, d_in_color, d_in_variance;
    DevBuf<zr_hit> d_hits;
    // motion tracking (zr_temporal_track_motion): the scene, commit and epoch of the frame in half `cur`, and this frame's (kind, index) plane
    bool track = false;
    const zr_scene* held_scene = nullptr; uint64_t held_serial = 0, held_epoch = 0;
    DevBuf<uint2> d_ki;
    size_t npx() const { return (size_t)W * H; }
    zr::TemporalPlanes planes(int k) { Half& h = half[k]; return zr::TemporalPlanes{h.pos.p, h.nrm.p, h.mat.p, h.col.p, h.var.p, h.len.p}; }
};

namespace zr_host {

int check_temporal_params(const zr_temporal_params* p) {
    if (!(p->alpha > 0 && p->alpha <= 1)) return fail(ZR_E_INVALID, "alpha %g outside (0, 1]", p->alpha);
    if (p->max_history < 1 || p->max_history > 65535) return fail(ZR_E_INVALID, "max_history %d outside 1..65535", p->max_history);
    if (!(p->plane_tolerance > 0) || !std::isfinite(p->plane_tolerance)) return fail(ZR_E_INVALID, "plane_tolerance %g is not positive and finite", p->plane_tolerance);
    if (!(p->normal_cos >= -1 && p->normal_cos <= 1)) return fail(ZR_E_INVALID, "normal_cos %g outside [-1, 1]", p->normal_cos);
    return ZR_OK;
}

int temporal_call_ready(const zr_temporal* t, const zr_ctx* c, const zr_scene* s, const zr_camera* cam, const char* entry) {
    if (t->ctx != c) return fail(ZR_E_INVALID, "history belongs to another context");
    const int W = cam->image_width < 1 ? 1 : cam->image_width, H = cam->image_height < 1 ? 1 : cam->image_height;
    if (W != t->W || H != t->H) return fail(ZR_E_INVALID, "camera of %d x %d px, history of %d x %d", W, H, t->W, t->H);
    zr::DCamera dc; zr::TemporalView v;
    camera_frame(*cam, dc); make_view(*cam, dc, v);
    if (!view_finite(v)) return fail(ZR_E_INVALID, "the camera has no finite view (lookfrom, lookat, vup, vfov, focus_dist)");
    return scene_ready(c, s, entry);
}

int temporal_accumulate_device(zr_temporal* t, const zr_temporal_params* p, const zr_scene* s, const zr_camera* cam, uint64_t seed, const double* d_color,
                               const double* d_variance, double* out_color, double* out_variance, int32_t* out_history) {
    zr_ctx* c = t->ctx;
    zr::DCamera dc; zr::TemporalView v;
    camera_frame(*cam, dc); make_view(*cam, dc, v);
    const int nxt = t->cur ^ 1;
    // a tracking history: the same world -> the static path; one refit later -> the motion build with the scene's table; anything else -> the frame restarts
    zr::TemporalMotion mv{}; bool moved = false;
    int rc;
    if (t->track && t->frames > 0) {
        const bool same = t->held_scene == s && t->held_serial == s->serial;
        if (same && s->epoch == t->held_epoch + 1) {
            const MotionView m = scene_motion_view(s);
            if (!m.leaf_word) return fail(ZR_E_DEVICE, "temporal: a refitted scene without a motion table (internal error)");
            if ((rc = t->d_ki.alloc(t->npx()))) return rc;
            mv.ki = t->d_ki.p; mv.leaf_word = m.leaf_word; mv.records = m.records; std::memcpy(mv.leaf_base, m.leaf_base, sizeof mv.leaf_base);
            mv.n_leaves = m.n_leaves; mv.n_slots = m.n_slots;
            moved = true;
        } else if (!(same && s->epoch == t->held_epoch)) t->frames = 0;
    }
    if ((rc = gbuffer_device(c, s, dc, seed, t->d_rays.p, t->d_hits.p, moved ? t->d_ki.p : nullptr))) return rc;
    const zr::TemporalPlanes now = t->planes(nxt), before = t->planes(t->cur);
    HIP_OK(zr::launch_gbuffer_pack(t->d_hits.p, t->d_rays.p, t->npx(), now.pos, now.nrm, nullptr, now.mat, c->stream));
    HIP_OK(zr::launch_temporal_reproject(t->W, t->H, v, t->view, t->frames > 0, *p, d_color, d_variance, now, before, moved ? &mv : nullptr, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    t->cur = nxt; t->view = v; t->frames++;
    t->held_scene = s; t->held_serial = s->serial; t->held_epoch = s->epoch;
    if ((rc = copy_out(out_color, now.col, t->npx() * 3)) || (rc = copy_out(out_variance, now.var, t->npx() * 3)) || (rc = copy_out(out_history, now.len, t->npx()))) return rc;
    return ZR_OK;
}

}  // namespace zr_host

extern "C" {

int zr_temporal_view(const zr_camera* cam, double out[16]) {
    if (!cam || !out) return fail(ZR_E_INVALID, "null argument");
    zr::DCamera dc; zr::TemporalView v;
    camera_frame(*cam, dc); make_view(*cam, dc, v);
    std::memcpy(out, &v, sizeof v);
    return ZR_OK;
}

int zr_render_gbuffer(zr_ctx* c, const zr_scene* s, const zr_camera* cam, uint64_t seed, double* out_position, double* out_normal, double* out_t,
                      uint32_t* out_mat) {
    if (!c || !s || !cam) return fail(ZR_E_INVALID, "null argument");
    int rc = scene_ready(c, s, "zr_render_gbuffer");
    if (rc) return rc;
    if (!out_position && !out_normal && !out_t && !out_mat) return ZR_OK;
    HIP_OK(hipSetDevice(c->device));
    zr::DCamera dc;
    camera_frame(*cam, dc);
    const size_t n = (size_t)dc.W * dc.H;
    DevBuf<double> d_rays, d_pos, d_nrm, d_t; DevBuf<uint32_t> d_mat; DevBuf<zr_hit> d_hits;
    if ((rc = d_rays.alloc(n * 6)) || (rc = d_hits.alloc(n)) || (rc = d_pos.alloc(n * 3)) || (rc = d_nrm.alloc(n * 3)) || (rc = d_t.alloc(n)) || (rc = d_mat.alloc(n))) return rc;
    if ((rc = gbuffer_device(c, s, dc, seed, d_rays.p, d_hits.p))) return rc;
    HIP_OK(zr::launch_gbuffer_pack(d_hits.p, d_rays.p, n, d_pos.p, d_nrm.p, d_t.p, d_mat.p, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    if ((rc = copy_out(out_position, d_pos.p, n * 3)) || (rc = copy_out(out_normal, d_nrm.p, n * 3)) || (rc = copy_out(out_t, d_t.p, n)) || (rc = copy_out(out_mat, d_mat.p, n))) return rc;
    return ZR_OK;
}

zr_temporal* zr_temporal_create(zr_ctx* c, int width, int height) {
    if (!c) { fail(ZR_E_INVALID, "null argument"); return nullptr; }
    if (width < 1 || height < 1 || width > zr::ST_MAX_FRAME_SIDE || height > zr::ST_MAX_FRAME_SIDE) { fail(ZR_E_INVALID, "history size %d x %d not supported", width, height); return nullptr; }
    if (hipSetDevice(c->device) != hipSuccess) { fail(ZR_E_DEVICE, "hipSetDevice(%d) failed", c->device); return nullptr; }
    std::unique_ptr<zr_temporal> t(new zr_temporal);
    t->ctx = c; t->device = c->device; t->W = width; t->H = height;
    const size_t n = t->npx();
    for (auto& h : t->half)
        if (h.pos.alloc(n * 3) || h.nrm.alloc(n * 3) || h.col.alloc(n * 3) || h.var.alloc(n * 3) || h.mat.alloc(n) || h.len.alloc(n)) return nullptr;
    if (t->d_rays.alloc(n * 6) || t->d_hits.alloc(n)) return nullptr;
    return t.release();
}

void zr_temporal_destroy(zr_temporal* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    delete t;
}

int zr_temporal_reset(zr_temporal* t) {
    if (!t) return fail(ZR_E_INVALID, "null argument");
    t->frames = 0;   // the next frame reads no history: every pixel starts at length 1
    return ZR_OK;
}

int zr_temporal_track_motion(zr_temporal* t, int on) {
    if (!t) return fail(ZR_E_INVALID, "null argument");
    t->track = on != 0;
    return ZR_OK;
}

int zr_render_gbuffer_entries(zr_ctx* c, zr_scene* s, const zr_camera* cam, uint64_t seed, uint32_t* out_entry) {
    if (!c || !s || !cam) return fail(ZR_E_INVALID, "null argument");
    int rc = scene_ready(c, s, "zr_render_gbuffer_entries");
    if (rc) return rc;
    HIP_OK(hipSetDevice(c->device));
    const uint32_t* d_leaf_entry = nullptr; MotionView m;
    if ((rc = scene_leaf_entries(s, &d_leaf_entry, &m))) return rc;
    if (!out_entry) return ZR_OK;
    zr::DCamera dc;
    camera_frame(*cam, dc);
    const size_t n = (size_t)dc.W * dc.H;
    DevBuf<double> d_rays; DevBuf<zr_hit> d_hits; DevBuf<uint2> d_ki; DevBuf<uint32_t> d_out;
    if ((rc = d_rays.alloc(n * 6)) || (rc = d_hits.alloc(n)) || (rc = d_ki.alloc(n)) || (rc = d_out.alloc(n))) return rc;
    if ((rc = gbuffer_device(c, s, dc, seed, d_rays.p, d_hits.p, d_ki.p))) return rc;
    zr::TemporalMotion mv{};
    mv.ki = d_ki.p; std::memcpy(mv.leaf_base, m.leaf_base, sizeof mv.leaf_base); mv.n_leaves = m.n_leaves;
    HIP_OK(zr::launch_gbuffer_entries(mv, d_leaf_entry, n, d_out.p, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return copy_out(out_entry, d_out.p, n);
}

int zr_temporal_state(const zr_temporal* t, int64_t out[4]) {
    if (!t || !out) return fail(ZR_E_INVALID, "null argument");
    out[0] = t->W; out[1] = t->H; out[2] = t->frames; out[3] = t->track ? 1 : 0;
    return ZR_OK;
}

int zr_temporal_accumulate(zr_temporal* t, const zr_temporal_params* p, const zr_scene* s, const zr_camera* cam, uint64_t seed, const double* color,
                           const double* variance, double* out_color, double* out_variance, int32_t* out_history) {
    if (!p) return fail(ZR_E_INVALID, "null argument");
    int rc = check_temporal_params(p);   // the parameters first: they need no device and no other argument
    if (rc) return rc;
    if (!t || !s || !cam || !color || !variance) return fail(ZR_E_INVALID, "null argument");
    if ((rc = temporal_call_ready(t, t->ctx, s, cam, "zr_temporal_accumulate"))) return rc;
    HIP_OK(hipSetDevice(t->device));
    const size_t n3 = t->npx() * 3;
    if ((rc = t->d_in_color.alloc(n3)) || (rc = t->d_in_variance.alloc(n3))) return rc;
    HIP_OK(hipMemcpy(t->d_in_color.p, color, n3 * sizeof(double), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(t->d_in_variance.p, variance, n3 * sizeof(double), hipMemcpyHostToDevice));
    HIP_OK(hipDeviceSynchronize());   // the context's streams do not wait for the null stream
    return temporal_accumulate_device(t, p, s, cam, seed, t->d_in_color.p, t->d_in_variance.p, out_color, out_variance, out_history);
}

}  // extern "C"
