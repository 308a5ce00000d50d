// zr_direct.cpp — the host side of direct light sampling (include/zr_capi.h): the scene's light table (built on the device from the final primitive
// arrays at the first direct render of a commit and refit epoch, then kept), the batch driver render_batch_samples hands a direct accumulator's batches to,
// zr_render_direct, the statistics and the known-answer entries.  The accumulator's own entries (zr_accum_set_direct / _get_direct) live in zr_accum.cpp.
#include "zr_frame.h"
#include "zr_light.h"
#include "zr_envlight.h"

namespace zr_host {

// The light table of one (commit, epoch) of a scene: the slots that are sampled, in table order, with their running sum, on both sides
struct LightCache {
    uint64_t serial = 0, epoch = 0;
    std::vector<zr_light_slot> slots;
    DevBuf<zr_light_slot> d_slots; DevBuf<double> d_cdf;
    double total = 0; uint64_t objects = 0;
};

namespace {

// Collects the table: the device marks and compacts the emissive records (zr_direct.hip), the host drops the slots that are not sampled and makes the running
// sum — sequentially in FP64, so that a NumPy cumsum reproduces it.  Queued on the context's stream, behind any refit.
int scene_lights(zr_ctx* c, const zr_scene* s, const LightCache** out) {
    if (s->lights && s->lights->serial == s->serial && s->lights->epoch == s->epoch) { *out = s->lights.get(); return ZR_OK; }
    HIP_OK(hipSetDevice(c->device));
    const uint64_t n_cand64 = (uint64_t)s->plan_cnt[ZR_PRIM_SPHERE] + s->plan_cnt[ZR_PRIM_TRIANGLE] + s->plan_cnt[ZR_PRIM_CUBE] + s->plan_cnt[ZR_KIND_PCUBE];
    if (n_cand64 > 0xFFFFFF00ull) return fail(ZR_E_INVALID, "too many primitives for a light table (%llu)", (unsigned long long)n_cand64);
    const uint32_t n_cand = (uint32_t)n_cand64, n_blocks = (n_cand + ZR_BLOCK - 1) / ZR_BLOCK;
    auto lc = std::make_shared<LightCache>();
    lc->serial = s->serial; lc->epoch = s->epoch;
    DevBuf<uint32_t> d_blocks, d_total; DevBuf<zr_light_slot> d_raw;
    int rc;
    if ((rc = d_blocks.alloc(std::max<size_t>(n_blocks, 1))) || (rc = d_total.alloc(1))) return rc;
    HIP_OK(zr::launch_light_count(s->ds, n_cand, d_blocks.p, d_total.p, c->stream));
    uint32_t raw = 0;
    HIP_OK(hipMemcpyAsync(&raw, d_total.p, sizeof raw, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    if (raw == 0xFFFFFFFFu) return fail(ZR_E_INVALID, "the scene's emitters make more than 2^32 slots: at most %u are sampled", ZR_DIRECT_MAX_SLOTS);
    std::vector<zr_light_slot> h(raw);
    if (raw) {
        if ((rc = d_raw.alloc(raw))) return rc;
        HIP_OK(zr::launch_light_emit(s->ds, n_cand, d_blocks.p, raw, d_raw.p, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        HIP_OK(hipMemcpy(h.data(), d_raw.p, (size_t)raw * sizeof(zr_light_slot), hipMemcpyDeviceToHost));
    }
    double run = 0;
    uint64_t last_key = ~0ull;
    for (const zr_light_slot& q : h) {
        if (!(q.weight > 0) || !std::isfinite(q.weight)) continue;
        zr_light_slot k = q;
        run += q.weight; k.cdf = run;
        lc->slots.push_back(k);
        const uint64_t key = ((uint64_t)q.kind << 32) | q.index;
        if (key != last_key) { lc->objects++; last_key = key; }
    }
    if (lc->slots.size() > ZR_DIRECT_MAX_SLOTS) return fail(ZR_E_INVALID, "the scene's emitters make %zu slots: at most %u (ZR_DIRECT_MAX_SLOTS) are sampled", lc->slots.size(), ZR_DIRECT_MAX_SLOTS);
    if (!std::isfinite(run)) { lc->slots.clear(); lc->objects = 0; run = 0; }   // (weights that are finite one by one and overflow together: nothing is sampled)
    lc->total = run;
    std::vector<double> cdf(lc->slots.size());
    for (size_t k = 0; k < cdf.size(); k++) cdf[k] = lc->slots[k].cdf;
    if ((rc = lc->d_slots.upload(lc->slots)) || (rc = lc->d_cdf.upload(cdf))) return rc;
    s->lights = lc;
    *out = lc.get();
    return ZR_OK;
}

// the kernels' view of the table for one render: what `flags` asks for of what the scene and the environment have
zr::LightTable make_light_table(const LightCache& lc, uint32_t flags, const zr::DEnv& de) {
    zr::LightTable lt{};
    lt.slots = lc.d_slots.p; lt.cdf = lc.d_cdf.p;
    lt.n = (flags & ZR_DIRECT_EMITTERS) ? (uint32_t)lc.slots.size() : 0u;
    lt.total = lc.total;
    const H3 sun = h3(de.sun);
    const bool has_sun = (flags & ZR_DIRECT_SUN) && de.mode == ZR_ENV_PHYSICAL_SUN && de.sun_on && de.sun_thr < 1.0 && len(sun) > 0.5;
    lt.sun = has_sun ? 1u : 0u;
    lt.p_choice = lt.n && has_sun ? 0.5 : 1.0;
    if (has_sun) {
        const H3 a = std::fabs(sun.x) > 0.9 ? H3{0, 1, 0} : H3{1, 0, 0};
        const H3 t = unit(cross(a, sun)), b = cross(sun, t);
        st3(lt.sun_dir, sun); st3(lt.sun_t, t); st3(lt.sun_b, b);
        lt.sun_thr = de.sun_thr;
        lt.sun_pdf = 1.0 / (2.0 * kPi * (1.0 - de.sun_thr));
    }
    return lt;
}

// what the two known-answer entries share once their own null tests have passed
int kat_ready(zr_ctx* c, const zr_scene* s, const zr_env* env, const zr_direct_params* dp, size_t n, const char* entry, zr::LightTable& lt) {
    int rc = check_direct_params(dp);
    if (rc) return rc;
    if (!c) return fail(ZR_E_INVALID, "null argument: context");
    if (!s) return fail(ZR_E_INVALID, "null argument: scene");
    if (!env) return fail(ZR_E_INVALID, "null argument: env");
    if (n > 0x7FFFFFFFu) return fail(ZR_E_INVALID, "n = %zu beyond 2^31", n);
    if ((rc = scene_ready(c, s, entry))) return rc;
    HIP_OK(hipSetDevice(c->device));
    zr::DEnv de;
    if ((rc = env_frame(*env, s, de))) return rc;
    const LightCache* lc = nullptr;
    if ((rc = scene_lights(c, s, &lc))) return rc;
    lt = make_light_table(*lc, dp->flags, de);
    return ZR_OK;
}

}  // namespace

int direct_tables(zr_ctx* c, const zr_scene* s, uint32_t direct, const zr::DEnv& de, zr::LightTable& lt, zr::EnvLight& el, uint64_t* slots, uint64_t* objects) {
    const LightCache* lc = nullptr;
    if (int rc = scene_lights(c, s, &lc)) return rc;
    lt = make_light_table(*lc, direct & (ZR_DIRECT_EMITTERS | ZR_DIRECT_SUN), de);
    el = zr::EnvLight{};
    if (direct & kDirectEnv) {
        if (int rc = scene_env_light(c, s, de, el)) return rc;
        if (el.on) { el.p_choice = lt.n ? 0.5 : 1.0; lt.p_choice = el.p_choice; }   // (a map and the sun are different modes: lt.sun is 0 here)
    }
    if (slots) *slots = lc->slots.size();
    if (objects) *objects = lc->objects;
    return ZR_OK;
}

int check_direct_params(const zr_direct_params* dp) {
    if (!dp) return fail(ZR_E_INVALID, "null argument: params");
    if (dp->flags & ~(ZR_DIRECT_EMITTERS | ZR_DIRECT_SUN)) return fail(ZR_E_INVALID, "params.flags = 0x%x holds bits outside ZR_DIRECT_EMITTERS | ZR_DIRECT_SUN", dp->flags);
    return ZR_OK;
}

int render_direct_samples(zr_ctx* c, const zr_scene* s, FrameJob& job, const uint32_t* pixels, uint32_t n_pix, int sample0, int n, HostTimer& timer) {
    const uint64_t units = (uint64_t)n_pix * (uint64_t)n;
    if (units > (1ull << 37)) return fail(ZR_E_NOMEM, "a batch of %d samples is %llu samples of radiance: ask for fewer", n, (unsigned long long)units);
    zr::LightTable lt; zr::EnvLight el;
    uint64_t slots = 0, objects = 0;
    if (int rc = direct_tables(c, s, job.direct, job.de, lt, el, &slots, &objects)) return rc;
    if (c->d_partial.n < units * 3) {
        HIP_OK(hipStreamSynchronize(job.stream));
        if (c->d_partial.alloc(units * 3) != ZR_OK) return fail(ZR_E_NOMEM, "no device memory for the per-sample radiance buffer (%zu bytes): ask for fewer samples", (size_t)units * 3 * sizeof(double));
    }
    c->last_path = 0;
    if (c->pending.size() > 4096) { int rr = resolve_times(c); if (rr) return rr; }
    c->render_id++; c->last_stream = job.stream; c->last_counted = job.count;
    c->direct_slots = slots; c->direct_objects = objects; c->direct_render = c->render_id;
    timer.begin(job.stream, 1);
    HIP_OK(zr::launch_direct_samples(s->ds, job.dc, job.de, lt, el, job.seed, pixels, n_pix, (uint32_t)sample0, (uint32_t)n, c->d_partial.p, c->d_ctr.p, job.count, job.stream));
    timer.end(job.stream, 1);
    if (job.keep_going) {
        HIP_OK(hipStreamSynchronize(job.stream));
        if (*job.keep_going == 0) return fail(ZR_E_CANCELLED, "batch cancelled");
    }
    return ZR_OK;
}

}  // namespace zr_host

extern "C" {

int zr_render_direct(zr_ctx* c, const zr_scene* s, const zr_camera* cam, const zr_env* env, uint64_t seed, const zr_region* region, const zr_direct_params* dp,
                     int collect_counters, double* out_rgb) {
    int rc = check_direct_params(dp);   // the parameters first: they need no device and no other argument
    if (rc) return rc;
    if (!c) return fail(ZR_E_INVALID, "null argument: context");
    if (!s) return fail(ZR_E_INVALID, "null argument: scene");
    if (!cam) return fail(ZR_E_INVALID, "null argument: camera");
    if (!env) return fail(ZR_E_INVALID, "null argument: env");
    if (!out_rgb) return fail(ZR_E_INVALID, "null argument: out_rgb");
    if ((rc = scene_ready(c, s, "zr_render_direct"))) return rc;
    zr_accum* a = zr_accum_create(c, cam->image_width < 1 ? 1 : cam->image_width, cam->image_height < 1 ? 1 : cam->image_height, region);
    if (!a) return ZR_E_INVALID;   // (zr_last_error holds zr_accum_create's reason)
    rc = zr_accum_set_direct(a, dp);
    if (!rc) rc = zr_render_accumulate(c, s, cam, env, seed, a, cam->samples_per_pixel < 1 ? 1 : cam->samples_per_pixel, collect_counters, nullptr);
    if (!rc) rc = zr_accum_resolve(a, out_rgb);
    const std::string why = rc ? zr_host::last_error() : "";
    zr_accum_destroy(a);
    return rc ? fail(rc, "%s", why.c_str()) : ZR_OK;
}

int zr_get_direct_stats(zr_ctx* c, zr_direct_stats* out) {
    if (!c) return fail(ZR_E_INVALID, "null argument: context");
    if (!out) return fail(ZR_E_INVALID, "null argument: out");
    std::memset(out, 0, sizeof *out);
    out->slots = c->direct_slots; out->sampled_objects = c->direct_objects;
    if (c->direct_render == 0 || c->direct_render != c->render_id || !c->last_counted) return ZR_OK;   // the counter block holds another render's words
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(hipStreamSynchronize(c->last_stream));
    unsigned long long h[3] = {0, 0, 0};
    static_assert(zr::CTR_DIRECT_VISIBLE == zr::CTR_DIRECT_SHADOW + 1 && zr::CTR_DIRECT_SUN == zr::CTR_DIRECT_SHADOW + 2, "read as a run of three");
    HIP_OK(hipMemcpy(h, c->d_ctr.p + zr::CTR_DIRECT_SHADOW, sizeof h, hipMemcpyDeviceToHost));
    out->shadow_queries = h[0]; out->shadow_visible = h[1]; out->sun_queries = h[2];
    return ZR_OK;
}

int64_t zr_scene_lights(zr_ctx* c, const zr_scene* s, zr_light_slot* out, size_t cap) {
    if (!c) return fail(ZR_E_INVALID, "null argument: context");
    if (!s) return fail(ZR_E_INVALID, "null argument: scene");
    if (!out && cap != 0) return fail(ZR_E_INVALID, "null argument: out");
    if (int rc = scene_ready(c, s, "zr_scene_lights")) return rc;
    const LightCache* lc = nullptr;
    if (int rc = scene_lights(c, s, &lc)) return rc;
    const size_t n = std::min(cap, lc->slots.size());
    if (n) std::memcpy(out, lc->slots.data(), n * sizeof(zr_light_slot));
    return (int64_t)lc->slots.size();
}

int zr_kat_light_sample(zr_ctx* c, const zr_scene* s, const zr_env* env, const zr_direct_params* dp, const double* origins3, const uint64_t* keys,
                        const uint32_t* bounces, const double* draws8, size_t n, zr_light_sample* out) {
    if (n && !origins3) return fail(ZR_E_INVALID, "null argument: origins");
    if (n && !keys) return fail(ZR_E_INVALID, "null argument: keys");
    if (n && !bounces) return fail(ZR_E_INVALID, "null argument: bounces");
    if (n && !out) return fail(ZR_E_INVALID, "null argument: out");
    zr::LightTable lt;
    int rc = kat_ready(c, s, env, dp, n, "zr_kat_light_sample", lt);
    if (rc || n == 0) return rc;
    DevBuf<double> d_o, d_f; DevBuf<uint64_t> d_k; DevBuf<uint32_t> d_b; DevBuf<zr_light_sample> d_out;
    if ((rc = d_o.upload(origins3, n * 3)) || (rc = d_k.upload(keys, n)) || (rc = d_b.upload(bounces, n)) || (draws8 && (rc = d_f.upload(draws8, n * 8))) ||
        (rc = d_out.alloc(n))) return rc;
    HIP_OK(zr::launch_kat_light_sample(lt, d_o.p, d_k.p, d_b.p, draws8 ? d_f.p : nullptr, n, d_out.p, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    HIP_OK(hipMemcpy(out, d_out.p, n * sizeof(zr_light_sample), hipMemcpyDeviceToHost));
    return ZR_OK;
}

int zr_kat_light_pdf(zr_ctx* c, const zr_scene* s, const zr_env* env, const zr_direct_params* dp, const double* origins3, const double* dirs3, size_t n,
                     double* out_pdf, uint64_t* out_key) {
    if (n && !origins3) return fail(ZR_E_INVALID, "null argument: origins");
    if (n && !dirs3) return fail(ZR_E_INVALID, "null argument: dirs");
    if (n && !out_pdf) return fail(ZR_E_INVALID, "null argument: out_pdf");
    if (n && !out_key) return fail(ZR_E_INVALID, "null argument: out_key");
    zr::LightTable lt;
    int rc = kat_ready(c, s, env, dp, n, "zr_kat_light_pdf", lt);
    if (rc || n == 0) return rc;
    DevBuf<double> d_o, d_d, d_p; DevBuf<uint64_t> d_k;
    if ((rc = d_o.upload(origins3, n * 3)) || (rc = d_d.upload(dirs3, n * 3)) || (rc = d_p.alloc(n)) || (rc = d_k.alloc(n))) return rc;
    HIP_OK(zr::launch_kat_light_pdf(s->ds, lt, d_o.p, d_d.p, n, d_p.p, d_k.p, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    HIP_OK(hipMemcpy(out_pdf, d_p.p, n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out_key, d_k.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return ZR_OK;
}

}  // extern "C"
