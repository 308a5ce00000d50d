// zr_envlight.cpp — the host side of environment-map light sampling (include/zr_capi.h): the scene's environment table (built on the device from
// the map's texels at the first use of a commit and texture, then kept), zr_render_direct_env, the table's dump, the statistics and the known-answer entries.
// The accumulator's switch (zr_accum_set_direct_env) lives in zr_accum.cpp, the batch driver that hands the table to the direct kernel in zr_direct.cpp.
#include "zr_frame.h"
#include "zr_light.h"
#include "zr_envlight.h"

namespace zr_host {

// The environment table of one (commit, texture) of a scene.  Rotation and intensity do not enter it, and a refit moves no texel.
struct EnvLightCache {
    uint64_t serial = 0; uint32_t tex = 0;
    uint32_t W = 0, H = 0;
    DevBuf<double> d_cdf, d_row_cdf, d_omega;
    std::vector<double> row_cdf;
    double total = 0; uint64_t weighted = 0;
    double build_ms = 0;
};

namespace {

// the map of an environment, where it has one that could be sampled: mode, an image texture with texels, a finite positive intensity
const zr_texture* env_map(const zr_scene* s, const zr::DEnv& de) {
    if (de.mode != ZR_ENV_HDR_MAP || de.hdr_tex == ZR_NO_TEXTURE || de.hdr_tex >= s->textures.size()) return nullptr;
    const zr_texture& t = s->textures[de.hdr_tex];
    if ((t.kind != ZR_TEX_IMAGE_F32 && t.kind != ZR_TEX_IMAGE_U8) || t.width == 0 || t.height == 0) return nullptr;
    if (!(de.intensity > 0) || !std::isfinite(de.intensity)) return nullptr;
    return &t;
}

// Builds the table: the host states each row's solid angle, the device sums the rows (zr_envlight.hip), the host sums the H row totals sequentially.
// Queued on the context's stream.
int env_cache(zr_ctx* c, const zr_scene* s, uint32_t tex, const zr_texture& t, const EnvLightCache** out) {
    if (s->env_light && s->env_light->serial == s->serial && s->env_light->tex == tex) { *out = s->env_light.get(); return ZR_OK; }
    HIP_OK(hipSetDevice(c->device));
    const uint32_t W = t.width, H = t.height;
    auto ec = std::make_shared<EnvLightCache>();
    ec->serial = s->serial; ec->tex = tex; ec->W = W; ec->H = H;
    std::vector<double> omega(H), row_total(H);
    std::vector<uint32_t> row_count(H);
    for (uint32_t j = 0; j < H; j++)
        omega[j] = (2.0 * kPi / (double)W) * (std::cos((double)j * kPi / (double)H) - std::cos((double)(j + 1) * kPi / (double)H));
    DevBuf<double> d_total; DevBuf<uint32_t> d_count;
    int rc;
    if ((rc = ec->d_omega.upload(omega)) || (rc = ec->d_cdf.alloc((size_t)W * H)) || (rc = d_total.alloc(H)) || (rc = d_count.alloc(H))) return rc;
    // the build kernel between two events, for zr_env_light_info::build_ms; both events are destroyed on every path, and the first error is the one reported
    struct Events {
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } ev;
    HIP_OK(hipEventCreate(&ev.a));
    HIP_OK(hipEventCreate(&ev.b));
    HIP_OK(hipEventRecord(ev.a, c->stream));
    HIP_OK(zr::launch_env_row_cdf(s->ds, tex, W, H, ec->d_omega.p, ec->d_cdf.p, d_total.p, d_count.p, c->stream));
    HIP_OK(hipEventRecord(ev.b, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, ev.a, ev.b));
    ec->build_ms = ms;
    HIP_OK(hipMemcpy(row_total.data(), d_total.p, (size_t)H * sizeof(double), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(row_count.data(), d_count.p, (size_t)H * sizeof(uint32_t), hipMemcpyDeviceToHost));
    ec->row_cdf.resize(H);
    double run = 0;
    for (uint32_t j = 0; j < H; j++) { run += row_total[j]; ec->row_cdf[j] = run; ec->weighted += row_count[j]; }
    ec->total = run;
    if ((rc = ec->d_row_cdf.upload(ec->row_cdf))) return rc;
    s->env_light = ec;
    *out = ec.get();
    return ZR_OK;
}

// what the entries below share once their own null tests have passed
int entry_ready(zr_ctx* c, const zr_scene* s, const zr_env* env, const char* entry, zr::DEnv& de) {
    if (!c) return fail(ZR_E_INVALID, "null argument: context");
    if (!s) return fail(ZR_E_INVALID, "null argument: scene");
    if (!env) return fail(ZR_E_INVALID, "null argument: env");
    if (int rc = scene_ready(c, s, entry)) return rc;
    HIP_OK(hipSetDevice(c->device));
    return env_frame(*env, s, de);
}

}  // namespace

int scene_env_light(zr_ctx* c, const zr_scene* s, const zr::DEnv& de, zr::EnvLight& el) {
    el = zr::EnvLight{};
    const zr_texture* t = env_map(s, de);
    if (!t) return ZR_OK;
    if ((uint64_t)t->width * t->height > ZR_DIRECT_ENV_MAX_TEXELS)
        return fail(ZR_E_INVALID, "the environment map (texture %u) has %u x %u texels: at most 2^25 (ZR_DIRECT_ENV_MAX_TEXELS) are sampled", de.hdr_tex, t->width, t->height);
    const EnvLightCache* ec = nullptr;
    if (int rc = env_cache(c, s, de.hdr_tex, *t, &ec)) return rc;
    if (!(ec->total > 0) || !std::isfinite(ec->total)) return ZR_OK;
    el.cdf = ec->d_cdf.p; el.row_cdf = ec->d_row_cdf.p; el.omega = ec->d_omega.p;
    el.W = ec->W; el.H = ec->H; el.on = 1; el.tex = de.hdr_tex;
    el.total = ec->total; el.p_choice = 1.0; el.intensity = de.intensity;
    return ZR_OK;
}

}  // namespace zr_host

extern "C" {

int zr_render_direct_env(zr_ctx* c, const zr_scene* s, const zr_camera* cam, const zr_env* env, uint64_t seed, const zr_region* region, const zr_direct_params* dp,
                         int collect_counters, double* out_rgb) {
    int rc = check_direct_params(dp);   // the parameters first: they need no device and no other argument
    if (rc) return rc;
    if (!c) return fail(ZR_E_INVALID, "null argument: context");
    if (!s) return fail(ZR_E_INVALID, "null argument: scene");
    if (!cam) return fail(ZR_E_INVALID, "null argument: camera");
    if (!env) return fail(ZR_E_INVALID, "null argument: env");
    if (!out_rgb) return fail(ZR_E_INVALID, "null argument: out_rgb");
    if ((rc = scene_ready(c, s, "zr_render_direct_env"))) return rc;
    zr_accum* a = zr_accum_create(c, cam->image_width < 1 ? 1 : cam->image_width, cam->image_height < 1 ? 1 : cam->image_height, region);
    if (!a) return ZR_E_INVALID;   // (zr_last_error holds zr_accum_create's reason)
    rc = zr_accum_set_direct(a, dp);
    if (!rc) rc = zr_accum_set_direct_env(a, 1);
    if (!rc) rc = zr_render_accumulate(c, s, cam, env, seed, a, cam->samples_per_pixel < 1 ? 1 : cam->samples_per_pixel, collect_counters, nullptr);
    if (!rc) rc = zr_accum_resolve(a, out_rgb);
    const std::string why = rc ? zr_host::last_error() : "";
    zr_accum_destroy(a);
    return rc ? fail(rc, "%s", why.c_str()) : ZR_OK;
}

int zr_scene_env_light(zr_ctx* c, const zr_scene* s, const zr_env* env, zr_env_light_info* info, double* row_cdf, double* cdf) {
    if (!info) return fail(ZR_E_INVALID, "null argument: info");
    zr::DEnv de;
    int rc = entry_ready(c, s, env, "zr_scene_env_light", de);
    if (rc) return rc;
    std::memset(info, 0, sizeof *info);
    if (de.mode == ZR_ENV_HDR_MAP && de.hdr_tex != ZR_NO_TEXTURE && de.hdr_tex < s->textures.size()) {
        const zr_texture& t = s->textures[de.hdr_tex];
        if (t.kind == ZR_TEX_IMAGE_F32 || t.kind == ZR_TEX_IMAGE_U8) { info->width = t.width; info->height = t.height; }
    }
    zr::EnvLight el;
    if ((rc = scene_env_light(c, s, de, el))) return rc;
    if (!el.on) return ZR_OK;
    const EnvLightCache& ec = *s->env_light;
    info->sampled = 1; info->total = ec.total; info->weighted = ec.weighted; info->build_ms = ec.build_ms;
    if (row_cdf) std::memcpy(row_cdf, ec.row_cdf.data(), (size_t)ec.H * sizeof(double));
    if (cdf) HIP_OK(hipMemcpy(cdf, ec.d_cdf.p, (size_t)ec.W * ec.H * sizeof(double), hipMemcpyDeviceToHost));
    return ZR_OK;
}

int zr_kat_env_light_sample(zr_ctx* c, const zr_scene* s, const zr_env* env, const zr_direct_params* dp, const double* origins3, const uint64_t* keys,
                            const uint32_t* bounces, const double* draws8, size_t n, zr_light_sample* out) {
    if (n && !origins3) return fail(ZR_E_INVALID, "null argument: origins");
    if (n && !keys) return fail(ZR_E_INVALID, "null argument: keys");
    if (n && !bounces) return fail(ZR_E_INVALID, "null argument: bounces");
    if (n && !out) return fail(ZR_E_INVALID, "null argument: out");
    int rc = check_direct_params(dp);
    if (rc) return rc;
    if (n > 0x7FFFFFFFu) return fail(ZR_E_INVALID, "n = %zu beyond 2^31", n);
    zr::DEnv de;
    if ((rc = entry_ready(c, s, env, "zr_kat_env_light_sample", de))) return rc;
    zr::LightTable lt; zr::EnvLight el;
    if ((rc = direct_tables(c, s, 0x80000000u | dp->flags | kDirectEnv, de, lt, el, nullptr, nullptr)) || n == 0) return rc;
    DevBuf<double> d_o, d_f; DevBuf<uint64_t> d_k; DevBuf<uint32_t> d_b; DevBuf<zr_light_sample> d_out;
    if ((rc = d_o.upload(origins3, n * 3)) || (rc = d_k.upload(keys, n)) || (rc = d_b.upload(bounces, n)) || (draws8 && (rc = d_f.upload(draws8, n * 8))) ||
        (rc = d_out.alloc(n))) return rc;
    HIP_OK(zr::launch_kat_env_light_sample(s->ds, de, lt, el, d_o.p, d_k.p, d_b.p, draws8 ? d_f.p : nullptr, n, d_out.p, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    HIP_OK(hipMemcpy(out, d_out.p, n * sizeof(zr_light_sample), hipMemcpyDeviceToHost));
    return ZR_OK;
}

int zr_kat_env_light_pdf(zr_ctx* c, const zr_scene* s, const zr_env* env, const zr_direct_params* dp, const double* dirs3, size_t n, double* out_pdf) {
    if (n && !dirs3) return fail(ZR_E_INVALID, "null argument: dirs");
    if (n && !out_pdf) return fail(ZR_E_INVALID, "null argument: out_pdf");
    int rc = check_direct_params(dp);
    if (rc) return rc;
    if (n > 0x7FFFFFFFu) return fail(ZR_E_INVALID, "n = %zu beyond 2^31", n);
    zr::DEnv de;
    if ((rc = entry_ready(c, s, env, "zr_kat_env_light_pdf", de))) return rc;
    zr::LightTable lt; zr::EnvLight el;
    if ((rc = direct_tables(c, s, 0x80000000u | dp->flags | kDirectEnv, de, lt, el, nullptr, nullptr)) || n == 0) return rc;
    DevBuf<double> d_d, d_p;
    if ((rc = d_d.upload(dirs3, n * 3)) || (rc = d_p.alloc(n))) return rc;
    HIP_OK(zr::launch_kat_env_light_pdf(s->ds, de, el, d_d.p, n, d_p.p, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    HIP_OK(hipMemcpy(out_pdf, d_p.p, n * sizeof(double), hipMemcpyDeviceToHost));
    return ZR_OK;
}

int zr_get_direct_env_stats(zr_ctx* c, uint64_t* env_queries, uint64_t* env_visible) {
    if (!c) return fail(ZR_E_INVALID, "null argument: context");
    if (!env_queries) return fail(ZR_E_INVALID, "null argument: env_queries");
    if (!env_visible) return fail(ZR_E_INVALID, "null argument: env_visible");
    *env_queries = 0; *env_visible = 0;
    if (c->direct_render == 0 || c->direct_render != c->render_id || !c->last_counted) return ZR_OK;   // the counter block holds another render's words
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(hipStreamSynchronize(c->last_stream));
    unsigned long long h[2] = {0, 0};
    static_assert(zr::CTR_DIRECT_ENV_VISIBLE == zr::CTR_DIRECT_ENV + 1, "read as a run of two");
    HIP_OK(hipMemcpy(h, c->d_ctr.p + zr::CTR_DIRECT_ENV, sizeof h, hipMemcpyDeviceToHost));
    *env_queries = h[0]; *env_visible = h[1];
    return ZR_OK;
}

}  // extern "C"
