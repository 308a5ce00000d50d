// zr_scenes_lib.cpp — libzr_scenes.so: the BASELINE.json scenes (scenes/zr_scenes.inc, the very file the
// oracle harness compiles against the genuine reference headers) compiled against the drop-in API
// (include/zenith/zenith.hpp).  Exposes (a) the flattened arrays, so that Python hosts (bench.py, tests)
// can feed them to the C ABI, and (b) a render through the drop-in's camera::render(world, env, post, flag),
// the same call the reference's main.cpp:1520-1521 makes.
#include <unistd.h>

#include <thread>

#include "../../include/zenith/zenith.hpp"

static void zr_hook_seed_scene(uint64_t seed, uint64_t stream) { zenith::seed_rng(seed, ZR_SCENE_PIXEL, stream); }
static shared_ptr<hittable> zr_hook_medium(shared_ptr<hittable> m) { return m; }  // media ids = flatten order

#include "../../scenes/zr_scenes.inc"
#include "../../scenes/zr_scenes_mix.inc"

namespace {
struct handle {
    zr_demo_scene s;
    zenith::flat_scene fs;
    zr_scene_desc desc{};
    zr_env env{};
    std::string warnings;
    std::vector<uint32_t> kat_tex;   // flattened ids of zr_demo_scene::kat_textures
};

// The scene's camera as a drop-in `camera` (which cannot be copied or moved: it holds an atomic, so this is a constructor and not a function that
// returns one).  spp/width/height <= 0 keep the scene's values.  reset_accumulator() is left to the caller, who sets the camera's flags first.
struct scene_camera : camera {
    scene_camera(const handle& h, int width, int height, int spp, int device) {
        const zr_camera& c = h.s.cam;
        image_width = width > 0 ? width : c.image_width;
        image_height = height > 0 ? height : c.image_height;
        samples_per_pixel = spp > 0 ? spp : c.samples_per_pixel;
        max_depth = c.max_depth; vfov = c.vfov;
        lookfrom = point3(c.lookfrom[0], c.lookfrom[1], c.lookfrom[2]);
        lookat = point3(c.lookat[0], c.lookat[1], c.lookat[2]);
        vup = vec3(c.vup[0], c.vup[1], c.vup[2]);
        defocus_angle = c.defocus_angle; focus_dist = c.focus_dist;
        seed = h.s.seed; this->device = device;
    }
};

// camera::render over bvh_node(world) as the reference's caller makes it (main.cpp:204, 1520-1521), with render_flag = flag0 going in: whether the frame finished
bool render_world(const handle& h, camera& cam, const post_processor& post, bool flag0 = true) {
    std::atomic<bool> flag{flag0};
    auto bvh_world = make_shared<bvh_node>(h.s.world);
    cam.render(*bvh_world, h.s.env, post, flag);
    return cam.lines_rendered.load() == cam.image_height;
}

void copy_out(const std::vector<color>& frame, double* out) {
    if (out) std::memcpy(out, frame.data(), frame.size() * sizeof(color));
}
}  // namespace

extern "C" {

void* zrs_build(const char* name, int a0, int a1, int a2, int a3) {
    handle* h = new handle();
    bool ok = zr_build_scene(name, h->s, a0, a1, a2, a3) || zr_build_scene_mix(name, h->s, a0);
    if (!ok) { delete h; return nullptr; }
    zenith::scene_builder b(h->fs);
    h->s.world.flatten(b);
    b.finish();
    h->env = zenith::to_zr_env(h->s.env, b);
    for (const auto& t : h->s.kat_textures) h->kat_tex.push_back(b.texture_id(t));
    h->desc = h->fs.desc();
    for (const auto& w : h->fs.warnings) { h->warnings += w; h->warnings += "\n"; }
    for (const auto& f : h->s.temp_files) ::unlink(f.c_str());
    h->s.temp_files.clear();
    return h;
}
void zrs_free(void* p) { delete (handle*)p; }
const zr_scene_desc* zrs_desc(void* p) { return &((handle*)p)->desc; }
const zr_camera* zrs_camera(void* p) { return &((handle*)p)->s.cam; }
const zr_env* zrs_env(void* p) { return &((handle*)p)->env; }
uint64_t zrs_seed(void* p) { return ((handle*)p)->s.seed; }
const char* zrs_warnings(void* p) { return ((handle*)p)->warnings.c_str(); }
int zrs_kat_textures(void* p, uint32_t* ids, int cap) {
    const handle* h = (const handle*)p;
    for (int k = 0; k < cap && k < (int)h->kat_tex.size(); k++) ids[k] = h->kat_tex[k];
    return (int)h->kat_tex.size();
}

// Renders through the drop-in C++ API exactly as the reference's caller does.  out = W*H*3 doubles.
// spp/width/height <= 0 keep the scene's values.  Returns 0, or -1 if the accumulator stayed empty.
int zrs_render_dropin(void* p, int width, int height, int spp, int device, double* out, zr_counters* ctr) {
    const handle& h = *(handle*)p;
    scene_camera cam(h, width, height, spp, device);
    cam.reset_accumulator();
    if (!render_world(h, cam, post_processor())) return -1;
    copy_out(cam.render_accumulator, out);
    if (ctr) *ctr = cam.last_counters;
    return 0;
}

// camera::render with camera::samples_per_pass set (the progressive render of include/zenith/zenith.hpp) and render_flag = flag0 going in.  info[0] =
// current_samples_count after the render, info[1] = the number of times render_accumulator was refreshed.  current_samples_count holds -7 when render() is
// called, so a render that leaves it alone (samples_per_pass = 0) reports -7.  Returns 0, or -1 if the render did not finish; `out` and `info` are filled either way.
int zrs_render_dropin_progressive(void* p, int width, int height, int spp, int device, int samples_per_pass, double* out, int* info, int flag0) {
    const handle& h = *(handle*)p;
    scene_camera cam(h, width, height, spp, device);
    cam.reset_accumulator();
    cam.samples_per_pass = samples_per_pass;
    cam.current_samples_count = -7;
    const bool done = render_world(h, cam, post_processor(), flag0 != 0);
    if (info) { info[0] = cam.current_samples_count; info[1] = cam.passes_rendered; }
    copy_out(cam.render_accumulator, out);
    return done ? 0 : -1;
}

// camera::render with camera::direct_lighting = on; split != 0 also sets use_reflection, with which the flag is ignored; samples_per_pass as above.
// info[0] = render_used_direct, info[1] = passes.  Returns 0, or -1 if the accumulator stayed empty.
int zrs_render_dropin_direct(void* p, int width, int height, int spp, int device, int on, int split, int samples_per_pass, double* out, int* info) {
    const handle& h = *(handle*)p;
    scene_camera cam(h, width, height, spp, device);
    cam.reset_accumulator();
    cam.direct_lighting = on != 0;
    cam.use_reflection = split != 0;
    cam.samples_per_pass = samples_per_pass;
    const bool done = render_world(h, cam, post_processor());
    if (info) { info[0] = cam.render_used_direct ? 1 : 0; info[1] = cam.passes_rendered; }
    copy_out(cam.render_accumulator, out);
    return done ? 0 : -1;
}

// ... and with camera::direct_environment = env beside camera::direct_lighting = on.  info[0] = render_used_direct, info[1] = passes,
// info[2] = render_used_direct_env.
int zrs_render_dropin_direct_env(void* p, int width, int height, int spp, int device, int on, int env, int samples_per_pass, double* out, int* info) {
    const handle& h = *(handle*)p;
    scene_camera cam(h, width, height, spp, device);
    cam.reset_accumulator();
    cam.direct_lighting = on != 0;
    cam.direct_environment = env != 0;
    cam.samples_per_pass = samples_per_pass;
    const bool done = render_world(h, cam, post_processor());
    if (info) { info[0] = cam.render_used_direct ? 1 : 0; info[1] = cam.passes_rendered; info[2] = cam.render_used_direct_env ? 1 : 0; }
    copy_out(cam.render_accumulator, out);
    return done ? 0 : -1;
}

// camera::render with camera::adaptive_threshold set (min_samples and step <= 0 keep the camera's defaults) and render_flag = flag0 going in.  counts = W*H ints
// (camera::sample_counts; left alone when the render left it empty), info[0] = current_samples_count after the render (-7 going in), info[1] = passes.  Returns 0,
// or -1 if the render did not finish; `out`, `counts` and `info` are filled either way.
int zrs_render_dropin_adaptive(void* p, int width, int height, int spp, int device, double threshold, int min_samples, int step, double* out, int* counts, int* info,
                               int flag0) {
    const handle& h = *(handle*)p;
    scene_camera cam(h, width, height, spp, device);
    cam.reset_accumulator();
    cam.adaptive_threshold = threshold;
    if (min_samples > 0) cam.adaptive_min_samples = min_samples;
    if (step > 0) cam.adaptive_step = step;
    cam.current_samples_count = -7;
    const bool done = render_world(h, cam, post_processor(), flag0 != 0);
    if (info) { info[0] = cam.current_samples_count; info[1] = cam.passes_rendered; }
    copy_out(cam.render_accumulator, out);
    if (counts && !cam.sample_counts.empty()) std::memcpy(counts, cam.sample_counts.data(), cam.sample_counts.size() * sizeof(int));
    return done ? 0 : -1;
}

// camera::render with camera::robust_resolve (flags & 1) and robust_strength = strength (< 0 keeps the camera's default) through the drop-in API: adaptively when
// threshold > 0 (min_samples and step <= 0 keep the camera's defaults), progressively when samples_per_pass > 0, else as the flag decides.  flags & 2: use_denoiser and
// denoise_variance_guided, so that variance_buffer is filled; flags & 4: temporal_accumulation (one frame: the history is the camera's, and the camera ends here).
// Outputs (any may be null): render_accumulator, variance_buffer, temporal_buffer (W*H*3 doubles each; the last two all -1 when the render left them empty), counts
// (W*H ints, camera::sample_counts; left alone when empty); info: resolve_used_robust, current_samples_count (-7 going in), passes_rendered.  Returns 0, or -1 if
// the render did not finish.
int zrs_render_dropin_robust(void* p, int width, int height, int spp, int device, double strength, double threshold, int min_samples, int step, int samples_per_pass,
                             int flags, double* out, double* var, double* temporal, int* counts, int* info) {
    const handle& h = *(handle*)p;
    scene_camera cam(h, width, height, spp, device);
    cam.robust_resolve = (flags & 1) != 0;
    if (strength >= 0) cam.robust_strength = strength;
    cam.use_denoiser = cam.denoise_variance_guided = (flags & 2) != 0;
    cam.temporal_accumulation = (flags & 4) != 0;
    cam.adaptive_threshold = threshold;
    if (min_samples > 0) cam.adaptive_min_samples = min_samples;
    if (step > 0) cam.adaptive_step = step;
    cam.samples_per_pass = samples_per_pass;
    cam.reset_accumulator();
    cam.current_samples_count = -7;
    if (!render_world(h, cam, post_processor())) return -1;
    copy_out(cam.render_accumulator, out);
    if (cam.variance_buffer.size() == cam.render_accumulator.size()) copy_out(cam.variance_buffer, var);
    else if (var) std::fill(var, var + cam.render_accumulator.size() * 3, -1.0);
    if (cam.temporal_buffer.size() == cam.render_accumulator.size()) copy_out(cam.temporal_buffer, temporal);
    else if (temporal) std::fill(temporal, temporal + cam.render_accumulator.size() * 3, -1.0);
    if (counts && !cam.sample_counts.empty()) std::memcpy(counts, cam.sample_counts.data(), cam.sample_counts.size() * sizeof(int));
    if (info) { info[0] = cam.resolve_used_robust ? 1 : 0; info[1] = cam.current_samples_count; info[2] = cam.passes_rendered; }
    return 0;
}

// camera::render with global_settings::bvh_debug_mode set (debug_bvh_level = level, bvh_thickness = thickness) through the drop-in API; the
// settings are restored afterwards.  `aux`, when not null, receives albedo_buffer (which the debug view leaves as reset_accumulator made it).
// Returns 0, or -1 if the render did not finish.
int zrs_render_dropin_bvh_debug(void* p, int width, int height, int spp, int device, int level, float thickness, double* out, double* aux) {
    const handle& h = *(handle*)p;
    scene_camera cam(h, width, height, spp, device);
    cam.use_albedo_buffer = aux != nullptr;
    cam.reset_accumulator();
    post_processor post;
    post.debug.bvh = true;   // main.cpp:1039-1044
    const bool m0 = global_settings::bvh_debug_mode; const float t0 = global_settings::bvh_thickness; const int l0 = global_settings::debug_bvh_level;
    global_settings::bvh_debug_mode = true; global_settings::bvh_thickness = thickness; global_settings::debug_bvh_level = level;
    const bool done = render_world(h, cam, post);
    global_settings::bvh_debug_mode = m0; global_settings::bvh_thickness = t0; global_settings::debug_bvh_level = l0;
    if (!done) return -1;
    copy_out(cam.render_accumulator, out);
    copy_out(cam.albedo_buffer, aux);
    return 0;
}

// The reference starts a fresh thread for every render (main.cpp:1520-1531): `n` renders of the scene, each on a thread of its own,
// one after the other.  Returns the number of device contexts the process has created so far (the drop-in keeps them in a
// process-wide pool: successive threads share one), or -1 if a render failed; `out` receives the last frame.
int zrs_render_dropin_threads(void* p, int width, int height, int spp, int device, int n, double* out) {
    int rc = 0;
    for (int k = 0; k < n && rc == 0; k++) {
        std::thread t([&]() { rc = zrs_render_dropin(p, width, height, spp, device, out, nullptr); });
        t.join();
    }
    return rc == 0 ? (int)zenith::contexts_created() : -1;
}

// The reference's whole frame pipeline through the drop-in API: render with auto-exposure and the reflection / refraction
// split, then the beauty image through the post stack (bloom + sharpening + ACES) and the reflection frame as a data pass —
// what main.cpp's render thread followed by save_render_pass(RGB) / save_render_pass(REFLECTIONS) does.
// rgb8 / refl8: W*H*3 bytes each; exposure_out: the auto-exposure value written back to post.exposure (camera.hpp:258-266)
int zrs_dropin_frame_to_rgb8(void* p, int spp, int device, unsigned char* rgb8, unsigned char* refl8, float* exposure_out) {
    const handle& h = *(handle*)p;
    scene_camera cam(h, 0, 0, spp, device);
    cam.use_reflection = true;
    cam.reset_accumulator();
    post_processor post;
    post.use_auto_exposure = true; post.exposure_compensation_stops = 0.5f;
    post.use_bloom = true; post.bloom_threshold = 0.8f; post.use_sharpening = true; post.use_aces_tone_mapping = true;
    if (!render_world(h, cam, post)) return -1;
    std::vector<unsigned char> a, b;
    if (!cam.process_framebuffer(cam.render_accumulator, post, a) || !cam.process_framebuffer(cam.reflection_buffer, post, b, true, true)) return -2;
    std::memcpy(rgb8, a.data(), a.size());
    std::memcpy(refl8, b.data(), b.size());
    if (exposure_out) *exposure_out = post.exposure;
    return 0;
}

// camera::render with use_denoiser set (camera.hpp:268-291) through the drop-in API.  flags: 1 = use_reflection and use_refraction,
// 2 = post.use_sharpening (sharpen_amount 0.2).  The public albedo / normal buffers stay off, so the denoiser's guides are the drop-in's
// private ones.  Outputs (W*H*3 doubles each, any may be null): render_accumulator, denoise_buffer, reflection_buffer,
// refraction_buffer, albedo_buffer, normal_buffer.  spp/width/height <= 0 keep the scene's values.  Returns 0, or -1 if the
// render did not finish.
int zrs_render_dropin_denoise(void* p, int width, int height, int spp, int device, int flags, double* acc, double* den, double* refl, double* refr,
                              double* alb, double* nrm) {
    const handle& h = *(handle*)p;
    scene_camera cam(h, width, height, spp, device);
    cam.use_denoiser = true;
    cam.use_reflection = cam.use_refraction = (flags & 1) != 0;
    cam.reset_accumulator();
    post_processor post;
    post.use_sharpening = (flags & 2) != 0;
    if (!render_world(h, cam, post)) return -1;
    copy_out(cam.render_accumulator, acc); copy_out(cam.denoise_buffer, den);
    copy_out(cam.reflection_buffer, refl); copy_out(cam.refraction_buffer, refr);
    copy_out(cam.albedo_buffer, alb); copy_out(cam.normal_buffer, nrm);
    return 0;
}

// camera::render with use_denoiser and camera::denoise_variance_guided (`guided` != 0) through the drop-in API: adaptively when threshold > 0
// (min = step = 64), progressively when samples_per_pass > 0, else in one shot.  Outputs (W*H*3 doubles each, any may be null): render_accumulator,
// denoise_buffer, variance_buffer (all -1 when the render left it empty); info (may be null): denoise_used_variance, current_samples_count.  Returns 0,
// or -1 if the render did not finish.
int zrs_render_dropin_denoise_guided(void* p, int width, int height, int spp, int device, double threshold, int samples_per_pass, int guided, double* acc,
                                     double* den, double* var, int* info) {
    const handle& h = *(handle*)p;
    scene_camera cam(h, width, height, spp, device);
    cam.use_denoiser = true;
    cam.denoise_variance_guided = guided != 0;
    cam.adaptive_threshold = threshold;
    cam.samples_per_pass = samples_per_pass;
    cam.reset_accumulator();
    if (!render_world(h, cam, post_processor())) return -1;
    copy_out(cam.render_accumulator, acc); copy_out(cam.denoise_buffer, den);
    if (cam.variance_buffer.size() == cam.render_accumulator.size()) copy_out(cam.variance_buffer, var);
    else if (var) std::fill(var, var + cam.render_accumulator.size() * 3, -1.0);
    if (info) { info[0] = cam.denoise_used_variance ? 1 : 0; info[1] = cam.current_samples_count; }
    return 0;
}

// camera::render with use_denoiser and the extension flags 1 = denoise_nlm, 2 = denoise_variance_guided, 4 = temporal_accumulation through the drop-in API:
// adaptively when threshold > 0 (min = step = 64), progressively when samples_per_pass > 0, else in one shot.  Outputs (W*H*3 doubles each, any may be null):
// render_accumulator, denoise_buffer, variance_buffer, denoise_error_buffer (all -1 when the render left it empty); info (may be null): denoise_used_nlm,
// denoise_used_variance, current_samples_count.  Returns 0, or -1 if the render did not finish.
int zrs_render_dropin_denoise_nlm(void* p, int width, int height, int spp, int device, double threshold, int samples_per_pass, int flags, double* acc,
                                  double* den, double* var, double* err, int* info) {
    const handle& h = *(handle*)p;
    scene_camera cam(h, width, height, spp, device);
    cam.use_denoiser = true;
    cam.denoise_nlm = (flags & 1) != 0;
    cam.denoise_variance_guided = (flags & 2) != 0;
    cam.temporal_accumulation = (flags & 4) != 0;
    cam.adaptive_threshold = threshold;
    cam.samples_per_pass = samples_per_pass;
    cam.reset_accumulator();
    if (!render_world(h, cam, post_processor())) return -1;
    const size_t n = cam.render_accumulator.size();
    copy_out(cam.render_accumulator, acc); copy_out(cam.denoise_buffer, den);
    if (cam.variance_buffer.size() == n) copy_out(cam.variance_buffer, var);
    else if (var) std::fill(var, var + n * 3, -1.0);
    if (cam.denoise_error_buffer.size() == n) copy_out(cam.denoise_error_buffer, err);
    else if (err) std::fill(err, err + n * 3, -1.0);
    if (info) { info[0] = cam.denoise_used_nlm ? 1 : 0; info[1] = cam.denoise_used_variance ? 1 : 0; info[2] = cam.current_samples_count; }
    return 0;
}

// A camera path through ONE camera object and one world object (camera::temporal_accumulation keeps its history across render() calls of the object): n_frames
// renders with lookfrom / lookat = cams6[k] (6 doubles a frame) and seed = the scene's + k.  flags: 1 = temporal_accumulation, 2 = use_denoiser with
// denoise_variance_guided, 4 = reset_temporal_history() before the last frame.  samples_per_pass > 0 renders progressively, else in one shot.  Outputs, n_frames frames
// each, any may be null: render_accumulator, temporal_buffer, variance_buffer, denoise_buffer (W*H*3 doubles a frame; all -1 for a frame that left the buffer
// empty) and temporal_history_length (W*H ints, -1 likewise).  Returns 0, or -1 if a render did not finish.
int zrs_render_dropin_temporal(void* p, int width, int height, int spp, int device, int n_frames, const double* cams6, int flags, int samples_per_pass, double* acc,
                               double* tmp, double* var, double* den, int* hist) {
    const handle& h = *(handle*)p;
    scene_camera cam(h, width, height, spp, device);
    cam.temporal_accumulation = (flags & 1) != 0;
    cam.use_denoiser = cam.denoise_variance_guided = (flags & 2) != 0;
    cam.samples_per_pass = samples_per_pass;
    const uint64_t seed0 = cam.seed;
    const auto bvh_world = make_shared<bvh_node>(h.s.world);
    const post_processor post;
    const size_t npx = (size_t)cam.image_width * cam.image_height;
    auto frame_out = [&](const std::vector<color>& frame, double* out, int k) {
        if (!out) return;
        if (frame.size() == npx) std::memcpy(out + (size_t)k * npx * 3, frame.data(), npx * sizeof(color));
        else std::fill(out + (size_t)k * npx * 3, out + (size_t)(k + 1) * npx * 3, -1.0);
    };
    for (int k = 0; k < n_frames; k++) {
        const double* c = cams6 + (size_t)k * 6;
        cam.lookfrom = point3(c[0], c[1], c[2]); cam.lookat = point3(c[3], c[4], c[5]);
        cam.seed = seed0 + (uint64_t)k;
        if ((flags & 4) && k == n_frames - 1) cam.reset_temporal_history();
        cam.reset_accumulator();
        std::atomic<bool> flag{true};
        cam.render(*bvh_world, h.s.env, post, flag);
        if (cam.lines_rendered.load() != cam.image_height) return -1;
        frame_out(cam.render_accumulator, acc, k); frame_out(cam.temporal_buffer, tmp, k); frame_out(cam.variance_buffer, var, k);
        frame_out(cam.use_denoiser ? cam.denoise_buffer : std::vector<color>(), den, k);
        if (hist) {
            if (cam.temporal_history_length.size() == npx) std::memcpy(hist + (size_t)k * npx, cam.temporal_history_length.data(), npx * sizeof(int));
            else std::fill(hist + (size_t)k * npx, hist + (size_t)(k + 1) * npx, -1);
        }
    }
    return 0;
}

// A moving world through ONE drop-in camera object (camera::reuse_scene = reuse != 0): n_frames renders of a small world of the shim's own — a
// ground sphere, a sphere that rises, and one shared cube placed twice — whose placements are moved the way reference code moves things: the same objects
// under a translate and a rotate_y re-created with new arguments for every frame.  From frame add_at on (add_at < 0: never) the world holds one object more.
// The handle supplies environment and seed; the camera looks at the shim's world.  out: n_frames frames of W*H*3 doubles (render_accumulator); refit: n_frames
// ints, camera::last_scene_refit after each render.  Returns 0, or -1 if a render did not finish.
int zrs_render_dropin_animated(void* p, int width, int height, int spp, int device, int n_frames, int reuse, int add_at, double* out, int* refit) {
    const handle& h = *(handle*)p;
    scene_camera cam(h, width, height, spp, device);
    cam.reuse_scene = reuse != 0;
    cam.max_depth = 8; cam.vfov = 40; cam.defocus_angle = 0;
    cam.lookfrom = point3(0.5, 2.5, 7); cam.lookat = point3(0.3, 0.4, 0); cam.vup = vec3(0, 1, 0);
    const auto ground = make_shared<lambertian>(color(0.5, 0.6, 0.4)), red = make_shared<lambertian>(color(0.8, 0.2, 0.2)), blue = make_shared<lambertian>(color(0.2, 0.3, 0.8)),
               white = make_shared<lambertian>(color(0.8, 0.8, 0.8));
    const shared_ptr<hittable> box = make_shared<cube>(point3(-0.5, -0.5, -0.5), point3(0.5, 0.5, 0.5), red);   // the shared object
    const post_processor post;
    const size_t npx = (size_t)cam.image_width * cam.image_height;
    for (int k = 0; k < n_frames; k++) {
        hittable_list world;
        world.add(make_shared<sphere>(point3(0, -100.5, 0), 100.0, ground));
        world.add(make_shared<sphere>(point3(0.2, 0.3 + 0.15 * k, 1.5), 0.4, blue));
        world.add(make_shared<translate>(make_shared<rotate_y>(box, 0.3 + 0.25 * k), vec3(-1.2 + 0.4 * k, 0.0, 0.0)));
        world.add(make_shared<translate>(make_shared<rotate_y>(box, -0.2 * k), vec3(1.6, 0.2 * k, -1.0)));
        if (add_at >= 0 && k >= add_at) world.add(make_shared<sphere>(point3(-1.5, 0.2, 2.0), 0.3, white));
        const auto bvh_world = make_shared<bvh_node>(world);
        cam.reset_accumulator();
        std::atomic<bool> flag{true};
        cam.render(*bvh_world, h.s.env, post, flag);
        if (cam.lines_rendered.load() != cam.image_height) return -1;
        if (out) std::memcpy(out + (size_t)k * npx * 3, cam.render_accumulator.data(), npx * sizeof(color));
        if (refit) refit[k] = cam.last_scene_refit;
    }
    return 0;
}

// zrs_render_dropin_animated's world and camera with camera::temporal_accumulation through a progressive render (samples_per_pass = 64: the variance the
// history needs).  flags: 1 = reuse_scene, 2 = temporal_accumulation, 4 = temporal_track_motion.  Outputs, n_frames frames each, any may be null:
// render_accumulator, temporal_buffer (all -1 for a frame that left it empty), temporal_history_length (-1 likewise), last_scene_refit.
int zrs_render_dropin_animated_temporal(void* p, int width, int height, int spp, int device, int n_frames, int flags, double* acc, double* tmp, int* hist, int* refit) {
    const handle& h = *(handle*)p;
    scene_camera cam(h, width, height, spp, device);
    cam.reuse_scene = (flags & 1) != 0; cam.temporal_accumulation = (flags & 2) != 0; cam.temporal_track_motion = (flags & 4) != 0;
    cam.samples_per_pass = 64;
    cam.max_depth = 8; cam.vfov = 40; cam.defocus_angle = 0;
    cam.lookfrom = point3(0.5, 2.5, 7); cam.lookat = point3(0.3, 0.4, 0); cam.vup = vec3(0, 1, 0);
    const auto ground = make_shared<lambertian>(color(0.5, 0.6, 0.4)), red = make_shared<lambertian>(color(0.8, 0.2, 0.2)), blue = make_shared<lambertian>(color(0.2, 0.3, 0.8));
    const shared_ptr<hittable> box = make_shared<cube>(point3(-0.5, -0.5, -0.5), point3(0.5, 0.5, 0.5), red);
    const post_processor post;
    const size_t npx = (size_t)cam.image_width * cam.image_height;
    for (int k = 0; k < n_frames; k++) {
        hittable_list world;   // (frame k of zrs_render_dropin_animated without the added object)
        world.add(make_shared<sphere>(point3(0, -100.5, 0), 100.0, ground));
        world.add(make_shared<sphere>(point3(0.2, 0.3 + 0.15 * k, 1.5), 0.4, blue));
        world.add(make_shared<translate>(make_shared<rotate_y>(box, 0.3 + 0.25 * k), vec3(-1.2 + 0.4 * k, 0.0, 0.0)));
        world.add(make_shared<translate>(make_shared<rotate_y>(box, -0.2 * k), vec3(1.6, 0.2 * k, -1.0)));
        const auto bvh_world = make_shared<bvh_node>(world);
        cam.reset_accumulator();
        std::atomic<bool> flag{true};
        cam.render(*bvh_world, h.s.env, post, flag);
        if (cam.lines_rendered.load() != cam.image_height) return -1;
        if (acc) std::memcpy(acc + (size_t)k * npx * 3, cam.render_accumulator.data(), npx * sizeof(color));
        if (tmp) {
            if (cam.temporal_buffer.size() == npx) std::memcpy(tmp + (size_t)k * npx * 3, cam.temporal_buffer.data(), npx * sizeof(color));
            else std::fill(tmp + (size_t)k * npx * 3, tmp + (size_t)(k + 1) * npx * 3, -1.0);
        }
        if (hist) {
            if (cam.temporal_history_length.size() == npx) std::memcpy(hist + (size_t)k * npx, cam.temporal_history_length.data(), npx * sizeof(int));
            else std::fill(hist + (size_t)k * npx, hist + (size_t)(k + 1) * npx, -1);
        }
        if (refit) refit[k] = cam.last_scene_refit;
    }
    return 0;
}

// The reference's per-ray virtual API through the drop-in classes: for n rays (o, d, tmin, tmax) calls
// bvh_node(world).hit(r, interval(tmin, tmax), rec), then rec.mat->emitted(...) and rec.mat->scatter(r, rec, att, scattered)
// with random_double() positioned on the stream (seed, pixel, k) — the layout of `zenith_ref kat <scene> hits`:
// recs n x 16 (hit, t, p, normal, front_face, u, v, tangent, first-seen material ordinal, 0), scat n x 14 (scattered, attenuation,
// origin, direction, emitted, draws).  Returns 0, or -1 when a call threw.
int zrs_dropin_virtuals(void* p, const double* rays8, int n, uint64_t seed, uint64_t pixel, double* recs16, double* scat14) {
    handle* h = (handle*)p;
    try {
        auto world = make_shared<bvh_node>(h->s.world);
        std::unordered_map<const material*, int> ordinal;
        for (int k = 0; k < n; k++) {
            const double* q = rays8 + (size_t)k * 8;
            double* e = recs16 + (size_t)k * 16; double* sc = scat14 + (size_t)k * 14;
            for (int c = 0; c < 16; c++) e[c] = 0;
            for (int c = 0; c < 14; c++) sc[c] = 0;
            ray r(point3(q[0], q[1], q[2]), vec3(q[3], q[4], q[5]));
            zenith::seed_rng(seed, pixel, (uint64_t)k);
            hit_record rec;
            if (!world->hit(r, interval(q[6], q[7]), rec)) continue;
            zenith::seed_rng(seed, pixel, (uint64_t)k);
            e[0] = 1; e[1] = rec.t; e[2] = rec.p.x(); e[3] = rec.p.y(); e[4] = rec.p.z();
            e[5] = rec.normal.x(); e[6] = rec.normal.y(); e[7] = rec.normal.z(); e[8] = rec.front_face ? 1 : 0; e[9] = rec.u; e[10] = rec.v;
            e[11] = rec.tangent.x(); e[12] = rec.tangent.y(); e[13] = rec.tangent.z();
            if (!rec.mat) { e[14] = -1; continue; }
            auto it = ordinal.find(rec.mat.get());
            if (it == ordinal.end()) { const int id = (int)ordinal.size(); ordinal[rec.mat.get()] = id; e[14] = id; } else e[14] = it->second;
            color em = rec.mat->emitted(rec.u, rec.v, rec.p);
            ray scattered; color att;
            const uint64_t k0 = zenith::rng_state().k;
            bool ok = rec.mat->scatter(r, rec, att, scattered);
            sc[0] = ok ? 1 : 0;
            if (ok) {
                sc[1] = att.x(); sc[2] = att.y(); sc[3] = att.z();
                sc[4] = scattered.origin().x(); sc[5] = scattered.origin().y(); sc[6] = scattered.origin().z();
                sc[7] = scattered.direction().x(); sc[8] = scattered.direction().y(); sc[9] = scattered.direction().z();
            }
            sc[10] = em.x(); sc[11] = em.y(); sc[12] = em.z();
            sc[13] = (double)(zenith::rng_state().k - k0);
        }
    } catch (const std::exception& ex) {
        std::cerr << "[zrs_dropin_virtuals] " << ex.what() << "\n";
        return -1;
    }
    return 0;
}

}  // extern "C"

// sizes of the ABI structs as the C++ compiler sees them (tests compare them with the ctypes mirrors)
extern "C" size_t zrs_sizeof(int which) {
    switch (which) {
        case 0: return sizeof(zr_xform_op);
        case 1: return sizeof(zr_object);
        case 2: return sizeof(zr_medium);
        case 3: return sizeof(zr_material);
        case 4: return sizeof(zr_texture);
        case 5: return sizeof(zr_env);
        case 6: return sizeof(zr_camera);
        case 7: return sizeof(zr_region);
        case 8: return sizeof(zr_counters);
        case 9: return sizeof(zr_hit);
        case 10: return sizeof(zr_scene_desc);
        case 11: return sizeof(zr_post_params);
        case 12: return sizeof(zr_image_stats);
        case 13: return sizeof(zr_aov_params);
        case 14: return sizeof(zr_denoise_params);
        case 15: return sizeof(zr_bvh_debug_params);
        case 16: return sizeof(zr_bvh_debug_hit);
        case 17: return sizeof(zr_tree_box);
        case 18: return sizeof(zr_denoise_guided_params);
        case 19: return sizeof(zr_temporal_params);
        case 20: return sizeof(zr_denoise_nlm_params);
        case 21: return sizeof(zr_robust_params);
        case 22: return sizeof(zr_direct_params);
        case 23: return sizeof(zr_direct_stats);
        case 24: return sizeof(zr_light_slot);
        case 25: return sizeof(zr_light_sample);
        case 26: return sizeof(zr_env_light_info);
        default: return 0;
    }
}
