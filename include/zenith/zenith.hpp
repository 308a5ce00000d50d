// zenith.hpp — the drop-in C++20 scene API of the MI355X integrator.
//
// Same class names, constructors and public signatures as the reference's scene-authoring and render
// API (global namespace, like the reference), so that code written against
//   /root/reference/{vec3,ray,interval,aabb,hittable,hittable_list,sphere,triangle,cube,constant_medium,
//                     translate,rotate_x,rotate_y,rotate_z,scale,material_instance,bvh,texture,material,
//                     environment,camera}.hpp
// compiles unchanged (scenes/zr_scenes.inc is compiled against both).  What differs, by design:
//   * objects EXPOSE their data through flatten(zenith::scene_builder&) — reference objects keep all
//     members private with no getters (e.g. sphere.hpp:85-89), so a device backend cannot introspect them;
//   * camera::render() does not run a CPU loop: it flattens the world into the arrays of
//     include/zr_capi.h and calls the C ABI (libzr_hip.so); if that library or a HIP device is
//     missing it reports the error on std::cerr and leaves the buffers zeroed — there is NO CPU fallback;
//   * hittable::hit() / material::scatter() of the built-in classes stay CALLABLE, but they are not CPU-evaluated: a
//     call flattens the object (cached in the object), commits it as a one-object device scene and sends the ray
//     through the same kernels the renderer uses (zr_trace / zr_kat_scatter of the C ABI).  One launch per call — the
//     per-ray virtual path is exactly what this drop-in replaces, so this is for probing and tests, never for rendering;
//   * random_double() draws from the seedable contract stream of include/zr_rng.h instead of a racy
//     process-global mt19937 (common.hpp:29-34).
// No code is taken from the reference; each class cites the interface it mirrors.
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <typeinfo>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../zr_capi.h"
#include "../zr_rng.h"
#ifdef ZENITH_STB_IMAGE
#include "stb_image.h"
#endif

using std::make_shared;
using std::shared_ptr;

// ---- common.hpp:14-44 ---------------------------------------------------------------------------
constexpr double infinity = std::numeric_limits<double>::infinity();
constexpr double pi = 3.14159265358979323846;
const double ray_epsilon = 0.0001;
inline double degrees_to_radians(double d) { return d * pi / 180.0; }

// common.hpp:120-124: the BVH debug view (bvh.hpp:46-110).  camera::render with bvh_debug_mode set renders the wireframe / volume view of the
// device's own trees through zr_render_bvh_debug (include/zr_capi.h); the drop-in objects' own hit() does not read these.
namespace global_settings {
inline bool bvh_debug_mode = false;
inline float bvh_thickness = 0.01f;
inline int debug_bvh_level = -1;
}  // namespace global_settings
inline double radians_to_degrees(double r) { return r * 180.0 / pi; }

namespace zenith {
struct host_rng { uint64_t key = zr_stream_key(0, ZR_SCENE_PIXEL, 0); uint64_t k = 0; };
inline host_rng& rng_state() { static thread_local host_rng s; return s; }
// extension (the reference has no seed API): position random_double() on a contract stream
inline void seed_rng(uint64_t seed, uint64_t pixel = ZR_SCENE_PIXEL, uint64_t sample = 0) {
    rng_state().key = zr_stream_key(seed, pixel, sample); rng_state().k = 0;
}
}  // namespace zenith
inline double random_double() { auto& s = zenith::rng_state(); return zr_bits_to_unit(zr_stream_bits(s.key, s.k++)); }
namespace zenith {
// The reference's bvh_node constructor draws random_int(0, 2) once per node it creates (bvh.hpp:17): one node per span of 1 or 2
// objects, 1 + left + right for longer spans split at span / 2 (bvh.hpp:25-41).  The drop-in builds its own tree at commit, but
// whoever constructs a bvh_node or loads a model (model.hpp:95) must find random_double() where the reference leaves it, or
// every random scene decision made afterwards differs: the constructors below consume exactly that many draws.
inline uint64_t bvh_ctor_draws(size_t n) { return n <= 2 ? (n ? 1 : 0) : 1 + bvh_ctor_draws(n / 2) + bvh_ctor_draws(n - n / 2); }
inline void consume_draws(uint64_t n) { rng_state().k += n; }
}  // namespace zenith
inline double random_double(double lo, double hi) { return lo + (hi - lo) * random_double(); }
inline int random_int(int lo, int hi) { return static_cast<int>(random_double(lo, hi + 1)); }

// ---- vec3.hpp ------------------------------------------------------------------------------------
class vec3 {
public:
    double e[3];
    constexpr vec3() : e{0, 0, 0} {}
    constexpr vec3(double a, double b, double c) : e{a, b, c} {}
    constexpr double x() const { return e[0]; }
    constexpr double y() const { return e[1]; }
    constexpr double z() const { return e[2]; }
    constexpr vec3 operator-() const { return vec3(-e[0], -e[1], -e[2]); }
    constexpr double operator[](int i) const { return e[i]; }
    double& operator[](int i) { return e[i]; }
    vec3& operator+=(const vec3& o) { e[0] += o.e[0]; e[1] += o.e[1]; e[2] += o.e[2]; return *this; }
    vec3& operator-=(const vec3& o) { e[0] -= o.e[0]; e[1] -= o.e[1]; e[2] -= o.e[2]; return *this; }
    vec3& operator*=(const vec3& o) { e[0] *= o.e[0]; e[1] *= o.e[1]; e[2] *= o.e[2]; return *this; }
    vec3& operator*=(double t) { e[0] *= t; e[1] *= t; e[2] *= t; return *this; }
    vec3& operator/=(double t) { return *this *= 1 / t; }
    constexpr double length_squared() const { return e[0] * e[0] + e[1] * e[1] + e[2] * e[2]; }
    double length() const { return std::sqrt(length_squared()); }
    bool near_zero() const { return std::fabs(e[0]) < 1e-8 && std::fabs(e[1]) < 1e-8 && std::fabs(e[2]) < 1e-8; }
    double luminance() const { return 0.2126 * e[0] + 0.7152 * e[1] + 0.0722 * e[2]; }
    static vec3 random() { double a = random_double(), b = random_double(), c = random_double(); return vec3(a, b, c); }
    static vec3 random(double lo, double hi) {
        double a = random_double(lo, hi), b = random_double(lo, hi), c = random_double(lo, hi);
        return vec3(a, b, c);
    }
};
using point3 = vec3;
using color = vec3;
inline std::ostream& operator<<(std::ostream& o, const vec3& v) { return o << v.e[0] << " " << v.e[1] << " " << v.e[2]; }
inline vec3 operator+(const vec3& a, const vec3& b) { return vec3(a.e[0] + b.e[0], a.e[1] + b.e[1], a.e[2] + b.e[2]); }
inline vec3 operator-(const vec3& a, const vec3& b) { return vec3(a.e[0] - b.e[0], a.e[1] - b.e[1], a.e[2] - b.e[2]); }
inline vec3 operator*(const vec3& a, const vec3& b) { return vec3(a.e[0] * b.e[0], a.e[1] * b.e[1], a.e[2] * b.e[2]); }
inline vec3 operator*(double t, const vec3& v) { return vec3(t * v.e[0], t * v.e[1], t * v.e[2]); }
inline vec3 operator*(const vec3& v, double t) { return t * v; }
inline vec3 operator/(const vec3& v, double t) { return (1 / t) * v; }
inline double dot(const vec3& a, const vec3& b) { return a.e[0] * b.e[0] + a.e[1] * b.e[1] + a.e[2] * b.e[2]; }
inline vec3 cross(const vec3& a, const vec3& b) {
    return vec3(a.e[1] * b.e[2] - a.e[2] * b.e[1], a.e[2] * b.e[0] - a.e[0] * b.e[2], a.e[0] * b.e[1] - a.e[1] * b.e[0]);
}
inline vec3 unit_vector(const vec3& v) { double l = v.length(); return l < 1e-8 ? vec3(0, 0, 0) : v / l; }
inline vec3 random_in_unit_disk() {
    for (;;) { double a = random_double(-1, 1), b = random_double(-1, 1); vec3 p(a, b, 0); if (p.length_squared() < 1) return p; }
}
inline vec3 random_unit_vector() {
    for (;;) { vec3 p = vec3::random(-1, 1); double l2 = p.length_squared(); if (1e-160 < l2 && l2 <= 1) return p / std::sqrt(l2); }
}
inline vec3 random_on_hemisphere(const vec3& n) { vec3 s = random_unit_vector(); return dot(s, n) > 0.0 ? s : -s; }
inline vec3 reflect(const vec3& v, const vec3& n) { return v - 2 * dot(v, n) * n; }
inline vec3 refract(const vec3& uv, const vec3& n, double eta) {
    double ct = std::fmin(dot(-uv, n), 1.0);
    vec3 perp = eta * (uv + ct * n);
    return perp + (-std::sqrt(std::fabs(1.0 - perp.length_squared())) * n);
}

// ---- ray.hpp, interval.hpp, aabb.hpp --------------------------------------------------------------
class ray {
public:
    point3 orig; vec3 dir; double tm = 0.0;
    ray() {}
    ray(const point3& o, const vec3& d) : orig(o), dir(d), tm(0.0) {}
    ray(const point3& o, const vec3& d, double t) : orig(o), dir(d), tm(t) {}
    const point3& origin() const { return orig; }
    const vec3& direction() const { return dir; }
    double time() const { return tm; }
    point3 at(double t) const { return orig + t * dir; }
};

class interval {
public:
    double min, max;
    interval() : min(+infinity), max(-infinity) {}
    interval(double lo, double hi) : min(lo), max(hi) {}
    interval(const interval& a, const interval& b) : min(std::fmin(a.min, b.min)), max(std::fmax(a.max, b.max)) {}
    interval expand(double delta) const { return interval(min - delta / 2, max + delta / 2); }
    double size() const { return max - min; }
    bool contains(double x) const { return min <= x && x <= max; }
    bool surrounds(double x) const { return min < x && max > x; }
    double clamp(double x) const { return x < min ? min : (x > max ? max : x); }
    static const interval empty, universe;
};
inline const interval interval::empty = interval(+infinity, -infinity);
inline const interval interval::universe = interval(-infinity, +infinity);
inline interval operator+(const interval& i, double d) { return interval(i.min + d, i.max + d); }
inline interval operator+(double d, const interval& i) { return i + d; }

class aabb {
public:
    interval x, y, z;
    aabb() {}
    aabb(const interval& a, const interval& b, const interval& c) : x(a), y(b), z(c) {}
    aabb(const point3& a, const point3& b)
        : x(std::fmin(a[0], b[0]), std::fmax(a[0], b[0])), y(std::fmin(a[1], b[1]), std::fmax(a[1], b[1])),
          z(std::fmin(a[2], b[2]), std::fmax(a[2], b[2])) {}
    aabb(const aabb& a, const aabb& b) : x(a.x, b.x), y(a.y, b.y), z(a.z, b.z) {}
    const interval& axis(int n) const { return n == 1 ? y : (n == 2 ? z : x); }
};
inline aabb operator+(const aabb& b, const vec3& o) { return aabb(b.x + o.x(), b.y + o.y(), b.z + o.z()); }
inline aabb operator+(const vec3& o, const aabb& b) { return b + o; }

class material;
class texture;
class hittable;

// ---- flattening: the part the reference does not have ---------------------------------------------
namespace zenith {

constexpr uint32_t no_material = 0xFFFFFFFFu;

// vectors of the large arrays: resize() leaves new elements uninitialised (no 160 MB zero-fill by one thread before the threads of
// a bulk flatten write them; their pages are first touched by those threads)
template <class T>
struct noinit_allocator : std::allocator<T> {
    template <class U> struct rebind { using other = noinit_allocator<U>; };
    noinit_allocator() = default;
    template <class U> noinit_allocator(const noinit_allocator<U>&) {}
    template <class U, class... A> void construct(U* p, A&&... a) { if constexpr (sizeof...(A) == 0) ::new ((void*)p) U; else ::new ((void*)p) U(std::forward<A>(a)...); }
};
template <class T> using nvec = std::vector<T, noinit_allocator<T>>;

// a texture coordinate of a triangle's corner (u to the right, v = 0 the image's first row: texture::value's convention)
struct texcoord { double u = 0, v = 0; };

struct flat_scene {
    std::vector<double> spheres, cubes;
    nvec<double> tri_v, tri_n;
    // per-vertex texture coordinates, 6 per triangle (u0 v0 u1 v1 u2 v2), or EMPTY: the array appears with the first triangle that brings coordinates
    // (zeros for the triangles before it, and for every later one that brings none), so a world without any flattens to what it always did
    nvec<double> tri_uv;
    std::vector<uint32_t> sphere_mat, cube_mat;
    nvec<uint32_t> tri_mat;
    std::vector<zr_medium> media;
    std::vector<zr_xform_op> ops;
    nvec<zr_object> objects;
    std::vector<zr_group> groups;
    std::vector<zr_material> materials;
    std::vector<zr_texture> textures;
    std::vector<unsigned char> texels;
    std::vector<std::string> warnings;
    // empties the scene but keeps the arrays' memory: a camera flattens its world on every render, and a quarter of a gigabyte of
    // freshly mapped pages costs more to touch than a million triangles cost to copy
    void clear() {
        spheres.clear(); cubes.clear(); tri_v.clear(); tri_n.clear(); tri_uv.clear(); sphere_mat.clear(); cube_mat.clear(); tri_mat.clear(); media.clear(); ops.clear();
        objects.clear(); groups.clear(); materials.clear(); textures.clear(); texels.clear(); warnings.clear();
    }
    zr_scene_desc desc() const {
        zr_scene_desc d{};
        d.spheres = spheres.data(); d.sphere_mat = sphere_mat.data(); d.n_spheres = sphere_mat.size();
        d.tri_v = tri_v.data(); d.tri_n = tri_n.data(); d.tri_mat = tri_mat.data(); d.n_tris = tri_mat.size();
        d.cubes = cubes.data(); d.cube_mat = cube_mat.data(); d.n_cubes = cube_mat.size();
        d.media = media.data(); d.n_media = media.size();
        d.ops = ops.data(); d.n_ops = ops.size();
        d.objects = objects.data(); d.n_objects = objects.size();
        d.materials = materials.data(); d.n_materials = materials.size();
        d.textures = textures.data(); d.n_textures = textures.size();
        d.texels = texels.data(); d.texel_bytes = texels.size();
        d.groups = groups.data(); d.n_groups = groups.size();
        return d;
    }
    // tri_uv in step with the n triangles there are now (call only once the array exists, or to create it): new entries are zero
    void sync_uv(size_t n) {
        const size_t had = tri_uv.size();
        tri_uv.resize(n * 6);
        if (n * 6 > had) std::memset(tri_uv.data() + had, 0, (n * 6 - had) * sizeof(double));
    }
    // hands the scene to the C ABI: the arrays borrowed until the commit (zr_scene_set_all_borrowed), the texture coordinates, if any, copied
    int give_to(zr_scene* sc) const {
        const zr_scene_desc d = desc();
        int rc = zr_scene_set_all_borrowed(sc, &d);
        if (rc == ZR_OK && !tri_uv.empty()) rc = zr_scene_set_triangle_uvs(sc, tri_uv.data(), tri_mat.size());
        return rc;
    }
    // the same with every array COPIED by the library (zr_scene_set_all): a scene that is to be moved in place (camera::reuse_scene)
    int give_copied_to(zr_scene* sc) const {
        const zr_scene_desc d = desc();
        int rc = zr_scene_set_all(sc, &d);
        if (rc == ZR_OK && !tri_uv.empty()) rc = zr_scene_set_triangle_uvs(sc, tri_uv.data(), tri_mat.size());
        return rc;
    }
    // equal to `o` in everything an update cannot change: all arrays byte for byte, except the a[3] of the ops and the numbers of the spheres
    bool same_but_placements(const flat_scene& o) const {
        auto eq = [](const auto& a, const auto& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0); };
        if (spheres.size() != o.spheres.size() || ops.size() != o.ops.size()) return false;
        for (size_t k = 0; k < ops.size(); k++) if (ops[k].kind != o.ops[k].kind || ops[k].mat != o.ops[k].mat) return false;
        return eq(cubes, o.cubes) && eq(tri_v, o.tri_v) && eq(tri_n, o.tri_n) && eq(tri_uv, o.tri_uv) && eq(sphere_mat, o.sphere_mat) && eq(cube_mat, o.cube_mat) && eq(tri_mat, o.tri_mat) &&
               eq(media, o.media) && eq(objects, o.objects) && eq(groups, o.groups) && eq(materials, o.materials) && eq(textures, o.textures) && eq(texels, o.texels);
    }
};

class scene_builder {
public:
    explicit scene_builder(flat_scene& f) : fs(f) {}
    flat_scene& fs;

    void push_op(uint32_t kind, double a0, double a1, double a2, uint32_t mat = 0) {
        zr_xform_op op{}; op.kind = kind; op.mat = mat; op.a[0] = a0; op.a[1] = a1; op.a[2] = a2; chain.push_back(op);
    }
    void pop_op() { chain.pop_back(); }

    uint32_t texture_id(const shared_ptr<texture>& t);
    uint32_t material_id(const shared_ptr<material>& m);
    uint32_t add_material(const zr_material& m) { fs.materials.push_back(m); return (uint32_t)fs.materials.size() - 1; }
    uint32_t add_texture(const zr_texture& t) { fs.textures.push_back(t); return (uint32_t)fs.textures.size() - 1; }
    uint64_t add_texels(const void* p, size_t bytes) {
        size_t off = (fs.texels.size() + 15) & ~size_t(15);
        fs.texels.resize(off + bytes);
        std::memcpy(fs.texels.data() + off, p, bytes);
        return off;
    }

    void emit_sphere(const point3& c, double radius_arg, const shared_ptr<material>& m) {
        fs.spheres.insert(fs.spheres.end(), {c.x(), c.y(), c.z(), radius_arg});
        fs.sphere_mat.push_back(material_id(m));
        emit(ZR_PRIM_SPHERE, (uint32_t)fs.sphere_mat.size() - 1);
    }
    // (the hot call of a flatten: a million-triangle world comes through here once per render, on the caller's clock)
    void emit_triangle(const point3 v[3], const vec3 n[3], const shared_ptr<material>& m, const texcoord* uv = nullptr) {
        const size_t i = fs.tri_mat.size();
        if (uv || !fs.tri_uv.empty()) {
            fs.sync_uv(i + 1);
            if (uv) { double* t = fs.tri_uv.data() + i * 6; for (int k = 0; k < 3; k++) { t[2 * k] = uv[k].u; t[2 * k + 1] = uv[k].v; } }
        }
        fs.tri_v.resize(i * 9 + 9); fs.tri_n.resize(i * 9 + 9);
        double* tv = fs.tri_v.data() + i * 9; double* tn = fs.tri_n.data() + i * 9;
        for (int k = 0; k < 3; k++) { tv[3 * k] = v[k].x(); tv[3 * k + 1] = v[k].y(); tv[3 * k + 2] = v[k].z(); tn[3 * k] = n[k].x(); tn[3 * k + 1] = n[k].y(); tn[3 * k + 2] = n[k].z(); }
        fs.tri_mat.push_back(material_id(m));
        emit(ZR_PRIM_TRIANGLE, (uint32_t)i);
    }
    // BULK: n bare triangles of one list in one go (hittable_list::flatten on long runs).  Returns false when the builder is in a
    // state where entries are not plain world entries (capturing a template, inside a medium's boundary): the caller then emits
    // them one by one.  Otherwise the arrays are grown by n, `first_tri` / `first_obj` say where, and every world entry of the run
    // shares ONE copy of the open wrapper chain.
    bool begin_bulk_triangles(size_t n, size_t& first_tri, size_t& first_obj, uint32_t& chain_first, uint32_t& chain_count, bool& entries) {
        if (in_boundary) return false;
        if (!caps.empty() && chain.size() != caps.back().base) return false;   // inside a template under wrappers of its own: members, one by one
        entries = caps.empty();   // inside a template the triangles are a run of the template, not world entries
        first_tri = fs.tri_mat.size(); first_obj = fs.objects.size();
        fs.tri_v.resize((first_tri + n) * 9); fs.tri_n.resize((first_tri + n) * 9); fs.tri_mat.resize(first_tri + n);
        chain_count = 0; chain_first = 0;
        if (entries) { fs.objects.resize(first_obj + n); chain_count = (uint32_t)chain.size(); chain_first = copy_chain(0, chain.size()); }
        return true;
    }
    void end_bulk_triangles(size_t first_tri, size_t run, size_t n_obj, bool entries) {   // the run is `run` long: cut the arrays back; in a template, note it
        fs.tri_v.resize((first_tri + run) * 9); fs.tri_n.resize((first_tri + run) * 9); fs.tri_mat.resize(first_tri + run);
        if (!fs.tri_uv.empty()) fs.sync_uv(first_tri + run);
        if (entries) { fs.objects.resize(n_obj); return; }
        tmpl& t = templates[caps.back().tmpl];
        if (!t.items.empty() && t.items.back().what == 0 && t.items.back().inner.empty() && t.items.back().index + t.items.back().count == first_tri) { t.items.back().count += (uint32_t)run; return; }
        tmpl_item m; m.what = 0; m.type = ZR_PRIM_TRIANGLE; m.index = (uint32_t)first_tri; m.count = (uint32_t)run;
        t.items.push_back(std::move(m));
    }
    // a list of n objects is about to be flattened: make room once instead of growing by doubling (mostly triangles in the lists
    // that are long enough to matter; capacity that stays unused is never touched)
    void reserve_hint(size_t n) {
        if (n < 4096) return;
        fs.tri_v.reserve(fs.tri_v.size() + n * 9); fs.tri_n.reserve(fs.tri_n.size() + n * 9); fs.tri_mat.reserve(fs.tri_mat.size() + n);
        if (caps.empty()) fs.objects.reserve(fs.objects.size() + n);
    }
    void emit_cube(const vec3& he, const point3& c, const point3& mn, const point3& mx, const shared_ptr<material>& m) {
        fs.cubes.insert(fs.cubes.end(), {he.x(), he.y(), he.z(), c.x(), c.y(), c.z(), mn.x(), mn.y(), mn.z(), mx.x(), mx.y(), mx.z()});
        fs.cube_mat.push_back(material_id(m));
        if (!in_boundary && !(c.x() == 0 && c.y() == 0 && c.z() == 0))
            fs.warnings.push_back("cube not centred at the origin: the reference tests it as if it were (cube.hpp:45-58) but culls "
                                  "with its true box; only origin-centred cubes (wrapped in translate) are reproduced");
        emit(ZR_PRIM_CUBE, (uint32_t)fs.cube_mat.size() - 1);
    }
    void emit_medium(const hittable& boundary, double density, uint32_t iso_material);

    void unsupported(const char* what) { fs.warnings.push_back(std::string("unsupported hittable skipped: ") + what); }

    // TWO-LEVEL BVH.  What the reference shares between instances — the same shared_ptr (a model, a bvh_node, a prefab list) inside
    // several translate / rotate_* / scale / material_instance objects — is flattened ONCE, in its own space, into a TEMPLATE:
    //   * its runs of bare triangles become zr_groups (stored once, a tree of their own on the device; every placement of the run
    //     is ONE ZR_PRIM_GROUP world entry carrying the wrapper chain),
    //   * its other members — spheres, cubes, media, primitives under wrappers of their own inside the child — are stored once
    //     too and referenced by index: a placement emits one world entry per member whose chain is the placement's followed by
    //     the member's inner chain,
    //   * a shared child INSIDE the child (a group inside a group) is a template of its own, referenced under its inner chain:
    //     its triangle runs are the same zr_groups wherever the outer child is placed.
    // So a composite prefab placed N times costs N small entries per member and per mesh, and its triangles once (round 2 shared
    // only children that were nothing but bare triangles; anything else was copied per placement, triangles included).
    // `children` flattens the child's parts.  A run placed only once in the end is dissolved by finish().
    template <class F>
    void emit_run(const void* identity, F&& children) {
        const char* e_ = std::getenv("ZR_GROUPS");
        const bool off = e_ && *e_ == '0';   // ZR_GROUPS=0: always one entry per primitive
        if (off || in_boundary || (caps.empty() && chain.empty())) { children(); return; }   // (a child added bare to the world is flattened in place)
        auto it = tmpl_ids.find(identity);
        if (it == tmpl_ids.end()) {
            const uint32_t id = (uint32_t)templates.size();
            templates.emplace_back();
            caps.push_back(capture{id, chain.size()});
            children();
            caps.pop_back();
            close_template(id);
            it = tmpl_ids.emplace(identity, id).first;
        }
        if (!caps.empty()) {   // met while an outer child is being captured: a member of that template, under the chain opened since
            tmpl_item m; m.what = 2; m.index = it->second;
            m.inner.assign(chain.begin() + (std::ptrdiff_t)caps.back().base, chain.end());
            templates[caps.back().tmpl].items.push_back(std::move(m));
            return;
        }
        expand(it->second);
    }
    // call once, after the world has been flattened and before flat_scene::desc(): groups placed a single time gain nothing from
    // a tree of their own — their placement is replaced by its triangles (each under the placement's chain) unless
    // ZR_GROUP_ALWAYS is set
    void finish() {
        if (fs.groups.empty()) return;
        const char* always = std::getenv("ZR_GROUP_ALWAYS");
        std::vector<uint32_t> uses(fs.groups.size(), 0);
        for (const zr_object& o : fs.objects) if (o.type == ZR_PRIM_GROUP) uses[o.index]++;
        std::vector<uint32_t> new_id(fs.groups.size(), 0xFFFFFFFFu);
        std::vector<zr_group> kept;
        for (size_t g = 0; g < fs.groups.size(); g++)
            if (uses[g] > 1 || (uses[g] == 1 && always && *always && *always != '0')) { new_id[g] = (uint32_t)kept.size(); kept.push_back(fs.groups[g]); }
        nvec<zr_object> out;
        out.reserve(fs.objects.size());
        for (const zr_object& o : fs.objects) {
            if (o.type != ZR_PRIM_GROUP) { out.push_back(o); continue; }
            if (new_id[o.index] != 0xFFFFFFFFu) { zr_object q = o; q.index = new_id[o.index]; out.push_back(q); continue; }
            const zr_group& g = fs.groups[o.index];
            for (uint32_t k = 0; k < g.triangle_count; k++) { zr_object q = o; q.type = ZR_PRIM_TRIANGLE; q.index = g.first_triangle + k; out.push_back(q); }
        }
        fs.objects.swap(out);
        fs.groups.swap(kept);
    }

private:
    std::vector<zr_xform_op> chain;  // wrappers currently open, outermost first
    size_t boundary_base = 0;
    bool in_boundary = false;
    zr_object captured{};            // the boundary primitive of the medium being flattened
    bool captured_ok = false;
    // templates of shared children (emit_run)
    struct tmpl_item { int what = 1; /* 0 run of triangles -> group, 1 primitive, 2 another template */ uint32_t type = 0, index = 0, count = 0; std::vector<zr_xform_op> inner; };
    struct tmpl { std::vector<tmpl_item> items; };
    struct capture { uint32_t tmpl; size_t base; /* chain.size() when the capture began: what follows is the member's inner chain */ };
    std::vector<tmpl> templates;
    std::vector<capture> caps;
    std::unordered_map<const void*, uint32_t> tmpl_ids;   // shared child -> its template
    std::unordered_map<const material*, uint32_t> mat_ids;
    const material* last_mat_ = nullptr; uint32_t last_mat_id_ = 0;   // the last lookup of material_id()
    std::unordered_map<const texture*, uint32_t> tex_ids;
public:
    std::unordered_map<uint32_t, shared_ptr<material>> mat_ptrs;   // flattened material id -> the object it came from
private:
    // a captured child is complete: its triangle runs become groups (a run shorter than ZR_GROUP_MIN_TRIS, default 4, beside other
    // members is not worth a tree of its own: it stays a list of triangles)
    void close_template(uint32_t id) {
        tmpl& t = templates[id];
        const char* e = std::getenv("ZR_GROUP_MIN_TRIS");
        const uint32_t min_tris = e && *e ? (uint32_t)std::atoi(e) : 4u;
        const bool pure = t.items.size() == 1 && t.items[0].what == 0;   // nothing but one run of triangles (a model): always a group
        std::vector<tmpl_item> out;
        for (tmpl_item& m : t.items) {
            if (m.what != 0) { out.push_back(std::move(m)); continue; }
            if (pure || m.count >= min_tris) {
                zr_group g{}; g.first_triangle = m.index; g.triangle_count = m.count;
                fs.groups.push_back(g);
                m.index = (uint32_t)fs.groups.size() - 1;
                out.push_back(std::move(m));
            } else
                for (uint32_t k = 0; k < m.count; k++) { tmpl_item q; q.what = 1; q.type = ZR_PRIM_TRIANGLE; q.index = m.index + k; out.push_back(std::move(q)); }
        }
        t.items.swap(out);
    }
    // one placement of a template under the chain that is open now
    void expand(uint32_t id) {
        for (size_t k = 0; k < templates[id].items.size(); k++) {
            const tmpl_item m = templates[id].items[k];   // (a copy: emit() below may grow `templates`' neighbours, never this vector, but stay safe)
            for (const zr_xform_op& op : m.inner) chain.push_back(op);
            if (m.what == 0) emit(ZR_PRIM_GROUP, m.index);
            else if (m.what == 1) emit(m.type, m.index);
            else expand(m.index);
            chain.resize(chain.size() - m.inner.size());
        }
    }

    uint32_t copy_chain(size_t from, size_t to) {
        uint32_t first = (uint32_t)fs.ops.size();
        for (size_t k = from; k < to; k++) fs.ops.push_back(chain[k]);
        return first;
    }
    void emit(uint32_t type, uint32_t index) {
        zr_object o{};
        o.type = type; o.index = index;
        if (!caps.empty() && !in_boundary) {   // inside a shared child that is being captured: a member of its template, not a world entry
            tmpl& t = templates[caps.back().tmpl];
            const size_t base = caps.back().base;
            if (type == ZR_PRIM_TRIANGLE && chain.size() == base && !t.items.empty() && t.items.back().what == 0 &&
                t.items.back().index + t.items.back().count == index) { t.items.back().count++; return; }   // the run goes on
            tmpl_item m;
            m.what = (type == ZR_PRIM_TRIANGLE && chain.size() == base) ? 0 : 1;
            m.type = type; m.index = index; m.count = 1;
            m.inner.assign(chain.begin() + (std::ptrdiff_t)base, chain.end());
            t.items.push_back(std::move(m));
            return;
        }
        if (in_boundary) {
            o.chain_count = (uint32_t)(chain.size() - boundary_base);
            o.chain_first = copy_chain(boundary_base, chain.size());
            captured = o; captured_ok = true;
        } else {
            o.chain_count = (uint32_t)chain.size();
            o.chain_first = copy_chain(0, chain.size());
            fs.objects.push_back(o);
        }
    }
};

[[noreturn]] inline void no_cpu_path(const char* what) {
    throw std::logic_error(std::string(what) + ": the MI355X drop-in does not evaluate rays on the CPU; render through camera::render()");
}

// hittable::hit / material::scatter of the built-in classes, answered by the device (defined at the end of this header)
struct device_object;
}  // namespace zenith
class hit_record;
namespace zenith {
bool device_hit(const hittable& self, const ray& r, const interval& ray_t, hit_record& rec);
bool device_scatter(const material& self, const ray& r_in, const hit_record& rec, vec3& attenuation, ray& scattered);
}  // namespace zenith

// ---- hittable.hpp ---------------------------------------------------------------------------------
class hit_record {
public:
    point3 p; vec3 normal, tangent, bitangent;
    shared_ptr<material> mat;
    bool front_face = false;
    double t = 0.0, u = 0.0, v = 0.0;
    void set_face_normal(const ray& r, const vec3& outward) {
        front_face = dot(r.direction(), outward) < 0;
        normal = front_face ? outward : -outward;
    }
};

class hittable {
public:
    virtual ~hittable() = default;
    virtual bool hit(const ray& r, interval ray_t, hit_record& rec, int depth = 0, bool debug_wire = false) const = 0;
    virtual aabb bounding_box() const = 0;
    // drop-in extension: hand the object's data to the device backend.  User-defined hittables that do
    // not override it are reported and skipped.
    virtual void flatten(zenith::scene_builder& b) const { b.unsupported(typeid(*this).name()); }
    mutable shared_ptr<zenith::device_object> zr_device_cache_;   // drop-in: the committed one-object scene hit() sends rays to
};

// ---- texture.hpp ----------------------------------------------------------------------------------
class texture {
public:
    virtual ~texture() = default;
    virtual color value(double u, double v, const point3& p) const = 0;
    virtual uint32_t flatten(zenith::scene_builder& b) const = 0;
};

class solid_color : public texture {
public:
    solid_color(const color& c) : albedo(c) {}
    solid_color(double r, double g, double b) : albedo(r, g, b) {}
    color value(double, double, const point3&) const override { return albedo; }
    uint32_t flatten(zenith::scene_builder& b) const override {
        zr_texture t{}; t.kind = ZR_TEX_SOLID; t.color[0] = albedo.x(); t.color[1] = albedo.y(); t.color[2] = albedo.z();
        return b.add_texture(t);
    }
private:
    color albedo;
};

class checker_texture : public texture {
public:
    checker_texture(double scale, shared_ptr<texture> odd, shared_ptr<texture> even) : inv_scale(1.0 / scale), odd(odd), even(even) {}
    checker_texture(double scale, color c1, color c2)
        : inv_scale(1.0 / scale), odd(make_shared<solid_color>(c1)), even(make_shared<solid_color>(c2)) {}
    color value(double u, double v, const point3& p) const override {
        int s = static_cast<int>(std::floor(inv_scale * p.x())) + static_cast<int>(std::floor(inv_scale * p.y())) +
                static_cast<int>(std::floor(inv_scale * p.z()));
        return s % 2 == 0 ? even->value(u, v, p) : odd->value(u, v, p);
    }
    uint32_t flatten(zenith::scene_builder& b) const override {
        zr_texture t{}; t.kind = ZR_TEX_CHECKER; t.inv_scale = inv_scale;
        t.odd = b.texture_id(odd); t.even = b.texture_id(even);
        return b.add_texture(t);
    }
private:
    double inv_scale; shared_ptr<texture> odd, even;
};

// image_texture(filename, is_hdr): texture.hpp:14-39.  The reference decodes through stb_image; the
// drop-in has its own readers for the two formats its scenes and tests use: Radiance .hdr (RGBE, flat or
// new-style RLE scanlines) for is_hdr, binary PPM (P6, maxval 255) otherwise.  Anything else behaves
// like the reference's failed load: width = height = 0 and value() returns cyan (texture.hpp:52-54).
// A host that has stb_image on its include path (the reference vendors it under libs/stb) defines ZENITH_STB_IMAGE before
// including this header (and STB_IMAGE_IMPLEMENTATION in one translation unit, as the reference's stb_impl.cpp does): every format
// stb decodes (JPEG, PNG, ...) then loads exactly as in the reference — stbi_loadf / stbi_load with 3 channels forced
// (texture.hpp:23,31) — and the built-in readers serve as the fallback.
class image_texture : public texture {
public:
    image_texture(const char* filename, bool is_hdr = false) : hdr(is_hdr) {
        bool ok = false;
#ifdef ZENITH_STB_IMAGE
        ok = load_stb(filename);
#endif
        if (!ok) ok = is_hdr ? load_hdr(filename) : load_ppm(filename);
        if (!ok) {
            std::cerr << (is_hdr ? "ERROR: Could not load HDR: " : "ERROR: Could not load texture: ") << filename << "\n";
            width = height = 0; f32.clear(); u8.clear();
        }
    }
    color value(double u, double v, const point3&) const override {
        if (width == 0 || height == 0) return color(0.0, 1.0, 1.0);
        u = u - std::floor(u);
        int i = std::clamp(static_cast<int>(u * width), 0, width - 1);
        int j = std::clamp(static_cast<int>(v * height), 0, height - 1);
        size_t o = ((size_t)j * width + i) * 3;
        if (hdr) return color(f32[o], f32[o + 1], f32[o + 2]);
        const double s = 1.0 / 255.0;
        return color(s * u8[o], s * u8[o + 1], s * u8[o + 2]);
    }
    uint32_t flatten(zenith::scene_builder& b) const override {
        zr_texture t{}; t.kind = hdr ? ZR_TEX_IMAGE_F32 : ZR_TEX_IMAGE_U8; t.width = (uint32_t)width; t.height = (uint32_t)height;
        if (width && height) t.texel_offset = hdr ? b.add_texels(f32.data(), f32.size() * 4) : b.add_texels(u8.data(), u8.size());
        return b.add_texture(t);
    }
    int image_width() const { return width; }
    int image_height() const { return height; }
private:
    bool hdr; int width = 0, height = 0;
    std::vector<float> f32; std::vector<unsigned char> u8;

#ifdef ZENITH_STB_IMAGE
    bool load_stb(const char* fn) {   // texture.hpp:20-36
        int w = 0, h = 0, ch = 0;
        if (hdr) {
            float* d = stbi_loadf(fn, &w, &h, &ch, 3);
            if (!d) return false;
            f32.assign(d, d + (size_t)w * h * 3); stbi_image_free(d);
        } else {
            unsigned char* d = stbi_load(fn, &w, &h, &ch, 3);
            if (!d) return false;
            u8.assign(d, d + (size_t)w * h * 3); stbi_image_free(d);
        }
        width = w; height = h; return w > 0 && h > 0;
    }
#endif
    bool load_ppm(const char* fn) {
        std::ifstream f(fn, std::ios::binary);
        if (!f) return false;
        std::string magic; int w = 0, h = 0, mx = 0;
        auto token = [&](std::string& s) {
            s.clear(); int c;
            for (;;) { c = f.get(); if (c == '#') { while (c != '\n' && c != EOF) c = f.get(); } else if (!isspace(c)) break; if (c == EOF) return; }
            while (c != EOF && !isspace(c)) { s.push_back((char)c); c = f.get(); }
        };
        std::string tw, th, tm;
        token(magic); token(tw); token(th); token(tm);
        if (magic != "P6") return false;
        w = std::atoi(tw.c_str()); h = std::atoi(th.c_str()); mx = std::atoi(tm.c_str());
        if (w <= 0 || h <= 0 || mx != 255) return false;
        u8.resize((size_t)w * h * 3);
        f.read((char*)u8.data(), (std::streamsize)u8.size());
        if ((size_t)f.gcount() != u8.size()) return false;
        width = w; height = h; return true;
    }
    bool load_hdr(const char* fn) {
        std::ifstream f(fn, std::ios::binary);
        if (!f) return false;
        std::string line;
        if (!std::getline(f, line) || (line.rfind("#?RADIANCE", 0) != 0 && line.rfind("#?RGBE", 0) != 0)) return false;
        bool fmt = false;
        while (std::getline(f, line)) { if (line.empty()) break; if (line == "FORMAT=32-bit_rle_rgbe") fmt = true; }
        if (!fmt || !std::getline(f, line)) return false;
        int h = 0, w = 0;
        if (std::sscanf(line.c_str(), "-Y %d +X %d", &h, &w) != 2 || w <= 0 || h <= 0) return false;
        std::vector<unsigned char> rgbe((size_t)w * h * 4);
        std::vector<unsigned char> rest((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        size_t pos = 0;
        bool flat = (w < 8 || w >= 32768) || rest.size() < 4 || rest[0] != 2 || rest[1] != 2 || (rest[2] & 0x80);
        if (flat) {
            if (rest.size() < rgbe.size()) return false;
            std::memcpy(rgbe.data(), rest.data(), rgbe.size());
        } else {
            for (int j = 0; j < h; j++) {
                if (pos + 4 > rest.size() || rest[pos] != 2 || rest[pos + 1] != 2 || ((rest[pos + 2] << 8) | rest[pos + 3]) != w) return false;
                pos += 4;
                for (int ch = 0; ch < 4; ch++) {
                    int i = 0;
                    while (i < w) {
                        if (pos >= rest.size()) return false;
                        int n = rest[pos++];
                        if (n > 128) { n -= 128; if (pos >= rest.size() || i + n > w) return false; unsigned char v = rest[pos++]; while (n--) rgbe[((size_t)j * w + i++) * 4 + ch] = v; }
                        else { if (n == 0 || pos + n > rest.size() || i + n > w) return false; while (n--) rgbe[((size_t)j * w + i++) * 4 + ch] = rest[pos++]; }
                    }
                }
            }
        }
        f32.resize((size_t)w * h * 3);
        for (size_t p = 0; p < (size_t)w * h; p++) {
            const unsigned char* q = &rgbe[p * 4];
            if (q[3] != 0) {
                float s = std::ldexp(1.0f, (int)q[3] - (128 + 8));
                f32[p * 3] = q[0] * s; f32[p * 3 + 1] = q[1] * s; f32[p * 3 + 2] = q[2] * s;
            } else f32[p * 3] = f32[p * 3 + 1] = f32[p * 3 + 2] = 0.f;
        }
        width = w; height = h; return true;
    }
};

// ---- material.hpp ---------------------------------------------------------------------------------
class material {
public:
    virtual ~material() = default;
    virtual color emitted(double, double, const point3&) const { return color(0, 0, 0); }
    virtual bool scatter(const ray& r_in, const hit_record& rec, color& attenuation, ray& scattered) const = 0;
    virtual color get_albedo(const hit_record&) const { return color(0, 0, 0); }
    virtual uint32_t flatten(zenith::scene_builder& b) const = 0;
    mutable shared_ptr<zenith::device_object> zr_device_cache_;   // drop-in: the committed scene scatter() runs on
};

class lambertian : public material {
public:
    lambertian(const color& albedo, shared_ptr<texture> bump = nullptr, double strength = 1.0)
        : tex(make_shared<solid_color>(albedo)), bump(bump), strength(strength) {}
    lambertian(shared_ptr<texture> tex, shared_ptr<texture> bump = nullptr, double strength = 1.0) : tex(tex), bump(bump), strength(strength) {}
    bool scatter(const ray& r_in, const hit_record& rec, color& attenuation, ray& scattered) const override { return zenith::device_scatter(*this, r_in, rec, attenuation, scattered); }
    color get_albedo(const hit_record& rec) const override { return tex->value(rec.u, rec.v, rec.p); }
    uint32_t flatten(zenith::scene_builder& b) const override {
        zr_material m{}; m.kind = ZR_MAT_LAMBERTIAN; m.tex = b.texture_id(tex); m.bump_tex = b.texture_id(bump); m.bump_strength = strength;
        return b.add_material(m);
    }
private:
    shared_ptr<texture> tex, bump; double strength;
};

class metal : public material {
public:
    metal(shared_ptr<texture> a, double f, shared_ptr<texture> bump = nullptr, double strength = 1.0)
        : albedo(a), fuzz(f < 1 ? f : 1), bump(bump), strength(strength) {}
    metal(const color& a, double f, shared_ptr<texture> bump = nullptr, double strength = 1.0)
        : albedo(make_shared<solid_color>(a)), fuzz(f < 1 ? f : 1), bump(bump), strength(strength) {}
    bool scatter(const ray& r_in, const hit_record& rec, color& attenuation, ray& scattered) const override { return zenith::device_scatter(*this, r_in, rec, attenuation, scattered); }
    color get_albedo(const hit_record& rec) const override { return albedo->value(rec.u, rec.v, rec.p); }
    uint32_t flatten(zenith::scene_builder& b) const override {
        zr_material m{}; m.kind = ZR_MAT_METAL; m.tex = b.texture_id(albedo); m.bump_tex = b.texture_id(bump); m.bump_strength = strength; m.param = fuzz;
        return b.add_material(m);
    }
private:
    shared_ptr<texture> albedo; double fuzz; shared_ptr<texture> bump; double strength;
};

class dielectric : public material {
public:
    dielectric(double ri, const color& a = color(1.0, 1.0, 1.0)) : ri(ri), albedo(a), bump(nullptr), strength(1.0) {}
    dielectric(double ri, const color& a, shared_ptr<texture> bump, double strength) : ri(ri), albedo(a), bump(bump), strength(strength) {}
    dielectric(double ri, shared_ptr<texture> bump, double strength) : ri(ri), albedo(1.0, 1.0, 1.0), bump(bump), strength(strength) {}
    bool scatter(const ray& r_in, const hit_record& rec, color& attenuation, ray& scattered) const override { return zenith::device_scatter(*this, r_in, rec, attenuation, scattered); }
    color get_albedo(const hit_record&) const override { return color(1.0, 1.0, 1.0); }
    uint32_t flatten(zenith::scene_builder& b) const override {
        zr_material m{}; m.kind = ZR_MAT_DIELECTRIC; m.tex = ZR_NO_TEXTURE; m.bump_tex = b.texture_id(bump); m.bump_strength = strength; m.param = ri;
        m.tint[0] = albedo.x(); m.tint[1] = albedo.y(); m.tint[2] = albedo.z();
        return b.add_material(m);
    }
private:
    double ri; color albedo; shared_ptr<texture> bump; double strength;
};

class diffuse_light : public material {
public:
    diffuse_light(shared_ptr<texture> a) : emit(a) {}
    diffuse_light(color c) : emit(make_shared<solid_color>(c)) {}
    bool scatter(const ray&, const hit_record&, color&, ray&) const override { return false; }
    color emitted(double u, double v, const point3& p) const override { return emit->value(u, v, p); }
    color get_albedo(const hit_record& rec) const override {
        color c = emit->value(rec.u, rec.v, rec.p);
        return color(std::fmin(c.x(), 1.0), std::fmin(c.y(), 1.0), std::fmin(c.z(), 1.0));
    }
    uint32_t flatten(zenith::scene_builder& b) const override {
        zr_material m{}; m.kind = ZR_MAT_LIGHT; m.tex = b.texture_id(emit); m.bump_tex = ZR_NO_TEXTURE;
        return b.add_material(m);
    }
private:
    shared_ptr<texture> emit;
};

// constant_medium.hpp:9-22
class isovolumetric : public material {
public:
    isovolumetric(color c) : tex(make_shared<solid_color>(c)) {}
    isovolumetric(shared_ptr<texture> t) : tex(t) {}
    bool scatter(const ray& r_in, const hit_record& rec, color& attenuation, ray& scattered) const override { return zenith::device_scatter(*this, r_in, rec, attenuation, scattered); }
    uint32_t flatten(zenith::scene_builder& b) const override {
        zr_material m{}; m.kind = ZR_MAT_ISOTROPIC; m.tex = b.texture_id(tex); m.bump_tex = ZR_NO_TEXTURE;
        return b.add_material(m);
    }
private:
    shared_ptr<texture> tex;
};

inline uint32_t zenith::scene_builder::texture_id(const shared_ptr<texture>& t) {
    if (!t) return ZR_NO_TEXTURE;
    auto it = tex_ids.find(t.get());
    if (it != tex_ids.end()) return it->second;
    uint32_t id = t->flatten(*this);
    tex_ids[t.get()] = id;
    return id;
}
inline uint32_t zenith::scene_builder::material_id(const shared_ptr<material>& m) {
    if (!m) return zenith::no_material;
    if (m.get() == last_mat_) return last_mat_id_;   // (a mesh's triangles share one material: no hash lookup per triangle)
    auto it = mat_ids.find(m.get());
    if (it != mat_ids.end()) { last_mat_ = m.get(); last_mat_id_ = it->second; }
    if (it != mat_ids.end()) return it->second;
    uint32_t id = m->flatten(*this);
    mat_ids[m.get()] = id;
    mat_ptrs[id] = m;
    last_mat_ = m.get(); last_mat_id_ = id;
    return id;
}

// ---- hittable_list.hpp ----------------------------------------------------------------------------
class hittable_list : public hittable {
public:
    std::vector<shared_ptr<hittable>> objects;
    hittable_list() {}
    hittable_list(shared_ptr<hittable> o) { add(o); }
    void clear() { objects.clear(); }
    void add(shared_ptr<hittable> o) { objects.push_back(o); bbox = aabb(bbox, o->bounding_box()); }
    bool hit(const ray& r, interval ray_t, hit_record& rec, int = 0, bool = false) const override { return zenith::device_hit(*this, r, ray_t, rec); }
    aabb bounding_box() const override { return bbox; }
    void flatten(zenith::scene_builder& b) const override;   // (defined after `triangle`: long runs of triangles are flattened by all threads)
private:
    aabb bbox;
};

// ---- sphere.hpp / triangle.hpp / cube.hpp -----------------------------------------------------------
class sphere : public hittable {
public:
    sphere(const point3& center, double radius, shared_ptr<material> mat) : center(center), radius_arg(radius), mat(mat) {
        vec3 rv(radius, radius, radius);
        bbox = aabb(center - rv, center + rv);  // from the raw argument, like sphere.hpp:13-14
    }
    bool hit(const ray& r, interval ray_t, hit_record& rec, int = 0, bool = false) const override { return zenith::device_hit(*this, r, ray_t, rec); }
    aabb bounding_box() const override { return bbox; }
    void set_material(shared_ptr<material> m) { mat = m; zr_device_cache_.reset(); }
    void flatten(zenith::scene_builder& b) const override { b.emit_sphere(center, radius_arg, mat); }
private:
    point3 center; double radius_arg; shared_ptr<material> mat; aabb bbox;
};

namespace zenith { template <class Get> size_t flatten_triangle_run(scene_builder& b, size_t n, Get&& get); }
class triangle : public hittable {
public:
    triangle(const point3& a, const point3& b, const point3& c, const vec3& n0, const vec3& n1, const vec3& n2, shared_ptr<material> m)
        : v{a, b, c}, n{n0, n1, n2}, mat(m) {}   // no texture coordinates: u = v = 0 on every hit, as the reference's triangle::hit leaves them
    // with per-vertex texture coordinates: hits carry the interpolated (u, v) and a tangent frame, so image textures and bump maps work on meshes
    triangle(const point3& a, const point3& b, const point3& c, const vec3& n0, const vec3& n1, const vec3& n2, const zenith::texcoord& t0,
             const zenith::texcoord& t1, const zenith::texcoord& t2, shared_ptr<material> m)
        : v{a, b, c}, n{n0, n1, n2}, mat(m), uv{t0, t1, t2}, has_uv(true) {}
    bool hit(const ray& r, interval ray_t, hit_record& rec, int = 0, bool = false) const override { return zenith::device_hit(*this, r, ray_t, rec); }
    aabb bounding_box() const override {  // triangle.hpp:84-101
        double lo[3], hi[3];
        for (int k = 0; k < 3; k++) {
            lo[k] = std::fmin(v[0][k], std::fmin(v[1][k], v[2][k])); hi[k] = std::fmax(v[0][k], std::fmax(v[1][k], v[2][k]));
            if (hi[k] - lo[k] < 0.0001) { lo[k] -= 0.0001; hi[k] += 0.0001; }
        }
        return aabb(point3(lo[0], lo[1], lo[2]), point3(hi[0], hi[1], hi[2]));
    }
    void set_material(shared_ptr<material> m) { mat = m; zr_device_cache_.reset(); }
    void flatten(zenith::scene_builder& b) const override { b.emit_triangle(v, n, mat, has_uv ? uv : nullptr); }
private:
    template <class Get> friend size_t zenith::flatten_triangle_run(zenith::scene_builder&, size_t, Get&&);
    point3 v[3]; vec3 n[3]; shared_ptr<material> mat;
    zenith::texcoord uv[3]; bool has_uv = false;
};

// A world is flattened once per render, on the caller's clock (the reference rebuilds its world on every restart, main.cpp:1492-1500):
// a million triangles one virtual call at a time took 0.21-0.25 s.  Runs of at least 16384 consecutive `triangle` objects are
// written by all threads instead (same arrays, same order: entry k of the run is triangle first + k), everything else as before.
// a run of triangle objects through the builder's bulk entry: `get(k)` = object k of n.  Returns how many were taken (0: the
// builder wants them one by one, or the first object is no triangle)
namespace zenith {
template <class Get>
inline size_t flatten_triangle_run(scene_builder& b, size_t n, Get&& get) {
    size_t first_tri = 0, first_obj = 0; uint32_t cf = 0, cc = 0; bool entries = true;
    if (n < 16384) return 0;
    { const hittable& head = get(0); if (typeid(head) != typeid(triangle)) return 0; }
    if (!b.begin_bulk_triangles(n, first_tri, first_obj, cf, cc, entries)) return 0;
    // optimistic: room for all n, every thread copies its share and stops at the first object that is not a triangle; the run ends
    // at the earliest such object and the arrays are cut back to it.  Materials are collected as pointers and turned into ids
    // afterwards, in order (registering a material flattens its textures: not a job for worker threads).
    std::vector<const material*> mp(n);
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t T = std::max<size_t>(1, std::min<size_t>(std::min<unsigned>(16u, hw ? hw : 1u), n / 8192));
    std::vector<size_t> stop(T, n);
    std::vector<char> saw_uv(T, 0);   // per thread: one of its triangles carries texture coordinates
    auto work = [&](size_t t, size_t a, size_t e) {
        for (size_t k = a; k < e; k++) {
            const hittable& h = get(k);
            if (typeid(h) != typeid(triangle)) { stop[t] = k; return; }
            const triangle& tr = static_cast<const triangle&>(h);
            double* tv = b.fs.tri_v.data() + (first_tri + k) * 9; double* tn = b.fs.tri_n.data() + (first_tri + k) * 9;
            for (int c = 0; c < 3; c++) { tv[3 * c] = tr.v[c].x(); tv[3 * c + 1] = tr.v[c].y(); tv[3 * c + 2] = tr.v[c].z(); tn[3 * c] = tr.n[c].x(); tn[3 * c + 1] = tr.n[c].y(); tn[3 * c + 2] = tr.n[c].z(); }
            mp[k] = tr.mat.get();
            if (tr.has_uv) saw_uv[t] = 1;
            if (entries) { zr_object o{}; o.type = ZR_PRIM_TRIANGLE; o.index = (uint32_t)(first_tri + k); o.chain_first = cf; o.chain_count = cc; b.fs.objects[first_obj + k] = o; }
        }
    };
    std::vector<std::thread> th;
    for (size_t t = 1; t < T; t++) th.emplace_back(work, t, n * t / T, n * (t + 1) / T);
    work(0, 0, n / T);
    for (auto& x : th) x.join();
    size_t run = n;
    for (size_t t = 0; t < T; t++) if (stop[t] < n) { run = stop[t]; break; }   // (chunks are in order: the first one that stopped ends the run)
    b.end_bulk_triangles(first_tri, run, first_obj + run, entries);
    {   // texture coordinates: a second pass, and only for a world that has any (the array appears with the first triangle that brings some)
        bool any = !b.fs.tri_uv.empty();
        for (size_t t = 0; t < T; t++) any = any || saw_uv[t];   // (a thread may have seen one beyond the run's end: then the array is merely created early, all zero)
        if (any) {
            b.fs.sync_uv(first_tri + run);
            auto uvwork = [&](size_t a, size_t e) {
                for (size_t k = a; k < e; k++) {
                    const triangle& tr = static_cast<const triangle&>(get(k));
                    if (!tr.has_uv) continue;
                    double* q = b.fs.tri_uv.data() + (first_tri + k) * 6;
                    for (int c = 0; c < 3; c++) { q[2 * c] = tr.uv[c].u; q[2 * c + 1] = tr.uv[c].v; }
                }
            };
            std::vector<std::thread> th2;
            for (size_t t = 1; t < T; t++) th2.emplace_back(uvwork, run * t / T, run * (t + 1) / T);
            uvwork(0, run / T);
            for (auto& x : th2) x.join();
        }
    }
    {   // pointers -> ids, in order; the triangle itself is visited again only when its material has not been seen just before
        const material* last = nullptr; uint32_t last_id = 0; bool have = false;
        for (size_t k = 0; k < run; k++) {
            if (!have || mp[k] != last) { last = mp[k]; last_id = b.material_id(static_cast<const triangle&>(get(k)).mat); have = true; }
            b.fs.tri_mat[first_tri + k] = last_id;
        }
    }
    return run;
}
}  // namespace zenith
inline void hittable_list::flatten(zenith::scene_builder& b) const {
    const size_t N = objects.size();
    b.reserve_hint(N);
    // The bulk path costs O(n) for the n entries it is offered (staging array, array growth, thread start) whatever it takes of them, so it is offered only what
    // it will probably take (offered the whole remaining list after every non-triangle member, a long MIXED list cost O(N^2)): a cheap serial look at
    // the next 16384 entries qualifies a run — a shorter run is flattened one by one without being looked at again — and the window offered grows only while
    // the run keeps filling it.
    size_t i = 0, window = 65536;
    while (i < N) {
        const size_t qmax = std::min<size_t>(N - i, 16384);
        size_t q = 0;
        for (; q < qmax; q++) { const hittable& h = *objects[i + q]; if (typeid(h) != typeid(triangle)) break; }
        size_t took = 0;
        if (q == 16384) {
            const size_t n = std::min(N - i, window);
            took = zenith::flatten_triangle_run(b, n, [&](size_t k) -> const hittable& { return *objects[i + k]; });
            window = (took == n) ? std::min<size_t>(window * 4, N) : 65536;
        }
        if (took) { i += took; continue; }
        const size_t one_by_one = std::max<size_t>(q, 1);   // a short run of triangles and / or one other member (or a builder that wants them one by one)
        for (size_t k = 0; k < one_by_one; k++) objects[i + k]->flatten(b);
        i += one_by_one;
    }
}

class cube : public hittable {
public:
    cube(const point3& mn, const point3& mx, shared_ptr<material> mat) : mat(mat), min_p(mn), max_p(mx) {
        half = 0.5 * (mx - mn); center = mn + half;
    }
    cube(const point3& c, shared_ptr<material> mat) : half(1.0, 1.0, 1.0), center(c), mat(mat) { min_p = c - half; max_p = c + half; }
    bool hit(const ray& r, interval ray_t, hit_record& rec, int = 0, bool = false) const override { return zenith::device_hit(*this, r, ray_t, rec); }
    aabb bounding_box() const override {
        return aabb(interval(min_p.x(), max_p.x()).expand(0.0001), interval(min_p.y(), max_p.y()).expand(0.0001),
                    interval(min_p.z(), max_p.z()).expand(0.0001));
    }
    void set_material(shared_ptr<material> m) { mat = m; zr_device_cache_.reset(); }
    void flatten(zenith::scene_builder& b) const override { b.emit_cube(half, center, min_p, max_p, mat); }
private:
    vec3 half; point3 center; shared_ptr<material> mat; point3 min_p, max_p;
};

// ---- constant_medium.hpp ----------------------------------------------------------------------------
class constant_medium : public hittable {
public:
    constant_medium(shared_ptr<hittable> boundary, double density, shared_ptr<texture> tex)
        : boundary(boundary), density(density), phase(make_shared<isovolumetric>(tex)) {}
    constant_medium(shared_ptr<hittable> boundary, double density, color c)
        : boundary(boundary), density(density), phase(make_shared<isovolumetric>(c)) {}
    bool hit(const ray& r, interval ray_t, hit_record& rec, int = 0, bool = false) const override { return zenith::device_hit(*this, r, ray_t, rec); }
    aabb bounding_box() const override { return boundary->bounding_box(); }
    void flatten(zenith::scene_builder& b) const override { b.emit_medium(*boundary, density, b.material_id(phase)); }
private:
    shared_ptr<hittable> boundary; double density; shared_ptr<material> phase;
};

inline void zenith::scene_builder::emit_medium(const hittable& boundary, double density, uint32_t iso_material) {
    if (in_boundary) { unsupported("constant_medium used as the boundary of another medium"); return; }
    in_boundary = true; boundary_base = chain.size(); captured_ok = false;
    size_t objects_before = fs.objects.size();
    boundary.flatten(*this);
    in_boundary = false;
    if (!captured_ok || fs.objects.size() != objects_before || (captured.type != ZR_PRIM_SPHERE && captured.type != ZR_PRIM_CUBE)) {
        unsupported("constant_medium boundary must be one (optionally wrapped) sphere or cube");
        return;
    }
    zr_medium m{};
    m.boundary_type = captured.type; m.boundary_index = captured.index;
    m.chain_first = captured.chain_first; m.chain_count = captured.chain_count;
    m.mat = iso_material; m.neg_inv_density = -1.0 / density;
    fs.media.push_back(m);
    emit(ZR_PRIM_MEDIUM, (uint32_t)fs.media.size() - 1);
}

// ---- wrappers: translate / rotate_* / scale / material_instance --------------------------------------
namespace zenith {
inline aabb rotated_box(const aabb& in, int axis, double s, double c) {
    point3 lo(infinity, infinity, infinity), hi(-infinity, -infinity, -infinity);
    for (int i = 0; i < 2; i++) for (int j = 0; j < 2; j++) for (int k = 0; k < 2; k++) {
        double x = i * in.x.max + (1 - i) * in.x.min, y = j * in.y.max + (1 - j) * in.y.min, z = k * in.z.max + (1 - k) * in.z.min;
        vec3 t(x, y, z);
        if (axis == 1) { t[0] = c * x - s * z; t[2] = s * x + c * z; }  // the true map; rotate_y.hpp:26-27 uses the inverse
        else if (axis == 0) { t[1] = c * y - s * z; t[2] = s * y + c * z; }
        else { t[0] = c * x - s * y; t[1] = s * x + c * y; }
        for (int q = 0; q < 3; q++) { lo[q] = std::fmin(lo[q], t[q]); hi[q] = std::fmax(hi[q], t[q]); }
    }
    return aabb(lo, hi);
}
}  // namespace zenith

class translate : public hittable {
public:
    translate(shared_ptr<hittable> p, const vec3& displacement) : ptr(p), offset(displacement) { bbox = ptr->bounding_box() + offset; }
    bool hit(const ray& r, interval ray_t, hit_record& rec, int = 0, bool = false) const override { return zenith::device_hit(*this, r, ray_t, rec); }
    aabb bounding_box() const override { return bbox; }
    void flatten(zenith::scene_builder& b) const override { b.push_op(ZR_OP_TRANSLATE, offset.x(), offset.y(), offset.z()); ptr->flatten(b); b.pop_op(); }
private:
    shared_ptr<hittable> ptr; vec3 offset; aabb bbox;
};

class rotate_y : public hittable {  // angle in RADIANS (rotate_y.hpp:9-12)
public:
    rotate_y(shared_ptr<hittable> p, double angle_rad) : ptr(p), s(std::sin(angle_rad)), c(std::cos(angle_rad)) {
        bbox = zenith::rotated_box(ptr->bounding_box(), 1, s, c);
    }
    bool hit(const ray& r, interval ray_t, hit_record& rec, int = 0, bool = false) const override { return zenith::device_hit(*this, r, ray_t, rec); }
    aabb bounding_box() const override { return bbox; }
    void flatten(zenith::scene_builder& b) const override { b.push_op(ZR_OP_ROTATE_Y, s, c, 0); ptr->flatten(b); b.pop_op(); }
private:
    shared_ptr<hittable> ptr; double s, c; aabb bbox;
};

class rotate_x : public hittable {  // angle in DEGREES (rotate_x.hpp:9-12)
public:
    rotate_x(shared_ptr<hittable> p, double angle) : ptr(p) {
        double r = degrees_to_radians(angle); s = std::sin(r); c = std::cos(r);
        bbox = zenith::rotated_box(ptr->bounding_box(), 0, s, c);
    }
    bool hit(const ray& r, interval ray_t, hit_record& rec, int = 0, bool = false) const override { return zenith::device_hit(*this, r, ray_t, rec); }
    aabb bounding_box() const override { return bbox; }
    void flatten(zenith::scene_builder& b) const override { b.push_op(ZR_OP_ROTATE_X, s, c, 0); ptr->flatten(b); b.pop_op(); }
private:
    shared_ptr<hittable> ptr; double s, c; aabb bbox;
};

class rotate_z : public hittable {  // angle in DEGREES (rotate_z.hpp:9-12)
public:
    rotate_z(shared_ptr<hittable> p, double angle) : ptr(p) {
        double r = degrees_to_radians(angle); s = std::sin(r); c = std::cos(r);
        bbox = zenith::rotated_box(ptr->bounding_box(), 2, s, c);
    }
    bool hit(const ray& r, interval ray_t, hit_record& rec, int = 0, bool = false) const override { return zenith::device_hit(*this, r, ray_t, rec); }
    aabb bounding_box() const override { return bbox; }
    void flatten(zenith::scene_builder& b) const override { b.push_op(ZR_OP_ROTATE_Z, s, c, 0); ptr->flatten(b); b.pop_op(); }
private:
    shared_ptr<hittable> ptr; double s, c; aabb bbox;
};

class scale : public hittable {
public:
    scale(shared_ptr<hittable> object, const vec3& factors) : object(object), s(factors) {
        aabb in = object->bounding_box();
        bbox = aabb(point3(in.x.min * s.x(), in.y.min * s.y(), in.z.min * s.z()), point3(in.x.max * s.x(), in.y.max * s.y(), in.z.max * s.z()));
    }
    bool hit(const ray& r, interval ray_t, hit_record& rec, int = 0, bool = false) const override { return zenith::device_hit(*this, r, ray_t, rec); }
    aabb bounding_box() const override { return bbox; }
    void flatten(zenith::scene_builder& b) const override { b.push_op(ZR_OP_SCALE, s.x(), s.y(), s.z()); object->flatten(b); b.pop_op(); }
private:
    shared_ptr<hittable> object; vec3 s; aabb bbox;
};

class material_instance : public hittable {
public:
    material_instance(shared_ptr<hittable> obj, shared_ptr<material> mat) : object(obj), new_material(mat) {}
    bool hit(const ray& r, interval ray_t, hit_record& rec, int = 0, bool = false) const override { return zenith::device_hit(*this, r, ray_t, rec); }
    aabb bounding_box() const override { return object->bounding_box(); }
    void set_material(shared_ptr<material> m) { new_material = m; zr_device_cache_.reset(); }
    void flatten(zenith::scene_builder& b) const override {
        // a null material falls back to magenta lambertian (material_instance.hpp:22-26)
        static const shared_ptr<material> error_mat = make_shared<lambertian>(color(1, 0, 1));
        b.push_op(ZR_OP_MATERIAL, 0, 0, 0, b.material_id(new_material ? new_material : error_mat));
        object->flatten(b);
        b.pop_op();
    }
private:
    shared_ptr<hittable> object; shared_ptr<material> new_material;
};

// ---- bvh.hpp: the tree itself is built on the device side of the ABI (zr_scene_commit) ---------------
class bvh_node : public hittable {
public:
    bvh_node(hittable_list l) : list(std::move(l)) { zenith::consume_draws(zenith::bvh_ctor_draws(list.objects.size())); }
    bool hit(const ray& r, interval ray_t, hit_record& rec, int = 0, bool = false) const override { return zenith::device_hit(*this, r, ray_t, rec); }
    aabb bounding_box() const override { return list.bounding_box(); }
    void flatten(zenith::scene_builder& b) const override { b.emit_run(this, [&] { list.flatten(b); }); }
private:
    hittable_list list;
};


// ---- model.hpp: OBJ mesh -> recentred, scaled triangles ------------------------------------------------
// model(filename, mat, scale): /root/reference/model.hpp:12-103.  The reference parses with the vendored
// tiny_obj_loader (float attributes, polygons triangulated); the drop-in has its own minimal Wavefront reader:
// `v x y z [r g b]`, `vn`, `f` with v, v/vt, v//vn, v/vt/vn and negative (relative) indices.  Triangulation follows
// tinyobj 2.0: quads are split along the SHORTER diagonal, compared in float ([0,1,2][0,2,3] if |v2-v0|^2 < |v3-v1|^2,
// else [0,1,3][1,2,3]); polygons with more than four vertices are fanned (tinyobj ear-clips them: documented
// deviation, the reference's assets contain triangles and quads only).
// Semantics kept: the bounding box is taken over ALL `v` lines; x/z are centred on it and y-min moves to 0
// (model.hpp:23-42); vertex = (v - offset) * scale in double (model.hpp:47-53); a face uses its vn normals when
// its first corner has one, otherwise one flat normal unit(cross(v1-v0, v2-v0)) (model.hpp:70-85).
// use_texcoords (off by default: the reference's triangles carry no coordinates, and the worlds that are compared with it are built without): the
// `vt` index of `f v/vt` and `f v/vt/vn` corners is resolved like the others, negative ones from the end of the `vt` lines read so far, and a
// corner's coordinate is (vt.u, 1 - vt.v) from the floats as parsed — OBJ's v = 0 is the bottom of the image, texture::value's the first row.  A
// face with a corner that has no valid `vt` gets zeros; the corners of quads and fans keep their own coordinates through the split.
class model : public hittable {
public:
    model(const std::string& filename, shared_ptr<material> mat, double scale = 1.0, bool use_texcoords = false) : mat(mat) {
        std::vector<float> V, N, VT;
        struct corner { int v, n, t; };
        std::vector<std::vector<corner>> faces;
        std::ifstream f(filename);
        if (!f) { std::cerr << "Cannot load the model: " << filename << std::endl; return; }
        std::string line;
        while (std::getline(f, line)) {
            const char* p = line.c_str();
            while (*p == ' ' || *p == '\t') p++;
            if (p[0] == 'v' && (p[1] == ' ' || p[1] == '\t')) {
                char* e; p += 2;
                for (int k = 0; k < 3; k++) { V.push_back((float)std::strtod(p, &e)); p = e; }
            } else if (p[0] == 'v' && p[1] == 'n' && (p[2] == ' ' || p[2] == '\t')) {
                char* e; p += 3;
                for (int k = 0; k < 3; k++) { N.push_back((float)std::strtod(p, &e)); p = e; }
            } else if (use_texcoords && p[0] == 'v' && p[1] == 't' && (p[2] == ' ' || p[2] == '\t')) {
                char* e; p += 3;
                for (int k = 0; k < 2; k++) { VT.push_back((float)std::strtod(p, &e)); p = e; }
            } else if (p[0] == 'f' && (p[1] == ' ' || p[1] == '\t')) {
                p += 2;
                std::vector<corner> fc;
                for (;;) {
                    while (*p == ' ' || *p == '\t') p++;
                    if (*p == 0 || *p == '\r' || *p == '\n' || *p == '#') break;
                    char* e;
                    long vi = std::strtol(p, &e, 10), ni = 0, ti = 0; bool has_n = false, has_t = false;
                    if (e == p) break;
                    p = e;
                    if (*p == '/') {
                        p++;
                        if (*p != '/') { ti = std::strtol(p, &e, 10); has_t = e != p; p = e; }   // vt
                        if (*p == '/') { p++; ni = std::strtol(p, &e, 10); has_n = e != p; p = e; }
                    }
                    corner c;
                    c.v = vi > 0 ? (int)vi - 1 : (int)(V.size() / 3) + (int)vi;
                    c.n = !has_n ? -1 : (ni > 0 ? (int)ni - 1 : (int)(N.size() / 3) + (int)ni);
                    c.t = !has_t || ti == 0 ? -1 : (ti > 0 ? (int)ti - 1 : (int)(VT.size() / 2) + (int)ti);
                    fc.push_back(c);
                }
                if (fc.size() >= 3) faces.push_back(fc);
            }
        }
        double lo[3] = {infinity, infinity, infinity}, hi[3] = {-infinity, -infinity, -infinity};
        for (size_t i = 0; i + 2 < V.size(); i += 3)
            for (int k = 0; k < 3; k++) { lo[k] = std::fmin(lo[k], V[i + k]); hi[k] = std::fmax(hi[k], V[i + k]); }
        const vec3 off((lo[0] + hi[0]) / 2.0, lo[1], (lo[2] + hi[2]) / 2.0);
        auto vert = [&](int i) { return point3((V[3 * i + 0] - off.x()) * scale, (V[3 * i + 1] - off.y()) * scale, (V[3 * i + 2] - off.z()) * scale); };
        auto norm = [&](int i) { return vec3(N[3 * i + 0], N[3 * i + 1], N[3 * i + 2]); };
        auto valid = [&](const corner& c) { return c.v >= 0 && (size_t)(3 * c.v + 2) < V.size(); };
        auto emit = [&](const corner& a, const corner& b, const corner& c) {
            if (!valid(a) || !valid(b) || !valid(c)) return;
            point3 v0 = vert(a.v), v1 = vert(b.v), v2 = vert(c.v);
            vec3 n0, n1, n2;
            if (a.n >= 0 && b.n >= 0 && c.n >= 0 && (size_t)(3 * std::max(a.n, std::max(b.n, c.n)) + 2) < N.size()) { n0 = norm(a.n); n1 = norm(b.n); n2 = norm(c.n); }
            else n0 = n1 = n2 = unit_vector(cross(v1 - v0, v2 - v0));
            if (use_texcoords) {
                auto has = [&](const corner& q) { return q.t >= 0 && (size_t)(2 * q.t + 1) < VT.size(); };
                auto tc = [&](const corner& q) { return zenith::texcoord{(double)VT[2 * q.t], 1.0 - (double)VT[2 * q.t + 1]}; };
                const bool all = has(a) && has(b) && has(c);
                const zenith::texcoord zero{};
                tris.push_back(make_shared<triangle>(v0, v1, v2, n0, n1, n2, all ? tc(a) : zero, all ? tc(b) : zero, all ? tc(c) : zero, mat));
            } else
            tris.push_back(make_shared<triangle>(v0, v1, v2, n0, n1, n2, mat));
            bbox = aabb(bbox, tris.back()->bounding_box());
        };
        for (const auto& fc : faces) {
            if (fc.size() == 3) emit(fc[0], fc[1], fc[2]);
            else if (fc.size() == 4 && valid(fc[0]) && valid(fc[1]) && valid(fc[2]) && valid(fc[3])) {
                const float* a = &V[3 * fc[0].v]; const float* b = &V[3 * fc[1].v]; const float* c = &V[3 * fc[2].v]; const float* d = &V[3 * fc[3].v];
                const float e02x = c[0] - a[0], e02y = c[1] - a[1], e02z = c[2] - a[2];
                const float e13x = d[0] - b[0], e13y = d[1] - b[1], e13z = d[2] - b[2];
                const float s02 = e02x * e02x + e02y * e02y + e02z * e02z, s13 = e13x * e13x + e13y * e13y + e13z * e13z;
                if (s02 < s13) { emit(fc[0], fc[1], fc[2]); emit(fc[0], fc[2], fc[3]); }
                else { emit(fc[0], fc[1], fc[3]); emit(fc[1], fc[2], fc[3]); }
            } else {
                for (size_t k = 1; k + 1 < fc.size(); k++) emit(fc[0], fc[k], fc[k + 1]);
            }
        }
        zenith::consume_draws(zenith::bvh_ctor_draws(tris.size()));   // mesh_bvh = make_shared<bvh_node>(triangles), model.hpp:95
        std::cout << "Model: " << filename << " loaded (" << tris.size() << " triangles)." << std::endl;
    }
    bool hit(const ray& r, interval ray_t, hit_record& rec, int = 0, bool = false) const override { return zenith::device_hit(*this, r, ray_t, rec); }
    aabb bounding_box() const override { return bbox; }
    void set_material(std::shared_ptr<material> m) { mat = m; }   // like the reference's: does not re-material existing triangles
    void flatten(zenith::scene_builder& b) const override {
        b.emit_run(this, [&] {
            size_t i = 0;
            while (i < tris.size()) {
                const size_t took = zenith::flatten_triangle_run(b, tris.size() - i, [&](size_t k) -> const hittable& { return *tris[i + k]; });
                if (took) { i += took; continue; }
                tris[i]->flatten(b); i++;
            }
        });
    }
    size_t triangle_count() const { return tris.size(); }
private:
    std::vector<shared_ptr<triangle>> tris;
    shared_ptr<material> mat;
    aabb bbox;
};

// ---- environment.hpp ---------------------------------------------------------------------------------
inline const std::string HDR_DIR = "assets/hdr_maps/";
struct EnvironmentSettings {
    enum Mode { PHYSICAL_SUN, HDR_MAP, SOLID_COLOR };
    Mode _mode = PHYSICAL_SUN;
    bool needs_ui_sync = false;
    Mode mode() const { return _mode; }
    void set_mode(Mode m) { if (_mode != m) { _mode = m; needs_ui_sync = true; } }
    color background_color = color(0.0, 0.0, 0.0);
    std::string current_hdr_name = "None";
    std::string current_hdr_path = HDR_DIR;
    double intensity = 1.0;
    double hdri_rotation = 0.0, hdri_tilt = 0.0, hdri_roll = 0.0;
    shared_ptr<image_texture> hdr_texture = nullptr;
    void load_hdr(const std::string& path) {
        if (path.empty()) { set_mode(SOLID_COLOR); background_color = color(0, 0, 0); current_hdr_name = "None (Black)"; return; }
        hdr_texture = make_shared<image_texture>(path.c_str(), true);
        size_t slash = path.find_last_of("/\\");
        current_hdr_name = slash == std::string::npos ? path : path.substr(slash + 1);
        current_hdr_path = path;
        set_mode(HDR_MAP);
    }
    vec3 sun_direction = unit_vector(vec3(1.0, 0.5, -0.5));
    color sun_color = color(1.0, 1.0, 1.0);
    bool auto_sun_color = true;
    double sun_intensity = 1.0;
    double sun_size = 1.0;
};

// post_processor (color_processing.hpp:44-75): the reference's public fields and defaults.  The arithmetic (process, bloom,
// sharpening, analyze_framebuffer) runs on the device: camera::process_framebuffer / camera::analyze below.
struct debug_flags {
    bool red = false, green = false, blue = false, luminance = false, bvh = false;
    bool any_active() const { return red || green || blue || luminance || bvh; }
};
struct image_statistics {
    float average_luminance = 0.0f, max_luminance = 0.0f;
    int histogram[256] = {0};
    float normalized_histogram[256] = {0.0f};
    void normalize() {  // color_processing.hpp:15-27
        int max_pixels = 0;
        for (int i = 0; i < 256; i++) if (histogram[i] > max_pixels) max_pixels = histogram[i];
        if (max_pixels > 0) for (int i = 0; i < 256; i++) normalized_histogram[i] = static_cast<float>(histogram[i]) / max_pixels;
    }
};
struct post_processor {
    mutable float exposure = 0.5f;
    float saturation = 1.0f, contrast = 1.0f, hue_shift = 0.0f, vignette_intensity = 1.0f;
    vec3 color_balance = vec3(1.0f, 1.0f, 1.0f);
    float z_depth_max_dist = 1.0f;
    float exposure_compensation_stops = 0.0f;
    bool use_aces_tone_mapping = false, use_auto_exposure = false;
    float target_luminance = 0.12f;
    mutable debug_flags debug;
    bool use_bloom = false;
    float bloom_threshold = 1.0f, bloom_intensity = 0.3f;
    int bloom_radius = 4;
    bool needs_update = true;
    mutable image_statistics last_stats;
    bool use_sharpening = false;
    double sharpen_amount = 0.2;

    double apply_auto_exposure(const image_statistics& stats) const {  // color_processing.hpp:186-205 (scalar, host)
        if (stats.average_luminance <= 0.0) return static_cast<double>(exposure);
        if (!use_auto_exposure) return std::clamp(static_cast<float>(exposure), 0.01f, 10.0f);
        double safe_luminance = std::max(static_cast<double>(stats.average_luminance), 0.02);
        double raw_exposure = target_luminance / safe_luminance;
        double current_exp = raw_exposure * std::pow(2.0, static_cast<double>(exposure_compensation_stops));
        return std::clamp(static_cast<float>(current_exp), 0.01f, 4.0f);
    }
    zr_post_params to_zr() const {
        zr_post_params p{};
        p.exposure = exposure; p.saturation = saturation; p.contrast = contrast; p.hue_shift = hue_shift; p.vignette_intensity = vignette_intensity;
        p.bloom_threshold = bloom_threshold; p.bloom_intensity = bloom_intensity; p.bloom_radius = bloom_radius;
        for (int k = 0; k < 3; k++) p.color_balance[k] = color_balance[k];
        p.sharpen_amount = sharpen_amount; p.use_aces_tone_mapping = use_aces_tone_mapping; p.use_bloom = use_bloom; p.use_sharpening = use_sharpening;
        p.debug_red = debug.red; p.debug_green = debug.green; p.debug_blue = debug.blue; p.debug_luminance = debug.luminance; p.debug_bvh = debug.bvh;
        return p;
    }
    // post-denoise sharpening (color_processing.hpp:207-227), on the device of the last render (zr_sharpen_frame); defined below
    void apply_sharpening(std::vector<color>& buffer, int width, int height, double amount) const;
};

namespace zenith {
inline zr_env to_zr_env(const EnvironmentSettings& e, scene_builder& b) {
    zr_env z{};
    z.mode = (uint32_t)e._mode;
    z.hdr_texture = e.hdr_texture ? b.texture_id(std::static_pointer_cast<texture>(e.hdr_texture)) : ZR_NO_TEXTURE;
    for (int k = 0; k < 3; k++) { z.background_color[k] = e.background_color[k]; z.sun_direction[k] = e.sun_direction[k]; z.sun_color[k] = e.sun_color[k]; }
    z.intensity = e.intensity; z.hdri_rotation = e.hdri_rotation; z.hdri_tilt = e.hdri_tilt; z.hdri_roll = e.hdri_roll;
    z.sun_intensity = e.sun_intensity; z.sun_size = e.sun_size;
    return z;
}
// Device contexts are kept in ONE process-wide pool, per device ordinal, and LEASED for the duration of a call: the reference
// starts a fresh thread for every render (main.cpp:1520-1531), and a context per thread would create — and free — the
// pipeline's buffers (tens of GB for a 1080p frame at 512 spp) on every restart.  A lease is exclusive (a zr_ctx serves one
// caller at a time); threads that render one after the other reuse the same context, threads that render at the same time get
// one each.  The pool lives as long as the process.
struct context_pool {
    struct entry { zr_ctx* c; int device; bool busy; };
    std::mutex m;
    std::condition_variable cv;
    std::vector<entry> all;
    ~context_pool() { for (entry& e : all) if (e.c) zr_destroy(e.c); }
    zr_ctx* acquire(int device) {
        {
            std::lock_guard<std::mutex> lk(m);
            for (entry& e : all) if (e.device == device && !e.busy) { e.busy = true; return e.c; }
        }
        zr_ctx* c = zr_create(device);   // (outside the lock: creating a context takes milliseconds)
        if (!c) return nullptr;
        std::lock_guard<std::mutex> lk(m);
        all.push_back(entry{c, device, true});
        return c;
    }
    void acquire(zr_ctx* c) {   // a particular context (the one a cached scene was committed on): wait until it is free
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { for (entry& e : all) if (e.c == c) return !e.busy; return true; });
        for (entry& e : all) if (e.c == c) e.busy = true;
    }
    void release(zr_ctx* c) {
        { std::lock_guard<std::mutex> lk(m); for (entry& e : all) if (e.c == c) e.busy = false; }
        cv.notify_all();
    }
    size_t created() { std::lock_guard<std::mutex> lk(m); return all.size(); }
};
inline context_pool& contexts() { static context_pool p; return p; }
// contexts created by this process so far (tests: three renders from three successive threads create one)
inline size_t contexts_created() { return contexts().created(); }
struct context_lease {
    zr_ctx* ctx;
    explicit context_lease(int device) : ctx(contexts().acquire(device)) {}
    explicit context_lease(zr_ctx* c) : ctx(c) { if (c) contexts().acquire(c); }
    context_lease(const context_lease&) = delete;
    context_lease& operator=(const context_lease&) = delete;
    ~context_lease() { if (ctx) contexts().release(ctx); }
    operator zr_ctx*() const { return ctx; }
};
// Flattened worlds are leased from a process-wide stash as well: a camera flattens its world on every render, and reusing the
// arrays of an earlier render saves touching a quarter of a gigabyte of fresh pages for a million triangles.
struct flat_stash { std::mutex m; std::vector<std::unique_ptr<flat_scene>> free; };
inline flat_stash& flat_scenes() { static flat_stash s; return s; }
struct flat_lease {
    std::unique_ptr<flat_scene> fs;
    flat_lease() {
        { std::lock_guard<std::mutex> lk(flat_scenes().m); if (!flat_scenes().free.empty()) { fs = std::move(flat_scenes().free.back()); flat_scenes().free.pop_back(); } }
        if (!fs) fs.reset(new flat_scene()); else fs->clear();
    }
    flat_lease(const flat_lease&) = delete;
    flat_lease& operator=(const flat_lease&) = delete;
    ~flat_lease() { std::lock_guard<std::mutex> lk(flat_scenes().m); if (flat_scenes().free.size() < 2) flat_scenes().free.push_back(std::move(fs)); }
};
// the device hit() / scatter() calls of scene objects use: the one of the camera that rendered last (camera::device), 0 before that
inline std::atomic<int>& object_device() { static std::atomic<int> d{0}; return d; }

// a frame of colours as the C ABI takes it: three doubles per pixel
inline double* doubles(std::vector<color>& frame) { return reinterpret_cast<double*>(frame.data()); }
inline const double* doubles(const std::vector<color>& frame) { return reinterpret_cast<const double*>(frame.data()); }
// the caller's render flag and row counter as the C ABI polls and advances them
static_assert(sizeof(std::atomic<bool>) == 1 && sizeof(std::atomic<int>) == sizeof(int), "flag layout");
inline volatile const uint8_t* flag_ptr(std::atomic<bool>& flag) { return reinterpret_cast<volatile const uint8_t*>(&flag); }
inline volatile int* rows_ptr(std::atomic<int>& rows) { return reinterpret_cast<volatile int*>(&rows); }
// owning handles of the C ABI's scene and accumulator
struct scene_deleter { void operator()(zr_scene* sc) const { zr_scene_destroy(sc); } };   // (frees the scene's device arrays; touches no context state: no lease)
struct accum_deleter { void operator()(zr_accum* acc) const { zr_accum_destroy(acc); } };
struct temporal_deleter { void operator()(zr_temporal* t) const { zr_temporal_destroy(t); } };
using scene_handle = std::unique_ptr<zr_scene, scene_deleter>;
using accum_handle = std::unique_ptr<zr_accum, accum_deleter>;
using temporal_handle = std::unique_ptr<zr_temporal, temporal_deleter>;

// ---- callable hit() / scatter(): one ray through the device ---------------------------------------------------------
// The object is flattened once and committed as a scene of its own (cached in the object, per context; set_material drops
// the cache, any other mutation of a child after the first call needs zenith::forget(obj)).  hit() = zr_trace over
// interval [ray_t.min, ray_t.max] with each primitive's own reading of the bounds; scatter() = zr_kat_scatter with the
// draws taken from the thread's random_double() stream, which is advanced by the number of draws the material made —
// i.e. the call consumes random_double() exactly as the reference's scatter would (common.hpp:29-34, material.hpp).
// A constant_medium draws its distance from the off-stream medium key of the current stream position (zr_rng.h).
struct device_object {
    zr_ctx* ctx = nullptr; scene_handle sc; int device = 0;
    flat_scene fs;
    std::unordered_map<uint32_t, shared_ptr<material>> mats;
};
template <class Flatten>
inline shared_ptr<device_object> device_commit(shared_ptr<device_object>& cache, const char* what, Flatten&& flatten) {
    if (cache && cache->device == object_device().load()) return cache;   // committed before, on a context of this device (which the pool keeps alive)
    context_lease lease(object_device().load());
    zr_ctx* ctx = lease;
    if (!ctx) throw std::runtime_error(std::string(what) + ": no device context: " + zr_last_error());
    auto d = make_shared<device_object>();
    d->ctx = ctx; d->device = object_device().load();
    scene_builder b(d->fs);
    flatten(b);
    b.finish();
    d->mats = b.mat_ptrs;
    for (const auto& w : d->fs.warnings) std::cerr << "[zenith] " << w << "\n";
    d->sc.reset(zr_scene_create(ctx));
    if (!d->sc || d->fs.give_to(d->sc.get()) != ZR_OK || zr_scene_commit(d->sc.get()) != ZR_OK)
        throw std::runtime_error(std::string(what) + ": " + zr_last_error());
    cache = d;
    return d;
}
inline void forget(const hittable& h) { h.zr_device_cache_.reset(); }
inline void forget(const material& m) { m.zr_device_cache_.reset(); }

inline bool device_hit(const hittable& self, const ray& r, const interval& ray_t, hit_record& rec) {
    auto d = device_commit(self.zr_device_cache_, "hittable::hit", [&](scene_builder& b) { self.flatten(b); });
    const double rays6[6] = {r.origin().x(), r.origin().y(), r.origin().z(), r.direction().x(), r.direction().y(), r.direction().z()};
    host_rng& g = rng_state();
    zr_hit h{};
    context_lease lease(d->ctx);   // the object's scene lives on that context: exclusive for the call
    // stream key of this call = (host key, host draw position, 0): a medium's off-stream draw changes as the host stream advances
    if (zr_trace(d->ctx, d->sc.get(), rays6, 1, ray_t.min, ray_t.max, g.key, g.k, 0, &h) != ZR_OK) throw std::runtime_error(std::string("hittable::hit: ") + zr_last_error());
    if (!d->fs.media.empty()) g.k++;   // constant_medium::hit consumes a draw (constant_medium.hpp:64)
    if (h.mat == 0xFFFFFFFFu && h.t == 0.0) return false;
    rec.p = point3(h.p[0], h.p[1], h.p[2]); rec.normal = vec3(h.normal[0], h.normal[1], h.normal[2]);
    rec.tangent = vec3(h.tangent[0], h.tangent[1], h.tangent[2]); rec.bitangent = vec3(h.bitangent[0], h.bitangent[1], h.bitangent[2]);
    rec.t = h.t; rec.u = h.u; rec.v = h.v; rec.front_face = h.front_face != 0;
    auto it = d->mats.find(h.mat);
    rec.mat = it != d->mats.end() ? it->second : nullptr;
    return true;
}

inline bool device_scatter(const material& self, const ray& r_in, const hit_record& rec, vec3& attenuation, ray& scattered) {
    uint32_t id = 0;
    auto d = device_commit(self.zr_device_cache_, "material::scatter", [&](scene_builder& b) { id = self.flatten(b); });
    id = (uint32_t)d->fs.materials.size() - 1;   // a material flattens its textures first and itself last
    const double rays6[6] = {r_in.origin().x(), r_in.origin().y(), r_in.origin().z(), r_in.direction().x(), r_in.direction().y(), r_in.direction().z()};
    zr_hit h{};
    for (int k = 0; k < 3; k++) { h.p[k] = rec.p[k]; h.normal[k] = rec.normal[k]; h.tangent[k] = rec.tangent[k]; h.bitangent[k] = rec.bitangent[k]; }
    h.t = rec.t; h.u = rec.u; h.v = rec.v; h.mat = id; h.front_face = rec.front_face ? 1u : 0u;
    host_rng& g = rng_state();
    zr_scatter_out o{};
    context_lease lease(d->ctx);
    if (zr_kat_scatter(d->ctx, d->sc.get(), rays6, &h, &g.key, &g.k, 1, &o) != ZR_OK) throw std::runtime_error(std::string("material::scatter: ") + zr_last_error());
    g.k += o.draws;
    if (!o.scattered) return false;
    attenuation = vec3(o.attenuation[0], o.attenuation[1], o.attenuation[2]);
    scattered = ray(point3(o.origin[0], o.origin[1], o.origin[2]), vec3(o.direction[0], o.direction[1], o.direction[2]));
    return true;
}
}  // namespace zenith

inline void post_processor::apply_sharpening(std::vector<color>& buffer, int width, int height, double amount) const {
    if (amount <= 0.0) return;   // color_processing.hpp:208-210
    if (width < 1 || height < 1 || buffer.size() != (size_t)width * height) { std::cerr << "[zenith] apply_sharpening: buffer size mismatch\n"; return; }
    zenith::context_lease lease(zenith::object_device().load());
    zr_ctx* ctx = lease;
    double* p = zenith::doubles(buffer);
    if (!ctx || zr_sharpen_frame(ctx, p, width, height, amount, p) != ZR_OK) std::cerr << "[zenith] apply_sharpening failed: " << zr_last_error() << "\n";
}

// ---- camera.hpp: public configuration + render() ------------------------------------------------------
class camera {
public:
    double aspect_ratio = 1.0;
    int image_width = 400, image_height = 225;
    int samples_per_pixel = 30;
    int current_samples_count = 0;
    int max_depth = 10;
    double sky_intesity = 1.0;
    double vfov = 30;
    point3 lookfrom = point3(10, 1.5, 0), lookat = point3(0, 0, 0);
    vec3 vup = vec3(0, 1, 0);
    double defocus_angle = 0.5, focus_dist = 10;
    bool use_denoiser = false;
    bool use_albedo_buffer = false, use_normal_buffer = false, use_z_depth_buffer = false, use_reflection = false, use_refraction = false;
    std::vector<color> render_accumulator;
    std::vector<color> albedo_buffer, normal_buffer, z_depth_buffer;  // first-hit passes (camera.hpp:81-83), filled when their flag is set
    std::vector<color> reflection_buffer, refraction_buffer;          // second-path split (camera.hpp:84-85, 490-517), filled when either flag is set
    std::vector<color> denoise_buffer;   // camera.hpp:80: the denoised copy of render_accumulator, filled when use_denoiser is set (not OIDN)
    std::atomic<int> lines_rendered{0};
    uint64_t seed = 0x5EED0000ull;  // extension: the reference cannot be seeded (common.hpp:30-31)
    int device = 0;                 // extension: HIP device ordinal
    // extension: > 0 renders the frame progressively, this many samples per pass (zr_render_accumulate).  After every pass render_accumulator holds the exact
    // image of the samples done so far, current_samples_count says how many that is, and render_flag is looked at: a cancelled render leaves the
    // current_samples_count-spp image.  The finished frame equals the one-shot frame bit for bit.  0: exactly the one-shot render.
    int samples_per_pass = 0;
    int passes_rendered = 0;        // extension: passes of the last progressive render that reached render_accumulator
    // extension: > 0 renders adaptively (zr_render_adaptive): every pixel gets adaptive_min_samples, then adaptive_step more per pass while its noise estimate (the
    // relative standard error of the pixel mean) is above adaptive_threshold, up to samples_per_pixel rounded down to a multiple of 64 (below 64 the flag is ignored
    // with a warning).  Afterwards render_accumulator is the resolved frame — a pixel that stopped at k samples is that pixel of the k-spp frame, bit for bit —
    // sample_counts holds the per-pixel counts and current_samples_count the largest.  render_flag is looked at between passes.  Takes precedence over
    // samples_per_pass.  0: exactly the render without it.
    double adaptive_threshold = 0;
    int adaptive_min_samples = 64, adaptive_step = 64;
    double adaptive_dark_floor = 0.01;
    std::vector<int> sample_counts;   // extension: samples per pixel of the last adaptive render (row-major like render_accumulator); empty otherwise
    // extension: with use_denoiser, denoise_buffer comes from the variance-guided filter (zr_denoise_guided with its default parameters) when the
    // frame came through an accumulator whose counts are multiples of 64 — adaptive_threshold > 0, or samples_per_pass > 0 with samples_per_pixel a multiple
    // of 64.  variance_buffer then holds the variance of every pixel's mean per channel (zr_accum_variance).  Without such a frame (a one-shot render, another
    // count) a warning is printed and the plain filter runs.  The reflection / refraction frames have no variance and keep the plain filter.  false: exactly
    // the render without it.
    bool denoise_variance_guided = false;
    std::vector<color> variance_buffer;   // extension: filled by a render with use_denoiser and denoise_variance_guided that had a variance; empty otherwise
    bool denoise_used_variance = false;   // extension: the last render's denoise_buffer came from the guided filter
    // extension: with use_denoiser, denoise_buffer comes from the dual-buffer non-local-means filter (zr_denoise_nlm with nlm_params) on a frame
    // that came through an accumulator with a variance (denoise_variance_guided's condition): the two half images of the accumulator filter each other.
    // variance_buffer then holds zr_accum_variance and denoise_error_buffer the filter's estimate of the output's variance per channel.  With both this and
    // denoise_variance_guided set, this one wins.  A temporally accumulated frame has no halves: with temporal_accumulation a warning is printed and the
    // render is what it is without this flag.  Without a variance a warning is printed and the plain filter runs.  The reflection / refraction frames keep
    // the plain filter.  false: exactly the render without it.
    bool denoise_nlm = false;
    zr_denoise_nlm_params nlm_params{ZR_DENOISE_NLM_DEFAULT_SEARCH_RADIUS, ZR_DENOISE_NLM_DEFAULT_PATCH_RADIUS, ZR_DENOISE_NLM_DEFAULT_DEMODULATE, 0,
                                     ZR_DENOISE_NLM_DEFAULT_K, ZR_DENOISE_NLM_DEFAULT_ALPHA, ZR_DENOISE_NLM_DEFAULT_SIGMA_NORMAL,
                                     ZR_DENOISE_NLM_DEFAULT_SIGMA_ALBEDO, ZR_DENOISE_NLM_DEFAULT_EPSILON};
    bool denoise_used_nlm = false;              // extension: the last render's denoise_buffer came from the non-local-means filter
    std::vector<color> denoise_error_buffer;    // extension: zr_denoise_nlm's out_error of the last render; empty when that filter did not run
    // extension: temporal accumulation across render() calls of this camera object (zr_accum_temporal with temporal_params).  A frame that came
    // through an accumulator with a variance (denoise_variance_guided's condition: adaptive_threshold > 0, or samples_per_pass > 0 with samples_per_pixel a
    // multiple of 64) is blended with the history of the frames before it, reprojected through the first hits of this camera's pixels: temporal_buffer holds
    // the blend, variance_buffer its variance and temporal_history_length the frames behind every pixel.  With use_denoiser && denoise_variance_guided the
    // guided filter takes those two in place of the frame's own.  The history belongs to a frame size and a world object (the `world` argument's address): it
    // is dropped when either changes, or on reset_temporal_history() — the caller's duty after editing the world in place (a moving world: see
    // temporal_track_motion below).  Without a
    // variance a warning is printed and the render is what it is without the flag.  render_accumulator is never touched.  false: exactly the render without it.
    bool temporal_accumulation = false;
    zr_temporal_params temporal_params{ZR_TEMPORAL_DEFAULT_ALPHA, ZR_TEMPORAL_DEFAULT_MAX_HISTORY, 0, ZR_TEMPORAL_DEFAULT_PLANE_TOLERANCE, ZR_TEMPORAL_DEFAULT_NORMAL_COS};
    std::vector<color> temporal_buffer;           // extension: the temporally accumulated frame of the last render; empty when it had none
    std::vector<int> temporal_history_length;     // extension: frames accumulated per pixel (row-major like render_accumulator); empty likewise
    void reset_temporal_history() { temporal_.reset(); }
    // extension: moving worlds (zr_scene_update_* / zr_scene_refit).  Off: every render() commits a fresh scene, as always.  On: the camera keeps the
    // committed scene between renders, as it keeps the temporal history; when the newly flattened world equals the kept one in everything but the arguments of
    // its wrappers (a translate's offset, a rotation's angle, a scale's factors) and the numbers of its spheres — the reference's way to move things: the same
    // objects under re-created translate / rotate_y wrappers — it updates the kept scene and refits its trees instead of building them again; any other
    // change, a refused update, another device context or a failed refit commits anew.  last_scene_refit says which it was: 0 committed, 1 refitted.
    // The frame is the same bit for bit either way.  Without temporal_track_motion the temporal history knows no object motion: reset_temporal_history() stays
    // the caller's duty.
    bool reuse_scene = false;
    // extension: the firefly-robust resolve (zr_accum_resolve_robust in ZR_ROBUST_GINI mode with robust_strength).  Wherever render() resolves an
    // accumulator whose counts are multiples of 64 — the adaptive render, and the progressive render after every pass that leaves such a count —
    // render_accumulator receives the Gini-trimmed mean of the pixel's 64 lane sums instead of their plain mean, and the variance handed to
    // denoise_variance_guided, denoise_nlm and temporal_accumulation is the variance of that mean (the half images denoise_nlm reads stay as they are).
    // Without adaptive_threshold and samples_per_pass, a frame of a multiple of 64 samples takes one pass of samples_per_pixel samples through an accumulator;
    // any other frame prints a warning and is rendered as without the flag.  resolve_used_robust says which it was.  A trimmed mean darkens pixels whose
    // samples are genuinely skewed (caustics): opt-in.  false: exactly the render without it.
    bool robust_resolve = false;
    double robust_strength = ZR_ROBUST_DEFAULT_STRENGTH;
    bool resolve_used_robust = false;   // extension: the last render's render_accumulator came from the robust resolve
    // extension: direct light sampling (zr_accum_set_direct with emitters and the sun): next-event estimation with multiple importance sampling
    // on the path the plain integrator walks.  render() then goes through an accumulator as robust_resolve does — the adaptive render, the progressive
    // render, or one pass of samples_per_pixel samples — and everything that reads the accumulator (variance, the guided and non-local-means filters,
    // temporal accumulation, the robust resolve) works on the direct frame.  The reflection / refraction split replays the plain integrator's paths: with
    // use_reflection or use_refraction a warning is printed and the render is what it is without the flag.  render_used_direct says which it was.
    // Same expectation as the plain render, other noise: opt-in.  false: exactly the render without it.
    bool direct_lighting = false;
    bool render_used_direct = false;    // extension: the last render's samples came from the direct-light integrator
    // extension: the direct-light integrator also importance-samples the HDR environment map (zr_accum_set_direct_env).  Takes effect only
    // together with direct_lighting; where the environment has no map to sample the render is direct_lighting's.  render_used_direct_env says whether the
    // switch was set on the last render's accumulator.
    bool direct_environment = false;
    bool render_used_direct_env = false;
    // extension: the temporal history follows a moving world (zr_temporal_track_motion).  Takes effect together with temporal_accumulation and
    // reuse_scene: the camera switches tracking on in the history it keeps, and keeps that history across a frame whose scene was refitted
    // (last_scene_refit == 1) although the `world` argument is a new object — the refit's motion table reprojects the moved objects' pixels.  Every other case
    // is left to the library's restart rule (a new commit, another scene: the frame starts anew).  false: exactly the renders without it.
    bool temporal_track_motion = false;
    int last_scene_refit = 0;
    void forget_scene() { kept_scene_.reset(); kept_ctx_ = nullptr; }
    zr_adaptive_stats last_adaptive{};
    zr_counters last_counters{};

    void reset_accumulator() {  // camera.hpp:209-233
        render_accumulator.assign((size_t)image_width * image_height, color(0, 0, 0));
        denoise_buffer.assign(render_accumulator.size(), color(0, 0, 0));
        albedo_buffer.assign(render_accumulator.size(), color(0, 0, 0));
        normal_buffer.assign(render_accumulator.size(), color(0, 0, 0));
        z_depth_buffer.assign(render_accumulator.size(), color(0, 0, 0));
        reflection_buffer.assign(render_accumulator.size(), color(0, 0, 0));
        refraction_buffer.assign(render_accumulator.size(), color(0, 0, 0));
        current_samples_count = 0; lines_rendered = 0;
    }

    // camera::process_framebuffer_to_image up to the PNG encoder (camera.hpp:701-780): bloom, sharpening, exposure,
    // post_processor::process, 8-bit RGB — on the device, byte-exact with the reference.  Data passes (albedo, normals, z-depth,
    // reflection, refraction) are clamped and gamma-corrected only, as save_render_pass asks (camera.hpp:314-345).
    bool process_framebuffer(const std::vector<color>& buffer, const post_processor& pp, std::vector<unsigned char>& rgb8,
                             bool is_data_pass = false, bool apply_gamma = true) const {
        rgb8.assign((size_t)image_width * image_height * 3, 0);
        zenith::context_lease lease(device);
        zr_ctx* ctx = lease;
        if (!ctx || buffer.size() != (size_t)image_width * image_height) { std::cerr << "[zenith] process_framebuffer: " << (ctx ? "buffer size mismatch" : zr_last_error()) << "\n"; return false; }
        zr_post_params p = pp.to_zr();
        int rc = zr_post_process(ctx, &p, zenith::doubles(buffer), image_width, image_height, is_data_pass, apply_gamma, rgb8.data());
        if (rc != ZR_OK) std::cerr << "[zenith] process_framebuffer failed: " << zr_last_error() << "\n";
        return rc == ZR_OK;
    }
    // post_processor::analyze_framebuffer (color_processing.hpp:150-183) on the device
    image_statistics analyze(const std::vector<color>& buffer) const {
        image_statistics st;
        zenith::context_lease lease(device);
        zr_ctx* ctx = lease;
        zr_image_stats z{};
        if (ctx && !buffer.empty() && zr_analyze_frame(ctx, zenith::doubles(buffer), buffer.size(), &z) == ZR_OK) {
            st.average_luminance = z.average_luminance; st.max_luminance = z.max_luminance;
            for (int i = 0; i < 256; i++) st.histogram[i] = z.histogram[i];
            st.normalize();
        }
        return st;
    }

    // camera.hpp:236.  Blocking; fills render_accumulator (mean radiance, row-major, idx = j*W + i)."
    void render(const hittable& world, const EnvironmentSettings& env, const post_processor& post, std::atomic<bool>& render_flag) {
        if (image_width < 1) image_width = 1;
        if (image_height < 1) image_height = 1;
        aspect_ratio = double(image_width) / image_height;
        lines_rendered = 0;
        render_accumulator.assign(pixels(), color(0, 0, 0));  // the reference only fills (camera.hpp:420)
        const bool stats = std::getenv("ZR_COMMIT_STATS") != nullptr;
        auto now_s = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        double t_ph = now_s();
        auto ph = [&](const char* what) { if (stats) { const double t = now_s(); std::fprintf(stderr, "[zenith] render: %-20s %.1f ms\n", what, (t - t_ph) * 1e3); t_ph = t; } };
        zenith::flat_lease lease_fs;                 // (the arrays of an earlier render of this process are reused: no fresh pages to touch)
        zenith::flat_scene& fs = *lease_fs.fs;
        zenith::scene_builder b(fs);
        world.flatten(b);
        b.finish();
        ph("flatten");
        const zr_env zenv = zenith::to_zr_env(env, b);
        for (const auto& w : fs.warnings) std::cerr << "[zenith] " << w << "\n";
        zenith::object_device() = device;
        // the debug view fills render_accumulator only: the AOV, split-pass and denoise buffers stay as reset_accumulator left them
        // (the reference would feed them the debug frame's records)
        const bool debug = global_settings::bvh_debug_mode;
        guide_frames guides;
        int rc;
        {
            zenith::context_lease lease(device);   // one context of the process-wide pool, exclusively, for this frame
            if (!lease.ctx) { std::cerr << "[zenith] render failed: " << zr_last_error() << "\n"; return; }
            zenith::scene_handle fresh;   // this frame's own scene, unless the camera keeps one (reuse_scene)
            const zr_scene* scene = nullptr;
            last_scene_refit = 0;
            if (reuse_scene) {
                rc = scene_for_frame(lease.ctx, fs);
                scene = kept_scene_.get();
            } else {
                forget_scene();
                fresh.reset(zr_scene_create(lease.ctx));
                rc = fresh ? fs.give_to(fresh.get()) : ZR_E_DEVICE;
                if (rc == ZR_OK) rc = zr_scene_commit(fresh.get());
                scene = fresh.get();
            }
            ph(last_scene_refit ? "update + refit" : "commit");
            if (rc == ZR_OK) {
                const frame_job job{lease.ctx, scene, to_zr(), zenv, render_flag, &world};
                sample_counts.clear();
                variance_buffer.clear(); denoise_used_variance = false;
                half_a_.clear(); half_b_.clear(); denoise_error_buffer.clear(); denoise_used_nlm = false;
                temporal_buffer.clear(); temporal_history_length.clear();
                resolve_used_robust = false; robust_variance_.clear();
                render_used_direct = false; render_used_direct_env = false;
                direct_now_ = direct_lighting && !debug && !(use_reflection || use_refraction);
                if (direct_lighting && !debug && !direct_now_)
                    std::cerr << "[zenith] direct_lighting ignored: the reflection / refraction split replays the plain integrator's paths\n";
                if (debug) rc = render_debug_view(job);
                else if (wants_adaptive()) rc = render_adaptive(job);
                else if (samples_per_pass > 0) rc = render_progressive(job, samples_per_pass);
                else if (robust_resolve && samples_per_pixel >= 64 && samples_per_pixel % 64 == 0) rc = render_progressive(job, samples_per_pixel);
                else if (direct_now_) rc = render_progressive(job, samples_per_pixel < 1 ? 1 : samples_per_pixel);
                else rc = render_one_shot(job);
                if (rc == ZR_OK && !debug && robust_resolve && !resolve_used_robust)
                    std::cerr << "[zenith] robust_resolve ignored: no whole lanes (it needs adaptive_threshold, or a multiple of 64 samples)\n";
                if (!debug) zr_get_counters(lease.ctx, &last_counters);
                if (rc == ZR_OK && !debug && temporal_accumulation && temporal_buffer.empty())
                    std::cerr << "[zenith] temporal_accumulation ignored: no variance (it needs adaptive_threshold, or samples_per_pass with a multiple of 64 samples)\n";
                ph(debug ? "zr_render_bvh_debug" : "zr_render");
                if (rc == ZR_OK && !debug) rc = render_aovs(job, post, guides);
                if (rc == ZR_OK && !debug) rc = render_split_passes(job);
            }
            if (rc != ZR_OK && rc != ZR_E_CANCELLED) std::cerr << "[zenith] render failed: " << zr_last_error() << "\n";
        }   // (the scene is destroyed and the lease ends here: analyze() and the denoiser below take their own)
        if (rc == ZR_OK && post.use_auto_exposure) {   // camera.hpp:258-266
            image_statistics stats = analyze(render_accumulator);
            post.last_stats = stats;
            post.exposure = static_cast<float>(post.apply_auto_exposure(stats));
        }
        if (rc == ZR_OK && use_denoiser && !debug) denoise_frames(post, guides);
    }

private:
    // what the stages of one render share
    struct frame_job {
        zr_ctx* ctx; const zr_scene* sc;
        zr_camera cam; zr_env env;
        std::atomic<bool>& flag;
        const hittable* world;
    };
    // the denoiser's guides when the public AOV buffers are off (the reference would hand OIDN zero guides then)
    struct guide_frames { std::vector<color> albedo, normal; };

    // reuse_scene: the kept scene made to hold the world just flattened — by updates and a refit where only placements changed, else by a commit
    int scene_for_frame(zr_ctx* ctx, const zenith::flat_scene& fs) {
        if (kept_scene_ && kept_ctx_ == ctx && fs.same_but_placements(kept_fs_)) {
            int rc = ZR_OK;
            auto differ = [](const zr_xform_op& a, const zr_xform_op& b) { return std::memcmp(a.a, b.a, sizeof a.a) != 0; };
            for (size_t k = 0; k < fs.ops.size() && rc == ZR_OK;) {   // one update per run of changed ops
                if (!differ(fs.ops[k], kept_fs_.ops[k])) { k++; continue; }
                size_t e = k + 1;
                while (e < fs.ops.size() && differ(fs.ops[e], kept_fs_.ops[e])) e++;
                rc = zr_scene_update_xform_ops(kept_scene_.get(), k, fs.ops.data() + k, e - k);
                k = e;
            }
            const size_t ns = fs.sphere_mat.size();
            for (size_t k = 0; k < ns && rc == ZR_OK;) {
                auto moved = [&](size_t i) { return std::memcmp(&fs.spheres[i * 4], &kept_fs_.spheres[i * 4], 4 * sizeof(double)) != 0; };
                if (!moved(k)) { k++; continue; }
                size_t e = k + 1;
                while (e < ns && moved(e)) e++;
                rc = zr_scene_update_spheres(kept_scene_.get(), k, fs.spheres.data() + k * 4, e - k);
                k = e;
            }
            if (rc == ZR_OK) rc = zr_scene_refit(kept_scene_.get(), nullptr);
            if (rc == ZR_OK) { kept_fs_.ops = fs.ops; kept_fs_.spheres = fs.spheres; last_scene_refit = 1; return ZR_OK; }
            // (a refused update — the world would be stored in another form — or a failed refit: build it anew)
        }
        forget_scene();
        kept_scene_.reset(zr_scene_create(ctx));
        int rc = kept_scene_ ? fs.give_copied_to(kept_scene_.get()) : ZR_E_DEVICE;
        if (rc == ZR_OK) rc = zr_scene_commit(kept_scene_.get());
        if (rc == ZR_OK) { kept_fs_ = fs; kept_ctx_ = ctx; } else forget_scene();
        return rc;
    }

    size_t pixels() const { return (size_t)image_width * image_height; }
    zr_camera to_zr() const {
        zr_camera zc{};
        zc.image_width = image_width; zc.image_height = image_height; zc.samples_per_pixel = samples_per_pixel; zc.max_depth = max_depth;
        zc.vfov = vfov; zc.defocus_angle = defocus_angle; zc.focus_dist = focus_dist;
        for (int k = 0; k < 3; k++) { zc.lookfrom[k] = lookfrom[k]; zc.lookat[k] = lookat[k]; zc.vup[k] = vup[k]; }
        return zc;
    }
    bool wants_adaptive() const {
        if (adaptive_threshold > 0 && samples_per_pixel < 64) std::cerr << "[zenith] adaptive_threshold ignored: samples_per_pixel is below 64\n";
        return adaptive_threshold > 0 && samples_per_pixel >= 64;
    }
    // the variance of the accumulator's pixel means, when the denoiser will ask for it (fetched before the accumulator is destroyed)
    int fetch_variance(zr_accum* acc) {
        if (!(use_denoiser && (denoise_variance_guided || wants_nlm()))) return ZR_OK;
        int rc = ZR_OK;
        if (!robust_variance_.empty()) variance_buffer = robust_variance_;   // (the frame is the robust mean: so is its variance)
        else {
            variance_buffer.assign(pixels(), color(0, 0, 0));
            rc = zr_accum_variance(acc, zenith::doubles(variance_buffer));
        }
        if (rc != ZR_OK) variance_buffer.clear();
        if (rc == ZR_OK && wants_nlm()) {   // and the two half images
            half_a_.assign(pixels(), color(0, 0, 0)); half_b_.assign(pixels(), color(0, 0, 0));
            rc = zr_accum_halves(acc, zenith::doubles(half_a_), zenith::doubles(half_b_));
            if (rc != ZR_OK) { half_a_.clear(); half_b_.clear(); }
        }
        return rc;
    }
    // What the accumulator holds into render_accumulator: with robust_resolve and whole lanes (every count a multiple of 64) the Gini-trimmed mean, and with
    // want_variance the variance of that mean for fetch_variance and accumulate_temporal; else the plain mean
    int resolve_frame(zr_accum* acc, bool whole_lanes, bool want_variance) {
        robust_variance_.clear(); resolve_used_robust = false;
        if (!(robust_resolve && whole_lanes)) return zr_accum_resolve(acc, zenith::doubles(render_accumulator));
        const zr_robust_params rp{ZR_ROBUST_GINI, 0, robust_strength};
        if (want_variance) robust_variance_.assign(pixels(), color(0, 0, 0));
        const int rc = zr_accum_resolve_robust(acc, &rp, zenith::doubles(render_accumulator), want_variance ? zenith::doubles(robust_variance_) : nullptr, nullptr);
        if (rc != ZR_OK) robust_variance_.clear();
        resolve_used_robust = rc == ZR_OK;
        return rc;
    }
    // direct_lighting: the integrator bound to the accumulator a render stage has just made
    int bind_direct(zr_accum* acc) {
        if (!direct_now_) return ZR_OK;
        const zr_direct_params dp{ZR_DIRECT_EMITTERS | ZR_DIRECT_SUN, 0};
        int rc = zr_accum_set_direct(acc, &dp);
        render_used_direct = rc == ZR_OK;
        if (rc == ZR_OK && direct_environment) {
            rc = zr_accum_set_direct_env(acc, 1);
            render_used_direct_env = rc == ZR_OK;
        }
        return rc;
    }
    // the non-local-means filter has been asked for and can run: the blend of temporal_accumulation has no half images
    bool wants_nlm() const { return denoise_nlm && !temporal_accumulation; }

    // the accumulator's frame into this camera's history (made anew when the frame size, the world object or the context differ from the history's)
    int accumulate_temporal(const frame_job& j, zr_accum* acc) {
        if (!temporal_accumulation) return ZR_OK;
        static_assert(sizeof(int) == sizeof(int32_t), "temporal_history_length layout");
        const bool track = temporal_track_motion && reuse_scene;
        const bool same_world = temporal_world_ == j.world || (track && last_scene_refit == 1);   // (a refitted scene is the kept world, moved)
        if (!temporal_ || temporal_ctx_ != j.ctx || !same_world || temporal_w_ != image_width || temporal_h_ != image_height) {
            temporal_.reset(zr_temporal_create(j.ctx, image_width, image_height));
            if (!temporal_) return ZR_E_DEVICE;
            temporal_ctx_ = j.ctx; temporal_w_ = image_width; temporal_h_ = image_height;
        }
        temporal_world_ = j.world;
        if (track || tracking_) { zr_temporal_track_motion(temporal_.get(), track ? 1 : 0); tracking_ = track; }
        temporal_buffer.assign(pixels(), color(0, 0, 0)); variance_buffer.assign(pixels(), color(0, 0, 0)); temporal_history_length.assign(pixels(), 0);
        // (a robust frame goes in from the host with its own variance; the plain one is resolved on the device)
        const int rc = !robust_variance_.empty()
            ? zr_temporal_accumulate(temporal_.get(), &temporal_params, j.sc, &j.cam, seed, zenith::doubles(render_accumulator), zenith::doubles(robust_variance_),
                                     zenith::doubles(temporal_buffer), zenith::doubles(variance_buffer), reinterpret_cast<int32_t*>(temporal_history_length.data()))
            : zr_accum_temporal(acc, temporal_.get(), &temporal_params, j.sc, &j.cam, seed, zenith::doubles(temporal_buffer), zenith::doubles(variance_buffer),
                                reinterpret_cast<int32_t*>(temporal_history_length.data()));
        if (rc != ZR_OK) { temporal_buffer.clear(); variance_buffer.clear(); temporal_history_length.clear(); }
        return rc;
    }

    int render_debug_view(const frame_job& j) {
        const zr_bvh_debug_params dp{global_settings::debug_bvh_level, global_settings::bvh_thickness};
        return zr_render_bvh_debug(j.ctx, j.sc, &j.cam, &j.env, seed, nullptr, &dp, zenith::doubles(render_accumulator), zenith::flag_ptr(j.flag),
                                   zenith::rows_ptr(lines_rendered));
    }
    int render_one_shot(const frame_job& j) {
        return zr_render(j.ctx, j.sc, &j.cam, &j.env, seed, nullptr, 0, zenith::doubles(render_accumulator), zenith::flag_ptr(j.flag), zenith::rows_ptr(lines_rendered));
    }
    int render_adaptive(const frame_job& j) {
        static_assert(sizeof(int) == sizeof(int32_t), "sample_counts layout");
        zr_adaptive_params ap{};
        ap.max_samples = samples_per_pixel / 64 * 64;
        ap.min_samples = std::min(adaptive_min_samples, ap.max_samples); ap.step_samples = adaptive_step;
        ap.threshold = adaptive_threshold; ap.dark_floor = adaptive_dark_floor;
        current_samples_count = 0; passes_rendered = 0;
        const zenith::accum_handle acc(zr_accum_create(j.ctx, image_width, image_height, nullptr));
        if (!acc) return ZR_E_DEVICE;
        if (const int brc = bind_direct(acc.get())) return brc;
        // a cancelled run leaves the image of the passes that completed; a refused one (bad counts) leaves nothing
        const int rc = zr_render_adaptive(j.ctx, j.sc, &j.cam, &j.env, seed, acc.get(), &ap, 0, zenith::flag_ptr(j.flag), &last_adaptive);
        if ((rc == ZR_OK || rc == ZR_E_CANCELLED) && last_adaptive.passes > 0) {
            sample_counts.assign(pixels(), 0);
            int64_t st4[4] = {0, 0, 0, 0};
            int qrc = resolve_frame(acc.get(), true, rc == ZR_OK);   // (an adaptive run's counts are multiples of 64)
            if (qrc == ZR_OK) qrc = zr_accum_sample_counts(acc.get(), reinterpret_cast<int32_t*>(sample_counts.data()));
            if (qrc == ZR_OK) qrc = zr_accum_state(acc.get(), st4);
            if (qrc == ZR_OK && rc == ZR_OK) qrc = fetch_variance(acc.get());
            if (qrc == ZR_OK && rc == ZR_OK) qrc = accumulate_temporal(j, acc.get());
            if (qrc != ZR_OK) return qrc;
            current_samples_count = (int)st4[1]; passes_rendered = (int)last_adaptive.passes;
        }
        if (rc == ZR_OK) lines_rendered = image_height;
        return rc;
    }
    // progressive (the reference's "real-time sample accumulation"): passes of samples_per_pass samples into a device accumulator
    int render_progressive(const frame_job& j, int per_pass) {
        const int spp = samples_per_pixel < 1 ? 1 : samples_per_pixel;
        current_samples_count = 0; passes_rendered = 0;
        const zenith::accum_handle acc(zr_accum_create(j.ctx, image_width, image_height, nullptr));
        if (!acc) return ZR_E_DEVICE;
        if (const int brc = bind_direct(acc.get())) return brc;
        while (current_samples_count < spp) {
            const int n = std::min(per_pass, spp - current_samples_count);
            int rc = zr_render_accumulate(j.ctx, j.sc, &j.cam, &j.env, seed, acc.get(), n, 0, zenith::flag_ptr(j.flag));
            // (a cancelled pass is discarded whole: the image stays the one of the passes before it)
            const int held = current_samples_count + n;
            if (rc == ZR_OK) rc = resolve_frame(acc.get(), held % 64 == 0, held == spp);
            if (rc != ZR_OK) return rc;
            current_samples_count += n; passes_rendered++;
            lines_rendered = current_samples_count < spp ? (int)((long long)image_height * current_samples_count / spp) : image_height;
            if (current_samples_count < spp && !j.flag.load()) return ZR_E_CANCELLED;
        }
        if (spp % 64 != 0) return ZR_OK;
        const int rc = fetch_variance(acc.get());
        return rc == ZR_OK ? accumulate_temporal(j, acc.get()) : rc;
    }
    // the first-hit passes whose flags are set, and the denoiser's guides: the public buffers when their flags are set, `guides` otherwise
    int render_aovs(const frame_job& j, const post_processor& post, guide_frames& guides) {
        std::vector<color>* const albedo = use_albedo_buffer ? &albedo_buffer : use_denoiser ? &guides.albedo : nullptr;
        std::vector<color>* const normal = use_normal_buffer ? &normal_buffer : use_denoiser ? &guides.normal : nullptr;
        std::vector<color>* const zdepth = use_z_depth_buffer ? &z_depth_buffer : nullptr;
        if (!albedo && !normal && !zdepth) return ZR_OK;
        auto cleared = [&](std::vector<color>* frame) -> double* { if (frame) frame->assign(pixels(), color(0, 0, 0)); return frame ? zenith::doubles(*frame) : nullptr; };
        const zr_aov_params ap{post.z_depth_max_dist};
        return zr_render_aov(j.ctx, j.sc, &j.cam, seed, nullptr, &ap, cleared(albedo), cleared(normal), cleared(zdepth));
    }
    // camera.hpp:490: either flag runs the second path and fills BOTH frames; the beauty image is what the reference's loop produces with the
    // flags on (same stream prefix), so it is not rendered again
    int render_split_passes(const frame_job& j) {
        if (!use_reflection && !use_refraction) return ZR_OK;
        reflection_buffer.assign(pixels(), color(0, 0, 0));
        refraction_buffer.assign(pixels(), color(0, 0, 0));
        return zr_render_passes(j.ctx, j.sc, &j.cam, &j.env, seed, nullptr, nullptr, zenith::doubles(reflection_buffer), zenith::doubles(refraction_buffer));
    }
    // camera.hpp:268-291; the a-trous filter of zr_denoise stands in for OIDN.  Each frame is filtered only if the one before succeeded.
    int denoise_frames(const post_processor& post, const guide_frames& guides) {
        const std::vector<color>& ga = use_albedo_buffer ? albedo_buffer : guides.albedo;
        const std::vector<color>& gn = use_normal_buffer ? normal_buffer : guides.normal;
        // (a temporally accumulated frame: the guided filter takes it and its variance in place of the frame's own)
        denoise_buffer = denoise_variance_guided && temporal_buffer.size() == render_accumulator.size() ? temporal_buffer : render_accumulator;
        int rc;
        if (denoise_nlm && temporal_accumulation) std::cerr << "[zenith] denoise_nlm ignored: a temporally accumulated frame has no half images\n";
        if (wants_nlm() && half_a_.size() == render_accumulator.size() && variance_buffer.size() == render_accumulator.size()) {
            denoise_buffer = half_a_;   // filtered in place
            denoise_error_buffer.assign(pixels(), color(0, 0, 0));
            double* p = zenith::doubles(denoise_buffer);
            rc = on_leased_context([&](zr_ctx* ctx) {
                return zr_denoise_nlm(ctx, &nlm_params, p, zenith::doubles(half_b_), zenith::doubles(variance_buffer), zenith::doubles(ga), zenith::doubles(gn),
                                      image_width, image_height, p, zenith::doubles(denoise_error_buffer));
            });
            denoise_used_nlm = rc == ZR_OK;
            if (rc != ZR_OK) denoise_error_buffer.clear();
            half_a_.clear(); half_b_.clear();
        } else if (denoise_variance_guided && variance_buffer.size() == render_accumulator.size()) {
            rc = denoise_guided(denoise_buffer, variance_buffer, ga, gn);
            denoise_used_variance = rc == ZR_OK;
        } else {
            if (wants_nlm())
                std::cerr << "[zenith] denoise_nlm ignored: no variance (it needs adaptive_threshold, or samples_per_pass with a multiple of 64 samples)\n";
            if (denoise_variance_guided)
                std::cerr << "[zenith] denoise_variance_guided ignored: no variance (it needs adaptive_threshold, or samples_per_pass with a multiple of 64 samples)\n";
            rc = denoise(denoise_buffer, ga, gn);
        }
        if (rc == ZR_OK && use_reflection) rc = denoise_split_pass(reflection_buffer, post, ga, gn);
        if (rc == ZR_OK && use_refraction) rc = denoise_split_pass(refraction_buffer, post, ga, gn);
        return rc;
    }
    // a split-pass frame has no variance: the plain filter, then the sharpening the reference applies to it
    int denoise_split_pass(std::vector<color>& frame, const post_processor& post, const std::vector<color>& albedo, const std::vector<color>& normal) const {
        const int rc = denoise(frame, albedo, normal);
        if (rc == ZR_OK && post.use_sharpening) post.apply_sharpening(frame, image_width, image_height, post.sharpen_amount);
        return rc;
    }
    // one call of the denoiser on a context leased for it; a message on failure
    template <class Call>
    int on_leased_context(Call&& call) const {
        zenith::context_lease lease(device);
        const int rc = lease.ctx ? call(lease.ctx) : ZR_E_DEVICE;
        if (rc != ZR_OK) std::cerr << "[zenith] denoise failed: " << zr_last_error() << "\n";
        return rc;
    }
    // apply_denoising (camera.hpp:581-699) in place, with zr_denoise's default parameters
    int denoise(std::vector<color>& buffer, const std::vector<color>& albedo, const std::vector<color>& normal) const {
        const zr_denoise_params dp{ZR_DENOISE_DEFAULT_ITERATIONS, ZR_DENOISE_DEFAULT_DEMODULATE, ZR_DENOISE_DEFAULT_SIGMA_COLOR, ZR_DENOISE_DEFAULT_SIGMA_NORMAL,
                                   ZR_DENOISE_DEFAULT_SIGMA_ALBEDO, 0.0f};
        double* p = zenith::doubles(buffer);
        return on_leased_context([&](zr_ctx* ctx) { return zr_denoise(ctx, &dp, p, zenith::doubles(albedo), zenith::doubles(normal), nullptr, image_width, image_height, p); });
    }
    // the variance-guided filter with zr_denoise_guided's default parameters: `buffer` in place, `variance` left as zr_accum_variance gave it
    int denoise_guided(std::vector<color>& buffer, const std::vector<color>& variance, const std::vector<color>& albedo, const std::vector<color>& normal) const {
        const zr_denoise_guided_params dp{ZR_DENOISE_GUIDED_DEFAULT_ITERATIONS, ZR_DENOISE_GUIDED_DEFAULT_DEMODULATE, ZR_DENOISE_GUIDED_DEFAULT_SIGMA_VARIANCE,
                                          ZR_DENOISE_GUIDED_DEFAULT_SIGMA_NORMAL, ZR_DENOISE_GUIDED_DEFAULT_SIGMA_ALBEDO, 0.0f, ZR_DENOISE_GUIDED_DEFAULT_EPSILON};
        double* p = zenith::doubles(buffer);
        return on_leased_context([&](zr_ctx* ctx) {
            return zr_denoise_guided(ctx, &dp, p, zenith::doubles(variance), zenith::doubles(albedo), zenith::doubles(normal), nullptr, image_width, image_height, p, nullptr);
        });
    }

    // the accumulator's half images between the render and the denoiser of one render() call (denoise_nlm)
    std::vector<color> half_a_, half_b_;
    bool direct_now_ = false;   // this render() call binds the direct-light integrator to its accumulator (direct_lighting, and no split)
    // the variance of the robust mean between the resolve and its readers of one render() call (robust_resolve)
    std::vector<color> robust_variance_;
    // the history of temporal_accumulation and what it was made for
    zenith::temporal_handle temporal_;
    // the scene reuse_scene keeps, the context it lives on and the flattened world it holds
    zenith::scene_handle kept_scene_;
    zr_ctx* kept_ctx_ = nullptr;
    zenith::flat_scene kept_fs_;
    zr_ctx* temporal_ctx_ = nullptr; const hittable* temporal_world_ = nullptr; int temporal_w_ = 0, temporal_h_ = 0;
    bool tracking_ = false;   // the switch was set in a history this camera made
};
