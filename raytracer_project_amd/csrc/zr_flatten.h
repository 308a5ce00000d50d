// zr_flatten.h — from the caller's world list to the arrays the kernels read: the classification of world entries (bare / baked / placed / wrapped),
// validation, the commit plan both builders work from, the Flattener, which turns the builder's tree into sibling-pair records, 4-wide quantised nodes and
// the primitive arrays in leaf order, and the host builder's CPU half.  An entry's bounding box and its stored record are zr_entry.h's, shared with the
// device builder.  No HIP in here: zr_commit.cpp includes it for the library, tests/native/flatten_check.cpp compiles it with zr_bvh.cpp alone.
#pragma once
#include "zr_entry.h"
#include "zr_scene_input.h"

namespace {

// the host's arrays as the entry rules read them (zr_entry.h); group_box: per zr_group the box of its triangles in their own space, or null
inline zr::BuildSceneIn scene_view(const SceneInput& s, const std::vector<zr::BuildBox>* group_box = nullptr) {
    zr::BuildSceneIn in;
    in.spheres = s.spheres.data(); in.sphere_mat = s.sphere_mat.data();
    in.tri_v = s.tri_v.data(); in.tri_n = s.tri_n.data(); in.tri_mat = s.tri_mat.data(); in.tri_uv = s.tri_uv.empty() ? nullptr : s.tri_uv.data();
    in.cubes = s.cubes.data(); in.cube_mat = s.cube_mat.data(); in.media = s.media.data(); in.ops = s.ops.data();
    if (group_box && !group_box->empty()) in.group_box = group_box->data()->lo;
    return in;
}

inline float f_down(double x) {
    float f = (float)x;
    if ((double)f > x) f = std::nextafterf(f, -std::numeric_limits<float>::infinity());
    return std::nextafterf(f, -std::numeric_limits<float>::infinity());
}
inline float f_up(double x) {
    float f = (float)x;
    if ((double)f < x) f = std::nextafterf(f, std::numeric_limits<float>::infinity());
    return std::nextafterf(f, std::numeric_limits<float>::infinity());
}

// what a world-list entry becomes in the tree: its leaf kind, and whether the host stores it "baked" (0 as is, 1 baked triangle,
// 2 material-only chain, 3 baked sphere, 4 placed cube) — see zr_entry.h: put_triangle under a chain, put_baked_sphere, put_pcube
inline void classify_object(const SceneInput& s, const zr_object& o, bool bake, uint32_t& kind, uint8_t& baked) {
    kind = o.chain_count ? ZR_KIND_WRAPPED : o.type;
    baked = 0;
    if (o.type == ZR_PRIM_GROUP) { kind = ZR_KIND_INSTANCE; return; }   // placed as one object, whatever its chain
    if (!bake || o.chain_count == 0) return;
    if (o.type == ZR_PRIM_TRIANGLE) {   // see zr_entry.h put_triangle
        bool ok = true;
        for (uint32_t q = 0; q < o.chain_count; q++) if (s.ops[o.chain_first + q].kind == ZR_OP_SCALE) ok = false;
        if (ok) { baked = 1; kind = ZR_PRIM_TRIANGLE; }
    }
    if (o.type == ZR_PRIM_SPHERE) {   // see zr_entry.h put_baked_sphere
        bool ok = true, moved = false; uint32_t mat = s.sphere_mat[o.index], translates = 0;
        for (int q = (int)o.chain_count - 1; q >= 0 && ok; q--) {
            const zr_xform_op& op = s.ops[o.chain_first + q];
            if (op.kind == ZR_OP_SCALE) { ok = op.a[0] > 0 && op.a[0] == op.a[1] && op.a[1] == op.a[2]; moved = true; }
            else if (op.kind == ZR_OP_TRANSLATE) { moved = true; translates++; }
            else if (op.kind == ZR_OP_MATERIAL) mat = op.mat;
            else ok = false;
        }
        if (ok && moved && translates <= 1 && mat < 0x7FFFFFFFu) { baked = 3; kind = ZR_PRIM_SPHERE; }
    }
    if (o.type == ZR_PRIM_CUBE) {   // see zr_entry.h put_pcube: [translate], [translate, rotate_y], each optionally followed by a scale — outermost first
        int pat = 0; bool ok = true;   // 0 nothing yet, 1 translate seen, 2 translate then rotate_y seen, 3 ... then a scale (the innermost wrapper)
        for (uint32_t q = 0; q < o.chain_count && ok; q++) {
            const zr_xform_op& op = s.ops[o.chain_first + q];
            const uint32_t kd = op.kind;
            if (kd == ZR_OP_MATERIAL) continue;
            if (kd == ZR_OP_TRANSLATE && pat == 0) pat = 1;
            else if (kd == ZR_OP_ROTATE_Y && pat == 1) pat = 2;
            else if (kd == ZR_OP_SCALE && (pat == 1 || pat == 2) && op.a[0] != 0.0 && op.a[1] != 0.0 && op.a[2] != 0.0) pat = 3;
            else ok = false;
        }
        if (ok && pat >= 1) { baked = 4; kind = ZR_KIND_PCUBE; }
    }
    if (!baked && (o.type == ZR_PRIM_SPHERE || o.type == ZR_PRIM_CUBE)) {
        bool only_material = true;
        for (uint32_t q = 0; q < o.chain_count; q++) if (s.ops[o.chain_first + q].kind != ZR_OP_MATERIAL) only_material = false;
        if (only_material) { baked = 2; kind = o.type; }
    }
}

inline int validate(const SceneInput& s, const std::vector<zr_object>& objs) {
    const size_t nm = s.materials.size(), nt = s.textures.size();
    auto mat_ok = [&](uint32_t m) { return m == 0xFFFFFFFFu || m < nm; };
    for (uint32_t m : s.sphere_mat) if (!mat_ok(m)) return fail(ZR_E_INVALID, "sphere material id %u out of range", m);
    for (uint32_t m : s.tri_mat) if (!mat_ok(m)) return fail(ZR_E_INVALID, "triangle material id %u out of range", m);
    for (uint32_t m : s.cube_mat) if (!mat_ok(m)) return fail(ZR_E_INVALID, "cube material id %u out of range", m);
    auto chain_ok = [&](uint32_t cf, uint32_t cn) {
        if (cn > ZR_MAX_CHAIN || (size_t)cf + cn > s.ops.size()) return false;
        for (uint32_t k = 0; k < cn; k++) {
            const zr_xform_op& op = s.ops[cf + k];
            if (op.kind > ZR_OP_MATERIAL) return false;
            if (op.kind == ZR_OP_MATERIAL && !mat_ok(op.mat)) return false;
        }
        return true;
    };
    auto prim_ok = [&](uint32_t type, uint32_t idx) {
        switch (type) {
            case ZR_PRIM_SPHERE: return idx < s.sphere_mat.size();
            case ZR_PRIM_TRIANGLE: return idx < s.tri_mat.size();
            case ZR_PRIM_CUBE: return idx < s.cube_mat.size();
            case ZR_PRIM_MEDIUM: return idx < s.media.size();
            case ZR_PRIM_GROUP: return idx < s.groups.size();
            default: return false;
        }
    };
    for (const zr_medium& m : s.media) {
        if (m.boundary_type != ZR_PRIM_SPHERE && m.boundary_type != ZR_PRIM_CUBE) return fail(ZR_E_INVALID, "medium boundary must be a sphere or a cube");
        if (!prim_ok(m.boundary_type, m.boundary_index) || !chain_ok(m.chain_first, m.chain_count) || !mat_ok(m.mat))
            return fail(ZR_E_INVALID, "medium references out of range (or wrapper chain longer than %d)", ZR_MAX_CHAIN);
    }
    for (const zr_group& g : s.groups)
        if (g.triangle_count == 0 || (size_t)g.first_triangle + g.triangle_count > s.tri_mat.size()) return fail(ZR_E_INVALID, "group of triangles out of range (or empty)");
    if (!s.groups.empty() && !s.objects_set) return fail(ZR_E_INVALID, "groups need an explicit world list (zr_scene_set_objects)");
    for (const zr_object& o : objs)
        if (!prim_ok(o.type, o.index) || !chain_ok(o.chain_first, o.chain_count))
            return fail(ZR_E_INVALID, "world-list entry references out of range (or wrapper chain longer than %d)", ZR_MAX_CHAIN);
    for (const zr_material& m : s.materials) {
        if (m.kind > ZR_MAT_ISOTROPIC) return fail(ZR_E_INVALID, "unknown material kind %u", m.kind);
        if (m.kind != ZR_MAT_DIELECTRIC && m.tex >= nt) return fail(ZR_E_INVALID, "material texture id out of range");
        if (m.bump_tex != ZR_NO_TEXTURE && m.bump_tex >= nt) return fail(ZR_E_INVALID, "material bump texture id out of range");
    }
    for (const zr_texture& t : s.textures) {
        if (t.kind > ZR_TEX_IMAGE_F32) return fail(ZR_E_INVALID, "unknown texture kind %u", t.kind);
        if (t.kind == ZR_TEX_CHECKER && (t.odd >= nt || t.even >= nt)) return fail(ZR_E_INVALID, "checker child texture out of range");
        if (t.kind >= ZR_TEX_IMAGE_U8 && t.width && t.height) {
            const unsigned id = (unsigned)(&t - s.textures.data());
            // texture::value indexes texels with int arithmetic (texture.hpp:60-66)
            if (t.width > (uint32_t)INT_MAX || t.height > (uint32_t)INT_MAX) return fail(ZR_E_INVALID, "image texture %u: %u x %u texels, each dimension is at most INT_MAX", id, t.width, t.height);
            // offset + width * height * texel <= blob size, with no sum or product that can wrap: width * height * texel <= room
            // <=> width <= (room / texel) / height in integer division
            const uint64_t texel = t.kind == ZR_TEX_IMAGE_F32 ? 12 : 3, have = s.texels.size();
            if (t.texel_offset > have || t.width > (have - t.texel_offset) / texel / t.height) return fail(ZR_E_INVALID, "image texture %u: texels out of range", id);
            if (t.kind == ZR_TEX_IMAGE_F32 && (t.texel_offset & 3)) return fail(ZR_E_INVALID, "float texels must be 4-byte aligned");
        }
    }
    // Every texture tree is one the device can walk (zr_device.h tex_value): at most ZR_MAX_CHECKER_DEPTH checkers above any leaf, and no cycle.
    // depth[t] = checkers on the longest way from t down to a leaf, by a depth-first walk on an explicit stack (a chain can be as long as the table).
    {
        enum : uint8_t { NEW = 0, OPEN = 1, DONE = 2 };
        std::vector<uint8_t> state(nt, NEW);
        std::vector<uint32_t> depth(nt, 0), stack;
        for (uint32_t root = 0; root < nt; root++) {
            if (state[root] != NEW) continue;
            stack.push_back(root);
            while (!stack.empty()) {
                const uint32_t id = stack.back();
                const zr_texture& t = s.textures[id];
                if (t.kind != ZR_TEX_CHECKER) { state[id] = DONE; stack.pop_back(); continue; }
                if (state[id] == NEW) {
                    state[id] = OPEN;
                    for (uint32_t c : {t.odd, t.even}) {
                        if (state[c] == OPEN) return fail(ZR_E_INVALID, "checker texture %u is its own descendant (through texture %u)", c, id);
                        if (state[c] == NEW) stack.push_back(c);
                    }
                    continue;
                }
                if (state[id] == OPEN) {   // both children are done
                    depth[id] = 1 + std::max(depth[t.odd], depth[t.even]);
                    if (depth[id] > ZR_MAX_CHECKER_DEPTH)
                        return fail(ZR_E_INVALID, "texture %u: %u checkers above a leaf, at most %d can be walked", id, depth[id], ZR_MAX_CHECKER_DEPTH);
                    state[id] = DONE;
                }
                stack.pop_back();
            }
        }
    }
    return ZR_OK;
}

// ZR_COMMIT_STATS: one line on stderr per phase of a commit, "[zr] <who>: <phase, padded to `width`> <time> ms"
struct PhaseTimer {
    const char* who; int width;
    double t0 = now();
    bool on = std::getenv("ZR_COMMIT_STATS") != nullptr;
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    void operator()(const char* what) { if (on) { const double t = now(); std::fprintf(stderr, "[zr] %s: %-*s %.1f ms\n", who, width, what, (t - t0) * 1e3); t0 = t; } }
};

// [0, n) split evenly over up to 16 threads (one below 65 536 items): fn(begin, end), the first part on the caller
template <class F>
void parallel_split(size_t n, F&& fn) {
    const int T = n < 65536 ? 1 : (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (int t = 1; t < T; t++) th.emplace_back([&fn, n, t, T]() { fn(n * t / T, n * (t + 1) / T); });
    fn((size_t)0, n / T);
    for (auto& x : th) x.join();
}

// The build knobs the two builders share: a frame must not depend on which builder made the tree, so neither has defaults of its own — these are the only ones.
struct BuildKnobs {
    bool bake;                  // ZR_BAKE_TRIANGLES (classify_object)
    double ct, ck[8];           // SAH cost of a traversal step and of testing one object of kind k
    int max_leaf, leaf_cap[8];  // objects per leaf; per kind, 0 = max_leaf
    double open_ratio;          // 4-wide collapse (Flattener::open_ratio, BuildParams::open_ratio)
};
inline BuildKnobs read_build_knobs() {
    BuildKnobs kn;
    kn.bake = env_double("ZR_BAKE_TRIANGLES", 1) != 0;
    kn.ct = env_double("ZR_BVH_COST_TRAVERSE", 1.0);
    const double ck[8] = {env_double("ZR_BVH_COST_SPHERE", 1.0), env_double("ZR_BVH_COST_TRI", 1.5), env_double("ZR_BVH_COST_CUBE", 1.0),
                          env_double("ZR_BVH_COST_MEDIUM", 3.0), env_double("ZR_BVH_COST_WRAPPED", 3.0), env_double("ZR_BVH_COST_PCUBE", 1.5),
                          env_double("ZR_BVH_COST_GROUP", 16.0), 1};
    kn.max_leaf = (int)env_double("ZR_BVH_MAX_LEAF", 4);
    // cubes, media and wrapped objects are few, large and dear to test: one per leaf, so that a ray only tests those whose own box it enters
    const int big = (int)env_double("ZR_BVH_MAX_LEAF_BIG", 1);
    const int leaf_cap[8] = {0, 0, big, big, big, big, 1, 0};   // a placement is always a leaf of its own (EXTEND enters it as a whole)
    for (int k = 0; k < 8; k++) { kn.ck[k] = ck[k]; kn.leaf_cap[k] = leaf_cap[k]; }
    kn.open_ratio = env_double("ZR_BVH_OPEN_RATIO", 1.25);
    return kn;
}

// the world list: the caller's, or every primitive that is not a medium's boundary, then the media
inline std::vector<zr_object> world_list(const SceneInput& s) {
    std::vector<zr_object> objs;
    if (s.objects_set) { objs.assign(s.objects.begin(), s.objects.end()); return objs; }
    std::vector<char> sb(s.sphere_mat.size(), 0), cb(s.cube_mat.size(), 0);
    for (const zr_medium& m : s.media) {
        if (m.boundary_type == ZR_PRIM_SPHERE && m.boundary_index < sb.size()) sb[m.boundary_index] = 1;
        if (m.boundary_type == ZR_PRIM_CUBE && m.boundary_index < cb.size()) cb[m.boundary_index] = 1;
    }
    for (uint32_t k = 0; k < s.sphere_mat.size(); k++) if (!sb[k]) objs.push_back({ZR_PRIM_SPHERE, k, 0, 0});
    for (uint32_t k = 0; k < s.tri_mat.size(); k++) objs.push_back({ZR_PRIM_TRIANGLE, k, 0, 0});
    for (uint32_t k = 0; k < s.cube_mat.size(); k++) if (!cb[k]) objs.push_back({ZR_PRIM_CUBE, k, 0, 0});
    for (uint32_t k = 0; k < s.media.size(); k++) objs.push_back({ZR_PRIM_MEDIUM, k, 0, 0});
    return objs;
}

// What both builders work from, computed once per commit (after validate): the world list, the knobs, what every entry becomes, and from that the final
// length of every primitive array.  Arrays of 8 are indexed by leaf kind (ZR_PRIM_* / ZR_KIND_*).
struct CommitPlan {
    std::vector<zr_object> objs;
    BuildKnobs kn;
    std::vector<uint8_t> code;   // per entry: leaf kind | baked << 4 (classify_object) — the form the device builder reads
    uint32_t cnt[8] = {};        // leaf objects
    size_t inner[8] = {};        // primitives inside media and wrapper chains: stored behind the leaf ranges (and, for triangles, behind the groups' runs)
    size_t group_tris = 0;       // triangles of all groups: behind the leaf triangles
    size_t size[8] = {};         // records of each kind's array
    uint32_t kind(size_t k) const { return code[k] & 7u; }
};
inline std::shared_ptr<CommitPlan> make_plan(const SceneInput& s, std::vector<zr_object>&& objs) {
    auto plan = std::make_shared<CommitPlan>();
    CommitPlan& p = *plan;
    p.objs = std::move(objs); p.kn = read_build_knobs(); p.code.resize(p.objs.size());
    std::atomic<uint32_t> cnt[8] = {};
    parallel_split(p.objs.size(), [&](size_t k0, size_t k1) {
        uint32_t c[8] = {};
        for (size_t k = k0; k < k1; k++) { uint32_t kind; uint8_t bk; classify_object(s, p.objs[k], p.kn.bake, kind, bk); p.code[k] = (uint8_t)(kind | (bk << 4)); c[kind & 7]++; }
        for (int k = 0; k < 8; k++) cnt[k] += c[k];
    });
    for (int k = 0; k < 8; k++) p.cnt[k] = cnt[k];
    auto count_inner = [&](uint32_t type, uint32_t idx, auto&& self) -> void {
        p.inner[type]++;
        if (type == ZR_PRIM_MEDIUM) self(s.media[idx].boundary_type, s.media[idx].boundary_index, self);
    };
    if (p.cnt[ZR_PRIM_MEDIUM] + p.cnt[ZR_KIND_WRAPPED])   // (a million-entry scan for nothing otherwise)
        for (size_t k = 0; k < p.objs.size(); k++) {
            const zr_object& o = p.objs[k];
            if (p.kind(k) == ZR_PRIM_MEDIUM) count_inner(s.media[o.index].boundary_type, s.media[o.index].boundary_index, count_inner);
            else if (p.kind(k) == ZR_KIND_WRAPPED) count_inner(o.type, o.index, count_inner);
        }
    for (const zr_group& g : s.groups) p.group_tris += g.triangle_count;
    for (int k = 0; k < 8; k++) p.size[k] = p.cnt[k] + p.inner[k];
    p.size[ZR_PRIM_TRIANGLE] += p.group_tris;
    return plan;
}

// flattens the build tree into sibling-pair records and 4-wide nodes and, leaf by leaf, the primitive arrays in leaf order.
// Built for commit latency like the builder (zr_bvh.cpp): one cheap serial walk fixes every index (pair numbers in pre-order,
// each leaf's range in its kind's array), then the primitive records, the pair records and the 4-wide nodes (whose shape
// depends on quantisation trials) are produced by all threads; nothing is appended under a lock.  The arrays are
// zr::RawArray (no zero-fill).  The result is the same as a serial depth-first emit, whatever the number of threads.
struct Flattener {
    const SceneInput& s;
    const std::vector<zr_object>& objs;
    const zr::BuildResult& br;
    zr::RawArray<zr::NodePair> pairs;
    std::vector<zr::NodeQ> quads;
    zr::RawArray<uint32_t> leaf_first; // per build node: device index of a leaf's first primitive
    int quad_depth = 0;
    zr::RawArray<double> spheres, tri_v, tri_s, cubes, pcubes;
    const zr::BuildSceneIn in = scene_view(s);   // what the entry rules (zr_entry.h) read ...
    zr::BuildPrimOut out;                        // ... and where they write: the arrays above and below (allocate_arrays; a group's flattener: the world's, base[] moved)
    zr::RawArray<uint32_t> sphere_mat, cube_mat, pcube_mat;
    zr::RawArray<zr::DMedium> media;
    zr::RawArray<zr::DWrapped> wrapped;
    zr::RawArray<zr::DInstance> insts;
    std::vector<uint32_t> inst_group;                     // per placement: its group
    const std::vector<zr::BuildResult>* runs = nullptr;   // per zr_group: the tree over its triangles (object space), built by the caller
    std::vector<uint32_t> run_root;                       // per group: pair index of its subtree's root
    std::vector<uint32_t> run_tri_base, run_qroot, run_demand;   // per group: first triangle (device index), its root among the 4-wide nodes, its worst-case stack entries
    std::vector<std::vector<zr_object>> run_objs;         // per group, while run() works: its triangles as a world list of bare entries ...
    std::vector<std::unique_ptr<Flattener>> run_fl;       // ... and the flattener of its tree over them: leaf order, pair records and 4-wide nodes on local indices
    bool root_in_array = false;                           // a group's own flattener: the root is a quantised node like any other (quads[0])
    size_t n_sph = 0, n_tri = 0, n_cube = 0, n_media = 0;   // filled sizes of the arrays that grow behind their leaf ranges (the arrays are sized exactly)
    std::function<void()> after_primitives;   // called by run() once spheres / triangles / cubes / media / wrapped are complete
    const CommitPlan* commit_plan = nullptr;       // the world's flattener: sizes, and per object code >> 4 = 0 as is, 1 baked triangle, 2 material-only chain, 3 baked sphere, 4 placed cube
    bool want_src = false;                         // fill src: per leaf kind, each leaf primitive's index in the caller's arrays (zr_scene::leaf_src)
    std::vector<uint32_t> src[8];
    int threads = 1;

    // Workers that live as long as run(): the level-synchronous passes below call parallel_for some forty times, and starting
    // thirty-one threads each time cost more than the passes' own work (plan + numbering 34 ms -> see profiles/r2_commit_stats.txt).
    struct Pool {
        std::vector<std::thread> th;
        std::mutex m;
        std::condition_variable go, done;
        std::function<void(int)> job;
        uint64_t gen = 0;
        int parts = 0, pending = 0;
        bool stop = false;
        explicit Pool(int workers) {
            for (int w = 1; w <= workers; w++)
                th.emplace_back([this, w]() {
                    uint64_t seen = 0;
                    for (;;) {
                        std::function<void(int)> f;
                        {
                            std::unique_lock<std::mutex> lk(m);
                            go.wait(lk, [&] { return stop || gen != seen; });
                            if (stop) return;
                            seen = gen;
                            if (w >= parts) continue;
                            f = job;
                        }
                        f(w);
                        { std::lock_guard<std::mutex> lk(m); if (--pending == 0) done.notify_one(); }
                    }
                });
        }
        ~Pool() {
            { std::lock_guard<std::mutex> lk(m); stop = true; }
            go.notify_all();
            for (auto& x : th) x.join();
        }
        void run(int n_parts, const std::function<void(int)>& f) {   // f(0 .. n_parts - 1), part 0 on the caller
            { std::lock_guard<std::mutex> lk(m); job = f; parts = n_parts; pending = n_parts - 1; gen++; }
            go.notify_all();
            f(0);
            std::unique_lock<std::mutex> lk(m);
            done.wait(lk, [&] { return pending == 0; });
        }
    };
    mutable std::unique_ptr<Pool> pool;
    template <class F>
    void parallel_for(size_t n, size_t grain, F&& fn) const {   // fn(begin, end) over [0, n) split evenly
        int T = threads;
        if (n < 2 * grain) T = 1; else T = (int)std::min<size_t>((size_t)T, n / grain);
        if (T <= 1) { fn((size_t)0, n); return; }
        if (pool && T <= (int)pool->th.size() + 1) {
            pool->run(T, [&fn, n, T](int t) { fn(n * (size_t)t / (size_t)T, n * (size_t)(t + 1) / (size_t)T); });
            return;
        }
        std::vector<std::thread> th;
        for (int t = 1; t < T; t++) th.emplace_back([&fn, n, t, T]() { fn(n * t / T, n * (t + 1) / T); });
        fn((size_t)0, n / T);
        for (auto& x : th) x.join();
    }

    // a primitive that is not a leaf object itself — a medium's boundary, the object inside a wrapper chain — goes behind the leaf
    // ranges of its kind's array (serial: such objects are few)
    uint32_t append_inner(uint32_t type, uint32_t idx) {
        switch (type) {
            case ZR_PRIM_SPHERE: zr::put_sphere(in, out, n_sph, idx, zr::kKeepMaterial); return (uint32_t)n_sph++;
            case ZR_PRIM_TRIANGLE: zr::put_triangle(in, out, n_tri, idx); return (uint32_t)n_tri++;
            case ZR_PRIM_CUBE: zr::put_cube(in, out, n_cube, idx, zr::kKeepMaterial); return (uint32_t)n_cube++;
            default: { const size_t di = n_media++; put_medium(di, idx); return (uint32_t)di; }
        }
    }
    void put_medium(size_t di, uint32_t idx) {
        const zr_medium& m = s.media[idx];
        zr::DMedium d{};
        d.btype = m.boundary_type; d.chain_first = m.chain_first; d.chain_count = m.chain_count;
        d.mat = m.mat; d.id = idx; d.neg_inv_density = m.neg_inv_density;
        d.bindex = append_inner(m.boundary_type, m.boundary_index);
        media[di] = d;
    }
    // The compound leaf objects — media, wrapped objects — with the primitives they contain, which go behind the leaf ranges: serial, in the order given.
    // The order decides where the inner primitives land, so each builder keeps its own: the host's is the leaves' emit order, the device's media before
    // wrapped objects, each in array order.
    struct Compound { uint32_t kind, di, oi; };   // leaf kind, index in its kind's array, world-list entry
    void finish_compounds(const std::vector<Compound>& todo) {
        for (const Compound& c : todo) {
            const zr_object& o = objs[c.oi];
            zr::note_src(out, c.kind, c.di, c.oi, o);
            if (c.kind == ZR_PRIM_MEDIUM) { put_medium(c.di, o.index); continue; }
            zr::DWrapped w{};
            w.type = o.type; w.chain_first = o.chain_first; w.chain_count = o.chain_count;
            w.index = append_inner(o.type, o.index);
            wrapped[c.di] = w;
        }
    }
    // the primitive arrays at the plan's sizes (untouched pages cost nothing), the fill counters at the ends of the leaf ranges
    void allocate_arrays(const CommitPlan& p) {
        const size_t* z = p.size;
        spheres.allocate(z[ZR_PRIM_SPHERE] * ZR_SPHERE_DOUBLES); sphere_mat.allocate(z[ZR_PRIM_SPHERE]);
        const size_t uv = s.tri_uv.empty() ? 0 : 6;   // the triangles' texture coordinates, 6 per stored triangle, behind the last shading record
        tri_v.allocate(z[ZR_PRIM_TRIANGLE] * ZR_TRI_STRIDE); tri_s.allocate(z[ZR_PRIM_TRIANGLE] * (ZR_TRI_SHADE_DOUBLES + uv));
        cubes.allocate(z[ZR_PRIM_CUBE] * ZR_CUBE_DOUBLES); cube_mat.allocate(z[ZR_PRIM_CUBE]);
        pcubes.allocate(z[ZR_KIND_PCUBE] * ZR_PCUBE_STRIDE); pcube_mat.allocate(z[ZR_KIND_PCUBE]);
        media.allocate(z[ZR_PRIM_MEDIUM]); wrapped.allocate(z[ZR_KIND_WRAPPED]);
        n_sph = p.cnt[ZR_PRIM_SPHERE]; n_tri = p.cnt[ZR_PRIM_TRIANGLE]; n_cube = p.cnt[ZR_PRIM_CUBE]; n_media = p.cnt[ZR_PRIM_MEDIUM];
        out.spheres = spheres.data(); out.sphere_mat = sphere_mat.data(); out.tri_v = tri_v.data(); out.tri_s = tri_s.data();
        out.tri_uv = uv && z[ZR_PRIM_TRIANGLE] ? tri_s.data() + z[ZR_PRIM_TRIANGLE] * ZR_TRI_SHADE_DOUBLES : nullptr;
        out.cubes = cubes.data(); out.cube_mat = cube_mat.data(); out.pcubes = pcubes.data(); out.pcube_mat = pcube_mat.data();
    }
    bool plain_media() const {   // every medium's boundary is an unwrapped sphere or cube
        for (size_t k = 0; k < media.size(); k++) if (media[k].chain_count != 0) return false;
        return true;
    }
    bool filled(const CommitPlan& p) const {   // every array ended exactly where the plan said it would
        return n_sph == p.size[ZR_PRIM_SPHERE] && n_tri == p.size[ZR_PRIM_TRIANGLE] && n_cube == p.size[ZR_PRIM_CUBE] && n_media == p.size[ZR_PRIM_MEDIUM];
    }

    // ---- the serial walk: pair numbers in pre-order, leaf ranges per kind, in the order a depth-first emit would visit them ----
    std::vector<int32_t> inner;        // inner build nodes, position = pair index
    zr::RawArray<uint32_t> pair_of;    // per build node
    std::vector<int32_t> leaves;       // leaf build nodes in emit order
    uint32_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // leaf objects per kind
    // Pair index of every inner node, first-primitive index of every leaf, and the two lists, in the order of a depth-first walk
    // (node, left subtree, right subtree).  The builder numbers nodes so that this order IS ascending node id (left = id + 1,
    // right = id + 2 x the left subtree's references: zr_bvh.cpp), with unused ids in between — fresh pages, all zero, which no
    // real node is (a leaf has count > 0, an inner node left = id + 1 > 0) — so the walk is two passes of prefix sums over the
    // id range, every thread on its own slice, instead of a serial recursion over two million nodes.
    void index_nodes() {
        static_assert(zr::NodeArray::zero_filled, "the unused ids between real nodes must read as zero (neither leaf nor inner)");
        const size_t N = br.nodes.size();
        const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, threads), N / 65536 + 1));
        struct Tally { size_t inner = 0, leaves = 0; uint32_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0}; };
        std::vector<Tally> tally((size_t)T);
        auto is_inner = [&](size_t id) { const zr::BuildNode& n = br.nodes[id]; return n.count == 0 && n.left == (int32_t)id + 1; };
        auto pass = [&](auto&& body) {
            std::vector<std::thread> th;
            for (int t = 1; t < T; t++) th.emplace_back([&body, t, T, N]() { body(t, N * (size_t)t / (size_t)T, N * (size_t)(t + 1) / (size_t)T); });
            body(0, (size_t)0, N / (size_t)T);
            for (auto& x : th) x.join();
        };
        pass([&](int t, size_t a, size_t b) {
            Tally y;
            for (size_t id = a; id < b; id++) {
                const zr::BuildNode& n = br.nodes[id];
                if (n.count) { y.leaves++; y.cnt[n.kind & 7] += n.count; } else if (is_inner(id)) y.inner++;
            }
            tally[(size_t)t] = y;
        });
        Tally run;
        std::vector<Tally> start((size_t)T);
        for (int t = 0; t < T; t++) {
            start[(size_t)t] = run;
            run.inner += tally[(size_t)t].inner; run.leaves += tally[(size_t)t].leaves;
            for (int k = 0; k < 8; k++) run.cnt[k] += tally[(size_t)t].cnt[k];
        }
        inner.resize(run.inner); leaves.resize(run.leaves);
        for (int k = 0; k < 8; k++) cnt[k] = run.cnt[k];
        pass([&](int t, size_t a, size_t b) {
            Tally y = start[(size_t)t];
            for (size_t id = a; id < b; id++) {
                const zr::BuildNode& n = br.nodes[id];
                if (n.count) { leaf_first[id] = y.cnt[n.kind & 7]; y.cnt[n.kind & 7] += n.count; leaves[y.leaves++] = (int32_t)id; }
                else if (is_inner(id)) { pair_of[id] = (uint32_t)y.inner; inner[y.inner++] = (int32_t)id; }
            }
        });
    }
    void fill_pair(uint32_t p, int32_t node_id) {
        const int32_t ch[2] = {br.nodes[node_id].left, br.nodes[node_id].right};
        for (int slot = 0; slot < 2; slot++) {
            const zr::BuildNode& n = br.nodes[ch[slot]];
            for (int k = 0; k < 3; k++) { pairs[p].lo[slot][k] = f_down(n.box.lo[k]); pairs[p].hi[slot][k] = f_up(n.box.hi[k]); }
            if (n.count) { pairs[p].child[slot] = leaf_first[ch[slot]]; pairs[p].meta[slot] = ((n.kind + 1u) << 16) | n.count; }
            else { pairs[p].child[slot] = pair_of[ch[slot]]; pairs[p].meta[slot] = 0; }
        }
    }
    void empty_child(uint32_t pair, int slot) {
        for (int k = 0; k < 3; k++) { pairs[pair].lo[slot][k] = 0.f; pairs[pair].hi[slot][k] = 0.f; }
        pairs[pair].child[slot] = 0;
        pairs[pair].meta[slot] = (1u << 16) | 0u;  // leaf with zero primitives
    }
    // ---- 4-wide nodes: collapse of the binary tree (largest-area internal child is opened first) ----
    static double area(const zr::BuildBox& b) {
        double dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
        return dx * dy + dy * dz + dz * dx;
    }
    // 8-bit planes of one axis: origin + q * scale, as a real number, must not exceed lo (lower plane) and must
    // reach hi (upper plane).  The comparison is the real one, as the device builder's is (zr_quant.h: plane_le, plane_ge): a = origin and m = q * scale
    // are exact doubles and TwoSum gives a + m = s + e exactly.  (A sum in long double is not exact: an origin just below 0 — f_down(0) is the
    // smallest subnormal — vanishes beside q * scale, and an upper plane that lay 2^-149 below hi passed for reaching it.)
    static long double plane(float origin, float scale, long q) { return (long double)origin + (long double)q * (long double)scale; }
    static void plane_sum(float origin, float scale, long q, double& s, double& e) {
        const double a = (double)origin, m = (double)q * (double)scale;
        s = a + m;
        const double bb = s - a;
        e = (a - (s - bb)) + (m - bb);
    }
    static bool plane_le(float origin, float scale, long q, double x) { double s, e; plane_sum(origin, scale, q, s, e); return s < x || (s == x && e <= 0.0); }
    static bool plane_ge(float origin, float scale, long q, double x) { double s, e; plane_sum(origin, scale, q, s, e); return s > x || (s == x && e >= 0.0); }
    static bool quant_axis(const double* lo, const double* hi, int n, float& origin, float& scale, uint8_t* qlo, uint8_t* qhi) {
        double mn = lo[0], mx = hi[0];
        for (int k = 1; k < n; k++) { mn = std::min(mn, lo[k]); mx = std::max(mx, hi[k]); }
        if (!std::isfinite(mn) || !std::isfinite(mx) || std::fabs(mn) > 1e30 || std::fabs(mx) > 1e30) return false;
        origin = f_down(mn);
        const double ext = mx - (double)origin;
        int e = ext > 0 ? (int)std::ceil(std::log2(ext / 255.0)) : -100;
        const int emin = origin != 0.0f ? std::max(-100, std::ilogb(origin) - 30) : -100;
        if (e < emin) e = emin;
        for (int tries = 0; tries < 64; tries++, e++) {
            scale = std::ldexp(1.0f, e);
            bool ok = true;
            for (int k = 0; k < n && ok; k++) {
                long ql = (long)std::floor((lo[k] - (double)origin) / (double)scale);
                ql = std::min(255l, std::max(0l, ql));
                while (ql > 0 && !plane_le(origin, scale, ql, lo[k])) ql--;
                if (!plane_le(origin, scale, ql, lo[k])) ok = false;
                long qh = (long)std::ceil((hi[k] - (double)origin) / (double)scale);
                qh = std::min(255l, std::max(0l, qh));
                while (qh < 255 && !plane_ge(origin, scale, qh, hi[k])) qh++;
                if (!plane_ge(origin, scale, qh, hi[k])) ok = false;
                qlo[k] = (uint8_t)ql; qhi[k] = (uint8_t)qh;
            }
            if (ok) return true;
        }
        return false;
    }
    double open_ratio = 1.25;  // a child is not opened when that would put a box on the grid with more than this times its true area
    zr::NodeF root{};
    size_t n_kept_closed = 0;
    // quantises the boxes of `kids` into nq; false when a box cannot be represented; *worst = largest area inflation
    bool quantise(const int32_t* kids, int nk, zr::NodeQ& nq, double* worst) const {
        uint8_t ql[3][4] = {}, qh[3][4] = {};
        for (int k = 0; k < 6; k++) nq.q[k] = 0;
        for (int ax = 0; ax < 3; ax++) {
            double lo[4], hi[4];
            for (int k = 0; k < nk; k++) { lo[k] = br.nodes[kids[k]].box.lo[ax]; hi[k] = br.nodes[kids[k]].box.hi[ax]; }
            if (!quant_axis(lo, hi, nk, nq.origin[ax], nq.scale[ax], ql[ax], qh[ax])) return false;
            for (int k = 0; k < nk; k++) { nq.q[ax] |= (uint32_t)ql[ax][k] << (8 * k); nq.q[3 + ax] |= (uint32_t)qh[ax][k] << (8 * k); }
        }
        *worst = 1;
        for (int k = 0; k < nk; k++) {
            zr::BuildBox qb;
            for (int ax = 0; ax < 3; ax++) {
                qb.lo[ax] = (double)plane(nq.origin[ax], nq.scale[ax], ql[ax][k]);
                qb.hi[ax] = (double)plane(nq.origin[ax], nq.scale[ax], qh[ax][k]);
            }
            const double at = area(br.nodes[kids[k]].box), aq = area(qb);
            const double r = at > 0 ? aq / at : (aq > 0 ? 1e300 : 1.0);
            if (!(r <= *worst)) *worst = r;
        }
        return true;
    }
    std::atomic<bool> quant_ok_a{true};   // false: a box below the root is not finite (the caller falls back to variant 0)
    bool quant_ok = true;
    std::atomic<size_t> kept_closed_a{0};
    // ---- 4-wide nodes.  Which children a node takes depends on quantisation trials, so a node's shape is only known once it is
    // planned; planning is level-synchronous — every node of a level in parallel, the inner children forming the next level — and
    // a serial pre-order walk then numbers the nodes and fills in the child references. ----
    struct QuadPlan { int32_t kids[4]; int nk; zr::NodeQ nq; };
    zr::RawArray<QuadPlan> plan;         // per build node (only quad roots are filled; not zero-filled)
    void plan_quad(int32_t node_id, bool is_root, QuadPlan& qp) const {
        int32_t* kids = qp.kids; int nk = 0;
        zr::NodeQ nq{};
        for (int ax = 0; ax < 3; ax++) nq.scale[ax] = 1;
        if (br.nodes[node_id].count) {   // a tree that is a single leaf: as a stored root (a group's) a node with one child
            kids[nk++] = node_id;
            double w = 1;
            if (!is_root && !quantise(kids, nk, nq, &w)) const_cast<Flattener*>(this)->quant_ok_a = false;
        } else {
            nk = 2;
            kids[0] = br.nodes[node_id].left; kids[1] = br.nodes[node_id].right;
            double worst = 1;
            if (!is_root && !quantise(kids, nk, nq, &worst)) const_cast<Flattener*>(this)->quant_ok_a = false;
            while (nk < 4) {
                // open the inner child with the largest area, unless the grid of the wider node would be too coarse
                // for one of the boxes (then the child keeps its own node, whose grid fits its own children)
                int best = -1; double ba = -1;
                for (int k = 0; k < nk; k++) if (br.nodes[kids[k]].count == 0 && area(br.nodes[kids[k]].box) > ba) { ba = area(br.nodes[kids[k]].box); best = k; }
                if (best < 0) break;
                int32_t trial[4];
                for (int k = 0; k < nk; k++) trial[k] = kids[k];
                trial[best] = br.nodes[kids[best]].left; trial[nk] = br.nodes[kids[best]].right;
                if (!is_root) {
                    zr::NodeQ tq = nq; double w = 1;
                    if (!quantise(trial, nk + 1, tq, &w)) { const_cast<Flattener*>(this)->quant_ok_a = false; break; }
                    if (w > open_ratio && w > worst) { const_cast<Flattener*>(this)->kept_closed_a++; break; }
                    nq = tq; worst = w;
                }
                for (int k = 0; k <= nk; k++) kids[k] = trial[k];
                nk++;
            }
        }
        qp.nk = nk; qp.nq = nq;
    }
    // Numbering: pre-order, as a serial depth-first emit would number them — node index = parent's index + 1 + the sizes of the
    // subtrees of its earlier inner siblings (the root has none: its first child is node 0).  Subtree sizes come from a pass over the
    // planned levels bottom-up, indices from a pass top-down, the records are written by all threads.
    std::vector<std::vector<int32_t>> levels;     // planned quad roots, level by level (levels[0] = {root})
    zr::RawArray<uint32_t> q_size, q_index;       // per build node: quads in its subtree (itself included), its own index
    void plan_quads(int32_t root_id) {
        plan.allocate(br.nodes.size());
        levels.clear();
        levels.push_back(std::vector<int32_t>{root_id});
        bool first = !root_in_array;
        for (;;) {
            const std::vector<int32_t>& level = levels.back();
            const int T = std::max(1, threads);
            std::vector<std::vector<int32_t>> out((size_t)T);
            std::atomic<int> slot{0};
            parallel_for(level.size(), 256, [&](size_t a2, size_t b2) {
                std::vector<int32_t>& mine = out[(size_t)slot.fetch_add(1)];
                for (size_t i = a2; i < b2; i++) {
                    QuadPlan& qp = plan[level[i]];
                    plan_quad(level[i], first, qp);
                    for (int k = 0; k < qp.nk; k++) if (br.nodes[qp.kids[k]].count == 0) mine.push_back(qp.kids[k]);
                }
            });
            std::vector<int32_t> next;
            for (auto& v : out) next.insert(next.end(), v.begin(), v.end());
            first = false;
            if (next.empty()) break;
            levels.push_back(std::move(next));
        }
    }
    void number_quads(int32_t root_id) {
        q_size.allocate(br.nodes.size()); q_index.allocate(br.nodes.size());
        for (size_t l = levels.size(); l-- > 0;) {   // bottom-up: subtree sizes
            const std::vector<int32_t>& level = levels[l];
            parallel_for(level.size(), 2048, [&](size_t a2, size_t b2) {
                for (size_t i = a2; i < b2; i++) {
                    const QuadPlan& qp = plan[level[i]];
                    uint32_t n = 1;
                    for (int k = 0; k < qp.nk; k++) if (br.nodes[qp.kids[k]].count == 0) n += q_size[qp.kids[k]];
                    q_size[level[i]] = n;
                }
            });
        }
        const size_t n_quads = (size_t)q_size[root_id] - (root_in_array ? 0 : 1);   // the world's root travels in the kernel arguments
        q_index[root_id] = root_in_array ? 0u : 0xFFFFFFFFu;                        // ... so that its first child becomes node 0
        quads.resize(n_quads);
        for (size_t l = 0; l < levels.size(); l++) {           // top-down: indices, and the records themselves
            const std::vector<int32_t>& level = levels[l];
            parallel_for(level.size(), 1024, [&](size_t a2, size_t b2) {
                for (size_t i = a2; i < b2; i++) {
                    const int32_t node_id = level[i];
                    const QuadPlan& qp = plan[node_id];
                    uint32_t refs[4] = {ZR_REF_EMPTY, ZR_REF_EMPTY, ZR_REF_EMPTY, ZR_REF_EMPTY};
                    uint32_t next = q_index[node_id] + 1u;
                    for (int k = 0; k < qp.nk; k++) {
                        const zr::BuildNode& n = br.nodes[qp.kids[k]];
                        if (n.count) refs[k] = ZR_REF_LEAF | ((uint32_t)n.kind << 28) | ((uint32_t)(n.count - 1u) << 24) | leaf_first[qp.kids[k]];
                        else { refs[k] = next; q_index[qp.kids[k]] = next; next += q_size[qp.kids[k]]; }
                    }
                    if (l == 0 && !root_in_array) {
                        for (int k = 0; k < qp.nk; k++) {
                            const zr::BuildBox& bb = br.nodes[qp.kids[k]].box;
                            root.lox[k] = f_down(bb.lo[0]); root.loy[k] = f_down(bb.lo[1]); root.loz[k] = f_down(bb.lo[2]);
                            root.hix[k] = f_up(bb.hi[0]); root.hiy[k] = f_up(bb.hi[1]); root.hiz[k] = f_up(bb.hi[2]);
                        }
                        for (int k = 0; k < 4; k++) root.ref[k] = refs[k];
                    } else {
                        zr::NodeQ nq = qp.nq;
                        for (int k = 0; k < 4; k++) nq.ref[k] = refs[k];
                        quads[q_index[node_id]] = nq;
                    }
                }
            });
        }
        quad_depth = (int)levels.size() - 1;
        quant_ok = quant_ok_a.load(); n_kept_closed = kept_closed_a.load();
    }
    // Worst-case number of entries the EXTEND kernel's per-lane stack holds for this 4-wide tree: visiting a node whose
    // nk children are all hit pushes nk - 1 of them and descends into the nearest (any child can be the nearest), or
    // pushes all nk when the nearest is a leaf and the lane already holds a postponed leaf (zr_stream.hip).
    // demand(node) = max(nk, max over inner children c of nk - 1 + demand(c)); exact, by DFS over the emitted nodes.
    uint32_t demand_of(const uint32_t refs[4]) const {
        uint32_t nk = 0, best = 0;
        for (int k = 0; k < 4; k++) if (refs[k] != ZR_REF_EMPTY) nk++;
        for (int k = 0; k < 4; k++) {
            if (refs[k] == ZR_REF_EMPTY) continue;
            if (refs[k] & ZR_REF_LEAF) {   // a placed run: one sentinel entry, then the run's own tree on the same stack (zr_stream.hip, level 3)
                if (((refs[k] >> 28) & 7u) == ZR_KIND_INSTANCE && !run_demand.empty() && !insts.empty()) {
                    const uint32_t g = inst_group[refs[k] & 0xFFFFFFu];
                    best = std::max(best, 1u + run_demand[g]);
                }
                continue;
            }
            best = std::max(best, demand_of(quads[refs[k]].ref));
        }
        return std::max(nk, nk ? nk - 1 + best : 0u);
    }
    uint32_t stack_demand() const { return demand_of(root.ref); }
    int run() {   // the world's flattener (needs `commit_plan`)
        PhaseTimer ph{"flatten", 18};
        {
            unsigned hw = std::thread::hardware_concurrency();
            if (const char* e = std::getenv("ZR_BVH_THREADS")) hw = (unsigned)std::max(1, std::atoi(e));
            threads = (int)std::max(1u, std::min(32u, hw));
        }
        if (threads > 1 && br.nodes.size() > 65536) pool.reset(new Pool(threads - 1));
        struct Unpool { std::unique_ptr<Pool>& p; ~Unpool() { p.reset(); } } unpool{pool};   // the workers end with run()
        if (br.nodes.empty()) {
            pairs.allocate(1); empty_child(0, 0); empty_child(0, 1);
            for (int k = 0; k < 4; k++) root.ref[k] = ZR_REF_EMPTY;
            return ZR_OK;
        }
        // 1. indices: the world's tree, and every group's by a flattener of its own over the group's triangles — the world's own code, on indices local to the group
        index_tree();
        const size_t ng = runs ? runs->size() : 0;
        run_objs.resize(ng); run_fl.resize(ng);
        for (size_t g = 0; g < ng; g++) {
            const zr_group& grp = s.groups[g];
            run_objs[g].reserve(grp.triangle_count);
            for (uint32_t k = 0; k < grp.triangle_count; k++) run_objs[g].push_back({ZR_PRIM_TRIANGLE, grp.first_triangle + k, 0, 0});
            run_fl[g].reset(new Flattener{s, run_objs[g], (*runs)[g]});
            run_fl[g]->open_ratio = open_ratio; run_fl[g]->root_in_array = true;
            run_fl[g]->index_tree();
        }
        ph("index pass");
        // 2. the arrays at the plan's sizes; what the walk counted must be what the plan classified
        for (int k = 0; k < 8; k++)
            if (cnt[k] != commit_plan->cnt[k]) return fail(ZR_E_DEVICE, "flattener: %u leaf objects of kind %d, the plan has %u (internal error)", cnt[k], k, commit_plan->cnt[k]);
        allocate_arrays(*commit_plan);
        insts.allocate(cnt[ZR_KIND_INSTANCE]); inst_group.assign(cnt[ZR_KIND_INSTANCE], 0);
        out.insts = insts.data(); out.inst_group = inst_group.data();
        if (want_src) for (int k = 0; k < 8; k++) { src[k].assign(commit_plan->size[k], 0xFFFFFFFFu); out.src[k] = src[k].data(); }
        // every group's records follow the world's own, its triangles the leaf triangles: where each group's start
        run_root.resize(ng); run_tri_base.resize(ng); run_qroot.resize(ng); run_demand.resize(ng);
        size_t n_pairs = std::max<size_t>(1, inner.size());
        for (size_t g = 0; g < ng; g++) {
            run_root[g] = (uint32_t)n_pairs; n_pairs += std::max<size_t>(1, run_fl[g]->inner.size());
            run_tri_base[g] = (uint32_t)n_tri; n_tri += s.groups[g].triangle_count;
            run_fl[g]->out = out; run_fl[g]->out.base[ZR_PRIM_TRIANGLE] = run_tri_base[g];
        }
        pairs.allocate(n_pairs);
        // 3. leaf primitives of the plain kinds: all threads; a group's triangles in the order of its leaves (serial: groups are shared, hence few)
        put_leaves();
        for (size_t g = 0; g < ng; g++) run_fl[g]->put_leaves();
        ph("primitive records");
        std::vector<Compound> todo;   // media and wrapped objects, in emit order
        if (cnt[ZR_PRIM_MEDIUM] + cnt[ZR_KIND_WRAPPED]) for (int32_t lf : leaves) {   // (a million-leaf scan for nothing otherwise)
            const zr::BuildNode& n = br.nodes[lf];
            if (n.kind != ZR_PRIM_MEDIUM && n.kind != ZR_KIND_WRAPPED) continue;
            for (uint32_t k = 0; k < n.count; k++) todo.push_back({n.kind, leaf_first[lf] + k, br.order[n.first + k]});
        }
        finish_compounds(todo);
        if (!filled(*commit_plan)) return fail(ZR_E_DEVICE, "flattener: the primitive arrays do not add up to the plan's sizes (internal error)");
        ph("media / wrapped");
        if (after_primitives) after_primitives();   // the primitive arrays are final: their upload can run beside the rest
        // 4. pair records: all threads; a group's are copied behind the world's with the indices moved (what DeviceBuilder::relocate does) — inner
        // references by the group's first pair, triangle references by the group's first triangle
        fill_pairs();
        for (size_t g = 0; g < ng; g++) {
            Flattener& sub = *run_fl[g];
            sub.pairs.allocate(std::max<size_t>(1, sub.inner.size()));
            sub.fill_pairs();
            for (size_t i = 0; i < sub.pairs.size(); i++) {
                zr::NodePair p = sub.pairs[i];
                for (int c = 0; c < 2; c++) {
                    if (p.meta[c] == 0) p.child[c] += run_root[g];
                    else if (p.meta[c] & 0xFFFFu) p.child[c] += run_tri_base[g];   // (an empty child names nothing)
                }
                pairs[run_root[g] + i] = p;
            }
        }
        ph("pair records");
        // 5. 4-wide nodes
        plan_quads(0);
        ph("4-wide plan");
        number_quads(0);
        ph("4-wide numbering");
        if (!ng) return ZR_OK;
        // a group's 4-wide nodes: same collapse, same quantisation, its root a stored node (a one-leaf group: a node with one child); copied behind the
        // world's, inner references moved by the group's first node, triangle references by its first triangle.  Placements get the roots.
        for (size_t g = 0; g < ng; g++) {
            Flattener& sub = *run_fl[g];
            sub.plan_quads(0);
            sub.number_quads(0);
            if (!sub.quant_ok) quant_ok = false;
            run_qroot[g] = (uint32_t)quads.size();
            for (zr::NodeQ nq : sub.quads) {
                for (int k = 0; k < 4; k++) {
                    if (nq.ref[k] == ZR_REF_EMPTY) continue;
                    if (nq.ref[k] & ZR_REF_LEAF) nq.ref[k] += run_tri_base[g];   // (the low 24 bits: the first primitive)
                    else nq.ref[k] += run_qroot[g];
                }
                quads.push_back(nq);
            }
            run_demand[g] = sub.demand_of(sub.quads[0].ref);
        }
        for (size_t i = 0; i < insts.size(); i++) { insts[i].root = run_root[inst_group[i]]; insts[i].pad_ = run_qroot[inst_group[i]]; }   // (pad_: DInstance::qroot)
        run_fl.clear(); run_objs.clear();
        ph("groups' 4-wide nodes");
        return ZR_OK;
    }
    // the steps of run(), which a group's own flattener takes too
    void index_tree() {   // pair numbers and leaf ranges
        leaf_first.allocate(br.nodes.size()); pair_of.allocate(br.nodes.size());   // fresh pages: zero
        if (br.nodes[0].count) { leaf_first[0] = 0; cnt[br.nodes[0].kind & 7] = br.nodes[0].count; leaves.push_back(0); }   // the whole tree fits one leaf
        else index_nodes();
    }
    void put_leaves() {   // every leaf object of a plain kind as its record (zr_entry.h), at its leaf's place behind out.base
        parallel_for(leaves.size(), 2048, [&](size_t a, size_t b) {
            for (size_t i = a; i < b; i++) {
                const zr::BuildNode& n = br.nodes[leaves[i]];
                if (n.kind == ZR_PRIM_MEDIUM || n.kind == ZR_KIND_WRAPPED) continue;
                for (uint32_t k = 0; k < n.count; k++) {
                    const uint32_t oi = br.order[n.first + k];
                    const size_t di = (size_t)out.base[n.kind & 7] + leaf_first[leaves[i]] + k;
                    zr::put_entry(in, out, objs[oi], commit_plan ? commit_plan->code[oi] >> 4 : 0, di);
                    zr::note_src(out, n.kind, di, oi, objs[oi]);
                }
            }
        });
    }
    void fill_pairs() {
        if (inner.empty()) fill_leaf_root();
        else parallel_for(inner.size(), 4096, [&](size_t a, size_t b) { for (size_t p = a; p < b; p++) fill_pair((uint32_t)p, inner[p]); });
    }
    void fill_leaf_root() {   // the whole world in one leaf: a pair whose second child is empty
        const zr::BuildNode& n = br.nodes[0];
        for (int k = 0; k < 3; k++) { pairs[0].lo[0][k] = f_down(n.box.lo[k]); pairs[0].hi[0][k] = f_up(n.box.hi[k]); }
        pairs[0].child[0] = leaf_first[0]; pairs[0].meta[0] = ((n.kind + 1u) << 16) | n.count;
        empty_child(0, 1);
    }
};

// ---- the host builder's CPU half: the groups' trees, the world's boxes, the binned-SAH tree over them and the flattener, ready to run() ----
struct HostBuild {   // lives on the heap (the flattener refers to its neighbours) and is freed, with everything in it, off the caller's clock
    std::shared_ptr<const CommitPlan> plan;
    std::vector<zr::BuildResult> runs;    // two-level BVH: every group of triangles gets a tree of its own, in its own space, once — however many objects place it
    std::vector<zr::BuildBox> group_box, boxes;
    std::vector<uint32_t> kinds;          // the plan's classification in the form zr::build_bvh reads
    zr::BuildResult br;
    std::unique_ptr<Flattener> fl;
};
inline int build_host_tree(const SceneInput& s, std::shared_ptr<const CommitPlan> plan, PhaseTimer& ph, HostBuild& hb) {
    const std::vector<zr_object>& objs = plan->objs;
    const BuildKnobs& kn = plan->kn;
    hb.plan = plan; hb.runs.resize(s.groups.size()); hb.group_box.resize(s.groups.size());
    const zr::BuildSceneIn tris = scene_view(s);
    const double ck_tri[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    for (size_t g = 0; g < s.groups.size(); g++) {
        const zr_group& grp = s.groups[g];
        std::vector<zr::BuildBox> tb(grp.triangle_count);
        std::vector<uint32_t> tk(grp.triangle_count, ZR_PRIM_TRIANGLE);
        zr::BuildBox all; for (int a = 0; a < 3; a++) { all.lo[a] = kInf; all.hi[a] = -kInf; }
        for (uint32_t k = 0; k < grp.triangle_count; k++) {
            tb[k] = zr::prim_box(tris, ZR_PRIM_TRIANGLE, grp.first_triangle + k);
            for (int a = 0; a < 3; a++) { all.lo[a] = std::fmin(all.lo[a], tb[k].lo[a]); all.hi[a] = std::fmax(all.hi[a], tb[k].hi[a]); }
        }
        hb.group_box[g] = all;
        zr::build_bvh(tb, tk, 4, ZR_STACK_DEPTH - 2, 1.0, ck_tri, hb.runs[g]);
        if (hb.runs[g].max_depth >= ZR_STACK_DEPTH - 1) return fail(ZR_E_INVALID, "group %zu: BVH depth %d exceeds the traversal stack", g, hb.runs[g].max_depth);
    }
    const zr::BuildSceneIn in = scene_view(s, &hb.group_box);
    hb.boxes.resize(objs.size()); hb.kinds.resize(objs.size());
    std::atomic<size_t> bad_box{(size_t)-1};
    parallel_split(objs.size(), [&](size_t k0, size_t k1) {
        for (size_t k = k0; k < k1; k++) {
            const zr_object& o = objs[k];
            hb.boxes[k] = zr::chain_box(in, o.type, o.index, o.chain_first, o.chain_count);
            hb.kinds[k] = plan->kind(k);
            for (int a = 0; a < 3; a++)
                if (!std::isfinite(hb.boxes[k].lo[a]) || !std::isfinite(hb.boxes[k].hi[a])) { size_t want = (size_t)-1; bad_box.compare_exchange_strong(want, k); }
        }
    });
    if (bad_box.load() != (size_t)-1) return fail(ZR_E_INVALID, "object %zu has a non-finite bounding box", bad_box.load());
    ph("boxes");
    zr::build_bvh(hb.boxes, hb.kinds, kn.max_leaf, ZR_STACK_DEPTH - 2, kn.ct, kn.ck, hb.br, kn.leaf_cap);
    ph("binned-SAH build");
    if (hb.br.max_depth >= ZR_STACK_DEPTH - 1) return fail(ZR_E_INVALID, "BVH depth %d exceeds the traversal stack", hb.br.max_depth);
    hb.fl.reset(new Flattener{s, objs, hb.br});
    hb.fl->commit_plan = plan.get();
    hb.fl->runs = hb.runs.empty() ? nullptr : &hb.runs;
    hb.fl->open_ratio = kn.open_ratio;
    hb.fl->want_src = true;
    return ZR_OK;
}

}  // namespace
