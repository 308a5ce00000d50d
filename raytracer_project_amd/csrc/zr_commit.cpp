// zr_commit.cpp — the scene side of the C ABI (include/zr_capi.h): setters and zr_scene_commit — world list, validation, the commit plan (zr_flatten.h), the
// tree and the primitive arrays through the host builder or the device builder, the shared end.  See zr_host_internal.h for the layout of the host side.
#include "zr_host_internal.h"
#include "zr_flatten.h"

namespace {

// The scene's primitive arrays, one by one: f(device array, the flattener's staging array, leaf kind, elements per record, elements per record of the array's
// tail — tri_s alone has one: the triangles' texture coordinates behind its last record, when the scene has any); stops at the first failure.
template <class F>
int each_prim_array(zr_scene* s, Flattener& fl, F&& f) {
    int rc;
    const size_t uv = s->tri_uv.empty() ? 0 : 6;
    if ((rc = f(s->d_spheres, fl.spheres, ZR_PRIM_SPHERE, ZR_SPHERE_DOUBLES, 0)) || (rc = f(s->d_sphere_mat, fl.sphere_mat, ZR_PRIM_SPHERE, 1, 0)) ||
        (rc = f(s->d_tri_v, fl.tri_v, ZR_PRIM_TRIANGLE, ZR_TRI_STRIDE, 0)) || (rc = f(s->d_tri_s, fl.tri_s, ZR_PRIM_TRIANGLE, ZR_TRI_SHADE_DOUBLES, uv)) ||
        (rc = f(s->d_cubes, fl.cubes, ZR_PRIM_CUBE, ZR_CUBE_DOUBLES, 0)) || (rc = f(s->d_cube_mat, fl.cube_mat, ZR_PRIM_CUBE, 1, 0)) ||
        (rc = f(s->d_pcubes, fl.pcubes, ZR_KIND_PCUBE, ZR_PCUBE_STRIDE, 0)) || (rc = f(s->d_pcube_mat, fl.pcube_mat, ZR_KIND_PCUBE, 1, 0)) ||
        (rc = f(s->d_media, fl.media, ZR_PRIM_MEDIUM, 1, 0)) || (rc = f(s->d_wrapped, fl.wrapped, ZR_KIND_WRAPPED, 1, 0))) return rc;
    return ZR_OK;
}

// ---- the commit with the tree built ON THE HOST (zr_bvh.cpp, zr_flatten.h: build_host_tree + Flattener) --------------------------------------------
// Leaves the scene's device arrays filled and `staging` holding everything large, for the caller to free off its clock.
int commit_host(zr_scene* s, std::shared_ptr<const CommitPlan> plan, PhaseTimer& ph, CommitSummary& cs, std::shared_ptr<HostBuild>& staging) {
    auto hb = std::make_shared<HostBuild>();
    int rc = build_host_tree(*s, plan, ph, *hb);
    if (rc) return rc;
    Flattener& fl = *hb->fl;
    // the primitive arrays (a quarter of a gigabyte for a million triangles) go to the device while the host still plans and
    // numbers the 4-wide nodes: a thread of its own, joined before the node arrays follow
    int up_rc = ZR_OK;
    std::string up_err;
    std::thread uploader;
    const int device = s->ctx ? s->ctx->device : 0;
    fl.after_primitives = [&]() {
        uploader = std::thread([&, device]() {
            auto go = [&]() -> int { HIP_OK(hipSetDevice(device)); return each_prim_array(s, fl, [](auto& d, auto& a, uint32_t, size_t, size_t) { return d.upload(a); }); };
            up_rc = go();
            if (up_rc != ZR_OK) up_err = zr_host::last_error();   // the error text is per thread
        });
    };
    struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{uploader};   // no path leaves the thread running
    if ((rc = fl.run())) return rc;
    ph("flatten + quantise");
    if ((rc = s->d_nodes.upload(fl.pairs)) || (rc = s->d_quads.upload(fl.quads))) return rc;
    if ((rc = s->d_insts.upload(fl.insts))) return rc;   // (after the groups' nodes were numbered: a placement names its group's root)
    if (uploader.joinable()) uploader.join();
    else { fl.after_primitives(); uploader.join(); }   // a world without nodes returned from run() before the hook: upload the (empty) arrays here
    if (up_rc != ZR_OK) return fail(up_rc, "%s", up_err.c_str());
    if ((rc = s->d_ops.upload(s->ops.data(), s->ops.size()))) return rc;
    fl.after_primitives = nullptr;   // (it captures locals of this call)
    for (int k = 0; k < 8; k++) s->leaf_src[k] = std::move(fl.src[k]);
    cs.root = fl.root; cs.quant_ok = fl.quant_ok; cs.n_pairs = fl.pairs.size(); cs.n_quads = fl.quads.size(); cs.plain_media = fl.plain_media();
    cs.stack_demand = fl.stack_demand(); cs.quad_depth = fl.quad_depth; cs.max_depth = hb->br.max_depth; cs.kept_closed = fl.n_kept_closed;
    cs.builder = "host (binned SAH)";
    s->group_box = hb->group_box;
    staging = std::move(hb);
    return ZR_OK;
}

// ---- the commit with the tree built ON THE DEVICE (zr_build.hip) ------------------------------------------------------------------
// The scene's arrays go to the device as they are; boxes, Morton keys, sort, PLOC merging, leaf collapse, the 4-wide quantised
// nodes, the pair records and the primitive records in leaf order are all produced there.  The host finishes the few compound
// objects (media, wrapped objects: each drags inner primitives behind the leaf ranges).
// The outcome travels beside the ZR_E_* code: UseHost says "this world is the host builder's" — the builder's own wants_host() (a tree deeper than the
// traversal stack, coordinates beyond 1e18), hipErrorOutOfMemory from the builder, more groups than ZR_BVH_DEVICE_MAX_GROUPS, or a DevBuf::alloc in here that
// found no room (the device build holds the scene as given, its arena and the final arrays at once; the host path's staging lives in host memory).  The code
// matters only with Failed.  A DevBuf::upload or a copy that fails, out of memory included, fails the commit: that asymmetry is inherited from the time the
// fallback was decided by the error's wording, not decided here.
enum class DeviceBuild { Done, UseHost, Failed };

struct DeviceTemps {   // the builder (its scratch arena, the trees' local records), the as-given copies, the groups' tables: freed off the caller's clock
    std::unique_ptr<zr::DeviceBuilder> builder;
    DevBuf<double> sph, tri_v, tri_n, tri_uv, cubes, gbox;
    DevBuf<uint32_t> sph_mat, tri_mat, cube_mat, inst_group, run_demand, run_root, run_qroot;
    DevBuf<zr_medium> media; DevBuf<zr_object> objs; DevBuf<uint8_t> code;
};

int commit_device(zr_scene* s, const CommitPlan& plan, const PhaseTimer& outer, CommitSummary& cs, DeviceBuild& outcome) {
    PhaseTimer ph{"commit(device)", 22, outer.t0};   // ("classify" is the plan, made by the caller)
    const std::vector<zr_object>& objs = plan.objs;
    const uint32_t n = (uint32_t)objs.size();
    const size_t* z = plan.size;
    hipStream_t st = s->ctx->stream;
    int rc;
    outcome = DeviceBuild::Failed;
    auto room = [&](int r) {   // of a DevBuf::alloc, whose only failure is "out of device memory"
        if (r) { outcome = DeviceBuild::UseHost; std::fprintf(stderr, "[zr] device BVH build: %s: host builder\n", zr_host::last_error()); }
        return r;
    };
    // every group's tree is a build of its own (a few dozen launches and a handful of synchronisations, ~1 ms however small the run):
    // a world of very many small groups is the host builder's, which builds them on its threads
    if ((double)s->groups.size() > env_double("ZR_BVH_DEVICE_MAX_GROUPS", 256)) {
        std::fprintf(stderr, "[zr] device BVH build: %zu groups of triangles: host builder\n", s->groups.size());
        outcome = DeviceBuild::UseHost;
        return ZR_OK;
    }
    ph("classify");
    // 1. the scene as given -> device (freed with this call), the final primitive arrays allocated.  The large arrays are pinned for the
    // copy (hipHostRegister: 2.4 ms per 160 MB on the GPU box, then 57 GB/s instead of the ~10 GB/s of a first pageable copy,
    // profiles/r3_affine_ab.txt) and travel asynchronously on the build's stream
    auto tmp = std::make_shared<DeviceTemps>();
    DeviceTemps& t = *tmp;
    // (an early return leaves copies in flight: they are waited for before their source pages are unpinned)
    struct Pinned { hipStream_t st; std::vector<void*> p; ~Pinned() { if (!p.empty()) (void)hipStreamSynchronize(st); for (void* q : p) (void)hipHostUnregister(q); } } pinned{st, {}};
    auto send = [&](auto& buf, const auto* src, size_t count) -> int {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(src)>>;
        int r = room(buf.alloc(count));
        if (r || count == 0) return r;
        const size_t bytes = count * sizeof(T);
        if (bytes >= (4u << 20) && hipHostRegister((void*)src, bytes, hipHostRegisterDefault) == hipSuccess) {
            pinned.p.push_back((void*)src);
            HIP_OK(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, st));
        } else {
            (void)hipGetLastError();
            HIP_OK(hipMemcpy(buf.p, src, bytes, hipMemcpyHostToDevice));
        }
        return ZR_OK;
    };
    if ((rc = send(t.tri_v, s->tri_v.data(), s->tri_v.size())) || (rc = send(t.tri_n, s->tri_n.data(), s->tri_n.size())) ||
        (!s->tri_uv.empty() && (rc = send(t.tri_uv, s->tri_uv.data(), s->tri_uv.size()))) ||
        (rc = send(t.objs, objs.data(), objs.size())) || (rc = send(t.tri_mat, s->tri_mat.data(), s->tri_mat.size())) ||
        (rc = send(t.sph, s->spheres.data(), s->spheres.size())) || (rc = send(t.sph_mat, s->sphere_mat.data(), s->sphere_mat.size())) ||
        (rc = send(t.cubes, s->cubes.data(), s->cubes.size())) || (rc = send(t.cube_mat, s->cube_mat.data(), s->cube_mat.size())) ||
        (rc = send(t.media, s->media.data(), s->media.size())) || (rc = s->d_ops.upload(s->ops.data(), s->ops.size())) || (rc = send(t.code, plan.code.data(), plan.code.size()))) return rc;
    static const zr::BuildResult no_tree;
    Flattener fl{*s, objs, no_tree};   // the compound objects' staging (step 5), filled by the flattener's own routines
    if ((rc = each_prim_array(s, fl, [&](auto& d, auto&, uint32_t kind, size_t per, size_t tail) { return room(d.alloc(z[kind] * (per + tail))); })) ||
        (rc = room(s->d_insts.alloc(z[ZR_KIND_INSTANCE]))) || (rc = room(t.inst_group.alloc(z[ZR_KIND_INSTANCE])))) return rc;
    ph("upload as given");
    zr::BuildSceneIn in;
    in.spheres = t.sph.p; in.sphere_mat = t.sph_mat.p; in.tri_v = t.tri_v.p; in.tri_n = t.tri_n.p; in.tri_mat = t.tri_mat.p;
    if (!s->tri_uv.empty()) in.tri_uv = t.tri_uv.p;
    in.cubes = t.cubes.p; in.cube_mat = t.cube_mat.p; in.media = t.media.p; in.ops = s->d_ops.p;   // (d_ops: the scene's own, uploaded above, alive beyond the build)
    const BuildKnobs& kn = plan.kn;
    zr::BuildParams bp;
    bp.ct = (float)kn.ct;
    for (int k = 0; k < 8; k++) { bp.ck[k] = (float)kn.ck[k]; bp.leaf_cap[k] = kn.leaf_cap[k]; }
    bp.max_leaf = kn.max_leaf;
    bp.open_ratio = (float)kn.open_ratio;
    bp.radius = (int)env_double("ZR_BVH_PLOC_RADIUS", 16);
    // PLOC stops at n / 64 clusters (4096 ... 65536) and the host's SAH builder arranges those: the larger the SAH-built top, the closer
    // the walk comes to the host tree's, and the longer the host's pass takes (cfg3 EXTEND per frame against the host tree's: no top
    // +8.3 %, 16384 clusters +2.6 %, 65536 +2.3 %, for 17 / 19 / 28 ms of commit — the reference commits once per frame, so the default
    // is the 16384 a million objects get; profiles/r3_builders.txt).  ZR_BVH_TOP overrides (0: PLOC to the root)
    {
        const double top_env = env_double("ZR_BVH_TOP", -1);
        bp.top_clusters = top_env >= 0 ? (int)top_env : (int)std::min<size_t>(65536, std::max<size_t>(4096, (size_t)n / 64));
    }
    // leaf primitive -> caller index (zr_scene_tree_boxes), written by the emit kernel
    DevBuf<uint32_t> d_src[8];
    for (int k = 0; k < 7; k++) {
        if ((rc = room(d_src[k].alloc(z[k])))) return rc;
        HIP_OK(hipMemsetAsync(d_src[k].p, 0xFF, std::max<size_t>(z[k], 1) * 4, st));
    }
    zr::BuildPrimOut out;
    for (int k = 0; k < 7; k++) out.src[k] = d_src[k].p;
    out.spheres = s->d_spheres.p; out.sphere_mat = s->d_sphere_mat.p; out.tri_v = s->d_tri_v.p; out.tri_s = s->d_tri_s.p;
    if (!s->tri_uv.empty() && z[ZR_PRIM_TRIANGLE]) out.tri_uv = s->d_tri_s.p + z[ZR_PRIM_TRIANGLE] * ZR_TRI_SHADE_DOUBLES;   // behind the last shading record
    out.cubes = s->d_cubes.p; out.cube_mat = s->d_cube_mat.p; out.pcubes = s->d_pcubes.p; out.pcube_mat = s->d_pcube_mat.p;
    out.insts = s->d_insts.p; out.inst_group = t.inst_group.p;
    t.builder.reset(new zr::DeviceBuilder(st));
    // the builder says when the input is the host builder's business; running out of memory is too — the device build's footprint is several times the
    // host path's, whose arrays this function's buffers make room for when it returns
    auto build_fail = [&](hipError_t e) -> int {
        if (t.builder->wants_host()) std::fprintf(stderr, "[zr] device BVH build: %s\n", t.builder->error());
        else if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            std::fprintf(stderr, "[zr] device BVH build: out of device memory (%s): host builder\n", t.builder->error());
            t.builder.reset();
        } else return fail(ZR_E_DEVICE, "device BVH build failed: %s (%s)", hipGetErrorString(e), t.builder->error());
        outcome = DeviceBuild::UseHost;
        return ZR_OK;
    };
    // 2. the groups' trees (two-level BVH: one tree per shared run of triangles, in its own space)
    const size_t ng = s->groups.size();
    std::vector<zr::BuiltTree> runs(ng);
    std::vector<double> gbox(ng * 6);
    std::vector<uint32_t> run_demand(ng);
    {
        size_t at = plan.cnt[ZR_PRIM_TRIANGLE];
        for (size_t g = 0; g < ng; g++) {
            const zr_group& grp = s->groups[g];
            zr::BuildPrimOut go = out;
            go.base[ZR_PRIM_TRIANGLE] = (uint32_t)at; at += grp.triangle_count;
            hipError_t e = t.builder->build(in, nullptr, nullptr, grp.first_triangle, grp.triangle_count, bp, true, go, nullptr, ZR_STACK_DEPTH - 2, false, runs[g]);
            if (e != hipSuccess) return build_fail(e);
            for (int k = 0; k < 6; k++) gbox[g * 6 + k] = runs[g].box[k];
            run_demand[g] = runs[g].demand;
        }
    }
    if (ng) { if ((rc = t.gbox.upload(gbox)) || (rc = t.run_demand.upload(run_demand))) return rc; in.group_box = t.gbox.p; }
    ph("groups' trees");
    // 3. the world's tree
    zr::BuiltTree world;
    world.want_boxes = std::getenv("ZR_BUILD_CHECK") != nullptr;
    {
        hipError_t e = t.builder->build(in, t.objs.p, t.code.p, 0, n, bp, false, out, ng ? t.run_demand.p : nullptr, ZR_STACK_DEPTH - 2, ph.on, world);
        if (e != hipSuccess) return build_fail(e);
    }
    if (ph.on)
        std::fprintf(stderr, "[zr] device build: boxes+keys %.2f, sort %.2f, PLOC %.2f (%u iterations), order %.2f, 4-wide %.2f, pairs %.2f, emit %.2f ms; depth %u, %u pairs, %u quads\n",
                     world.ms[0], world.ms[1], world.ms[2], world.ploc_iterations, world.ms[3], world.ms[4], world.ms[5], world.ms[6], world.depth, world.n_pairs, world.n_quads);
    if (world.want_boxes) {   // self-check: every object's device box must contain the box the host's compilation of chain_box (zr_entry.h) computes for it
        zr::BuildSceneIn hin = scene_view(*s);
        hin.group_box = gbox.data();
        size_t bad = 0;
        for (uint32_t k = 0; k < n; k++) {
            const zr::BuildBox hb = zr::chain_box(hin, objs[k].type, objs[k].index, objs[k].chain_first, objs[k].chain_count);
            const float* d = &world.dbg_boxes[(size_t)k * 8];
            bool ok = true;
            for (int a = 0; a < 3; a++) if (!((double)d[a] <= hb.lo[a]) || !((double)d[4 + a] >= hb.hi[a])) ok = false;
            if (!ok && bad++ < 8)
                std::fprintf(stderr, "[zr] BUILD_CHECK: object %u (type %u, chain %u): device box [%g %g %g | %g %g %g] does not contain the host's [%g %g %g | %g %g %g]\n", k, objs[k].type,
                             objs[k].chain_count, d[0], d[1], d[2], d[4], d[5], d[6], hb.lo[0], hb.lo[1], hb.lo[2], hb.hi[0], hb.hi[1], hb.hi[2]);
        }
        if (bad) return fail(ZR_E_DEVICE, "ZR_BUILD_CHECK: %zu of %u object boxes computed on the device do not contain the host's", bad, n);
    }
    for (int k = 0; k < 8; k++)
        if (world.cnt[k] != plan.cnt[k]) return fail(ZR_E_DEVICE, "device BVH build: %u leaf primitives of kind %d, expected %u (internal error)", world.cnt[k], k, plan.cnt[k]);
    ph("world tree");
    // 4. the scene's node arrays at their exact sizes: the world's records first, then every group's
    size_t n_pairs = world.n_pairs, n_quads = world.n_quads;
    std::vector<uint32_t> run_root(ng), run_qroot(ng);
    for (size_t g = 0; g < ng; g++) { run_root[g] = (uint32_t)n_pairs; run_qroot[g] = (uint32_t)n_quads; n_pairs += runs[g].n_pairs; n_quads += runs[g].n_quads; }
    if ((rc = room(s->d_nodes.alloc(n_pairs))) || (rc = room(s->d_quads.alloc(n_quads)))) return rc;
    {
        hipError_t e = t.builder->relocate(world, s->d_nodes.p, 0, s->d_quads.p, 0);
        for (size_t g = 0; g < ng && e == hipSuccess; g++) e = t.builder->relocate(runs[g], s->d_nodes.p, run_root[g], s->d_quads.p, run_qroot[g]);
        if (e == hipSuccess && z[ZR_KIND_INSTANCE]) {
            if ((rc = t.run_root.upload(run_root)) || (rc = t.run_qroot.upload(run_qroot))) return rc;
            e = t.builder->patch_instances(s->d_insts.p, t.inst_group.p, (uint32_t)z[ZR_KIND_INSTANCE], t.run_root.p, t.run_qroot.p);
        }
        if (e != hipSuccess) return fail(ZR_E_DEVICE, "device BVH build: %s", hipGetErrorString(e));
    }
    // 5. compound objects on the host: a medium's boundary, the object inside a wrapper chain (on staging arrays whose untouched pages cost
    // nothing; only what the host wrote is uploaded: the records behind the leaf ranges, media and wrapped objects whole)
    if (z[ZR_PRIM_MEDIUM] + z[ZR_KIND_WRAPPED]) {
        fl.allocate_arrays(plan); fl.n_tri += plan.group_tris;
        std::vector<Flattener::Compound> todo;   // media before wrapped objects, each in array order
        for (size_t k = 0; k + 1 < world.compound.size(); k += 2) todo.push_back({plan.kind(world.compound[k]), world.compound[k + 1], world.compound[k]});
        std::sort(todo.begin(), todo.end(), [](const Flattener::Compound& a, const Flattener::Compound& b) { return a.kind != b.kind ? a.kind < b.kind : a.di < b.di; });
        fl.finish_compounds(todo);
        if (!fl.filled(plan)) return fail(ZR_E_DEVICE, "device BVH build: compound objects do not add up (internal error)");
        rc = each_prim_array(s, fl, [&](auto& d, auto& a, uint32_t kind, size_t per, size_t tail) -> int {
            const size_t first = kind == ZR_PRIM_MEDIUM || kind == ZR_KIND_WRAPPED ? 0 : z[kind] - plan.inner[kind];
            const size_t from = first * per, to = z[kind] * per;
            if (to > from) HIP_OK(hipMemcpyAsync(d.p + from, &a[from], (to - from) * sizeof(a[0]), hipMemcpyHostToDevice, st));
            const size_t tfrom = to + first * tail, tto = to + z[kind] * tail;   // the same records' share of the tail
            if (tto > tfrom) HIP_OK(hipMemcpyAsync(d.p + tfrom, &a[tfrom], (tto - tfrom) * sizeof(a[0]), hipMemcpyHostToDevice, st));
            return ZR_OK;
        });
        if (rc) return rc;
    }
    HIP_OK(hipStreamSynchronize(st));   // (the staging arrays die with this call)
    for (int k = 0; k < 8; k++) {
        s->leaf_src[k].assign(d_src[k].n, 0xFFFFFFFFu);
        if (d_src[k].n) HIP_OK(hipMemcpy(s->leaf_src[k].data(), d_src[k].p, d_src[k].n * 4, hipMemcpyDeviceToHost));
    }
    ph("node arrays + compound");
    cs.root = world.root; cs.quant_ok = world.quant_ok;
    for (const zr::BuiltTree& r : runs) cs.quant_ok = cs.quant_ok && r.quant_ok;
    cs.n_pairs = n_pairs; cs.n_quads = n_quads; cs.plain_media = fl.plain_media();
    cs.stack_demand = world.demand; cs.quad_depth = (int)world.quad_depth; cs.max_depth = (int)world.depth;
    cs.builder = "device (PLOC)";
    s->group_box.resize(ng);
    for (size_t g = 0; g < ng; g++) for (int k = 0; k < 3; k++) { s->group_box[g].lo[k] = gbox[g * 6 + k]; s->group_box[g].hi[k] = gbox[g * 6 + 3 + k]; }
    s->ctx->free_later([tmp = std::move(tmp), device = s->ctx->device]() mutable { (void)hipSetDevice(device); tmp.reset(); });
    ph("release");
    outcome = DeviceBuild::Done;
    return ZR_OK;
}

// ---- the shared end of a commit: the tables every scene has (materials, textures), the DScene the kernels receive, the kernel builds the world needs ----
int finish_commit(zr_scene* s, const CommitPlan& plan, const CommitSummary& cs) {
    int rc;
    const size_t* z = plan.size;
    if (std::getenv("ZR_QUANT_STATS")) std::fprintf(stderr, "[zr] 4-wide nodes: %zu quantised (64 B) + FP32 root; %zu children kept closed for the grid\n", cs.n_quads, cs.kept_closed);
    s->quad_ok = cs.quant_ok && cs.n_quads < (1u << 31) && plan.kn.max_leaf <= 16;
    for (int k = 0; k < 8; k++) s->quad_ok = s->quad_ok && z[k] < zr::ST_MAX_LEAF_PRIMS;
    {
        // zr_material::pad_ on the device copy: the material reads u/v/tangent (image texture anywhere in its
        // texture tree, or a bump map) -> the kernels compute those hit-record fields only then
        std::vector<zr_material> mats = s->materials;
        auto tex_uses_uv = [&](uint32_t id) {
            std::vector<uint32_t> todo{id}; int guard = 0;
            while (!todo.empty() && guard++ < 4096) {
                uint32_t t = todo.back(); todo.pop_back();
                if (t >= s->textures.size()) continue;
                const zr_texture& tx = s->textures[t];
                if (tx.kind >= ZR_TEX_IMAGE_U8) return true;
                if (tx.kind == ZR_TEX_CHECKER) { todo.push_back(tx.odd); todo.push_back(tx.even); }
            }
            return guard >= 4096;
        };
        for (zr_material& m : mats) m.pad_ = (m.bump_tex != ZR_NO_TEXTURE || (m.kind != ZR_MAT_DIELECTRIC && tex_uses_uv(m.tex))) ? 1u : 0u;
        if ((rc = s->d_mats.upload(mats))) return rc;
    }
    if ((rc = s->d_texs.upload(s->textures))) return rc;
    if ((rc = s->d_texels.upload(s->texels.data(), s->texels.size()))) return rc;

    zr::DScene& d = s->ds;
    d.nodes = s->d_nodes.p; d.quads = s->d_quads.p;
    d.spheres = s->d_spheres.p; d.sphere_mat = s->d_sphere_mat.p;
    d.tri_v = s->d_tri_v.p; d.tri_s = s->d_tri_s.p;
    if (!s->tri_uv.empty() && z[ZR_PRIM_TRIANGLE] * (ZR_TRI_SHADE_DOUBLES / 4) > 0xFFFFFFFFull) return fail(ZR_E_INVALID, "too many triangles for texture coordinates (%zu stored)", z[ZR_PRIM_TRIANGLE]);
    // (the kernels' builds that read texture coordinates are launched when this is not zero; ZR_TRI_SHADE_DOUBLES / 4 units a record)
    d.tri_uv_at = s->tri_uv.empty() ? 0u : (uint32_t)(z[ZR_PRIM_TRIANGLE] * (ZR_TRI_SHADE_DOUBLES / 4));
    d.cubes = s->d_cubes.p; d.cube_mat = s->d_cube_mat.p;
    d.pcubes = s->d_pcubes.p; d.pcube_mat = s->d_pcube_mat.p;
    d.media = s->d_media.p; d.wrapped = s->d_wrapped.p; d.insts = s->d_insts.p; d.ops = s->d_ops.p;
    d.mats = s->d_mats.p; d.texs = s->d_texs.p; d.texels = s->d_texels.p;
    d.n_mats = (uint32_t)s->materials.size();
    d.mat_kinds = 0;
    for (const zr_material& m : s->materials) d.mat_kinds |= 1u << m.kind;
    d.root = cs.root;
    s->leaf_objects = 0;
    for (int k = 0; k < 7; k++) { d.leaf_cnt[k] = plan.cnt[k]; s->leaf_objects += plan.cnt[k]; }   // (no leaf kind 7 exists)
    // a small world's objects for the fused kernel's arguments (refresh_fused_objects, below; a refit runs it again)
    for (int k = 0; k < 8; k++) s->plan_cnt[k] = plan.cnt[k];
    if ((rc = refresh_fused_objects(s))) return rc;
    {   // which build of the EXTEND kernel this world needs (zr_stream.hip)
        if (z[ZR_KIND_INSTANCE]) s->leaf_level = 3;   // placed runs of triangles: the build with the nested walk
        else if (z[ZR_KIND_WRAPPED] || !cs.plain_media) s->leaf_level = 2;
        else if (z[ZR_PRIM_CUBE] || z[ZR_KIND_PCUBE] || z[ZR_PRIM_MEDIUM]) s->leaf_level = 1;
        else s->leaf_level = 0;
        const int force = (int)env_double("ZR_EXTEND_LEVEL", -1);
        if (force > s->leaf_level && force <= 3) s->leaf_level = force;
        // SHADE's lean build (zr_device.h: lean_rec / lean_shade): a world of bare triangles and spheres whose materials are lambertian / metal / dielectric / light
        // over solid-colour textures, no bump maps — nothing in it reads u, v, a tangent, an image or a wrapper chain
        bool lean = s->leaf_level == 0 && env_double("ZR_SHADE_LEAN", 1) != 0;
        for (const zr_material& m : s->materials) {
            if (m.kind != ZR_MAT_LAMBERTIAN && m.kind != ZR_MAT_METAL && m.kind != ZR_MAT_DIELECTRIC && m.kind != ZR_MAT_LIGHT) lean = false;
            if (m.bump_tex != ZR_NO_TEXTURE) lean = false;
            if (m.kind != ZR_MAT_DIELECTRIC && (m.tex >= s->textures.size() || s->textures[m.tex].kind != ZR_TEX_SOLID)) lean = false;
        }
        d.shade_lean = lean ? 1u : 0u;
        // ... and its escape stage (zr_stream.hip, stream_shade): on wherever the lean pair runs; ZR_SHADE_ESCAPE=0 switches it off for A/B runs
        d.shade_escape = lean && env_double("ZR_SHADE_ESCAPE", 1) != 0 ? 1u : 0u;
    }
    s->stack_demand = cs.stack_demand;
    if (std::getenv("ZR_QUANT_STATS")) std::fprintf(stderr, "[zr] 4-wide tree: depth %d, worst-case traversal stack %u entries\n", cs.quad_depth, s->stack_demand);
    s->stats[0] = cs.n_pairs; s->stats[1] = (uint64_t)cs.max_depth; s->stats[2] = plan.objs.size();
    s->stats[3] = cs.n_pairs * sizeof(zr::NodePair) + cs.n_quads * sizeof(zr::NodeQ) + (z[ZR_PRIM_SPHERE] * ZR_SPHERE_DOUBLES + z[ZR_PRIM_TRIANGLE] * (ZR_TRI_STRIDE + ZR_TRI_SHADE_DOUBLES) + z[ZR_PRIM_CUBE] * ZR_CUBE_DOUBLES +
                   z[ZR_KIND_PCUBE] * ZR_PCUBE_STRIDE) * sizeof(double) + (z[ZR_PRIM_SPHERE] + z[ZR_PRIM_CUBE]) * sizeof(uint32_t) + s->texels.size() +
                  (s->tri_uv.empty() ? 0 : z[ZR_PRIM_TRIANGLE] * 6 * sizeof(double));
    s->builder = cs.builder;
    if (std::getenv("ZR_COMMIT_HASH")) {   // development / test aid: a hash of the committed 4-wide node array and pair records — the tree AND its layout in memory
        (void)hipDeviceSynchronize();
        auto fnv = [](const void* dev, size_t bytes) -> unsigned long long {
            std::vector<unsigned char> h(bytes);
            unsigned long long x = 1469598103934665603ull;
            if (bytes && hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost) == hipSuccess) for (unsigned char b : h) { x ^= b; x *= 1099511628211ull; }
            return x;
        };
        std::fprintf(stderr, "[zr] commit hash (%s): quads %016llx (%zu), pairs %016llx (%zu)\n", cs.builder, fnv(s->d_quads.p, cs.n_quads * sizeof(zr::NodeQ)), cs.n_quads,
                     fnv(s->d_nodes.p, cs.n_pairs * sizeof(zr::NodePair)), cs.n_pairs);
    }
    s->committed = true;
    if (!s->borrowed) { s->plan_objs = plan.objs; s->plan_code = plan.code; s->plan_bake = plan.kn.bake; }   // a copied scene can be baked again: zr_scene_update_*
    if (s->borrowed) {   // the caller's arrays are not read again: forget them (a second commit needs a new zr_scene_set_*)
        s->spheres.drop(); s->sphere_mat.drop(); s->tri_v.drop(); s->tri_n.drop(); s->tri_mat.drop(); s->tri_uv.drop(); s->cubes.drop(); s->cube_mat.drop();
        s->media.drop(); s->ops.drop(); s->objects.drop(); s->texels.drop(); s->objects_set = false; s->borrowed = false; s->released = true;
    }
    return ZR_OK;
}

}  // namespace

// A small world's objects for the fused kernel's arguments (zr_launch.h: FusedObjs): read back from the device arrays, whichever builder made them and
// whatever a refit has rewritten since (a few hundred bytes).  The arguments are copies, so a refit calls this again.
int refresh_fused_objects(zr_scene* s) {
    int rc;
    s->fused_ok = false;
    if (s->leaf_objects > 0 && s->leaf_objects <= ZR_FUSED_OBJECTS && s->plan_cnt[ZR_KIND_INSTANCE] == 0) {
        zr::FusedObjs fo{};
        auto take = [&](uint32_t kind, const double* d_src, size_t stride, size_t doubles) -> int {
            for (uint32_t i = 0; i < s->plan_cnt[kind]; i++) {
                fo.kind[fo.n] = kind; fo.index[fo.n] = i;
                HIP_OK(hipMemcpy(fo.rec[fo.n], d_src + (size_t)i * stride, doubles * sizeof(double), hipMemcpyDeviceToHost));
                fo.n++;
            }
            return ZR_OK;
        };
        if ((rc = take(ZR_PRIM_SPHERE, s->d_spheres.p, ZR_SPHERE_DOUBLES, ZR_SPHERE_DOUBLES)) || (rc = take(ZR_PRIM_TRIANGLE, s->d_tri_v.p, ZR_TRI_STRIDE, 9)) ||
            (rc = take(ZR_PRIM_CUBE, s->d_cubes.p, ZR_CUBE_DOUBLES, ZR_CUBE_DOUBLES)) || (rc = take(ZR_KIND_PCUBE, s->d_pcubes.p, ZR_PCUBE_STRIDE, ZR_PCUBE_STRIDE))) return rc;
        std::vector<zr::DMedium> hm(s->plan_cnt[ZR_PRIM_MEDIUM]);
        if (!hm.empty()) HIP_OK(hipMemcpy(hm.data(), s->d_media.p, hm.size() * sizeof(zr::DMedium), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < hm.size(); i++) {
            if (hm[i].chain_count != 0) continue;   // a wrapped boundary: tested through the scene's arrays (level 2)
            fo.kind[fo.n] = ZR_PRIM_MEDIUM; fo.index[fo.n] = i;
            const bool sph = hm[i].btype == ZR_PRIM_SPHERE;
            HIP_OK(hipMemcpy(fo.rec[fo.n], sph ? s->d_spheres.p + (size_t)hm[i].bindex * ZR_SPHERE_DOUBLES : s->d_cubes.p + (size_t)hm[i].bindex * ZR_CUBE_DOUBLES, (sph ? ZR_SPHERE_DOUBLES : ZR_CUBE_DOUBLES) * sizeof(double), hipMemcpyDeviceToHost));
            fo.rec[fo.n][6] = hm[i].neg_inv_density;
            const uint64_t idb = hm[i].id, tb = hm[i].btype;
            std::memcpy(&fo.rec[fo.n][7], &idb, 8); std::memcpy(&fo.rec[fo.n][8], &tb, 8);
            fo.n++;
        }
        bool scaled = false;   // the fused kernel's placed-cube code carries no scale (zr_device.h pcube_ray<false>): such a world takes the pipeline
        for (uint32_t i = 0; i < fo.n; i++) if (fo.kind[i] == ZR_KIND_PCUBE && fo.rec[i][15] != 0.0) scaled = true;
        s->fused = fo; s->fused_ok = !scaled;
    }
    return ZR_OK;
}

extern "C" {

zr_scene* zr_scene_create(zr_ctx* c) {
    if (!c) { fail(ZR_E_INVALID, "null context"); return nullptr; }
    zr_scene* s = new zr_scene();
    s->ctx = c; s->device = c->device;
    return s;
}
void zr_scene_destroy(zr_scene* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);   // (not through s->ctx: the context may be gone)
    delete s;
}

// A borrowed commit drops every geometry view (`released`): the scene can be committed again only after ALL of them were given
// again — zr_scene_set_all / zr_scene_set_all_borrowed, or each of the six geometry setters (SET_* bits).  A lone
// zr_scene_set_materials must not re-arm the commit: it would build an empty world and return ZR_OK.
enum { SET_SPHERES = 1, SET_TRIANGLES = 2, SET_CUBES = 4, SET_MEDIA = 8, SET_OPS = 16, SET_OBJECTS = 32, SET_ALL_GEOMETRY = 63 };
#define CHECK_SCENE(s) do { if (!(s)) return fail(ZR_E_INVALID, "null scene"); (s)->committed = false; } while (0)
#define GEOMETRY_SET(s, bit) do { if ((s)->released) { (s)->reset_mask |= (bit); if (((s)->reset_mask & SET_ALL_GEOMETRY) == SET_ALL_GEOMETRY) { (s)->released = false; (s)->reset_mask = 0; } } } while (0)

int zr_scene_set_spheres(zr_scene* s, const double* p, const uint32_t* mat, size_t n) {
    CHECK_SCENE(s);
    if (n && (!p || !mat)) return fail(ZR_E_INVALID, "null sphere arrays");
    s->spheres.copy(p, n * 4); s->sphere_mat.copy(mat, n);
    GEOMETRY_SET(s, SET_SPHERES);
    return ZR_OK;
}
int zr_scene_set_triangles(zr_scene* s, const double* v9, const double* n9, const uint32_t* mat, size_t n) {
    CHECK_SCENE(s);
    if (n && (!v9 || !n9 || !mat)) return fail(ZR_E_INVALID, "null triangle arrays");
    s->tri_v.copy(v9, n * 9); s->tri_n.copy(n9, n * 9); s->tri_mat.copy(mat, n);
    s->tri_uv.drop();   // texture coordinates belong to the triangles they were given for
    GEOMETRY_SET(s, SET_TRIANGLES);
    return ZR_OK;
}
int zr_scene_set_triangle_uvs(zr_scene* s, const double* uv6, size_t n) {
    if (!s) return fail(ZR_E_INVALID, "null scene");
    if (!uv6 && n) return fail(ZR_E_INVALID, "null texture-coordinate array for %zu triangles", n);
    if (!uv6) { s->committed = false; s->tri_uv.drop(); return ZR_OK; }
    if (n != s->tri_mat.size()) return fail(ZR_E_INVALID, "texture coordinates for %zu triangles, the scene has %zu", n, s->tri_mat.size());
    for (size_t k = 0; k < n * 6; k++)
        if (!std::isfinite(uv6[k])) return fail(ZR_E_INVALID, "texture coordinate %zu of triangle %zu is not finite", k % 6, k / 6);
    s->committed = false;
    s->tri_uv.copy(uv6, n * 6);
    return ZR_OK;
}
int zr_scene_set_cubes(zr_scene* s, const double* q, const uint32_t* mat, size_t n) {
    CHECK_SCENE(s);
    if (n && (!q || !mat)) return fail(ZR_E_INVALID, "null cube arrays");
    s->cubes.copy(q, n * 12); s->cube_mat.copy(mat, n);
    GEOMETRY_SET(s, SET_CUBES);
    return ZR_OK;
}
int zr_scene_set_media(zr_scene* s, const zr_medium* m, size_t n) {
    CHECK_SCENE(s);
    if (n && !m) return fail(ZR_E_INVALID, "null media array");
    s->media.copy(m, n);
    GEOMETRY_SET(s, SET_MEDIA);
    return ZR_OK;
}
int zr_scene_set_xform_ops(zr_scene* s, const zr_xform_op* o, size_t n) {
    CHECK_SCENE(s);
    if (n && !o) return fail(ZR_E_INVALID, "null op array");
    s->ops.copy(o, n);
    GEOMETRY_SET(s, SET_OPS);
    return ZR_OK;
}
int zr_scene_set_objects(zr_scene* s, const zr_object* o, size_t n) {
    CHECK_SCENE(s);
    if (n && !o) return fail(ZR_E_INVALID, "null object array");
    s->objects.copy(o, n); s->objects_set = n > 0;
    GEOMETRY_SET(s, SET_OBJECTS);
    return ZR_OK;
}
int zr_scene_set_groups(zr_scene* s, const zr_group* g, size_t n) {
    CHECK_SCENE(s);
    if (n && !g) return fail(ZR_E_INVALID, "null group array");
    s->groups.assign(g, g + n);
    return ZR_OK;
}
int zr_scene_set_materials(zr_scene* s, const zr_material* m, size_t n) {
    CHECK_SCENE(s);
    if (n && !m) return fail(ZR_E_INVALID, "null material array");
    s->materials.assign(m, m + n);
    return ZR_OK;
}
int zr_scene_set_textures(zr_scene* s, const zr_texture* t, size_t n, const void* blob, size_t bytes) {
    CHECK_SCENE(s);
    if ((n && !t) || (bytes && !blob)) return fail(ZR_E_INVALID, "null texture arrays");
    s->textures.assign(t, t + n);
    s->texels.copy((const unsigned char*)blob, bytes);
    return ZR_OK;
}
int zr_scene_set_all(zr_scene* s, const zr_scene_desc* d) {
    CHECK_SCENE(s);
    if (!d) return fail(ZR_E_INVALID, "null scene description");
    int rc;
    if ((rc = zr_scene_set_spheres(s, d->spheres, d->sphere_mat, d->n_spheres))) return rc;
    if ((rc = zr_scene_set_triangles(s, d->tri_v, d->tri_n, d->tri_mat, d->n_tris))) return rc;
    if ((rc = zr_scene_set_cubes(s, d->cubes, d->cube_mat, d->n_cubes))) return rc;
    if ((rc = zr_scene_set_media(s, d->media, d->n_media))) return rc;
    if ((rc = zr_scene_set_xform_ops(s, d->ops, d->n_ops))) return rc;
    if ((rc = zr_scene_set_objects(s, d->objects, d->n_objects))) return rc;
    if ((rc = zr_scene_set_groups(s, d->groups, d->n_groups))) return rc;
    if ((rc = zr_scene_set_materials(s, d->materials, d->n_materials))) return rc;
    return zr_scene_set_textures(s, d->textures, d->n_textures, d->texels, d->texel_bytes);
}

int zr_scene_set_all_borrowed(zr_scene* s, const zr_scene_desc* d) {
    CHECK_SCENE(s);
    if (!d) return fail(ZR_E_INVALID, "null scene description");
    if ((d->n_spheres && (!d->spheres || !d->sphere_mat)) || (d->n_tris && (!d->tri_v || !d->tri_n || !d->tri_mat)) || (d->n_cubes && (!d->cubes || !d->cube_mat)) ||
        (d->n_media && !d->media) || (d->n_ops && !d->ops) || (d->n_objects && !d->objects) || (d->texel_bytes && !d->texels))
        return fail(ZR_E_INVALID, "null array in the scene description");
    s->spheres.borrow(d->spheres, d->n_spheres * 4); s->sphere_mat.borrow(d->sphere_mat, d->n_spheres);
    s->tri_v.borrow(d->tri_v, d->n_tris * 9); s->tri_n.borrow(d->tri_n, d->n_tris * 9); s->tri_mat.borrow(d->tri_mat, d->n_tris);
    s->tri_uv.drop();
    s->cubes.borrow(d->cubes, d->n_cubes * 12); s->cube_mat.borrow(d->cube_mat, d->n_cubes);
    s->media.borrow(d->media, d->n_media);
    s->ops.borrow(d->ops, d->n_ops);
    s->objects.borrow(d->objects, d->n_objects); s->objects_set = d->n_objects > 0;
    s->texels.borrow((const unsigned char*)d->texels, d->texel_bytes);
    s->borrowed = true; s->released = false; s->reset_mask = 0;
    int rc;
    if ((rc = zr_scene_set_groups(s, d->groups, d->n_groups))) return rc;
    if ((rc = zr_scene_set_materials(s, d->materials, d->n_materials))) return rc;   // the small tables are copied: render calls validate against them
    if (d->n_textures && !d->textures) return fail(ZR_E_INVALID, "null texture array");
    s->textures.assign(d->textures, d->textures + d->n_textures);
    return ZR_OK;
}

int zr_scene_commit(zr_scene* s) {
    if (!s) return fail(ZR_E_INVALID, "null scene");
    if (s->released) return fail(ZR_E_STATE, "the arrays given to zr_scene_set_all_borrowed were released by the previous commit: set the scene again");
    s->committed = false;
    HIP_OK(hipSetDevice(s->ctx->device));
    static std::atomic<uint64_t> commits{0};
    s->stale = false; s->epoch = 0; s->serial = ++commits; s->refit.reset();   // (a new serial: a history tells a new commit from a refit)  // what updates and refits built on the previous commit (the refit state holds device memory)
    std::vector<zr_object>().swap(s->plan_objs); std::vector<uint8_t>().swap(s->plan_code); s->group_box.clear();
    PhaseTimer ph{"commit", 22};
    std::vector<zr_object> objs = world_list(*s);
    int rc = validate(*s, objs);
    if (rc) return rc;
    ph("world list + validate");
    if (s->media.size() > 65535) return fail(ZR_E_INVALID, "at most 65535 media (RNG key layout, zr_rng.h)");
    std::shared_ptr<const CommitPlan> plan = make_plan(*s, std::move(objs));
    // which builder.  ZR_BVH_BUILD=device | host forces one; otherwise worlds of at least ZR_BVH_DEVICE_MIN entries (131072: from
    // there on the device build's top is arranged by SAH, zr_build.h) are built on the device: cfg3's 1M triangles commit in
    // 19 ms instead of 106 and the frame takes 1 % longer than on the host's tree (EXTEND alone 2.6 %) — profiles/r3_builders.txt;
    // a small world is built faster by the host than a few dozen kernel launches take
    const char* bm = std::getenv("ZR_BVH_BUILD");
    const bool force_dev = bm && std::strcmp(bm, "device") == 0, force_host = bm && std::strcmp(bm, "host") == 0;
    const size_t n = plan->objs.size();
    const bool use_dev = !force_host && n != 0 && n < (1u << 30) && (force_dev || (double)n >= env_double("ZR_BVH_DEVICE_MIN", 131072));
    CommitSummary cs;
    DeviceBuild how = DeviceBuild::UseHost;
    if (use_dev) {
        rc = commit_device(s, *plan, ph, cs, how);
        if (how == DeviceBuild::Failed) return rc;
        if (how == DeviceBuild::UseHost) ph("device build refused");
    }
    std::shared_ptr<HostBuild> staging;
    if (how == DeviceBuild::UseHost && (rc = commit_host(s, plan, ph, cs, staging))) return rc;
    if ((rc = finish_commit(s, *plan, cs))) return rc;
    if (staging) {   // unmapping half a gigabyte of staging arrays takes tens of milliseconds: not on the caller's clock
        ph("upload");
        s->ctx->free_later([staging = std::move(staging), plan = std::move(plan)]() mutable { staging.reset(); plan.reset(); });
        ph("release");
    }
    return ZR_OK;
}

}  // extern "C"
