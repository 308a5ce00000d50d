// zr_update.h — the host half of a moving world (include/zr_capi.h: zr_scene_update_*, zr_scene_refit): which world-list entries an op or a sphere reaches,
// where each entry's leaf primitive lives in the committed arrays, the guard that an update leaves every entry's stored form as the commit classified it, and an
// entry's new box and record as patches for the device (zr_refit.h).  Nothing is derived anew: the box is zr_entry.h's chain_box, the record its put_entry, the
// classification zr_flatten.h's classify_object — a refitted scene then holds what a fresh commit of the moved world would hold, record for record.
// No HIP in here, like zr_flatten.h: zr_update.cpp includes it for the library, tests/native/update_check.cpp compiles it alone.
#pragma once
#include <map>

#include "zr_flatten.h"
#define ZR_REFIT_TYPES_ONLY   // the patch formats; zr_update.cpp includes zr_refit.h whole before this header
#include "zr_refit.h"
#undef ZR_REFIT_TYPES_ONLY

namespace {

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

// the committed world as updates see it: the scene's own copy of the arrays (writable), and what the commit kept of its plan
struct UpdateWorld {
    SceneInput& s;
    const std::vector<zr_object>& objs;          // CommitPlan::objs
    const std::vector<uint8_t>& code;            // CommitPlan::code: leaf kind | baked << 4
    bool bake;                                   // BuildKnobs::bake
    const std::vector<zr::BuildBox>& group_box;  // per zr_group
    zr::BuildSceneIn view() const { return scene_view(s, &group_box); }
    uint32_t kind(size_t oi) const { return code[oi] & 7u; }
};

// one entry's record in the arrays of its kind, as put_entry writes it (zr_entry.h), for one record at index 0
struct EntryRecord {
    double sphere[ZR_SPHERE_DOUBLES], tri_v[ZR_TRI_STRIDE], tri_s[ZR_TRI_SHADE_DOUBLES], cube[ZR_CUBE_DOUBLES], pcube[ZR_PCUBE_STRIDE];
    uint32_t sphere_mat = 0, cube_mat = 0, pcube_mat = 0;
    void make(const UpdateWorld& w, const zr::BuildSceneIn& in, uint32_t oi) {
        zr::BuildPrimOut out;
        out.spheres = sphere; out.sphere_mat = &sphere_mat; out.tri_v = tri_v; out.tri_s = tri_s; out.cubes = cube; out.cube_mat = &cube_mat;
        out.pcubes = pcube; out.pcube_mat = &pcube_mat;
        zr::put_entry(in, out, w.objs[oi], w.code[oi] >> 4, 0);
    }
};

// an entry's new box and, for the stored forms that hold the placement in the record itself, its new record
struct EntryPatch {
    zr::RefitBoxPatch box;
    uint32_t rec_doubles = 0;   // 0: the record does not change (a wrapped object, a medium, a placed group: their chains live in the op array)
    double rec[18];
    bool finite = true;
};
inline uint32_t record_doubles(uint32_t kind, uint32_t baked) {   // of the patch of an entry of this stored form
    if (kind == ZR_PRIM_SPHERE) return ZR_SPHERE_DOUBLES;          // bare, material-only chain, baked: the sphere's four numbers
    if (kind == ZR_PRIM_TRIANGLE && baked == 1) return 18;         // baked: vertices and vertex normals (a bare triangle cannot move)
    if (kind == ZR_KIND_PCUBE) return ZR_PCUBE_STRIDE;
    return 0;
}
inline EntryPatch entry_patch(const UpdateWorld& w, const zr::BuildSceneIn& in, uint32_t oi, uint32_t di) {
    EntryPatch p;
    const zr_object& o = w.objs[oi];
    const zr::BuildBox b = zr::chain_box(in, o.type, o.index, o.chain_first, o.chain_count);
    p.box.kind = w.kind(oi); p.box.di = di;
    for (int a = 0; a < 3; a++) {
        if (!std::isfinite(b.lo[a]) || !std::isfinite(b.hi[a])) p.finite = false;
        p.box.lo[a] = f_down(b.lo[a]); p.box.hi[a] = f_up(b.hi[a]);
    }
    p.rec_doubles = record_doubles(w.kind(oi), w.code[oi] >> 4);
    if (p.rec_doubles) {
        EntryRecord r{};
        r.make(w, in, oi);
        if (w.kind(oi) == ZR_PRIM_SPHERE) std::memcpy(p.rec, r.sphere, sizeof r.sphere);
        else if (w.kind(oi) == ZR_PRIM_TRIANGLE) std::memcpy(p.rec, r.tri_s, 18 * sizeof(double));   // (words 0-8 are the vertex record's too)
        else std::memcpy(p.rec, r.pcube, sizeof r.pcube);
    }
    return p;
}

struct UpdateIndex {
    std::vector<uint32_t> op_at, op_entries;     // op k reaches entries op_entries[op_at[k] .. op_at[k + 1]): through their own chain, or as media through the medium's inner chain
    std::vector<uint32_t> sph_at, sph_entries;   // sphere k is the leaf primitive of entries sph_entries[sph_at[k] .. sph_at[k + 1]) (bare, material-only chain, baked)
    std::vector<uint8_t> sph_locked;             // sphere k is a medium's boundary or sits inside a generic (wrapped) chain: its numbers cannot be updated
    std::vector<uint32_t> slot;                  // per entry: the index of its leaf primitive in the array of its kind
    std::vector<uint8_t> dirty;                  // per entry: reached by an update since the last refit
    std::vector<uint32_t> dirty_list;
    size_t op_lo = (size_t)-1, op_hi = 0;        // the ops changed since the last refit: [op_lo, op_hi)
    size_t movable = 0, movable_doubles = 0;     // entries any update can reach and the doubles of their record patches: the most one refit can send

    template <class F> static void ops_of(const UpdateWorld& w, uint32_t oi, F&& f) {
        const zr_object& o = w.objs[oi];
        for (uint32_t k = 0; k < o.chain_count; k++) f(o.chain_first + k);
        if (o.type == ZR_PRIM_MEDIUM) { const zr_medium& m = w.s.media[o.index]; for (uint32_t k = 0; k < m.chain_count; k++) f(m.chain_first + k); }
    }
    void build_reverse(const UpdateWorld& w) {
        const size_t n = w.objs.size(), n_ops = w.s.ops.size(), n_sph = w.s.sphere_mat.size();
        op_at.assign(n_ops + 1, 0); sph_at.assign(n_sph + 1, 0); sph_locked.assign(n_sph, 0);
        auto leaf_sphere = [&](size_t oi) { return w.objs[oi].type == ZR_PRIM_SPHERE && w.kind(oi) == ZR_PRIM_SPHERE; };
        for (size_t oi = 0; oi < n; oi++) {
            ops_of(w, (uint32_t)oi, [&](uint32_t op) { op_at[op + 1]++; });
            if (leaf_sphere(oi)) sph_at[w.objs[oi].index + 1]++;
            else if (w.objs[oi].type == ZR_PRIM_SPHERE) sph_locked[w.objs[oi].index] = 1;
        }
        for (const zr_medium& m : w.s.media) if (m.boundary_type == ZR_PRIM_SPHERE) sph_locked[m.boundary_index] = 1;
        for (size_t k = 0; k < n_ops; k++) op_at[k + 1] += op_at[k];
        for (size_t k = 0; k < n_sph; k++) sph_at[k + 1] += sph_at[k];
        op_entries.resize(op_at[n_ops]); sph_entries.resize(sph_at[n_sph]);
        std::vector<uint32_t> oa(op_at.begin(), op_at.end() - 1), sa(sph_at.begin(), sph_at.end() - 1);
        movable = 0; movable_doubles = 0;
        for (size_t oi = 0; oi < n; oi++) {
            bool reach = false;
            ops_of(w, (uint32_t)oi, [&](uint32_t op) { op_entries[oa[op]++] = (uint32_t)oi; reach = true; });
            if (leaf_sphere(oi)) { sph_entries[sa[w.objs[oi].index]++] = (uint32_t)oi; reach = true; }
            if (reach) { movable++; movable_doubles += record_doubles(w.kind(oi), w.code[oi] >> 4); }
        }
        dirty.assign(n, 0); dirty_list.clear(); op_lo = (size_t)-1; op_hi = 0;
    }

    // entry -> leaf primitive, inverted from the back-references the commit kept (zr_scene::leaf_src: a wrapped object's and a placement's name the entry, the
    // plain kinds' name the caller's primitive).  Entries that share a primitive of a plain kind — one sphere baked under two chains — are told apart by their
    // records: fetch(kind, di, rec, mat) reads the committed record of leaf primitive di (a sphere's 4 doubles, a triangle's 9 vertices, a cube's 6, a placed
    // cube's 16, and its material word); entries with equal records are interchangeable.  Must run while the host arrays still hold the committed values.
    template <class Fetch>
    int build_slots(const UpdateWorld& w, const std::vector<uint32_t>* leaf_src, const uint32_t* cnt, Fetch&& fetch) {
        const size_t n = w.objs.size();
        slot.assign(n, kNoSlot);
        const zr::BuildSceneIn in = w.view();
        for (uint32_t k : {(uint32_t)ZR_KIND_WRAPPED, (uint32_t)ZR_KIND_INSTANCE}) {
            if (leaf_src[k].size() < cnt[k]) return fail(ZR_E_DEVICE, "refit: %zu back-references of kind %u, %u leaf primitives (internal error)", leaf_src[k].size(), k, cnt[k]);
            for (uint32_t di = 0; di < cnt[k]; di++) {
                const uint32_t oi = leaf_src[k][di];
                if (oi >= n || w.kind(oi) != k || slot[oi] != kNoSlot) return fail(ZR_E_DEVICE, "refit: leaf primitive %u of kind %u names entry %u wrongly (internal error)", di, k, oi);
                slot[oi] = di;
            }
        }
        for (uint32_t k : {(uint32_t)ZR_PRIM_SPHERE, (uint32_t)ZR_PRIM_TRIANGLE, (uint32_t)ZR_PRIM_CUBE, (uint32_t)ZR_PRIM_MEDIUM, (uint32_t)ZR_KIND_PCUBE}) {
            if (cnt[k] == 0) continue;
            if (leaf_src[k].size() < cnt[k]) return fail(ZR_E_DEVICE, "refit: %zu back-references of kind %u, %u leaf primitives (internal error)", leaf_src[k].size(), k, cnt[k]);
            const size_t n_prim = k == ZR_PRIM_SPHERE ? w.s.sphere_mat.size() : k == ZR_PRIM_TRIANGLE ? w.s.tri_mat.size() : k == ZR_PRIM_MEDIUM ? w.s.media.size() : w.s.cube_mat.size();
            std::vector<uint32_t> first_di(n_prim, kNoSlot);
            std::map<uint32_t, std::vector<uint32_t>> more;   // primitive -> all its leaf primitives, when it has several
            for (uint32_t di = 0; di < cnt[k]; di++) {
                const uint32_t p = leaf_src[k][di];
                if (p >= n_prim) return fail(ZR_E_DEVICE, "refit: leaf primitive %u of kind %u names primitive %u of %zu (internal error)", di, k, p, n_prim);
                if (first_di[p] == kNoSlot) first_di[p] = di;
                else { auto& v = more[p]; if (v.empty()) v.push_back(first_di[p]); v.push_back(di); }
            }
            std::map<uint32_t, std::vector<uint32_t>> shared;   // primitive -> the entries that share it
            for (size_t oi = 0; oi < n; oi++) {
                if (w.kind(oi) != k) continue;
                const uint32_t p = w.objs[oi].index;
                if (first_di[p] == kNoSlot) return fail(ZR_E_DEVICE, "refit: entry %zu has no leaf primitive (internal error)", oi);
                if (more.count(p)) shared[p].push_back((uint32_t)oi);
                else if (first_di[p] & 0x80000000u) return fail(ZR_E_DEVICE, "refit: two entries for one leaf primitive (internal error)");
                else { slot[oi] = first_di[p]; first_di[p] |= 0x80000000u; }   // (taken)
            }
            for (auto& [p, dis] : more) {
                std::vector<uint32_t>& ents = shared[p];
                if (ents.size() != dis.size()) return fail(ZR_E_DEVICE, "refit: primitive %u has %zu leaf primitives and %zu entries (internal error)", p, dis.size(), ents.size());
                for (uint32_t di : dis) {
                    double rec[ZR_PCUBE_STRIDE] = {}; uint32_t mat = 0;
                    if (int rc = fetch(k, di, rec, mat)) return rc;
                    size_t hit = ents.size();
                    for (size_t e = 0; e < ents.size() && hit == ents.size(); e++) {
                        if (ents[e] == kNoSlot) continue;
                        EntryRecord r{};
                        if (k != ZR_PRIM_MEDIUM) r.make(w, in, ents[e]);
                        uint64_t tmat = 0; std::memcpy(&tmat, &r.tri_s[18], 8);
                        const bool same = k == ZR_PRIM_MEDIUM ? true
                                        : k == ZR_PRIM_SPHERE ? (std::memcmp(rec, r.sphere, sizeof r.sphere) == 0 && mat == r.sphere_mat)
                                        : k == ZR_PRIM_TRIANGLE ? (std::memcmp(rec, r.tri_v, 9 * sizeof(double)) == 0 && mat == (uint32_t)tmat)
                                        : k == ZR_PRIM_CUBE ? (std::memcmp(rec, r.cube, sizeof r.cube) == 0 && mat == r.cube_mat)
                                        : (std::memcmp(rec, r.pcube, sizeof r.pcube) == 0 && mat == r.pcube_mat);
                        if (same) hit = e;
                    }
                    if (hit == ents.size()) return fail(ZR_E_DEVICE, "refit: no entry of primitive %u (kind %u) wrote leaf primitive %u (internal error)", p, k, di);
                    slot[ents[hit]] = di; ents[hit] = kNoSlot;
                }
            }
        }
        for (size_t oi = 0; oi < n; oi++) if (slot[oi] == kNoSlot || slot[oi] >= cnt[w.kind(oi)]) return fail(ZR_E_DEVICE, "refit: entry %zu has no leaf primitive (internal error)", oi);
        return ZR_OK;
    }

    void mark(uint32_t oi) { if (!dirty[oi]) { dirty[oi] = 1; dirty_list.push_back(oi); } }
    void clear_dirty() { for (uint32_t oi : dirty_list) dirty[oi] = 0; dirty_list.clear(); op_lo = (size_t)-1; op_hi = 0; }

    // zr_scene_update_xform_ops on the host copy: everything is checked before anything stays changed
    int update_ops(UpdateWorld& w, size_t first, const zr_xform_op* ops, size_t n) {
        const size_t have = w.s.ops.size();
        if (first > have || n > have - first) return fail(ZR_E_INVALID, "ops [%zu, %zu + %zu) leave the %zu committed ops", first, first, n, have);
        if (n == 0) return ZR_OK;
        if (!ops) return fail(ZR_E_INVALID, "null op array");
        zr_xform_op* mine = w.s.ops.own_data();
        if (!mine) return fail(ZR_E_STATE, "the scene holds no copy of its ops");
        for (size_t k = 0; k < n; k++) {
            if (ops[k].kind != mine[first + k].kind || ops[k].mat != mine[first + k].mat)
                return fail(ZR_E_INVALID, "op %zu: kind or material differ from the committed op's (only a[3] may change)", first + k);
            for (int a = 0; a < 3; a++) if (!std::isfinite(ops[k].a[a])) return fail(ZR_E_INVALID, "op %zu: a[%d] is not finite", first + k, a);
        }
        const std::vector<zr_xform_op> old(mine + first, mine + first + n);
        std::copy(ops, ops + n, mine + first);
        for (size_t k = first; k < first + n; k++)
            for (uint32_t e = op_at[k]; e < op_at[k + 1]; e++) {
                const uint32_t oi = op_entries[e];
                uint32_t kind; uint8_t bk;
                classify_object(w.s, w.objs[oi], w.bake, kind, bk);
                if ((uint8_t)(kind | (bk << 4)) != w.code[oi]) {
                    std::copy(old.begin(), old.end(), mine + first);
                    return fail(ZR_E_INVALID, "op %zu: world-list entry %u would be stored in another form than the commit chose (%u/%u, committed %u/%u): commit anew", k, oi, kind,
                                (unsigned)bk, w.code[oi] & 7u, w.code[oi] >> 4);
                }
            }
        for (size_t k = first; k < first + n; k++) for (uint32_t e = op_at[k]; e < op_at[k + 1]; e++) mark(op_entries[e]);
        op_lo = std::min(op_lo, first); op_hi = std::max(op_hi, first + n);
        return ZR_OK;
    }
    // zr_scene_update_spheres on the host copy
    int update_spheres(UpdateWorld& w, size_t first, const double* cxyz_r, size_t n) {
        const size_t have = w.s.sphere_mat.size();
        if (first > have || n > have - first) return fail(ZR_E_INVALID, "spheres [%zu, %zu + %zu) leave the %zu committed spheres", first, first, n, have);
        if (n == 0) return ZR_OK;
        if (!cxyz_r) return fail(ZR_E_INVALID, "null sphere array");
        double* mine = w.s.spheres.own_data();
        if (!mine) return fail(ZR_E_STATE, "the scene holds no copy of its spheres");
        for (size_t k = 0; k < n * 4; k++) if (!std::isfinite(cxyz_r[k])) return fail(ZR_E_INVALID, "sphere %zu: value %zu is not finite", first + k / 4, k % 4);
        for (size_t k = first; k < first + n; k++)
            if (sph_locked[k]) return fail(ZR_E_INVALID, "sphere %zu is a medium's boundary or sits inside a generic wrapper chain: it is no leaf primitive of its own", k);
        std::copy(cxyz_r, cxyz_r + n * 4, mine + first * 4);
        for (size_t k = first; k < first + n; k++) for (uint32_t e = sph_at[k]; e < sph_at[k + 1]; e++) mark(sph_entries[e]);
        return ZR_OK;
    }
};

}  // namespace
