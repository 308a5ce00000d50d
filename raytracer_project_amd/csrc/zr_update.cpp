// zr_update.cpp — moving worlds (include/zr_capi.h): zr_scene_update_xform_ops / zr_scene_update_spheres change the host copy of a committed world and mark
// the scene stale; zr_scene_refit makes the device scene agree — the moved entries' records and boxes as compact patches, the op range, then the boxes of the
// world's trees level by level (zr_refit.hip).  The host rules are zr_update.h's (no HIP); this file holds the refit state and talks to the device.
#include "zr_host_internal.h"
#include "zr_refit.h"
#include "zr_update.h"
#include "zr_motion.h"

// What a refit works from, made once per commit (by the first update or refit after it) and dropped by the next commit.
struct RefitState {
    UpdateIndex ix;                      // reverse indices, entry -> leaf primitive, the dirty set
    std::vector<float> host_box[7];      // the committed boxes of the leaf primitives, until they are on the device
    // device side, made by the first refit: nothing below is allocated or freed by a later one
    bool on_device = false;
    DevBuf<float> prim_box[7], quad_box, pair_box;
    DevBuf<uint32_t> q_order, p_order;
    std::vector<zr::RefitLevel> q_levels, p_levels;   // deepest first
    uint32_t n_blocks = 0;               // per-block partial sums of the pair kernels
    DevBuf<unsigned char> d_result;      // RefitResult, then n_blocks doubles
    DevBuf<zr::RefitBoxPatch> d_box; DevBuf<zr::RefitRecPatch> d_rec; DevBuf<double> d_payload;
    // pinned staging: the patches, the changed ops, the read-back
    zr::RefitBoxPatch* h_box = nullptr; zr::RefitRecPatch* h_rec = nullptr; double* h_payload = nullptr; zr_xform_op* h_ops = nullptr; unsigned char* h_result = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // the motion of the last refit (zr_motion.h).  Host: every movable entry's map as of the previous epoch and the last refit's records; per leaf
    // primitive of the world's tree, addressed leaf_base[kind] + index, its entry.  Device, allocated with the rest and never again: one word per leaf primitive
    // (a slot, STATIC, CUT); the records live in d_payload behind the record patches, from motion_at on, until the next refit overwrites them.
    MotionTable motion;
    std::vector<uint32_t> leaf_entry; uint32_t leaf_base[8] = {}, n_leaves = 0;
    DevBuf<uint32_t> d_leaf_word, d_leaf_entry;
    std::vector<uint32_t> marked;        // the entries whose leaf word on the device is not STATIC
    size_t motion_at = 0;
    double area0 = 0;                    // sum of the half-areas of the world tree's pair boxes as the refit kernels compute it over the committed world
    ~RefitState() {
        for (void* p : {(void*)h_box, (void*)h_rec, (void*)h_payload, (void*)h_ops, (void*)h_result}) if (p) (void)hipHostFree(p);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
    size_t result_bytes() const { return sizeof(zr::RefitResult) + (size_t)n_blocks * sizeof(double); }
};

namespace {

UpdateWorld world_of(zr_scene* s) { return UpdateWorld{*s, s->plan_objs, s->plan_code, s->plan_bake, s->group_box}; }

// what every update checks first
int update_ready(zr_scene* s, const char* entry) {
    if (!s) return fail(ZR_E_INVALID, "null scene");
    if (!s->committed) return fail(ZR_E_STATE, "zr_scene_commit must precede %s", entry);
    if (s->released) return fail(ZR_E_STATE, "%s: the scene was committed from borrowed arrays, which it has released: give it with zr_scene_set_all to move it", entry);
    return ZR_OK;
}

// The host half of the refit state: reverse indices, every entry's leaf primitive, the committed boxes.  Runs before the first update changes anything.
int ensure_index(zr_scene* s) {
    if (s->refit) return ZR_OK;
    HIP_OK(hipSetDevice(s->ctx->device));
    auto st = std::make_shared<RefitState>();
    UpdateWorld w = world_of(s);
    st->ix.build_reverse(w);
    // committed records of the leaf primitives that share a caller's primitive: read back whole arrays, once, only when such entries exist
    std::vector<double> rec[8]; std::vector<uint32_t> mats[8];
    auto fetch = [&](uint32_t kind, uint32_t di, double* out, uint32_t& mat) -> int {
        if (kind == ZR_PRIM_MEDIUM) return ZR_OK;
        const double* d_src = kind == ZR_PRIM_SPHERE ? s->d_spheres.p : kind == ZR_PRIM_TRIANGLE ? s->d_tri_v.p : kind == ZR_PRIM_CUBE ? s->d_cubes.p : s->d_pcubes.p;
        const size_t per = kind == ZR_PRIM_SPHERE ? ZR_SPHERE_DOUBLES : kind == ZR_PRIM_TRIANGLE ? ZR_TRI_STRIDE : kind == ZR_PRIM_CUBE ? ZR_CUBE_DOUBLES : ZR_PCUBE_STRIDE;
        const size_t n = s->plan_cnt[kind];
        if (rec[kind].empty()) {
            rec[kind].resize(n * per); mats[kind].resize(n);
            HIP_OK(hipStreamSynchronize(s->ctx->stream));
            HIP_OK(hipMemcpy(rec[kind].data(), d_src, n * per * sizeof(double), hipMemcpyDeviceToHost));
            if (kind == ZR_PRIM_TRIANGLE) {   // the material: the low word of word 18 of the shading record
                std::vector<double> ts(n * ZR_TRI_SHADE_DOUBLES);
                HIP_OK(hipMemcpy(ts.data(), s->d_tri_s.p, ts.size() * sizeof(double), hipMemcpyDeviceToHost));
                for (size_t k = 0; k < n; k++) { uint64_t m; std::memcpy(&m, &ts[k * ZR_TRI_SHADE_DOUBLES + 18], 8); mats[kind][k] = (uint32_t)m; }
            } else {
                const uint32_t* d_mat = kind == ZR_PRIM_SPHERE ? s->d_sphere_mat.p : kind == ZR_PRIM_CUBE ? s->d_cube_mat.p : s->d_pcube_mat.p;
                HIP_OK(hipMemcpy(mats[kind].data(), d_mat, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
            }
        }
        std::memcpy(out, &rec[kind][(size_t)di * per], per * sizeof(double));
        mat = mats[kind][di];
        return ZR_OK;
    };
    if (int rc = st->ix.build_slots(w, s->leaf_src, s->plan_cnt, fetch)) return rc;
    for (int k = 0; k < 7; k++) st->host_box[k].assign((size_t)s->plan_cnt[k] * 6, 0.0f);
    const zr::BuildSceneIn in = w.view();
    std::atomic<size_t> bad{(size_t)-1};
    parallel_split(w.objs.size(), [&](size_t a, size_t b) {
        for (size_t oi = a; oi < b; oi++) {
            const EntryPatch p = entry_patch(w, in, (uint32_t)oi, st->ix.slot[oi]);
            if (!p.finite) { size_t want = (size_t)-1; bad.compare_exchange_strong(want, oi); }
            float* d = &st->host_box[p.box.kind][(size_t)p.box.di * 6];
            for (int c = 0; c < 3; c++) { d[c] = p.box.lo[c]; d[3 + c] = p.box.hi[c]; }
        }
    });
    if (bad.load() != (size_t)-1) return fail(ZR_E_DEVICE, "refit: committed entry %zu has a box that is not finite (internal error)", bad.load());
    for (int k = 0; k < 7; k++) st->leaf_base[k + 1] = st->leaf_base[k] + s->plan_cnt[k];
    st->n_leaves = st->leaf_base[7];
    st->leaf_entry.assign(st->n_leaves, kNoSlot);
    for (size_t oi = 0; oi < w.objs.size(); oi++) st->leaf_entry[st->leaf_base[w.kind(oi)] + st->ix.slot[oi]] = (uint32_t)oi;
    st->motion.build(w);
    s->refit = std::move(st);
    return ZR_OK;
}

template <class T> int pinned(T*& p, size_t count) {
    HIP_OK(hipHostMalloc((void**)&p, std::max<size_t>(count * sizeof(T), 64), hipHostMallocDefault));
    return ZR_OK;
}

// the world's trees as a refit walks them: nodes by level, deepest first, derived from the committed records of either builder (group subtrees are not entered)
int make_schedule(zr_scene* s, RefitState& st) {
    const size_t n_quads = s->d_quads.n, n_pairs = s->d_nodes.n;
    std::vector<zr::NodeQ> quads(n_quads);
    std::vector<zr::NodePair> pairs(n_pairs);
    if (n_quads) HIP_OK(hipMemcpy(quads.data(), s->d_quads.p, n_quads * sizeof(zr::NodeQ), hipMemcpyDeviceToHost));
    if (n_pairs) HIP_OK(hipMemcpy(pairs.data(), s->d_nodes.p, n_pairs * sizeof(zr::NodePair), hipMemcpyDeviceToHost));
    const uint32_t* cnt = s->plan_cnt;
    auto leaf_ok = [&](uint32_t kind, uint32_t first, uint32_t count) { return kind < 7 && count >= 1 && (uint64_t)first + count <= cnt[kind]; };
    // 4-wide nodes: from the FP32 root's references
    std::vector<std::vector<uint32_t>> levels;
    std::vector<uint8_t> seen(n_quads, 0);
    auto scan_refs = [&](const uint32_t refs[4], std::vector<uint32_t>& next) -> int {
        bool ended = false;
        for (int c = 0; c < 4; c++) {
            const uint32_t r = refs[c];
            if (r == ZR_REF_EMPTY) { ended = true; continue; }
            if (ended) return fail(ZR_E_DEVICE, "refit: a 4-wide node's children are not at its first slots (internal error)");
            if (r & ZR_REF_LEAF) { if (!leaf_ok((r >> 28) & 7u, r & 0xFFFFFFu, ((r >> 24) & 15u) + 1u)) return fail(ZR_E_DEVICE, "refit: leaf reference %#x outside the leaf primitives (internal error)", r); }
            else { if (r >= n_quads || seen[r]) return fail(ZR_E_DEVICE, "refit: node reference %u outside the %zu nodes, or met twice (internal error)", r, n_quads); seen[r] = 1; next.push_back(r); }
        }
        return ZR_OK;
    };
    {
        std::vector<uint32_t> next;
        if (int rc = scan_refs(s->ds.root.ref, next)) return rc;
        while (!next.empty()) {
            if (levels.size() > 2 * ZR_STACK_DEPTH) return fail(ZR_E_DEVICE, "refit: 4-wide tree deeper than the traversal stack (internal error)");
            levels.push_back(std::move(next));
            next.clear();
            for (uint32_t q : levels.back()) if (int rc = scan_refs(quads[q].ref, next)) return rc;
        }
    }
    std::vector<uint32_t> order;
    st.q_levels.clear();
    for (size_t l = levels.size(); l-- > 0;) { st.q_levels.push_back({(uint32_t)order.size(), (uint32_t)levels[l].size(), 0u}); order.insert(order.end(), levels[l].begin(), levels[l].end()); }
    if (int rc = st.q_order.upload(order)) return rc;
    // pair records: from record 0
    levels.clear(); order.clear();
    std::vector<uint8_t> pseen(n_pairs, 0);
    auto empty = [](uint32_t meta) { return meta != 0 && (meta & 0xFFFFu) == 0; };
    if (n_pairs && !(empty(pairs[0].meta[0]) && empty(pairs[0].meta[1]))) {
        std::vector<uint32_t> next{0u};
        pseen[0] = 1;
        while (!next.empty()) {
            if (levels.size() > 2 * ZR_STACK_DEPTH) return fail(ZR_E_DEVICE, "refit: pair tree deeper than the traversal stack (internal error)");
            levels.push_back(std::move(next));
            next.clear();
            for (uint32_t p : levels.back())
                for (int c = 0; c < 2; c++) {
                    const uint32_t meta = pairs[p].meta[c], ch = pairs[p].child[c];
                    if (empty(meta)) continue;
                    if (meta == 0) { if (ch >= n_pairs || pseen[ch]) return fail(ZR_E_DEVICE, "refit: pair reference %u outside the %zu records, or met twice (internal error)", ch, n_pairs); pseen[ch] = 1; next.push_back(ch); }
                    else if (!leaf_ok((meta >> 16) - 1u, ch, meta & 0xFFFFu)) return fail(ZR_E_DEVICE, "refit: pair leaf %#x at %u outside the leaf primitives (internal error)", meta, ch);
                }
        }
    }
    st.p_levels.clear(); st.n_blocks = 0;
    for (size_t l = levels.size(); l-- > 0;) {
        st.p_levels.push_back({(uint32_t)order.size(), (uint32_t)levels[l].size(), st.n_blocks});
        st.n_blocks += ((uint32_t)levels[l].size() + 255u) / 256u;
        order.insert(order.end(), levels[l].begin(), levels[l].end());
    }
    return st.p_order.upload(order);
}

zr::RefitScene device_view(zr_scene* s, RefitState& st) {
    zr::RefitScene v{};
    v.quads = s->d_quads.p; v.pairs = s->d_nodes.p;
    for (int k = 0; k < 7; k++) v.prim_box[k] = st.prim_box[k].p;
    v.quad_box = st.quad_box.p; v.pair_box = st.pair_box.p;
    v.spheres = s->d_spheres.p; v.tri_v = s->d_tri_v.p; v.tri_s = s->d_tri_s.p; v.pcubes = s->d_pcubes.p;
    return v;
}

// the level launches and the one read-back: root, quantisation flag, partial sums -> st.h_result (valid after the caller's stream synchronisation)
int queue_trees(zr_scene* s, RefitState& st) {
    hipStream_t q = s->ctx->stream;
    const zr::RefitScene v = device_view(s, st);
    zr::RefitResult* d_res = (zr::RefitResult*)st.d_result.p;
    HIP_OK(hipMemsetAsync(st.d_result.p, 0, st.result_bytes(), q));
    HIP_OK(zr::refit_quads(q, v, st.q_order.p, st.q_levels.data(), st.q_levels.size(), s->ds.root, d_res));
    HIP_OK(zr::refit_pairs(q, v, st.p_order.p, st.p_levels.data(), st.p_levels.size(), (double*)(st.d_result.p + sizeof(zr::RefitResult))));
    HIP_OK(hipEventRecord(st.ev1, q));
    HIP_OK(hipMemcpyAsync(st.h_result, st.d_result.p, st.result_bytes(), hipMemcpyDeviceToHost, q));
    return ZR_OK;
}
// after the synchronisation: the new root into the kernel arguments, the sum of the pair boxes' half-areas (block order: the same bits for the same boxes)
int take_result(zr_scene* s, RefitState& st, double& area) {
    zr::RefitResult res;
    std::memcpy(&res, st.h_result, sizeof res);
    if (res.quant_fail) return fail(ZR_E_INVALID, "refit: a box of the moved world cannot be put on a 4-wide node's grid (not finite, or beyond 1e30): commit anew");
    s->ds.root = res.root;
    area = 0;
    for (uint32_t b = 0; b < st.n_blocks; b++) { double x; std::memcpy(&x, st.h_result + sizeof res + (size_t)b * sizeof(double), sizeof x); area += x; }
    return ZR_OK;
}

// The device half, by the first refit of a commit: the schedule, every buffer a refit will ever use, the committed boxes, and one pass of the tree kernels over
// the unmoved world — its area sum is the 1.0 of zr_refit_info::area_ratio, so the ratio compares like with like (the builders round their boxes in their own ways).
int ensure_device(zr_scene* s, RefitState& st) {
    if (st.on_device) return ZR_OK;
    if (!s->quad_ok) return fail(ZR_E_INVALID, "refit: the world's leaf references do not fit the 4-wide nodes (more than 2^24 primitives of a kind): commit anew");
    hipStream_t q = s->ctx->stream;
    HIP_OK(hipStreamSynchronize(q));
    if (int rc = make_schedule(s, st)) return rc;
    int rc;
    for (int k = 0; k < 7; k++) { if ((rc = st.prim_box[k].upload(st.host_box[k]))) return rc; std::vector<float>().swap(st.host_box[k]); }
    if ((rc = st.quad_box.alloc(s->d_quads.n * 6)) || (rc = st.pair_box.alloc(s->d_nodes.n * 6)) || (rc = st.d_result.alloc(st.result_bytes()))) return rc;
    const size_t m = st.ix.movable, md = st.ix.movable_doubles + m * (kMotionDoubles + 2), n_ops = s->ops.size();   // (behind the record patches: the motion records, then two leaf-word pairs per entry)
    if ((rc = st.d_leaf_word.alloc(st.n_leaves))) return rc;
    HIP_OK(hipMemset(st.d_leaf_word.p, 0xFF, std::max<size_t>(st.n_leaves * sizeof(uint32_t), 4)));   // ZR_MOTION_STATIC
    if ((rc = st.d_box.alloc(m)) || (rc = st.d_rec.alloc(m)) || (rc = st.d_payload.alloc(md))) return rc;
    if ((rc = pinned(st.h_box, m)) || (rc = pinned(st.h_rec, m)) || (rc = pinned(st.h_payload, md)) || (rc = pinned(st.h_ops, n_ops)) || (rc = pinned(st.h_result, st.result_bytes()))) return rc;
    HIP_OK(hipEventCreate(&st.ev0));
    HIP_OK(hipEventCreate(&st.ev1));
    if ((rc = queue_trees(s, st))) return rc;
    HIP_OK(hipStreamSynchronize(q));
    if ((rc = take_result(s, st, st.area0))) return rc;
    st.on_device = true;
    return ZR_OK;
}

int refit(zr_scene* s, zr_refit_info& info) {
    const double t0 = PhaseTimer::now();
    HIP_OK(hipSetDevice(s->ctx->device));
    int rc;
    if ((rc = ensure_index(s))) return rc;
    RefitState& st = *s->refit;
    if ((rc = ensure_device(s, st))) return rc;
    hipStream_t q = s->ctx->stream;
    UpdateIndex& ix = st.ix;
    UpdateWorld w = world_of(s);
    // 1. the dirty entries as patches, by the shared rules on the host (zr_update.h)
    const size_t nd = ix.dirty_list.size();
    if (nd > ix.movable) return fail(ZR_E_DEVICE, "refit: %zu dirty entries, %zu can move (internal error)", nd, ix.movable);
    std::vector<uint32_t> rec_at(nd + 1, 0);   // where each entry's record patch and payload go: a prefix sum, so the patches can be made by all threads
    std::vector<uint32_t> rec_no(nd + 1, 0);
    for (size_t k = 0; k < nd; k++) {
        const uint32_t oi = ix.dirty_list[k], doubles = record_doubles(w.kind(oi), w.code[oi] >> 4);
        rec_at[k + 1] = rec_at[k] + doubles; rec_no[k + 1] = rec_no[k] + (doubles ? 1u : 0u);
    }
    if (rec_at[nd] > ix.movable_doubles) return fail(ZR_E_DEVICE, "refit: patch payload beyond its buffer (internal error)");
    const zr::BuildSceneIn in = w.view();
    std::atomic<size_t> bad{(size_t)-1};
    parallel_split(nd, [&](size_t a, size_t b) {
        for (size_t k = a; k < b; k++) {
            const uint32_t oi = ix.dirty_list[k];
            const EntryPatch p = entry_patch(w, in, oi, ix.slot[oi]);
            if (!p.finite) { size_t want = (size_t)-1; bad.compare_exchange_strong(want, (size_t)oi); }
            st.h_box[k] = p.box;
            if (p.rec_doubles) {
                st.h_rec[rec_no[k]] = zr::RefitRecPatch{p.box.kind, p.box.di, rec_at[k], p.rec_doubles};
                std::memcpy(st.h_payload + rec_at[k], p.rec, p.rec_doubles * sizeof(double));
            }
        }
    });
    if (bad.load() != (size_t)-1) return fail(ZR_E_INVALID, "refit: world-list entry %zu has a box that is not finite: commit anew", bad.load());
    // 1b. the motion of this step (zr_motion.h): records behind the record patches, then one (leaf address, word) pair per entry whose word changes — the entries
    // of the previous table that did not move again go back to STATIC.  They ride in the payload copy; the table is the scene's from here on.
    st.motion.step(w, ix.dirty_list);
    st.motion_at = rec_at[nd];
    const size_t n_mrec = st.motion.records.size();
    if (n_mrec) std::memcpy(st.h_payload + st.motion_at, st.motion.records.data(), n_mrec * sizeof(double));
    uint32_t* pairs = (uint32_t*)(st.h_payload + st.motion_at + n_mrec);
    uint32_t n_pairs = 0;
    auto leaf_of = [&](uint32_t oi) { return st.leaf_base[w.kind(oi)] + ix.slot[oi]; };
    for (uint32_t oi : st.marked) if (!ix.dirty[oi]) { pairs[2 * n_pairs] = leaf_of(oi); pairs[2 * n_pairs + 1] = kMotionStatic; n_pairs++; }
    for (size_t k = 0; k < nd; k++) { pairs[2 * n_pairs] = leaf_of(ix.dirty_list[k]); pairs[2 * n_pairs + 1] = st.motion.slot[k]; n_pairs++; }
    st.marked = ix.dirty_list;
    const size_t payload_doubles = st.motion_at + n_mrec + n_pairs;
    if (payload_doubles > st.d_payload.n) return fail(ZR_E_DEVICE, "refit: motion table beyond its buffer (internal error)");
    // 2. everything on the context's stream: patches and the changed ops up, scatter, the trees level by level, one read-back
    HIP_OK(hipEventRecord(st.ev0, q));
    const uint32_t n_rec = rec_no[nd];
    if (nd) HIP_OK(hipMemcpyAsync(st.d_box.p, st.h_box, nd * sizeof(zr::RefitBoxPatch), hipMemcpyHostToDevice, q));
    if (n_rec) HIP_OK(hipMemcpyAsync(st.d_rec.p, st.h_rec, n_rec * sizeof(zr::RefitRecPatch), hipMemcpyHostToDevice, q));
    if (payload_doubles) HIP_OK(hipMemcpyAsync(st.d_payload.p, st.h_payload, payload_doubles * sizeof(double), hipMemcpyHostToDevice, q));
    if (ix.op_hi > ix.op_lo) {   // the chains of wrapped objects, media and placed groups live here: patched as one range
        std::memcpy(st.h_ops, s->ops.data() + ix.op_lo, (ix.op_hi - ix.op_lo) * sizeof(zr_xform_op));
        HIP_OK(hipMemcpyAsync(s->d_ops.p + ix.op_lo, st.h_ops, (ix.op_hi - ix.op_lo) * sizeof(zr_xform_op), hipMemcpyHostToDevice, q));
    }
    HIP_OK(zr::refit_patch(q, device_view(s, st), st.d_box.p, (uint32_t)nd, st.d_rec.p, n_rec, st.d_payload.p));
    HIP_OK(zr::refit_motion(q, st.d_payload.p + st.motion_at + n_mrec, n_pairs, st.d_leaf_word.p, st.n_leaves));
    if ((rc = queue_trees(s, st))) return rc;
    HIP_OK(hipStreamSynchronize(q));   // the one synchronisation: the root is a kernel argument of every render
    double area = 0;
    if ((rc = take_result(s, st, area))) return rc;
    if (s->leaf_objects <= ZR_FUSED_OBJECTS && (rc = refresh_fused_objects(s))) return rc;   // (the fused kernel's arguments are copies; the stream is idle here)
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, st.ev0, st.ev1));
    info.epoch = s->epoch + 1;
    info.dirty_entries = (uint32_t)nd;
    info.levels = (uint32_t)st.q_levels.size();
    info.area_ratio = st.area0 > 0 ? area / st.area0 : 1.0;
    info.device_ms = ms;
    info.host_ms = (PhaseTimer::now() - t0) * 1e3;
    ix.clear_dirty();
    return ZR_OK;
}

}  // namespace

MotionView scene_motion_view(const zr_scene* s) {
    MotionView v;
    if (!s->refit || !s->refit->on_device) return v;
    const RefitState& st = *s->refit;
    v.leaf_word = st.d_leaf_word.p; v.records = st.d_payload.p + st.motion_at;
    std::memcpy(v.leaf_base, st.leaf_base, sizeof v.leaf_base);
    v.n_leaves = st.n_leaves; v.n_slots = (uint32_t)(st.motion.records.size() / kMotionDoubles);
    return v;
}

int scene_leaf_entries(zr_scene* s, const uint32_t** d_leaf_entry, MotionView* view) {
    if (int rc = update_ready(s, "zr_render_gbuffer_entries")) return rc;
    if (int rc = ensure_index(s)) return rc;
    RefitState& st = *s->refit;
    if (!st.d_leaf_entry.p) { HIP_OK(hipSetDevice(s->ctx->device)); if (int rc = st.d_leaf_entry.upload(st.leaf_entry)) return rc; }
    *d_leaf_entry = st.d_leaf_entry.p;
    std::memcpy(view->leaf_base, st.leaf_base, sizeof view->leaf_base);
    view->n_leaves = st.n_leaves;
    return ZR_OK;
}

extern "C" {

int zr_scene_motion(const zr_scene* s, uint32_t* out_slot_per_entry, double* out_records21, size_t capacity, size_t* out_count) {
    if (!s) return fail(ZR_E_INVALID, "null scene");
    if (!s->committed) return fail(ZR_E_STATE, "zr_scene_commit must precede zr_scene_motion");
    if (s->released) return fail(ZR_E_STATE, "zr_scene_motion: the scene was committed from borrowed arrays, which it has released: give it with zr_scene_set_all to move it");
    if (s->stale) return fail(ZR_E_STATE, "scene updated but not refitted: zr_scene_refit must precede zr_scene_motion");
    const size_t n = s->plan_objs.size();
    if (out_count) *out_count = n;
    if (!out_slot_per_entry && !out_records21) return ZR_OK;
    if (capacity < n) return fail(ZR_E_INVALID, "room for %zu world-list entries, the scene has %zu", capacity, n);
    const MotionTable* t = s->refit ? &s->refit->motion : nullptr;
    if (out_slot_per_entry) {
        std::fill(out_slot_per_entry, out_slot_per_entry + n, kMotionStatic);
        if (t) for (size_t k = 0; k < t->entries.size(); k++) out_slot_per_entry[t->entries[k]] = t->slot[k];
    }
    if (out_records21 && t && !t->records.empty()) std::memcpy(out_records21, t->records.data(), t->records.size() * sizeof(double));
    return ZR_OK;
}

int zr_scene_update_xform_ops(zr_scene* s, size_t first, const zr_xform_op* ops, size_t n) {
    if (int rc = update_ready(s, "zr_scene_update_xform_ops")) return rc;
    if (int rc = ensure_index(s)) return rc;
    UpdateWorld w = world_of(s);
    if (int rc = s->refit->ix.update_ops(w, first, ops, n)) return rc;
    if (n) s->stale = true;
    return ZR_OK;
}

int zr_scene_update_spheres(zr_scene* s, size_t first, const double* cxyz_r, size_t n) {
    if (int rc = update_ready(s, "zr_scene_update_spheres")) return rc;
    if (int rc = ensure_index(s)) return rc;
    UpdateWorld w = world_of(s);
    if (int rc = s->refit->ix.update_spheres(w, first, cxyz_r, n)) return rc;
    if (n) s->stale = true;
    return ZR_OK;
}

int zr_scene_refit(zr_scene* s, zr_refit_info* out) {
    if (int rc = update_ready(s, "zr_scene_refit")) return rc;
    zr_refit_info info{};
    if (int rc = refit(s, info)) {   // loud and safe: the device scene may be half rewritten, so nothing renders it until it is committed anew
        s->committed = false; s->stale = false;
        return rc;
    }
    s->epoch = info.epoch; s->stale = false;
    if (out) *out = info;
    return ZR_OK;
}

}  // extern "C"
