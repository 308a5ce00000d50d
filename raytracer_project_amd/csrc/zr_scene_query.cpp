// zr_scene_query.cpp — what a committed scene answers (include/zr_capi.h): statistics, the kernel builds it renders through, the traversal stack it
// needs, the builder that made its tree, and the boxes of its trees read back from the device (zr_scene_tree_boxes).
#include "zr_host_internal.h"

extern "C" {

int zr_scene_stats(const zr_scene* s, uint64_t out[4]) {
    if (!s || !s->committed) return fail(ZR_E_STATE, "scene not committed");
    std::memcpy(out, s->stats, sizeof s->stats);
    return ZR_OK;
}

int zr_scene_kernels(const zr_scene* s, uint32_t out[4]) {
    if (!s || !out) return fail(ZR_E_INVALID, "null argument");
    if (!s->committed) return fail(ZR_E_STATE, "scene not committed");
    out[0] = (uint32_t)s->leaf_level; out[1] = s->ds.shade_lean; out[2] = s->fused_ok ? 1u : 0u; out[3] = (uint32_t)s->leaf_objects;
    return ZR_OK;
}

int zr_scene_tree_boxes(const zr_scene* s, zr_tree_box* out, size_t cap) {
    if (!s) return fail(ZR_E_INVALID, "null scene");
    if (!s->committed) return fail(ZR_E_STATE, "scene not committed");
    if (s->stale) return fail(ZR_E_STATE, "scene updated but not refitted: zr_scene_refit must precede zr_scene_tree_boxes");
    if (cap && !out) return fail(ZR_E_INVALID, "null output array");
    HIP_OK(hipSetDevice(s->device));
    const size_t n_pairs = s->d_nodes.n;
    std::vector<zr::NodePair> pairs(n_pairs);
    std::vector<zr::DInstance> insts(s->d_insts.n);
    if (n_pairs) HIP_OK(hipMemcpy(pairs.data(), s->d_nodes.p, n_pairs * sizeof(zr::NodePair), hipMemcpyDeviceToHost));
    if (!insts.empty()) HIP_OK(hipMemcpy(insts.data(), s->d_insts.p, insts.size() * sizeof(zr::DInstance), hipMemcpyDeviceToHost));
    auto empty = [](uint32_t meta) { return meta != 0 && (meta & 0xFFFFu) == 0; };
    std::vector<zr_tree_box> boxes;
    // one tree from its first record R, in pre-order (the order the debug walk meets its boxes)
    auto walk = [&](uint32_t R) -> int {
        if (R >= n_pairs) return fail(ZR_E_DEVICE, "tree root %u outside the %zu pair records (internal error)", R, n_pairs);
        const zr::NodePair& rp = pairs[R];
        const bool e0 = empty(rp.meta[0]), e1 = empty(rp.meta[1]);
        if (e0 && e1) return ZR_OK;
        zr_tree_box root{};
        for (int a = 0; a < 3; a++) {
            root.lo[a] = e0 ? rp.lo[1][a] : (e1 ? rp.lo[0][a] : std::fmin(rp.lo[0][a], rp.lo[1][a]));
            root.hi[a] = e0 ? rp.hi[1][a] : (e1 ? rp.hi[0][a] : std::fmax(rp.hi[0][a], rp.hi[1][a]));
        }
        root.id = ZR_BVH_ROOT_BOX | R; root.tree = R; root.parent = ZR_BVH_NO_BOX; root.depth = 0; root.first = R; root.subtree = ZR_BVH_NO_BOX;
        boxes.push_back(root);
        struct E { uint32_t id; int depth; uint32_t parent; };   // a child box: id = 2 * record + slot
        std::vector<E> st;
        auto push_children = [&](uint32_t rec, int depth, uint32_t parent) {   // right first: the left subtree is emitted first
            for (int s2 = 1; s2 >= 0; s2--) if (!empty(pairs[rec].meta[s2])) st.push_back({2 * rec + (uint32_t)s2, depth, parent});
        };
        push_children(R, 1, root.id);
        while (!st.empty()) {
            const E e = st.back(); st.pop_back();
            if (e.depth > ZR_STACK_DEPTH + 2) return fail(ZR_E_DEVICE, "tree %u deeper than the traversal stack (internal error)", R);
            const uint32_t rec = e.id >> 1, s2 = e.id & 1u;
            const zr::NodePair& np = pairs[rec];
            zr_tree_box b{};
            for (int a = 0; a < 3; a++) { b.lo[a] = np.lo[s2][a]; b.hi[a] = np.hi[s2][a]; }
            b.id = e.id; b.tree = R; b.parent = e.parent; b.depth = e.depth; b.slot = s2; b.subtree = ZR_BVH_NO_BOX; b.first = np.child[s2];
            for (int k = 0; k < 4; k++) b.src[k] = ZR_BVH_NO_BOX;
            if (np.meta[s2] != 0) {
                b.leaf = 1; b.kind = (np.meta[s2] >> 16) - 1; b.count = np.meta[s2] & 0xFFFFu;
                const std::vector<uint32_t>& src = s->leaf_src[b.kind & 7];
                for (uint32_t k = 0; k < b.count && k < 4; k++) if ((size_t)b.first + k < src.size()) b.src[k] = src[b.first + k];
                if (b.kind == ZR_KIND_INSTANCE && b.first < insts.size()) b.subtree = insts[b.first].root;
            }
            boxes.push_back(b);
            if (np.meta[s2] == 0) {
                if (b.first >= n_pairs) return fail(ZR_E_DEVICE, "child record %u outside the %zu pair records (internal error)", b.first, n_pairs);
                push_children(b.first, e.depth + 1, b.id);
            }
        }
        return ZR_OK;
    };
    int rc = walk(0);
    if (rc) return rc;
    std::vector<uint32_t> roots;
    for (const zr::DInstance& in : insts) roots.push_back(in.root);
    std::sort(roots.begin(), roots.end());
    roots.erase(std::unique(roots.begin(), roots.end()), roots.end());
    for (uint32_t R : roots) if ((rc = walk(R))) return rc;
    const size_t n = std::min(cap, boxes.size());
    if (n) std::memcpy(out, boxes.data(), n * sizeof(zr_tree_box));
    return (int)std::min<size_t>(boxes.size(), 0x7FFFFFFF);
}

uint32_t zr_scene_traversal_stack(const zr_scene* s) { return s && s->committed ? s->stack_demand : 0u; }
const char* zr_scene_builder(const zr_scene* s) { return s && s->committed ? s->builder : ""; }

}  // extern "C"
