// zr_debug.hip — the BVH debug view (global_settings::bvh_debug_mode: bvh.hpp:46-110, aabb.hpp:44-84, camera.hpp:455-461, 928-953, 989-1004)
// for gfx950, on the device's own trees: the binary sibling-pair records (NodePair) the known-answer kernels walk.  The rule and the departures
// are in include/zr_capi.h and DESIGN §10; tests/bvh_debug_model.py restates it in NumPy.  Built without contraction (Makefile) so that the
// model can follow the box, edge and thickness arithmetic operation for operation.
//
// The walk reproduces the reference's recursion — a node's box test on the interval narrowed by the best hit so far, the edge test of a
// current-level node, then the left subtree and the right subtree — on an explicit stack: entering the left child at once and pushing the
// right one visits the nodes in the same order with the same narrowing.  A hit found below a current-level node takes its volume colour:
// for a level L >= 0 that node is the box of depth L visited last (a stack entry deeper than L descends from it), for level -1 the leaf
// itself.  A placed run of triangles is walked by a nested call with a stack of its own; its result is re-coloured by the outer tree's
// current-level ancestor when there is one (the outer override comes last).
#include "zr_device.h"
#include "zr_launch.h"

#define ZR_DBG_BLOCK 128

namespace zr {

namespace {

struct DHit {
    double t;
    uint32_t cls, box, tree, kind, idx;   // kind / idx: the primitive of a SURFACE hit (as closest_hit reports it)
    int depth;
    uint32_t anc; int anc_depth;         // current-level ancestor in the tree that recorded the hit (ZR_BVH_NO_BOX: none)
};

struct Box { double lo[3], hi[3]; };

// aabb::hit (aabb.hpp:44-66) on the interval [mn, mx]: false when it becomes empty
__device__ __forceinline__ bool box_hit(const Box& b, const Ray& r, double& mn, double& mx) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double invD = 1.0 / get(r.d, a);
        const double o = get(r.o, a);
        double t0 = (b.lo[a] - o) * invD;
        double t1 = (b.hi[a] - o) * invD;
        if (invD < 0.0) { const double x = t0; t0 = t1; t1 = x; }
        if (t0 > mn) mn = t0;
        if (t1 < mx) mx = t1;
        if (mx <= mn) return false;
    }
    return true;
}

// aabb::is_on_edge (aabb.hpp:68-84): within `th` of a plane on at least two axes
__device__ __forceinline__ bool on_edge(const Box& b, V3 p, double th) {
    int n = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double x = get(p, a);
        if (fabs(x - b.lo[a]) < th || fabs(x - b.hi[a]) < th) n++;
    }
    return n >= 2;
}

// diffuse_light colour of a frame (bvh.hpp:79-84) or a volume (bvh.hpp:97-100) at `depth`
__device__ __forceinline__ V3 debug_color(uint32_t cls, int depth) {
    const float g = fminf((float)depth * 0.15f, 1.0f);
    const V3 base = mk((double)0.4f, (double)g, (double)(1.0f - g));
    return cls == ZR_BVH_EDGE ? base * (double)4.0f : base * (double)0.1f;
}

__device__ __forceinline__ Box child_box(const NodePair& np, int s) {
    Box b;
    for (int a = 0; a < 3; a++) { b.lo[a] = (double)np.lo[s][a]; b.hi[a] = (double)np.hi[s][a]; }
    return b;
}
// a child slot with meta != 0 and no primitives is the empty second child of a one-leaf tree: no node at all
__device__ __forceinline__ bool slot_empty(uint32_t meta) { return meta != 0 && (meta & 0xFFFFu) == 0; }

// One tree's debug walk from its first record R on the interval (tmin, tbest]; returns whether anything was hit and leaves the resolved
// answer in `best`.  INNER: the tree of a placed run (leaves are triangles; the stack is private) — else the world's (LDS stack, two words
// per entry: box id, depth).
template <bool INNER>
__device__ bool dbg_walk(const DScene& sc, uint32_t R, const Ray& r, double tmin, double& tbest, int level, float thick, const Rng& g,
                         uint32_t* stk, int stride, DHit& best) {
    const NodePair& rp = sc.nodes[R];
    const bool e0 = slot_empty(rp.meta[0]), e1 = slot_empty(rp.meta[1]);
    if (e0 && e1) return false;
    bool found = false;
    uint32_t lvl = ZR_BVH_NO_BOX;   // the box of depth `level` visited last
    int sp = 0;
    // the current node: its box id, depth, and either its children's record (inner) or its range (leaf)
    uint32_t id = ZR_BVH_ROOT_BOX | R;
    int depth = 0;
    Box box;
    for (int a = 0; a < 3; a++) {
        const float lo = e0 ? rp.lo[1][a] : (e1 ? rp.lo[0][a] : fminf(rp.lo[0][a], rp.lo[1][a]));
        const float hi = e0 ? rp.hi[1][a] : (e1 ? rp.hi[0][a] : fmaxf(rp.hi[0][a], rp.hi[1][a]));
        box.lo[a] = (double)lo; box.hi[a] = (double)hi;
    }
    bool leaf = false;
    uint32_t child = R, meta = 0;
    for (;;) {
        bool descend = false;
        double mn = tmin, mx = tbest;
        if (box_hit(box, r, mn, mx)) {
            const bool cur = level < 0 ? leaf : depth == level;
            bool edge = false;
            if (cur) {
                const float th = (float)((double)thick * ((double)0.05f + mn * (double)0.1f));
                const V3 p_in = at(r, mn + (double)0.0001f), p_out = at(r, mx - (double)0.0001f);
                double te = 0;
                if (on_edge(box, p_in, (double)th)) { te = mn; edge = true; }
                else if (on_edge(box, p_out, (double)th)) { te = mx; edge = true; }
                if (edge) {
                    tbest = te; found = true;
                    best.t = te; best.cls = ZR_BVH_EDGE; best.box = id; best.tree = R; best.depth = depth; best.anc = ZR_BVH_NO_BOX; best.anc_depth = -1;
                }
            }
            if (!edge) {
                if (level >= 0 && depth == level) lvl = id;
                const uint32_t anc = level < 0 ? (leaf ? id : ZR_BVH_NO_BOX) : (depth >= level ? lvl : ZR_BVH_NO_BOX);
                const int anc_depth = level < 0 ? depth : level;
                if (leaf) {
                    const uint32_t kind = (meta >> 16) - 1, cnt = meta & 0xFFFFu;
                    for (uint32_t k = 0; k < cnt; k++) {
                        double t;
                        bool placed = false;
                        if constexpr (!INNER) placed = kind == ZR_KIND_INSTANCE;
                        if (placed) {
                          if constexpr (!INNER) {
                            const DInstance in = sc.insts[child + k];
                            const Ray lr = chain_ray(sc, in.chain_first, in.chain_count, r);
                            uint32_t istk[2 * ZR_STACK_DEPTH];
                            DHit ih;
                            double tb = tbest;
                            if (dbg_walk<true>(sc, in.root, lr, tmin, tb, level, thick, g, istk, 1, ih)) {
                                tbest = tb; found = true;
                                best = ih;
                                if (ih.cls == ZR_BVH_SURFACE) best.kind = ZR_KIND_INSTANCE | ((child + k) << 8);
                                best.anc = anc; best.anc_depth = anc_depth;
                            }
                          }
                        } else {
                            const bool h = INNER ? triangle_t(sc.tri_v + (size_t)(child + k) * ZR_TRI_STRIDE, r, tmin, tbest, t)
                                                 : object_t(sc, kind, child + k, r, tmin, tbest, g, t);
                            if (h) {
                                tbest = t; found = true;
                                best.t = t; best.cls = ZR_BVH_SURFACE; best.box = id; best.tree = R; best.depth = depth;
                                best.kind = INNER ? ZR_PRIM_TRIANGLE : kind; best.idx = child + k; best.anc = anc; best.anc_depth = anc_depth;
                            }
                        }
                    }
                } else {
                    descend = true;
                }
            }
        }
        if (descend) {
            // left child now, right child later (with the interval the left subtree leaves)
            const NodePair& np = sc.nodes[child];
            const int d1 = depth + 1;
            if (!slot_empty(np.meta[1]) && sp < ZR_STACK_DEPTH) { stk[(2 * sp) * stride] = 2 * child + 1; stk[(2 * sp + 1) * stride] = (uint32_t)d1; sp++; }
            if (!slot_empty(np.meta[0])) {
                id = 2 * child; depth = d1; box = child_box(np, 0); leaf = np.meta[0] != 0; meta = np.meta[0]; child = np.child[0];
                continue;
            }
        }
        if (sp == 0) break;
        sp--;
        id = stk[(2 * sp) * stride]; depth = (int)stk[(2 * sp + 1) * stride];
        const uint32_t rec = id >> 1, s = id & 1u;
        const NodePair& np = sc.nodes[rec];
        box = child_box(np, (int)s); leaf = np.meta[s] != 0; meta = np.meta[s]; child = np.child[s];
    }
    if (found && best.anc != ZR_BVH_NO_BOX) {   // bvh.hpp:94-100: the volume colour of the current-level node above the hit
        best.cls = ZR_BVH_VOLUME; best.box = best.anc; best.depth = best.anc_depth; best.tree = R;
    }
    if (found) best.anc = ZR_BVH_NO_BOX;
    return found;
}

__device__ __forceinline__ bool world_walk(const DScene& sc, const Ray& r, double tmin, int level, float thick, const Rng& g, uint32_t* stk, DHit& h) {
    double tb = __builtin_huge_val();
    return dbg_walk<false>(sc, 0, r, tmin, tb, level, thick, g, stk, ZR_DBG_BLOCK, h);
}

// what a debug hit emits: the frame / volume colour, or the surface's emitted()
template <bool UV>
__device__ __forceinline__ V3 hit_emission(const DScene& sc, const Ray& r, const DHit& h) {
    if (h.cls != ZR_BVH_SURFACE) return debug_color(h.cls, h.depth);
    Rec rec;
    object_rec<true, UV>(sc, h.kind, h.idx, r, h.t, rec);
    return emitted(sc, rec);
}

// one primary sample of the debug view: camera.hpp:455-461, 519-520 with ray_color_from_hit (989-1004) and ray_color's debug branch (928-953)
template <bool UV>
__device__ V3 debug_sample(const DScene& sc, const DCamera& cam, const DEnv& env, int px, int py, int level, float thick, Rng& g, uint32_t* stk) {
    const Ray r = camera_ray(cam, px, py, g);
    DHit h;
    const bool hit = world_walk(sc, r, 0.001, level, thick, g, stk, h);
    g.bounce++;
    if (!hit) return background(sc, env, r.d);
    if (h.cls != ZR_BVH_SURFACE) return debug_color(h.cls, h.depth);   // diffuse_light: emits, does not scatter
    Rec rec;
    object_rec<true, UV>(sc, h.kind, h.idx, r, h.t, rec);
    const V3 L0 = emitted(sc, rec);
    V3 att; Ray sr;
    if (!scatter(sc, r, rec, att, sr, g)) return L0;
    V3 c = mk(0, 0, 0);
    if (cam.max_depth - 1 > 0) {
        DHit h2;
        if (world_walk(sc, sr, 0.001, level, thick, g, stk, h2)) {
            const V3 e = hit_emission<UV>(sc, sr, h2);
            c = len(e) > 0.1 ? e : mk(0.01, 0.01, 0.01);
        }
        g.bounce++;
    }
    return L0 + att * c;
}

// UV: the build for scenes whose triangles carry texture coordinates (zr_device.h: triangle_rec_uv)
template <bool UV>
__global__ __launch_bounds__(ZR_DBG_BLOCK) void bvh_debug_pixels(DScene sc, DCamera cam, DEnv env, uint64_t seed, WorkDesc wd, int level, float thick,
                                                                  double* __restrict__ out) {
    __shared__ uint32_t lds_stack[2 * ZR_STACK_DEPTH * ZR_DBG_BLOCK];
    uint32_t* stk = lds_stack + threadIdx.x;
    const long long q = (long long)blockIdx.x * ZR_DBG_BLOCK + threadIdx.x;   // one lane per pixel
    const int tpix = wd.tile_size * wd.tile_size;
    if (q >= (long long)wd.n_tiles * tpix) return;
    const int tile = wd.tiles[q / tpix];
    const int local = (int)(q % tpix);
    const int px = (tile % wd.tiles_x) * wd.tile_size + local % wd.tile_size;
    const int py = (tile / wd.tiles_x) * wd.tile_size + local / wd.tile_size;
    if (px < wd.x0 || px >= wd.x1 || py < wd.y0 || py >= wd.y1) return;
    const uint64_t pixel = (uint64_t)py * (uint64_t)cam.W + (uint64_t)px;
    V3 sum = mk(0, 0, 0);
    for (int s = 0; s < cam.spp; s++) {
        Rng g; g.key = zr_stream_key(seed, pixel, (uint64_t)s); g.k = 0; g.bounce = 0;
        sum = sum + debug_sample<UV>(sc, cam, env, px, py, level, thick, g, stk);
    }
    const double scale = 1.0 / cam.spp;   // camera.hpp:437,531
    double* o = out + (size_t)pixel * 3;
    o[0] = sum.x * scale; o[1] = sum.y * scale; o[2] = sum.z * scale;
}

// UV: the build for scenes whose triangles carry texture coordinates (zr_device.h: triangle_rec_uv)
template <bool UV>
__global__ __launch_bounds__(ZR_DBG_BLOCK) void bvh_debug_trace(DScene sc, const double* __restrict__ rays, size_t n, double tmin, uint64_t seed, uint64_t pixel,
                                                                 uint32_t bounce, int level, float thick, zr_bvh_debug_hit* __restrict__ out) {
    __shared__ uint32_t lds_stack[2 * ZR_STACK_DEPTH * ZR_DBG_BLOCK];
    const size_t k = (size_t)blockIdx.x * ZR_DBG_BLOCK + threadIdx.x;
    if (k >= n) return;
    Ray r; r.o = ld3(rays + k * 6); r.d = ld3(rays + k * 6 + 3);
    Rng g; g.key = zr_stream_key(seed, pixel, k); g.k = 0; g.bounce = bounce;
    DHit h;
    zr_bvh_debug_hit o;
    for (int c = 0; c < 3; c++) { o.hit.p[c] = 0; o.hit.normal[c] = 0; o.hit.tangent[c] = 0; o.hit.bitangent[c] = 0; o.color[c] = 0; }
    o.hit.t = 0; o.hit.u = 0; o.hit.v = 0; o.hit.mat = 0xFFFFFFFFu; o.hit.front_face = 0;
    o.cls = ZR_BVH_MISS; o.depth = -1; o.tree = ZR_BVH_NO_BOX; o.box = ZR_BVH_NO_BOX;
    if (world_walk(sc, r, tmin, level, thick, g, lds_stack + threadIdx.x, h)) {
        o.cls = h.cls; o.depth = h.depth; o.tree = h.tree; o.box = h.box;
        V3 e;
        if (h.cls == ZR_BVH_SURFACE) {
            Rec rec;
            object_rec<true, UV>(sc, h.kind, h.idx, r, h.t, rec, true);
            o.hit.p[0] = rec.p.x; o.hit.p[1] = rec.p.y; o.hit.p[2] = rec.p.z;
            o.hit.normal[0] = rec.n.x; o.hit.normal[1] = rec.n.y; o.hit.normal[2] = rec.n.z;
            o.hit.tangent[0] = rec.tan.x; o.hit.tangent[1] = rec.tan.y; o.hit.tangent[2] = rec.tan.z;
            o.hit.bitangent[0] = rec.bit.x; o.hit.bitangent[1] = rec.bit.y; o.hit.bitangent[2] = rec.bit.z;
            o.hit.t = rec.t; o.hit.u = rec.u; o.hit.v = rec.v; o.hit.mat = rec.mat; o.hit.front_face = rec.front ? 1u : 0u;
            e = emitted(sc, rec);
        } else {
            const V3 p = at(r, h.t);
            o.hit.p[0] = p.x; o.hit.p[1] = p.y; o.hit.p[2] = p.z; o.hit.normal[2] = 1.0; o.hit.t = h.t;
            e = debug_color(h.cls, h.depth);
        }
        o.color[0] = e.x; o.color[1] = e.y; o.color[2] = e.z;
    }
    out[k] = o;
}

}  // namespace

hipError_t launch_bvh_debug(const DScene& sc, const DCamera& cam, const DEnv& env, uint64_t seed, const WorkDesc& wd, int level, float thickness, double* out,
                            hipStream_t stream) {
    const long long pixels = (long long)wd.n_tiles * wd.tile_size * wd.tile_size;
    const long long blocks = (pixels + ZR_DBG_BLOCK - 1) / ZR_DBG_BLOCK;
    if (blocks <= 0) return hipSuccess;
    if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    if (sc.tri_uv_at) hipLaunchKernelGGL(bvh_debug_pixels<true>, dim3((unsigned)blocks), dim3(ZR_DBG_BLOCK), 0, stream, sc, cam, env, seed, wd, level, thickness, out);
    else hipLaunchKernelGGL(bvh_debug_pixels<false>, dim3((unsigned)blocks), dim3(ZR_DBG_BLOCK), 0, stream, sc, cam, env, seed, wd, level, thickness, out);
    return hipGetLastError();
}

hipError_t launch_trace_bvh_debug(const DScene& sc, const double* rays, size_t n, double tmin, uint64_t seed, uint64_t pixel, uint32_t bounce, int level,
                                  float thickness, zr_bvh_debug_hit* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (sc.tri_uv_at) hipLaunchKernelGGL(bvh_debug_trace<true>, dim3((unsigned)((n + ZR_DBG_BLOCK - 1) / ZR_DBG_BLOCK)), dim3(ZR_DBG_BLOCK), 0, stream, sc, rays, n, tmin, seed, pixel,
                       bounce, level, thickness, out);
    else hipLaunchKernelGGL(bvh_debug_trace<false>, dim3((unsigned)((n + ZR_DBG_BLOCK - 1) / ZR_DBG_BLOCK)), dim3(ZR_DBG_BLOCK), 0, stream, sc, rays, n, tmin, seed, pixel,
                       bounce, level, thickness, out);
    return hipGetLastError();
}

}  // namespace zr
